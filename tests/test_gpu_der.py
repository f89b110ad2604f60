"""GPU: the diarisation error rate (csrc/der.hip) against its host model (tests/der_model.py).  The contract is exact, so
every comparison of counts and cluster numbers is ==; the map, which is not canonical among equal-weight optima, is checked
for its properties (der_model.check_map).

Every device call of this file goes through _run / _run_sweep: the inputs sit between -1 / NaN neighbours and every output
between guard bands filled with a payload that must stay intact outside the output and be gone inside it."""
import ctypes as C

import numpy as np
import pytest

import der_model as M

pytestmark = pytest.mark.gpu

GUARD = 4 << 10            # elements on either side
PAYLOAD = 0x7FC0DEAD
E_INVAL = -1


def _dev():
    import torch
    return torch.device("cuda", 0)


def _guarded_input(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.empty(GUARD + t.numel() + GUARD, dtype=t.dtype, device=_dev())
    buf.fill_(float("nan") if t.dtype.is_floating_point else -1)
    body = buf[GUARD:GUARD + t.numel()]
    body.copy_(t.to(_dev()))
    return buf, body


class _Out:
    """a 1-D output of `count` elements between guard bands, everything pre-filled with the payload"""

    def __init__(self, count, dtype):
        import torch
        self.count = count
        self.words_per = torch.empty(0, dtype=dtype).element_size() // 4
        n = (GUARD + count + GUARD) * self.words_per
        self.words = torch.full((n,), PAYLOAD, dtype=torch.int32, device=_dev())
        self.body = self.words.view(dtype)[GUARD:GUARD + count]

    def ptr(self):
        return self.body.data_ptr() if self.count else self.words.view(self.body.dtype)[GUARD:].data_ptr()

    def check(self, what, written=True):
        w = self.words.cpu().numpy().reshape(-1, self.words_per)
        lo, hi = GUARD, GUARD + self.count
        assert (w[:lo] == np.int32(PAYLOAD)).all() and (w[hi:] == np.int32(PAYLOAD)).all(), "%s: guard band overwritten" % what
        left = int((w[lo:hi] == np.int32(PAYLOAD)).all(1).sum())
        if written:
            assert left == 0, "%s: %d output elements never written" % (what, left)
        else:
            assert left == self.count, "%s: %d output elements written by a failing call" % (what, self.count - left)
        return self.body.cpu().numpy().copy()


def _lib():
    from plda_amd import _native as N
    return N.load()


def _vp(x):
    return C.c_void_p(int(x)) if x else None


def _hp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _run(eng, ref, hyp, offsets, dur=None, want_map=True, expect=0):
    """plda_der_dev on guarded buffers -> (counts int64 [R, 4], map int32 [R, 64] or None), or the status when expect != 0"""
    import torch
    offsets = np.ascontiguousarray(offsets, np.int64)
    r = len(offsets) - 1
    keep = [_guarded_input(np.asarray(a, np.int32)) for a in (ref, hyp)] + ([_guarded_input(np.asarray(dur, np.int32))] if dur is not None else [])
    oC, oM = _Out(max(r, 0) * 4, torch.int64), _Out(max(r, 0) * M.MAX_REF, torch.int32)
    torch.cuda.synchronize()
    rc = _lib().plda_der_dev(eng._h, _vp(keep[0][1].data_ptr()), _vp(keep[1][1].data_ptr()), _vp(keep[2][1].data_ptr()) if dur is not None else None,
                             _hp(offsets), r, _vp(oC.ptr()), _vp(oM.ptr()) if want_map else None)
    torch.cuda.synchronize()
    assert rc == expect, "status %d: %s" % (rc, eng._lib.plda_last_error(eng._h).decode())
    if expect:
        oC.check("counts", written=False)
        oM.check("map", written=False)
        return rc
    counts = oC.check("counts").reshape(r, 4)
    if want_map:
        return counts, oM.check("map").reshape(r, M.MAX_REF)
    oM.check("map", written=False)
    return counts, None


def _run_sweep(eng, merges, offsets, ref, thresholds, dur=None, num_speakers=None, expect=0):
    """plda_der_sweep_dev on guarded buffers -> (counts int64 [Q, R, 4], n_clusters int32 [Q, R])"""
    import torch
    from plda_amd import diarize
    offsets = np.ascontiguousarray(offsets, np.int64)
    thresholds = np.ascontiguousarray(thresholds, np.float64)
    r, q = len(offsets) - 1, len(thresholds)
    minc = diarize.stop_args(offsets, 0.0, num_speakers)[2]
    ma, mb, mc = merges
    keep = [_guarded_input(np.asarray(ma, np.int32)), _guarded_input(np.asarray(mb, np.int32)), _guarded_input(np.asarray(mc, np.float64)),
            _guarded_input(np.asarray(ref, np.int32))] + ([_guarded_input(np.asarray(dur, np.int32))] if dur is not None else [])
    oC, oK = _Out(q * r * 4, torch.int64), _Out(q * r, torch.int32)
    torch.cuda.synchronize()
    rc = _lib().plda_der_sweep_dev(eng._h, *[_vp(k[1].data_ptr()) for k in keep[:3]], _hp(offsets), r, _vp(keep[3][1].data_ptr()),
                                   _vp(keep[4][1].data_ptr()) if dur is not None else None, _hp(thresholds), q, _hp(minc), _vp(oC.ptr()),
                                   _vp(oK.ptr()))
    torch.cuda.synchronize()
    assert rc == expect, "status %d: %s" % (rc, eng._lib.plda_last_error(eng._h).decode())
    if expect:
        oC.check("counts", written=False)
        oK.check("n_clusters", written=False)
        return rc
    return oC.check("counts").reshape(q, r, 4), oK.check("n_clusters").reshape(q, r)


def _check(eng, recs, what, want_map=True):
    """recs: [(ref, hyp, dur or None)] with dur given for all or none -> the device counts, after comparing with the model"""
    from plda_amd import diarize
    offsets = diarize.offsets_of([len(x[0]) for x in recs])
    ref, hyp = np.concatenate([x[0] for x in recs]), np.concatenate([x[1] for x in recs])
    dur = None if recs[0][2] is None else np.concatenate([x[2] for x in recs])
    counts, mp = _run(eng, ref, hyp, offsets, dur, want_map)
    want = M.score(ref, hyp, offsets, dur)
    assert np.array_equal(counts, want), "%s: counts\n%r\nmodel\n%r" % (what, counts[:8], want[:8])
    if want_map:
        for q, (a, b, d) in enumerate(recs):
            M.check_map(mp[q], a, b, d)
    return counts, mp


@pytest.fixture(scope="module")
def eng():
    from plda_amd import MPlda
    return MPlda(0)


# ------------------------------------------------------------------------------------------- counts against the model
@pytest.mark.parametrize("shape", [(1, 1), (5, 2), (2, 5), (64, 64), (64, 1), (1, 300)])
def test_counts_equal_the_model_at_the_shapes(eng, shape):
    sr, sh = shape
    rng = np.random.default_rng(100 * sr + sh)
    n = max(sr, sh) + 37
    ref, hyp, dur = M.exact_shape(rng, n, sr, sh)
    assert len(set(ref.tolist())) == sr and len(set(hyp.tolist())) == sh
    _check(eng, [(ref, hyp, dur)], "shape %r" % (shape,))
    ref2, hyp2 = ref.copy(), hyp.copy()                      # the same with non-speech on either side
    ref2[::7] = -1
    hyp2[3::5] = -1
    _check(eng, [(ref2, hyp2, dur)], "shape %r with non-speech" % (shape,))


def test_edge_recordings(eng):
    i32 = lambda *v: np.asarray(v, np.int32)
    rng = np.random.default_rng(3)
    recs = [(i32(3), i32(7), i32(5)),                                                    # N = 1
            (i32(-1), i32(7), i32(5)), (i32(3), i32(-1), i32(5)), (i32(-1), i32(-1), i32(5)),
            (i32(-1, -1, -1, -1), i32(0, 1, -1, 1), i32(2, 3, 4, 5)),                    # ref all -1: speech = 0
            (i32(0, 1, 2, 1), i32(-1, -1, -1, -1), i32(2, 3, 4, 5)),                     # hyp all -1
            (i32(-1, 0, -1, 5, 5), i32(-1, -1, 2, 2, -1), i32(1, 2, 3, 4, 5)),           # -1 on both sides
            (i32(63, 7, 63, 40, 7, 63), i32(4095, 4095, 100, 64, 63, 0), i32(1, 2, 3, 4, 5, 6))]   # label values with gaps
    recs.append(M.random_case(rng, 50, 4, 6, gap=9))
    recs.append(M.random_case(rng, 50, 6, 4, gap=12, max_dur=1))                         # dur holding many zeros
    counts, _ = _check(eng, recs, "edges")
    assert counts[4].tolist() == [0, 0, 10, 0] and counts[3].tolist() == [0, 0, 0, 0]
    assert counts[0].tolist() == [5, 0, 0, 0] and counts[7, 0] == 21


def test_null_dur_equals_explicit_ones(eng):
    from plda_amd import diarize
    rng = np.random.default_rng(4)
    recs = [M.random_case(rng, n, sr, sh)[:2] for n, sr, sh in ((1, 1, 1), (30, 3, 5), (300, 10, 40), (77, 64, 64))]
    offsets = diarize.offsets_of([len(a) for a, _ in recs])
    ref, hyp = np.concatenate([a for a, _ in recs]), np.concatenate([b for _, b in recs])
    c_null, m_null = _run(eng, ref, hyp, offsets, None)
    c_ones, m_ones = _run(eng, ref, hyp, offsets, np.ones(len(ref), np.int32))
    assert np.array_equal(c_null, c_ones) and np.array_equal(m_null, m_ones)
    assert np.array_equal(c_null, M.score(ref, hyp, offsets))
    zero = np.zeros(len(ref), np.int32)
    c_zero, m_zero = _run(eng, ref, hyp, offsets, zero)
    assert (c_zero == 0).all() and (m_zero == -1).all()


def test_sums_beyond_32_and_40_bits(eng):
    """dur = 2^31 - 1 on 4096 segments: speech = 4096 (2^31 - 1) > 2^42, cells of the matrix beyond 2^40"""
    rng = np.random.default_rng(5)
    n = 4096
    ref = rng.integers(0, 3, n).astype(np.int32)
    hyp = ((ref + (rng.random(n) < 0.2)) % 3).astype(np.int32)
    ref[:40], hyp[40:90] = -1, -1
    dur = np.full(n, 2 ** 31 - 1, np.int32)
    counts, _ = _check(eng, [(ref, hyp, dur)], "large durations")
    assert counts[0, 0] == int((ref >= 0).sum()) * (2 ** 31 - 1) > 2 ** 42
    C = M.confusion(ref, hyp, dur)[0]
    assert max(int(v) for v in C.ravel()) > 2 ** 40


@pytest.mark.parametrize("shape", [(4, 4, 40), (8, 8, 64), (6, 9, 54), (64, 64, 640), (16, 200, 1600)])
def test_tie_heavy_matrices(eng, shape):
    """all durations equal, uniform random labels: many cells hold the same count"""
    sr, sh, n = shape
    rng = np.random.default_rng(n)
    recs = []
    for _ in range(4):
        recs.append((rng.integers(0, sr, n).astype(np.int32), rng.integers(0, sh, n).astype(np.int32), np.full(n, 3, np.int32)))
    _check(eng, recs, "ties %r" % (shape,))


def test_a_greedy_map_fails(eng):
    """[[10, 9], [9, 0]]: the largest cell first gives 10, the optimum 18; the 6 x 6 family built the same way"""
    a, b, d = M.from_matrix(M.greedy_trap(1))
    counts, mp = _check(eng, [(a, b, d)], "2 x 2 trap")
    assert counts[0].tolist() == [28, 0, 0, 10] and mp[0, :2].tolist() == [1, 0]
    recs = [M.from_matrix(M.greedy_trap(3), seed=1), M.from_matrix(M.greedy_trap(3), seed=2, unit=1),
            M.from_matrix(M.greedy_trap(3).T[::-1], seed=3), M.from_matrix(M.greedy_trap(3)[:, ::-1] * 1000, seed=4)]
    counts, _ = _check(eng, recs, "6 x 6 traps")
    assert counts[0].tolist() == [28 * 6, 0, 0, 10 * 6] and counts[1].tolist() == counts[0].tolist()


# ------------------------------------------------------------------------------------------- classes, launches, batches
def _boundary(eng, sr):
    from plda_amd import der
    return der.plan(eng, sr, 1)["lds_max"]


def test_plan_names_the_classes(eng):
    from plda_amd import der
    w64 = _boundary(eng, 64)
    assert 64 < w64 < 4096
    assert der.plan(eng, 64, w64) == {"cls": 0, "scratch_bytes": 0, "lds_max": w64}
    assert der.plan(eng, 64, w64 + 1) == {"cls": 1, "scratch_bytes": 8 * 64 * (w64 + 1), "lds_max": w64}
    assert der.plan(eng, 64, 4096)["scratch_bytes"] == 2 << 20
    assert der.plan(eng, 1, 300)["cls"] == 0 and der.plan(eng, 0, 0)["cls"] == 0
    assert der.plan(eng, 1, 4096) == {"cls": 1, "scratch_bytes": 8 * 4096, "lds_max": _boundary(eng, 1)}     # (the column state alone is 128 KiB)
    w20 = _boundary(eng, 20)
    assert w64 < w20 < 4096 and der.plan(eng, 20, w20 + 1)["cls"] == 1
    out = (C.c_int32 * 3)()
    assert _lib().plda_der_plan(eng._h, 65, 1, out) == E_INVAL and _lib().plda_der_plan(eng._h, 1, 4097, out) == E_INVAL
    assert _lib().plda_der_plan(eng._h, -1, 1, out) == E_INVAL


@pytest.mark.parametrize("sr", [64, 20])
def test_both_classes_at_the_boundary(eng, sr):
    """the largest shape of the LDS class and the first of the scratch class, from plda_der_plan"""
    w = _boundary(eng, sr)
    rng = np.random.default_rng(sr)
    recs = [M.exact_shape(rng, sh + 50, sr, sh) for sh in (w - 1, w, w + 1, w + 2)]
    _check(eng, recs, "boundary sr = %d" % sr)


def test_64_by_4096(eng):
    """every segment its own hypothesis speaker: the largest matrix, the scratch class"""
    rng = np.random.default_rng(6)
    n = 4096
    ref = np.concatenate([np.arange(64), rng.integers(0, 64, n - 64)]).astype(np.int32)
    rng.shuffle(ref)
    hyp = rng.permutation(n).astype(np.int32)
    dur = rng.integers(1, 1000, n).astype(np.int32)
    counts, mp = _check(eng, [(ref, hyp, dur)], "64 x 4096")
    # the optimum keeps the longest segment of every reference speaker
    keep = sum(int(dur[ref == s].max()) for s in range(64))
    assert counts[0].tolist() == [int(dur.sum()), 0, 0, int(dur.sum()) - keep]
    assert (mp[0] >= 0).all()


def _mixed_recordings(eng, count, seed):
    """recordings of mixed sizes and of both classes"""
    w = _boundary(eng, 64)
    rng = np.random.default_rng(seed)
    recs = []
    for q in range(count):
        kind = q % 7
        if kind == 0:
            recs.append(M.exact_shape(rng, w + 60 + q, 64, w + 1 + q % 5))                 # scratch class
        elif kind == 1:
            recs.append(M.exact_shape(rng, 900, 30, 700 + q))                              # scratch class, fewer rows
        elif kind == 2:
            recs.append(M.random_case(rng, 1 + q % 3, 2, 2))
        elif kind == 3:
            n = 200
            recs.append((rng.integers(0, 8, n).astype(np.int32), rng.integers(0, 8, n).astype(np.int32), np.full(n, 2, np.int32)))   # ties
        else:
            recs.append(M.random_case(rng, int(rng.integers(5, 400)), int(rng.integers(1, 20)), int(rng.integers(1, 60)), gap=1 + q % 4))
    return recs


def test_several_launches_equal_one(monkeypatch, eng):
    """a scratch budget of 1 MiB holds one or two scratch-class matrices: the results equal those of the default budget"""
    from plda_amd import MPlda
    recs = _mixed_recordings(eng, 28, 7)
    monkeypatch.setenv("PLDA_DER_SCRATCH_BYTES", str(1 << 20))
    small = MPlda(0)
    monkeypatch.delenv("PLDA_DER_SCRATCH_BYTES")
    held = _lib().plda_device_bytes_held()
    c_small, m_small = _check(small, recs, "several launches")
    assert _lib().plda_device_bytes_held() - held < (3 << 20)        # (the budget's scratch, not the call's 1.3 MB of matrices)
    c_one, m_one = _check(eng, recs, "one launch")
    assert np.array_equal(c_small, c_one) and np.array_equal(m_small, m_one)


def test_a_recording_scores_the_same_alone_or_in_a_batch(eng):
    recs = _mixed_recordings(eng, 70, 8)
    counts, mp = _check(eng, recs, "batch of 70")
    for q in (0, 1, 2, 3, 4, 35, 69):
        c1, m1 = _run(eng, recs[q][0], recs[q][1], [0, len(recs[q][0])], recs[q][2])
        assert np.array_equal(c1[0], counts[q]) and np.array_equal(m1[0], mp[q]), "recording %d" % q


def test_map_properties(eng):
    rng = np.random.default_rng(9)
    ref = np.asarray([10, 10, 20, 20, 20, 63, -1, 0], np.int32)
    hyp = np.asarray([4000, 4000, 4000, 7, 7, -1, 7, 9], np.int32)
    dur = np.asarray([5, 5, 3, 2, 2, 9, 9, 0], np.int32)          # ref 0 meets hyp 9 for 0 ticks only: not reported
    counts, mp = _check(eng, [(ref, hyp, dur), M.random_case(rng, 500, 64, 64, gap=1)], "map")
    want = np.full(64, -1, np.int32)
    want[10], want[20] = 4000, 7
    assert np.array_equal(mp[0], want)
    assert counts[0].tolist() == [26, 9, 9, 3]
    c2, none = _run(eng, ref, hyp, [0, 8], dur, want_map=False)
    assert none is None and np.array_equal(c2[0], counts[0])


def test_host_forms_equal_device_forms(eng):
    from plda_amd import der, diarize
    recs = _mixed_recordings(eng, 14, 10)
    offsets = diarize.offsets_of([len(x[0]) for x in recs])
    ref, hyp, dur = (np.concatenate([x[k] for x in recs]) for k in range(3))
    counts, mp = _run(eng, ref, hyp, offsets, dur)
    res = der.der(eng, ref, hyp, offsets, dur, return_map=True)
    assert res.counts.dtype == np.int64 and np.array_equal(res.counts, counts) and np.array_equal(res.map, mp)
    res2 = eng.der(ref.astype(np.int64), hyp.tolist(), offsets.tolist(), dur)
    assert np.array_equal(res2.counts, counts) and res2.map is None
    errs = counts[:, 1:].sum(1)
    assert np.array_equal(res.der, errs / counts[:, 0])
    assert res.total == int(errs.sum()) / int(counts[:, 0].sum())
    from liblda.plda import PLDA
    p = PLDA(0)
    assert np.array_equal(p.der(ref, hyp, offsets, dur).counts, counts)


# ------------------------------------------------------------------------------------------- sweep
@pytest.fixture(scope="module")
def sweep_case(eng):
    """planted-speaker blocks of N = 1, 40 and one size above the AHC's LDS class; their full merge records; a reference
    with non-speech; nine thresholds"""
    from plda_amd import diarize
    big = diarize.plan(eng, 1)["lds_max"] + 9
    blocks, ref = [], []
    for q, sizes in enumerate(([1], [9, 14, 17], [big // 4, big // 2, big - big // 4 - big // 2], [3, 3, 3, 3], [2])):
        S, g = M.planted_block(sizes, 40 + q, noise=0.6)
        blocks.append(S)
        ref.append(g)
    assert [b.shape[0] for b in blocks] == [1, 40, big, 12, 2]
    ref = np.concatenate(ref).astype(np.int32)
    ref_ns = ref.copy()
    ref_ns[5::6] = -1
    labels, ncl, merges = diarize.ahc(eng, blocks, None, 1, return_merges=True)
    assert (ncl == 1).all() and (merges[0] >= 0).all()
    offsets = diarize.offsets_of([b.shape[0] for b in blocks])
    cost = np.sort(merges[2])
    thresholds = np.asarray([-cost[len(cost) // 2], -cost[-1] - 1.0, 0.0, -cost[0] + 1.0, -cost[len(cost) // 3], 0.0, 0.35,
                             -cost[-8], -1e300], np.float64)
    assert (-thresholds[1] > cost).all() and (-thresholds[3] < cost).all()       # below / above every merge cost
    dur = np.random.default_rng(41).integers(0, 300, len(ref)).astype(np.int32)
    return blocks, merges, offsets, ref, ref_ns, dur, thresholds


@pytest.mark.parametrize("variant", ["plain", "num_speakers", "ref_with_non_speech", "null_dur"])
def test_sweep_equals_cut_then_der(eng, sweep_case, variant):
    from plda_amd import der, diarize
    blocks, merges, offsets, ref, ref_ns, dur, thresholds = sweep_case
    ns = [1, 5, 2, 12, 3] if variant == "num_speakers" else None
    rf = ref_ns if variant == "ref_with_non_speech" else ref
    du = None if variant == "null_dur" else dur
    counts, ncl = _run_sweep(eng, merges, offsets, rf, thresholds, du, ns)
    for q, thr in enumerate(thresholds):
        labels, k = diarize.cut(merges, offsets, float(thr), ns)
        assert np.array_equal(ncl[q], k), "n_clusters at threshold %d" % q
        assert np.array_equal(counts[q], M.score(rf, labels, offsets, du)), "counts at threshold %d against cut + model" % q
        assert np.array_equal(counts[q], der.der(eng, rf, labels, offsets, du).counts), "counts at threshold %d against cut + der" % q
    assert np.array_equal(counts[2], counts[5]) and np.array_equal(ncl[2], ncl[5])          # the two equal thresholds
    sizes = np.diff(offsets)
    assert np.array_equal(ncl[3], sizes) and np.array_equal(ncl[1], np.minimum(sizes, ns) if ns else np.ones(5))
    if variant == "plain":
        assert len({tuple(k) for k in ncl.tolist()}) >= 4                                # the interior thresholds cut differently
        res = der.sweep(eng, merges, offsets, rf, thresholds, du)
        assert np.array_equal(res.counts, counts) and np.array_equal(res.n_clusters, ncl)
        assert res.best == der.best_index(counts) and res.der[res.best] == np.nanmin(res.der)


def test_sweep_of_a_truncated_record_fails(eng, sweep_case):
    from plda_amd import diarize
    blocks, _, offsets, ref, _, dur, thresholds = sweep_case
    _, ncl, part = diarize.ahc(eng, blocks, 0.0, None, return_merges=True)               # stops at 0: the tail holds -1
    assert (part[0] < 0).any()
    counts, k = _run_sweep(eng, part, offsets, ref, [1e9, 2e9], dur)                     # no merge is asked for: the tail is never reached
    assert np.array_equal(k[0], np.diff(offsets)) and np.array_equal(k[1], k[0])
    assert _run_sweep(eng, part, offsets, ref, [1e9, -0.5], dur, expect=E_INVAL) == E_INVAL
    assert "not a full record" in eng._lib.plda_last_error(eng._h).decode()
    with pytest.raises(ValueError):
        diarize.cut(part, offsets, -0.5)
    bad = (part[0].copy(), part[1].copy(), part[2].copy())
    bad[1][0] = 4096                                                                     # an entry that is no merge
    bad[2][0] = -1e9
    assert _run_sweep(eng, bad, offsets, ref, [1e9, 0.0], dur, expect=E_INVAL) == E_INVAL


# ------------------------------------------------------------------------------------------- errors
def test_bad_input_fails_and_writes_nothing(eng, sweep_case):
    i32 = lambda *v: np.asarray(v, np.int32)
    ref, hyp, dur, off = i32(0, 1, 2, 3, 4, 5), i32(0, 0, 1, 1, 2, 2), i32(1, 2, 3, 4, 5, 6), [0, 4, 6]
    assert np.array_equal(_run(eng, ref, hyp, off, dur)[0], M.score(ref, hyp, off, dur))

    def put(a, k, v):
        a = a.copy()
        a[k] = v
        return a

    for r_, h_, d_ in ((put(ref, 1, 64), hyp, dur), (ref, put(hyp, 5, 4096), dur), (put(ref, 0, -2), hyp, dur), (ref, put(hyp, 3, -2), dur),
                       (ref, hyp, put(dur, 2, -1)), (put(ref, 4, 2 ** 31 - 1), hyp, None), (ref, put(hyp, 0, -2 ** 31), None)):
        assert _run(eng, r_, h_, off, d_, expect=E_INVAL) == E_INVAL
        assert "1 invalid" in eng._lib.plda_last_error(eng._h).decode()
    assert _run(eng, put(ref, 1, 64), put(put(hyp, 0, -5), 1, 9999), off, put(dur, 5, -7), expect=E_INVAL) == E_INVAL
    assert "3 invalid" in eng._lib.plda_last_error(eng._h).decode()
    for bad_off in ([0, 6, 4], [0, 4, 4], [1, 4, 6], [0, 4, 4 + 4097]):                  # not ascending, empty, not from 0, too long
        big = 4 + 4097 if bad_off[-1] > 6 else 6
        z = np.zeros(big, np.int32)
        assert _run(eng, z, z, bad_off, None, expect=E_INVAL) == E_INVAL
    assert _run(eng, ref, hyp, [0], dur, expect=E_INVAL) == E_INVAL                      # R = 0
    blocks, merges, offsets, sref, _, sdur, thresholds = sweep_case
    assert _run_sweep(eng, merges, offsets, sref, [], sdur, expect=E_INVAL) == E_INVAL   # Q = 0
    assert _run_sweep(eng, merges, offsets, sref, [0.0, float("nan")], sdur, expect=E_INVAL) == E_INVAL
    assert "NaN" in eng._lib.plda_last_error(eng._h).decode()
    assert _run_sweep(eng, merges, offsets, put(sref, 7, 64), [0.0], sdur, expect=E_INVAL) == E_INVAL
    assert _run_sweep(eng, merges, offsets, sref, [0.0], put(sdur, 0, -1), expect=E_INVAL) == E_INVAL
    assert _run_sweep(eng, merges, offsets, sref, [0.0], sdur, num_speakers=[1, 1, 0, 1, 1], expect=E_INVAL) == E_INVAL
    # after the failures the handle works as before
    assert np.array_equal(_run(eng, ref, hyp, off, dur)[0], M.score(ref, hyp, off, dur))


# ------------------------------------------------------------------------------------------- tune_threshold
def _model_params(d, seed, psi_scale=1.0):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    return rng.random(d), q * (0.5 + rng.random(d))[:, None], np.sort(rng.random(d) * 3.0 + 0.05)[::-1].copy() * psi_scale


def test_tune_threshold_equals_cluster_then_sweep_and_q_separate_runs():
    from liblda.plda import PLDA
    from plda_amd import der, diarize
    d, counts = 16, (4, 9, 14)
    mean, T, psi = _model_params(d, 11, psi_scale=4.0)
    p = PLDA(0)
    e = p._instance
    e.set_model(mean, T, psi)
    rng = np.random.default_rng(12)
    rows, ref = [], []
    for _ in range(5):
        g = rng.permutation(np.repeat(np.arange(len(counts)), counts))
        y = rng.standard_normal((len(counts), d)) * np.sqrt(psi)
        rows.append(mean + (y[g] + rng.standard_normal((len(g), d))) @ np.linalg.inv(T).T)
        ref.append(g)
    x, ref = np.concatenate(rows), np.concatenate(ref).astype(np.int32)
    offsets = diarize.offsets_of([sum(counts)] * 5)
    dur = rng.integers(1, 50, len(ref)).astype(np.int32)
    thresholds = np.asarray([-40.0, -10.0, -3.0, 0.0, 0.0, 3.0, 10.0, 40.0])
    best, res = p.tune_threshold(x, offsets, ref, thresholds, dur)
    _, _, merges = p.cluster(x, offsets, threshold=None, num_speakers=1, return_merges=True)
    hand = der.sweep(e, merges, offsets, ref, thresholds, dur)
    assert np.array_equal(res.counts, hand.counts) and np.array_equal(res.n_clusters, hand.n_clusters) and res.best == hand.best
    totals = []
    for q, thr in enumerate(thresholds):
        labels, ncl = p.cluster(x, offsets, threshold=float(thr))
        one = p.der(ref, labels, offsets, dur)
        assert np.array_equal(one.counts, res.counts[q]) and np.array_equal(ncl, res.n_clusters[q]), "threshold %d" % q
        totals.append(one.total)
    assert best == thresholds[int(np.argmin(totals))] and res.best == int(np.argmin(totals))
    assert len(set(totals)) > 2
    with pytest.raises(ValueError):
        p.tune_threshold(x, offsets, ref, [0.0, float("nan")], dur)
    with pytest.raises(ValueError):
        p.tune_threshold(x, offsets, ref[:-1], [0.0], dur)
