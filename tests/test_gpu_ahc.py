"""GPU: the speaker clustering (csrc/ahc.hip) against its NumPy model (tests/ahc_model.py).  The contract is exact, so every
comparison is array_equal on the bits of labels, n_clusters, merge_a, merge_b and merge_cost: no tolerances.

Every device call of this file goes through _run: the scores sit between NaN neighbours, every output between guard bands
filled with a payload that must stay intact outside the output and be gone inside it (the pattern of
tests/test_gpu_guard_bands.py).  The families run once on fresh and once on poisoned scratch, bit-identical (the pattern of
tests/test_gpu_scratch_poison.py), and ten create -> cluster -> destroy cycles give back every byte."""
import gc

import numpy as np
import pytest

import ahc_model as M

pytestmark = pytest.mark.gpu

GUARD = 16 << 10           # elements on either side
PAYLOAD = 0x7FC0DEAD
E_INVAL = -1


def _dev():
    import torch
    return torch.device("cuda", 0)


def _guarded_input(a):
    """a 1-D host array inside a device buffer whose neighbours are NaN (floats) or -1"""
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
        if written:
            left = int((w[lo:hi] == np.int32(PAYLOAD)).all(1).sum())
            assert left == 0, "%s: %d output elements never written" % (what, left)
        return self.body.cpu().numpy().copy()


def _lib():
    from plda_amd import _native as N
    return N.load()


def _raw_call(eng, dscores, block_off, offsets, r, has_t, thr, minc, outs):
    """the C entry point itself -> status code"""
    import ctypes as C
    vp = lambda x: C.c_void_p(int(x)) if x else None
    hp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    return _lib().plda_ahc_matrix_dev(eng._h, vp(dscores), hp(block_off), hp(offsets), int(r), int(has_t), float(thr), hp(minc),
                                      *[vp(o) for o in outs])


def _stop(offsets, threshold, num_speakers):
    from plda_amd import diarize
    return diarize.stop_args(offsets, threshold, num_speakers)


def _run(eng, blocks, threshold=None, num_speakers=1, merges=True, expect=0):
    """plda_ahc_matrix_dev on guarded buffers -> (labels, n_clusters, merge_a, merge_b, merge_cost) (merges=False: the last
    three None), or the status code when expect != 0"""
    import torch
    from plda_amd import diarize
    scores, block_off, offsets = diarize.pack(blocks)
    has_t, thr, minc = _stop(offsets, threshold, num_speakers)
    r, t = len(blocks), int(offsets[-1])
    _, ds = _guarded_input(scores)
    oL, oK = _Out(t, torch.int32), _Out(r, torch.int32)
    oA, oB, oC = _Out(t - r, torch.int32), _Out(t - r, torch.int32), _Out(t - r, torch.float64)
    torch.cuda.synchronize()
    outs = [oL.ptr(), oK.ptr()] + ([oA.ptr(), oB.ptr(), oC.ptr()] if merges else [None, None, None])
    rc = _raw_call(eng, ds.data_ptr(), block_off, offsets, r, has_t, thr, minc, outs)
    torch.cuda.synchronize()
    assert rc == expect, "status %d: %s" % (rc, eng._lib.plda_last_error(eng._h).decode())
    if expect:
        for o, name in ((oL, "labels"), (oK, "n_clusters"), (oA, "merge_a"), (oB, "merge_b"), (oC, "merge_cost")):
            o.check(name, written=False)
        return rc
    res = [oL.check("labels"), oK.check("n_clusters")]
    for o, name in ((oA, "merge_a"), (oB, "merge_b"), (oC, "merge_cost")):
        res.append(o.check(name) if merges else None)
        if not merges:
            o.check(name, written=False)
            assert (o.body.view(torch.int32) == PAYLOAD).all()
    return tuple(res)


def _assert_equal(got, want, what=""):
    for g, w, name in zip(got, want, ("labels", "n_clusters", "merge_a", "merge_b", "merge_cost")):
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), "%s %s: %d of %d differ" % (what, name, int((g != w).sum()), g.size)


@pytest.fixture(scope="module")
def eng():
    from plda_amd import MPlda
    return MPlda(0)


@pytest.fixture(scope="module")
def lds_max(eng):
    from plda_amd import diarize
    return diarize.plan(eng, 1)["lds_max"]


FAMILIES = {"gaussian": lambda n: M.gaussian(n, 7 * n + 1), "integers": lambda n: M.integers(n, 3 * n + 2), "chain": lambda n: M.chain(n),
            "chain_reverse": lambda n: M.chain(n, True), "equal": lambda n: M.all_equal(n), "zeros": lambda n: M.signed_zeros(n, n)}
_REF = {}


def _ref(family, n):
    """the model's full merge record of one block, computed once per (family, n) and left unchanged"""
    if (family, n) not in _REF:
        S = FAMILIES[family](n)
        S.setflags(write=False)
        _REF[family, n] = (S, M.cluster([S], None, 1))
    return _REF[family, n]


def test_plan_names_the_classes(eng, lds_max):
    from plda_amd import diarize
    assert 64 < lds_max < 257
    assert diarize.plan(eng, lds_max) == {"cls": 0, "scratch_bytes": 0, "lds_max": lds_max}
    assert diarize.plan(eng, lds_max + 1) == {"cls": 1, "scratch_bytes": 8 * (lds_max + 1) ** 2, "lds_max": lds_max}
    assert diarize.plan(eng, 4096)["scratch_bytes"] == 8 * 4096 * 4096
    out = (__import__("ctypes").c_int32 * 3)()
    assert _lib().plda_ahc_plan(eng._h, 0, out) == E_INVAL and _lib().plda_ahc_plan(eng._h, 4097, out) == E_INVAL


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("which", ["small", "boundary", "hbm257", "hbm513"])
def test_full_merge_record_equals_the_model(eng, lds_max, family, which):
    """every size on its own call: N in {1, 2, 3, 63, 64, 65}, L - 1, L, L + 1 around the class boundary, 257 and 513"""
    sizes = {"small": [1, 2, 3, 63, 64, 65], "boundary": [lds_max - 1, lds_max, lds_max + 1], "hbm257": [257], "hbm513": [513]}[which]
    for n in sizes:
        S, want = _ref(family, n)
        _assert_equal(_run(eng, [S], None, 1), want, "%s n=%d" % (family, n))


def _mixed_blocks(lds_max):
    return [FAMILIES[f](n) for f, n in (("gaussian", 5), ("integers", 64), ("gaussian", lds_max), ("integers", lds_max + 1),
                                        ("gaussian", 257), ("zeros", 9), ("gaussian", 1), ("chain", 70))]


@pytest.mark.parametrize("rule", ["above_every_score", "mid", "count_1", "count_n", "count_mixed", "both"])
def test_stop_rules(eng, lds_max, rule):
    blocks = _mixed_blocks(lds_max)
    sizes = [b.shape[0] for b in blocks]
    r = len(blocks)
    thr, ns = {"above_every_score": (1e6, None), "mid": (0.25, None), "count_1": (None, 1), "count_n": (None, sizes),
               "count_mixed": (None, [1, 64, 3, 7, 200, 2, 1, 70]), "both": (-0.4, [1, 30, 2, 100, 5, 1, 1, 2])}[rule]
    want = M.cluster(blocks, thr, ns)
    got = _run(eng, blocks, thr, ns)
    _assert_equal(got, want, rule)
    if rule in ("above_every_score", "count_n"):          # no merge anywhere: the whole record is tail
        assert (got[2] == -1).all() and (got[3] == -1).all() and np.isposinf(got[4]).all()
        assert got[1].tolist() == sizes
    if rule == "both":                                    # each rule binds somewhere
        minc = np.asarray(ns)
        assert (got[1] == np.maximum(minc, 1)).any() and (got[1] > np.maximum(minc, 1)).any()
    _assert_equal(_run(eng, blocks, thr, ns, merges=False), want[:2] + (None, None, None), rule + " without merges")


def test_ragged_call_equals_one_call_each(monkeypatch, lds_max):
    """about 300 recordings of both classes, shuffled, more than one launch holds in flight: a scratch budget of 1 MiB puts two
    or three HBM-class recordings into a launch, and the LDS class brings more workgroups than the device runs at once"""
    from plda_amd import MPlda
    rng = np.random.default_rng(2024)
    sizes = np.concatenate([rng.integers(1, lds_max + 1, 270), rng.integers(lds_max + 1, 241, 30), [lds_max, lds_max + 1]])
    rng.shuffle(sizes)
    blocks = [(M.gaussian if i % 3 else M.integers)(int(n), 50_000 + i) for i, n in enumerate(sizes)]
    ns = rng.integers(1, 4, len(blocks))
    monkeypatch.setenv("PLDA_AHC_SCRATCH_BYTES", str(1 << 20))
    small = MPlda(0)
    monkeypatch.delenv("PLDA_AHC_SCRATCH_BYTES")
    want = M.cluster(blocks, 0.1, ns)
    held = _lib().plda_device_bytes_held()
    got = _run(small, blocks, 0.1, ns)
    _assert_equal(got, want, "ragged")
    assert _lib().plda_device_bytes_held() - held < (4 << 20)      # (the scratch is the budget's, not the call's 13 MB of sums)
    from plda_amd import diarize
    offsets = diarize.offsets_of(sizes)
    sl = diarize.merge_slices(offsets)
    big = MPlda(0)
    for q, S in enumerate(blocks):
        one = _run(big if q % 2 else small, [S], 0.1, int(ns[q]))
        a, b = sl[q]
        _assert_equal(one, (got[0][offsets[q]:offsets[q + 1]], got[1][q:q + 1], got[2][a:b], got[3][a:b], got[4][a:b]), "recording %d" % q)


def test_non_finite_scores_fail_with_the_count(eng, lds_max):
    blocks = [M.gaussian(6, 1).copy(), M.gaussian(lds_max + 2, 2).copy(), M.gaussian(40, 3).copy()]
    blocks[0][3, 3] = np.nan                               # the diagonal is never read
    blocks[1][7, 7] = np.inf
    _assert_equal(_run(eng, blocks, 0.0, None), M.cluster(blocks, 0.0, None), "NaN on the diagonal")
    blocks[0][1, 4] = np.nan
    blocks[1][200, 3] = -np.inf
    blocks[2][39, 0] = np.inf
    assert _run(eng, blocks, 0.0, None, expect=E_INVAL) == E_INVAL
    assert "3 non-finite" in eng._lib.plda_last_error(eng._h).decode()
    _assert_equal(_run(eng, [blocks[2][:20, :20].copy()], 0.0, None), M.cluster([blocks[2][:20, :20]], 0.0, None), "after a failure")


def test_bad_arguments(eng):
    import torch
    S = M.gaussian(4, 1)
    ds = torch.from_numpy(np.concatenate([S.ravel(), S.ravel()])).to(_dev())
    L, K = torch.zeros(8, dtype=torch.int32, device=_dev()), torch.zeros(2, dtype=torch.int32, device=_dev())
    A, B = torch.zeros(6, dtype=torch.int32, device=_dev()), torch.zeros(6, dtype=torch.int32, device=_dev())
    Cc = torch.zeros(6, dtype=torch.float64, device=_dev())
    i64 = lambda *v: np.asarray(v, np.int64)
    full = [L.data_ptr(), K.data_ptr(), A.data_ptr(), B.data_ptr(), Cc.data_ptr()]

    def call(block_off=i64(0, 16, 32), offsets=i64(0, 4, 8), r=2, minc=None, outs=full, scores=ds.data_ptr()):
        return _raw_call(eng, scores, block_off, offsets, r, 1, 0.0, minc, outs)

    assert call() == 0
    assert call(offsets=i64(1, 4, 8)) == E_INVAL                          # not from 0
    assert call(offsets=i64(0, 4, 4)) == E_INVAL                          # an empty recording
    assert call(offsets=i64(0, 5, 4)) == E_INVAL                          # descending
    assert call(offsets=i64(0, 4, 4 + 4097)) == E_INVAL                   # above PLDA_AHC_MAX
    assert "PLDA_AHC_MAX" in eng._lib.plda_last_error(eng._h).decode()
    assert call(block_off=i64(0, 15, 32)) == E_INVAL                      # a block shorter than N * N
    assert call(block_off=i64(0, 16, 31)) == E_INVAL
    assert call(minc=np.asarray([1, 0], np.int32)) == E_INVAL
    assert call(minc=np.asarray([-3, 1], np.int32)) == E_INVAL
    assert call(r=0) == E_INVAL
    assert call(scores=None) == E_INVAL
    assert call(outs=[None] + full[1:]) == E_INVAL and call(outs=[full[0], None] + full[2:]) == E_INVAL
    for keep in range(3):                                                 # one merge pointer alone, or two
        outs = full[:2] + [full[2 + j] if j == keep else None for j in range(3)]
        assert call(outs=outs) == E_INVAL
        outs = full[:2] + [None if j == keep else full[2 + j] for j in range(3)]
        assert call(outs=outs) == E_INVAL
    assert "together" in eng._lib.plda_last_error(eng._h).decode()
    assert call(outs=full[:2] + [None, None, None]) == 0
    with pytest.raises(ValueError, match="num_speakers"):
        from plda_amd import diarize
        diarize.ahc(eng, [S], threshold=None, num_speakers=None)


def test_host_form_equals_device_form(eng, lds_max):
    from plda_amd import diarize
    blocks = _mixed_blocks(lds_max)[:5]
    want = M.cluster(blocks, 0.0, 2)
    labels, ncl, merges = diarize.ahc(eng, blocks, 0.0, 2, return_merges=True)
    _assert_equal((labels, ncl) + merges, want, "host form")
    labels, ncl = diarize.ahc(eng, blocks, 0.0, 2)
    _assert_equal((labels, ncl), want[:2], "host form without merges")
    c_labels, c_ncl = diarize.cut(M.cluster(blocks, None, 1)[2:], diarize.offsets_of([b.shape[0] for b in blocks]), 0.0, 2)
    _assert_equal((c_labels, c_ncl), (labels, ncl), "cut of a full record")


# ------------------------------------------------------------------------------------------- poisoned scratch, leaks
def _engine(monkeypatch, poison):
    from plda_amd import MPlda
    if poison:
        monkeypatch.setenv("PLDA_SCRATCH_POISON", "1")
    else:
        monkeypatch.delenv("PLDA_SCRATCH_POISON", raising=False)
    monkeypatch.setenv("PLDA_AHC_SCRATCH_BYTES", str(2 << 20))
    e = MPlda(0)
    monkeypatch.delenv("PLDA_SCRATCH_POISON", raising=False)
    monkeypatch.delenv("PLDA_AHC_SCRATCH_BYTES")
    return e


def _model_params(d, seed, psi_scale=1.0):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    return rng.random(d), q * (0.5 + rng.random(d))[:, None], np.sort(rng.random(d) * 3.0 + 0.05)[::-1].copy() * psi_scale


@pytest.mark.parametrize("family", ["matrix", "operand"])
def test_fresh_and_poisoned_scratch_agree(monkeypatch, lds_max, family):
    from plda_amd import MPlda, diarize
    blocks = _mixed_blocks(lds_max) + [M.integers(lds_max + 3, 5), M.gaussian(230, 6)]
    rng = np.random.default_rng(5)
    sizes = [1, 5, 64, lds_max + 1, 37]
    vecs, offsets = rng.standard_normal((sum(sizes), 24)), diarize.offsets_of(sizes)
    res = {}
    for poison in (False, True):
        e = _engine(monkeypatch, poison)
        if family == "matrix":
            res[poison] = _run(e, blocks, 0.05, 2)
        else:
            e.set_model(*_model_params(24, 3))
            labels, ncl, mg = diarize.ahc_vectors(e, vecs, offsets, 0.0, 1, return_merges=True)
            res[poison] = (labels, ncl) + mg
        e.synchronize()
        del e
    MPlda(0)                       # the switch off again for whatever runs next in this process
    _assert_equal(res[True], res[False], "poisoned against fresh")
    if family == "matrix":
        _assert_equal(res[False], M.cluster(blocks, 0.05, 2), "fresh")


def test_create_cluster_destroy_gives_back_every_byte(lds_max):
    from plda_amd import MPlda, diarize
    blocks = [M.gaussian(30, 1), M.gaussian(lds_max + 5, 2)]
    rng = np.random.default_rng(6)
    vecs, offsets = rng.standard_normal((80, 16)), diarize.offsets_of([50, 30])
    gc.collect()
    first = _lib().plda_device_bytes_held()
    for cycle in range(10):
        e = MPlda(0)
        diarize.ahc(e, blocks, 0.0)
        e.set_model(*_model_params(16, 2))
        diarize.ahc_vectors(e, vecs, offsets, 0.0)
        assert _lib().plda_device_bytes_held() > first
        del e
        gc.collect()
        held = _lib().plda_device_bytes_held()
        assert held == first, "cycle %d: %d bytes of device memory not given back" % (cycle, held - first)


# ------------------------------------------------------------------------------------------- operand form
def _scored_blocks(eng, dX, offsets):
    """every recording's block as plda_score_matrix_dev writes it (ld_out = N) from the device rows dX"""
    import torch
    blocks = []
    for q in range(len(offsets) - 1):
        n = int(offsets[q + 1] - offsets[q])
        S = torch.full((n, n), float("nan"), dtype=torch.float32, device=_dev())
        x = dX[int(offsets[q]):int(offsets[q + 1])]
        torch.cuda.synchronize()
        eng.score_matrix_dev(x.data_ptr(), None, 1, n, x.data_ptr(), n, S.data_ptr(), n)
        eng.synchronize()
        blocks.append(S.cpu().numpy())
    return blocks


def _run_operands(eng, dX, offsets, thr, ns):
    """plda_score_ahc_dev with guarded outputs -> (labels, n_clusters, merge_a, merge_b, merge_cost)"""
    import torch
    has_t, t, minc = _stop(offsets, thr, ns)
    tot, r = int(offsets[-1]), len(offsets) - 1
    oL, oK = _Out(tot, torch.int32), _Out(r, torch.int32)
    oA, oB, oC = _Out(tot - r, torch.int32), _Out(tot - r, torch.int32), _Out(tot - r, torch.float64)
    torch.cuda.synchronize()
    eng.score_ahc_dev(dX.data_ptr(), offsets, has_t, t, minc, oL.ptr(), oK.ptr(), oA.ptr(), oB.ptr(), oC.ptr())
    torch.cuda.synchronize()
    return (oL.check("labels"), oK.check("n_clusters"), oA.check("merge_a"), oB.check("merge_b"), oC.check("merge_cost"))


@pytest.mark.parametrize("d", [8, 200])
def test_operand_form_equals_matrix_form_on_scored_blocks(eng, d):
    """recordings of 1, 5, 64 and 200 segments: plda_score_ahc_dev == plda_ahc_matrix_dev on the blocks plda_score_matrix_dev
    writes (ld_out = N), exactly; both equal the model on those blocks"""
    import torch
    from plda_amd import diarize
    eng.set_model(*_model_params(d, d))
    sizes = [1, 5, 64, 200]
    offsets = diarize.offsets_of(sizes)
    rng = np.random.default_rng(d)
    spk = rng.standard_normal((6, d)) * 1.5
    vecs = np.concatenate([spk[rng.integers(0, 6, n)] + rng.standard_normal((n, d)) for n in sizes])
    dX = torch.from_numpy(vecs).to(_dev())
    blocks = _scored_blocks(eng, dX, offsets)
    for thr, ns in ((0.0, None), (None, 2), (5.0, [1, 2, 3, 4])):
        got = _run_operands(eng, dX, offsets, thr, ns)
        _assert_equal(got, _run(eng, blocks, thr, ns), "operand against matrix form")
        _assert_equal(got, M.cluster(blocks, thr, ns), "operand form against the model")
        host = diarize.ahc_vectors(eng, vecs, offsets, thr, ns, return_merges=True)
        _assert_equal((host[0], host[1]) + host[2], got, "host operand form")


def _generate(mean, T, psi, counts, rng):
    """rows from the model's own generative form: u = y_speaker + e in the model's space (y ~ N(0, psi), e ~ N(0, I)),
    x = mean + T^-1 u; the speakers' segments interleaved at random -> (rows, speaker of each row)"""
    d = len(mean)
    g = rng.permutation(np.repeat(np.arange(len(counts)), counts))
    y = rng.standard_normal((len(counts), d)) * np.sqrt(psi)
    u = y[g] + rng.standard_normal((len(g), d))
    return mean + u @ np.linalg.inv(T).T, g


def test_cluster_recovers_planted_speakers():
    """PLDA.cluster on raw rows == transform + operand form; with num_speakers = 4 and no threshold it returns the planted
    partition of rows drawn from the model itself (between-speaker variances 8 x those of _model_params: the model, run on the
    device's own score blocks, recovers the partition -- asserted first)"""
    import torch
    from liblda.plda import PLDA
    from plda_amd import diarize
    d, counts = 24, (3, 7, 12, 20)
    mean, T, psi = _model_params(d, 77, psi_scale=8.0)
    p = PLDA(0)
    e = p._instance
    e.set_model(mean, T, psi)
    rng = np.random.default_rng(77)
    rows, groups = zip(*[_generate(mean, T, psi, counts, rng) for _ in range(6)])
    x = np.concatenate(rows)
    n = sum(counts)
    offsets = diarize.offsets_of([n] * 6)
    labels, ncl, merges = p.cluster(x, offsets, threshold=None, num_speakers=4, return_merges=True)
    vecs = e.transform_array(x, 1)
    via = diarize.ahc_vectors(e, vecs, offsets, None, 4, return_merges=True)
    _assert_equal((labels, ncl) + merges, (via[0], via[1]) + via[2], "PLDA.cluster against transform + operand form")
    dX = torch.from_numpy(vecs).to(_dev())
    blocks = []
    for q in range(6):
        S = torch.empty((n, n), dtype=torch.float32, device=_dev())
        xq = dX[q * n:(q + 1) * n]
        torch.cuda.synchronize()
        e.score_matrix_dev(xq.data_ptr(), None, 1, n, xq.data_ptr(), n, S.data_ptr(), n)
        e.synchronize()
        blocks.append(S.cpu().numpy())
    want = M.cluster(blocks, None, 4)
    _assert_equal((labels, ncl) + merges, want, "against the model on the device's blocks")
    assert ncl.tolist() == [4] * 6
    for q in range(6):
        assert np.array_equal(labels[q * n:(q + 1) * n], M.first_member_labels(groups[q])), "recording %d" % q
    with pytest.raises(ValueError, match="num_speakers"):
        p.cluster(x, offsets, threshold=None)


# ------------------------------------------------------------------------------------------- full size
def _unequal_sizes(total, groups, seed):
    rng = np.random.default_rng(seed)
    w = rng.random(groups) + 0.2
    s = np.maximum(1, np.floor(w / w.sum() * total).astype(np.int64))
    s[0] += total - s.sum()
    assert s.sum() == total and s.min() >= 1 and len(set(s.tolist())) > groups // 2
    return s


def test_full_size_recording_of_4096_segments(eng):
    """N = PLDA_AHC_MAX: 16 planted groups of unequal sizes, +1 inside and -1 across, threshold 0 -- the largest shape and the
    heaviest tie load (every within-group pair ties at every step).  Only the labels are checked: the groups numbered by
    first member.  That the RULE yields this answer is shown by the model on the same construction at N = 256."""
    S256, g256 = M.planted(_unequal_sizes(256, 16, 9), seed=9)
    want256 = M.cluster([S256], 0.0, None)
    assert np.array_equal(want256[0], M.first_member_labels(g256)) and want256[1].tolist() == [16]
    _assert_equal(_run(eng, [S256], 0.0, None), want256, "n = 256")
    S, g = M.planted(_unequal_sizes(4096, 16, 10), seed=10)
    labels, ncl, _, _, _ = _run(eng, [S], 0.0, None, merges=False)
    assert ncl.tolist() == [16]
    assert np.array_equal(labels, M.first_member_labels(g))
