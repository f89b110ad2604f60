"""GPU: the time-based diarisation error rate (csrc/der_time.hip, the atom form of csrc/der.hip's solve) against its host
models (tests/der_time_model.py).  The contract is exact: every comparison of counts is ==, for every recording generated.

Every device call goes through _run / _run_sweep: inputs between -1 / NaN neighbours, outputs between guard bands filled with
a payload that must stay intact outside the output and be gone inside it (the helpers of test_gpu_der)."""
import ctypes as C

import numpy as np
import pytest

import der_model as M
import der_time_model as T
from test_gpu_der import E_INVAL, GUARD, _guarded_input, _hp, _lib, _Out, _vp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from plda_amd import MPlda
    return MPlda(0)


def _ptr(buf):
    """the device address of a guarded input (an empty one: the address behind the leading guard, never NULL)"""
    whole, body = buf
    return _vp(body.data_ptr() if body.numel() else whole[GUARD:].data_ptr())


def _inputs(turns, ss, sd, uem):
    keep = [_guarded_input(np.asarray(a, np.int32)) for a in (turns[0], turns[1], turns[2], ss, sd)]
    ukeep = [_guarded_input(np.asarray(a, np.int32)) for a in uem[:2]] if uem is not None else None
    return keep, ukeep


def _run(eng, packed, collar=0, flags=0, want_map=True, expect=0):
    """plda_der_timed_dev on guarded buffers -> (counts int64 [R, 4], map int32 [R, 64] or None), or the status"""
    import torch
    turns, ss, sd, hyp, off, uem = packed
    r = len(off) - 1
    keep, ukeep = _inputs(turns, ss, sd, uem)
    khyp = _guarded_input(np.asarray(hyp, np.int32))
    oC, oM = _Out(max(r, 0) * 4, torch.int64), _Out(max(r, 0) * M.MAX_REF, torch.int32)
    torch.cuda.synchronize()
    rc = _lib().plda_der_timed_dev(eng._h, _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), _hp(np.ascontiguousarray(turns[3], np.int64)),
                                   _ptr(keep[3]), _ptr(keep[4]), _ptr(khyp), _hp(np.ascontiguousarray(off, np.int64)), r,
                                   _ptr(ukeep[0]) if uem is not None else None, _ptr(ukeep[1]) if uem is not None else None,
                                   _hp(np.ascontiguousarray(uem[2], np.int64)) if uem is not None else None, collar, flags, _vp(oC.ptr()),
                                   _vp(oM.ptr()) if want_map else None)
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


def _run_sweep(eng, merges, packed, thresholds, num_speakers=None, collar=0, flags=0, expect=0):
    """plda_der_timed_sweep_dev on guarded buffers -> (counts int64 [Q, R, 4], n_clusters int32 [Q, R]), or the status"""
    import torch
    from plda_amd import diarize
    turns, ss, sd, _, off, uem = packed
    off = np.ascontiguousarray(off, np.int64)
    thresholds = np.ascontiguousarray(thresholds, np.float64)
    r, q = len(off) - 1, len(thresholds)
    minc = diarize.stop_args(off, 0.0, num_speakers)[2]
    keep, ukeep = _inputs(turns, ss, sd, uem)
    km = [_guarded_input(np.asarray(merges[0], np.int32)), _guarded_input(np.asarray(merges[1], np.int32)),
          _guarded_input(np.asarray(merges[2], np.float64))]
    oC, oK = _Out(q * r * 4, torch.int64), _Out(q * r, torch.int32)
    torch.cuda.synchronize()
    rc = _lib().plda_der_timed_sweep_dev(eng._h, _ptr(km[0]), _ptr(km[1]), _ptr(km[2]), _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]),
                                         _hp(np.ascontiguousarray(turns[3], np.int64)), _ptr(keep[3]), _ptr(keep[4]), _hp(off), r,
                                         _ptr(ukeep[0]) if uem is not None else None, _ptr(ukeep[1]) if uem is not None else None,
                                         _hp(np.ascontiguousarray(uem[2], np.int64)) if uem is not None else None, collar, flags,
                                         _hp(thresholds), q, _hp(minc), _vp(oC.ptr()), _vp(oK.ptr()))
    torch.cuda.synchronize()
    assert rc == expect, "status %d: %s" % (rc, eng._lib.plda_last_error(eng._h).decode())
    if expect:
        oC.check("counts", written=False)
        oK.check("n_clusters", written=False)
        return rc
    return oC.check("counts").reshape(q, r, 4), oK.check("n_clusters").reshape(q, r)


def _check(eng, recs, what, collar=0, skip=False, model=T.score_ticks, want_map=False):
    counts, mp = _run(eng, T.pack(recs), collar, T.SKIP_OVERLAP if skip else 0, want_map)
    want = T.counts(recs, collar, skip, model)
    assert np.array_equal(counts, want), "%s: counts\n%r\nmodel\n%r" % (what, counts[:8], want[:8])
    return counts, mp


def _last(eng):
    return eng._lib.plda_last_error(eng._h).decode()


# ------------------------------------------------------------------------------------------- the definition at its edges
def test_worked_example_from_the_public_interface(eng):
    from liblda.plda import PLDA
    turns, ss, sd, hyp, off, _ = T.pack([T.rec(ts=[0, 5], td=[10, 10], tk=[0, 1], ss=[0], sd=[15], hyp=[7])])
    p = PLDA(0)
    assert p.der_timed(turns, ss, sd, hyp, off).counts.tolist() == [[20, 5, 0, 5]]
    res = p.der_timed(turns, ss, sd, hyp, off, collar=1, return_map=True)
    assert res.counts.tolist() == [[12, 3, 0, 3]] and res.total == 0.5
    assert sorted(res.map[0][:2].tolist()) == [-1, 7] and (res.map[0][2:] == -1).all()


def _edge_recordings():
    all64 = T.rec(ts=np.full(64, 3), td=np.full(64, 20), tk=np.arange(64), ss=[0], sd=[30], hyp=[9])
    same_tick = T.rec(ts=[5, 15, 15, 25], td=[10, 10, 10, 5], tk=[0, 0, 1, 2], ss=[0, 15], sd=[15, 20], hyp=[1, 2], us=[0, 15], ud=[15, 30])
    return [("one turn, one segment", T.rec([2], [9], [5], [4], [12], [3]), 0, False),
            ("no turns: all false alarm", T.rec(ss=[0, 10], sd=[5, 7], hyp=[1, 2]), 0, False),
            ("no turns under a collar", T.rec(ss=[0, 10], sd=[5, 7], hyp=[1, 2]), 3, False),
            ("no hypothesis speech: all miss", T.rec([0, 4], [10, 10], [0, 1], [0, 10], [10, 10], [-1, -1]), 0, False),
            ("empty segments only", T.rec([0, 4], [10, 10], [0, 1], [3, 8], [0, 0], [1, 2]), 0, False),
            ("abutting turns of one speaker", T.rec([0, 10, 20], [10, 10, 5], [3, 3, 3], [0], [30], [0]), 0, False),
            ("abutting turns under a collar", T.rec([0, 10, 20], [10, 10, 5], [3, 3, 3], [0], [30], [0]), 2, False),
            ("three speakers overlapping", T.rec([0, 5, 8], [20, 20, 20], [0, 1, 2], [0, 12], [12, 20], [0, 1]), 0, False),
            ("three speakers, overlap skipped", T.rec([0, 5, 8], [20, 20, 20], [0, 1, 2], [0, 12], [12, 20], [0, 1]), 0, True),
            ("three speakers, collar and overlap skipped", T.rec([0, 5, 8], [20, 20, 20], [0, 1, 2], [0, 12], [12, 20], [0, 1]), 2, True),
            ("64 speakers at once", all64, 0, False), ("64 speakers at once, collar", all64, 4, False),
            ("64 speakers at once, overlap skipped", all64, 0, True),
            ("collar larger than every turn", T.rec([10, 30, 35], [8, 6, 9], [0, 1, 0], [0], [60], [0]), 5, False),
            ("collar zones below tick 0", T.rec([0, 2], [30, 9], [0, 1], [0], [40], [0]), 7, False),
            ("every kind of event on one tick", same_tick, 5, False), ("the same without collar", same_tick, 0, False),
            ("UEM outside the speech", T.rec([10], [10], [0], [10], [10], [0], us=[0, 30], ud=[10, 50]), 0, False),
            ("UEM cuts mid-turn", T.rec([10], [10], [0], [5], [20], [0], us=[12, 14], ud=[5, 2]), 1, False)]


def test_edge_recordings_one_by_one(eng):
    seen = {}
    for what, r, collar, skip in _edge_recordings():
        counts, mp = _check(eng, [r], what, collar, skip, want_map=True)
        assert np.array_equal(counts, T.counts([r], collar, skip, T.score_atoms)), what
        T.check_map(mp[0], r, collar, skip)
        seen[what] = counts[0].tolist()
    assert seen["no turns: all false alarm"] == [0, 0, 12, 0] and seen["no hypothesis speech: all miss"] == [20, 20, 0, 0]
    assert seen["collar larger than every turn"][0] == 0 and seen["UEM outside the speech"] == [0, 0, 0, 0]
    assert seen["64 speakers at once"] == [64 * 20, 63 * 20, 10, 0] and seen["64 speakers at once, overlap skipped"] == [0, 0, 10, 0]
    assert seen["empty segments only"] == [20, 20, 0, 0] and seen["abutting turns of one speaker"] == [25, 0, 5, 0]


def test_one_turn_per_segment_equals_the_segment_form(eng):
    from test_gpu_der import _run as run_segments
    from plda_amd import diarize
    rng = np.random.default_rng(21)
    recs, seg = [], []
    for n, sr, sh in ((1, 1, 1), (40, 3, 5), (300, 10, 40), (90, 64, 64)):
        ref, hyp, dur = M.random_case(rng, n, sr, sh)
        start = np.concatenate([[0], np.cumsum(dur + rng.integers(0, 3, n))[:-1]]).astype(np.int32)
        keep = ref >= 0
        recs.append(T.rec(start[keep], dur[keep], ref[keep], start, dur, hyp))
        seg.append((ref, hyp, dur))
    offsets = diarize.offsets_of([len(a) for a, _, _ in seg])
    want, _ = run_segments(eng, np.concatenate([a for a, _, _ in seg]), np.concatenate([b for _, b, _ in seg]), offsets,
                           np.concatenate([d for _, _, d in seg]))
    counts, _ = _run(eng, T.pack(recs))
    assert np.array_equal(counts, want)


@pytest.fixture(scope="module")
def seeded():
    rng = np.random.default_rng(77)
    recs = []
    for k in range(200):
        n, nt = (1, 0) if k == 0 else (60, 80) if k == 1 else (int(rng.integers(1, 61)), int(rng.integers(0, 81)))
        recs.append(T.random_recording(rng, n, nt, n_spk=int(rng.integers(1, 9)), span=int(rng.integers(20, 260)), n_hyp=int(rng.integers(1, 8)),
                                       n_uem=int(rng.integers(1, 4)) if k % 4 == 0 else 0))
    return recs


@pytest.mark.parametrize("collar", [0, 1, 7])
def test_200_seeded_recordings_in_one_call(eng, seeded, collar):
    counts, mp = _check(eng, seeded, "200 recordings, collar %d" % collar, collar, collar == 1, want_map=True)
    assert counts[:, 0].sum() > 0 and (collar > 0 or (counts[:, 3] > 0).sum() > 20)      # (confusion does occur)
    for q in (0, 1, 2, 57, 128, 199):                                     # alone = in the batch
        c1, m1 = _run(eng, T.pack([seeded[q]]), collar, T.SKIP_OVERLAP if collar == 1 else 0)
        assert np.array_equal(c1[0], counts[q]) and np.array_equal(m1[0], mp[q]), "recording %d" % q
    for q in range(0, 200, 9):
        T.check_map(mp[q], seeded[q], collar, collar == 1)


# ------------------------------------------------------------------------------------------- event-sort classes, limits
def _sized(rng, nt, n, nu=0, span=None):
    return T.random_recording(rng, n, nt, n_spk=64 if nt > 2000 else 8, span=span or 40 * (nt + n) + 100, n_hyp=50, n_uem=nu)


def test_plan_names_the_classes(eng):
    from plda_amd import der
    top = der.plan_timed(eng, 0, 1)["lds_max"]
    assert top == 16384
    nt = (top - 2 * 60) // 2
    assert der.plan_timed(eng, nt, 60) == {"cls": 0, "scratch_bytes": 0, "lds_max": top, "events": top}
    assert der.plan_timed(eng, nt + 1, 60) == {"cls": 1, "scratch_bytes": 8 * 2 * top, "lds_max": top, "events": top + 2}
    assert der.plan_timed(eng, 16384, 4096, 1024, 25) == {"cls": 1, "scratch_bytes": 1 << 20, "lds_max": top, "events": 6 * 16384 + 8192 + 2048}
    assert der.plan_timed(eng, 0, 0)["cls"] == 0
    out = (C.c_int32 * 3)()
    for bad in ((16385, 1, 0, 0), (1, 4097, 0, 0), (1, 1, 1025, 0), (1, 1, 0, -1), (1, 1, 0, (1 << 20) + 1), (-1, 1, 0, 0)):
        assert _lib().plda_der_timed_plan(eng._h, *bad, out) == E_INVAL


def test_both_classes_at_the_boundary(eng):
    """Event counts are even (2 or 6 per turn, 2 per segment and interval): the largest count of the LDS class and its two
    neighbours on either side are top - 2, top, top + 2."""
    from plda_amd import der
    top = der.plan_timed(eng, 0, 1)["lds_max"]
    rng = np.random.default_rng(31)
    recs = [_sized(rng, (top - 120) // 2 + d, 60) for d in (-1, 0, 1)]
    assert [der.plan_timed(eng, len(r["ts"]), 60)["cls"] for r in recs] == [0, 0, 1]
    _check(eng, recs, "boundary, collar 0", 0, model=T.score_atoms)
    recs = [_sized(rng, (top - 120 - 4) // 6 + d, 60, 2) for d in (0, 1)]                # 6 events per turn: top and top + 6
    assert [der.plan_timed(eng, len(r["ts"]), 60, 2, 9)["cls"] for r in recs] == [0, 1]
    _check(eng, recs, "boundary, collar 9", 9, model=T.score_atoms)


@pytest.mark.parametrize("limit", ["turns", "segments", "uem"])
def test_the_limits(eng, limit):
    rng = np.random.default_rng(32)
    nt, n, nu = {"turns": (16384, 50, 0), "segments": (300, 4096, 0), "uem": (300, 50, 1024)}[limit]
    r = _sized(rng, nt, n, nu, span=900000 if limit == "turns" else None)
    _check(eng, [r], "limit of %s" % limit, 25, model=T.score_atoms)
    turns, ss, sd, hyp, off, uem = T.pack([r])
    if limit == "turns":
        more = tuple(np.concatenate([a, a[:1]]) for a in turns[:3]) + (np.asarray([0, nt + 1]),)
        assert _run(eng, (more, ss, sd, hyp, off, uem), expect=E_INVAL) == E_INVAL and "PLDA_DER_MAX_TURNS" in _last(eng)
    if limit == "uem":
        more = (np.concatenate([uem[0], uem[0][:1]]), np.concatenate([uem[1], uem[1][:1]]), np.asarray([0, nu + 1]))
        assert _run(eng, (turns, ss, sd, hyp, off, more), expect=E_INVAL) == E_INVAL and "PLDA_DER_MAX_UEM" in _last(eng)


def test_sums_beyond_32_bits(eng):
    """64 speakers talking over each other for 2^30 ticks under one hypothesis segment: speech = 2^36"""
    r = T.rec(ts=np.zeros(64), td=np.full(64, 1 << 30), tk=np.arange(64), ss=[0], sd=[1 << 30], hyp=[4095])
    counts, mp = _check(eng, [r], "2^36", 0, model=T.score_atoms, want_map=True)
    assert counts[0].tolist() == [1 << 36, 63 << 30, 0, 0] and (mp[0] >= 0).sum() == 1
    counts, _ = _check(eng, [r], "2^36 under the largest collar", 1 << 20, model=T.score_atoms)
    assert counts[0, 0] == 64 * ((1 << 30) - (1 << 21))


def test_several_launches_equal_one(monkeypatch, eng):
    """six scratch-class recordings of 65536 key slots (512 KiB each, collar 3: six events a turn): a budget of 1 MiB sorts
    them two to a launch, the default budget all in one; the results are equal, and the small handle holds 2 MiB less"""
    from plda_amd import MPlda, der
    rng = np.random.default_rng(33)
    recs = [_sized(rng, 8200 + 10 * k, 30) for k in range(6)] + [_sized(rng, 40, 20), _sized(rng, 3000, 100, 5)]
    assert all(der.plan_timed(eng, len(r["ts"]), 30, 0, 3)["scratch_bytes"] == 512 << 10 for r in recs[:6])
    packed = T.pack(recs)
    monkeypatch.setenv("PLDA_DER_SCRATCH_BYTES", str(1 << 20))
    small = MPlda(0)
    monkeypatch.delenv("PLDA_DER_SCRATCH_BYTES")
    fresh = MPlda(0)
    held = _lib().plda_device_bytes_held()
    c_small, m_small = _run(small, packed, 3)
    d_small = _lib().plda_device_bytes_held() - held
    c_one, m_one = _run(fresh, packed, 3)
    d_one = _lib().plda_device_bytes_held() - held - d_small
    assert d_one - d_small >= 2 << 20, (d_small, d_one)                   # (3 MiB of keys in flight against 1 MiB)
    assert np.array_equal(c_small, c_one) and np.array_equal(m_small, m_one)
    assert np.array_equal(c_one, T.counts(recs, 3, False, T.score_atoms))


# ------------------------------------------------------------------------------------------- host forms, sweep, tune_threshold
def test_host_forms_equal_device_forms(eng, seeded):
    from liblda.plda import PLDA
    from plda_amd import der
    recs = seeded[:40]
    packed = T.pack(recs)
    turns, ss, sd, hyp, off, uem = packed
    counts, mp = _run(eng, packed, 2, T.SKIP_OVERLAP)
    res = der.der_timed(eng, turns, ss, sd, hyp, off, 2, uem, True, return_map=True)
    assert res.counts.dtype == np.int64 and np.array_equal(res.counts, counts) and np.array_equal(res.map, mp)
    res2 = eng.der_timed(tuple(a.tolist() for a in turns), ss.astype(np.int64), sd.tolist(), hyp, off.tolist(), collar=2, uem=uem, skip_overlap=True)
    assert np.array_equal(res2.counts, counts) and res2.map is None
    assert np.array_equal(PLDA(0).der_timed(turns, ss, sd, hyp, off, 2, uem, True).counts, counts)
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    d = [dev(a) for a in (turns[0], turns[1], turns[2], ss, sd, hyp, uem[0], uem[1])]
    out = torch.zeros((len(off) - 1, 4), dtype=torch.int64, device="cuda")
    eng.der_timed_dev([x.data_ptr() for x in d[:3]], turns[3], d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), off, out.data_ptr(),
                      duem=(d[6].data_ptr(), d[7].data_ptr()), uem_off=uem[2], collar=2, flags=1)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), counts)


@pytest.fixture(scope="module")
def sweep_case(eng):
    """six planted-speaker blocks, their full merge records, segments on a time line, overlapping reference turns"""
    from plda_amd import diarize
    rng = np.random.default_rng(51)
    blocks, recs = [], []
    for q, sizes in enumerate(([1], [9, 14, 17], [5, 5], [3, 3, 3, 3], [2], [20, 30, 10])):
        S, g = M.planted_block(sizes, 60 + q, noise=0.6)
        blocks.append(S)
        n = len(g)
        dur = rng.integers(0, 30, n).astype(np.int32)
        start = np.concatenate([[0], np.cumsum(dur + rng.integers(0, 4, n))[:-1]]).astype(np.int32)
        ts, td, tk = list(start), list(dur + rng.integers(0, 6, n)), list(g)          # the planted speaker, running on a little
        merged = {}
        for s, d, k in sorted(zip(ts, td, tk)):                                        # (per-speaker disjoint: merge what runs on)
            runs = merged.setdefault(int(k), [])
            if runs and s <= runs[-1][1]:
                runs[-1][1] = max(runs[-1][1], int(s + d))
            else:
                runs.append([int(s), int(s + d)])
        turns = [(a, b - a, k) for k, runs in merged.items() for a, b in runs] + [(int(start[n // 2]), 40, 63)]   # + one who talks over
        recs.append(T.rec([t[0] for t in turns], [t[1] for t in turns], [t[2] for t in turns], start, dur, np.zeros(n)))
    _, ncl, merges = diarize.ahc(eng, blocks, None, 1, return_merges=True)
    assert (ncl == 1).all()
    cost = np.sort(merges[2])
    thresholds = np.asarray([-cost[len(cost) // 2], -cost[-1] - 1.0, 0.0, -cost[0] + 1.0, -cost[len(cost) // 3]], np.float64)
    return recs, merges, thresholds


@pytest.mark.parametrize("num_speakers", [None, [1, 5, 2, 12, 2, 3]])
def test_sweep_equals_cut_then_der_timed(eng, sweep_case, num_speakers):
    from plda_amd import der, diarize
    recs, merges, thresholds = sweep_case
    packed = T.pack(recs)
    turns, ss, sd, _, off, _ = packed
    counts, ncl = _run_sweep(eng, merges, packed, thresholds, num_speakers, collar=2)
    assert counts.shape == (5, 6, 4)
    for q, thr in enumerate(thresholds):
        labels, k = diarize.cut(merges, off, float(thr), num_speakers)
        assert np.array_equal(ncl[q], k), "n_clusters at threshold %d" % q
        assert np.array_equal(counts[q], _run(eng, (turns, ss, sd, labels, off, None), 2, want_map=False)[0]), "threshold %d" % q
        cut = [dict(r, hyp=labels[off[i]:off[i + 1]]) for i, r in enumerate(recs)]
        assert np.array_equal(counts[q], T.counts(cut, 2)), "threshold %d against the tick model" % q
    assert len({tuple(k) for k in ncl.tolist()}) >= 3
    res = der.sweep_timed(eng, merges, turns, ss, sd, off, thresholds, num_speakers, collar=2)
    assert np.array_equal(res.counts, counts) and np.array_equal(res.n_clusters, ncl) and res.best == der.best_index(counts)


def test_tune_threshold_with_turns_equals_cluster_then_sweep_timed():
    from liblda.plda import PLDA
    from plda_amd import der, diarize
    from test_gpu_der import _model_params
    d, sizes = 16, (4, 9, 14)
    mean, Tm, psi = _model_params(d, 11, psi_scale=4.0)
    p = PLDA(0)
    e = p._instance
    e.set_model(mean, Tm, psi)
    rng = np.random.default_rng(12)
    rows, recs = [], []
    for _ in range(4):
        g = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
        y = rng.standard_normal((len(sizes), d)) * np.sqrt(psi)
        rows.append(mean + (y[g] + rng.standard_normal((len(g), d))) @ np.linalg.inv(Tm).T)
        start = (np.arange(len(g)) * 10).astype(np.int32)
        recs.append(T.rec(list(start) + [35], [10] * len(g) + [60], list(g) + [40], start, np.full(len(g), 10), np.zeros(len(g))))
    x = np.concatenate(rows)
    turns, ss, sd, _, off, _ = T.pack(recs)
    thresholds = np.asarray([-40.0, -10.0, -3.0, 0.0, 3.0, 10.0, 40.0])
    best, res = p.tune_threshold(x, off, None, thresholds, turns=turns, seg_start=ss, seg_dur=sd, collar=1)
    _, _, merges = p.cluster(x, off, threshold=None, num_speakers=1, return_merges=True)
    hand = der.sweep_timed(e, merges, turns, ss, sd, off, thresholds, collar=1)
    assert np.array_equal(res.counts, hand.counts) and np.array_equal(res.n_clusters, hand.n_clusters) and res.best == hand.best
    assert best == thresholds[hand.best] and len(set(res.der.tolist())) > 2
    for q, thr in enumerate(thresholds):
        labels, ncl = p.cluster(x, off, threshold=float(thr))
        assert np.array_equal(p.der_timed(turns, ss, sd, labels, off, collar=1).counts, res.counts[q]), "threshold %d" % q
    with pytest.raises(ValueError):
        p.tune_threshold(x, off, np.zeros(len(x), np.int32), thresholds, turns=turns, seg_start=ss, seg_dur=sd)
    with pytest.raises(ValueError):
        p.tune_threshold(x, off, None, thresholds, turns=turns, seg_start=ss[:-1], seg_dur=sd)


# ------------------------------------------------------------------------------------------- errors
def _base():
    return T.pack([T.rec([0, 5, 20], [10, 10, 5], [0, 1, 0], [0, 15], [15, 10], [3, 4]), T.rec([1], [4], [2], [0], [9], [0])])


def _put(packed, where, k, v):
    """a copy of the packed call with entry k of array `where` = (group, index) set to v"""
    out = [list(packed[0]), packed[1], packed[2], packed[3], packed[4], packed[5]]
    grp, idx = where
    if grp == "turns":
        a = np.array(out[0][idx]); a[k] = v; out[0][idx] = a
    else:
        a = np.array(out[idx]); a[k] = v; out[idx] = a
    out[0] = tuple(out[0])
    return tuple(out)


def test_every_violation_fails_with_its_count_and_writes_nothing(eng):
    base = _base()
    want = T.counts([T.rec([0, 5, 20], [10, 10, 5], [0, 1, 0], [0, 15], [15, 10], [3, 4]), T.rec([1], [4], [2], [0], [9], [0])])
    assert np.array_equal(_run(eng, base)[0], want)
    entries = [(("turns", 2), 1, 64), (("turns", 2), 0, -1), (("turns", 0), 3, -1), (("turns", 1), 2, -1), (("turns", 1), 0, (1 << 30) + 1),
               (("turns", 0), 1, (1 << 30) - 5), (("seg", 1), 0, -3), (("seg", 2), 1, -1), (("seg", 2), 2, (1 << 30) + 1), (("seg", 3), 0, 4096),
               (("seg", 3), 2, -2)]
    for where, k, v in entries:
        assert _run(eng, _put(base, where, k, v), expect=E_INVAL) == E_INVAL
        assert "1 invalid entries" in _last(eng) and "0 invalid events" in _last(eng), (where, k, v, _last(eng))
    two = _put(_put(base, ("turns", 2), 1, 99), ("seg", 3), 1, 5000)
    assert _run(eng, two, collar=3, expect=E_INVAL) == E_INVAL and "2 invalid entries" in _last(eng)
    uem = (np.asarray([0, 5], np.int32), np.asarray([9, -1], np.int32), np.asarray([0, 1, 2]))
    assert _run(eng, base[:5] + (uem,), expect=E_INVAL) == E_INVAL and "1 invalid entries" in _last(eng)
    # a turn of speaker 0 that starts inside the first one: its start finds the speaker talking, the first end then finds
    # them silent -- two events
    inside = _put(_put(base, ("turns", 0), 2, 4), ("turns", 1), 2, 3)
    assert _run(eng, inside, expect=E_INVAL) == E_INVAL and "0 invalid entries" in _last(eng) and "2 invalid events" in _last(eng)
    assert _run(eng, inside, collar=2, flags=1, expect=E_INVAL) == E_INVAL
    shared = _put(base, ("seg", 1), 1, 14)                                # segment 1 starts on the last tick of segment 0
    assert _run(eng, shared, expect=E_INVAL) == E_INVAL and "1 invalid events" in _last(eng)
    assert np.array_equal(_run(eng, _put(base, ("seg", 1), 1, 15))[0], want)
    # the host's checks, before any device work
    for arr, bad in (("turn_off", [0, 4, 3]), ("turn_off", [1, 3, 4]), ("offsets", [0, 2, 2]), ("offsets", [0, 3, 2])):
        call = (base[0][:3] + (np.asarray(bad),),) + base[1:] if arr == "turn_off" else base[:4] + (np.asarray(bad), None)
        assert _run(eng, call, expect=E_INVAL) == E_INVAL and arr.split("_")[0] in _last(eng)
    assert _run(eng, base[:5] + ((np.zeros(2, np.int32), np.ones(2, np.int32), np.asarray([0, 2, 1])),), expect=E_INVAL) == E_INVAL
    assert "uem_off" in _last(eng)
    assert _run(eng, base, collar=-1, expect=E_INVAL) == E_INVAL and "collar" in _last(eng)
    assert _run(eng, base, collar=(1 << 20) + 1, expect=E_INVAL) == E_INVAL
    assert _run(eng, base, flags=2, expect=E_INVAL) == E_INVAL and "flags" in _last(eng)
    merges = (np.asarray([0], np.int32), np.asarray([1], np.int32), np.asarray([-1.0]))
    assert _run_sweep(eng, merges, base, [0.0, float("nan")], expect=E_INVAL) == E_INVAL and "NaN" in _last(eng)
    assert _run_sweep(eng, merges, base, [], expect=E_INVAL) == E_INVAL
    assert _run_sweep(eng, merges, inside, [0.0], expect=E_INVAL) == E_INVAL and "2 invalid events" in _last(eng)
    assert _run_sweep(eng, (merges[0], np.asarray([7], np.int32), merges[2]), base, [1e9, 0.0], expect=E_INVAL) == E_INVAL
    assert "not a full record" in _last(eng)
    assert np.array_equal(_run(eng, base)[0], want)                       # the handle works as before


def test_null_arguments_are_refused_by_name(eng):
    import torch
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = _vp(buf.data_ptr())
    off, toff = np.asarray([0, 1], np.int64), np.asarray([0, 1], np.int64)
    thr = np.zeros(1)
    lib = _lib()
    names = ["turn_start", "turn_dur", "turn_spk", "turn_off", "seg_start", "seg_dur", "hyp", "offsets"]
    good = [p, p, p, _hp(toff), p, p, p, _hp(off)]
    texts = {"turn_start": "turn_start, turn_dur or turn_spk is NULL", "turn_dur": "turn_start, turn_dur or turn_spk is NULL",
             "turn_spk": "turn_start, turn_dur or turn_spk is NULL"}
    for k, name in enumerate(names):
        args = list(good)
        args[k] = None
        assert lib.plda_der_timed_dev(eng._h, *args, 1, None, None, None, 0, 0, p, None) == E_INVAL
        assert _last(eng) == "der_timed: " + texts.get(name, name + " is NULL"), name
    assert lib.plda_der_timed_dev(eng._h, *good, 1, None, None, None, 0, 0, None, None) == E_INVAL and _last(eng) == "der_timed: counts is NULL"
    assert lib.plda_der_timed_dev(eng._h, *good, 1, p, p, None, 0, 0, p, None) == E_INVAL and _last(eng) == "der_timed: uem_off is NULL"
    assert lib.plda_der_timed_dev(eng._h, *good, 1, None, p, _hp(toff), 0, 0, p, None) == E_INVAL
    assert _last(eng) == "der_timed: uem_start or uem_dur is NULL"
    assert lib.plda_der_timed_dev(None, *good, 1, None, None, None, 0, 0, p, None) == E_INVAL
    sweep = lambda counts, ncl, thresholds: lib.plda_der_timed_sweep_dev(eng._h, None, None, None, p, p, p, _hp(toff), p, p, _hp(off), 1, None,
                                                                         None, None, 0, 0, thresholds, 1, None, counts, ncl)
    assert sweep(p, None, _hp(thr)) == E_INVAL and _last(eng) == "der_timed_sweep: n_clusters is NULL"
    assert sweep(None, p, _hp(thr)) == E_INVAL and _last(eng) == "der_timed_sweep: counts is NULL"
    assert sweep(p, p, None) == E_INVAL and _last(eng) == "der_timed_sweep: thresholds is NULL"
    off2 = np.asarray([0, 2], np.int64)
    assert lib.plda_der_timed_sweep_dev(eng._h, None, p, p, p, p, p, _hp(toff), p, p, _hp(off2), 1, None, None, None, 0, 0, _hp(thr), 1, None, p,
                                        p) == E_INVAL and _last(eng) == "der_timed_sweep: merge_a, merge_b or merge_cost is NULL"
    host = np.zeros(8, np.int32)
    hp = _hp(host)
    cnt = np.zeros(4, np.int64)
    assert lib.plda_der_timed(eng._h, hp, hp, hp, _hp(toff), hp, None, hp, _hp(off), 1, None, None, None, 0, 0, _hp(cnt), None) == E_INVAL
    assert _last(eng) == "der_timed: seg_dur is NULL"
