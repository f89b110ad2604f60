"""GPU: the time-based diarisation error rate with two hypothesis labels per segment (plda_der_timed_ovl[_dev]; csrc/der_time.hip,
the OVL form of csrc/der.hip's solve) against its host model (tests/der_overlap_model.py).  The contract is exact: every
comparison of counts is ==.

Every device call goes through _run2: inputs between -1 neighbours, outputs between guard bands filled with a payload that must
stay intact outside the output and be gone inside it (the helpers of test_gpu_der and test_gpu_der_time)."""
import numpy as np
import pytest

import der_model as M
import der_overlap_model as O
import der_time_model as T
from test_gpu_der import E_INVAL, _guarded_input, _hp, _lib, _Out, _vp
from test_gpu_der_time import _inputs, _last, _ptr, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from plda_amd import MPlda
    return MPlda(0)


def _run2(eng, packed, collar=0, flags=0, want_map=True, expect=0, null_hyp2=False):
    """plda_der_timed_ovl_dev on guarded buffers; packed = der_overlap_model.pack's tuple -> (counts int64 [R, 4], map int32
    [R, 64] or None), or the status"""
    import torch
    turns, ss, sd, hyp, off, uem, hyp2 = packed
    r = len(off) - 1
    keep, ukeep = _inputs(turns, ss, sd, uem)
    khyp, khyp2 = _guarded_input(np.asarray(hyp, np.int32)), _guarded_input(np.asarray(hyp2, np.int32))
    oC, oM = _Out(r * 4, torch.int64), _Out(r * M.MAX_REF, torch.int32)
    torch.cuda.synchronize()
    rc = _lib().plda_der_timed_ovl_dev(eng._h, _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), _hp(np.ascontiguousarray(turns[3], np.int64)),
                                       _ptr(keep[3]), _ptr(keep[4]), _ptr(khyp), None if null_hyp2 else _ptr(khyp2),
                                       _hp(np.ascontiguousarray(off, np.int64)), r, _ptr(ukeep[0]) if uem is not None else None,
                                       _ptr(ukeep[1]) if uem is not None else None,
                                       _hp(np.ascontiguousarray(uem[2], np.int64)) if uem is not None else None, collar, flags,
                                       _vp(oC.ptr()), _vp(oM.ptr()) if want_map else None)
    torch.cuda.synchronize()
    assert rc == expect, "status %d: %s" % (rc, _last(eng))
    if expect:
        oC.check("counts", written=False)
        oM.check("map", written=False)
        return rc
    counts = oC.check("counts").reshape(r, 4)
    if want_map:
        return counts, oM.check("map").reshape(r, M.MAX_REF)
    oM.check("map", written=False)
    return counts, None


# ------------------------------------------------------------------------------------------- the definition
EXAMPLES = [([0, 5, 10], [5, 5, 5], [3, 3, 8], [-1, 8, -1], [20, 0, 0, 0]),
            ([0], [15], [3], [8], [20, 0, 10, 0]),
            ([0], [15], [3], [-1], [20, 5, 0, 5])]


@pytest.mark.parametrize("ss, sd, hyp, hyp2, want", EXAMPLES)
def test_header_examples_from_the_public_interface(ss, sd, hyp, hyp2, want):
    from liblda.plda import PLDA
    r = O.rec(ts=[0, 5], td=[10, 10], tk=[0, 1], ss=ss, sd=sd, hyp=hyp, hyp2=hyp2)
    assert O.score_ticks(r)[0] == want
    turns, ss, sd, hyp, off, _, hyp2 = O.pack([r])
    res = PLDA(0).der_timed(turns, ss, sd, hyp, off, hyp2=hyp2, return_map=True)
    assert res.counts.tolist() == [want]
    O.check_map(res.map[0], r)


@pytest.fixture(scope="module")
def seeded():
    """80 seeded recordings with a second label on about 20 % of the segments, and their model counts at three settings:
    computed once, left unchanged"""
    rng = np.random.default_rng(2121)
    recs = []
    for k in range(80):
        n, nt = (1, 0) if k == 0 else (40, 50) if k == 1 else (int(rng.integers(1, 41)), int(rng.integers(0, 51)))
        recs.append(O.random_recording(rng, n, nt, n_spk=int(rng.integers(1, 9)), span=int(rng.integers(20, 260)), n_hyp=int(rng.integers(1, 8)),
                                       n_uem=int(rng.integers(1, 4)) if k % 4 == 0 else 0))
    want = {(collar, skip): O.counts(recs, collar, skip) for collar, skip in ((0, False), (1, True), (7, False))}
    return recs, want


@pytest.mark.parametrize("collar, skip", [(0, False), (1, True), (7, False)])
def test_seeded_recordings_in_one_call(eng, seeded, collar, skip):
    recs, want = seeded
    flags = T.SKIP_OVERLAP if skip else 0
    counts, mp = _run2(eng, O.pack(recs), collar, flags)
    assert np.array_equal(counts, want[collar, skip]), "counts\n%r\nmodel\n%r" % (counts[:8], want[collar, skip][:8])
    second = sum(int((r["hyp2"] >= 0).sum()) for r in recs) / sum(int((r["hyp"] >= 0).sum()) for r in recs)
    assert 0.1 < second < 0.3 and (counts >= 0).all()
    if collar == 0:
        assert (counts[:, 3] > 0).sum() > 10 and (counts[:, 2] > 0).sum() > 10
    for q in range(0, 80, 7):
        O.check_map(mp[q], recs[q], collar, skip)
    for q in (0, 1, 2, 33, 79):                                           # alone = in the batch
        c1, m1 = _run2(eng, O.pack([recs[q]]), collar, flags)
        assert np.array_equal(c1[0], counts[q]) and np.array_equal(m1[0], mp[q]), "recording %d" % q


def test_no_second_label_equals_der_timed(eng, seeded):
    recs, _ = seeded
    packed = O.pack(recs)
    base_c, base_m = _run(eng, packed[:6], 2, T.SKIP_OVERLAP)               # plda_der_timed_dev
    c, m = _run2(eng, packed, 2, T.SKIP_OVERLAP, null_hyp2=True)
    assert np.array_equal(c, base_c) and np.array_equal(m, base_m)
    none = packed[:6] + (np.full(len(packed[3]), -1, np.int32),)
    c, m = _run2(eng, none, 2, T.SKIP_OVERLAP)
    assert np.array_equal(c, base_c) and np.array_equal(m, base_m)
    c, m = _run2(eng, none, 2, T.SKIP_OVERLAP, want_map=False)
    assert np.array_equal(c, base_c) and m is None


# ------------------------------------------------------------------------------------------- classes
def _scratch_events(eng):
    """a recording at the smallest segment count of the scratch event class, at 2600 turns under a collar (6 events a turn)"""
    from plda_amd import der
    nt, collar = 2600, 3
    top = der.plan_timed(eng, 0, 1)["lds_max"]
    n = (top - 6 * nt) // 2 + 1
    assert der.plan_timed(eng, nt, n, 0, collar)["cls"] == 1 and der.plan_timed(eng, nt, n - 1, 0, collar)["cls"] == 0
    rng = np.random.default_rng(61)
    return O.random_recording(rng, n, nt, n_spk=8, span=40 * (nt + n), n_hyp=50), collar


def _hbm_matrix(eng):
    """a recording whose matrix (40 reference speakers, more than 500 hypothesis labels over both arrays) takes the scratch class"""
    from plda_amd import der
    rng = np.random.default_rng(62)
    r = O.random_recording(rng, 2500, 400, n_spk=40, span=100000, n_hyp=520, p_ns=0.05)
    _, _, rl, hl = O.score_atoms(r)
    assert len(rl) == 40 and len(hl) > 500
    assert der.plan(eng, len(rl), len(hl))["cls"] == 1 and der.plan(eng, len(rl), 40)["cls"] == 0
    return r


@pytest.fixture(scope="module")
def classes(eng):
    big, collar = _scratch_events(eng)
    rng = np.random.default_rng(63)
    recs = [O.random_recording(rng, 30, 40, n_spk=5, span=400, n_hyp=6), big, _hbm_matrix(eng), O.random_recording(rng, 1, 0, n_hyp=2),
            O.random_recording(rng, 12, 9, n_spk=3, span=90, n_hyp=3, n_uem=2)]
    return recs, collar, O.counts(recs, collar)


def test_scratch_event_class_and_hbm_matrix_class(eng, classes):
    recs, collar, want = classes
    for q in (1, 2):
        counts, mp = _run2(eng, O.pack([recs[q]]), collar)
        assert np.array_equal(counts[0], want[q]), (q, counts, want[q])
        O.check_map(mp[0], recs[q], collar)
        assert (recs[q]["hyp2"] >= 0).sum() > 50 and counts[0, 0] > 0


def test_mixed_classes_in_one_call_equal_each_alone(eng, classes):
    recs, collar, want = classes
    counts, mp = _run2(eng, O.pack(recs), collar)
    assert np.array_equal(counts, want)
    for q, r in enumerate(recs):
        c1, m1 = _run2(eng, O.pack([r]), collar)
        assert np.array_equal(c1[0], counts[q]) and np.array_equal(m1[0], mp[q]), "recording %d" % q


# ------------------------------------------------------------------------------------------- errors
def test_every_entry_violation_is_counted_and_writes_nothing(eng):
    good = [O.rec([0, 5, 20], [10, 10, 5], [0, 1, 0], [0, 15, 30], [15, 10, 4], [3, 4, -1], [4, -1, -1]), O.rec([1], [4], [2], [0], [9], [0], [-1])]
    want = O.counts(good)
    packed = O.pack(good)
    assert np.array_equal(_run2(eng, packed)[0], want)

    def put(**at):
        h, h2 = np.array(packed[3]), np.array(packed[6])
        for k, v in at.get("hyp", {}).items():
            h[k] = v
        for k, v in at.get("hyp2", {}).items():
            h2[k] = v
        return packed[:3] + (h,) + packed[4:6] + (h2,)
    kinds = {"below -1": put(hyp2={1: -2}), "at PLDA_AHC_MAX": put(hyp2={1: 4096}), "a second label without a first": put(hyp2={2: 5}),
             "equal to the first": put(hyp2={0: 3}), "equal to the first, last recording": put(hyp2={3: 0}),
             "the first label taken away": put(hyp={0: -1})}
    for kind, call in kinds.items():
        assert _run2(eng, call, expect=E_INVAL) == E_INVAL, kind
        assert "1 invalid entries" in _last(eng) and "0 invalid events" in _last(eng) and "second label" in _last(eng), (kind, _last(eng))
    assert _run2(eng, put(hyp2={1: -2, 2: 5, 3: 4096}), collar=2, expect=E_INVAL) == E_INVAL and "3 invalid entries" in _last(eng)
    assert _run2(eng, put(hyp={1: 4096}), expect=E_INVAL) == E_INVAL and "1 invalid entries" in _last(eng)          # hyp's own range
    shared = packed[:1] + (np.asarray([0, 14, 30, 0], np.int32),) + packed[2:]
    assert _run2(eng, shared, expect=E_INVAL) == E_INVAL and "1 invalid events" in _last(eng)    # segments stay disjoint
    assert np.array_equal(_run2(eng, packed)[0], want)                     # the handle works as before


def test_null_arguments_and_host_checks(eng):
    import torch
    p = _vp(torch.zeros(64, dtype=torch.int64, device="cuda").data_ptr())
    off = np.asarray([0, 1], np.int64)
    lib = _lib()
    assert lib.plda_der_timed_ovl_dev(eng._h, p, p, p, _hp(off), p, p, None, p, _hp(off), 1, None, None, None, 0, 0, p, None) == E_INVAL
    assert _last(eng) == "der_timed_ovl: hyp is NULL"
    assert lib.plda_der_timed_ovl_dev(eng._h, p, p, p, _hp(off), p, p, p, p, _hp(off), 1, None, None, None, 0, 0, None, None) == E_INVAL
    assert _last(eng) == "der_timed_ovl: counts is NULL"
    assert lib.plda_der_timed_ovl_dev(eng._h, p, p, p, _hp(off), p, p, p, p, _hp(off), 1, None, None, None, 0, 4, p, None) == E_INVAL
    assert "flags" in _last(eng)


def test_host_forms_equal_the_device_form(eng, seeded):
    import torch
    from liblda.plda import PLDA
    from plda_amd import der
    recs, want = seeded
    turns, ss, sd, hyp, off, uem, hyp2 = O.pack(recs[:30])
    counts, mp = _run2(eng, O.pack(recs[:30]), 2, T.SKIP_OVERLAP)
    res = der.der_timed(eng, turns, ss, sd, hyp, off, 2, uem, True, return_map=True, hyp2=hyp2)
    assert res.counts.dtype == np.int64 and np.array_equal(res.counts, counts) and np.array_equal(res.map, mp)
    res = PLDA(0).der_timed(turns, ss, sd, hyp.tolist(), off, 2, uem, True, hyp2=hyp2.astype(np.int64))
    assert np.array_equal(res.counts, counts) and res.map is None
    with pytest.raises(ValueError):
        eng.der_timed(turns, ss, sd, hyp, off, hyp2=hyp)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    d = [dev(a) for a in (turns[0], turns[1], turns[2], ss, sd, hyp, hyp2, uem[0], uem[1])]
    out = torch.zeros((len(off) - 1, 4), dtype=torch.int64, device="cuda")
    eng.der_timed_ovl_dev([x.data_ptr() for x in d[:3]], turns[3], d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), off,
                          out.data_ptr(), duem=(d[7].data_ptr(), d[8].data_ptr()), uem_off=uem[2], collar=2, flags=1)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), counts)


# ------------------------------------------------------------------------------------------- the pipeline
def test_diarize_with_a_posterior_floor_then_der_timed():
    """planted two-speaker overlap: segments of speaker 0, of speaker 1 and of both at once (the mean of their vectors).  Only
    what the definition guarantees is asserted: a second label cannot raise the miss and does not change the speech."""
    from liblda.plda import PLDA
    from test_gpu_der import _model_params
    d = 16
    mean, Tm, psi = _model_params(d, 11, psi_scale=4.0)
    p = PLDA(0)
    p._instance.set_model(mean, Tm, psi)
    rng = np.random.default_rng(14)
    rows, recs = [], []
    for _ in range(3):
        g = rng.permutation(np.repeat([0, 1, 2], [14, 12, 8]))            # 2: both speakers
        y = rng.standard_normal((2, d)) * np.sqrt(psi)
        centre = np.where((g == 2)[:, None], 0.5 * (y[0] + y[1]), y[np.minimum(g, 1)])
        rows.append(mean + (centre + rng.standard_normal((len(g), d))) @ np.linalg.inv(Tm).T)
        start = (np.arange(len(g)) * 10).astype(np.int32)
        ts = np.concatenate([start[g != 1], start[g != 0]])
        tk = np.concatenate([np.zeros((g != 1).sum()), np.ones((g != 0).sum())])
        recs.append(T.rec(ts, np.full(len(ts), 10), tk, start, np.full(len(g), 10), np.zeros(len(g))))
    x = np.concatenate(rows)
    turns, ss, sd, _, off, _ = T.pack(recs)
    vbx = dict(Fa=1.0, Fb=1.0, loop_prob=0.9)                             # (the defaults collapse so short a recording to one speaker)
    labels, ncl, labels2 = p.diarize(x, off, threshold=0.0, min_posterior=1e-3, **vbx)
    plain = p.diarize(x, off, threshold=0.0, **vbx)
    assert len(plain) == 2 and np.array_equal(plain[0], labels) and np.array_equal(plain[1], ncl)
    assert labels2.dtype == np.int32 and labels2.shape == labels.shape and ((labels2 == -1) | ((labels2 >= 0) & (labels2 != labels))).all()
    one = p.der_timed(turns, ss, sd, labels, off).counts
    two = p.der_timed(turns, ss, sd, labels, off, hyp2=labels2).counts
    print("one label %r\ntwo labels %r\nsecond labels kept: %d of %d" % (one.tolist(), two.tolist(), int((labels2 >= 0).sum()), len(labels2)))
    assert np.array_equal(two[:, 0], one[:, 0]) and (two[:, 1] <= one[:, 1]).all()
    with pytest.raises(ValueError):
        p.diarize(x, off, threshold=0.0, min_posterior=0.1, return_posteriors=True)
    mask = np.zeros(len(labels), bool)
    mask[::3] = True
    by_mask = p.diarize(x, off, threshold=0.0, overlap=mask, **vbx)[2]
    assert (by_mask[~mask] == -1).all() and np.array_equal(by_mask[mask] >= 0, np.repeat(ncl, np.diff(off))[mask] > 1)
