"""GPU: the Jaccard error rate and the per-speaker figures (plda_der_jer*, plda_der_timed_jer*; the JER form of csrc/der.hip's
solve) against the host model (tests/jer_model.py).  The contract is exact: jer, counts and spk are compared with ==; jmap,
which is not canonical among equal optima, is checked for its laws (jer_model.check_outputs).

Every device call goes through _timed / _seg / _sweep_*: inputs between -1 neighbours, outputs between guard bands filled with
a payload that must stay intact outside the output and be gone inside it (the helpers of test_gpu_der and test_gpu_der_time)."""
import math

import numpy as np
import pytest

import der_model as M
import der_overlap_model as O
import der_time_model as T
import jer_model as J
from test_gpu_der import E_INVAL, _guarded_input, _hp, _lib, _Out, _vp
from test_gpu_der import _run as _der_dev, _run_sweep as _der_sweep_dev
from test_gpu_der_overlap import _run2 as _ovl_dev
from test_gpu_der_time import _inputs, _last, _ptr, _run_sweep as _timed_sweep_dev
from test_gpu_der_time import sweep_case  # noqa: F401  (a fixture: six planted recordings, their merge records, thresholds)

pytestmark = pytest.mark.gpu
R64 = M.MAX_REF


@pytest.fixture(scope="module")
def eng():
    from plda_amd import MPlda
    return MPlda(0)


class _JerOut:
    def __init__(self, rows, maps=None, want_jmap=True, want_spk=True):
        import torch
        self.rows, self.maps = rows, rows if maps is None else maps
        self.jer, self.jmap, self.spk = _Out(rows * 2, torch.int64), _Out(self.maps * R64, torch.int32), _Out(self.maps * R64 * 3, torch.int64)
        self.want_jmap, self.want_spk = want_jmap, want_spk

    def args(self, null_jer=False):
        return (None if null_jer else _vp(self.jer.ptr()), _vp(self.jmap.ptr()) if self.want_jmap else None,
                _vp(self.spk.ptr()) if self.want_spk else None)

    def untouched(self):
        for o, what in ((self.jer, "jer"), (self.jmap, "jmap"), (self.spk, "spk")):
            o.check(what, written=False)

    def read(self, shape):
        jer = self.jer.check("jer").reshape(shape + (2,))
        jmap = self.jmap.check("jmap", self.want_jmap)
        spk = self.spk.check("spk", self.want_spk)
        return jer, jmap.reshape(self.maps, R64) if self.want_jmap else None, spk.reshape(self.maps, R64, 3) if self.want_spk else None


def _timed(eng, packed, collar=0, flags=0, want_map=True, want_jmap=True, want_spk=True, expect=0, null_hyp2=False, null_jer=False):
    """plda_der_timed_jer_dev on guarded buffers; packed = der_overlap_model.pack's tuple -> (counts, map, jer, jmap, spk)"""
    import torch
    turns, ss, sd, hyp, off, uem, hyp2 = packed
    r = len(off) - 1
    keep, ukeep = _inputs(turns, ss, sd, uem)
    khyp, khyp2 = _guarded_input(np.asarray(hyp, np.int32)), _guarded_input(np.asarray(hyp2, np.int32))
    oC, oM, oJ = _Out(r * 4, torch.int64), _Out(r * R64, torch.int32), _JerOut(r, want_jmap=want_jmap, want_spk=want_spk)
    torch.cuda.synchronize()
    rc = _lib().plda_der_timed_jer_dev(eng._h, _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), _hp(np.ascontiguousarray(turns[3], np.int64)),
                                       _ptr(keep[3]), _ptr(keep[4]), _ptr(khyp), None if null_hyp2 else _ptr(khyp2),
                                       _hp(np.ascontiguousarray(off, np.int64)), r, _ptr(ukeep[0]) if uem is not None else None,
                                       _ptr(ukeep[1]) if uem is not None else None,
                                       _hp(np.ascontiguousarray(uem[2], np.int64)) if uem is not None else None, collar, flags,
                                       _vp(oC.ptr()), _vp(oM.ptr()) if want_map else None, *oJ.args(null_jer))
    torch.cuda.synchronize()
    assert rc == expect, "status %d: %s" % (rc, _last(eng))
    if expect:
        oC.check("counts", written=False)
        oM.check("map", written=False)
        oJ.untouched()
        return rc
    mp = oM.check("map", want_map)
    return (oC.check("counts").reshape(r, 4), mp.reshape(r, R64) if want_map else None) + oJ.read((r,))


def _seg(eng, ref, hyp, offsets, dur=None, expect=0, want_jmap=True, want_spk=True, null_jer=False):
    """plda_der_jer_dev on guarded buffers -> (counts, map, jer, jmap, spk)"""
    import torch
    offsets = np.ascontiguousarray(offsets, np.int64)
    r = len(offsets) - 1
    keep = [_guarded_input(np.asarray(a, np.int32)) for a in (ref, hyp)] + ([_guarded_input(np.asarray(dur, np.int32))] if dur is not None else [])
    oC, oM, oJ = _Out(r * 4, torch.int64), _Out(r * R64, torch.int32), _JerOut(r, want_jmap=want_jmap, want_spk=want_spk)
    torch.cuda.synchronize()
    rc = _lib().plda_der_jer_dev(eng._h, _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]) if dur is not None else None, _hp(offsets), r,
                                 _vp(oC.ptr()), _vp(oM.ptr()), *oJ.args(null_jer))
    torch.cuda.synchronize()
    assert rc == expect, "status %d: %s" % (rc, _last(eng))
    if expect:
        oC.check("counts", written=False)
        oM.check("map", written=False)
        oJ.untouched()
        return rc
    return (oC.check("counts").reshape(r, 4), oM.check("map").reshape(r, R64)) + oJ.read((r,))


def _sweep_seg(eng, merges, offsets, ref, thresholds, dur=None, num_speakers=None, expect=0):
    """plda_der_jer_sweep_dev on guarded buffers -> (counts [Q, R, 4], n_clusters [Q, R], jer [Q, R, 2])"""
    import torch
    from plda_amd import diarize
    offsets, thresholds = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(thresholds, np.float64)
    r, q = len(offsets) - 1, len(thresholds)
    minc = diarize.stop_args(offsets, 0.0, num_speakers)[2]
    keep = [_guarded_input(np.asarray(merges[0], np.int32)), _guarded_input(np.asarray(merges[1], np.int32)),
            _guarded_input(np.asarray(merges[2], np.float64)), _guarded_input(np.asarray(ref, np.int32))]
    kd = _guarded_input(np.asarray(dur, np.int32)) if dur is not None else None
    oC, oK, oJ = _Out(q * r * 4, torch.int64), _Out(q * r, torch.int32), _Out(q * r * 2, torch.int64)
    torch.cuda.synchronize()
    rc = _lib().plda_der_jer_sweep_dev(eng._h, _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), _hp(offsets), r, _ptr(keep[3]),
                                       _ptr(kd) if kd is not None else None, _hp(thresholds), q, _hp(minc), _vp(oC.ptr()), _vp(oK.ptr()),
                                       _vp(oJ.ptr()))
    torch.cuda.synchronize()
    assert rc == expect, "status %d: %s" % (rc, _last(eng))
    if expect:
        for o, what in ((oC, "counts"), (oK, "n_clusters"), (oJ, "jer")):
            o.check(what, written=False)
        return rc
    return oC.check("counts").reshape(q, r, 4), oK.check("n_clusters").reshape(q, r), oJ.check("jer").reshape(q, r, 2)


def _sweep_timed(eng, merges, packed, thresholds, num_speakers=None, collar=0, flags=0, expect=0, null_jer=False):
    """plda_der_timed_jer_sweep_dev on guarded buffers -> (counts [Q, R, 4], n_clusters [Q, R], jer [Q, R, 2]), or the status"""
    import torch
    from plda_amd import diarize
    turns, ss, sd, _, off, uem = packed[:6]
    off, thresholds = np.ascontiguousarray(off, np.int64), np.ascontiguousarray(thresholds, np.float64)
    r, q = len(off) - 1, len(thresholds)
    minc = diarize.stop_args(off, 0.0, num_speakers)[2]
    keep, ukeep = _inputs(turns, ss, sd, uem)
    km = [_guarded_input(np.asarray(merges[0], np.int32)), _guarded_input(np.asarray(merges[1], np.int32)),
          _guarded_input(np.asarray(merges[2], np.float64))]
    oC, oK, oJ = _Out(q * r * 4, torch.int64), _Out(q * r, torch.int32), _Out(q * r * 2, torch.int64)
    torch.cuda.synchronize()
    rc = _lib().plda_der_timed_jer_sweep_dev(eng._h, _ptr(km[0]), _ptr(km[1]), _ptr(km[2]), _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]),
                                             _hp(np.ascontiguousarray(turns[3], np.int64)), _ptr(keep[3]), _ptr(keep[4]), _hp(off), r,
                                             _ptr(ukeep[0]) if uem is not None else None, _ptr(ukeep[1]) if uem is not None else None,
                                             _hp(np.ascontiguousarray(uem[2], np.int64)) if uem is not None else None, collar, flags,
                                             _hp(thresholds), q, _hp(minc), _vp(oC.ptr()), _vp(oK.ptr()), None if null_jer else _vp(oJ.ptr()))
    torch.cuda.synchronize()
    assert rc == expect, "status %d: %s" % (rc, _last(eng))
    if expect:
        for o, what in ((oC, "counts"), (oK, "n_clusters"), (oJ, "jer")):
            o.check(what, written=False)
        return rc
    return oC.check("counts").reshape(q, r, 4), oK.check("n_clusters").reshape(q, r), oJ.check("jer").reshape(q, r, 2)


def _model(recs, collar=0, skip=False):
    """per recording: (counts, (C, rt, ht, rl, hl))"""
    out = []
    for r in recs:
        four, C, rt, ht, rl, hl = J.atoms_intervals(r, collar, skip)
        out.append((four[:3] + [four[3] - O.best_map_scipy(C)], (C, rt, ht, rl, hl)))
    return out


def _compare(got, model, what=""):
    counts, mp, jer, jmap, spk = got
    for q, (want, mats) in enumerate(model):
        assert counts[q].tolist() == want, "%s recording %d: counts %r, model %r" % (what, q, counts[q].tolist(), want)
        J.check_outputs(jer[q], jmap[q], spk[q], *mats)


# ------------------------------------------------------------------------------------------- the definition
def test_symbols_exist():
    lib = _lib()
    for name in ("plda_der_jer_plan", "plda_der_jer", "plda_der_jer_dev", "plda_der_jer_sweep", "plda_der_jer_sweep_dev", "plda_der_timed_jer",
                 "plda_der_timed_jer_dev", "plda_der_timed_jer_sweep", "plda_der_timed_jer_sweep_dev"):
        assert hasattr(lib, name), name


@pytest.mark.parametrize("ss, sd, hyp, hyp2, ts, td, tk, counts, jer, jmaps", [
    ([0], [15], [3], [-1], [0, 5], [10, 10], [0, 1], [20, 5, 0, 5], [2, 2863311530], ({0: 3}, {1: 3})),
    ([0, 5, 10], [5, 5, 5], [3, 3, 8], [-1, 8, -1], [0, 5], [10, 10], [0, 1], [20, 0, 0, 0], [2, 8589934592], ({0: 3, 1: 8},)),
    ([0, 40, 200], [40, 30, 1000], [3, 8, 3], [-1, -1, -1], [0], [100], [0], [100, 30, 1000, 30], [1, 1288490188], ({0: 8},))])
def test_header_examples_from_the_public_interface(ss, sd, hyp, hyp2, ts, td, tk, counts, jer, jmaps):
    from liblda.plda import PLDA
    r = O.rec(ts=ts, td=td, tk=tk, ss=ss, sd=sd, hyp=hyp, hyp2=hyp2)
    assert J.score(r, atoms=J.atoms_ticks) == (counts, jer)
    turns, ss, sd, hyp, off, _, hyp2 = O.pack([r])
    res = PLDA(0).der_timed(turns, ss, sd, hyp, off, hyp2=hyp2, return_map=True, jer=True)
    assert res.counts.tolist() == [counts] and res.jer_counts.tolist() == [jer]
    assert {i: int(j) for i, j in enumerate(res.jer_map[0]) if j >= 0} in jmaps
    assert res.jer[0] == J.rate(jer) == res.jer_total
    four, C, rt, ht, rl, hl = J.atoms_ticks(r)
    for lab, hl_, ticks, inter, union, rate in res.speakers[0]:
        assert ticks == rt[rl.index(lab)] and hl_ == int(res.jer_map[0][lab]) and rate == 1.0 - inter / union
    if len(tk) == 1:                                                       # example 3: the two maps differ
        assert res.map[0][0] == 3 and res.jer_map[0][0] == 8 and res.speakers[0] == [(0, 8, 100, 30, 100, 1.0 - 30 / 100)]
    plain = PLDA(0).der_timed(turns, ss, sd, hyp, off, hyp2=hyp2, return_map=True)
    assert plain.jer is None and plain.jer_counts is None and plain.speakers is None and np.array_equal(plain.map, res.map)


SPECS = [  # n_seg, n_turns, n_spk, n_hyp, span, n_uem
    (1, 0, 1, 1, 40, 0), (1, 3, 1, 1, 40, 0), (2, 5, 2, 3, 60, 0), (2, 0, 1, 2, 50, 1), (63, 40, 2, 5, 900, 0), (64, 80, 8, 3, 900, 2),
    (65, 30, 1, 9, 900, 0), (257, 300, 64, 6, 6000, 0), (400, 640, 64, 90, 20000, 1), (400, 100, 4, 120, 20000, 0), (63, 500, 64, 2, 5000, 0),
    (64, 20, 2, 40, 700, 0), (65, 60, 5, 5, 800, 3), (2, 2, 2, 1, 30, 0), (257, 9, 1, 30, 4000, 0), (1, 6, 3, 1, 80, 0), (30, 30, 6, 6, 400, 0),
    (12, 9, 3, 3, 90, 2), (40, 50, 8, 7, 260, 0), (7, 0, 1, 4, 60, 0), (64, 64, 2, 2, 500, 0), (90, 12, 1, 1, 900, 0), (33, 44, 4, 9, 300, 1),
    (400, 30, 2, 5, 9000, 0)]


@pytest.fixture(scope="module")
def batch():
    """24 seeded recordings over the listed sizes, about 20 % second labels; [19] has no turns, [20] a hypothesis of -1 alone"""
    rng = np.random.default_rng(2222)
    recs = [O.random_recording(rng, n, nt, n_spk=k, span=span, n_hyp=nh, n_uem=nu) for n, nt, k, nh, span, nu in SPECS]
    recs[20]["hyp"][:] = -1
    recs[20]["hyp2"][:] = -1
    assert len(recs) == 24 and {len(r["hyp"]) for r in recs} >= {1, 2, 63, 64, 65, 257, 400}
    plain = [dict(r, us=None, ud=None) for r in recs]
    return {True: recs, False: plain}, {}


@pytest.mark.parametrize("collar, skip, uem", [(0, False, True), (3, True, True), (3, False, False), (0, True, False)])
def test_seeded_batch_in_one_call(eng, batch, collar, skip, uem):
    recs, cache = batch[0][uem], batch[1]
    model = cache.setdefault((collar, skip, uem), _model(recs, collar, skip))
    flags = T.SKIP_OVERLAP if skip else 0
    packed = O.pack(recs)
    got = _timed(eng, packed, collar, flags)
    _compare(got, model, "collar %d skip %d uem %d" % (collar, skip, uem))
    counts, mp, jer, jmap, spk = got
    base_c, base_m = _ovl_dev(eng, packed, collar, flags)                   # plda_der_timed_ovl_dev on the same input
    assert np.array_equal(counts, base_c) and np.array_equal(mp, base_m)
    n_ref = jer[:, 0].tolist()
    if collar == 0 and not skip:
        assert {0, 1, 2, 64} <= set(n_ref) and n_ref[19] == 0 and jer[20].tolist()[1] == 0 and n_ref[20] > 0
        sh = [len(m[1][4]) for m in model]
        assert any(a > b > 0 for a, b in zip(sh, n_ref)) and any(0 < a < b for a, b in zip(sh, n_ref))
        second = sum(int((r["hyp2"] >= 0).sum()) for r in recs) / sum(int((r["hyp"] >= 0).sum()) for r in recs)
        assert 0.1 < second < 0.3
        assert sum(0 < js < n << 32 for n, js in jer.tolist()) > 12
    for q in (0, 7, 8, 19, 20):                                            # alone = in the batch, bit for bit
        one = _timed(eng, O.pack([recs[q]]), collar, flags)
        assert all(np.array_equal(a[0], b[q]) for a, b in zip(one, got)), "recording %d" % q


def test_no_second_label_and_null_outputs(eng, batch):
    recs = batch[0][True][:12]
    packed = O.pack(recs)
    none = packed[:6] + (np.full(len(packed[3]), -1, np.int32),)
    a = _timed(eng, none, 2)
    b = _timed(eng, packed, 2, null_hyp2=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = _timed(eng, packed, 2, null_hyp2=True, want_map=False, want_jmap=False, want_spk=False)
    assert c[1] is None and c[3] is None and c[4] is None and np.array_equal(c[0], a[0]) and np.array_equal(c[2], a[2])
    d = _timed(eng, packed, 2, null_hyp2=True, want_jmap=False)
    assert d[3] is None and np.array_equal(d[4], a[4])
    assert _timed(eng, packed, 2, expect=E_INVAL, null_jer=True) == E_INVAL and _last(eng) == "der_timed_jer: jer is NULL"


# ------------------------------------------------------------------------------------------- classes and wide matrices
def test_more_than_256_columns(eng):
    """a thread of the solve owns two columns, and the second pass reads ht beyond the first 256"""
    rng = np.random.default_rng(31)
    r = O.random_recording(rng, 1200, 200, n_spk=7, span=60000, n_hyp=330, p_ns=0.05)
    model = _model([r], 1)
    assert len(model[0][1][4]) > 300
    _compare(_timed(eng, O.pack([r]), 1), model)


def _past_the_boundary(eng):
    """64 reference speakers and more hypothesis labels than the JER form keeps in LDS (the way of test_gpu_der_overlap's
    _hbm_matrix)"""
    from plda_amd import der
    top = der.plan_jer(eng, 64, 64)["lds_max"]
    assert 64 < top < der.plan(eng, 64, 64)["lds_max"]                     # the JER form's boundary is its own
    rng = np.random.default_rng(62)
    r = O.random_recording(rng, 2500, 640, n_spk=64, span=100000, n_hyp=top + 120, p_ns=0.05)
    rl, hl = O._labels(r)
    assert len(rl) == 64 and len(hl) > top
    assert der.plan_jer(eng, 64, len(hl)) == {"cls": 1, "scratch_bytes": 8 * 64 * len(hl), "lds_max": top}
    assert der.plan_jer(eng, 64, top)["cls"] == 0 and der.plan_jer(eng, 64, top + 1)["cls"] == 1
    return r


@pytest.fixture(scope="module")
def classes(eng):
    rng = np.random.default_rng(63)
    recs = [O.random_recording(rng, 30, 40, n_spk=5, span=400, n_hyp=6), _past_the_boundary(eng), O.random_recording(rng, 1, 0, n_hyp=2),
            O.random_recording(rng, 12, 9, n_spk=3, span=90, n_hyp=3, n_uem=2)]
    return recs, _model(recs, 2)


def test_scratch_class_alone_and_mixed_classes_equal_each_alone(eng, classes):
    recs, model = classes
    got = _timed(eng, O.pack(recs), 2)
    _compare(got, model)
    assert got[2][1, 0] == 64 and 0 < got[2][1, 1] < 64 << 32
    from plda_amd import der
    first = dict(recs[1], hyp2=np.full(len(recs[1]["hyp"]), -1, np.int32))          # one label per segment: the timed form's own kernel
    assert der.plan_jer(eng, 64, len(O._labels(first)[1]))["cls"] == 1
    _compare(_timed(eng, O.pack([recs[1]]), 2, null_hyp2=True), _model([first], 2), "hyp2 = NULL")
    for q, r in enumerate(recs):
        one = _timed(eng, O.pack([r]), 2)
        assert all(np.array_equal(a[0], b[q]) for a, b in zip(one, got)), "recording %d" % q


def test_both_classes_at_the_boundary_segment_form(eng):
    """exactly lds_max and lds_max + 1 hypothesis labels under 64 reference labels: the last LDS and the first scratch matrix"""
    from plda_amd import der, diarize
    top = der.plan_jer(eng, 64, 64)["lds_max"]
    rng = np.random.default_rng(64)
    recs = [M.exact_shape(rng, sh + 50, 64, sh) for sh in (top, top + 1)]
    off = diarize.offsets_of([len(x[0]) for x in recs])
    ref, hyp, dur = (np.concatenate([x[k] for x in recs]) for k in range(3))
    counts, mp, jer, jmap, spk = _seg(eng, ref, hyp, off, dur)
    base_c, base_m = _der_dev(eng, ref, hyp, off, dur)
    assert np.array_equal(counts, base_c) and np.array_equal(mp, base_m)
    for q, (a, b, d) in enumerate(recs):
        four, C, rt, ht, rl, hl = J.atoms_segments(a, b, d)
        assert len(rl) == 64 and len(hl) == top + q
        J.check_outputs(jer[q], jmap[q], spk[q], C, rt, ht, rl, hl)


# ------------------------------------------------------------------------------------------- the quantisation edges
def test_quantisation_edges(eng):
    big = 1 << 30
    recs = [O.rec(ts=[0, 50], td=[20, 30], tk=[5, 9], ss=[0, 50], sd=[20, 30], hyp=[70, 4000]),           # a perfect match: w = 2^32
            O.rec(ts=[0], td=[20], tk=[5], ss=[30], sd=[20], hyp=[7]),                                     # no common tick
            O.rec(ts=[0], td=[big], tk=[0], ss=[0], sd=[big - 1], hyp=[1]),                                # C 2^32 just below 2^62
            O.rec(ts=[0], td=[big], tk=[63], ss=[0], sd=[big], hyp=[4095]),                                # C 2^32 = 2^62
            O.rec(ts=[0], td=[40], tk=[2], ss=[0, 10, 20, 30], sd=[10, 10, 10, 10], hyp=[9, 6, -1, -1]),   # two equal indices
            O.rec(ts=[0], td=[100], tk=[0], ss=[0, 40, 200], sd=[40, 30, 1000], hyp=[3, 8, 3])]            # header example 3
    model = _model(recs)
    got = _timed(eng, O.pack(recs))
    _compare(got, model)
    counts, mp, jer, jmap, spk = got
    assert jer.tolist() == [[2, 2 << 32], [1, 0], [1, (big - 1) * J.ONE // big], [1, 1 << 32], [1, 10 * J.ONE // 40], [1, 1288490188]]
    assert (jmap[1] == -1).all() and spk[1, 5].tolist() == [20, 0, 20] and spk[2, 0].tolist() == [big, big - 1, big]
    assert jmap[4, 2] in (6, 9) and mp[5, 0] == 3 and jmap[5, 0] == 8
    assert [J.rate(x) for x in jer.tolist()][:2] == [0.0, 1.0]


# ------------------------------------------------------------------------------------------- the segment form
@pytest.fixture(scope="module")
def seg_case():
    from plda_amd import diarize
    rng = np.random.default_rng(71)
    i32 = lambda *v: np.asarray(v, np.int32)
    recs = [(i32(3), i32(7), i32(5)), (i32(-1), i32(7), i32(5)), (i32(3), i32(-1), i32(5)), (i32(-1, -1, -1), i32(0, 1, -1), i32(2, 3, 4)),
            (i32(63, 7, 63, 40, 7, 63), i32(4095, 4095, 100, 64, 63, 0), i32(1, 2, 3, 4, 5, 6)),
            (i32(4, 9, 4), i32(1, 2, 2), i32(0, 0, 7)),                                   # label 9: only an empty segment
            M.random_case(rng, 50, 4, 6, gap=9), M.random_case(rng, 50, 6, 4, gap=12, max_dur=1), M.random_case(rng, 300, 10, 40),
            M.exact_shape(rng, 101, 64, 64), M.exact_shape(rng, 400, 3, 300)]
    return recs, diarize.offsets_of([len(x[0]) for x in recs])


def test_segment_form_equals_the_model_and_plda_der(eng, seg_case):
    from liblda.plda import PLDA
    recs, off = seg_case
    ref, hyp, dur = (np.concatenate([x[k] for x in recs]) for k in range(3))
    counts, mp, jer, jmap, spk = _seg(eng, ref, hyp, off, dur)
    base_c, base_m = _der_dev(eng, ref, hyp, off, dur)
    assert np.array_equal(counts, base_c) and np.array_equal(mp, base_m) and np.array_equal(counts, M.score(ref, hyp, off, dur))
    for q, (a, b, d) in enumerate(recs):
        four, C, rt, ht, rl, hl = J.atoms_segments(a, b, d)
        J.check_outputs(jer[q], jmap[q], spk[q], C, rt, ht, rl, hl)
    assert jer[5].tolist() == [1, 7 * J.ONE // 7] and spk[5, 9].tolist() == [0, 0, 0] and jer[1].tolist() == [0, 0]
    ones = _seg(eng, ref, hyp, off, None)
    assert all(np.array_equal(x, y) for x, y in zip(ones, _seg(eng, ref, hyp, off, np.ones(len(ref), np.int32))))
    res = PLDA(0).der(ref.tolist(), hyp, off, dur, return_map=True, jer=True)                    # the host form
    assert all(np.array_equal(x, y) for x, y in zip((res.counts, res.map, res.jer_counts, res.jer_map), (counts, mp, jer, jmap)))
    assert math.isnan(res.jer[1]) and res.jer_total == J.rate(jer.sum(0)) and res.speakers[5] == [(4, 2, 7, 7, 7, 0.0)]
    no_map = _seg(eng, ref, hyp, off, dur, want_jmap=False, want_spk=False)
    assert no_map[3] is None and no_map[4] is None and np.array_equal(no_map[2], jer)


def test_segment_form_refuses_more_than_2_30_ticks(eng, seg_case):
    recs, off = seg_case
    ref, hyp, dur = (np.concatenate([x[k] for x in recs]) for k in range(3))
    base = _seg(eng, ref, hyp, off, dur)
    at = int(off[8])
    for add, bad in ((0, 0), (1, 1)):
        d = dur.copy()
        d[at] += (1 << 30) - int(dur[off[8]:off[9]].sum()) + add          # recording 8 adds up to 2^30 (+ 1)
        if bad:
            assert _seg(eng, ref, hyp, off, d, expect=E_INVAL) == E_INVAL and "1 invalid entries" in _last(eng) and "2^30" in _last(eng)
        else:
            assert _seg(eng, ref, hyp, off, d)[2][8, 0] == base[2][8, 0]
        assert _der_dev(eng, ref, hyp, off, d)[0].shape == (len(off) - 1, 4)                      # plda_der keeps accepting it
    d = dur.copy()
    d[3], d[at], d[at + 1] = -1, 1 << 30, 1 << 30
    assert _seg(eng, ref, hyp, off, d, expect=E_INVAL) == E_INVAL and "2 invalid entries" in _last(eng)
    h = hyp.copy()
    h[2] = 4096
    assert _seg(eng, ref, h, off, dur, expect=E_INVAL) == E_INVAL and "1 invalid entries" in _last(eng)
    assert _seg(eng, ref, hyp, off, dur, expect=E_INVAL, null_jer=True) == E_INVAL and _last(eng) == "der_jer: jer is NULL"
    assert all(np.array_equal(x, y) for x, y in zip(base, _seg(eng, ref, hyp, off, dur)))        # the handle works as before
    with pytest.raises(ValueError):
        eng.der(ref, hyp, off, np.where(np.arange(len(ref)) == at, 1 << 30, dur), jer=True)


# ------------------------------------------------------------------------------------------- the sweeps
def test_timed_sweep_equals_cut_then_the_jer_call(eng, sweep_case):
    from plda_amd import der, diarize
    recs, merges, thresholds = sweep_case
    packed = T.pack(recs)
    turns, ss, sd, _, off, _ = packed
    for num_speakers in (None, [1, 5, 2, 12, 2, 3]):
        counts, ncl, jer = _sweep_timed(eng, merges, packed, thresholds, num_speakers, collar=2)
        base_c, base_k = _timed_sweep_dev(eng, merges, packed, thresholds, num_speakers, collar=2)
        assert np.array_equal(counts, base_c) and np.array_equal(ncl, base_k)
        for q, thr in enumerate(thresholds):
            labels, k = diarize.cut(merges, off, float(thr), num_speakers)
            cut = [O.rec(r["ts"], r["td"], r["tk"], r["ss"], r["sd"], labels[off[i]:off[i + 1]]) for i, r in enumerate(recs)]
            one = _timed(eng, O.pack(cut), 2, null_hyp2=True)
            assert np.array_equal(one[0], counts[q]) and np.array_equal(one[2], jer[q]) and np.array_equal(ncl[q], k), "threshold %d" % q
            assert [J.score(r, 2)[1] for r in cut] == jer[q].tolist(), "threshold %d against the model" % q
    res = der.sweep_timed(eng, merges, turns, ss, sd, off, thresholds, None, collar=2, jer=True)
    counts, ncl, jer = _sweep_timed(eng, merges, packed, thresholds, None, collar=2)
    assert np.array_equal(res.counts, counts) and np.array_equal(res.n_clusters, ncl) and np.array_equal(res.jer_counts, jer)
    assert res.best_jer == der.best_jer_index(jer) and res.jer.tolist() == [der.pooled_jer(j) for j in jer]
    plain = der.sweep_timed(eng, merges, turns, ss, sd, off, thresholds, None, collar=2)
    assert plain.jer_counts is None and plain.best == res.best and np.array_equal(plain.counts, res.counts)


def test_segment_sweep_equals_cut_then_the_jer_call(eng, sweep_case):
    from plda_amd import der, diarize
    recs, merges, thresholds = sweep_case
    off = T.pack(recs)[4]
    rng = np.random.default_rng(72)
    n = int(off[-1])
    ref = rng.integers(-1, 5, n).astype(np.int32)
    dur = rng.integers(0, 9, n).astype(np.int32)
    counts, ncl, jer = _sweep_seg(eng, merges, off, ref, thresholds, dur)
    base_c, base_k = _der_sweep_dev(eng, merges, off, ref, thresholds, dur)
    assert np.array_equal(counts, base_c) and np.array_equal(ncl, base_k)
    for q, thr in enumerate(thresholds):
        labels, k = diarize.cut(merges, off, float(thr), None)
        one = _seg(eng, ref, labels, off, dur)
        assert np.array_equal(one[0], counts[q]) and np.array_equal(one[2], jer[q]) and np.array_equal(ncl[q], k), "threshold %d" % q
        want = [J.jer(*J.atoms_segments(ref[off[i]:off[i + 1]], labels[off[i]:off[i + 1]], dur[off[i]:off[i + 1]])[1:4]) for i in range(len(off) - 1)]
        assert want == jer[q].tolist(), "threshold %d against the model" % q
    res = der.sweep(eng, merges, off, ref, thresholds, dur, jer=True)
    assert np.array_equal(res.jer_counts, jer) and np.array_equal(res.counts, counts) and res.best_jer == der.best_jer_index(jer)
    big = dur.copy()
    big[0] = (1 << 30) + 1
    assert _sweep_seg(eng, merges, off, ref, thresholds, big, expect=E_INVAL) == E_INVAL and "1 invalid entries" in _last(eng)
    assert _lib().plda_der_jer_sweep_dev(eng._h, None, None, None, _hp(np.asarray([0, 1], np.int64)), 1, _vp(8), None,
                                         _hp(np.zeros(1)), 1, None, _vp(8), _vp(8), None) == E_INVAL
    assert _last(eng) == "der_jer_sweep: jer is NULL"


@pytest.fixture(scope="module")
def wide_sweep(eng):
    """one recording of 460 segments whose sweep reaches the scratch class: a full merge record, thresholds that leave every
    segment alone, more clusters than the JER form keeps in LDS, about as many, and few; a time line with 64 reference speakers
    and per-segment reference labels over 64 speakers"""
    from plda_amd import der, diarize
    S, _ = M.planted_block([60, 90, 45, 70, 55, 80, 60], 77, noise=0.6)
    n = len(S)
    _, ncl, merges = diarize.ahc(eng, [S], None, 1, return_merges=True)
    assert n == 460 and ncl[0] == 1
    cost = np.sort(merges[2])
    thresholds = np.asarray([-cost[0] + 1.0, -cost[60], -cost[150], -cost[400], -cost[-1] - 1.0], np.float64)
    rng = np.random.default_rng(78)
    rec = O.rec(**{k: v for k, v in T.random_recording(rng, n, 700, n_spk=64, span=60000, n_hyp=3).items() if k in ("ts", "td", "tk", "ss", "sd", "hyp")})
    ref = rng.permutation(np.concatenate([np.arange(64), rng.integers(-1, 64, n - 64)])).astype(np.int32)
    dur = rng.integers(1, 9, n).astype(np.int32)
    return merges, thresholds, rec, ref, dur, der.plan_jer(eng, 64, 64)["lds_max"]


def test_timed_sweep_in_the_scratch_class(eng, wide_sweep):
    from plda_amd import der, diarize
    merges, thresholds, rec, _, _, top = wide_sweep
    packed = T.pack([O.without_second(rec)])
    off = packed[4]
    counts, ncl, jer = _sweep_timed(eng, merges, packed, thresholds, None, collar=2)
    base_c, base_k = _timed_sweep_dev(eng, merges, packed, thresholds, None, collar=2)
    assert np.array_equal(counts, base_c) and np.array_equal(ncl, base_k)
    assert ncl[0, 0] == 460 and (ncl[:, 0] > top).sum() >= 2 and (ncl[:, 0] <= top).sum() >= 2 and ncl[-1, 0] == 1
    for q, thr in enumerate(thresholds):
        labels, k = diarize.cut(merges, off, float(thr), None)
        cut = O.rec(rec["ts"], rec["td"], rec["tk"], rec["ss"], rec["sd"], labels)
        want_counts, want_jer = J.score(cut, 2)
        assert counts[q, 0].tolist() == want_counts and jer[q, 0].tolist() == want_jer and ncl[q, 0] == k[0], "threshold %d" % q
        one = _timed(eng, O.pack([cut]), 2, null_hyp2=True)
        assert np.array_equal(one[0], counts[q]) and np.array_equal(one[2], jer[q]), "threshold %d" % q
        if q == 0:
            assert want_jer[0] == 64 and der.plan_jer(eng, 64, int(k[0]))["cls"] == 1


def test_segment_sweep_in_the_scratch_class(eng, wide_sweep):
    from plda_amd import der, diarize
    merges, thresholds, _, ref, dur, top = wide_sweep
    off = np.asarray([0, len(ref)], np.int64)
    counts, ncl, jer = _sweep_seg(eng, merges, off, ref, thresholds, dur)
    base_c, base_k = _der_sweep_dev(eng, merges, off, ref, thresholds, dur)
    assert np.array_equal(counts, base_c) and np.array_equal(ncl, base_k)
    assert ncl[0, 0] == 460 and (ncl[:, 0] > top).sum() >= 2 and (ncl[:, 0] <= top).sum() >= 2
    for q, thr in enumerate(thresholds):
        labels, k = diarize.cut(merges, off, float(thr), None)
        four, C, rt, ht, rl, hl = J.atoms_segments(ref, labels, dur)
        assert len(rl) == 64 and der.plan_jer(eng, 64, len(hl))["cls"] == (1 if len(hl) > top else 0)
        assert jer[q, 0].tolist() == J.jer(C, rt, ht) and counts[q, 0].tolist() == M.score(ref, labels, off, dur)[0].tolist(), "threshold %d" % q
        one = _seg(eng, ref, labels, off, dur)
        assert np.array_equal(one[0], counts[q]) and np.array_equal(one[2], jer[q]) and ncl[q, 0] == k[0], "threshold %d" % q
        J.check_outputs(one[2][0], one[3][0], one[4][0], C, rt, ht, rl, hl)


# ------------------------------------------------------------------------------------------- errors of the timed form
def test_timed_sweep_violations_write_nothing_and_null_jer_is_refused_everywhere(eng, sweep_case):
    recs, merges, thresholds = sweep_case
    packed = T.pack(recs)
    base = _sweep_timed(eng, merges, packed, thresholds, None, collar=2)
    bad = (packed[0], np.where(np.arange(len(packed[1])) == 3, -1, packed[1]).astype(np.int32)) + packed[2:]       # a negative segment start
    assert _sweep_timed(eng, merges, bad, thresholds, None, collar=2, expect=E_INVAL) == E_INVAL and "1 invalid entries" in _last(eng)
    turns = (packed[0][0], packed[0][1], np.where(np.arange(len(packed[0][2])) == 0, 64, packed[0][2]).astype(np.int32), packed[0][3])
    assert _sweep_timed(eng, merges, (turns,) + packed[1:], thresholds, None, expect=E_INVAL) == E_INVAL and "1 invalid entries" in _last(eng)
    short = (np.where(np.arange(len(merges[0])) == 0, -1, merges[0]).astype(np.int32), merges[1], merges[2])       # a record that is not full
    assert _sweep_timed(eng, short, packed, thresholds[1:2], None, expect=E_INVAL) == E_INVAL and "not a full record" in _last(eng)
    assert _sweep_timed(eng, merges, packed, thresholds, None, expect=E_INVAL, null_jer=True) == E_INVAL
    assert _last(eng) == "der_timed_jer_sweep: jer is NULL"
    assert all(np.array_equal(x, y) for x, y in zip(base, _sweep_timed(eng, merges, packed, thresholds, None, collar=2)))
    # the host forms: one recording of one segment, every array in host memory, jer = NULL
    lib, one = _lib(), np.asarray([0, 1], np.int64)
    i32 = lambda *v: np.asarray(v, np.int32)
    ts, td, tk, ss, sd, hyp, ref, thr = i32(0), i32(5), i32(0), i32(0), i32(5), i32(0), i32(0), np.zeros(1)
    counts, ncl, mp = np.full(4, 7, np.int64), np.full(1, 7, np.int32), np.full(64, 7, np.int32)
    assert lib.plda_der_jer(eng._h, _hp(ref), _hp(hyp), None, _hp(one), 1, _hp(counts), _hp(mp), None, None, None) == E_INVAL
    assert _last(eng) == "der_jer: jer is NULL"
    assert lib.plda_der_jer_sweep(eng._h, None, None, None, _hp(one), 1, _hp(ref), None, _hp(thr), 1, None, _hp(counts), _hp(ncl), None) == E_INVAL
    assert _last(eng) == "der_jer_sweep: jer is NULL"
    assert lib.plda_der_timed_jer(eng._h, _hp(ts), _hp(td), _hp(tk), _hp(one), _hp(ss), _hp(sd), _hp(hyp), None, _hp(one), 1, None, None, None, 0, 0,
                                  _hp(counts), _hp(mp), None, None, None) == E_INVAL
    assert _last(eng) == "der_timed_jer: jer is NULL"
    assert lib.plda_der_timed_jer_sweep(eng._h, None, None, None, _hp(ts), _hp(td), _hp(tk), _hp(one), _hp(ss), _hp(sd), _hp(one), 1, None, None, None,
                                        0, 0, _hp(thr), 1, None, _hp(counts), _hp(ncl), None) == E_INVAL
    assert _last(eng) == "der_timed_jer_sweep: jer is NULL"
    assert (counts == 7).all() and (ncl == 7).all() and (mp == 7).all()
    jer = np.zeros(2, np.int64)                                            # and with it the same calls go through
    assert lib.plda_der_timed_jer_sweep(eng._h, None, None, None, _hp(ts), _hp(td), _hp(tk), _hp(one), _hp(ss), _hp(sd), _hp(one), 1, None, None, None,
                                        0, 0, _hp(thr), 1, None, _hp(counts), _hp(ncl), _hp(jer)) == 0
    assert counts.tolist() == [5, 0, 0, 0] and ncl.tolist() == [1] and jer.tolist() == [1, 1 << 32]
    assert lib.plda_der_jer_sweep(eng._h, None, None, None, _hp(one), 1, _hp(ref), None, _hp(thr), 1, None, _hp(counts), _hp(ncl), _hp(jer)) == 0
    assert counts.tolist() == [1, 0, 0, 0] and jer.tolist() == [1, 1 << 32]


def test_every_entry_violation_is_counted_and_writes_nothing(eng):
    good = [O.rec([0, 5, 20], [10, 10, 5], [0, 1, 0], [0, 15, 30], [15, 10, 4], [3, 4, -1], [4, -1, -1]), O.rec([1], [4], [2], [0], [9], [0], [-1])]
    packed = O.pack(good)
    base = _timed(eng, packed)
    _compare(base, _model(good))

    def put(k, at, v):
        arrs = [np.array(a) for a in (packed[3], packed[6], packed[1], packed[2], packed[0][0], packed[0][1], packed[0][2])]
        arrs[k][at] = v
        turns = (arrs[4], arrs[5], arrs[6], packed[0][3])
        return (turns, arrs[2], arrs[3], arrs[0], packed[4], packed[5], arrs[1])
    kinds = {"hyp2 below -1": put(1, 1, -2), "hyp2 at PLDA_AHC_MAX": put(1, 1, 4096), "a second label without a first": put(1, 2, 5),
             "equal to the first": put(1, 0, 3), "hyp at PLDA_AHC_MAX": put(0, 1, 4096), "a negative segment start": put(2, 0, -1),
             "a segment beyond 2^30": put(3, 3, (1 << 30) + 1), "a speaker at 64": put(6, 1, 64), "a negative turn": put(5, 0, -3)}
    for kind, call in kinds.items():
        assert _timed(eng, call, expect=E_INVAL) == E_INVAL, kind
        assert "1 invalid entries" in _last(eng) and "0 invalid events" in _last(eng), (kind, _last(eng))
    shared = put(2, 1, 14)
    assert _timed(eng, shared, expect=E_INVAL) == E_INVAL and "1 invalid events" in _last(eng)    # two segments share a tick
    assert all(np.array_equal(x, y) for x, y in zip(base, _timed(eng, packed)))                   # the handle works as before


# ------------------------------------------------------------------------------------------- host forms, history, the pipeline
def test_host_forms_equal_the_device_forms(eng, batch):
    import torch
    from plda_amd import der
    recs = batch[0][True][:12]
    turns, ss, sd, hyp, off, uem, hyp2 = O.pack(recs)
    counts, mp, jer, jmap, spk = _timed(eng, O.pack(recs), 3, T.SKIP_OVERLAP)
    res = der.der_timed(eng, turns, ss, sd, hyp, off, 3, uem, True, return_map=True, hyp2=hyp2, jer=True)
    assert all(np.array_equal(x, y) for x, y in zip((res.counts, res.map, res.jer_counts, res.jer_map), (counts, mp, jer, jmap)))
    for q in range(len(recs)):
        assert res.speakers[q] == [(i, int(jmap[q, i]), int(spk[q, i, 0]), int(spk[q, i, 1]), int(spk[q, i, 2]), 1.0 - spk[q, i, 1] / spk[q, i, 2])
                                   for i in range(R64) if spk[q, i, 0] > 0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    d = [dev(a) for a in (turns[0], turns[1], turns[2], ss, sd, hyp, hyp2, uem[0], uem[1])]
    r = len(off) - 1
    oc, oj = torch.zeros((r, 4), dtype=torch.int64, device="cuda"), torch.zeros((r, 2), dtype=torch.int64, device="cuda")
    eng.der_timed_jer_dev([x.data_ptr() for x in d[:3]], turns[3], d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), off,
                          oc.data_ptr(), oj.data_ptr(), duem=(d[7].data_ptr(), d[8].data_ptr()), uem_off=uem[2], collar=3, flags=1)
    torch.cuda.synchronize()
    assert np.array_equal(oc.cpu().numpy(), counts) and np.array_equal(oj.cpu().numpy(), jer)


def test_after_other_calls_the_bits_of_a_fresh_handle(eng, classes, seg_case):
    """a handle that has run DER, VBx and JER calls of both classes returns what a fresh handle returns"""
    import vbx_model as V
    from plda_amd import MPlda, diarize
    recs, _ = classes
    packed = O.pack(recs)
    segs, off = seg_case
    ref, hyp, dur = (np.concatenate([x[k] for x in segs]) for k in range(3))
    from test_gpu_der import _model_params
    old = MPlda(0)
    old.set_model(*_model_params(16, 11, psi_scale=4.0))                   # (VBx wants some model on the handle)
    _ovl_dev(old, packed, 1)
    _der_dev(old, ref, hyp, off, dur)
    y, labels = V.generate(64, 16, 4, 8, 5)[:2]
    diarize.vbx(old, y, diarize.offsets_of([64]), labels, 30.0 * np.exp(-4.0 * np.arange(16) / 16), max_iters=4)
    _seg(old, ref, hyp, off, dur)
    a, b = _timed(old, packed, 2), _timed(MPlda(0), packed, 2)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    a, b = _seg(old, ref, hyp, off, dur), _seg(MPlda(0), ref, hyp, off, dur)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_tune_threshold_on_jer_equals_the_models_argmin():
    from liblda.plda import PLDA
    from test_gpu_der import _model_params
    d, sizes = 16, (4, 9, 14)
    mean, Tm, psi = _model_params(d, 11, psi_scale=4.0)
    p = PLDA(0)
    p._instance.set_model(mean, Tm, psi)
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
    best, res = p.tune_threshold(x, off, None, thresholds, turns=turns, seg_start=ss, seg_dur=sd, collar=1, metric="jer")
    pooled = []
    for q, thr in enumerate(thresholds):
        labels, _ = p.cluster(x, off, threshold=float(thr))
        cut = [O.rec(r["ts"], r["td"], r["tk"], r["ss"], r["sd"], labels[off[i]:off[i + 1]]) for i, r in enumerate(recs)]
        pairs = [J.score(r, 1)[1] for r in cut]
        assert pairs == res.jer_counts[q].tolist(), "threshold %d" % q
        pooled.append((sum(a for a, _ in pairs), sum(b for _, b in pairs)))
    assert all(n == pooled[0][0] > 0 for n, _ in pooled)                   # (the reference speakers do not depend on the threshold,
    want = max(range(len(pooled)), key=lambda q: (pooled[q][1], -q))       #  so the least pooled JER is the largest sum, first of equals)
    assert best == thresholds[want] and res.best_jer == want and len(set(res.jer.tolist())) > 2
    by_der, res_der = p.tune_threshold(x, off, None, thresholds, turns=turns, seg_start=ss, seg_dur=sd, collar=1)
    assert res_der.jer_counts is None and np.array_equal(res_der.counts, res.counts) and by_der == thresholds[res_der.best]
    ref = np.concatenate([np.repeat(np.arange(len(sizes)), sizes)] * 4).astype(np.int32)
    best2, res2 = p.tune_threshold(x, off, ref, thresholds, metric="jer")                       # the segment form
    assert best2 == thresholds[res2.best_jer] and res2.jer_counts.shape == (7, 4, 2)
    with pytest.raises(ValueError):
        p.tune_threshold(x, off, ref, thresholds, metric="eer")
