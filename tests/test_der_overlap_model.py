"""CPU: the host models of the time-based DER with two hypothesis labels per segment (tests/der_overlap_model.py) against each
other and against der_time_model where there is no second label; the header's worked examples; the host side of the feature:
rttm.pack_hyp / rttm.write(labels2=), diarize.apply_overlap, der.timed_args on hyp2, the ctypes table."""
import ctypes as C
import io

import numpy as np
import pytest

import der_overlap_model as O
import der_time_model as T


def _cases():
    """300 seeded small recordings: up to 4 reference speakers, up to 12 segments, collars that swallow whole turns, UEM
    intervals that cut segments mid-way, every third one with skip-overlap"""
    rng = np.random.default_rng(2100)
    for k in range(300):
        n_seg, n_turns = int(rng.integers(1, 13)), int(rng.integers(0, 9))
        span = int(rng.integers(12, 90))
        r = O.random_recording(rng, n_seg, n_turns, n_spk=int(rng.integers(1, 5)), span=span, n_hyp=int(rng.integers(1, 6)),
                               n_uem=int(rng.integers(1, 4)) if k % 3 == 1 else 0, p_second=0.35)
        collar = int(rng.choice([0, 0, 1, 3, span // 4]))                # (span / 4 is longer than most turns)
        yield k, r, collar, k % 3 == 2


def test_300_seeded_cases_models_agree():
    seconds = swallowed = cut = 0
    for k, r, collar, skip in _cases():
        a, b = O.score_ticks(r, collar, skip), O.score_atoms(r, collar, skip)
        assert a[0] == b[0] and (a[1] == b[1]).all() and a[2:] == b[2:], "case %d: ticks %r atoms %r" % (k, a[0], b[0])
        assert min(a[0]) >= 0
        seconds += int((r["hyp2"] >= 0).sum())
        swallowed += int(collar > 0 and ((r["td"] > 0) & (r["td"] <= 2 * collar)).any())
        if r["us"] is not None:
            e = r["ss"] + r["sd"]
            cut += int(any(((r["ss"] < u) & (u < e)).any() for u in np.concatenate([r["us"], r["us"] + r["ud"]])))
        plain = dict(r, hyp2=np.full(len(r["hyp"]), -1, np.int32))
        want = T.score_ticks(O.without_second(plain), collar, skip)
        for model in (O.score_ticks, O.score_atoms):
            got = model(plain, collar, skip)
            assert got[0] == want[0] and (got[1] == want[1]).all() and got[2:] == want[2:], "case %d without a second label" % k
        assert T.score_atoms(O.without_second(plain), collar, skip)[0] == want[0]
    assert seconds > 300 and swallowed > 30 and cut > 30, (seconds, swallowed, cut)


def _example(segs):
    ss, sd, hyp, hyp2 = zip(*segs)
    return O.rec(ts=[0, 5], td=[10, 10], tk=[0, 1], ss=ss, sd=sd, hyp=hyp, hyp2=hyp2)


EXAMPLES = [([(0, 5, 0, -1), (5, 5, 0, 1), (10, 5, 1, -1)], [20, 0, 0, 0]),
            ([(0, 15, 0, 1)], [20, 0, 10, 0]),
            ([(0, 15, 0, -1)], [20, 5, 0, 5])]


@pytest.mark.parametrize("segs, want", EXAMPLES)
def test_header_examples(segs, want):
    r = _example(segs)
    assert O.score_ticks(r)[0] == want and O.score_atoms(r)[0] == want


def test_exhaustive_map_against_scipy():
    rng = np.random.default_rng(5)
    for _ in range(200):
        c = rng.integers(0, 6, (int(rng.integers(0, 5)), int(rng.integers(0, 7))))
        assert O.best_map_exhaustive(c.tolist()) == O.best_map_scipy(c.astype(object))


# ------------------------------------------------------------------------------------------- rttm
def test_pack_hyp_cuts_turns_and_round_trips():
    from plda_amd import rttm
    turns = {"a": [(0, 50, "x"), (30, 40, "y"), (70, 10, "x"), (100, 5, "z"), (100, 5, "y"), (120, 0, "x")],
             "b": [(10, 20, "only")], "c": []}
    ss, sd, hyp, hyp2, off = rttm.pack_hyp(turns, ["a", "b", "c", "d"])
    assert off.tolist() == [0, 5, 6, 7, 8] and off.dtype == np.int64 and all(a.dtype == np.int32 for a in (ss, sd, hyp, hyp2))
    assert list(zip(ss.tolist(), sd.tolist(), hyp.tolist(), hyp2.tolist()))[:6] == [
        (0, 30, 0, -1), (30, 20, 0, 1), (50, 20, 1, -1), (70, 10, 0, -1), (100, 5, 1, 2), (10, 20, 0, -1)]
    assert (hyp[6:] == -1).all() and (hyp2[6:] == -1).all() and (sd[6:] == 0).all()       # no speech: one empty segment
    assert ((hyp2 < 0) | (hyp < hyp2)).all()                              # the lower label is hyp
    f = io.StringIO()
    rttm.write(f, ["a", "b", "c", "d"], off, hyp, ss, sd, labels2=hyp2)
    back = rttm.read(io.StringIO(f.getvalue()))
    assert sorted(back) == ["a", "b"]
    # spk0 = x: [0, 50) and [70, 80) (abutting pieces merged per speaker); spk1 = y: [30, 70), [100, 105); spk2 = z
    assert sorted(back["a"]) == sorted([(0, 50, "spk0"), (70, 10, "spk0"), (30, 40, "spk1"), (100, 5, "spk1"), (100, 5, "spk2")])
    assert back["b"] == [(10, 20, "spk0")]
    again = rttm.pack_hyp(back, ["a", "b", "c", "d"])
    for x, y in zip(again, (ss, sd, hyp, hyp2, off)):
        assert np.array_equal(x, y)


def test_write_without_labels2_is_unchanged():
    from plda_amd import rttm
    off, lab = np.asarray([0, 4, 6]), np.asarray([1, 1, -1, 0, 2, 2])
    st, du = np.asarray([0, 10, 20, 30, 5, 16]), np.asarray([10, 10, 10, 5, 10, 4])
    a, b, c = io.StringIO(), io.StringIO(), io.StringIO()
    rttm.write(a, ["r0", "r1"], off, lab, st, du)
    rttm.write(b, ["r0", "r1"], off, lab, st, du, labels2=None)
    assert a.getvalue() == b.getvalue() and a.getvalue().count("\n") == 4
    rttm.write(c, ["r0", "r1"], off, lab, st, du, labels2=np.full(6, -1))
    assert sorted(c.getvalue().splitlines()) == sorted(a.getvalue().splitlines())
    with pytest.raises(ValueError):
        rttm.write(io.StringIO(), ["r0", "r1"], off, lab, st, du, labels2=np.zeros(5, np.int32))


def test_pack_hyp_refuses_three_at_once():
    from plda_amd import rttm
    turns = {"rec7": [(0, 50, "x"), (30, 40, "y"), (45, 10, "z")]}
    with pytest.raises(ValueError, match=r"rec7.*tick 45"):
        rttm.pack_hyp(turns, ["rec7"])
    rttm.pack_hyp({"rec7": turns["rec7"][:2] + [(50, 10, "z")]}, ["rec7"])                # z starts as x ends: depth 2


# ------------------------------------------------------------------------------------------- apply_overlap, timed_args
def test_apply_overlap():
    from plda_amd import diarize
    l2 = np.asarray([1, 0, -1, 2, 1], np.int32)
    p2 = np.asarray([0.4, 0.05, 0.0, 0.2, 0.1])
    mask = np.asarray([False, True, True, False, False])
    assert diarize.apply_overlap(l2, p2, overlap=mask).tolist() == [-1, 0, -1, -1, -1]
    assert diarize.apply_overlap(l2, p2, min_posterior=0.2).tolist() == [1, -1, -1, 2, -1]
    out = diarize.apply_overlap(l2, p2, overlap=mask, min_posterior=0.2)
    assert out.tolist() == [1, 0, -1, 2, -1] and out.dtype == np.int32
    assert diarize.apply_overlap(l2, p2, min_posterior=0.0).tolist() == [1, 0, -1, 2, 1]  # (no second speaker stays -1)
    for bad in (dict(), dict(overlap=mask[:4]), dict(overlap=mask.astype(np.int32)), dict(min_posterior="x"), dict(min_posterior=float("nan"))):
        with pytest.raises(ValueError):
            diarize.apply_overlap(l2, p2, **bad)
    with pytest.raises(ValueError):
        diarize.apply_overlap(l2, p2[:3], min_posterior=0.1)


def test_timed_args_checks_hyp2():
    from plda_amd import der
    turns = (np.asarray([0]), np.asarray([10]), np.asarray([0]), np.asarray([0, 1]))
    ss, sd, off = np.asarray([0, 5, 9]), np.asarray([5, 4, 3]), np.asarray([0, 3])
    hyp = np.asarray([2, -1, 0])
    good = der.timed_args(turns, ss, sd, off, 0, None, False, hyp, np.asarray([0, -1, -1]))
    assert len(good) == 13 and good[12].dtype == np.int32 and good[12].tolist() == [0, -1, -1]
    assert len(der.timed_args(turns, ss, sd, off, 0, None, False)) == 12
    bad = {"shape": np.asarray([0, -1]), "dtype": np.asarray([0.0, -1.0, -1.0]), "below": np.asarray([-2, -1, -1]),
           "above": np.asarray([4096, -1, -1]), "second without first": np.asarray([-1, 3, -1]), "equal to first": np.asarray([-1, -1, 0])}
    for kind, h2 in bad.items():
        with pytest.raises(ValueError):
            der.timed_args(turns, ss, sd, off, 0, None, False, hyp, h2)
        with pytest.raises(ValueError):                                   # der_timed: before any device work (no engine is touched)
            der.der_timed(None, turns, ss, sd, hyp, off, hyp2=h2)
    with pytest.raises(ValueError):
        der.timed_args(turns, ss, sd, off, 0, None, False, None, np.asarray([0, -1, -1]))


def test_ctypes_table_has_the_four_entries():
    from plda_amd import _native as N
    for name, base in (("plda_der_timed_ovl_dev", "plda_der_timed_dev"), ("plda_der_timed_ovl", "plda_der_timed")):
        assert N.SIGNATURES[name][1] == N.SIGNATURES[base][1][:8] + [C.c_void_p] + N.SIGNATURES[base][1][8:]
    for name, base in (("plda_vbx_top2_dev", "plda_vbx_dev"), ("plda_vbx_top2", "plda_vbx")):
        assert N.SIGNATURES[name][1] == N.SIGNATURES[base][1] + [C.c_void_p] * 2
    lib = N.load()
    assert all(hasattr(lib, n) for n in ("plda_der_timed_ovl_dev", "plda_der_timed_ovl", "plda_vbx_top2_dev", "plda_vbx_top2"))
