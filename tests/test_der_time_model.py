"""CPU: the two host models of the time-based DER (tests/der_time_model.py) against each other and against the worked example
of include/plda_hip.h; the optimum against scipy; the RTTM / UEM helpers of plda_amd/rttm.py; the argument checks of
plda_amd/der.py (no engine, no device); the ctypes table."""
import io

import numpy as np
import pytest

import der_model as M
import der_time_model as T


def _example():
    return T.rec(ts=[0, 5], td=[10, 10], tk=[0, 1], ss=[0], sd=[15], hyp=[7])


def test_worked_example():
    for model in (T.score_ticks, T.score_atoms):
        assert model(_example(), 0)[0] == [20, 5, 0, 5]
        assert model(_example(), 1)[0] == [12, 3, 0, 3]
        assert model(_example(), 0, True)[0] == [10, 0, 0, 5]            # [5, 10) is not scored; X maps to one of A, B
        assert model(_example(), 100)[0] == [0, 0, 0, 0]


def _small_case(k):
    rng = np.random.default_rng(1000 + k)
    span = int(rng.integers(1, 267 if k % 3 == 0 else 400))               # (a UEM interval may end at 1.5 span: at most 400 ticks)
    r = T.random_recording(rng, int(rng.integers(1, 12)), int(rng.integers(0, 14)), n_spk=int(rng.integers(1, 7)), span=span,
                           n_hyp=int(rng.integers(1, 6)), n_uem=int(rng.integers(0, 4)) if k % 3 == 0 else 0)
    collar = (0, 1, 3, 25, span)[k % 5]                                   # 25 and span swallow whole turns; zones overlap
    return r, collar, k % 4 == 1


def test_interval_model_equals_tick_model_on_320_cases():
    swallowed = cut = 0
    for k in range(320):
        r, collar, skip = _small_case(k)
        a, b = T.score_ticks(r, collar, skip), T.score_atoms(r, collar, skip)
        assert a[0] == b[0], "case %d: ticks %r, atoms %r" % (k, a[0], b[0])
        assert (a[1] == b[1]).all() and a[2:] == b[2:], "case %d: matrices differ" % k
        assert len(a[2]) <= 6
        swallowed += collar > 0 and bool((r["td"] > 0).any()) and bool((r["td"][r["td"] > 0] <= 2 * collar).any())
        if r["us"] is not None and len(r["ts"]):
            e = r["ts"] + r["td"]
            cut += any(((r["ts"] < u) & (u < e)).any() for u in np.concatenate([r["us"], r["us"] + r["ud"]]).tolist())
    assert swallowed > 50 and cut > 20                                    # the cases the issue names do occur


def test_correct_equals_scipy():
    from scipy.optimize import linear_sum_assignment
    for k in range(0, 320, 4):
        r, collar, skip = _small_case(k)
        c, C, rl, hl = T.score_atoms(r, collar, skip)
        Ci = np.asarray(C, np.int64).reshape(len(rl), len(hl))
        rows, cols = linear_sum_assignment(Ci, maximize=True) if Ci.size else ([], [])
        both = c[0] - c[1]                                                # speech - miss = the sum of min(nref, nhyp)
        assert both - c[3] == int(Ci[rows, cols].sum()) == M.assign(C)[0]


def test_pack_turns_merges_and_refuses_65_speakers():
    from plda_amd import rttm
    turns = {"a": [(0, 10, "y"), (10, 5, "y"), (30, 0, "y"), (12, 8, "y"), (40, 5, "y"), (3, 4, "x")], "b": [(1, 2, "z")]}
    (ts, td, tk, off), names = rttm.pack_turns(turns, ["a", "c", "b"])
    assert names == [["x", "y"], [], ["z"]] and off.tolist() == [0, 3, 3, 4]
    assert list(zip(ts.tolist(), td.tolist(), tk.tolist())) == [(3, 4, 0), (0, 20, 1), (40, 5, 1), (1, 2, 0)]
    assert ts.dtype == td.dtype == tk.dtype == np.int32 and off.dtype == np.int64
    many = {"a": [(k, 1, "s%02d" % k) for k in range(65)]}
    with pytest.raises(ValueError):
        rttm.pack_turns(many, ["a"])
    assert len(rttm.pack_turns({"a": many["a"][:64]}, ["a"])[1][0]) == 64


def test_cut_windows():
    from plda_amd import rttm
    # 150-tick windows every 75 (overlap 75, odd: 38 to the earlier), a gap, an abutting pair, a second recording
    s, d = rttm.cut_windows([0, 75, 150, 400, 450, 0, 10], [150, 150, 150, 50, 20, 20, 20], [0, 5, 7])
    assert s.tolist() == [0, 113, 188, 400, 450, 0, 15] and d.tolist() == [113, 75, 112, 50, 20, 15, 15]
    e = s + d
    assert (e[:4] <= s[1:5]).all() and s.dtype == np.int32
    s, d = rttm.cut_windows([0, 3], [4, 4], [0, 2])                      # overlap 1: the extra tick goes to the earlier window
    assert s.tolist() == [0, 4] and d.tolist() == [4, 3]
    with pytest.raises(ValueError):
        rttm.cut_windows([10, 0], [5, 5], [0, 2])


def test_read_uem_round_trip():
    from plda_amd import rttm
    text = ";; comment\nrecA 1 0.00 12.50\nrecB 1 3.10 4.00\nrecA 1 20.00 20.75\n\n"
    uem = rttm.read_uem(io.StringIO(text))
    assert uem == {"recA": [(0, 1250), (2000, 75)], "recB": [(310, 90)]}
    us, ud, off = rttm.pack_uem(uem, ["recB", "none", "recA"])
    assert us.tolist() == [310, 0, 2000] and ud.tolist() == [90, 1250, 75] and off.tolist() == [0, 1, 1, 3]
    out = io.StringIO()
    for rec_id, ivs in uem.items():
        for a, b in ivs:
            out.write("%s 1 %.2f %.2f\n" % (rec_id, a * 0.01, (a + b) * 0.01))
    assert rttm.read_uem(io.StringIO(out.getvalue())) == uem
    with pytest.raises(ValueError):
        rttm.read_uem(io.StringIO("recA 1 5.0 4.0\n"))


def test_argument_checks_raise_without_an_engine():
    from plda_amd import der
    from plda_amd.libplda import MPlda
    turns, ss, sd, hyp, off, _ = T.pack([_example()])
    ok = lambda **kw: der.timed_args(kw.get("turns", turns), kw.get("ss", ss), kw.get("sd", sd), kw.get("off", off), kw.get("collar", 0),
                                     kw.get("uem"), False)
    assert ok()[10:] == (0, 0) and der.timed_args(turns, ss, sd, off, 5, None, True)[10:] == (5, der.SKIP_OVERLAP)
    put = lambda k, v: tuple(np.asarray(v) if i == k else a for i, a in enumerate(turns))
    for bad in (dict(turns=None), dict(turns=turns[:3]), dict(turns=put(2, [0, 64])), dict(turns=put(2, [0, -1])), dict(turns=put(0, [0, -5])),
                dict(turns=put(1, [10, 2 ** 30])), dict(turns=put(1, [10.0, 1.0])), dict(turns=put(3, [0, 1])), dict(turns=put(3, [1, 2])),
                dict(turns=put(3, [0, 2, 2])), dict(ss=[-1]), dict(sd=[2 ** 30 + 1]), dict(sd=[1, 2]), dict(off=[0, 0]), dict(off=[1, 2]),
                dict(collar=-1), dict(collar=2 ** 20 + 1), dict(collar=0.25), dict(uem=([0], [5])), dict(uem=([0], [5], [0, 2])),
                dict(uem=([0], [-5], [0, 1]))):
        with pytest.raises(ValueError):
            ok(**bad)
    assert ok(uem=([0, 3], [5, 5], [0, 2]))[9].tolist() == [0, 2]
    for call in (lambda: der.der_timed(None, turns, ss, sd, [4096], off), lambda: der.der_timed(None, turns, ss, sd, [0, 1], off),
                 lambda: der.sweep_timed(None, (np.zeros(0), np.zeros(0), np.zeros(0)), turns, ss, sd, off, [float("nan")]),
                 lambda: der.sweep_timed(None, (np.zeros(1), np.zeros(0), np.zeros(0)), turns, ss, sd, off, [0.0]),
                 lambda: der.sweep_timed(None, (np.zeros(0), np.zeros(0), np.zeros(0)), turns, ss, sd, off, [])):
        with pytest.raises(ValueError):
            call()
    for name in ("der_timed", "der_timed_dev", "der_timed_sweep_dev"):
        assert callable(getattr(MPlda, name))


def test_signatures():
    import ctypes as C
    from plda_amd import _native as N
    for name, nargs in (("plda_der_timed_plan", 6), ("plda_der_timed_dev", 17), ("plda_der_timed", 17), ("plda_der_timed_sweep_dev", 22),
                        ("plda_der_timed_sweep", 22)):
        assert name in N.SIGNATURES and len(N.SIGNATURES[name][1]) == nargs, name
    assert N.SIGNATURES["plda_der_timed_dev"][1][9] == C.c_int64 and N.SIGNATURES["plda_der_timed_dev"][1][13:15] == [C.c_int32] * 2
    assert N.SIGNATURES["plda_der_timed_sweep"][1][11] == C.c_int64 and N.SIGNATURES["plda_der_timed_sweep"][1][18] == C.c_int64
    lib = N.load()
    assert all(hasattr(lib, n) for n in N.SIGNATURES if n.startswith("plda_der_timed"))
