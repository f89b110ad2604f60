"""CPU: the definition of a side (include/plda_hip.h, "quality-aware calibration") in its two host forms -- the test model
tests/fusion_side_model.py and the package's plda_amd.fusion.side_values -- on hand-made cases, the planted case through the
host fit of tests/fusion_model.py on materialised sides, and the argument checks of plda_amd.fusion.Side that come before
any device call."""
import numpy as np
import pytest

import fusion_model as fm
import fusion_side_model as sm

F = np.float32


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


HAND = [
    # op, e, t, expected (ties, signed zeros and negative values by the written comparison)
    ("min", [1, 5, -3, 2, 0.0, -0.0], [2, 4, -2, 2, -0.0, 0.0], [1, 4, -3, 2, -0.0, 0.0]),     # 0 < -0 is false: t
    ("max", [1, 5, -3, 2, 0.0, -0.0], [2, 4, -2, 2, -0.0, 0.0], [2, 5, -2, 2, -0.0, 0.0]),
    ("sum", [1, -5, 0.0, -0.0, 1e30], [2, 5, -0.0, -0.0, 1e30], [3, 0.0, 0.0, -0.0, 2e30]),
    ("absdiff", [1, -5, 3, 0.0, -0.0], [2, 5, 3, -0.0, 0.0], [1, 10, 0.0, 0.0, 0.0]),
    ("prod", [1, -5, -3, 0.0, -0.0], [2, 5, -2, -1, -1], [2, -25, 6, -0.0, 0.0]),
]


@pytest.mark.parametrize("op,e,t,exp", HAND)
def test_side_values_on_hand_made_cases(op, e, t, exp):
    from plda_amd import fusion as FU
    for f in (sm.side_values, FU.side_values):
        got = f(op, np.array(e, F), np.array(t, F))
        assert got.dtype == np.float32
        assert _bits(got) == _bits(np.array(exp, F)), (f.__module__, op, got)
        assert _bits(f(sm.OPS.index(op), np.array(e, F), np.array(t, F))) == _bits(got)          # the op by its code


def test_side_values_are_single_fp32_operations_and_broadcast():
    from plda_amd import fusion as FU
    rng = np.random.default_rng(1)
    e, t = (rng.standard_normal(40) * 10.0 ** rng.integers(-3, 4, 40)).astype(F), (rng.standard_normal(70) * 3).astype(F)
    e[3], t[5] = np.nan, np.inf
    exp = {"min": np.where(e[:, None] < t[None, :], e[:, None], t[None, :]), "max": np.where(e[:, None] > t[None, :], e[:, None], t[None, :]),
           "sum": e[:, None] + t[None, :], "absdiff": np.abs(e[:, None] - t[None, :]), "prod": e[:, None] * t[None, :]}
    for op in sm.OPS:
        with np.errstate(all="ignore"):
            a, b = sm.side_values(op, e[:, None], t[None, :]), FU.side_values(op, e[:, None], t[None, :])
        assert a.shape == b.shape == (40, 70) and a.dtype == b.dtype == np.float32
        assert _bits(a) == _bits(b) == _bits(exp[op].astype(F)), op
    # a NaN on the enrol side: the comparison is false, MIN and MAX return t; the other three return NaN
    assert np.array_equal(sm.side_values("min", e[3], t[:5]), t[:5]) and np.all(np.isnan(sm.side_values("sum", e[3], t[:5])))
    with pytest.raises(ValueError):
        sm.side_values(5, e, e)
    with pytest.raises(ValueError):
        FU.side_values("mean", e, e)


def _fit(es, ts, feats, prior=0.5):
    pos, neg = fm.split(feats, es, ts)
    return fm.fit(pos, neg, prior)


def test_planted_case_quality_terms_lower_cllr():
    es, ts, s, qe, qt = sm.planted_case()
    assert s.shape == (300, 500) and int((es[:, None] == ts[None, :]).sum()) == 2468
    alone = _fit(es, ts, [s])
    assert alone["converged"] and not alone["separable"]
    for ops in (("min", "max"), ("min", "absdiff")):
        f = _fit(es, ts, [s] + sm.materialise([(op, qe, qt) for op in ops], 300, 500))
        print("score alone: Cllr %.4f in %d iterations; with %s: %.4f in %d" % (alone["cllr_after"], alone["iterations"], ops,
                                                                                f["cllr_after"], f["iterations"]))
        assert f["converged"] and not f["separable"]
        assert f["cllr_after"] < alone["cllr_after"]
        assert f["a"].shape == (3,)


def test_planted_case_dependent_sides_are_refused_on_the_pivot():
    es, ts, s, qe, qt = sm.planted_case()
    twice = sm.materialise([("min", qe, qt), ("min", qe, qt)], 300, 500)
    with pytest.raises(ValueError, match="Cholesky pivot of system 2"):
        _fit(es, ts, [s] + twice)
    # min + max = sum exactly in exact arithmetic: the third is an affine function of the two before it
    with pytest.raises(ValueError, match="Cholesky pivot of system 3"):
        _fit(es, ts, [s] + sm.materialise([("min", qe, qt), ("max", qe, qt), ("sum", qe, qt)], 300, 500))


def test_side_refuses_bad_arguments_before_any_device_call():
    from plda_amd import fusion as FU
    e, t = np.zeros(5, F), np.zeros(7, F)
    with pytest.raises(ValueError, match="unknown side op"):
        FU.Side("mean", e, t)
    with pytest.raises(ValueError, match="unknown side op"):
        FU.Side(5, e, t)
    with pytest.raises(ValueError, match="1-D"):
        FU.Side("min", np.zeros((5, 1), F), t)
    s = FU.Side("absdiff", e, t)
    assert s.op == "absdiff" and s.code == 3
    s.check(5, 7)
    for m, nt in ((7, 5), (5, 8), (4, 7)):
        with pytest.raises(ValueError, match="5 enrol and 7 test values"):
            s.check(m, nt)
    # the device entry points check the lengths first: no engine is touched (None would fail on any use)
    for call in (lambda: FU.pass_with_sides_dev(None, [1], [8], [s], 5, 8, 0, 0, [0.0, 0.0]),
                 lambda: FU.fit_with_sides_dev(None, [1], [8], [s], 4, 7, 0, 0),
                 lambda: FU.apply_with_sides_dev(None, [1], [8], [s], 5, 8, FU.QualityFusion([1.0, 1.0], 0.0, ["absdiff"]), 1, 8),
                 lambda: FU.fit_from_operands_with_sides_dev(None, 1, None, 1, 5, 1, 8, None, None, 1, 1, [s])):
        with pytest.raises(ValueError, match="5 enrol and 7 test values"):
            call()


def test_quality_fusion_maps_host_values_in_fp64():
    from plda_amd import fusion as FU
    es, ts, s, qe, qt = sm.planted_case()
    q = FU.QualityFusion([0.5, -0.25, 2.0], 0.125, ["min", "absdiff"], prior=0.3)
    assert q.n_systems == 1 and q.n_sides == 2 and q.ops == ("min", "absdiff") and isinstance(q, FU.Fusion)
    mats = sm.materialise([("min", qe, qt), ("absdiff", qe, qt)], 300, 500)
    exp = 0.125 + 0.5 * s.astype(np.float64) - 0.25 * mats[0].astype(np.float64) + 2.0 * mats[1].astype(np.float64)
    got = q([s], [(qe, qt), (qe, qt)])
    assert got.dtype == np.float64 and np.allclose(got, exp, rtol=1e-15, atol=1e-15)
    lab = es[:, None] == ts[None, :]
    i, j = np.nonzero(lab)
    assert np.array_equal(q([s[lab]], [(qe[i], qt[j]), (qe[i], qt[j])]), got[lab])                # listed trials
    with pytest.raises(ValueError):
        q([s], [(qe, qt)])
    with pytest.raises(ValueError):
        FU.QualityFusion([1.0], 0.0, ["min"])
