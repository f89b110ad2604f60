"""CPU: the ROC-convex-hull yardstick (tests/rocch_model.py) against a brute-force hull, sklearn's isotonic regression and
the closed forms; then the library's pure host steps (plda_rocch_hull / plda_rocch_finish) against the yardstick, driven with
NumPy ranks."""
import math

import numpy as np
import pytest

import rocch_model as RM


def _lists(rng, n_pos, n_neg, quant, shift=1.0):
    pos = rng.normal(shift, 1.0, n_pos).astype(np.float32)
    neg = rng.normal(0.0, 1.0, n_neg).astype(np.float32)
    if quant:
        pos, neg = (np.round(pos / quant) * quant).astype(np.float32), (np.round(neg / quant) * quant).astype(np.float32)
    return pos, neg


def check_library_against_model(pos, neg):
    """plda_rocch_hull + plda_rocch_finish on the NumPy reduced points == the sort-based model."""
    from plda_amd import rocch as R
    from plda_amd import _native as N
    m = RM.model(pos, neg)
    edge_class, u, olt, ole, elt, ele = RM.reduced_points(pos, neg)
    rc, res, verts, llr = R.host_hull(u, olt, ole, elt, ele, edge_class, len(pos), len(neg))
    assert rc == N.PLDA_OK
    assert res["n_vertices"] == len(m["vertices"]) == len(verts)
    assert np.all(np.isnan(verts["threshold"]))
    lo, hi = RM.neighbours(pos, neg, [None] + [int(k) for k in verts["key"][1:]])
    rc, verts = R.host_finish(verts, lo, hi)
    assert rc == N.PLDA_OK
    got = [(int(v["x"]), int(v["y"]), int(v["fa"]), int(v["miss"]), int(v["key"]), int(v["has_key"]), float(v["threshold"])) for v in verts]
    assert got == m["vertices"]
    assert len(llr) == len(m["llr"])
    for a, b in zip(llr, m["llr"]):
        assert a == b if math.isinf(b) else abs(a - b) <= 1e-12 * max(1.0, abs(b))
    assert abs(res["min_cllr"] - m["min_cllr"]) <= 1e-12
    assert RM.ulp_distance(res["eer"], float(m["eer"])) <= 4
    Np, Nn = len(pos), len(neg)
    assert (res["eer_far_lo"], res["eer_frr_lo"]) == ((Nn - m["eer_lo"][0]) / Nn, m["eer_lo"][1] / Np)
    assert (res["eer_far_hi"], res["eer_frr_hi"]) == ((Nn - m["eer_hi"][0]) / Nn, m["eer_hi"][1] / Np)
    return m, res


# ---------------------------------------------------------------------------------------------- the model itself
@pytest.mark.parametrize("seed", range(12))
def test_model_hull_is_the_brute_force_hull(seed):
    rng = np.random.default_rng(seed)
    pos, neg = _lists(rng, int(rng.integers(1, 7)), int(rng.integers(1, 7)), (1.0, 0.5, 0.0)[seed % 3])
    pts = RM.roc_points(pos, neg)
    if len(pts) > 12:
        pts = pts[:12]
    assert [(p[0], p[1]) for p in RM.lower_hull(pts)] == RM.brute_hull(pts)


@pytest.mark.parametrize("quant", [0.0, 0.25, 1.0])
def test_model_min_cllr_is_isotonic_regression(quant):
    iso = pytest.importorskip("sklearn.isotonic")
    rng = np.random.default_rng(3)
    for n_pos, n_neg in ((40, 300), (300, 40), (120, 120)):
        pos, neg = _lists(rng, n_pos, n_neg, quant)
        m = RM.model(pos, neg)
        s = np.concatenate([pos, neg]).astype(np.float64)
        y = np.concatenate([np.ones(n_pos), np.zeros(n_neg)])
        p = iso.IsotonicRegression(y_min=0.0, y_max=1.0, increasing=True).fit(s, y).predict(s)
        with np.errstate(divide="ignore"):
            llr = np.log(p) - np.log1p(-p) - math.log(n_pos / n_neg)
        assert abs(RM.cllr_of_llrs(llr[:n_pos], llr[n_pos:]) - m["min_cllr"]) <= 1e-9
        # and the model's own map gives the same figure through its segments
        assert abs(RM.cllr_of_llrs(RM.pav_apply(m, pos).astype(np.float64), RM.pav_apply(m, neg).astype(np.float64)) - m["min_cllr"]) <= 1e-6


def test_model_closed_forms():
    sep = RM.model([2.0, 3.0, 3.0], [-1.0, 0.0, 1.0, 1.0])
    assert sep["min_cllr"] == 0.0 and len(sep["vertices"]) == 3 and sep["llr"] == [-math.inf, math.inf] and sep["eer"] == 0
    one = RM.model([0.5] * 5, [0.5] * 3)
    assert one["min_cllr"] == 1.0 and len(one["vertices"]) == 2 and one["llr"] == [0.0] and one["eer"] == Fraction12()
    rev = RM.model([-1.0, -2.0], [1.0, 2.0, 3.0])
    assert rev["min_cllr"] == 1.0 and len(rev["vertices"]) == 2 and rev["eer"] == Fraction12()


def Fraction12():
    from fractions import Fraction
    return Fraction(1, 2)


# ---------------------------------------------------------------------------------------------- the library's host steps
@pytest.mark.parametrize("quant", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("shape", [(1, 1), (1, 50), (50, 1), (7, 7), (30, 400), (400, 30), (200, 200)])
def test_library_hull_matches_the_model(shape, quant):
    rng = np.random.default_rng(100 * shape[0] + shape[1] + int(quant * 8))
    check_library_against_model(*_lists(rng, shape[0], shape[1], quant))


def test_library_closed_forms_and_edge_scores():
    _, sep = check_library_against_model(np.float32([2.0, 3.0, 3.0]), np.float32([-1.0, 0.0, 1.0, 1.0]))
    assert sep["min_cllr"] == 0.0 and sep["n_vertices"] == 3 and sep["eer"] == 0.0
    _, one = check_library_against_model(np.float32([0.5] * 5), np.float32([0.5] * 3))
    assert one["min_cllr"] == 1.0 and one["n_vertices"] == 2 and one["eer"] == 0.5
    _, rev = check_library_against_model(np.float32([-1.0, -2.0]), np.float32([1.0, 2.0, 3.0]))
    assert rev["min_cllr"] == 1.0 and rev["n_vertices"] == 2 and rev["eer"] == 0.5
    fmax, den = np.finfo(np.float32).max, np.float32(1e-45)
    check_library_against_model(np.float32([0.0, -0.0, den, fmax, 1.0]), np.float32([-0.0, 0.0, -den, -fmax, den, 1.0, fmax]))


def test_library_hull_refuses_inconsistent_points():
    from plda_amd import rocch as R
    from plda_amd import _native as N
    pos, neg = _lists(np.random.default_rng(5), 20, 60, 0.5)
    ec, u, olt, ole, elt, ele = RM.reduced_points(pos, neg)
    ok = R.host_hull(u, olt, ole, elt, ele, ec, 20, 60)
    assert ok[0] == N.PLDA_OK
    assert R.host_hull(u, olt, ole, elt, ele, ec, 20, 60, cap_vertices=1)[0] == N.PLDA_E_CAPACITY
    assert R.host_hull(u[::-1], olt, ole, elt, ele, ec, 20, 60)[0] == N.PLDA_E_INVAL           # keys not ascending
    assert R.host_hull(u, olt, ole, elt, ele, ec, 21, 60)[0] == N.PLDA_E_INVAL                 # the edge counts miss the total
    assert R.host_hull(u, olt, ole, elt, ele, ec, 20, 0)[0] == N.PLDA_E_INVAL                  # an empty class
    bad = ole.copy()
    bad[0] = 61
    assert R.host_hull(u, olt, bad, elt, ele, ec, 20, 60)[0] == N.PLDA_E_INVAL                 # more than the other class holds
    assert R.host_hull(u, olt, ole, elt, ele, 2, 20, 60)[0] == N.PLDA_E_INVAL


def test_host_pav_is_the_model_map():
    from plda_amd import rocch as R
    rng = np.random.default_rng(9)
    pos, neg = _lists(rng, 60, 500, 0.25)
    m = RM.model(pos, neg)
    verts = np.zeros(len(m["vertices"]), R.VERTEX_DTYPE)
    for i, v in enumerate(m["vertices"]):
        verts[i] = v[:4] + (v[6], v[4], v[5])
    pav = R.Pav(verts, m["llr"])
    probe = np.concatenate([pos, neg, np.float32([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e30, -1e30])])
    for bound in (0.0, 3.0):
        a, b = pav(probe, bound), RM.pav_apply(m, probe, bound)
        assert np.array_equal(a, b, equal_nan=True)
    mapped = pav(np.sort(np.concatenate([pos, neg])))
    assert np.all(mapped[1:] >= mapped[:-1])
