"""CPU: the host model of the AS-norm statistics (tests/asnorm_model.py) against a brute-force evaluation in exact rational
arithmetic, the Lipschitz facts the GPU tolerances rest on, and mutants that the exact comparison must reject -- so that the
yardstick of tests/test_gpu_asnorm.py is itself pinned.  Also the ABI surface of the feature (header, exports, ctypes)."""
from fractions import Fraction
import math

import numpy as np
import pytest

import asnorm_model as am


def _exact(row32, K):
    """(mean, variance) of the K largest values, as Fractions: sort, take, exact arithmetic."""
    vals = sorted((Fraction(float(v)) for v in np.asarray(row32, np.float32)), reverse=True)[:K]
    mean = sum(vals, Fraction(0)) / K
    var = sum(((v - mean) ** 2 for v in vals), Fraction(0)) / K
    return mean, var


def _sqrt_fraction(q):
    """sqrt of a non-negative Fraction as a float, without overflow or underflow of the intermediate."""
    if q == 0:
        return 0.0
    e = (q.numerator.bit_length() - q.denominator.bit_length()) // 2 * 2
    return math.sqrt(float(q / Fraction(2) ** e)) * 2.0 ** (e // 2)


def _agrees(got, row32, K):
    """The exact comparison: float64 results within a few roundings of the exact rational values; exactly so where the
    top-K values are all equal."""
    mean, std = got
    em, ev = _exact(row32, K)
    if ev == 0:
        return float(mean) == float(em) and float(std) == 0.0
    es = _sqrt_fraction(ev)
    ok_mean = abs(Fraction(float(mean)) - em) <= Fraction(2) ** -51 * abs(em) + Fraction(2) ** -60 * Fraction(es)
    ok_std = abs(float(std) - es) <= 2.0 ** -45 * es
    return bool(ok_mean and ok_std)


def _rows():
    rng = np.random.default_rng(1)
    f = np.float32
    rows = {
        "random": (rng.standard_normal(97) * 20 - 30).astype(f),
        "signs": np.array([-3.5, 2.25, -0.125, 7.0, 0.0, -11.0, 2.25, 1e-3, -1e-3, 5.5], f),
        "ties_straddle": np.array([5, 4, 4, 4, 4, 3, 3, 1, 0, -2], f),
        "all_equal": np.full(33, -17.375, f),
        "zeros": np.array([0.0, -0.0, 0.0, -0.0, -1.0, -0.0, 1e-30], f),
        "subnormal": np.array([1e-41, -1e-41, 3e-42, 0.0, -0.0, 1e-38, 2.5e-39], f),
        "wide": np.array([3e30, -3e30, 1.5, 2e-20, 1e30, 7.0, 7.0], f),
        "one": np.array([-42.0], f),
    }
    return rows


@pytest.mark.parametrize("name", sorted(_rows()))
def test_topk_stats_equals_exact_rational_evaluation(name):
    row = _rows()[name]
    n = row.shape[0]
    for K in sorted({1, 2, 3, 4, 5, 6, n // 2, n - 1, n} & set(range(1, n + 1))):
        got = am.topk_stats(row[None, :], K)
        assert _agrees((got[0][0], got[1][0]), row, K), (name, K, got, _exact(row, K))


def test_all_equal_top_k_is_exact():
    row = np.array([2.5, 2.5, 2.5, 2.5, 1.0, -3.0, 2.5], np.float32)
    for K in (1, 3, 5):
        mean, std = am.topk_stats(row[None, :], K)
        assert mean[0] == 2.5 and std[0] == 0.0
    mean, std = am.topk_stats(np.array([[0.0, -0.0, -0.0, -5.0]], np.float32), 3)
    assert mean[0] == 0.0 and std[0] == 0.0


def test_lipschitz_facts():
    """Sorted vectors are non-expansive in the sup norm, and the population std is 1-Lipschitz in ||.||_2 / sqrt(K): two rows
    that differ by at most eps element-wise have top-K means and stds within eps."""
    rng = np.random.default_rng(7)
    for trial in range(60):
        n = int(rng.integers(5, 400))
        K = int(rng.integers(1, n + 1))
        eps = float(10.0 ** rng.uniform(-6, 0))
        a = (rng.standard_normal(n) * 10).astype(np.float32)
        b = (a.astype(np.float64) + rng.uniform(-eps, eps, n)).astype(np.float32)
        e = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
        (ma, sa), (mb, sb) = am.topk_stats(a[None], K), am.topk_stats(b[None], K)
        slack = 1e-12 * (1.0 + abs(ma[0]) + sa[0])
        assert abs(ma[0] - mb[0]) <= e + slack and abs(sa[0] - sb[0]) <= e + slack, (trial, n, K, e)


# ---- mutants: each is a plausible wrong implementation; the exact comparison must reject every one
def _stats_of(vals):
    vals = np.asarray(vals, np.float64)
    return vals.mean(), vals.std()


def _m_fewer(row, K):
    return _stats_of(np.sort(row)[::-1][:K - 1])


def _m_more(row, K):
    return _stats_of(np.sort(row)[::-1][:K + 1])


def _m_sample_std(row, K):
    v = np.sort(row)[::-1][:K].astype(np.float64)
    return v.mean(), v.std(ddof=1)


def _m_smallest(row, K):
    return _stats_of(np.sort(row)[:K])


def _m_ties_once(row, K):
    return _stats_of(np.unique(row)[::-1][:K])


def _m_drop_last_column(row, K):
    return _stats_of(np.sort(row[:-1])[::-1][:K])


@pytest.mark.parametrize("mutant", [_m_fewer, _m_more, _m_sample_std, _m_smallest, _m_ties_once, _m_drop_last_column])
def test_exact_comparison_rejects_mutants(mutant):
    rng = np.random.default_rng(11)
    base = np.round(rng.standard_normal(300) * 8, 1).astype(np.float32)      # one decimal: many ties
    top = np.float32(base.max() + 1.0)
    row = np.concatenate([base, np.float32([top, top])])       # the last column is in every top-K set, and tied with another
    for K in (7, 50, 200):
        good = am.topk_stats(row[None], K)
        assert _agrees((good[0][0], good[1][0]), row, K)
        assert not _agrees(mutant(row, K), row, K), (mutant.__name__, K)


def test_snorm_apply_model():
    raw = np.array([[1.0, -2.0, 0.5], [4.0, 0.0, -8.0]], np.float32)
    em, es = np.array([0.5, -1.0]), np.array([2.0, 0.0])
    tm, ts = np.array([0.0, 1.0, 2.0]), np.array([1.0, 0.0, 4.0])
    both = am.snorm_apply(raw, em, es, tm, ts)
    assert both[0, 0] == 0.5 * ((1.0 - 0.5) / 2.0 + 1.0)
    assert both[0, 1] == 0.5 * ((-2.0 - 0.5) / 2.0 + -2.0)          # tstd == 0: that side contributes raw
    assert both[1, 2] == 0.5 * (-8.0 + (-8.0 - 2.0) / 4.0)          # estd == 0
    assert both[1, 1] == 0.0
    assert np.array_equal(am.snorm_apply(raw, em, es), am.snorm_sides(raw, em, es)[0])
    assert np.array_equal(am.snorm_apply(raw, None, None, tm, ts), am.snorm_sides(raw, None, None, tm, ts)[1])
    assert np.array_equal(am.snorm_apply(raw, np.zeros(2), np.ones(2), np.zeros(3), np.ones(3)), raw.astype(np.float64))


def test_abi_declares_and_exports_the_asnorm_entry_points():
    import ctypes
    from plda_amd import _native
    names = ["plda_cohort_stats", "plda_cohort_stats_dev", "plda_cohort_stats_sharded_dev", "plda_score_matrix_snorm",
             "plda_score_matrix_snorm_dev", "plda_device_bytes_peak"]
    lib = ctypes.CDLL(_native.SO_PATH)
    for n in names:
        assert n in _native.SIGNATURES and hasattr(lib, n), n
    peak = _native.load().plda_device_bytes_peak
    assert peak(1) >= 0 and peak(0) == _native.load().plda_device_bytes_held()


def test_python_surface():
    from liblda.plda import PLDA
    from plda_amd.libplda import MPlda
    for cls, names in ((MPlda, ("cohort_stats", "cohort_stats_dev", "score_matrix_snorm_dev", "score_matrix_asnorm",
                                "score_trials_asnorm", "cohort_stats_sharded_dev")),
                       (PLDA, ("cohort_stats", "score_matrix_asnorm", "score_trials_asnorm"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls.__name__, n)
