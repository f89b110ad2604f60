"""CPU: the model of tests/fit_model.py is sound before tests/test_gpu_fit_edges.py holds the device to it.

  * grid_data is what it says: on the grid, exactly shiftable, skewed, with the singletons and constant columns asked for;
  * both oracles (oracle/plda_oracle.c and oracle/plda_oracle_np.py, class-centred scatter) fitted on exactly shifted rows meet
    the shift identities at the tolerances of tests/test_gpu_fit.py:test_fit_matches_oracle, and agree with each other;
  * the oracle's scatter is the extended-precision one's at every shift;
  * Kaldi's order of the same sums, X^T diag(1 / n) X - M^T M, which the library and both oracles used before, misses those
    tolerances from c = 1024 on -- so the cases expose that defect;
  * plain fp64 NumPy evaluating T x + offset stays inside transform_bound on the GPU test's own inputs: the bound is a property of
    the formula.
"""
import functools

import numpy as np
import pytest

import fit_model as M
from oracle import plda_oracle_np as onp

SCATTER_TOL = 1e-10     # test_fit_matches_oracle: the scatter
MODEL_TOL = 1e-9        # ... W, B, psi, T^T T, T^T Psi T
ITERS = 10


@functools.lru_cache(maxsize=None)
def _data(n, d, k):
    return M.grid_data(n + d + k, n, d, k)


def test_grid_data_is_exactly_shiftable_and_skewed():
    x, y = M.grid_data(3, 500, 7, 30, singles=4, const_cols=(2, 5))
    assert np.array_equal(np.round(x / M.GRID) * M.GRID, x)
    for c in M.SHIFTS:
        M.assert_exact_shift(x, c)
    counts = np.bincount(y.astype(np.int64))
    assert len(counts) == 30 and (counts[:4] == 1).all() and (counts[4:] >= 2).all()
    assert len(np.unique(counts)) >= 8 and counts.max() > 5 * np.median(counts)
    for k in range(30):
        rows = x[y == k]
        assert (rows[:, [2, 5]] == rows[0, [2, 5]]).all() and (k < 4 or rows[:, 0].std() > 0)
    assert (np.diff(y.astype(np.int64)) < 0).any()          # shuffled, not grouped
    ones, _ = M.grid_data(4, 40, 5, 40, singles=40)
    assert ones.shape == (40, 5)
    with pytest.raises(AssertionError):
        M.assert_exact_shift(x + 2.0 ** -40, 131072.0)


def _fit_errors(fit, stats, x, y, c, want, want_st):
    got, st = fit(x + c, y, ITERS), stats(x + c, y)
    tt = lambda m: m["transform"].T @ m["transform"]
    tpt = lambda m: m["transform"].T @ np.diag(m["psi"]) @ m["transform"]
    t = got["transform"]
    return dict(counts=float(not np.array_equal(st["counts"], want_st["counts"])),
                scatter=M.rel(st["scatter"], want_st["scatter"]),
                means=float((np.abs(st["means"] - want_st["means"]) / M.mean_bound(st["counts"], np.abs(x + c).max())).max()),
                sum=M.rel(st["sum"], want_st["sum"]),
                mean=float(np.abs(got["mean"] - want["mean"]).max() / M.model_mean_bound(st["counts"], np.abs(x + c).max())),
                W=M.rel(got["W"], want["W"]), B=M.rel(got["B"], want["B"]),
                psi=float(np.abs(got["psi"] - want["psi"]).max() / want["psi"].max()),
                TtT=M.rel(tt(got), tt(want)), TtPsiT=M.rel(tpt(got), tpt(want)),
                offset=float(np.abs(got["offset"] + t @ got["mean"]).max() / (np.abs(t) @ np.abs(got["mean"])).max()))


def _assert_identities(e):
    assert e["counts"] == 0.0
    assert e["scatter"] < SCATTER_TOL, e
    # the oracles divide the class sum (correctly rounded, one rounding) and add c to a mean that is not on the grid (one more)
    assert e["means"] <= 3.0 and e["mean"] <= 1.0 and e["sum"] < 1e-12, e
    assert max(e["W"], e["B"], e["psi"], e["TtT"], e["TtPsiT"]) < MODEL_TOL, e
    assert e["offset"] <= 1e-12, e


@pytest.mark.parametrize("c", M.SHIFTS)
@pytest.mark.parametrize("n,d,k", M.FIT_SHAPES)
def test_both_oracles_meet_the_shift_identities(oracle, n, d, k, c):
    x, y = _data(n, d, k)
    M.assert_exact_shift(x, c)
    for mod in (oracle, _NumpyOracle):
        _assert_identities(_fit_errors(mod.fit, mod.stats, x, y, c, M.expected_fit(mod, x, y, c, ITERS), M.expected_stats(mod, x, y, c)))


class _NumpyOracle:
    """oracle/plda_oracle_np.py behind the C binding's two calls."""
    stats = staticmethod(onp.stats)

    @staticmethod
    def fit(x, y, iters):
        return onp.fit(x, y, iters, return_wb=True)


@pytest.mark.parametrize("n,d,k", M.FIT_SHAPES)
def test_c_and_numpy_oracles_agree_on_shifted_rows(oracle, n, d, k):
    x, y = _data(n, d, k)
    c = 8192.0
    a, b = oracle.fit(x + c, y, ITERS), onp.fit(x + c, y, ITERS, return_wb=True)
    sa, sb = oracle.stats(x + c, y), onp.stats(x + c, y)
    assert np.array_equal(sa["counts"], sb["counts"])
    assert M.rel(sa["scatter"], sb["scatter"]) < 1e-12 and M.rel(sa["means"], sb["means"]) < 1e-15
    assert M.rel(a["W"], b["W"]) < MODEL_TOL and M.rel(a["B"], b["B"]) < MODEL_TOL
    assert np.abs(a["psi"] - b["psi"]).max() < MODEL_TOL * b["psi"].max()
    assert M.rel(a["transform"].T @ a["transform"], b["transform"].T @ b["transform"]) < MODEL_TOL


@pytest.mark.parametrize("d,n,k", M.STAT_SHAPES)
def test_oracle_scatter_is_the_extended_precision_one_at_every_shift(d, n, k):
    x, y = _data(n, d, k)
    want = M.scatter_longdouble(x, y)
    for c in M.SHIFTS:
        got = onp.stats(x + c, y)["scatter"]
        assert float(np.abs(got - want).max() / np.abs(want).max()) < 1e-12, c
        assert np.abs(M.means_longdouble(x + c, y) - (M.means_longdouble(x, y) + c)).max() <= 2.0 ** -64 * (8.0 + c)


@pytest.mark.parametrize("n,d,k", M.FIT_SHAPES)
def test_uncentred_sums_miss_the_identities_from_shift_1024_on(n, d, k):
    """What tests/test_gpu_fit_edges.py is for: the statistics in Kaldi's order lose about eps (c / spread)^2.  At c = 0 the
    old formula is as good as the new one; from c = 1024 on it misses the scatter's 1e-10 and the model's 1e-9."""
    x, y = _data(n, d, k)
    want, want_st = onp.fit(x, y, ITERS, return_wb=True), onp.stats(x, y)
    rows = []
    for c in M.SHIFTS:
        got, st = M.fit_uncentred(x + c, y, ITERS), M.stats_uncentred(x + c, y)
        e = (M.rel(st["scatter"], want_st["scatter"]), M.rel(got["W"], want["W"]),
             float(np.abs(got["psi"] - want["psi"]).max() / want["psi"].max()))
        rows.append((c, e))
        if c == 0:
            assert e[0] < SCATTER_TOL and e[1] < MODEL_TOL and e[2] < MODEL_TOL, e
        else:
            assert e[0] > SCATTER_TOL and e[1] > MODEL_TOL and e[2] > MODEL_TOL, (c, e)
    for c, e in rows:
        print("uncentred sums, %d x %d, K = %d, shift %6d: scatter %.1e  W %.1e  psi %.1e" % ((n, d, k, int(c)) + e))


@pytest.mark.parametrize("d", [33, 209])
def test_fp64_numpy_transform_stays_inside_the_bound(d):
    """y = T x + offset in plain fp64 (NumPy's order of summation, BLAS fused multiply-adds or not) on the inputs of
    test_gpu_fit_edges.py:test_transform_on_offset_rows: inside transform_bound, and not by orders of magnitude at the large
    shifts -- the bound measures the formula's cancellation, it is not a blanket."""
    x, n = M.transform_rows(d, 257, d)
    worst = []
    for c in M.SHIFTS:
        mean, t, psi = M.transform_model(d + 1, d, c)
        offset = -(t @ mean)
        model = dict(mean=mean, transform=t, psi=psi, offset=offset)
        got = onp.transform_ivector(model, x + c, n)
        want, _, _ = M.transform_longdouble(t, offset, psi, x + c, n)
        bound = M.transform_bound(t, offset, psi, x + c, n)
        ratio = float((np.abs(got - want) / bound).max())
        worst.append(ratio)
        assert ratio <= 1.0, (c, ratio)
    assert worst[-1] > 1e-4, worst
