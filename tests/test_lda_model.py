"""CPU: the LDA model of tests/lda_model.py is sound before tests/test_gpu_lda_edges.py holds the device to it.

  * the oracle with centred scatter (oracle/lda_oracle_np.py) still reproduces the reference's own outputs
    (tests/golden/lda_*.npz), by the assertions of tests/test_lda_oracle.py;
  * fitted on exactly shifted data it meets the shift identities to 1e-10 relative (it measures 5e-12 or better; a factor 20);
  * the uncentred scatter formulas the library used before miss the same identities by more than 1e-7 at c = 8192, so the
    cases are able to expose that defect;
  * the extended-precision row functions and the dot-product bound are what they say.
"""
import numpy as np
import pytest

import lda_model as M
import test_lda_oracle as TO
from oracle import lda_oracle_np as lo

SHAPES = [(600, 24, 12), (900, 40, 60)]          # K - 1 < D and K - 1 >= D (eigen coef well defined only in the second)
IDENTITY = 1e-10
EXPOSED = 1e-7


@pytest.mark.parametrize("path", TO.GOLD, ids=[p.split("lda_")[-1][:-4] for p in TO.GOLD])
@pytest.mark.parametrize("solver", ["svd", "eigen", "lsqr"])
def test_centred_oracle_reproduces_the_reference(path, solver):
    TO.test_oracle_matches_reference_outputs(path, solver)


def _priors(k, given):
    return np.random.default_rng(k).random(k) + 0.2 if given else None


def _identity_errors(fit, n, d, k, c, solver, given):
    """Relative misses of `fit` on the shifted data against the model carried across the shift."""
    X, y, Xt = M.exact_shift_case(n, d, k, c, seed=n + d + k)
    pri = _priors(k, given)
    want = M.expected_at_shift(X, y, solver, pri, c)
    got = fit(X + c, y, solver, pri)
    err = dict(means=M.rel(got["means"], want["means"]))
    well_defined = solver != "eigen" or k - 1 >= d
    if well_defined:
        err["coef"] = M.rel(got["coef"], want["coef"])
        err["intercept"] = M.rel(got["intercept"], want["intercept"])
    if solver == "svd":
        err["xbar"] = M.rel(got["xbar"], want["xbar"])
        assert got["scalings"].shape == want["scalings"].shape
        err["scalings"] = M.rel(got["scalings"] @ got["scalings"].T, want["scalings"] @ want["scalings"].T)
        err["log_proba"] = M.rel(lo.predict_log_proba(got, Xt + c), lo.predict_log_proba(want, Xt + c))
        # the decision values themselves do not move with the shift
        err["decision"] = M.rel(lo.decision_function(got, Xt + c), lo.decision_function(lo.fit(X, y, solver, pri), Xt))
    if solver == "eigen":
        err["evr"] = M.rel(got["explained_variance_ratio"], want["explained_variance_ratio"])
        lead = min(k - 1, d)
        err["scalings"] = float(np.abs(M.align_columns(got["scalings"][:, :lead], want["scalings"][:, :lead]) - 1.0).max())
    return err


@pytest.mark.parametrize("given", [False, True], ids=["freq", "priors"])
@pytest.mark.parametrize("c", [0, 256, 8192])
@pytest.mark.parametrize("solver", ["svd", "eigen", "lsqr"])
@pytest.mark.parametrize("n,d,k", SHAPES)
def test_centred_oracle_meets_the_shift_identities(n, d, k, solver, c, given):
    err = _identity_errors(lo.fit, n, d, k, c, solver, given)
    print(n, d, k, solver, c, given, err)
    assert max(err.values()) < IDENTITY, err


@pytest.mark.parametrize("solver,key", [("svd", "coef"), ("eigen", "evr"), ("lsqr", "coef")])
def test_uncentred_formulas_miss_the_identities_at_8192(solver, key):
    err = _identity_errors(M.fit_uncentred, 900, 40, 60, 8192, solver, False)
    print(solver, err)
    assert err[key] > EXPOSED, err
    assert _identity_errors(M.fit_uncentred, 900, 40, 60, 0, solver, False)[key] < IDENTITY     # and are fine unshifted


def test_uncentred_svd_misses_at_the_small_shape_too():
    err = _identity_errors(M.fit_uncentred, 600, 24, 12, 8192, "svd", False)
    print(err)
    assert err["coef"] > EXPOSED and err["log_proba"] > EXPOSED, err


def test_row_functions():
    v = np.array([[0.0, 0.0], [800.0, -800.0], [-3.0, 1.5]])
    ls = M.log_softmax(v)
    assert ls.dtype == np.longdouble
    assert abs(ls[0, 0] + np.log(np.longdouble(2))) < 1e-18
    assert ls[1, 0] == 0 and ls[1, 1] == -1600            # exp(-1600) is below the rounding of 1 even in extended precision
    assert np.abs(np.exp(ls).sum(1) - 1).max() < 1e-18
    p = M.logistic(v)
    assert p[0, 0] == 0.5 and p[1, 0] == 1 and 0 < p[1, 1] < 1e-300      # no underflow to 0 where fp64 has none left
    assert np.abs(p + M.logistic(-v) - 1).max() < 1e-18
    o = M.one_vs_rest(v)
    assert np.abs(o.sum(1) - 1).max() < 1e-18 and o[0, 0] == 0.5
    # against fp64 NumPy where fp64 is unremarkable
    w = np.random.default_rng(0).standard_normal((5, 9))
    model = dict(coef=np.eye(9), intercept=np.zeros(9), classes=np.arange(9))
    assert np.abs(M.log_softmax(w) - lo.predict_log_proba(model, w)).max() < 1e-14
    assert np.abs(M.one_vs_rest(w) - lo.predict_proba(model, w)).max() < 1e-15


def test_dot_bound_holds_for_other_summation_orders():
    rng = np.random.default_rng(1)
    for d in (1, 5, 40, 333):
        x, w, b = rng.standard_normal((7, d)) + 100.0, rng.standard_normal((3, d)), rng.standard_normal(3)
        exact = M.exact_decision(x, w, b)
        bound = M.dot_bound(x, w, b)
        assert bound.shape == (7, 3) and (bound > 0).all()
        forward = x @ w.T + b
        backward = x[:, ::-1] @ w[:, ::-1].T + b
        strided = sum(x[:, i::4] @ w[:, i::4].T for i in range(min(4, d))) + b
        for got in (forward, backward, strided):
            assert (np.abs(got - exact) <= 2 * bound).all()
    assert M.gamma(1) == M.U / (1 - M.U)
