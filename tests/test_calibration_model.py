"""CPU: the host model of the score calibration (tests/calibration_model.py) against facts that do not depend on it, and
the surface of the feature (C ABI names, ctypes table, Python methods).  The GPU tests (tests/test_gpu_calibration.py) hold
the device code to this model."""
import math
import warnings

import numpy as np
import pytest

import calibration_model as cm

U = 2.0 ** -53


def _gauss(seed, npos, nneg, m, v, k=1.0, d=0.0):
    rng = np.random.default_rng(seed)
    pos = (k * (m + math.sqrt(v) * rng.standard_normal(npos)) + d).astype(np.float32)
    neg = (k * (-m + math.sqrt(v) * rng.standard_normal(nneg)) + d).astype(np.float32)
    return pos, neg


def _F(pos, neg, a, b, prior):
    return cm.objective(cm.pass_record(pos, neg, a, b + cm.logit(prior)), prior)


@pytest.mark.parametrize("prior", [0.5, 0.05])
@pytest.mark.parametrize("point", [(0.0, 0.0), (1.0, 0.0), (0.6, -0.3)])
def test_gradient_and_hessian_equal_finite_differences(point, prior):
    """Central differences with step h = 1e-4 in either parameter.  Their own error: truncation h^2 / 6 times the third
    (gradient) or fourth (Hessian, differences of the gradient) derivative of F, which are bounded by max|softplus'''| =
    1 / (6 sqrt 3) resp. max|softplus''''| = 1 / 8 times max(|s|, 1)^3 resp. ^4; rounding 8 u |F| / h resp. 8 u |g| / h."""
    pos, neg = _gauss(3, 4000, 30000, 1.0, 1.5)
    a, b = point
    h = 1e-4
    smax = max(1.0, float(np.abs(np.concatenate([pos, neg])).max()))
    rec = cm.pass_record(pos, neg, a, b + cm.logit(prior))
    F, g, H = cm.objective(rec, prior), cm.gradient(rec, prior), cm.hessian(rec, prior)
    fd_g = np.array([(_F(pos, neg, a + h, b, prior) - _F(pos, neg, a - h, b, prior)) / (2 * h),
                     (_F(pos, neg, a, b + h, prior) - _F(pos, neg, a, b - h, prior)) / (2 * h)])
    bound_g = h * h / 6 * smax ** 3 / (6 * math.sqrt(3)) + 8 * U * abs(F) / h
    assert np.abs(fd_g - g).max() <= bound_g, (fd_g, g, bound_g)

    def grad(a_, b_):
        return cm.gradient(cm.pass_record(pos, neg, a_, b_ + cm.logit(prior)), prior)
    fd_H = np.stack([(grad(a + h, b) - grad(a - h, b)) / (2 * h), (grad(a, b + h) - grad(a, b - h)) / (2 * h)])
    bound_H = h * h / 6 * smax ** 4 / 8 + 8 * U * max(1.0, np.abs(g).max() + smax) / h
    assert np.abs(fd_H - H).max() <= bound_H, (fd_H, H, bound_H)
    assert H[0, 1] == H[1, 0]


def test_zero_map_gives_one_bit_and_fit_cannot_do_worse():
    pos, neg = _gauss(5, 700, 9000, 0.8, 1.0, k=3.0, d=1.0)
    rec = cm.pass_record(pos, neg, 0.0, 0.0)
    assert cm.objective(rec, 0.5) == pytest.approx(math.log(2.0), rel=4 * U)       # F(0, 0; 0.5) = ln 2: Cllr = 1 bit
    assert cm.cllr(pos, neg, 0.0, 0.0) == pytest.approx(1.0, rel=8 * U)
    r = cm.fit(pos, neg)
    assert r["converged"] and not r["separable"]
    assert r["cllr_after"] <= min(1.0, r["cllr_before"])
    assert r["cllr_after"] == pytest.approx(cm.cllr(pos, neg, r["a"], r["b"]), rel=1e-14)
    assert r["passes"] == r["iterations"] + 2          # no rejected trial point on this set; +1 start, +1 Cllr before


@pytest.mark.parametrize("prior", [0.5, 0.1])
def test_affine_equivariance_and_refit(prior):
    """Fitting k s + d gives (a / k, b - a d / k); refitting calibrated scores gives (1, 0).  The transformed scores are
    rounded to fp32 again, which moves each by <= 2^-24 relative: the parameters agree to 1e-5, not to the last bit."""
    pos, neg = _gauss(7, 3000, 40000, 1.2, 2.0)
    r = cm.fit(pos, neg, prior)
    k, d = 8.0, -3.0                                    # a power of two and a small integer: k s + d is exact in fp32 here
    r2 = cm.fit((k * pos.astype(np.float64) + d).astype(np.float32), (k * neg.astype(np.float64) + d).astype(np.float32), prior)
    assert r2["a"] == pytest.approx(r["a"] / k, rel=1e-5)
    assert r2["b"] == pytest.approx(r["b"] - r["a"] * d / k, abs=1e-5)
    r3 = cm.fit((r["a"] * pos.astype(np.float64) + r["b"]).astype(np.float32),
                (r["a"] * neg.astype(np.float64) + r["b"]).astype(np.float32), prior)
    assert r3["a"] == pytest.approx(1.0, abs=1e-5) and r3["b"] == pytest.approx(0.0, abs=1e-5)
    assert r3["cllr_before"] == pytest.approx(r3["cllr_after"], abs=1e-9)


def gaussian_case(seed=11, n=20000, m=1.5, v=2.0):
    """Scores N(+m, v) / N(-m, v), n of each: the LLR is 2 m s / v.  With equal class sizes and prior 0.5, F is the mean
    log-loss over the 2 n trials, so the inverse Fisher information of the logistic model is (2 n H_F)^-1."""
    pos, neg = _gauss(seed, n, n, m, v)
    return pos, neg, 2.0 * m / v


def gaussian_standard_errors(pos, neg, a, b):
    H = cm.hessian(cm.pass_record(pos, neg, a, b), 0.5)
    cov = np.linalg.inv(H * (pos.shape[0] + neg.shape[0]))
    return math.sqrt(cov[0, 0]), math.sqrt(cov[1, 1])


def test_gaussian_scores_recover_the_closed_form_llr():
    """Seed 11, 20 000 + 20 000 trials, m = 1.5, v = 2: a = 1.5, b = 0 within five standard errors (confirmed on the CPU:
    the fit lands within 0.7 of one)."""
    pos, neg, a_true = gaussian_case()
    r = cm.fit(pos, neg)
    se_a, se_b = gaussian_standard_errors(pos, neg, r["a"], r["b"])
    print("a = %.6f (true %.3f, se %.4f), b = %.6f (se %.4f)" % (r["a"], a_true, se_a, r["b"], se_b))
    assert abs(r["a"] - a_true) <= 5 * se_a and abs(r["b"]) <= 5 * se_b
    assert se_a < 0.05 and se_b < 0.05                 # the bound says something


@pytest.mark.parametrize("prior", [0.5, 0.02])
def test_agrees_with_scipy_minimize(prior):
    """BFGS on the same fp64 objective with the model's gradient, gtol = 1e-9 on max|g|: at its solution x_s,
    |x_s - x*| <= |H^-1| |g(x_s)| to first order, so the two answers differ by at most 2 |H^-1|_inf gtol."""
    from scipy.optimize import minimize
    pos, neg = _gauss(13, 5000, 95000, 1.0, 1.3, k=2.0, d=0.5)
    tau = cm.logit(prior)

    def fg(x):
        rec = cm.pass_record(pos, neg, x[0], x[1] + tau)
        return cm.objective(rec, prior), cm.gradient(rec, prior)
    gtol = 1e-9
    res = minimize(fg, np.zeros(2), jac=True, method="BFGS", options={"gtol": gtol, "maxiter": 500})
    assert np.abs(res.jac).max() <= gtol, res
    r = cm.fit(pos, neg, prior)
    H = cm.hessian(cm.pass_record(pos, neg, r["a"], r["b"] + tau), prior)
    bound = 2 * np.abs(np.linalg.inv(H)).sum(axis=1).max() * gtol
    assert abs(res.x[0] - r["a"]) <= bound and abs(res.x[1] - r["b"]) <= bound, (res.x, r, bound)


def test_separable_and_degenerate_inputs():
    rng = np.random.default_rng(2)
    pos, neg = rng.uniform(5, 6, 200).astype(np.float32), rng.uniform(-6, -5, 3000).astype(np.float32)
    r = cm.fit(pos, neg, max_iter=100)
    assert r["separable"] and r["cllr_after"] < 1e-3 and r["passes"] <= 100 + 30 + 2
    same = np.full(50, 1.25, np.float32)
    with pytest.raises(ValueError, match="equal"):
        cm.fit(same, np.full(70, 1.25, np.float32))
    with pytest.raises(ValueError, match="non-finite"):
        cm.fit(np.array([1.0, np.inf], np.float32), np.array([0.0, -1.0], np.float32))
    with pytest.raises(ValueError, match="at least one"):
        cm.fit(np.zeros(0, np.float32), np.array([0.0, -1.0], np.float32))
    with pytest.raises(ValueError, match="prior"):
        cm.fit(pos, neg, prior=1.0)


def test_saturating_pass_is_finite():
    """|y| of a few hundred: the overflow-free forms give finite sums, and terms beyond |y| = 746 vanish."""
    pos, neg = _gauss(17, 500, 5000, 2.0, 1.0, k=100.0)
    rec = cm.pass_record(pos, neg, 1.0, 0.0)
    assert all(np.isfinite(rec[n + c]) for n in cm.SUMS for c in ("_t", "_n"))
    far = cm.pass_record(np.float32([900.0]), np.float32([-900.0]), 1.0, 0.0)
    assert far["L_t"] == 0.0 and far["L_n"] == 0.0 and far["H0_t"] == 0.0 and far["G0_n"] == 0.0


def test_counts_threshold_convention_and_dcf():
    pos = np.float32([-1.0, 0.0, 0.5, 2.0])
    neg = np.float32([-3.0, 0.0, 0.5, 0.25, 1.0])
    rec = cm.pass_record(pos, neg, 1.0, 0.0, theta=0.5)
    assert (rec["Np"], rec["Nn"], rec["miss"], rec["fa"]) == (4, 5, 2, 2)         # target < theta; non-target >= theta
    assert (rec["min_t"], rec["max_t"], rec["min_n"], rec["max_n"]) == (-1.0, 2.0, -3.0, 1.0)
    assert cm.act_dcf(pos, neg, 0.5) == pytest.approx((0.5 * 1 / 4 + 0.5 * 4 / 5) / 0.5)      # theta = 0: one miss, four false alarms
    assert cm.bayes_theta(0.5) == 0.0 and cm.bayes_theta(0.1, a=2.0, b=1.0) == pytest.approx((math.log(9.0) - 1.0) / 2.0)


def test_matrix_labelling_equals_the_lists():
    rng = np.random.default_rng(23)
    es, ts = rng.integers(0, 7, 40), rng.integers(0, 7, 90)
    S = rng.standard_normal((40, 90)).astype(np.float32)
    pos, neg = cm.split(S, es, ts)
    a = cm.pass_matrix(S, es, ts, 0.7, -0.2, 0.1, rows=16)
    b = cm.pass_record(pos, neg, 0.7, -0.2, 0.1)
    for k in ("Np", "Nn", "miss", "fa", "min_t", "max_n"):
        assert a[k] == b[k]
    for n in cm.SUMS:
        assert a[n + "_t"] == pytest.approx(b[n + "_t"], rel=1e-14) and a[n + "_n"] == pytest.approx(b[n + "_n"], rel=1e-14)


def test_apply_map_is_one_rounding():
    from fractions import Fraction
    rng = np.random.default_rng(29)
    s = (rng.standard_normal(2000) * 50).astype(np.float32)
    a, b = 0.0371234567891234, -1.23456789012345
    got = cm.apply_map(s, a, b)
    for x, y in zip(s[:300], got[:300]):
        exact = Fraction(a) * Fraction(float(x)) + Fraction(b)
        f64 = float(exact)                                   # Fraction -> float rounds correctly
        assert np.float32(f64) == y


# ------------------------------------------------------------------------------------------ the surface of the feature
NAMES = ["plda_calib_pass_matrix_dev", "plda_calib_pass_lists", "plda_score_calib_pass_dev", "plda_calib_fit_matrix_dev",
         "plda_calib_fit_lists", "plda_score_calib_fit_dev", "plda_affine_map_dev"]


def test_abi_declares_and_exports_the_calibration_entry_points():
    import ctypes
    from plda_amd import _native
    lib = ctypes.CDLL(_native.SO_PATH)
    for n in NAMES:
        assert n in _native.SIGNATURES and hasattr(lib, n), n
    assert _native.load().plda_abi_version() == 2


def test_record_layout_matches_the_header():
    from plda_amd import calibration as CB
    assert CB.RECORD_DTYPE.itemsize == 12 * 8 + 5 * 8 + 4 * 4 and CB.RECORD_DTYPE.fields["np"][1] == 96
    assert CB.RECORD_DTYPE.fields["min_t"][1] == 136
    assert CB.FIT_DTYPE.itemsize == 6 * 8 + 4 * 4 and CB.FIT_DTYPE.fields["iterations"][1] == 48


def test_python_surface():
    import plda_amd
    from liblda.plda import PLDA
    from plda_amd import calibration as CB
    from plda_amd.libplda import MPlda
    assert plda_amd.Calibration is CB.Calibration
    for n in ("pass_from_lists", "pass_from_matrix_dev", "pass_from_operands_dev", "fit_from_lists", "fit_from_matrix_dev",
              "fit_from_operands_dev", "cllr", "act_dcf", "apply_dev"):
        assert callable(getattr(CB, n)), n
    for cls in (MPlda, PLDA):
        assert callable(getattr(cls, "calibrate")), cls.__name__
    cal = CB.Calibration(2.0, -1.0, 0.3)
    assert np.array_equal(cal(np.float32([0.5, 1.0])), [0.0, 1.0]) and cal.prior == 0.3
    rec = {"Np": 4, "Nn": 5, "miss": 1, "fa": 3, "L_t": 4 * math.log(2.0), "L_n": 5 * math.log(2.0)}
    assert CB.cllr(rec) == pytest.approx(1.0)
    assert CB.act_dcf(rec, 0.5) == pytest.approx((0.5 * 1 / 4 + 0.5 * 3 / 5) / 0.5)
    assert CB.act_dcf(lambda theta: dict(rec, theta=theta), 0.1, calibration=cal) == pytest.approx((0.1 / 4 + 0.9 * 3 / 5) / 0.1)
    with pytest.raises(ValueError):
        CB.bayes_theta(0.5, calibration=CB.Calibration(-1.0, 0.0))


def test_warnings_for_separable_and_unconverged_fits():
    from plda_amd import calibration as CB
    raw = np.zeros(1, CB.FIT_DTYPE)
    raw["a"], raw["converged"], raw["separable"] = 40.0, 0, 1
    with pytest.warns(RuntimeWarning, match="separable"):
        CB._calibration(raw, 0.5)
    raw["separable"] = 0
    with pytest.warns(RuntimeWarning, match="did not converge"):
        CB._calibration(raw, 0.5)
    raw["converged"] = 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert CB._calibration(raw, 0.5).a == 40.0
