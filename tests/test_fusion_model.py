"""CPU: the host model of the multi-system score fusion (tests/fusion_model.py) against what can be known without a GPU,
and the library's pure Newton step (plda_fusion_newton) against the model's.

  1. at K = 1 the model's record equals calibration_model.pass_record sum for sum;
  2. gradient and Hessian from ONE record agree with central differences of F;
  3. K independent Gaussian systems: the fit recovers a_k = 2 mu_k / sigma_k^2, b = 0 within standard errors;
  4. equivariance: rescaling / shifting one system, permuting systems;
  5. the whole fit driven through plda_fusion_newton on model records matches the model's own fit, `passes` included;
  6. a duplicated and a constant system are refused by name (model and library);
  7. the struct layouts of plda_amd/fusion.py match the header."""
import math
import os
import re

import numpy as np
import pytest

import calibration_model as cm
import fusion_model as fm
from conftest import ROOT


def _systems(seed, npos, nneg, mus, sigmas, scale=None, shift=None):
    """K independent Gaussian systems: class means +/- mu_k, standard deviation sigma_k; K target and K non-target arrays."""
    rng = np.random.default_rng(seed)
    k = len(mus)
    scale, shift = scale or [1.0] * k, shift or [0.0] * k
    pos = [(scale[j] * (mus[j] + sigmas[j] * rng.standard_normal(npos)) + shift[j]).astype(np.float32) for j in range(k)]
    neg = [(scale[j] * (-mus[j] + sigmas[j] * rng.standard_normal(nneg)) + shift[j]).astype(np.float32) for j in range(k)]
    return pos, neg


def _F(pos, neg, x, prior):
    return fm.objective(fm.pass_record(pos, neg, x[1:], x[0] + fm.logit(prior)), prior)


# ------------------------------------------------------------------------------------------- 1. K = 1 is the calibration
def test_k1_record_equals_the_calibration_model_sum_for_sum():
    pos, neg = _systems(3, 4000, 60000, [1.2], [1.5])
    f = cm.fit(pos[0], neg[0], 0.3)
    for a, c, theta in ((1.0, 0.0, 0.25), (f["a"], f["b"] + cm.logit(0.3), -0.4)):
        got = fm.pass_record(pos, neg, [a], c, theta)
        ref = cm.pass_record(pos[0], neg[0], a, c, 0.0)
        for cls in ("t", "n"):
            assert got["L_" + cls] == ref["L_" + cls]
            assert got["G_" + cls][0] == ref["G0_" + cls] and got["G_" + cls][1] == ref["G1_" + cls]
            assert [got["H_" + cls][i] for i in range(3)] == [ref["H0_" + cls], ref["H1_" + cls], ref["H2_" + cls]]
            assert got["abs"]["H_" + cls][2] == ref["abs"]["H2_" + cls]
        assert (got["Np"], got["Nn"], got["nonfinite"]) == (ref["Np"], ref["Nn"], ref["nonfinite"])
        assert got["smin"][0] == min(ref["min_t"], ref["min_n"]) and got["smax"][0] == max(ref["max_t"], ref["max_n"])
        # miss / fa are counted on the chain value, not on the raw score
        y_t, y_n = fm.chain(pos, [a], c), fm.chain(neg, [a], c)
        assert got["miss"] == int((y_t < theta).sum()) and got["fa"] == int((y_n >= theta).sum())
        assert got["ymin_t"] == y_t.min() and got["ymax_n"] == y_n.max()


def test_chain_exact_is_the_fma_chain():
    rng = np.random.default_rng(5)
    S = [(rng.standard_normal(300) * 10.0 ** rng.integers(-3, 4)).astype(np.float32) for _ in range(4)]
    a = rng.standard_normal(4) * 3.0
    y, ye = fm.chain(S, a, 0.37), fm.chain_exact(S, a, 0.37)
    # np.longdouble rounds twice: at most one ulp of the step from the correctly rounded chain, K steps
    assert np.all(np.abs(y - ye) <= 4 * 2.0 ** -52 * (abs(0.37) + sum(abs(ak) * np.abs(s.astype(np.float64)) for ak, s in zip(a, S))))
    one = fm.chain_exact([np.float32([3.0])], [1.0 / 3.0], 2.0 ** -60)
    assert one[0] == 1.0 + 2.0 ** -52 or one[0] == 1.0      # (1/3 rounded) * 3 + 2^-60, rounded once
    from fractions import Fraction
    assert one[0] == float(Fraction(1.0 / 3.0) * 3 + Fraction(2.0 ** -60))


# ------------------------------------------------------------------------------------------- 2. derivatives
@pytest.mark.parametrize("prior", [0.5, 0.05])
@pytest.mark.parametrize("k", [1, 3])
def test_gradient_and_hessian_equal_finite_differences(k, prior):
    """Central differences with step h = 1e-4: truncation h^2 / 6 times a third derivative of O(1) on these scores, and
    rounding u F / h (resp. 4 u F / h^2 for the second difference of F, which is why the Hessian is checked as the difference
    of GRADIENTS): bounds 1e-7 and 1e-6."""
    pos, neg = _systems(7 + k, 1500, 9000, [1.0, 0.6, 0.8][:k], [1.2, 0.9, 1.4][:k])
    x = np.array([0.2, 0.5, -0.3, 0.4][:k + 1])
    rec = fm.pass_record(pos, neg, x[1:], x[0] + fm.logit(prior))
    g, H = fm.gradient(rec, prior), fm.hessian(rec, prior)
    h = 1e-4
    for j in range(k + 1):
        e = np.zeros(k + 1)
        e[j] = h
        assert abs((_F(pos, neg, x + e, prior) - _F(pos, neg, x - e, prior)) / (2 * h) - g[j]) <= 1e-7
        gp = fm.gradient(fm.pass_record(pos, neg, (x + e)[1:], (x + e)[0] + fm.logit(prior)), prior)
        gm = fm.gradient(fm.pass_record(pos, neg, (x - e)[1:], (x - e)[0] + fm.logit(prior)), prior)
        assert np.all(np.abs((gp - gm) / (2 * h) - H[:, j]) <= 1e-6)
    assert np.array_equal(H, H.T) and np.all(np.linalg.eigvalsh(H) > 0)


# ------------------------------------------------------------------------------------------- 3. Gaussian closed form
def _standard_errors(pos, neg, f):
    rec = fm.pass_record(pos, neg, f["a"], f["b"])
    cov = np.linalg.inv(fm.hessian(rec, 0.5) * (pos[0].shape[0] + neg[0].shape[0]))
    return np.sqrt(np.diag(cov))                      # (b, a_0 ..), as gaussian_standard_errors of the calibration tests


def test_independent_gaussian_systems_recover_the_closed_form():
    """Independent systems with class means +/- mu_k and variance sigma_k^2: the LLR is sum_k 2 mu_k s_k / sigma_k^2.  Equal
    class sizes, prior 0.5 = the data's."""
    mus, sigmas = [0.9, 0.5, 0.7], [1.3, 0.8, 1.6]
    pos, neg = _systems(11, 20000, 20000, mus, sigmas)
    f = fm.fit(pos, neg)
    se = _standard_errors(pos, neg, f)
    true = [2.0 * m / s ** 2 for m, s in zip(mus, sigmas)]
    print("b = %.4f (se %.4f); a = %s, true %s, se %s" % (f["b"], se[0], f["a"], true, se[1:]))
    assert f["converged"] and not f["separable"]
    assert abs(f["b"]) <= 5 * se[0]
    for j in range(3):
        assert abs(f["a"][j] - true[j]) <= 5 * se[1 + j]
    assert np.all(se < 0.05)                            # the bound says something


# ------------------------------------------------------------------------------------------- 4. equivariance
def test_equivariance_under_units_shifts_and_permutations():
    mus, sigmas = [1.0, 0.4, 0.7], [1.2, 0.7, 1.5]
    pos, neg = _systems(17, 3000, 30000, mus, sigmas)
    prior = 0.1
    f = fm.fit(pos, neg, prior)
    # system 1 in other units: s' = 250 s - 20  =>  a' = a / 250, b' = b + 20 a / 250 (= b + 20 a')
    k, d = 250.0, -20.0
    pos2 = [pos[0], (k * pos[1].astype(np.float64) + d).astype(np.float32), pos[2]]
    neg2 = [neg[0], (k * neg[1].astype(np.float64) + d).astype(np.float32), neg[2]]
    f2 = fm.fit(pos2, neg2, prior)
    # (the fp32 rounding of s' perturbs the data by 6e-8 relative: the optimum moves by that order)
    assert f2["a"][1] == pytest.approx(f["a"][1] / k, rel=1e-5)
    assert f2["a"][0] == pytest.approx(f["a"][0], rel=1e-5) and f2["a"][2] == pytest.approx(f["a"][2], rel=1e-5)
    assert f2["b"] == pytest.approx(f["b"] - f["a"][1] * d / k, abs=1e-5)
    assert f2["objective"] == pytest.approx(f["objective"], rel=1e-6)
    perm = [2, 0, 1]
    f3 = fm.fit([pos[i] for i in perm], [neg[i] for i in perm], prior)
    assert np.allclose(f3["a"], f["a"][perm], rtol=1e-7, atol=0) and f3["b"] == pytest.approx(f["b"], abs=1e-8)
    assert f3["objective"] == pytest.approx(f["objective"], rel=1e-12)


# ------------------------------------------------------------------------------------------- 5. the library's Newton step
@pytest.mark.parametrize("prior", [0.5, 0.05])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_fit_driven_through_the_librarys_newton_step(k, prior):
    from plda_amd import fusion as FU
    mus = [0.9, 0.5, 0.7, 0.3, 0.6, 0.4, 0.2, 0.8][:k]
    sigmas = [1.3, 0.8, 1.6, 1.0, 1.1, 0.9, 1.2, 1.4][:k]
    scale = [1.0, 200.0, 0.01, 1.0, 30.0, 1.0, 1.0, 5.0][:k]
    shift = [0.0, 0.0, 0.0, -20.0, 0.0, 3.0, 0.0, 0.0][:k]
    pos, neg = _systems(23 + k, 800, 6000, mus, sigmas, scale, shift)
    ref = fm.fit(pos, neg, prior)
    got = fm.fit(pos, neg, prior, step=FU.newton)
    assert got["passes"] == ref["passes"] and got["iterations"] == ref["iterations"] and got["converged"] and ref["converged"]
    assert np.allclose(got["a"], ref["a"], rtol=1e-9, atol=0) and got["b"] == pytest.approx(ref["b"], rel=1e-9, abs=1e-12)
    assert got["lambda2"] <= 1e-18
    # one step compared directly, at the start
    rec = fm.pass_record(pos, neg, np.zeros(k), fm.logit(prior))
    F, d, lam2 = FU.newton(rec, prior)
    Fm, dm, lm = fm.newton(rec, prior)
    assert F == Fm and np.allclose(d, dm, rtol=1e-12, atol=0) and lam2 == pytest.approx(lm, rel=1e-12)
    # and against a plain solve of the unscaled system
    g, H = fm.gradient(rec, prior), fm.hessian(rec, prior)
    assert np.allclose(d, -np.linalg.solve(H, g), rtol=1e-8, atol=0) and lam2 == pytest.approx(g @ np.linalg.solve(H, g), rel=1e-8)


# ------------------------------------------------------------------------------------------- 6. refusals
def test_duplicated_and_constant_systems_are_refused_by_name():
    from plda_amd import fusion as FU
    from plda_amd._native import PLDA_E_INVAL, PldaError
    pos, neg = _systems(31, 500, 4000, [1.0, 0.5], [1.0, 1.0])
    dup_p, dup_n = [pos[0], pos[1], pos[0]], [neg[0], neg[1], neg[0]]
    with pytest.raises(ValueError, match="pivot of system 2"):
        fm.fit(dup_p, dup_n)
    rec = fm.pass_record(dup_p, dup_n, np.zeros(3), 0.0)
    with pytest.raises(PldaError, match="pivot of system 2") as ei:
        FU.newton(rec, 0.5)
    assert ei.value.code == PLDA_E_INVAL
    # an affine copy is a duplicate too: 3 s_0 - 2 is exact in fp32 for these small values only up to rounding, so the pivot is
    # tiny but not zero; it is far below 1e-12 all the same
    aff_p = [pos[0], (3.0 * pos[0].astype(np.float64) - 2.0).astype(np.float32)]
    aff_n = [neg[0], (3.0 * neg[0].astype(np.float64) - 2.0).astype(np.float32)]
    with pytest.raises(ValueError, match="pivot of system 1"):
        fm.fit(aff_p, aff_n)
    const_p, const_n = [pos[0], np.full(500, 2.5, np.float32)], [neg[0], np.full(4000, 2.5, np.float32)]
    with pytest.raises(ValueError, match="system 1 is constant"):
        fm.fit(const_p, const_n)
    # the step alone sees the constant system as a pivot (it has no smin / smax rule): still named
    rec = fm.pass_record(const_p, const_n, np.zeros(2), 0.0)
    with pytest.raises(PldaError, match="pivot of system 1"):
        FU.newton(rec, 0.5)
    with pytest.raises(PldaError):
        FU.newton(rec, 1.0)                                # prior outside (0, 1)


# ------------------------------------------------------------------------------------------- 7. layouts and surface
def test_struct_layouts_match_the_header():
    from plda_amd import fusion as FU
    text = open(os.path.join(ROOT, "include", "plda_hip.h")).read()
    kmax = int(re.search(r"#define PLDA_FUSION_MAX_SYSTEMS (\d+)", text).group(1))
    assert kmax == FU.MAX_SYSTEMS == 8
    nsum = 1 + (kmax + 1) + (kmax + 1) * (kmax + 2) // 2
    assert FU.SUMS_DTYPE.itemsize == 8 * nsum
    assert FU.RECORD_DTYPE.itemsize == 2 * 8 * nsum + 4 * 8 + 5 * 8 + 2 * 4 * kmax + 2 * 4 == 1024
    assert FU.RECORD_DTYPE.fields["ymin"][1] == 16 * nsum and FU.RECORD_DTYPE.fields["np"][1] == 16 * nsum + 32
    assert FU.RECORD_DTYPE.fields["smin"][1] == 16 * nsum + 72 and FU.RECORD_DTYPE.fields["n_systems"][1] == 1016
    assert FU.FIT_DTYPE.itemsize == 8 * kmax + 4 * 8 + 4 * 4 and FU.FIT_DTYPE.fields["iterations"][1] == 8 * kmax + 32
    # field order of the header's structs
    body = re.search(r"typedef struct plda_fusion_fit \{(.*?)\} plda_fusion_fit;", text, re.S).group(1)
    order = [body.index(n) for n in ("a[", " b;", "objective", "cllr_after", "lambda2", "iterations")]
    assert order == sorted(order)
    # a round trip through the dict form
    rec = fm.pass_record(*_systems(2, 50, 60, [1.0, 0.5], [1.0, 1.0]), a=[0.5, -0.25], c=0.1)
    back = FU._record(FU.record_to_raw(rec))
    assert back["K"] == 2 and back["Np"] == 50 and np.array_equal(back["H_t"], rec["H_t"]) and back["L_n"] == rec["L_n"]
    assert np.array_equal(back["smin"], rec["smin"]) and back["ymax_t"] == rec["ymax_t"]


def test_python_surface():
    import plda_amd
    from liblda.plda import PLDA
    from plda_amd import fusion as FU
    from plda_amd.libplda import MPlda
    assert plda_amd.Fusion is FU.Fusion
    for n in ("pass_from_matrices_dev", "pass_from_lists", "fit_from_matrices_dev", "fit_from_lists", "apply_dev", "objective", "cllr",
              "act_dcf", "newton"):
        assert callable(getattr(FU, n)), n
    for cls in (MPlda, PLDA):
        assert callable(getattr(cls, "fuse")) and callable(getattr(cls, "score_matrix_fused")), cls.__name__
    f = FU.Fusion([2.0, -1.0], 0.5, 0.3)
    s = [np.float32([1.0, 2.0]), np.float32([3.0, 5.0])]
    assert np.array_equal(f(s), [0.5 + 2.0 - 3.0, 0.5 + 4.0 - 5.0]) and f.n_systems == 2
    with pytest.raises(ValueError):
        FU.Fusion(np.zeros(9), 0.0)
    rec = {"Np": 4, "Nn": 10, "L_t": 2.0, "L_n": 5.0, "miss": 1, "fa": 2}
    assert FU.objective(rec, 0.5) == 0.5 / 4 * 2.0 + 0.5 / 10 * 5.0 and FU.cllr(rec) == FU.objective(rec, 0.5) / math.log(2.0)
    assert FU.act_dcf(rec, 0.5) == (0.5 * 1 / 4 + 0.5 * 2 / 10) / 0.5
