"""tests/lda_model.py -- what the LDA of csrc/lda.hip must compute where its kernels can go wrong, stated on the CPU so that the
statement does not share a weak step with the code under test.

    exact_shift_case(n, d, k, c, seed)   data on the grid 2^-20 and a power-of-two shift c: X + c is exact in fp64, so the model of
                                         the shifted data is known from the model of the unshifted data by identities, not by a fit
    expected_at_shift(X, y, solver, priors, c)
                                         oracle/lda_oracle_np.fit on the UNSHIFTED data (where centred and uncentred scatter agree to
                                         rounding), carried across the shift:
                                           svd    coef, scalings, decision values, probabilities unchanged; means' = means + c,
                                                  xbar' = xbar + c, intercept' = intercept - c coef.sum(1)
                                           eigen  scalings, explained-variance ratio unchanged; coef' = (means + c) E E^T
                                           lsqr   coef' = coef + c (Sw^-1 1)^T, Sw the centred within-class covariance
                                           eigen, lsqr: intercept' = -0.5 means'_k . coef'_k + log p_k, their definition
    fit_uncentred(X, y, solver, priors)  the scatter formulas the library used before it centred its rows (differences of uncentred
                                         sums), in NumPy: tests/test_lda_model.py shows that the cases here expose their loss
    log_softmax / logistic / one_vs_rest the row functions of lda_row_kernel in np.longdouble
    gamma(n), dot_bound(x, w, b)         the rounding bound of a length-n dot product in ANY summation order (Higham, Accuracy and
                                         Stability of Numerical Algorithms, section 3.1): |fl(x.w) - x.w| <= gamma_n sum |x_d w_d|,
                                         gamma_n = n u / (1 - n u), u = 2^-53; a fused multiply-add only removes roundings
"""
import numpy as np

from oracle import lda_oracle_np as lo

U = 2.0 ** -53
GRID = 2.0 ** -20
NT = 67            # test rows: more than one wave of rows, not a multiple of any tile


def _quantise(a):
    return np.round(a / GRID) * GRID


def exact_shift_case(n, d, k, c, seed):
    """-> (X, y, Xt) UNSHIFTED, on the grid 2^-20; labels sparse and not zero-based; every class has at least two rows (the
    reference's empirical_covariance cannot take a single row).  Asserts that the shift by c loses nothing."""
    assert n >= 2 * k and (c == 0 or (c > 0 and 2.0 ** int(np.log2(c)) == c))
    rng = np.random.default_rng(seed)
    dense = np.concatenate([np.arange(k), np.arange(k), rng.integers(0, k, n - 2 * k)])
    rng.shuffle(dense)
    y = dense * 3 + 11
    centres = 0.5 * rng.standard_normal((k, d))
    X = _quantise(rng.random((n, d)) + centres[dense])
    Xt = _quantise(rng.random((NT, d)) + centres[rng.integers(0, k, NT)])
    for a in (X, Xt):
        assert np.array_equal((a + c) - c, a)
    return X, y, Xt


def expected_at_shift(X, y, solver, priors, c):
    """The model of (X + c, y), from the centred oracle on X.  Keys as lda_oracle_np.fit returns them."""
    m = lo.fit(X, y, solver, priors)
    out = dict(m)
    means = m["means"] + c
    out["means"] = means
    if solver == "svd":
        out["xbar"] = m["xbar"] + c
        out["intercept"] = m["intercept"] - c * m["coef"].sum(1)
        return out
    if solver == "eigen":
        e = m["scalings"]
        out["coef"] = means @ e @ e.T
    else:
        _, dense, counts, mu = lo.class_stats(X, y)
        sw = lo.within_cov(np.asarray(X, np.float64), dense, counts, mu, m["priors"])
        out["coef"] = m["coef"] + c * np.linalg.solve(sw, np.ones(sw.shape[0]))[None, :]
    out["intercept"] = -0.5 * np.einsum("kd,kd->k", means, out["coef"]) + np.log(m["priors"])
    return out


def _eigh_desc(a):
    lam, v = np.linalg.eigh(0.5 * (a + a.T))
    return lam[::-1], v[:, ::-1]


def fit_uncentred(X, y, solver, priors=None):
    """lda_oracle_np.fit with every scatter matrix a difference of uncentred sums (S = X^T X - sum n_k m_k m_k^T,
    Sw = X^T diag(p/n) X - sum p_k m_k m_k^T, St = X^T X / N - mu mu^T) and the svd solver through the two Gram matrices."""
    X = np.asarray(X, np.float64)
    n, d = X.shape
    classes, dense, counts, means = lo.class_stats(X, y)
    k = len(classes)
    p = lo.resolve_priors(counts, priors)
    out = dict(classes=classes, priors=p, means=means, solver=solver)
    if solver == "svd":
        xbar = p @ means
        s = X.T @ X - (means * counts[:, None]).T @ means
        var = np.diag(s) / n
        std = np.sqrt(np.where(var > 0, var, 0.0))
        std[std == 0] = 1.0
        fac = 1.0 / (n - k)
        lam, v = _eigh_desc(fac * s / np.outer(std, std))
        s1 = np.sqrt(np.maximum(lam, 0.0))
        r1 = int((s1 > lo.TOL).sum())
        scal1 = (v[:, :r1] / std[:, None]) / s1[:r1]
        cen = (np.sqrt(n * p * fac)[:, None] * (means - xbar)) @ scal1
        lam2, v2 = _eigh_desc(cen.T @ cen)
        s2 = np.sqrt(np.maximum(lam2, 0.0))
        r2 = int((s2 > lo.TOL * s2[0]).sum())
        scalings = scal1 @ v2[:, :r2]
        proj = (means - xbar) @ scalings
        coef = proj @ scalings.T
        out.update(xbar=xbar, scalings=scalings, coef=coef,
                   intercept=-0.5 * (proj ** 2).sum(1) + np.log(p) - xbar @ coef.T)
        return out
    w = (p / counts)[dense]
    sw = (X * w[:, None]).T @ X - (means * p[:, None]).T @ means
    if solver == "eigen":
        from scipy.linalg import eigh
        mu = X.mean(0)
        st = X.T @ X / n - np.outer(mu, mu)
        evals, evecs = eigh(st - sw, sw)
        evecs = evecs[:, np.argsort(evals)[::-1]]
        evecs = evecs / np.linalg.norm(evecs, axis=0)
        coef = means @ evecs @ evecs.T
        out.update(scalings=evecs, coef=coef, explained_variance_ratio=np.sort(evals / evals.sum())[::-1])
    else:
        coef = np.linalg.lstsq(sw, means.T, rcond=None)[0].T
        out.update(coef=coef)
    out["intercept"] = -0.5 * np.einsum("kd,kd->k", means, coef) + np.log(p)
    return out


# ---- the row functions of lda_row_kernel (modes 1, 2, 3), in extended precision ----
def log_softmax(v):
    v = np.asarray(v, np.longdouble)
    z = v - v.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


def logistic(v):
    v = np.asarray(v, np.longdouble)
    return 1 / (1 + np.exp(-v))


def one_vs_rest(v):
    p = logistic(v)
    return p / p.sum(axis=1, keepdims=True)


# ---- rounding bounds ----
def gamma(n):
    return n * U / (1.0 - n * U)


def dot_bound(x, w, b):
    """x [N, D], w [K, D], b [K] -> [N, K]: gamma_D (sum_d |x_nd w_kd| + |b_k|), in extended precision."""
    x, w, b = (np.abs(np.asarray(a, np.longdouble)) for a in (x, w, b))
    return gamma(x.shape[1]) * (x @ w.T + b)


def exact_decision(x, w, b):
    """x w^T + b in extended precision (64-bit significand: 2^-11 of an fp64 rounding per operation)."""
    x, w, b = (np.asarray(a, np.longdouble) for a in (x, w, b))
    return x @ w.T + b


def rel(a, b):
    """max |a - b| / max |b|, the measure of tests/test_gpu_lda.py."""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def align_columns(s, r):
    """|<s_j, r_j>| of unit columns: 1 where they are equal up to sign."""
    return np.abs((np.asarray(s) * np.asarray(r)).sum(0))
