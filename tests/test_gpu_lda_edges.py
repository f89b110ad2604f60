"""GPU: the LDA (plda_amd.lda.LDA, csrc/lda.hip) where its kernels can go wrong, against the CPU model of tests/lda_model.py.

  C1  shift invariance: data on the grid 2^-20 shifted by an exact power of two; the expected model comes from the centred
      oracle on the UNSHIFTED data by identities (lda_model.expected_at_shift), not from a fit that shares the kernel's formula
  C2  lda_row_kernel alone: a model installed with LDA.load whose decision values are exact in fp64, rows across the kernel's
      256-thread stride and its four waves, values hundreds of nats apart, against the row functions in np.longdouble
  C3  transform values for every n_components, and transform(X, j) == transform(X)[:, :j]
  C4  constant, class-constant and duplicated features, D = 1, singleton classes
  C5  a small fit after a large one on the same handle, then a loaded model

Every number below is one of: a tolerance of tests/test_gpu_lda.py (1e-8 relative on coef / intercept / decision values /
probabilities / scalings, 1e-9 on log-probabilities and the explained-variance ratio, 1e-13 on means, 1e-7 on transformed
rows), or a rounding bound built here from u = 2^-53, D and K.
"""
import functools
import os

import numpy as np
import pytest

import lda_model as M
from oracle import lda_oracle_np as lo

pytestmark = pytest.mark.gpu

U = M.U
SHAPES = [(600, 24, 12), (900, 40, 60)]      # K - 1 < D (svd rank 11); K - 1 >= D (the eigen coef is well defined only here)
DEC_FACTOR = 4     # decision = fl(x . coef_k) + intercept_k: the dot product's gamma_D bound, once more for the rounding of the
                   # sum with the intercept (<= u (sum |x w| + |b|) <= gamma_D (...)), and a factor 2 over the two in reserve


@pytest.fixture(scope="module")
def eng():
    from plda_amd import MPlda
    return MPlda(0)


def _check(figures):
    """figures: (name, measured, limit).  Every figure is printed before any is asserted."""
    for name, got, lim in figures:
        print("    %-28s %.3e   (limit %.3e)" % (name, got, lim))
    bad = [(n, g, l) for n, g, l in figures if not g <= l]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ C1: shift invariance
@functools.lru_cache(maxsize=None)
def _case(n, d, k):
    X, y, Xt = M.exact_shift_case(n, d, k, 8192, seed=n + d + k)      # exact at 8192, hence at 256
    for a in (X, Xt):
        assert np.array_equal((a + 256) - 256, a)
    return X, y, Xt


def _priors(k, given):
    return np.random.default_rng(k).random(k) + 0.2 if given else None


@functools.lru_cache(maxsize=None)
def _expected(n, d, k, solver, given, c):
    X, y, Xt = _case(n, d, k)
    pri = _priors(k, given)
    base = lo.fit(X, y, solver, pri)
    return base, M.expected_at_shift(X, y, solver, pri, c)


@pytest.mark.parametrize("given", [False, True], ids=["freq", "priors"])
@pytest.mark.parametrize("c", [0, 256, 8192])
@pytest.mark.parametrize("solver", ["svd", "eigen", "lsqr"])
@pytest.mark.parametrize("n,d,k", SHAPES)
def test_shift_invariance(eng, n, d, k, solver, c, given):
    from plda_amd.lda import LDA
    X, y, Xt = _case(n, d, k)
    base, want = _expected(n, d, k, solver, given, c)
    pri = _priors(k, given)
    lda = LDA(solver, None if pri is None else pri.copy(), engine=eng)
    lda.fit(X + c, y)
    well_defined = solver != "eigen" or k - 1 >= d
    fig = [("means", M.rel(lda._means, want["means"]), 1e-13),
           ("priors", M.rel(lda.priors, want["priors"]), 1e-14)]
    assert np.array_equal(lda._classes, want["classes"])
    if well_defined:
        fig += [("coef", M.rel(lda._coef, want["coef"]), 1e-8),
                ("intercept", M.rel(lda._intercept, want["intercept"]), 1e-8)]
    dec = lda.decision_function(Xt + c)
    if solver == "svd":
        assert lda._scalings.shape == want["scalings"].shape
        # decision values and everything after them do not move with the shift: the expectation is the unshifted model's
        fig += [("xbar", M.rel(lda._xbar, want["xbar"]), 1e-13),
                ("scalings S S^T", M.rel(lda._scalings @ lda._scalings.T, want["scalings"] @ want["scalings"].T), 1e-8),
                ("decision", M.rel(dec, lo.decision_function(base, Xt)), 1e-8),
                ("log_proba", M.rel(lda.predict_log_proba(Xt + c), lo.predict_log_proba(base, Xt)), 1e-9),
                ("proba", M.rel(lda.predict_proba(Xt + c), lo.predict_proba(base, Xt)), 1e-8)]
    if solver == "eigen":
        lead = min(k - 1, d)
        fig += [("evr", M.rel(lda.explained_variance_ratio_, want["explained_variance_ratio"]), 1e-9),
                ("scalings alignment", float(np.abs(M.align_columns(lda._scalings[:, :lead], want["scalings"][:, :lead]) - 1).max()),
                 1e-8)]
    if solver != "svd" and c == 0:
        fig += [("log_proba", M.rel(lda.predict_log_proba(Xt), lo.predict_log_proba(base, Xt)), 1e-9)]
        if well_defined:
            fig += [("proba", M.rel(lda.predict_proba(Xt), lo.predict_proba(base, Xt)), 1e-8)]
    # The decision values of eigen and lsqr on shifted data are differences of terms near c^2, so they are held to the
    # rounding bound of the model's own coef and intercept (DEC_FACTOR above), for svd as well.
    excess = np.abs(dec - M.exact_decision(Xt + c, lda._coef, lda._intercept)) / M.dot_bound(Xt + c, lda._coef, lda._intercept)
    fig += [("decision / dot_bound", float(excess.max()), DEC_FACTOR)]
    _check(fig)


# ------------------------------------------------------------------------------------------------ C2: the row kernel
ROW_K = [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 513, 1025]


def _row_families(K, rng):
    """-> [(name, r[K])], every value a multiple of 1/8 below 2^10 in magnitude."""
    fam = [("ordinary", rng.integers(-80, 81, K) / 8.0)]
    for pos in sorted({0, 255, 256, K - 1}):
        if pos < K:
            r = rng.integers(-6400, 6401, K) / 8.0                       # +-800: exp underflows, the logistic saturates
            r[pos] = 808.0                                               # 1 % clear of the rest after the scaling below
            fam.append(("wide, max at %d" % pos, r))
    if K >= 2:
        r = rng.integers(-80, 81, K) / 8.0
        r[0] = r[K - 1] = 12.0
        if K > 256:
            r[255] = r[256] = 12.0                                       # the tie also across the thread stride
        fam.append(("tied max", r))
    r = -800.0 - rng.integers(0, 81, K) / 8.0                            # every logistic value underflows ...
    r[K // 2] = 1.0                                                      # ... but one of order 1 (a zero row sum is NaN in the reference too)
    fam.append(("all but one underflow", r))
    return fam


def _install(eng, tmp_path, coef, intercept):
    from plda_amd.lda import LDA
    k, d = coef.shape
    path = str(tmp_path / "rows.npz")
    np.savez(path, solver=np.array("lsqr"), classes=np.arange(k), priors=np.full(k, 1.0 / k), means=np.zeros((k, d)),
             coef=coef, intercept=intercept)
    return LDA(engine=eng).load(path)


def _row_errors(name, got, want, K):
    """The worst error in units of its limit: log-softmax |err| / ((K + 8) u (1 + |want|)); logistic and one-vs-rest |err| /
    ((K + 8) u want) where want >= 1e-300 and |err| / 1e-300 below."""
    got = np.asarray(got, np.longdouble)
    unit = (K + 8) * U      # gamma_K of a K-term positive sum in any order + single roundings of exp, log, divide, subtract
    if name == "log_proba":
        return float((np.abs(got - want) / (1 + np.abs(want))).max() / unit)
    big = want >= 1e-300
    rel = float((np.abs(got - want)[big] / want[big]).max() / unit) if big.any() else 0.0
    small = float(np.abs(got - want)[~big].max() / 1e-300) if (~big).any() else 0.0
    return max(rel, small)


@pytest.mark.parametrize("D", [1, 5])
@pytest.mark.parametrize("K", ROW_K)
def test_row_kernel_against_extended_precision(eng, tmp_path, K, D):
    rng = np.random.default_rng(1000 * D + K)
    b = rng.integers(-8, 9, K) / 16.0
    split = np.array([1.0]) if D == 1 else np.array([0.25, 0.25, 0.25, 0.125, 0.125])
    fig = []
    for fname, r in _row_families(K, rng):
        lda = _install(eng, tmp_path, r[:, None] * split[None, :], b)
        for N in (1, 67):
            s = 1.0 - (np.arange(N) % 4) / 8.0                           # row n is s_n r + b, exactly
            X = np.repeat(s[:, None], D, axis=1)
            V = M.exact_decision(X, lda._coef, lda._intercept)
            assert np.array_equal(V, (s[:, None] * r[None, :] + b).astype(np.longdouble))
            dec = lda.decision_function(X)
            if K == 1:
                assert dec.shape == (N,)                                 # the ravel of lda.py:279
                dec = dec[:, None]
            assert np.array_equal(dec, V.astype(np.float64)), "%s: the decision values are exact in fp64" % fname
            lp = lda.predict_log_proba(X)
            pp = lda.predict_proba(X)
            assert lp.shape == (N, K)
            tag = "%s N=%d " % (fname, N)
            fig.append((tag + "log_proba / (K+8)u(1+|v|)", _row_errors("log_proba", lp, M.log_softmax(V), K), 1.0))
            logi = lda._predict(X, 2)
            fig.append((tag + "logistic / (K+8)u", _row_errors("logistic", logi, M.logistic(V), K), 1.0))
            if K == 2:
                assert pp.shape == (N, 4)                                # lda.py:299-300 stacks both halves
                assert np.array_equal(pp[:, 2:], logi) and np.array_equal(pp[:, :2], 1 - logi)
            else:
                assert pp.shape == (N, K)
                fig.append((tag + "one-vs-rest / (K+8)u", _row_errors("ovr", pp, M.one_vs_rest(V), K), 1.0))
            if fname.startswith("wide"):
                assert (lp.argmax(1) == int(fname.split()[-1])).all()
    _check(fig)


# ------------------------------------------------------------------------------------------------ C3: transform values
def _sign_aligned(got, want):
    sign = np.sign((got * want).sum(0))
    return got * sign


@pytest.mark.parametrize("solver,shape", [("svd", SHAPES[0]), ("eigen", SHAPES[1])])
def test_transform_values_for_every_n_components(eng, solver, shape):
    from plda_amd.lda import LDA
    n, d, k = shape
    X, y, Xt = _case(n, d, k)
    base, _ = _expected(n, d, k, solver, False, 0)
    lda = LDA(solver, engine=eng)
    lda.fit(X, y)
    R = lda._scalings.shape[1]
    assert R == (11 if solver == "svd" else d) == base["scalings"].shape[1]
    full = lda.transform(Xt)
    assert full.shape == (M.NT, R)
    off = lda._xbar @ lda._scalings if solver == "svd" else np.zeros(R)
    bound = M.dot_bound(Xt, lda._scalings.T, off)                       # [NT, R]
    fig = []
    for j in (1, 2, R - 1, R, None):
        got = lda.transform(Xt, j)
        want = lo.transform(base, Xt, j)
        cols = R if j is None else j
        assert got.shape == want.shape == (M.NT, cols)
        fig.append(("transform n=%s" % j, M.rel(_sign_aligned(got, want), want), 1e-7))
        # the same columns whatever the leading dimension of the output: 2 * bound, one bound for each of the two results
        fig.append(("prefix n=%s / bound" % j, float((np.abs(got - full[:, :cols]) / bound[:, :cols]).max()), 2.0))
    _check(fig)


# ------------------------------------------------------------------------------------------------ C4: degenerate columns
DEG = (300, 6, 5)


def _degenerate(kind):
    X, y, Xt = M.exact_shift_case(*DEG, 0, seed=7)
    X, y = X.copy(), y.copy()
    dense = np.unique(y, return_inverse=True)[1]
    if kind.startswith("constant "):
        X[:, 2] = float(kind.split()[1])                                # exactly representable: the class means are exact
    elif kind == "class-constant":
        X[:, 2] = (np.arange(DEG[2]) * 0.25 - 0.5)[dense]
    elif kind == "duplicated":
        X[:, 3] = X[:, 1]
        Xt = Xt.copy()
        Xt[:, 3] = Xt[:, 1]
    elif kind == "D=1":
        X, Xt = X[:, :1].copy(), Xt[:, :1].copy()
    elif kind == "singletons":
        y[:3] = [1000, 1001, 1002]
    return X, y, Xt


DEG_CASES = [(kind, s) for kind in ("constant 0", "constant 0.5", "constant 3.0", "class-constant", "duplicated", "D=1")
             for s in ("svd", "eigen", "lsqr")] + [("singletons", "svd")]


@pytest.mark.parametrize("kind,solver", DEG_CASES, ids=["%s-%s" % c for c in DEG_CASES])
def test_degenerate_columns(eng, kind, solver):
    from plda_amd.lda import LDA
    X, y, Xt = _degenerate(kind)
    lda = LDA(solver, engine=eng)
    try:
        want = lo.fit(X, y, solver)
    except np.linalg.LinAlgError:
        # a feature without within-class variance makes Sw singular: scipy's eigh(Sb, Sw) raises in the reference, as the
        # golden files record (eigen_error)
        assert solver == "eigen" and kind != "D=1"
        with pytest.raises(np.linalg.LinAlgError):
            lda.fit(X, y)
        return
    lda.fit(X, y)
    k, d = want["coef"].shape
    fig = [("means", M.rel(lda._means, want["means"]), 1e-13),
           ("log_proba", M.rel(lda.predict_log_proba(Xt), lo.predict_log_proba(want, Xt)), 1e-9)]
    if solver != "eigen" or k - 1 >= d:
        fig += [("coef", M.rel(lda._coef, want["coef"]), 1e-8),
                ("intercept", M.rel(lda._intercept, want["intercept"]), 1e-8)]
    if solver == "svd":
        assert lda._scalings.shape == want["scalings"].shape          # the dropped direction is dropped on the device too
        fig += [("scalings S S^T", M.rel(lda._scalings @ lda._scalings.T, want["scalings"] @ want["scalings"].T), 1e-8)]
    if solver == "eigen":
        fig += [("evr", M.rel(lda.explained_variance_ratio_, want["explained_variance_ratio"]), 1e-9)]
    assert np.array_equal(lda._means, want["means"])                  # sums of grid values are exact; divided once: exact means
    _check(fig)


# ------------------------------------------------------------------------------------------------ C5: handle reuse
def _golden_checks(lda, g, solver):
    """The comparisons of tests/test_gpu_lda.py::test_lda_matches_reference_outputs, on an LDA that is already fitted."""
    k, d = g[solver + "_coef"].shape
    well_defined = solver != "eigen" or k - 1 >= d
    fig = [("priors", M.rel(lda.priors, g[solver + "_priors"]), 1e-14)]
    lp = lda.predict_log_proba(g["Xt"])
    assert lp.shape == g[solver + "_log_proba"].shape
    fig.append(("log_proba", M.rel(lp, g[solver + "_log_proba"]), 1e-9))
    assert lda.predict_proba(g["Xt"]).shape == g[solver + "_proba"].shape
    if well_defined:
        fig += [("coef", M.rel(lda._coef, g[solver + "_coef"]), 1e-8),
                ("intercept", M.rel(lda._intercept, g[solver + "_intercept"]), 1e-8),
                ("decision", M.rel(lda.decision_function(g["Xt"]), g[solver + "_decision"]), 1e-8),
                ("proba", M.rel(lda.predict_proba(g["Xt"]), g[solver + "_proba"]), 1e-8)]
    if solver == "svd":
        assert lda._scalings.shape == g["svd_scalings"].shape
        fig += [("xbar", M.rel(lda._xbar, g["svd_xbar"]), 1e-13),
                ("scalings S S^T", M.rel(lda._scalings @ lda._scalings.T, g["svd_scalings"] @ g["svd_scalings"].T), 1e-8)]
    if solver == "eigen":
        lead = min(k - 1, d)
        fig += [("evr", M.rel(lda.explained_variance_ratio_, g["eigen_evr"]), 1e-9),
                ("scalings alignment", float(np.abs(M.align_columns(lda._scalings[:, :lead], g["eigen_scalings"][:, :lead]) - 1).max()),
                 1e-8)]
        assert lda.transform(g["Xt"], 2).shape == g["eigen_transform2"].shape
        if well_defined:
            fig.append(("transform", M.rel(np.abs(lda.transform(g["Xt"])), np.abs(g["eigen_transform"])), 1e-7))
    return fig


def test_small_fit_after_a_large_one_on_the_same_handle(tmp_path):
    from plda_amd import MPlda
    from plda_amd.lda import LDA
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "lda_small_k5_d6.npz"))
    assert not [s for s in ("svd", "eigen", "lsqr") if s + "_error" in g]
    rng = np.random.default_rng(1730)
    yb = rng.integers(0, 30, 1500)
    Xb = rng.random((1500, 200)) + 0.5 * rng.standard_normal((30, 200))[yb]
    used, fresh = MPlda(0), MPlda(0)
    fig = []
    for solver in ("svd", "eigen", "lsqr"):
        LDA(solver, engine=used).fit(Xb, yb)                            # leaves the larger problem in every scratch buffer
        a, b = LDA(solver, engine=used), LDA(solver, engine=fresh)
        assert a.fit(g["X"], g["y"]) is None and b.fit(g["X"], g["y"]) is None
        fig += [(solver + " " + n, v, l) for n, v, l in _golden_checks(a, g, solver)]
        names = ["_means", "_coef", "_intercept"] + {"svd": ["_xbar", "_scalings"], "eigen": ["_scalings", "explained_variance_ratio_"],
                                                      "lsqr": []}[solver]
        for name in names:
            fig.append(("%s %s used vs fresh" % (solver, name), M.rel(getattr(a, name), getattr(b, name)), 1e-13))
        fig.append((solver + " log_proba used vs fresh", M.rel(a.predict_log_proba(g["Xt"]), b.predict_log_proba(g["Xt"])), 1e-13))
        if solver != "lsqr":
            fig.append((solver + " transform used vs fresh", M.rel(a.transform(g["Xt"]), b.transform(g["Xt"])), 1e-13))
    # then a loaded K = 3, D = 2 model on the used handle: every product below is exact in fp64
    coef = np.array([[1.0, -0.5], [0.25, 2.0], [-1.5, 0.75]])
    icpt = np.array([0.5, -0.25, 1.0])
    xbar = np.array([0.5, -1.0])
    scal = np.array([[2.0, 0.5], [-0.25, 1.0]])
    path = str(tmp_path / "k3d2.npz")
    np.savez(path, solver=np.array("svd"), classes=np.array([3, 5, 9]), priors=np.full(3, 1.0 / 3), means=np.zeros((3, 2)), coef=coef,
             intercept=icpt, xbar=xbar, scalings=scal)
    lda = LDA(engine=used).load(path)
    X = rng.integers(-16, 17, (67, 2)) / 4.0
    V = X @ coef.T + icpt
    assert np.array_equal(lda.decision_function(X), V)
    T = (X - xbar) @ scal
    assert np.array_equal(lda.transform(X), T) and np.array_equal(lda.transform(X, 1), T[:, :1])
    fig += [("loaded log_proba / (K+8)u(1+|v|)", _row_errors("log_proba", lda.predict_log_proba(X), M.log_softmax(V), 3), 1.0),
            ("loaded one-vs-rest / (K+8)u", _row_errors("ovr", lda.predict_proba(X), M.one_vs_rest(V), 3), 1.0)]
    _check(fig)
