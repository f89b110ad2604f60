"""tests/fit_model.py -- what PLDA.fit (csrc/fit.hip) and transform must compute on data with a common offset, stated on the CPU
so that the statement does not share a weak step with the code under test.

    grid_data(seed, n, d, k, between, singles, const_cols)
                                  conftest.make_data's distribution (uniform [0, 1) rows + between * N(0, 1) class centres) on the
                                  grid 2^-20, with skewed class sizes: x + c is exact in fp64 for every power of two c <= 2^17, so
                                  the fit of the shifted rows is known from the fit of the unshifted rows by identities, not by a fit
    expected_stats / expected_fit(oracle, x, y, c[, iters])
                                  oracle.stats / oracle.fit on the UNSHIFTED rows (where the oracle is accurate to 1e-14), carried
                                  across x -> x + c:
                                    counts, scatter, W, B, psi, T^T T, T^T Psi T     unchanged
                                    class means, the model mean                      + c
                                    sum                                              + c * class_weight
                                    offset + T mean                                  = 0
    scatter_longdouble(x, y)      class-centred rows and their weighted product in np.longdouble: the yardstick of the statistics
    means_longdouble(x, y)        class means in np.longdouble
    mean_bound / model_mean_bound the a-priori rounding bounds of a class mean and of the model mean (derived at the functions)
    stats_uncentred / fit_uncentred
                                  the formula the library and both oracles used before they centred their rows, Kaldi's AddSamples
                                  order  X^T diag(1 / n) X - M^T M,  in NumPy: tests/test_fit_model.py records what it loses
    transform_longdouble, transform_bound
                                  Plda::TransformIvector (T x + offset, length-normalised) in np.longdouble and its a-priori bound
"""
import numpy as np

from oracle import plda_oracle_np as onp

U = 2.0 ** -53
GRID = 2.0 ** -20
SHIFTS = (0.0, 1024.0, 8192.0, 131072.0)

# (N, D, K, between) of the whole-fit cases; (D, N, K) of the statistics pass's dispatch classes (csrc/linalg.hip:
# syrk_pair_f64 -- the triangle kernel to D = 208, the block kernel for EVEN D in 210 .. 512, two GEMMs otherwise)
FIT_SHAPES = [(60, 6, 5), (1200, 33, 40), (3000, 64, 100)]
STAT_SHAPES = [(6, 60, 5), (33, 1200, 40), (208, 700, 9), (209, 700, 9), (210, 700, 9), (300, 900, 12), (513, 800, 7)]
BETWEEN = 0.5


def _quantise(a):
    return np.round(a / GRID) * GRID


def grid_data(seed, n, d, k, between=BETWEEN, singles=0, const_cols=()):
    """-> (x [n, d] float64 on the grid 2^-20, y [n] uint64 dense 0..k-1).  The first `singles` classes have one row; every other
    class has at least two, the rest dealt with probability ~ 1 / (1 + rank): many distinct n_k, one class much larger than the
    others.  Columns in const_cols hold ONE value per class.  Rows are shuffled."""
    assert 0 <= singles <= k and n >= singles + 2 * (k - singles)
    rng = np.random.default_rng(seed)
    many = np.arange(singles, k)
    dense = np.concatenate([np.arange(singles), many, many])
    free = n - len(dense)
    if len(many):
        p = 1.0 / (1.0 + np.arange(len(many)))
        dense = np.concatenate([dense, rng.choice(many, free, p=p / p.sum())])
    else:
        assert free == 0
    rng.shuffle(dense)
    centres = between * rng.standard_normal((k, d))
    x = rng.random((n, d)) + centres[dense]
    for j in const_cols:
        x[:, j] = 0.5 + centres[dense, j]
    return _quantise(x), dense.astype(np.uint64)


def assert_exact_shift(x, c):
    assert c == 0 or (c > 0 and 2.0 ** int(np.log2(c)) == c and c <= 2.0 ** 17)
    assert np.array_equal((x + c) - c, x)


def total_scale(x):
    """The largest diagonal entry of the rows' total covariance."""
    return float(np.asarray(x, np.longdouble).var(axis=0).max())


# ---------------------------------------------------------------------------------------------------------- the shift identities
def expected_stats(oracle, x, y, c):
    st = dict(oracle.stats(x, y))
    st["means"] = st["means"] + c
    st["sum"] = st["sum"] + c * st["class_weight"]
    return st


def expected_fit(oracle, x, y, c, iters):
    """The model of (x + c, y) from the oracle's fit of x: W, B, psi and transform are the unshifted fit's (the transform up to
    the signs of its rows: compare T^T T and T^T Psi T)."""
    m = dict(oracle.fit(x, y, iters))
    m["mean"] = m["mean"] + c
    del m["offset"]               # (moves with the transform's arbitrary row signs: offset + T mean = 0 is what holds)
    return m


# ------------------------------------------------------------------------------------------------------ extended-precision yardsticks
def means_longdouble(x, y):
    xl = np.asarray(x, np.float64).astype(np.longdouble)
    y = np.asarray(y).astype(np.int64)
    k = int(y.max()) + 1
    return np.stack([xl[y == c].sum(0) / np.longdouble(int((y == c).sum())) for c in range(k)])


def scatter_longdouble(x, y):
    """sum_i (1 / n_label(i)) (x_i - m_label(i)) (x_i - m_label(i))^T with means, centring and product in np.longdouble (64-bit
    significand), like oracle/plda_oracle_np.py:fit_wb_longdouble.  On grid data the rows x + c are exact, so the scatter of the
    shifted rows IS the scatter of the unshifted ones: call it on the unshifted rows, where even the means are exact."""
    xl = np.asarray(x, np.float64).astype(np.longdouble)
    y = np.asarray(y).astype(np.int64)
    m = means_longdouble(x, y)
    s = np.zeros((xl.shape[1], xl.shape[1]), np.longdouble)
    for c in range(m.shape[0]):
        xc = xl[y == c] - m[c]
        s += (xc.T @ xc) / np.longdouble(xc.shape[0])
    return s


def mean_bound(counts, xmax):
    """|fl(m_k) - m_k| <= n_k u max|x| for the class mean the statistics pass forms: a sum of the class's n_k rows in row order,
    times fl(1 / n_k).

    The sum: n_k - 1 additions, each rounding a partial sum of magnitude at most n_k max|x|, so |fl(s) - s| <= (n_k - 1) u n_k max|x|
    to first order (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4 with sum |x_i| <= n_k max|x|) -- (n_k - 1) u max|x|
    after the division by n_k.  The scaling by fl(1 / n_k) adds two roundings of the mean, 2 u max|x|: (n_k + 1) u max|x| in
    general.  On grid_data's rows every partial sum is a multiple of 2^-20 below 2^53 * 2^-20, i.e. EXACT, and what is left is the
    scaling: nothing for n_k = 1 and n_k = 2 (1 / n_k exact), at most 2 u max|x| <= n_k u max|x| from n_k = 3 on.  So n_k u max|x|
    bounds the kernel on these rows whatever order it sums in, and a kernel that loses a row, a bit of the offset or a
    correctly-rounded sum's worth of precision exceeds it.  (A relative 1e-13 allows 1.3e-8 at |x| ~ 131072: 1000 u max|x|.)"""
    return np.asarray(counts, np.float64)[:, None] * U * float(xmax)


def model_mean_bound(counts, xmax):
    """The model mean is sum_k w_k m_k / sum_k w_k, w_k = 1 / n_k: a convex combination of the class means, so it inherits their
    worst error max_k n_k u max|x| (mean_bound), plus the rounding of the K products w_k m_k, of their sum and of sum w_k in any
    order -- gamma_{K+1} of sum_k w_k |m_k| / sum_k w_k <= max|x| each for numerator and denominator, and the division: at most
    (max_k n_k + 2 K + 4) u max|x| to first order."""
    counts = np.asarray(counts)
    return (float(counts.max()) + 2.0 * len(counts) + 4.0) * U * float(xmax)


# ------------------------------------------------------------------------------- the formula before the rows were centred (Kaldi's order)
def stats_uncentred(x, y):
    """oracle/plda_oracle_np.py:stats with the offset scatter as PldaStats::AddSamples accumulates it,
    X^T diag(1 / n_label) X - sum_k m_k m_k^T: a difference of uncentred sums."""
    x = np.asarray(x, np.float64)
    st = dict(onp.stats(x, y))
    lab = np.asarray(y).astype(np.int64)
    w = 1.0 / st["counts"]
    s = (x * w[lab][:, None]).T @ x - st["means"].T @ st["means"]
    st["scatter"] = 0.5 * (s + s.T)
    return st


def fit_uncentred(x, y, iters):
    st = stats_uncentred(x, y)
    d = st["scatter"].shape[0]
    w, b = np.eye(d), np.eye(d)
    for _ in range(iters):
        w, b = onp.em_iter(st, w, b)
    m = onp.get_output(st, w, b)
    m["W"], m["B"] = w, b
    return m


def rel(a, b):
    """max |a - b| / max |b|, the measure of tests/test_gpu_fit.py."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# -------------------------------------------------------------------------------------------------------------- transform on offset rows
def gamma(n):
    return n * U / (1.0 - n * U)


def transform_model(seed, d, c):
    """-> (mean + c, T, psi): an explicit model whose mean carries the rows' offset; T is a scaled orthogonal matrix."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    t = q * (0.5 + rng.random(d))[:, None]
    psi = np.sort(rng.random(d) * 3.0 + 0.05)[::-1].copy()
    return rng.random(d) + c, t, psi


def transform_rows(seed, r, d):
    """-> (rows on the grid 2^-20 [r, d], ragged utterance counts [r] with 1 and a large one present)."""
    rng = np.random.default_rng(seed)
    x = _quantise(rng.random((r, d)) + 0.5 * rng.standard_normal((r, d)))
    n = rng.choice([1, 2, 3, 7, 40], r).astype(np.int32)
    n[:5] = [1, 2, 3, 7, 40]
    return x, n


def transform_longdouble(t, offset, psi, x, n):
    """oracle/plda_oracle_np.py:transform_ivector (Plda::TransformIvector, normalize_length, not simple_length_norm) in
    np.longdouble on the model's arrays AS LOADED (the offset the library holds, not a recomputed one).
    -> (v [R, D], y = T x + offset [R, D], the normalisation factor f [R])."""
    ld = np.longdouble
    t, offset, psi, x = (np.asarray(a, np.float64).astype(ld) for a in (t, offset, psi, x))
    n = np.asarray(n).astype(ld)
    y = x @ t.T + offset
    d = ld(y.shape[1])
    q = (y * y / (psi[None, :] + 1 / n[:, None])).sum(1)
    f = np.sqrt(d / q)
    return y * f[:, None], y, f


def transform_bound(t, offset, psi, x, n):
    """The a-priori bound of v = f y,  y = T x + offset,  f = sqrt(D / q),  q = sum_d y_d^2 / (psi_d + 1 / n), evaluated in fp64
    in ANY summation order, with or without fused multiply-adds.

    y: a dot product of length D plus one more term, |fl(y_j) - y_j| <= e_j = gamma_{D+1} (sum_d |T_jd x_d| + |offset_j|)
    (Higham, section 3.1).  With a common offset c in x and -T c in the offset the terms are of size c while y stays of size 1:
    this is Kaldi's formula, kept by the kernel, and e_j is what it costs.
    q: its terms are positive.  The error of y moves q by at most dq = sum_d (2 |y_d| e_d + e_d^2) / (psi_d + 1 / n); evaluating
    it rounds psi + 1 / n (2 u with the reciprocal of n), the square, the quotient and a sum of D terms: gamma_{D+4} q.
    f = sqrt(D / q): a relative change of q moves f by half of it; the division and the square root add 2 u:
    df / f <= 0.5 (dq / q + gamma_{D+4}) + 2 u.
    v_j = f y_j, one more rounding:  |fl(v_j) - v_j| <= f e_j + |v_j| (df / f + u), to first order.
    Everything is evaluated in np.longdouble, and the bound is doubled for the second-order terms dropped above."""
    ld = np.longdouble
    tl, ol, xl = (np.abs(np.asarray(a, np.float64).astype(ld)) for a in (t, offset, x))
    v, y, f = transform_longdouble(t, offset, psi, x, n)
    dd = y.shape[1]
    e = gamma(dd + 1) * (xl @ tl.T + ol)
    den = np.asarray(psi, np.float64).astype(ld)[None, :] + 1 / np.asarray(n).astype(ld)[:, None]
    q = (y * y / den).sum(1)
    dq = ((2 * np.abs(y) * e + e * e) / den).sum(1)
    dff = 0.5 * (dq / q + gamma(dd + 4)) + 2 * U
    return 2 * (f[:, None] * e + np.abs(v) * (dff[:, None] + U))
