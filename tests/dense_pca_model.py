"""tests/dense_pca_model.py -- NumPy model of recording-dependent PCA before dense PLDA scoring (K19; include/plda_hip.h,
"dense scoring in a recording's PCA subspace"; Kaldi: ivector-plda-scoring-dense --target-energy, Plda::ApplyTransform,
restated, parity unpinned).  Written from the definition with np.linalg.eigh and np.linalg.cholesky; a second route takes the
PCA from np.linalg.svd of the centred rows.  Everything is fp64; the block is returned in fp64 (the device rounds it once).
"""
import numpy as np

LOG_2PI = float(np.log(2.0 * np.pi))
RANK_TOL = 2.0 ** -40


def model_covariances(model):
    """(W, B) of an untruncated model: W = T^-1 T^-T, B = T^-1 diag(psi) T^-T."""
    T = np.asarray(model["transform"], np.float64)
    if T.shape[0] != T.shape[1]:
        raise ValueError("the model is truncated")
    Ti = np.linalg.inv(T)
    return Ti @ Ti.T, (Ti * np.asarray(model["psi"], np.float64)[None, :]) @ Ti.T


def pca(x, route="eigh"):
    """Step 1, 2 and 4 for every direction: (lam [m] descending, floored at 0; vecs [m, D], eigenvectors of C as rows --
    rows of zero variance may be anything)."""
    x = np.asarray(x, np.float64)
    n, dd = x.shape
    xc = x - (x[0] + (x - x[0]).mean(0))       # the mean about the first row: equal rows centre to exact zeros
    m = min(n, dd)
    if route == "svd":
        _, s, vt = np.linalg.svd(xc, full_matrices=False)
        return np.maximum(s * s / n, 0.0)[:m], vt[:m]
    if route != "eigh":
        raise ValueError(route)
    if n <= dd:
        w, u = np.linalg.eigh(xc @ xc.T / n)
        w, u = w[::-1], u[:, ::-1]
        lam = np.maximum(w, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            vecs = (xc.T @ u / np.sqrt(n * lam)[None, :]).T
        return lam, vecs
    w, v = np.linalg.eigh(xc.T @ xc / n)
    return np.maximum(w[::-1], 0.0), v[:, ::-1].T


def rank_of(lam):
    return int((lam > RANK_TOL * lam[0]).sum()) if len(lam) and lam[0] > 0 else 0


def energy_dim(lam, target):
    """Kaldi's rule to the letter (lam descending): dim = 1, energy = 0; while energy / E <= target: energy += lam[dim - 1],
    dim++.  (The loop also ends when the eigenvalues run out, which only rounding in E can cause.)"""
    lam = np.asarray(lam, np.float64)
    e = 0.0
    for v in lam:           # fixed ascending-index order, as the device sums
        e += v
    if not e > 0.0:
        return 0
    dim, energy = 1, 0.0
    while energy / e <= target and dim - 1 < len(lam):
        energy += lam[dim - 1]
        dim += 1
    return dim


def retained(lam, target):
    """d = min(dim, rank); 0 when E = 0."""
    return min(energy_dim(lam, target), rank_of(lam))


def subspace_model(W, B, P):
    """Step 5: (M [d, D], psi' [d] descending) with M W M^T = I, M B M^T = diag(psi')."""
    Wp, Bp = P @ W @ P.T, P @ B @ P.T
    Wp, Bp = (Wp + Wp.T) / 2, (Bp + Bp.T) / 2
    L = np.linalg.cholesky(Wp)
    Li = np.linalg.inv(L)
    Z = Li @ Bp @ Li.T
    psi, U = np.linalg.eigh((Z + Z.T) / 2)
    psi, U = psi[::-1], U[:, ::-1]
    return U.T @ Li @ P, psi


def llr_block(psi, y):
    """Step 7: S[i, j] = LogLikelihoodRatio(enrol y_i with n = 1, test y_j), per-pair form summed over the dimensions."""
    c = psi / (psi + 1.0)
    var = 1.0 + c
    var0 = 1.0 + psi
    diff = y[None, :, :] - (c * y)[:, None, :]
    given = -0.5 * (np.log(var).sum() + LOG_2PI * len(psi) + (diff * diff / var).sum(2))
    without = -0.5 * (np.log(var0).sum() + LOG_2PI * len(psi) + (y * y / var0).sum(1))
    return given - without[None, :]


def score_block(model, x, target, route="eigh", rot=None, wb=None):
    """Steps 1 to 7 of one recording: (S float64 [N, N], d, lam [m]).  rot: an orthogonal [d, d] matrix applied to the basis
    (the scores must not depend on it)."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    lam, vecs = pca(x, route)
    d = retained(lam, target)
    if d == 0:
        return np.zeros((n, n)), 0, lam
    P = vecs[:d]
    if rot is not None:
        P = rot @ P
    W, B = wb if wb is not None else model_covariances(model)
    M, psi = subspace_model(W, B, P)
    y = (x - np.asarray(model["mean"], np.float64)) @ M.T
    y = y * np.sqrt(d / (y * y / (psi + 1.0)).sum(1))[:, None]
    return llr_block(psi, y), d, lam


def score_blocks(model, x, offsets, target, route="eigh"):
    """Every recording of a call: ([S_r], dims int32 [R], eig float64 [T] in the layout of the C ABI)."""
    wb = model_covariances(model)
    blocks, dims, eig = [], [], np.zeros(int(offsets[-1]))
    for r in range(len(offsets) - 1):
        a, b = int(offsets[r]), int(offsets[r + 1])
        s, d, lam = score_block(model, x[a:b], target, route, wb=wb)
        blocks.append(s)
        dims.append(d)
        eig[a:a + len(lam)] = lam
    return blocks, np.asarray(dims, np.int32), eig


def full_model_llr(model, x):
    """The full model's scores of the rows of one recording (num_examples = 1): TransformIvector, then the LLR."""
    T, psi = np.asarray(model["transform"], np.float64), np.asarray(model["psi"], np.float64)
    y = (np.asarray(x, np.float64) - model["mean"]) @ T.T
    y = y * np.sqrt(T.shape[0] / (y * y / (psi + 1.0)).sum(1))[:, None]
    return llr_block(psi, y)


# ------------------------------------------------------------------------------------------- inputs of the tests
def random_model(rng, d):
    """An untruncated model with a well-conditioned transform and a decaying psi."""
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    t = (q * np.exp(rng.uniform(-0.5, 0.5, d))[None, :]) @ np.linalg.qr(rng.standard_normal((d, d)))[0]
    psi = np.sort(np.exp(rng.uniform(-2.0, 2.0, d)))[::-1].copy()
    return {"mean": rng.standard_normal(d) * 0.3, "transform": t, "psi": psi}


def planted_rows(rng, n, d, ratio=0.7, offset=1.0, scales=None):
    """Gaussian rows times a geometric scale (ratio per direction), times a random orthogonal matrix, plus an offset."""
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    sc = ratio ** np.arange(d) if scales is None else np.asarray(scales, np.float64)
    return (rng.standard_normal((n, d)) * sc[None, :]) @ q + offset * rng.standard_normal(d)


def margins(lam, target):
    """(the smallest |cumulative energy share - target| over k, (lam[d-1] - lam[d]) / lam[0] or inf without a cut)."""
    lam = np.asarray(lam, np.float64)
    e = lam.sum()
    if not e > 0:
        return np.inf, np.inf
    share = np.abs(np.concatenate([[0.0], np.cumsum(lam)]) / e - target).min()
    d = retained(lam, target)
    gap = (lam[d - 1] - lam[d]) / lam[0] if d < len(lam) else np.inf
    return float(share), float(gap)


def case(seed, sizes, d, target, ratio=0.7, check=True):
    """(model, x [T, d], offsets) of one call: planted rows per recording.  The seed is stepped by 1000 until the MODEL's own
    numbers keep every cumulative energy share 1e-6 away from the target and the cut 1e-3 lam_1 wide (so that rounding cannot
    move the retained dimension); the tests assert both again."""
    from_seed = seed
    while True:
        rng = np.random.default_rng(seed)
        model = random_model(rng, d)
        x = np.concatenate([planted_rows(rng, n, d, ratio) for n in sizes])
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        if not check:
            return model, x, offsets
        ok = True
        for r in range(len(sizes)):
            share, gap = margins(pca(x[offsets[r]:offsets[r + 1]])[0], target)
            ok = ok and share >= 2e-6 and gap >= 2e-3
        if ok:
            return model, x, offsets
        seed += 1000
        if seed > from_seed + 50000:
            raise RuntimeError("no seed meets the margins")


def ill_conditioned_case(seed=70, n=40, d=8, span=1e-6):
    """(model, x, offsets, target) of the ill-conditioned test: a planted spectrum of variances spanning `span`, target
    0.99999, so that directions near span * lam_1 are retained."""
    rng = np.random.default_rng(seed)
    model = random_model(rng, d)
    x = planted_rows(rng, n, d, scales=np.sqrt(span) ** (np.arange(d) / (d - 1.0)))
    return model, x, np.asarray([0, n], np.int64), 0.99999
