"""Host model (NumPy fp64) of PLDA domain adaptation (include/plda_hip.h, "PLDA domain adaptation"): the statistics record
about a pilot, Kaldi's PldaUnsupervisedAdaptor::UpdatePlda in Kaldi's own order of operations (restated from the published
algorithm, parity unpinned), the short form the engine computes as a second, independent function, and the interpolation
of two models.  Shared by tests/test_adapt_model.py (CPU) and tests/test_gpu_adapt.py."""
import numpy as np


def synthetic_model(d, seed):
    """A well-conditioned model: an orthogonal matrix times row scales in [0.5, 1.5], psi descending in [0.05, 3.05] (the
    recipe of tests/test_gpu_scratch_poison.py:_model).  Returns (mean, transform, psi)."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    return rng.random(d), q * (0.5 + rng.random(d))[:, None], np.sort(rng.random(d) * 3.0 + 0.05)[::-1].copy()


def covariances(transform, psi):
    """(W, B): within-class (T^T T)^-1 and between-class T^-1 diag(psi) T^-T."""
    tinv = np.linalg.inv(transform)
    return tinv @ tinv.T, (tinv * psi[None, :]) @ tinv.T


def sample(mean, transform, psi, n, seed, scale=1.0, offset=None):
    """n rows with covariance scale^2 (W + B) of the model, around mean (+ offset)."""
    rng = np.random.default_rng(seed)
    W, B = covariances(transform, psi)
    L = np.linalg.cholesky(W + B)
    x = mean[None, :] + scale * rng.standard_normal((n, mean.shape[0])) @ L.T
    return x if offset is None else x + offset[None, :]


# ------------------------------------------------------------------------------------------------------------ record
def record(x, pilot, weights=None, dtype=np.float64):
    """dict(tot_weight, rows, pilot, s1, s2): the sums about the pilot.  dtype=np.longdouble: the (nearly) exact variant."""
    x = np.asarray(x, dtype)
    w = np.ones(x.shape[0], dtype) if weights is None else np.asarray(weights, dtype)
    c = x - np.asarray(pilot, dtype)[None, :]
    return dict(tot_weight=w.sum(), rows=x.shape[0], pilot=np.asarray(pilot, np.float64).copy(), s1=(c * w[:, None]).sum(0),
                s2=(c * w[:, None]).T @ c)


def record_bound(x, pilot, weights=None):
    """sum_i w_i |x_i - p|_a |x_i - p|_b, the elementwise scale of the record's rounding error, [D + 1, D + 1] in the
    augmented layout [S2 | S1; S1 | tw]."""
    c = np.abs(np.asarray(x, np.float64) - pilot[None, :])
    c = np.concatenate([c, np.ones((c.shape[0], 1))], axis=1)
    w = np.ones(c.shape[0]) if weights is None else np.asarray(weights, np.float64)
    return (c * w[:, None]).T @ c


def augmented(rec):
    d = rec["s1"].shape[0]
    a = np.zeros((d + 1, d + 1), rec["s2"].dtype)
    a[:d, :d] = rec["s2"]
    a[:d, d] = a[d, :d] = rec["s1"]
    a[d, d] = rec["tot_weight"]
    return a


def merge(a, b):
    assert np.array_equal(a["pilot"], b["pilot"])
    return dict(tot_weight=a["tot_weight"] + b["tot_weight"], rows=a["rows"] + b["rows"], pilot=a["pilot"], s1=a["s1"] + b["s1"],
                s2=a["s2"] + b["s2"])


def centred_variance(rec):
    """S2 / tw - delta delta^T: the variance about the data's own mean, from the pilot form."""
    d = rec["s1"] / rec["tot_weight"]
    return rec["s2"] / rec["tot_weight"] - np.outer(d, d)


def naive_variance(x, weights=None, dtype=np.float64):
    """Kaldi's form: sum w x x^T / tw - mean mean^T, the sums taken about 0."""
    x = np.asarray(x, dtype)
    w = np.ones(x.shape[0], dtype) if weights is None else np.asarray(weights, dtype)
    tw = w.sum()
    m = (x * w[:, None]).sum(0) / tw
    return (x * w[:, None]).T @ x / tw - np.outer(m, m)


# --------------------------------------------------------------------------------------- simultaneous diagonalisation
def simdiag(W, B):
    """(transform, psi) with T W T^T = I, T B T^T = diag(psi), psi descending and floored at 0: PldaEstimator::GetOutput's
    recipe (Cholesky whitening of W, eigenvectors of the whitened B, stable descending sort)."""
    cinv = np.linalg.inv(np.linalg.cholesky(0.5 * (W + W.T)))
    g = cinv @ B @ cinv.T
    lam, q = np.linalg.eigh(0.5 * (g + g.T))
    order = np.argsort(-lam, kind="stable")
    return q[:, order].T @ cinv, np.maximum(lam[order], 0.0)


def _eig_desc(a):
    lam, q = np.linalg.eigh(0.5 * (a + a.T))
    order = np.argsort(-lam, kind="stable")
    return lam[order], q[:, order]


# ------------------------------------------------------------------------------------------------------------ update
def update_kaldi(mean, transform, psi, rec, within_scale=0.3, between_scale=0.7, mean_diff_scale=1.0):
    """PldaUnsupervisedAdaptor::UpdatePlda as Kaldi orders it: the centred variance plus mean_diff_scale times the outer
    product of the mean difference; projection with the rows of the transform scaled by 1 / sqrt(1 + psi); eigenvalues
    descending; ws e and bs e added to the DIAGONALS of the model's within / between covariances in the P basis; back with
    the general inverse of P^T Tm; Cholesky, eigh, stable descending sort.  `mean` must be the record's pilot."""
    assert np.array_equal(mean, rec["pilot"])
    tw = rec["tot_weight"]
    delta = rec["s1"] / tw
    new_mean = rec["pilot"] + delta
    variance = centred_variance(rec) + mean_diff_scale * np.outer(delta, delta)
    tm = transform / np.sqrt(1.0 + psi)[:, None]
    s, p = _eig_desc(tm @ variance @ tm.T)
    pt = p.T
    wproj = pt @ np.diag(1.0 / (1.0 + psi)) @ pt.T
    bproj = pt @ np.diag(psi / (1.0 + psi)) @ pt.T
    excess = np.where(s > 1.0, s - 1.0, 0.0)
    wproj[np.diag_indices_from(wproj)] += within_scale * excess
    bproj[np.diag_indices_from(bproj)] += between_scale * excess
    back = np.linalg.inv(pt @ tm)
    W = back @ wproj @ back.T
    B = back @ bproj @ back.T
    t_new, psi_new = simdiag(W, B)
    return dict(mean=new_mean, transform=t_new, psi=psi_new, s=s, W=W, B=B)


def update_short(mean, transform, psi, rec, within_scale=0.3, between_scale=0.7, mean_diff_scale=1.0):
    """The form of the header: V = S2 / tw - (1 - mds) delta delta^T, E = Tm^-1 P diag(max(s - 1, 0)) P^T Tm^-T with
    Tm^-1 = W T^T diag(sqrt(1 + psi)), W' = W + ws E, B' = B + bs E.  No general inverse: W = (T^T T)^-1."""
    assert np.array_equal(mean, rec["pilot"])
    tw = rec["tot_weight"]
    delta = rec["s1"] / tw
    V = rec["s2"] / tw - (1.0 - mean_diff_scale) * np.outer(delta, delta)
    a = transform.T @ transform
    W = np.linalg.inv(0.5 * (a + a.T))
    W = 0.5 * (W + W.T)
    tinv = W @ transform.T
    B = (tinv * psi[None, :]) @ tinv.T
    tm = transform / np.sqrt(1.0 + psi)[:, None]
    s, p = _eig_desc(tm @ V @ tm.T)
    f = (tinv * np.sqrt(1.0 + psi)[None, :]) @ p
    E = (f * np.maximum(s - 1.0, 0.0)[None, :]) @ f.T
    Wn, Bn = W + within_scale * E, B + between_scale * E
    t_new, psi_new = simdiag(Wn, Bn)
    return dict(mean=rec["pilot"] + delta, transform=t_new, psi=psi_new, s=s, W=Wn, B=Bn)


# ------------------------------------------------------------------------------------------------------------- blend
def blend(model, other, alpha, alpha_mean=None):
    """(mean, transform, psi) triples in, dict out: covariances and means interpolated, then diagonalised."""
    am = alpha if alpha_mean is None else alpha_mean
    W1, B1 = covariances(model[1], model[2])
    W2, B2 = covariances(other[1], other[2])
    W, B = (1.0 - alpha) * W1 + alpha * W2, (1.0 - alpha) * B1 + alpha * B2
    t_new, psi_new = simdiag(W, B)
    return dict(mean=(1.0 - am) * model[0] + am * other[0], transform=t_new, psi=psi_new, W=W, B=B)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


# ------------------------------------------------------------------------------------------ the comparison rule
def gram(T, psi):
    return T.T @ T, T.T @ (T * psi[:, None])


def assert_model(got, ref, band=1e-8):
    """mean' at 1e-12 relative; T^T T, T^T diag(psi) T and psi at `band` of the reference's largest element (transforms are
    compared through T^T T: the rows' signs are free)."""
    assert np.abs(got["mean"] - ref["mean"]).max() <= 1e-12 * np.abs(ref["mean"]).max()
    g1, g2 = gram(got["transform"], got["psi"])
    r1, r2 = gram(ref["transform"], ref["psi"])
    assert np.abs(g1 - r1).max() <= band * np.abs(r1).max()
    assert np.abs(g2 - r2).max() <= band * np.abs(r2).max()
    assert np.abs(got["psi"] - ref["psi"]).max() <= band * np.abs(ref["psi"]).max()
