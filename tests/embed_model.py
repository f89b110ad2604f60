"""tests/embed_model.py -- NumPy model of the embedding chain (K18; include/plda_hip.h, "embedding chain"): the five steps
literally, the fit of the three kinds, and the a-priori elementwise error bound of a device result."""
import numpy as np

U = 2.0 ** -53


class Chain(object):
    """The plain tuple of the definition; any of m_in, A, m_out may be None."""
    def __init__(self, m_in=None, len_in=0.0, A=None, m_out=None, len_out=0.0):
        self.m_in, self.len_in, self.A, self.m_out, self.len_out = m_in, float(len_in), A, m_out, float(len_out)


def _steps(chain, x, dtype):
    """-> (v after step 2, u after step 4, out) in `dtype`."""
    x = np.asarray(x).astype(dtype)                      # fp32 widens exactly
    v = x - (np.asarray(chain.m_in, dtype) if chain.m_in is not None else dtype(0))
    if chain.len_in > 0:
        nv = np.sqrt(np.sum(v * v, axis=1, keepdims=True))
        with np.errstate(invalid="ignore", divide="ignore"):
            v = np.where(nv == 0, dtype(0), v * (dtype(chain.len_in) / nv))
    u = v @ np.asarray(chain.A, dtype).T if chain.A is not None else v.copy()
    if chain.m_out is not None:
        u = u - np.asarray(chain.m_out, dtype)
    out = u
    if chain.len_out > 0:
        nu = np.sqrt(np.sum(u * u, axis=1, keepdims=True))
        with np.errstate(invalid="ignore", divide="ignore"):
            out = np.where(nu == 0, dtype(0), u * (dtype(chain.len_out) / nu))
    return v, u, out


def apply(chain, x, dtype=np.float64):
    """The five steps, literally, in `dtype` (np.float64 or np.longdouble)."""
    return _steps(chain, x, dtype)[2]


def error_bound(chain, x):
    """Elementwise bound [R, Dout] on |device - longdouble model|, everything from the longdouble model:
        e_d = (Din + 8) 2^-53 (sum_k |A_dk| |v_k| + |m_out,d|)                                  (v after step 2)
        len_out > 0:  4 [ s2 e_d + |out_d| (|e|_2 / |u|_2 + (Dout + 8) 2^-53) ]                 (s2 = len_out / |u|)
        otherwise:    4 [ e_d + |out_d| 2^-53 ]
    Derived, not measured: centring is one rounding per element, the k-sum's error constant is Din 2^-53 in any order, the
    first norm's relative error (Din + 2) 2^-53 / 2 and its scaling two roundings are inside the (Din + 8); the second norm
    moves with the error of u and its own (Dout + 8) 2^-53; a factor 4 on top."""
    ld = np.longdouble
    v, u, out = _steps(chain, x, ld)
    din = v.shape[1]
    absA = np.abs(np.asarray(chain.A, ld)) if chain.A is not None else None
    s = np.abs(v) @ absA.T if absA is not None else np.abs(v)
    dout = s.shape[1]
    mo = np.abs(np.asarray(chain.m_out, ld)) if chain.m_out is not None else ld(0)
    e = (din + 8) * ld(U) * (s + mo)
    if chain.len_out > 0:
        nu = np.sqrt(np.sum(u * u, axis=1, keepdims=True))
        ne = np.sqrt(np.sum(e * e, axis=1, keepdims=True))
        with np.errstate(invalid="ignore", divide="ignore"):
            s2 = np.where(nu == 0, ld(0), ld(chain.len_out) / nu)
            rel = np.where(nu == 0, ld(0), ne / nu)
        b = 4 * (s2 * e + np.abs(out) * (rel + (dout + 8) * ld(U)))
    else:
        b = 4 * (e + np.abs(out) * ld(U))
    return np.asarray(b, np.float64)


def scatter(x, labels, len_in):
    """-> (m_in, mu, C, W, B) of the fit's definition (W, B None without labels), float64."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    m_in = x[0] + np.mean(x - x[0], axis=0)
    v = _steps(Chain(m_in, len_in), x, np.float64)[0]
    mu = v[0] + np.mean(v - v[0], axis=0)
    c = v - mu
    C = c.T @ c / n
    W = B = None
    if labels is not None:
        labels = np.asarray(labels)
        W = np.zeros_like(C)
        B = np.zeros_like(C)
        for k in np.unique(labels):
            vk = v[labels == k]
            mk = vk.mean(axis=0)
            W += (vk - mk).T @ (vk - mk)
            B += len(vk) * np.outer(mk - mu, mk - mu)
        W /= n
        B /= n
    return m_in, mu, C, W, B


def fit(x, labels, kind, dout, len_in, len_out):
    """-> (Chain, eigenvalues or None).  kind 0 "centre", 1 "whiten", 2 "lda"; LinAlgError for a singular W, ValueError for
    a covariance of rank < dout."""
    x = np.asarray(x, np.float64)
    n, din = x.shape
    m_in, mu, C, W, B = scatter(x, labels if kind == 2 else None, len_in)
    if kind == 0:
        return Chain(m_in, len_in, None, mu, len_out), None
    if kind == 1:
        lam, Q = np.linalg.eigh(C)
        lam, Q = lam[::-1], Q[:, ::-1]
        if not lam[dout - 1] > n * din * U * lam[0]:
            raise ValueError("covariance of rank < dout")
        A = (Q[:, :dout] / np.sqrt(lam[:dout])).T
        return Chain(m_in, len_in, A, A @ mu, len_out), lam[:dout].copy()
    L = np.linalg.cholesky(W)
    Li = np.linalg.inv(L)
    G = Li @ B @ Li.T
    e, V = np.linalg.eigh((G + G.T) / 2)
    e, V = e[::-1], V[:, ::-1]
    A = (V[:, :dout].T) @ Li
    return Chain(m_in, len_in, A, A @ mu, len_out), e[:dout].copy()
