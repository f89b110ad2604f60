"""The NumPy restatement of the spectral clustering contract (include/plda_hip.h, "spectral clustering with auto-tuned
pruning"; csrc/spectral.hip): steps 1-6, every fp64 operation in the contract's order.  Steps 1, 2, 4 and 6 are exact, so the
GPU tests compare them with array_equal; step 3's eigenvalues come from numpy.linalg.eigh here and from the library's
eigensolver there, so the end-to-end comparison needs inputs whose decisions clear a margin (margins())."""
import numpy as np

SPECTRAL_MAX = 2048
SPECTRAL_MAX_SPK = 64
SPECTRAL_MAX_P = 16
P_FRACTIONS = (0.03, 0.05, 0.08, 0.12, 0.16, 0.2, 0.25, 0.3)


# ------------------------------------------------------------------------------------------------ steps 1 and 2
def similarity(S):
    """c(i, j) = ((double)S[i, j] + (double)S[j, i]) / 2; the diagonal is set to 0 and never used."""
    S = np.asarray(S, np.float32).astype(np.float64)
    c = (S + S.T) / 2.0
    np.fill_diagonal(c, 0.0)
    return c


def neighbours(c, p):
    """B [N, N] of 0 / 1: row i keeps its p_eff = min(p, N - 1) best partners j != i by (c descending, j ascending)."""
    n = c.shape[0]
    pe = min(int(p), n - 1)
    B = np.zeros((n, n), np.int64)
    for i in range(n):
        js = [j for j in range(n) if j != i]
        js.sort(key=lambda j: (-(c[i, j] + 0.0), j))        # (-0.0 + 0.0 == +0.0; Python compares floats with IEEE <)
        B[i, js[:pe]] = 1
    return B


def neighbours_fast(c, p):
    """The same by a stable argsort of -c (what the CPU tests hold neighbours() against, and what the GPU tests use)."""
    n = c.shape[0]
    pe = min(int(p), n - 1)
    key = -(c + 0.0)
    key[np.arange(n), np.arange(n)] = np.inf
    order = np.argsort(key, axis=1, kind="stable")
    B = np.zeros((n, n), np.int64)
    if pe > 0:
        np.put_along_axis(B, order[:, :pe], 1, axis=1)
    return B


def laplacian(B):
    """(L fp64 [N, N], deg2 int [N]) with A = (B + B^T) / 2, deg = sum_j A, L = diag(deg) - A; deg2 = 2 deg."""
    A2 = B + B.T
    deg2 = A2.sum(1)
    L = -0.5 * A2.astype(np.float64)
    L[np.arange(len(B)), np.arange(len(B))] = 0.5 * deg2
    return L + 0.0, deg2.astype(np.int32)


# ------------------------------------------------------------------------------------------------ steps 3 and 4
def gap_rule(lam_small, lam_n, n, p_eff, max_speakers):
    """(k_gap, r) from the min(max_speakers + 1, N) smallest eigenvalues ascending and the largest one."""
    kp = min(int(max_speakers), n - 1)
    kg, eb = 1, lam_small[1] - lam_small[0]
    for k in range(2, kp + 1):
        e = lam_small[k] - lam_small[k - 1]
        if e > eb:
            eb, kg = e, k
    g = eb / (lam_n + 1e-10)
    r = np.inf if g <= 0 else np.float64(p_eff) / g
    return kg, np.float64(r)


def eig_row(lam_asc, max_speakers):
    """One row of the `eig` output: the smallest eigenvalues, +inf behind them, lambda_N last."""
    n = len(lam_asc)
    row = np.full(max_speakers + 2, np.inf)
    have = min(max_speakers + 1, n)
    row[:have] = lam_asc[:have]
    row[-1] = lam_asc[-1]
    return row


def choose(eig_rows, n, p_row, max_speakers):
    """Steps 3-4 on the rows of an `eig` output [P, max_speakers + 2] -> (position used, p_used, k_gap, [r of every position])."""
    best, rs = None, []
    for pos, p in enumerate(p_row):
        pe = min(int(p), n - 1)
        kg, r = gap_rule(eig_rows[pos], eig_rows[pos][-1], n, pe, max_speakers)
        rs.append(r)
        if best is None or r < best[0] or (r == best[0] and pe < best[1]):
            best = (r, pe, pos, kg)
    return best[2], best[1], best[3], rs


# ------------------------------------------------------------------------------------------------ step 6
def _dist(U, m):
    d = np.zeros(U.shape[0])
    for c in range(U.shape[1]):
        t = U[:, c] - m[c]
        d = d + t * t
    return d


def kmeans(U, max_iters=20):
    """The contract's k-means on U [N, k] -> (labels int32 [N] renumbered by first occurrence, n_clusters)."""
    U = np.ascontiguousarray(U, np.float64)
    n, k = U.shape
    cen = np.zeros((k, k))
    cen[0] = U[0]
    mind = _dist(U, cen[0])
    for t in range(1, k):
        cen[t] = U[int(np.argmax(mind))]                    # (argmax: the first of the maxima = the lowest row)
        mind = np.minimum(mind, _dist(U, cen[t]))
    lab = np.full(n, -1)
    for _ in range(int(max_iters)):
        D = np.stack([_dist(U, cen[m]) for m in range(k)], 1)
        new = np.argmin(D, 1)                               # (the first of the minima = the lowest centre)
        moved = (new != lab).any()
        lab = new
        if not moved:
            break
        for m in range(k):
            idx = np.flatnonzero(lab == m)
            if len(idx):
                s = np.zeros(k)
                for i in idx:
                    s = s + U[i]
                cen[m] = s / np.float64(len(idx))
    out, seen = np.empty(n, np.int32), {}
    for i in range(n):
        out[i] = seen.setdefault(int(lab[i]), len(seen))
    return out, len(seen)


# ------------------------------------------------------------------------------------------------ the whole contract
def default_p(n, fractions=P_FRACTIONS):
    """p = min(N - 1, max(2, ceil(f N))) for every fraction (at least 1: a p_table entry is >= 1)."""
    return [max(1, min(n - 1, max(2, int(np.ceil(f * n))))) for f in fractions]


def spectral(S, p_row, max_speakers=16, num_speakers=0, max_iters=20):
    """One recording -> a dict of every output of the C ABI (eig [P, max_speakers + 2], embed [N, max_speakers], ...) plus
    "L" (the exact Laplacian at the value used), "rs" (r of every position) and "gaps" (the sorted gaps of every position)."""
    S = np.asarray(S, np.float32)
    n, ms = S.shape[0], int(max_speakers)
    P = len(p_row)
    if n == 1:
        row = np.full(ms + 2, np.inf)
        row[0] = row[-1] = 0.0
        emb = np.zeros((1, ms))
        emb[0, 0] = 1.0
        return {"labels": np.zeros(1, np.int32), "n_clusters": 1, "p_used": 0, "k_gap": 1, "eig": np.tile(row, (P, 1)), "embed": emb,
                "deg2": np.zeros(1, np.int32), "L": np.zeros((1, 1)), "rs": [np.inf] * P, "gaps": [np.zeros(0)] * P, "k": 1}
    c = similarity(S)
    rows, vecs, Ls, degs, gaps = [], [], [], [], []
    for p in p_row:
        L, deg2 = laplacian(neighbours_fast(c, p))
        lam, V = np.linalg.eigh(L)
        lam = np.maximum(lam, 0.0)
        rows.append(eig_row(lam, ms)); vecs.append(V); Ls.append(L); degs.append(deg2)
        kp = min(ms, n - 1)
        gaps.append(np.sort(np.diff(lam[:kp + 1]))[::-1])
    pos, p_used, k_gap, rs = choose(rows, n, p_row, ms)
    k = min(int(num_speakers), n) if num_speakers and num_speakers > 0 else k_gap
    U = vecs[pos][:, :k]
    labels, ncl = kmeans(U, max_iters)
    emb = np.zeros((n, ms))
    emb[:, :k] = U
    return {"labels": labels, "n_clusters": ncl, "p_used": p_used, "k_gap": k_gap, "eig": np.stack(rows), "embed": emb, "deg2": degs[pos],
            "L": Ls[pos], "rs": rs, "gaps": gaps, "k": k, "pos": pos}


def margins(res):
    """(the largest ratio second gap / first gap over the pruning values, the ratio winner's r / runner-up's r): the end-to-end
    comparison is meaningful when both are <= 1 - 1e-6 (a single pruning value has no runner-up: 0)."""
    gr = max((g[1] / g[0] if len(g) > 1 and g[0] > 0 else 0.0) for g in res["gaps"])
    rs = np.sort(np.unique(np.asarray(res["rs"], np.float64)))
    return gr, (rs[0] / rs[1] if len(rs) > 1 else 0.0)


# ------------------------------------------------------------------------------------------------ inputs
def planted(n, k, noise, seed, d=32):
    """(S fp32 [N, N] of dot products of unit-norm vectors around k random centres, the planted labels)."""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((k, d))
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    lab = np.arange(n) % k
    rng.shuffle(lab)
    x = cen[lab] + noise * rng.standard_normal((n, d)) / np.sqrt(d)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return (x @ x.T).astype(np.float32), lab


def quantised(n, levels, seed):
    """a block of `levels` distinct score values: ties everywhere"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, levels, (n, n)).astype(np.float32) - levels // 2) * np.float32(0.5)


def all_equal(n, value=1.5):
    return np.full((n, n), value, np.float32)


def same_partition(a, b):
    """True iff two labelings are the same partition."""
    a, b = np.asarray(a), np.asarray(b)
    return len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))
