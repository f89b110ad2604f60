"""tests/ahc_model.py -- the speaker clustering of include/plda_hip.h ("speaker clustering", csrc/ahc.hip) restated in NumPy,
to the bit: average-linkage agglomerative clustering on SUMS, every candidate value one fp64 division of a sum by an integer
product of sizes, the pair to merge the minimum under (v, a, b), -0.0 == +0.0.

    cluster_one(S, ...)          one recording, the working model: the matrix of candidate values is kept and only the merged
                                 row and column are recomputed (O(N^2) per merge for the argmin, N ~ 500 in under a second)
    cluster_one_definition(S,..) the definition itself: every live pair re-evaluated at every step (O(N^3); small N only) --
                                 tests/test_ahc_model.py holds the two equal
    cluster(blocks, ...)         R recordings -> the arrays of the C ABI (labels, n_clusters, merge record with its -1 / +inf tails)

The row-major argmin over the upper triangle IS the lexicographic tie-break: NumPy's argmin returns the first of equal minima
and compares with <, under which -0.0 and +0.0 are equal.
"""
import numpy as np


class NonFinite(ValueError):
    def __init__(self, count):
        ValueError.__init__(self, "%d non-finite scores" % count)
        self.count = count


def costs(S):
    """c(i, j) = -((double)S[i, j] + (double)S[j, i]) / 2, exact in fp64; the diagonal is never read (set to 0 here)."""
    S = np.asarray(S)
    assert S.dtype == np.float32 and S.ndim == 2 and S.shape[0] == S.shape[1]
    n = S.shape[0]
    off = ~np.eye(n, dtype=bool)
    bad = int(np.count_nonzero(~np.isfinite(S[off])))
    if bad:
        raise NonFinite(bad)
    Sd = np.where(off, S, np.float32(0)).astype(np.float64)
    return -((Sd + Sd.T) / 2.0)


def _stops(k, v, threshold, min_clusters):
    if k <= max(1, int(min_clusters)):
        return True
    return threshold is not None and not (v <= -np.float64(threshold))


def _finish(n, slot_of, merges):
    live = np.unique(slot_of)
    labels = np.searchsorted(live, slot_of).astype(np.int32)
    ma = np.full(max(n - 1, 0), -1, np.int32)
    mb = np.full(max(n - 1, 0), -1, np.int32)
    mc = np.full(max(n - 1, 0), np.inf, np.float64)
    for i, (a, b, v) in enumerate(merges):
        ma[i], mb[i], mc[i] = a, b, v
    return labels, len(live), ma, mb, mc


def cluster_one(S, threshold=None, min_clusters=1):
    """-> (labels int32 [N], k, merge_a, merge_b, merge_cost [N - 1])."""
    sums = costs(S)
    n = sums.shape[0]
    size = np.ones(n, np.int64)
    alive = np.ones(n, bool)
    slot_of = np.arange(n)
    V = np.where(np.triu(np.ones((n, n), bool), 1), sums, np.inf)      # sizes are 1: v = sum / 1.0 = sum
    merges = []
    k = n
    while k > 1:
        flat = int(np.argmin(V))
        a, b = divmod(flat, n)
        v = V[a, b]
        if _stops(k, v, threshold, min_clusters):
            break
        merges.append((a, b, v))
        others = alive.copy()
        others[a] = others[b] = False
        x = np.nonzero(others)[0]
        s = sums[a, x] + sums[b, x]                       # one addition, the operands in this order
        sums[a, x] = s
        sums[x, a] = s
        size[a] += size[b]
        alive[b] = False
        slot_of[slot_of == b] = a
        V[b, :] = np.inf
        V[:, b] = np.inf
        vn = s / (size[a] * size[x]).astype(np.float64)   # integer product, one conversion, one division
        lo, hi = x < a, x > a
        V[x[lo], a] = vn[lo]
        V[a, x[hi]] = vn[hi]
        k -= 1
    return _finish(n, slot_of, merges)


def cluster_one_definition(S, threshold=None, min_clusters=1):
    """The definition: all live pairs re-evaluated at every step."""
    sums = costs(S)
    n = sums.shape[0]
    size = np.ones(n, np.int64)
    alive = np.ones(n, bool)
    slot_of = np.arange(n)
    upper = np.triu(np.ones((n, n), bool), 1)
    merges = []
    k = n
    while k > 1:
        mask = upper & alive[:, None] & alive[None, :]
        prod = (size[:, None] * size[None, :]).astype(np.float64)
        V = np.where(mask, sums / prod, np.inf)
        a, b = divmod(int(np.argmin(V)), n)
        v = V[a, b]
        if _stops(k, v, threshold, min_clusters):
            break
        merges.append((a, b, v))
        for x in range(n):
            if alive[x] and x != a and x != b:
                sums[a, x] = sums[a, x] + sums[b, x]
                sums[x, a] = sums[a, x]
        size[a] += size[b]
        alive[b] = False
        slot_of[slot_of == b] = a
        k -= 1
    return _finish(n, slot_of, merges)


def cluster(blocks, threshold=None, min_clusters=None, one=cluster_one):
    """R recordings -> (labels [T], n_clusters [R], merge_a, merge_b, merge_cost [T - R]) as the C ABI lays them out."""
    r = len(blocks)
    minc = np.broadcast_to(np.asarray(1 if min_clusters is None else min_clusters), (r,))
    L, K, A, B, Cc = [], [], [], [], []
    for q, S in enumerate(blocks):
        labels, k, ma, mb, mc = one(np.asarray(S, np.float32), threshold, int(minc[q]))
        L.append(labels); K.append(k); A.append(ma); B.append(mb); Cc.append(mc)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return cat(L, np.int32), np.asarray(K, np.int32), cat(A, np.int32), cat(B, np.int32), cat(Cc, np.float64)


# ---- data families shared by the CPU and GPU tests
def gaussian(n, seed):
    return np.random.default_rng(seed).standard_normal((n, n)).astype(np.float32)


def integers(n, seed):
    """integer scores in -2 .. 2: ties everywhere, the row cache is invalidated at almost every merge"""
    return np.random.default_rng(seed).integers(-2, 3, (n, n)).astype(np.float32)


def chain(n, reverse=False):
    """S[i, j] = -|i - j| (reverse: the indices mirrored after a shift that makes the far end the cheap one)"""
    i = np.arange(n)
    d = np.abs(i[:, None] - i[None, :]).astype(np.float32)
    if reverse:
        w = (n - np.minimum(i[:, None], i[None, :])).astype(np.float32)      # pairs near the END are the closest
        return (-d * w).astype(np.float32)
    return -d


def all_equal(n, value=0.25):
    return np.full((n, n), value, np.float32)


def signed_zeros(n, seed):
    """+0.0 and -0.0 at random, asymmetrically: costs of +0.0 and -0.0 that must compare equal"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((n, n)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)


def planted(sizes, seed=None):
    """+1 inside a group, -1 across; the groups interleaved at random (seed) or contiguous (None) -> (S, group of each row)"""
    g = np.repeat(np.arange(len(sizes)), sizes)
    if seed is not None:
        g = np.random.default_rng(seed).permutation(g)
    return np.where(g[:, None] == g[None, :], np.float32(1), np.float32(-1)).astype(np.float32), g


def first_member_labels(g):
    """the groups numbered by their first member: what labels-by-ascending-slot gives for a recovered partition"""
    _, first = np.unique(g, return_index=True)
    order = np.argsort(first)
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return rank[np.searchsorted(np.unique(g), g)].astype(np.int32)
