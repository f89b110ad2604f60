"""Host model of the exact minimum detection cost (include/plda_hip.h, "exact minimum detection cost"): the definition by
sorting, a brute-force count for small sets, and a driver that runs the library's exported host step level by level with
NumPy histograms standing in for the kernels (no GPU).

A cut is "reject every trial whose key is <= k" for a key present in the data, plus the cut that rejects nothing; its cost
at (prior, c_miss, c_fa) is v = ((c_miss * prior) * miss) / Np + ((c_fa * (1 - prior)) * fa) / Nn in float64, exactly the
expression of plda_amd/calibration.py:act_dcf; the smallest v wins, the lowest cut among equal v; the normalised
figure reported is min(v / min(c_miss * prior, c_fa * (1 - prior)), 1)."""
import numpy as np

SHIFTS, BITS = (21, 10, 0), (11, 11, 10)


def keys(f):
    """The order-preserving uint32 key of fp32 scores (-0.0 == +0.0)."""
    u = np.ascontiguousarray(f, np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_score(k):
    """The score of a key, as float64 (the zero comes back as +0.0)."""
    k = np.asarray(k, np.uint32)
    u = np.where((k & np.uint32(0x80000000)) != 0, k & np.uint32(0x7fffffff), ~k).astype(np.uint32)
    return u.view(np.float32).astype(np.float64)


def value(point, miss, fa, n_pos, n_neg):
    pi, cm, cf = (float(x) for x in point)
    return ((cm * pi) * np.asarray(miss, np.float64)) / float(n_pos) + ((cf * (1.0 - pi)) * np.asarray(fa, np.float64)) / float(n_neg)


def _report(point, v, miss, fa, n_pos, n_neg, i, allk):
    pi, cm, cf = (float(x) for x in point)
    if i == 0:
        thr = float(key_score(allk[0]))
    elif i == len(allk):
        thr = float("inf")
    else:
        s, s2 = float(key_score(allk[i - 1])), float(key_score(allk[i]))
        thr = s + (s2 - s) / 2.0
    # (min(., 1): the better trivial cut costs exactly 1 in exact arithmetic; above 1 the quotient is rounding alone)
    return {"min_dcf": min(float(v) / min(cm * pi, cf * (1.0 - pi)), 1.0), "threshold": thr, "far": float(fa) / float(n_neg),
            "frr": float(miss) / float(n_pos), "miss": int(miss), "fa": int(fa), "cut": i}


def model(pos, neg, points):
    """The definition: sort, cumulative counts, first minimum.  One dict per point; "cut" = number of distinct keys
    rejected."""
    kp, kn = np.sort(keys(pos)), np.sort(keys(neg))
    allk = np.unique(np.concatenate([kp, kn]))
    miss = np.concatenate([[0], np.searchsorted(kp, allk, side="right")])
    fa = np.concatenate([[len(kn)], len(kn) - np.searchsorted(kn, allk, side="right")])
    out = []
    for pt in points:
        v = value(pt, miss, fa, len(kp), len(kn))
        i = int(np.argmin(v))                    # the first minimum is the lowest cut
        out.append(_report(pt, v[i], miss[i], fa[i], len(kp), len(kn), i, allk))
    return out


def brute(pos, neg, points):
    """O(n^2): every cut counted on its own with comparisons of the SCORES (not the keys)."""
    pos, neg = np.asarray(pos, np.float32), np.asarray(neg, np.float32)
    cand = sorted(set(float(x) for x in np.concatenate([pos, neg])))     # -0.0 == 0.0 collapse in the set
    cuts = [(0, len(neg))] + [(int(np.sum(pos <= np.float32(c))), int(np.sum(neg > np.float32(c)))) for c in cand]
    out = []
    for pt in points:
        best = None
        for i, (m, f) in enumerate(cuts):
            v = float(value(pt, m, f, len(pos), len(neg)))
            if best is None or v < best[0]:
                best = (v, m, f, i)
        out.append(best)
    return out


def refine(pos, neg, points, slots_chunk=None):
    """The whole refinement through the library's host step (`plda_amd.dcf.host_step` / `host_finish`), the per-node
    histograms made with NumPy.  slots_chunk: nodes handed to one host step (None: a level at once).  Returns (results,
    survivors per level as lists of (prefix, miss_below, nn_below), state)."""
    from plda_amd import dcf as D
    kp, kn = keys(pos), keys(neg)
    state = np.zeros(1, D.STATE_DTYPE)
    nodes = np.zeros(1, D.NODE_DTYPE)
    survivors = []
    for level in range(3):
        if len(nodes) == 0:
            break
        sh, nb, hi = SHIFTS[level], 1 << BITS[level], SHIFTS[level] + BITS[level]
        hist = np.zeros((len(nodes), 2, 2048), np.uint64)
        for i, nd in enumerate(nodes):
            sp = kp if level == 0 else kp[(kp >> np.uint32(hi)) == nd["prefix"]]
            sn = kn if level == 0 else kn[(kn >> np.uint32(hi)) == nd["prefix"]]
            hist[i, 1, :nb] = np.bincount(((sp >> np.uint32(sh)) & np.uint32(nb - 1)).astype(np.int64), minlength=nb)
            hist[i, 0, :nb] = np.bincount(((sn >> np.uint32(sh)) & np.uint32(nb - 1)).astype(np.int64), minlength=nb)
        step = len(nodes) if not slots_chunk else int(slots_chunk)
        nxt = []
        for c0 in range(0, len(nodes), step):
            rc, got = D.host_step(level, nodes[c0:c0 + step], hist[c0:c0 + step], points, state, 2048 * step)
            if rc != 0:
                return rc, survivors, state
            nxt.append(got)
        nodes = np.concatenate(nxt) if nxt else np.zeros(0, D.NODE_DTYPE)
        survivors.append([(int(n["prefix"]), int(n["miss_below"]), int(n["nn_below"])) for n in nodes])
    allk = np.unique(np.concatenate([kp, kn]))
    below, above = [], []
    for p in range(len(points)):
        cut = state[0]["best"][p]
        idx = int(np.searchsorted(allk, cut["edge"], side="right")) if cut["has_edge"] else 0
        below.append(int(allk[idx - 1]) if idx > 0 else 0)
        above.append(int(allk[idx]) if idx < len(allk) else 0xffffffff)
    rc, res = D.host_finish(state, points, below, above)
    return (rc if rc != 0 else res), survivors, state


def same(a, b):
    """Bit-for-bit equality of two result dicts (value, counts, threshold, rates)."""
    f = lambda x: np.float64(x).tobytes()        # noqa: E731
    return (a["miss"] == b["miss"] and a["fa"] == b["fa"]
            and all(f(a[k]) == f(b[k]) for k in ("min_dcf", "threshold", "far", "frr")))


# ---------------------------------------------------------------------------------------------- the cases of the tests
NIST = ((0.01, 1.0, 1.0), (0.005, 1.0, 1.0))
FIVE = ((0.01, 1.0, 1.0), (0.05, 1.0, 1.0), (0.001, 1.0, 1.0), (0.5, 1.0, 1.0), (0.005, 10.0, 1.0))


def gaussian_lists(seed, n_pos, n_neg, mu_t, sd_t, mu_n, sd_n, quantum=None):
    rng = np.random.default_rng(seed)
    pos, neg = rng.normal(mu_t, sd_t, n_pos), rng.normal(mu_n, sd_n, n_neg)
    if quantum:
        pos, neg = np.round(pos / quantum) * quantum, np.round(neg / quantum) * quantum
    return pos.astype(np.float32), neg.astype(np.float32)


def flat_cost_lists(n=6000):
    """Targets and non-targets alternating over 20 octaves: at prior = 1/2 the cost after every pair is the same, so the
    bound prunes nothing at level 0."""
    s = np.exp(np.linspace(np.log(1e-3), np.log(1e3), 2 * n)).astype(np.float32)
    assert len(np.unique(s)) == 2 * n
    return s[0::2].copy(), s[1::2].copy()


def labelled_matrix(seed, m, nt, speakers, mu_t=2.5, quantum=None):
    """A Gaussian trials matrix N(0, 1) with the target trials shifted by mu_t, and the speaker ids of both sides."""
    rng = np.random.default_rng(seed)
    espk = rng.integers(0, speakers, m).astype(np.int64)
    tspk = rng.integers(0, speakers, nt).astype(np.int64)
    s = rng.standard_normal((m, nt), dtype=np.float32)
    s += np.float32(mu_t) * (espk[:, None] == tspk[None, :]).astype(np.float32)
    if quantum:
        s = (np.round(s / np.float32(quantum)) * np.float32(quantum)).astype(np.float32)
    return s, espk, tspk


def split(s, espk, tspk):
    tgt = espk[:, None] == tspk[None, :]
    return s[tgt], s[~tgt]
