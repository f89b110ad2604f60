"""The yardstick of the ROC convex hull (include/plda_hip.h, "ROC convex hull"): sort-based, in Python ints and fractions.
Full ROC -> lower hull (strict vertices) -> PAV segments -> minCllr by math.fsum -> the ROCCH-EER as an exact rational.
Nothing here is shared with the library: tests/test_rocch_model.py holds this file to a brute-force hull, to sklearn's
isotonic regression and to the closed forms, and holds the library to this file."""
import math
from fractions import Fraction

import numpy as np


def score_keys(scores):
    """uint32 keys: a < b <=> key(a) < key(b); -0.0 == +0.0."""
    u = np.ascontiguousarray(scores, np.float32).view(np.uint32).astype(np.int64)
    u[u == 0x80000000] = 0
    return np.where(u & 0x80000000, u ^ 0xffffffff, u | 0x80000000).astype(np.uint32)


def key_score(k):
    k = int(k)
    u = (k & 0x7fffffff) if (k & 0x80000000) else (k ^ 0xffffffff)
    return float(np.array([u], np.uint32).view(np.float32)[0])


def roc_points(pos, neg):
    """[(x, y, key)] of every cut in ascending order, the empty cut (0, 0, None) first: one point per distinct key.  (The
    sort and the running counts are NumPy's, on int64; the hull works on the Python ints.)"""
    kp, kn = np.sort(score_keys(pos)), np.sort(score_keys(neg))
    keys = np.unique(np.concatenate([kp, kn]))
    x = np.searchsorted(kn, keys, "right").tolist()
    y = np.searchsorted(kp, keys, "right").tolist()
    return [(0, 0, None)] + list(zip(x, y, keys.tolist()))


def cross(a, b, c):
    return (b[0] - a[0]) * (c[1] - b[1]) - (b[1] - a[1]) * (c[0] - b[0])


def lower_hull(pts):
    """Monotone chain over points ascending in (x, y): a middle point goes when the cross product is <= 0."""
    st = []
    for p in pts:
        while len(st) >= 2 and cross(st[-2], st[-1], p) <= 0:
            st.pop()
        st.append(p)
    return st


def brute_hull(pts):
    """The hull by definition, for tiny inputs: among all subsets that hold both end points, the one whose chain is strictly
    convex (every turn a left turn) and a minorant (every point on or to the left of every chain edge's line)."""
    from itertools import combinations
    pts = sorted(set((p[0], p[1]) for p in pts))
    inner, found = pts[1:-1], []
    for r in range(len(inner) + 1):
        for sub in combinations(inner, r):
            ch = [pts[0]] + list(sub) + [pts[-1]]
            if all(cross(a, b, c) > 0 for a, b, c in zip(ch, ch[1:], ch[2:])) and \
               all(cross(a, b, p) >= 0 for a, b in zip(ch, ch[1:]) for p in pts):
                found.append(ch)
    assert len(found) == 1, found
    return found[0]


def midpoint(k_lo, k_hi):
    s = key_score(k_lo)
    return s + (key_score(k_hi) - s) / 2.0


def model(pos, neg):
    """dict: np, nn, vertices [(x, y, fa, miss, key, has_key, threshold)], llr [float], min_cllr (float), eer (Fraction),
    eer_lo / eer_hi (the vertices around the crossing)."""
    pos, neg = np.asarray(pos, np.float32), np.asarray(neg, np.float32)
    Np, Nn = len(pos), len(neg)
    assert Np and Nn and np.all(np.isfinite(pos)) and np.all(np.isfinite(neg))
    pts = roc_points(pos, neg)
    keys = [p[2] for p in pts[1:]]
    nxt = dict(zip(keys, keys[1:]))
    hull = lower_hull(pts)
    verts = []
    for i, (x, y, k) in enumerate(hull):
        if k is None:
            thr = key_score(keys[0])
        elif i == len(hull) - 1:
            thr = math.inf
        else:
            thr = midpoint(k, nxt[k])
        verts.append((x, y, Nn - x, y, 0 if k is None else k, 0 if k is None else 1, thr))
    llr, tt, tn = [], [], []
    for a, b in zip(hull, hull[1:]):
        dn, dt = b[0] - a[0], b[1] - a[1]
        if dt == 0:
            llr.append(-math.inf)
        elif dn == 0:
            llr.append(math.inf)
        else:
            llr.append(math.log(Fraction(dt, dn)) - math.log(Fraction(Np, Nn)))
            tt.append(float(Fraction(dt, Np)) * math.log1p(Fraction(dn * Np, dt * Nn)))
            tn.append(float(Fraction(dn, Nn)) * math.log1p(Fraction(dt * Nn, dn * Np)))
    min_cllr = (math.fsum(tt) + math.fsum(tn)) / (2.0 * math.log(2.0))
    # the crossing with y / Np = 1 - x / Nn
    f = lambda p: Fraction(p[1], Np) + Fraction(p[0], Nn) - 1      # noqa: E731
    j = next(i for i, p in enumerate(hull) if f(p) >= 0)
    a, b = hull[j - 1], hull[j]
    t = -f(a) / (f(b) - f(a))
    eer = (a[1] + t * (b[1] - a[1])) / Np
    assert eer == 1 - (a[0] + t * (b[0] - a[0])) / Nn
    return {"np": Np, "nn": Nn, "vertices": verts, "llr": llr, "min_cllr": min_cllr, "eer": eer, "eer_lo": a, "eer_hi": b}


def reduced_points(pos, neg):
    """The library's reduced points by NumPy ranks: (edge_class, edge_key, other_lt, other_le, edge_lt, edge_le)."""
    kp, kn = np.sort(score_keys(pos)), np.sort(score_keys(neg))
    edge_class = 1 if len(kp) <= len(kn) else 0
    ke, ko = (kp, kn) if edge_class else (kn, kp)
    u = np.unique(ke)
    return (edge_class, u, np.searchsorted(ko, u, "left").astype(np.uint64), np.searchsorted(ko, u, "right").astype(np.uint64),
            np.searchsorted(ke, u, "left").astype(np.uint64), np.searchsorted(ke, u, "right").astype(np.uint64))


def neighbours(pos, neg, edges):
    """Per cut edge e ("reject every key <= e"; None: the empty cut): (largest key <= e, smallest key > e) among all keys,
    0 / 0xffffffff where there is none."""
    k = np.unique(np.concatenate([score_keys(pos), score_keys(neg)]))
    lo, hi = [], []
    for e in edges:
        i = 0 if e is None else int(np.searchsorted(k, e, "right"))
        lo.append(int(k[i - 1]) if i > 0 else 0)
        hi.append(int(k[i]) if i < len(k) else 0xffffffff)
    return np.array(lo, np.uint32), np.array(hi, np.uint32)


def pav_apply(m, scores, bound=0.0):
    """The PAV map of `model(...)` on fp32 scores -> fp32 (NaN stays NaN)."""
    s = np.asarray(scores, np.float32)
    inner = np.array([v[4] for v in m["vertices"][1:-1]], np.uint32)
    tab = np.array(m["llr"], np.float64)
    if bound > 0:
        tab = np.clip(tab, -bound, bound)
    out = tab.astype(np.float32)[np.searchsorted(inner, score_keys(s.reshape(-1)), "left")].reshape(s.shape)
    out[np.isnan(s)] = np.nan
    return out


def cllr_of_llrs(llr_pos, llr_neg):
    """Cllr of already-mapped scores in fp64 (an infinite llr on the right side costs 0, on the wrong side inf)."""
    with np.errstate(over="ignore"):
        ct = np.logaddexp(0.0, -np.asarray(llr_pos, np.float64)).mean()
        cn = np.logaddexp(0.0, np.asarray(llr_neg, np.float64)).mean()
    return float((ct + cn) / (2.0 * math.log(2.0)))


def ulp_distance(a, b):
    ia, ib = np.array([a, b], np.float64).view(np.int64)
    return abs(int(ia) - int(ib))
