"""Host model of the multi-system score fusion (plda_amd/csrc/fusion.hip), for the tests: the definitions of
include/plda_hip.h ("multi-system score fusion") restated in NumPy fp64, independent of the product's arithmetic.

  chain(S, a, c)          the fused value y of K fp32 score arrays: c, then one a_k * s_k + y rounded once per step (np.longdouble
                          carries the step to 64 bits before the fp64 rounding; where that double rounding matters a test
                          decides with chain_exact).
  chain_exact(S, a, c)    the same chain on fractions.Fraction (float(Fraction) rounds correctly): the bit-exact reference of
                          the map and of y, for small arrays.
  pass_record(pos, neg, a, c, theta)   one fusion pass over K parallel target arrays and K parallel non-target arrays: per
                          class L, G[K + 1], H[(K + 1)(K + 2) / 2] (t(i, j) = j (j + 1) / 2 + i), the exact counts, the extremes.
                          Terms in fp64, sums chunk by chunk in np.longdouble combined with math.fsum.  `abs` holds
                          sum |term| per sum (the scale of the 1e-12 band) and `Ymax` = max (|c| + sum |a_k s_k|).
  pass_matrices(S, espk, tspk, ...)    the same with the labelling rule of the matrix form.
  objective / gradient / hessian       F(x; pi) and its derivatives from ONE record taken at c = b + logit(pi),
                                       x = (b, a_0 .. a_{K-1}).
  newton(rec, prior)      the step of the header: unit-diagonal scaling, Cholesky, (F, d, lambda2); ValueError naming the system.
  fit(pos, neg, prior, tol, max_iter, take_pass, step)   the damped Newton iteration of the header.
The record is the dict of plda_amd/fusion.py (K, Np, Nn, miss, fa, nonfinite, smin, smax, ymin_t .. ymax_n, L_*, G_*, H_*)."""
import math
from fractions import Fraction

import numpy as np

LN2 = math.log(2.0)
CHUNK = 1 << 20
PIVOT_MIN = 1e-12


def logit(p):
    return math.log(p / (1.0 - p))


def n_h(k):
    return (k + 1) * (k + 2) // 2


def t_index(i, j):
    return j * (j + 1) // 2 + i


def _f64(S):
    return [np.asarray(s, np.float32).astype(np.float64).reshape(-1) for s in S]


def chain(S, a, c):
    y = np.full(_f64(S)[0].shape, c, np.float64)
    for ak, s in zip(a, _f64(S)):
        y = (np.longdouble(ak) * s.astype(np.longdouble) + y.astype(np.longdouble)).astype(np.float64)
    return y


def chain_exact(S, a, c):
    cols = _f64(S)
    out = np.empty(cols[0].shape[0], np.float64)
    fa = [Fraction(float(x)) for x in a]
    for t in range(out.shape[0]):
        y = float(c)
        for ak, s in zip(fa, cols):
            y = float(ak * Fraction(float(s[t])) + Fraction(y))          # one correctly rounded fma
        out[t] = y
    return out


def map_exact(S, a, b):
    """(float)chain: the fp64 chain value rounded once to fp32."""
    return chain_exact(S, a, b).astype(np.float32)


def terms(S, a, c, target):
    """([1 + (K + 1) + n_h(K), n] per-trial terms in the order L, G[0 .. K], H[0 ..), y, Y)."""
    cols = _f64(S)
    k = len(cols)
    y = chain(S, a, c)
    Y = abs(c) + sum(abs(ak) * np.abs(s) for ak, s in zip(a, cols))
    e = np.exp(-np.abs(y))
    l1p = np.log1p(e)
    d = 1.0 + e
    pos = y >= 0.0
    p = np.where(pos, 1.0 / d, e / d)
    q = np.where(pos, e / d, 1.0 / d)
    w = e / (d * d)
    if target:
        L, g = np.maximum(-y, 0.0) + l1p, q
    else:
        L, g = np.maximum(y, 0.0) + l1p, p
    phi = [np.ones_like(y)] + cols
    rows = [L] + [g * phi[j] for j in range(k + 1)]
    H = [None] * n_h(k)
    for j in range(k + 1):
        for i in range(j + 1):
            H[t_index(i, j)] = w * phi[i] * phi[j]
    return np.stack(rows + H), y, Y


class Acc(object):
    """Chunk-wise accumulator of one record."""

    def __init__(self, k):
        self.k = k
        self.ne = 1 + (k + 1) + n_h(k)
        self.parts = [[[] for _ in range(self.ne)] for _ in (0, 1)]
        self.aparts = [[[] for _ in range(self.ne)] for _ in (0, 1)]
        self.count = [0, 0]
        self.miss = self.fa = self.nonfinite = 0
        self.ylo, self.yhi = [math.inf, math.inf], [-math.inf, -math.inf]
        self.slo = np.full(k, np.inf, np.float32)
        self.shi = np.full(k, -np.inf, np.float32)
        self.Ymax = 0.0
        self.y = [[], []]                      # every chain value per class (the tests place theta between two of them)

    def add(self, S, a, c, theta, target):
        S = [np.asarray(s, np.float32).reshape(-1) for s in S]
        cl = 1 if target else 0
        n = S[0].shape[0]
        for i in range(0, n, CHUNK):
            X = [s[i:i + CHUNK] for s in S]
            if X[0].shape[0] == 0:
                continue
            self.count[cl] += int(X[0].shape[0])
            bad = np.zeros(X[0].shape[0], bool)
            for j, x in enumerate(X):
                bad |= ~np.isfinite(x)
                self.slo[j] = min(self.slo[j], x.min())
                self.shi[j] = max(self.shi[j], x.max())
            self.nonfinite += int(bad.sum())
            with np.errstate(all="ignore"):
                t, y, Y = terms(X, a, c, target)
                t = t.astype(np.longdouble)
            if target:
                self.miss += int((y < theta).sum())
            else:
                self.fa += int((y >= theta).sum())
            self.ylo[cl], self.yhi[cl] = min(self.ylo[cl], float(y.min())), max(self.yhi[cl], float(y.max()))
            self.Ymax = max(self.Ymax, float(Y.max()))
            self.y[cl].append(y)
            for e in range(self.ne):
                self.parts[cl][e].append(float(t[e].sum()))
                self.aparts[cl][e].append(float(np.abs(t[e]).sum()))

    def record(self):
        k = self.k
        r = {"K": k, "Np": self.count[1], "Nn": self.count[0], "miss": self.miss, "fa": self.fa, "nonfinite": self.nonfinite,
             "smin": self.slo.copy(), "smax": self.shi.copy(), "Ymax": self.Ymax, "abs": {},
             "y_t": np.concatenate(self.y[1]) if self.y[1] else np.zeros(0), "y_n": np.concatenate(self.y[0]) if self.y[0] else np.zeros(0)}
        for cl, cls in ((1, "t"), (0, "n")):
            r["ymin_" + cls], r["ymax_" + cls] = self.ylo[cl], self.yhi[cl]
            for dst, src in ((r, self.parts), (r["abs"], self.aparts)):
                v = [math.fsum(src[cl][e]) for e in range(self.ne)]
                dst["L_" + cls] = v[0]
                dst["G_" + cls] = np.array(v[1:k + 2])
                dst["H_" + cls] = np.array(v[k + 2:])
        return r


def pass_record(pos, neg, a, c, theta=0.0):
    acc = Acc(len(pos))
    acc.add(pos, a, c, theta, True)
    acc.add(neg, a, c, theta, False)
    return acc.record()


def split(S, espk, tspk):
    """(K target arrays, K non-target arrays) of K labelled matrices: trial (i, j) is a target iff espk[i] == tspk[j]."""
    lab = np.asarray(espk)[:, None] == np.asarray(tspk)[None, :]
    S = [np.asarray(s, np.float32) for s in S]
    return [s[lab] for s in S], [s[~lab] for s in S]


def pass_matrices(S, espk, tspk, a, c, theta=0.0):
    pos, neg = split(S, espk, tspk)
    return pass_record(pos, neg, a, c, theta)


def check(rec):
    if rec["nonfinite"]:
        raise ValueError("%d trials with a non-finite score" % rec["nonfinite"])
    if rec["Np"] == 0 or rec["Nn"] == 0:
        raise ValueError("need at least one target and one non-target trial")


def _weights(rec, prior):
    return prior / rec["Np"], (1.0 - prior) / rec["Nn"]


def objective(rec, prior):
    wt, wn = _weights(rec, prior)
    return wt * rec["L_t"] + wn * rec["L_n"]


def gradient(rec, prior):
    wt, wn = _weights(rec, prior)
    return np.array([-wt * float(t) + wn * float(n) for t, n in zip(rec["G_t"], rec["G_n"])])


def hessian(rec, prior):
    wt, wn = _weights(rec, prior)
    n = rec["K"] + 1
    H = np.zeros((n, n))
    for j in range(n):
        for i in range(j + 1):
            H[i, j] = H[j, i] = wt * float(rec["H_t"][t_index(i, j)]) + wn * float(rec["H_n"][t_index(i, j)])
    return H


def _who(j):
    return "the offset" if j == 0 else "system %d" % (j - 1)


def newton(rec, prior):
    """(F, d, lambda2) of the header's step, every operation in the order of the library's (plain Python floats)."""
    n = rec["K"] + 1
    F = objective(rec, prior)
    g = [float(x) for x in gradient(rec, prior)]
    H = hessian(rec, prior)
    sc = []
    for j in range(n):
        if not H[j, j] > 0.0:
            raise ValueError("the Hessian's diagonal entry of %s is not positive" % _who(j))
        sc.append(1.0 / math.sqrt(float(H[j, j])))
    L = [[0.0] * n for _ in range(n)]
    for j in range(n):
        for i in range(j + 1):
            v = (float(H[j, i]) * sc[j]) * sc[i]
            for k in range(i):
                v -= L[j][k] * L[i][k]
            if i < j:
                L[j][i] = v / L[i][i]
            else:
                if not v > PIVOT_MIN:
                    raise ValueError("the Cholesky pivot of %s is <= 1e-12" % _who(j))
                L[j][j] = math.sqrt(v)
    z, lam = [0.0] * n, 0.0
    for j in range(n):
        v = g[j] * sc[j]
        for k in range(j):
            v -= L[j][k] * z[k]
        z[j] = v / L[j][j]
        lam += z[j] * z[j]
    x = [0.0] * n
    for j in range(n - 1, -1, -1):
        v = z[j]
        for k in range(j + 1, n):
            v -= L[k][j] * x[k]
        x[j] = v / L[j][j]
    return F, np.array([-(x[j] * sc[j]) for j in range(n)]), lam


def fit(pos, neg, prior=0.5, tol=1e-18, max_iter=100, take_pass=None, step=None, trace=None):
    """The damped Newton iteration of the header on x = (b, a_0 ..).  take_pass(a, c) -> record (default: pass_record on
    pos / neg); step(record, prior) -> (F, d, lambda2) (default: `newton`; the CPU test passes the library's own).
    Returns a dict with the fields of plda_fusion_fit."""
    if not 0.0 < prior < 1.0:
        raise ValueError("prior outside (0, 1)")
    take = take_pass or (lambda a, c: pass_record(pos, neg, np.zeros(len(pos)) if a is None else a, c))
    step = step or newton
    tau = logit(prior)
    rec = take(None, tau)                      # a = None: the start, every weight 0
    k = rec["K"]
    check(rec)
    passes = 1
    for j in range(k):
        if rec["smin"][j] == rec["smax"][j]:
            raise ValueError("system %d is constant" % j)
    x = np.zeros(k + 1)
    it, lam2, converged = 0, float("inf"), False
    while True:
        try:
            F, d, lam2 = step(rec, prior)
        except Exception:
            if it > 0 and rec["ymin_t"] > rec["ymax_n"]:      # separable and run away: the iteration stops here
                break
            raise
        if trace is not None:
            trace.append((it, x.copy(), F, lam2))
        if lam2 <= tol:
            converged = True
            break
        if it >= max_iter:
            break
        t, accepted = 1.0, False
        for _ in range(31):
            nx = x + t * d
            trial = take(nx[1:], nx[0] + tau)
            passes += 1
            if objective(trial, prior) <= F - 1e-4 * t * lam2 + 2.0 ** -44 * abs(F):
                accepted = True
                break
            t *= 0.5
        if not accepted:
            break
        x, rec = nx, trial
        it += 1
    if prior == 0.5:
        after = rec
    else:
        after = take(x[1:], x[0])
        passes += 1
    return {"a": x[1:].copy(), "b": float(x[0]), "objective": objective(rec, prior) / LN2, "cllr_after": objective(after, 0.5) / LN2,
            "lambda2": lam2, "iterations": it, "passes": passes, "converged": converged,
            "separable": bool(rec["ymin_t"] > rec["ymax_n"])}

