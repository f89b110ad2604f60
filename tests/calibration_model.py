"""Host model of the score calibration (plda_amd/csrc/calib.hip), for the tests: the definitions of include/plda_hip.h
("linear score calibration") restated in NumPy fp64, independent of the product's arithmetic.

  pass_record(pos, neg, a, c, theta)   one calibration pass over target / non-target fp32 scores: per class the six sums
                         L, G0, G1, H0, H1, H2 of y = a * (double)s + c in the overflow-free forms of the header, the exact
                         counts and the fp32 extremes.  Every term is evaluated in fp64; the sums are taken chunk by chunk
                         in np.longdouble and combined with math.fsum, so that their error is far below the 1e-12 band the
                         device is held to.  `abs` holds sum |term| per sum (the scale of that band).
  pass_matrix(S, espk, tspk, ...)      the same with the labelling rule of the matrix forms, row chunk by row chunk.
  objective / gradient / hessian       F(a, b; pi) and its derivatives from ONE record taken at c = b + logit(pi).
  fit(pos, neg, prior, tol, max_iter)  the damped Newton iteration of the header on `pass_record` (or on `take_pass`).
  cllr, act_dcf, bayes_theta, apply_map
"""
import math

import numpy as np

LN2 = math.log(2.0)
SUMS = ("L", "G0", "G1", "H0", "H1", "H2")
CHUNK = 1 << 22


def logit(p):
    return math.log(p / (1.0 - p))


def terms(s32, a, c, target, fast=False):
    """The six per-trial terms [6, n] (fp64) of one class."""
    s = np.asarray(s32, np.float32).astype(np.float64)
    if fast:
        y = a * s + c                                # two roundings: one ulp of y, inside the (|y| + c0) u of the band
    else:
        y = (np.longdouble(a) * s.astype(np.longdouble) + np.longdouble(c)).astype(np.float64)      # a * s + c rounded once
    e = np.exp(-np.abs(y))
    l1p = np.log1p(e)
    d = 1.0 + e
    pos = y >= 0.0
    p = np.where(pos, 1.0 / d, e / d)           # sigmoid(y)
    q = np.where(pos, e / d, 1.0 / d)           # 1 - sigmoid(y)
    w = e / (d * d)
    if target:
        L, g = np.maximum(-y, 0.0) + l1p, q
    else:
        L, g = np.maximum(y, 0.0) + l1p, p
    return np.stack([L, g, g * s, w, w * s, w * s * s])


class Acc(object):
    """Chunk-wise accumulator of one record.  fast=True (the 1e9-trial test): chunk sums by NumPy's pairwise fp64
    summation instead of np.longdouble -- an error of about log2(chunk) u = 2.4e-15 of sum|term|, still 400 times
    below the band."""

    def __init__(self, fast=False):
        self.fast = fast
        self.parts = {(k, n): [] for k in (0, 1) for n in SUMS}
        self.aparts = {(k, n): [] for k in (0, 1) for n in SUMS}
        self.count = [0, 0]
        self.miss = self.fa = self.nonfinite = 0
        self.lo = [np.float32(np.inf), np.float32(np.inf)]
        self.hi = [np.float32(-np.inf), np.float32(-np.inf)]

    def add(self, s32, a, c, theta, target):
        s32 = np.asarray(s32, np.float32).reshape(-1)
        k = 1 if target else 0
        for i in range(0, s32.shape[0], CHUNK):
            x = s32[i:i + CHUNK]
            self.count[k] += int(x.shape[0])
            self.nonfinite += int((~np.isfinite(x)).sum())
            if target:
                self.miss += int((x.astype(np.float64) < theta).sum())
            else:
                self.fa += int((x.astype(np.float64) >= theta).sum())
            self.lo[k] = min(self.lo[k], x.min())
            self.hi[k] = max(self.hi[k], x.max())
            with np.errstate(all="ignore"):
                t = terms(x, a, c, target, self.fast)
                if not self.fast:
                    t = t.astype(np.longdouble)
            for j, n in enumerate(SUMS):
                self.parts[(k, n)].append(float(t[j].sum()))
                self.aparts[(k, n)].append(float(np.abs(t[j]).sum()))

    def record(self):
        r = {"Np": self.count[1], "Nn": self.count[0], "miss": self.miss, "fa": self.fa, "nonfinite": self.nonfinite,
             "min_t": self.lo[1], "max_t": self.hi[1], "min_n": self.lo[0], "max_n": self.hi[0], "abs": {}}
        for k, cls in ((1, "t"), (0, "n")):
            for n in SUMS:
                r[n + "_" + cls] = math.fsum(self.parts[(k, n)])
                r["abs"][n + "_" + cls] = math.fsum(self.aparts[(k, n)])
        return r


def pass_record(pos, neg, a, c, theta=0.0):
    acc = Acc()
    acc.add(pos, a, c, theta, True)
    acc.add(neg, a, c, theta, False)
    return acc.record()


def split(S, espk, tspk):
    """(pos, neg) of a labelled matrix: trial (i, j) is a target iff espk[i] == tspk[j]."""
    S = np.asarray(S, np.float32)
    lab = np.asarray(espk)[:, None] == np.asarray(tspk)[None, :]
    return S[lab], S[~lab]


def pass_matrix(S, espk, tspk, a, c, theta=0.0, rows=256):
    S = np.asarray(S, np.float32)
    espk, tspk = np.asarray(espk), np.asarray(tspk)
    acc = Acc()
    for r0 in range(0, S.shape[0], rows):
        pos, neg = split(S[r0:r0 + rows], espk[r0:r0 + rows], tspk)
        acc.add(pos, a, c, theta, True)
        acc.add(neg, a, c, theta, False)
    return acc.record()


def check(rec):
    if rec["nonfinite"]:
        raise ValueError("%d non-finite scores" % rec["nonfinite"])
    if rec["Np"] == 0 or rec["Nn"] == 0:
        raise ValueError("need at least one target and one non-target trial")


def _weights(rec, prior):
    return prior / rec["Np"], (1.0 - prior) / rec["Nn"]


def objective(rec, prior):
    wt, wn = _weights(rec, prior)
    return wt * rec["L_t"] + wn * rec["L_n"]


def gradient(rec, prior):
    wt, wn = _weights(rec, prior)
    return np.array([-wt * rec["G1_t"] + wn * rec["G1_n"], -wt * rec["G0_t"] + wn * rec["G0_n"]])


def hessian(rec, prior):
    wt, wn = _weights(rec, prior)
    h = [wt * rec[n + "_t"] + wn * rec[n + "_n"] for n in ("H2", "H1", "H0")]
    return np.array([[h[0], h[1]], [h[1], h[2]]])


def solve2(H, g):
    """(d, lambda2) with H d = -g, lambda2 = g' H^-1 g; None if H is not positive definite in fp64 (Cholesky)."""
    h00, h01, h11 = float(H[0, 0]), float(H[0, 1]), float(H[1, 1])
    if not h00 > 0.0:
        return None
    l10 = h01 / math.sqrt(h00)
    s = h11 - l10 * l10
    if not s > 0.0:
        return None
    l00, l11 = math.sqrt(h00), math.sqrt(s)
    z0 = g[0] / l00
    z1 = (g[1] - l10 * z0) / l11
    x1 = z1 / l11
    x0 = (z0 - l10 * x1) / l00
    return np.array([-x0, -x1]), z0 * z0 + z1 * z1


def cllr(pos, neg, a=1.0, b=0.0):
    rec = pass_record(pos, neg, a, b)
    check(rec)
    return objective(rec, 0.5) / LN2


def bayes_theta(prior, c_miss=1.0, c_fa=1.0, a=1.0, b=0.0):
    """The raw-score threshold at which a * s + b crosses the Bayes threshold (a > 0)."""
    return (math.log(c_fa * (1.0 - prior) / (c_miss * prior)) - b) / a


def act_dcf(pos, neg, prior, c_miss=1.0, c_fa=1.0, a=1.0, b=0.0):
    pos, neg = np.asarray(pos, np.float32).astype(np.float64), np.asarray(neg, np.float32).astype(np.float64)
    theta = bayes_theta(prior, c_miss, c_fa, a, b)
    miss, fa = int((pos < theta).sum()), int((neg >= theta).sum())
    return (c_miss * prior * miss / pos.shape[0] + c_fa * (1.0 - prior) * fa / neg.shape[0]) / min(c_miss * prior, c_fa * (1.0 - prior))


def fit(pos, neg, prior=0.5, tol=1e-18, max_iter=100, take_pass=None, trace=None):
    """The damped Newton iteration of the header.  Returns a dict with the fields of the fit record."""
    if not 0.0 < prior < 1.0:
        raise ValueError("prior outside (0, 1)")
    take = take_pass or (lambda a, c: pass_record(pos, neg, a, c))
    tau = logit(prior)
    passes = 1
    before = take(1.0, 0.0)
    check(before)
    if min(before["min_t"], before["min_n"]) == max(before["max_t"], before["max_n"]):
        raise ValueError("all scores are equal")
    a = b = 0.0
    rec = take(a, b + tau)
    passes += 1
    it, lam2, converged = 0, float("inf"), False
    while True:
        F, g, H = objective(rec, prior), gradient(rec, prior), hessian(rec, prior)
        sol = solve2(H, g)
        if sol is None:
            raise ValueError("the Hessian is not positive definite")
        d, lam2 = sol
        if trace is not None:
            trace.append((it, a, b, F, lam2))
        if lam2 <= tol:
            converged = True
            break
        if it >= max_iter:
            break
        t, accepted = 1.0, False
        for _ in range(31):
            na, nb = a + t * d[0], b + t * d[1]
            trial = take(na, nb + tau)
            passes += 1
            if objective(trial, prior) <= F - 1e-4 * t * lam2 + 2.0 ** -44 * abs(F):     # (the rounding of F itself)
                accepted = True
                break
            t *= 0.5
        if not accepted:
            break
        a, b, rec = na, nb, trial
        it += 1
    if prior == 0.5:
        after = rec
    else:
        after = take(a, b)
        passes += 1
    return {"a": a, "b": b, "objective": objective(rec, prior) / LN2, "cllr_before": objective(before, 0.5) / LN2,
            "cllr_after": objective(after, 0.5) / LN2, "lambda2": lam2, "iterations": it, "passes": passes,
            "converged": converged, "separable": bool(before["min_t"] > before["max_n"])}


def apply_map(s32, a, b):
    """(float)fma(a, (double)s, b): the exact a * s + b rounded once to fp64, then once to fp32 (np.longdouble carries
    the 53 x 24-bit product exactly on x86; where its 64-bit sum rounds, tests decide with fractions.Fraction)."""
    s = np.asarray(s32, np.float32).astype(np.longdouble)
    return (np.longdouble(a) * s + np.longdouble(b)).astype(np.float64).astype(np.float32)


def equivariant(a, b, a2, b2, k, d):
    """Is (a2, b2) the fit of the scores k * s + d, given the fit (a, b) of s?  The map undoes the scale and the shift: a2 = a / k
    to 1e-5 relative, b2 = b - a d / k to 1e-5 absolute (the one statement of the equivariance rule: the device test asserts it,
    the sweep's generator filters its draws by it)."""
    return abs(a2 - a / k) <= max(1e-5 * abs(a / k), 1e-12) and abs(b2 - (b - a * d / k)) <= 1e-5
