"""plda_amd/identify.py -- rank-N identification figures from the ids that `MPlda.top_n` returns.  Pure NumPy.

  rank_rates(ids, truth, ranks)   the fraction of lines whose true id is among the first r of the line, for every r
  cmc(ids, truth)                 the whole cumulative match characteristic: the rank-r rate for r = 1 ... n
  affine_f32(a, scores, b)        (float)fma(a, (double)score, b) on the host: the stored calibration applied to the n scores
"""
from fractions import Fraction

import numpy as np


def _first_hit(ids, truth):
    """Per line the position of the first entry equal to the line's true id, n where there is none."""
    ids = np.asarray(ids)
    if ids.ndim != 2:
        raise ValueError("ids must be [lines, n], got %s" % (tuple(ids.shape),))
    truth = np.asarray(truth).reshape(-1)
    if truth.shape[0] != ids.shape[0]:
        raise ValueError("truth must name the true id of each of the %d lines, got %d" % (ids.shape[0], truth.shape[0]))
    hit = ids == truth[:, None]
    return np.where(hit.any(axis=1), hit.argmax(axis=1), ids.shape[1])


def cmc(ids, truth):
    """float64 [n]: element r - 1 is the fraction of lines whose true id is among the first r ids of the line."""
    ids = np.asarray(ids)
    first = _first_hit(ids, truth)
    if ids.shape[0] == 0:
        raise ValueError("cmc: no lines")
    found = np.bincount(first, minlength=ids.shape[1] + 1)[:ids.shape[1]]
    return np.cumsum(found) / float(ids.shape[0])


def rank_rates(ids, truth, ranks=(1, 5, 10)):
    """{r: rank-r identification rate} for the ranks asked for; every r must be in 1 ... n."""
    curve = cmc(ids, truth)
    for r in ranks:
        if not 1 <= int(r) <= curve.shape[0]:
            raise ValueError("rank %r is outside 1 ... n = %d" % (r, curve.shape[0]))
    return {int(r): float(curve[int(r) - 1]) for r in ranks}


def affine_f32(a, scores, b):
    """float32 array: (float)fma(a, (double)s, b) for every fp32 score s -- what the device's affine map computes.  NumPy has
    no fused multiply-add.  r = a * s + b in fp64 errs by at most half an ulp of the product and half an ulp of r, and the
    fused value lies within that of r too; where both ends of that interval round to the same fp32 (rounding is monotone)
    so does the fused value.  The few other elements are evaluated exactly, in rationals."""
    a, b = float(a), float(b)
    s = np.ascontiguousarray(scores, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * s.astype(np.float64)
        r = p + b
        out = r.astype(np.float32)
        err = (np.abs(p) + np.abs(r)) * 2.0 ** -52
        risky = np.isfinite(r) & ((r - err).astype(np.float32).view(np.uint32) != (r + err).astype(np.float32).view(np.uint32))
    flat_out, flat_s = out.reshape(-1), s.reshape(-1)
    for i in np.flatnonzero(risky.reshape(-1)):
        exact = Fraction(a) * Fraction(float(flat_s[i])) + Fraction(b)
        with np.errstate(over="ignore"):
            flat_out[i] = np.float32(float(exact))       # one rounding to fp64 (as the fma), one to fp32
    return out
