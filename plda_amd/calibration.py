"""plda_amd/calibration.py -- linear score calibration, Cllr and actual DCF on the GPU (csrc/calib.hip; the definitions are
in include/plda_hip.h, "linear score calibration").  Thin ctypes glue in the manner of plda_amd/eer.py: a calibration PASS
returns one record (dict) of fp64 sums and exact counts, a FIT returns a `Calibration`."""
import ctypes as C
import math
import warnings

import numpy as np

from . import _native as N

LN2 = math.log(2.0)
SUMS = ("L", "G0", "G1", "H0", "H1", "H2")

# struct plda_calib_record / plda_calib_fit of include/plda_hip.h
RECORD_DTYPE = np.dtype([("sum", np.float64, (2, 6)), ("np", np.uint64), ("nn", np.uint64), ("miss", np.uint64), ("fa", np.uint64),
                         ("nonfinite", np.uint64), ("min_t", np.float32), ("max_t", np.float32), ("min_n", np.float32),
                         ("max_n", np.float32)], align=True)
FIT_DTYPE = np.dtype([("a", np.float64), ("b", np.float64), ("objective", np.float64), ("cllr_before", np.float64),
                      ("cllr_after", np.float64), ("lambda2", np.float64), ("iterations", np.int32), ("passes", np.int32),
                      ("converged", np.int32), ("separable", np.int32)], align=True)
assert RECORD_DTYPE.itemsize == 152 and FIT_DTYPE.itemsize == 64


def _p(x):
    return C.c_void_p(int(x)) if x else None


def _record(raw):
    """The flat record as a dict: Np, Nn, miss, fa, nonfinite (int), min_t .. max_n (np.float32) and the twelve sums
    L_t .. H2_t, L_n .. H2_n (float)."""
    r = raw[0]
    out = {"Np": int(r["np"]), "Nn": int(r["nn"]), "miss": int(r["miss"]), "fa": int(r["fa"]), "nonfinite": int(r["nonfinite"]),
           "min_t": r["min_t"], "max_t": r["max_t"], "min_n": r["min_n"], "max_n": r["max_n"]}
    for k, cls in ((1, "t"), (0, "n")):
        for j, name in enumerate(SUMS):
            out[name + "_" + cls] = float(r["sum"][k][j])
    return out


class Calibration(object):
    """The affine map llr = a * s + b of a fit, with what the fit reported.  Calling it maps HOST scores (fp64 in, fp64
    out; the device map, rounded once to fp32, is `apply_dev`)."""

    def __init__(self, a, b, prior=0.5, cllr_before=float("nan"), cllr_after=float("nan"), converged=True, separable=False,
                 objective=float("nan"), lambda2=float("nan"), iterations=0, passes=0):
        self.a, self.b, self.prior = float(a), float(b), float(prior)
        self.cllr_before, self.cllr_after = float(cllr_before), float(cllr_after)
        self.converged, self.separable = bool(converged), bool(separable)
        self.objective, self.lambda2 = float(objective), float(lambda2)
        self.iterations, self.passes = int(iterations), int(passes)

    def __call__(self, scores):
        return self.a * np.asarray(scores, np.float64) + self.b

    def __repr__(self):
        return "Calibration(a=%r, b=%r, prior=%r, cllr_before=%r, cllr_after=%r, converged=%r, separable=%r)" % (
            self.a, self.b, self.prior, self.cllr_before, self.cllr_after, self.converged, self.separable)


def _calibration(raw, prior):
    f = raw[0]
    cal = Calibration(f["a"], f["b"], prior, f["cllr_before"], f["cllr_after"], f["converged"] != 0, f["separable"] != 0,
                      f["objective"], f["lambda2"], f["iterations"], f["passes"])
    if cal.separable:
        warnings.warn("calibration: the two classes are separable (min target > max non-target): the optimum is at infinity, "
                      "a = %g is where the iteration stopped" % cal.a, RuntimeWarning, stacklevel=3)
    elif not cal.converged:
        warnings.warn("calibration: the Newton iteration did not converge (lambda2 = %g after %d iterations)"
                      % (cal.lambda2, cal.iterations), RuntimeWarning, stacklevel=3)
    return cal


# ---------------------------------------------------------------------------------------------- passes
def pass_from_lists(engine, truescores, impostscores, a=1.0, c=0.0, theta=0.0):
    pos = np.ascontiguousarray(truescores, np.float32)
    neg = np.ascontiguousarray(impostscores, np.float32)
    raw = np.zeros(1, RECORD_DTYPE)
    N.check(engine._h, engine._lib.plda_calib_pass_lists(engine._h, C.c_void_p(pos.ctypes.data), pos.shape[0], C.c_void_p(neg.ctypes.data),
                                                         neg.shape[0], float(a), float(c), float(theta), C.c_void_p(raw.ctypes.data)))
    return _record(raw)


def pass_from_matrix_dev(engine, dscores, ld, m, nt, denrol_spk, dtest_spk, a=1.0, c=0.0, theta=0.0):
    """One pass over an HBM-resident fp32 trials matrix; trial (i, j) is a target iff enrol_spk[i] == test_spk[j] (int64
    device arrays)."""
    raw = np.zeros(1, RECORD_DTYPE)
    N.check(engine._h, engine._lib.plda_calib_pass_matrix_dev(engine._h, _p(dscores), int(ld), int(m), int(nt), _p(denrol_spk),
                                                              _p(dtest_spk), float(a), float(c), float(theta),
                                                              C.c_void_p(raw.ctypes.data)))
    return _record(raw)


def pass_from_operands_dev(engine, dU, dn, n_uniform, m, dV, nt, denrol_spk, dtest_spk, dzmean=None, dzstd=None, a=1.0, c=0.0,
                           theta=0.0):
    """One pass over the m x nt trials between HBM-resident transformed vectors without the matrix (arguments as
    `eer.eer_from_operands_dev`); the slabs are scored once per pass."""
    raw = np.zeros(1, RECORD_DTYPE)
    N.check(engine._h, engine._lib.plda_score_calib_pass_dev(engine._h, _p(dU), _p(dn), int(n_uniform), int(m), _p(dV), int(nt),
                                                             _p(dzmean), _p(dzstd), _p(denrol_spk), _p(dtest_spk), float(a),
                                                             float(c), float(theta), C.c_void_p(raw.ctypes.data)))
    return _record(raw)


# ---------------------------------------------------------------------------------------------- fits
def fit_from_lists(engine, truescores, impostscores, prior=0.5, tol=0.0, max_iter=0):
    """Prior-weighted logistic regression of llr = a * s + b on target / non-target score arrays.  tol = 0 / max_iter = 0:
    the library's defaults (1e-18, 100)."""
    pos = np.ascontiguousarray(truescores, np.float32)
    neg = np.ascontiguousarray(impostscores, np.float32)
    raw = np.zeros(1, FIT_DTYPE)
    N.check(engine._h, engine._lib.plda_calib_fit_lists(engine._h, C.c_void_p(pos.ctypes.data), pos.shape[0], C.c_void_p(neg.ctypes.data),
                                                        neg.shape[0], float(prior), float(tol), int(max_iter), C.c_void_p(raw.ctypes.data)))
    return _calibration(raw, prior)


def fit_from_matrix_dev(engine, dscores, ld, m, nt, denrol_spk, dtest_spk, prior=0.5, tol=0.0, max_iter=0):
    raw = np.zeros(1, FIT_DTYPE)
    N.check(engine._h, engine._lib.plda_calib_fit_matrix_dev(engine._h, _p(dscores), int(ld), int(m), int(nt), _p(denrol_spk),
                                                             _p(dtest_spk), float(prior), float(tol), int(max_iter),
                                                             C.c_void_p(raw.ctypes.data)))
    return _calibration(raw, prior)


def fit_from_operands_dev(engine, dU, dn, n_uniform, m, dV, nt, denrol_spk, dtest_spk, dzmean=None, dzstd=None, prior=0.5, tol=0.0,
                          max_iter=0):
    raw = np.zeros(1, FIT_DTYPE)
    N.check(engine._h, engine._lib.plda_score_calib_fit_dev(engine._h, _p(dU), _p(dn), int(n_uniform), int(m), _p(dV), int(nt),
                                                            _p(dzmean), _p(dzstd), _p(denrol_spk), _p(dtest_spk), float(prior),
                                                            float(tol), int(max_iter), C.c_void_p(raw.ctypes.data)))
    return _calibration(raw, prior)


# ---------------------------------------------------------------------------------------------- figures from a record
def objective(record, prior):
    """F(a, b; prior) in nats of a record taken at c = b + logit(prior)."""
    return prior / record["Np"] * record["L_t"] + (1.0 - prior) / record["Nn"] * record["L_n"]


def cllr(record):
    """Cllr (bits) of a record taken at (a, c) = (a, b): F(a, b; 0.5) / ln 2.  `pass_from_*(..., a=1, c=0)` gives the Cllr of
    the scores as they are."""
    return objective(record, 0.5) / LN2


def bayes_theta(prior, c_miss=1.0, c_fa=1.0, calibration=None):
    """The raw-score threshold at which the (calibrated) score crosses the Bayes threshold log(Cfa (1-pi) / (Cmiss pi))."""
    a, b = (calibration.a, calibration.b) if calibration is not None else (1.0, 0.0)
    if not a > 0.0:
        raise ValueError("act_dcf needs a calibration with a > 0 (got a = %r)" % a)
    if not 0.0 < prior < 1.0:
        raise ValueError("prior must lie inside (0, 1)")
    return (math.log(c_fa * (1.0 - prior) / (c_miss * prior)) - b) / a


def act_dcf(record_or_pass, prior, c_miss=1.0, c_fa=1.0, calibration=None):
    """The actual (normalised) detection cost at the Bayes threshold of (prior, c_miss, c_fa).  `record_or_pass` is either a
    callable theta -> record (e.g. `lambda th: pass_from_matrix_dev(eng, ..., theta=th)`), which is called with the
    raw-score threshold that `calibration` (None: the scores are LLRs already) implies, or a record already taken at
    `bayes_theta(prior, c_miss, c_fa, calibration)`."""
    theta = bayes_theta(prior, c_miss, c_fa, calibration)
    rec = record_or_pass(theta) if callable(record_or_pass) else record_or_pass
    return ((c_miss * prior * rec["miss"] / rec["Np"] + c_fa * (1.0 - prior) * rec["fa"] / rec["Nn"])
            / min(c_miss * prior, c_fa * (1.0 - prior)))


def apply_dev(engine, dscores, ld, m, nt, calibration, dout=None, ld_out=None):
    """out[i, j] = (float)fma(a, (double)s[i, j], b) on an HBM-resident fp32 matrix; in place when dout is None.  Enqueued
    on the engine's stream (no synchronisation)."""
    N.check(engine._h, engine._lib.plda_affine_map_dev(engine._h, _p(dscores), int(ld), int(m), int(nt), float(calibration.a),
                                                       float(calibration.b), _p(dout if dout is not None else dscores),
                                                       int(ld if ld_out is None else ld_out)))
