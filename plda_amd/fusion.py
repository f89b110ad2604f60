"""plda_amd/fusion.py -- linear fusion of K systems' scores by prior-weighted logistic regression on the GPU
(csrc/fusion.hip; the definitions are in include/plda_hip.h, "multi-system score fusion").  Thin ctypes glue in the manner
of plda_amd/calibration.py: a fusion PASS returns one record (dict) of fp64 sums and exact counts, a FIT returns a `Fusion`."""
import ctypes as C
import math
import warnings

import numpy as np

from . import _native as N

LN2 = math.log(2.0)
MAX_SYSTEMS = 8

# struct plda_fusion_sums / plda_fusion_record / plda_fusion_fit of include/plda_hip.h
SUMS_DTYPE = np.dtype([("L", np.float64), ("G", np.float64, (MAX_SYSTEMS + 1,)),
                       ("H", np.float64, ((MAX_SYSTEMS + 1) * (MAX_SYSTEMS + 2) // 2,))], align=True)
RECORD_DTYPE = np.dtype([("sum", SUMS_DTYPE, (2,)), ("ymin", np.float64, (2,)), ("ymax", np.float64, (2,)), ("np", np.uint64),
                         ("nn", np.uint64), ("miss", np.uint64), ("fa", np.uint64), ("nonfinite", np.uint64),
                         ("smin", np.float32, (MAX_SYSTEMS,)), ("smax", np.float32, (MAX_SYSTEMS,)), ("n_systems", np.int32),
                         ("reserved", np.int32)], align=True)
FIT_DTYPE = np.dtype([("a", np.float64, (MAX_SYSTEMS,)), ("b", np.float64), ("objective", np.float64), ("cllr_after", np.float64),
                      ("lambda2", np.float64), ("iterations", np.int32), ("passes", np.int32), ("converged", np.int32),
                      ("separable", np.int32)], align=True)
assert SUMS_DTYPE.itemsize == 440 and RECORD_DTYPE.itemsize == 1024 and FIT_DTYPE.itemsize == 112


def _p(x):
    return C.c_void_p(int(x)) if x else None


def n_g(k):
    return k + 1


def n_h(k):
    return (k + 1) * (k + 2) // 2


def _record(raw):
    """The flat record as a dict: K, Np, Nn, miss, fa, nonfinite (int); smin, smax (np.float32 [K]); ymin_t .. ymax_n, L_t, L_n
    (float); G_t, G_n (float64 [K + 1]) and H_t, H_n (float64 [(K + 1)(K + 2) / 2], t(i, j) = j (j + 1) / 2 + i)."""
    r = raw[0]
    k = int(r["n_systems"])
    out = {"K": k, "Np": int(r["np"]), "Nn": int(r["nn"]), "miss": int(r["miss"]), "fa": int(r["fa"]),
           "nonfinite": int(r["nonfinite"]), "smin": r["smin"][:k].copy(), "smax": r["smax"][:k].copy()}
    for c, cls in ((1, "t"), (0, "n")):
        out["ymin_" + cls], out["ymax_" + cls] = float(r["ymin"][c]), float(r["ymax"][c])
        out["L_" + cls] = float(r["sum"][c]["L"])
        out["G_" + cls] = r["sum"][c]["G"][:n_g(k)].copy()
        out["H_" + cls] = r["sum"][c]["H"][:n_h(k)].copy()
    return out


def record_to_raw(rec):
    """The dict form back into one plda_fusion_record (entries beyond K zero): what plda_fusion_newton takes."""
    raw = np.zeros(1, RECORD_DTYPE)
    r, k = raw[0], int(rec["K"])
    r["n_systems"], r["np"], r["nn"], r["miss"], r["fa"], r["nonfinite"] = k, rec["Np"], rec["Nn"], rec["miss"], rec["fa"], rec["nonfinite"]
    r["smin"][:k], r["smax"][:k] = rec["smin"], rec["smax"]
    for c, cls in ((1, "t"), (0, "n")):
        r["ymin"][c], r["ymax"][c] = rec["ymin_" + cls], rec["ymax_" + cls]
        r["sum"][c]["L"] = rec["L_" + cls]
        r["sum"][c]["G"][:n_g(k)] = rec["G_" + cls]
        r["sum"][c]["H"][:n_h(k)] = rec["H_" + cls]
    return raw


class Fusion(object):
    """The linear fusion llr = b + sum_k a[k] * s_k of a fit, with what the fit reported.  Calling it maps HOST scores (a
    sequence of K arrays; fp64 in, fp64 out; the device map, the FMA chain rounded once to fp32, is `apply_dev`)."""

    def __init__(self, a, b, prior=0.5, cllr_after=float("nan"), converged=True, separable=False, objective=float("nan"),
                 lambda2=float("nan"), iterations=0, passes=0):
        self.a = np.array(a, np.float64).reshape(-1)
        if not 1 <= self.a.shape[0] <= MAX_SYSTEMS:
            raise ValueError("a fusion has 1 .. %d systems" % MAX_SYSTEMS)
        self.b, self.prior = float(b), float(prior)
        self.cllr_after = float(cllr_after)
        self.converged, self.separable = bool(converged), bool(separable)
        self.objective, self.lambda2 = float(objective), float(lambda2)
        self.iterations, self.passes = int(iterations), int(passes)

    @property
    def n_systems(self):
        return int(self.a.shape[0])

    def __call__(self, scores):
        if len(scores) != self.n_systems:
            raise ValueError("this fusion takes the scores of %d systems" % self.n_systems)
        y = np.full(np.shape(scores[0]), self.b, np.float64)
        for ak, s in zip(self.a, scores):
            y = y + ak * np.asarray(s, np.float64)
        return y

    def __repr__(self):
        return "Fusion(a=%r, b=%r, prior=%r, cllr_after=%r, converged=%r, separable=%r)" % (
            self.a.tolist(), self.b, self.prior, self.cllr_after, self.converged, self.separable)


def _fusion(raw, k, prior):
    f = raw[0]
    fus = Fusion(f["a"][:k], f["b"], prior, f["cllr_after"], f["converged"] != 0, f["separable"] != 0, f["objective"], f["lambda2"],
                 f["iterations"], f["passes"])
    if fus.separable:
        warnings.warn("fusion: the two classes are separable by the fused value (min target > max non-target): the optimum is "
                      "at infinity, a = %s is where the iteration stopped" % fus.a.tolist(), RuntimeWarning, stacklevel=3)
    elif not fus.converged:
        warnings.warn("fusion: the Newton iteration did not converge (lambda2 = %g after %d iterations)"
                      % (fus.lambda2, fus.iterations), RuntimeWarning, stacklevel=3)
    return fus


def _matrix_args(dscores, ld):
    """(K, host array of K device pointers, host array of K pitches); the arrays must outlive the call."""
    ptrs = np.array([int(p) if p else 0 for p in dscores], np.uint64)
    lds = np.array([int(x) for x in ld], np.int64)
    if ptrs.shape[0] != lds.shape[0]:
        raise ValueError("one pitch per system")
    return int(ptrs.shape[0]), ptrs, lds


def _list_args(lists):
    arrs = [np.ascontiguousarray(x, np.float32).reshape(-1) for x in lists]
    if len({a.shape[0] for a in arrs}) > 1:
        raise ValueError("the K lists of one class are parallel: element t of every list is the same trial")
    return arrs, np.array([a.ctypes.data for a in arrs], np.uint64)


def _weights(a, k):
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    if a.shape[0] != k:
        raise ValueError("one weight per system (%d weights for %d systems)" % (a.shape[0], k))
    return a


def _vp(arr):
    return C.c_void_p(arr.ctypes.data)


# ---------------------------------------------------------------------------------------------- passes
def pass_from_matrices_dev(engine, dscores, ld, m, nt, denrol_spk, dtest_spk, a, c=0.0, theta=0.0):
    """One pass over K HBM-resident fp32 trials matrices (dscores: K device pointers, ld: K pitches); trial (i, j) is a
    target iff enrol_spk[i] == test_spk[j] (int64 device arrays)."""
    k, ptrs, lds = _matrix_args(dscores, ld)
    a = _weights(a, k)
    raw = np.zeros(1, RECORD_DTYPE)
    N.check(engine._h, engine._lib.plda_fusion_pass_matrices_dev(engine._h, k, _vp(ptrs), _vp(lds), int(m), int(nt), _p(denrol_spk),
                                                                 _p(dtest_spk), _vp(a), float(c), float(theta), _vp(raw)))
    return _record(raw)


def pass_from_lists(engine, truescores, impostscores, a, c=0.0, theta=0.0):
    """One pass over K parallel target arrays and K parallel non-target arrays on the host."""
    pos, pp = _list_args(truescores)
    neg, pn = _list_args(impostscores)
    if len(pos) != len(neg):
        raise ValueError("as many target lists as non-target lists")
    k = len(pos)
    a = _weights(a, k)
    raw = np.zeros(1, RECORD_DTYPE)
    N.check(engine._h, engine._lib.plda_fusion_pass_lists(engine._h, k, _vp(pp), pos[0].shape[0] if k else 0, _vp(pn),
                                                          neg[0].shape[0] if k else 0, _vp(a), float(c), float(theta), _vp(raw)))
    return _record(raw)


# ---------------------------------------------------------------------------------------------- fits
def fit_from_matrices_dev(engine, dscores, ld, m, nt, denrol_spk, dtest_spk, prior=0.5, tol=0.0, max_iter=0):
    """Prior-weighted logistic regression of llr = b + sum a_k s_k on K labelled HBM-resident matrices.  tol = 0 /
    max_iter = 0: the library's defaults (1e-18, 100)."""
    k, ptrs, lds = _matrix_args(dscores, ld)
    raw = np.zeros(1, FIT_DTYPE)
    N.check(engine._h, engine._lib.plda_fusion_fit_matrices_dev(engine._h, k, _vp(ptrs), _vp(lds), int(m), int(nt), _p(denrol_spk),
                                                                _p(dtest_spk), float(prior), float(tol), int(max_iter), _vp(raw)))
    return _fusion(raw, k, prior)


def fit_from_lists(engine, truescores, impostscores, prior=0.5, tol=0.0, max_iter=0):
    pos, pp = _list_args(truescores)
    neg, pn = _list_args(impostscores)
    if len(pos) != len(neg):
        raise ValueError("as many target lists as non-target lists")
    k = len(pos)
    raw = np.zeros(1, FIT_DTYPE)
    N.check(engine._h, engine._lib.plda_fusion_fit_lists(engine._h, k, _vp(pp), pos[0].shape[0] if k else 0, _vp(pn),
                                                         neg[0].shape[0] if k else 0, float(prior), float(tol), int(max_iter), _vp(raw)))
    return _fusion(raw, k, prior)


def newton(record, prior):
    """The Newton step of the fit as the library's pure function (no handle, no GPU): (F in nats, d[K + 1] in the order
    (b, a_0 ..), lambda2) from a record taken at c = b + logit(prior)."""
    lib = N.load()
    raw = record_to_raw(record)
    F, lam2, d = C.c_double(), C.c_double(), np.zeros(MAX_SYSTEMS + 1)
    N.check(None, lib.plda_fusion_newton(_vp(raw), float(prior), C.byref(F), _vp(d), C.byref(lam2)))
    return F.value, d[:int(record["K"]) + 1].copy(), lam2.value


# ---------------------------------------------------------------------------------------------- figures from a record
def objective(record, prior):
    """F(x; prior) in nats of a record taken at c = b + logit(prior)."""
    return prior / record["Np"] * record["L_t"] + (1.0 - prior) / record["Nn"] * record["L_n"]


def cllr(record):
    """Cllr (bits) of a record taken at (a, c) = (a, b): F(x; 0.5) / ln 2."""
    return objective(record, 0.5) / LN2


def bayes_theta(prior, c_miss=1.0, c_fa=1.0):
    """The Bayes threshold log(Cfa (1-pi) / (Cmiss pi)) on the fused value (a pass compares the chain value with theta)."""
    if not 0.0 < prior < 1.0:
        raise ValueError("prior must lie inside (0, 1)")
    return math.log(c_fa * (1.0 - prior) / (c_miss * prior))


def act_dcf(record_or_pass, prior, c_miss=1.0, c_fa=1.0):
    """The actual (normalised) detection cost of the fused value at the Bayes threshold of (prior, c_miss, c_fa).
    `record_or_pass` is a callable theta -> record (e.g. `lambda th: pass_from_matrices_dev(eng, ..., a=f.a, c=f.b, theta=th)`)
    or a record already taken at `bayes_theta(prior, c_miss, c_fa)` with (a, c) = (fusion.a, fusion.b)."""
    theta = bayes_theta(prior, c_miss, c_fa)
    rec = record_or_pass(theta) if callable(record_or_pass) else record_or_pass
    return ((c_miss * prior * rec["miss"] / rec["Np"] + c_fa * (1.0 - prior) * rec["fa"] / rec["Nn"])
            / min(c_miss * prior, c_fa * (1.0 - prior)))


def apply_dev(engine, dscores, ld, m, nt, fusion, dout, ld_out):
    """out[i, j] = (float)(the FMA chain from b over the K systems) on HBM-resident fp32 matrices; dout may be one of the
    inputs with ld_out equal to its pitch (in place).  Enqueued on the engine's stream (no synchronisation)."""
    k, ptrs, lds = _matrix_args(dscores, ld)
    a = _weights(fusion.a, k)
    N.check(engine._h, engine._lib.plda_fusion_map_dev(engine._h, k, _vp(ptrs), _vp(lds), int(m), int(nt), _vp(a), float(fusion.b),
                                                       _p(dout), int(ld_out)))


# ---------------------------------------------------------------------------------------------- sides (K25, csrc/fusion.hip)
SIDE_OPS = ("min", "max", "sum", "absdiff", "prod")          # PLDA_SIDE_MIN .. PLDA_SIDE_PROD of include/plda_hip.h
SIDE_DTYPE = np.dtype([("enrol", np.uint64), ("test", np.uint64), ("op", np.int32), ("reserved", np.int32)], align=True)
assert SIDE_DTYPE.itemsize == 24


def _side_op(op):
    if isinstance(op, str):
        if op not in SIDE_OPS:
            raise ValueError("unknown side op %r: one of %s" % (op, ", ".join(SIDE_OPS)))
        return SIDE_OPS.index(op)
    if isinstance(op, (int, np.integer)) and 0 <= int(op) < len(SIDE_OPS):
        return int(op)
    raise ValueError("unknown side op %r: one of %s" % (op, ", ".join(SIDE_OPS)))


def side_values(op, e, t):
    """The value of a side as include/plda_hip.h defines it, in NumPy: ONE fp32 operation on e and t (broadcast against each
    other: e[:, None] and t[None, :] give the [M, Nt] matrix of a side, two equally long arrays the values of listed
    trials).  Ties and signed zeros follow the written comparison: min is `e < t ? e : t`, max is `e > t ? e : t`."""
    code = _side_op(op)
    e, t = np.asarray(e, np.float32), np.asarray(t, np.float32)
    with np.errstate(all="ignore"):
        if code == 0:
            return np.where(e < t, e, t).astype(np.float32)
        if code == 1:
            return np.where(e > t, e, t).astype(np.float32)
        if code == 2:
            return np.add(e, t, dtype=np.float32)
        if code == 3:
            return np.abs(np.subtract(e, t, dtype=np.float32))
        return np.multiply(e, t, dtype=np.float32)


class Side(object):
    """One side-information term of a quality-aware calibration: `op` ("min" | "max" | "sum" | "absdiff" | "prod") on a
    per-enrol-row and a per-test-column quality.  `enrol` / `test` are 1-D float32 torch tensors on the device, or host
    sequences (uploaded by `on(device)`); their lengths are checked against (M, Nt) before any device call."""

    def __init__(self, op, enrol, test):
        self.code = _side_op(op)
        self.op = SIDE_OPS[self.code]
        self.enrol, self.test = enrol, test
        for name, v in (("enrol", enrol), ("test", test)):
            if v is None or len(np.shape(v)) != 1:
                raise ValueError("side %r: the %s values are a 1-D sequence (one per %s row)" % (self.op, name, name))

    def check(self, m, nt):
        if len(self.enrol) != int(m) or len(self.test) != int(nt):
            raise ValueError("side %r: %d enrol and %d test values for a %d x %d trials matrix"
                             % (self.op, len(self.enrol), len(self.test), int(m), int(nt)))

    def on(self, device):
        """The side with both vectors as contiguous float32 device tensors (itself if they already are)."""
        import torch

        def up(v):
            if isinstance(v, torch.Tensor):
                if v.dtype != torch.float32:
                    raise ValueError("side %r: device vectors are float32" % self.op)
                return v.to(device).contiguous()
            return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(device)
        return Side(self.code, up(self.enrol), up(self.test))

    def __repr__(self):
        return "Side(%r, enrol[%d], test[%d])" % (self.op, len(self.enrol), len(self.test))


def _side_args(sides, m, nt):
    """(Q, the host array of Q plda_fusion_side, the device tensors it points into -- keep them alive over the call)."""
    sides = list(sides)
    for s in sides:
        if not isinstance(s, Side):
            raise ValueError("a side is a plda_amd.fusion.Side")
        s.check(m, nt)
    raw = np.zeros(max(len(sides), 1), SIDE_DTYPE)
    keep = []
    for q, s in enumerate(sides):
        if not (hasattr(s.enrol, "data_ptr") and hasattr(s.test, "data_ptr")):
            raise ValueError("side %d: the vectors must be on the device (Side.on(device))" % q)
        if str(s.enrol.dtype) != "torch.float32" or str(s.test.dtype) != "torch.float32" or not s.enrol.is_contiguous() or not s.test.is_contiguous():
            raise ValueError("side %d: the device vectors are contiguous float32" % q)
        raw[q]["enrol"], raw[q]["test"], raw[q]["op"] = s.enrol.data_ptr(), s.test.data_ptr(), s.code
        keep.append((s.enrol, s.test))
    return len(sides), raw, keep


class QualityFusion(Fusion):
    """A fusion over K systems and Q sides: a = (a of the systems, then a of the sides).  Calling it maps HOST values in
    fp64: `scores` a sequence of K arrays, `qualities` a sequence of Q (enrol_values, test_values) pairs broadcast against
    the scores' shape ([M] and [Nt] for [M, Nt] scores; equally long arrays for listed trials)."""

    def __init__(self, a, b, ops, **kw):
        Fusion.__init__(self, a, b, **kw)
        self.ops = tuple(SIDE_OPS[_side_op(o)] for o in ops)
        if self.n_sides >= self.a.shape[0]:
            raise ValueError("a quality fusion has at least one system beside its %d sides" % self.n_sides)

    @property
    def n_sides(self):
        return len(self.ops)

    @property
    def n_systems(self):
        return int(self.a.shape[0]) - self.n_sides

    def __call__(self, scores, qualities=()):
        if len(scores) != self.n_systems or len(qualities) != self.n_sides:
            raise ValueError("this fusion takes the scores of %d systems and %d qualities" % (self.n_systems, self.n_sides))
        shape = np.shape(scores[0])
        feats = [np.asarray(s, np.float64) for s in scores]
        for op, (e, t) in zip(self.ops, qualities):
            e, t = np.asarray(e, np.float32), np.asarray(t, np.float32)
            if len(shape) == 2 and e.ndim == 1 and t.ndim == 1:
                e, t = e[:, None], t[None, :]
            feats.append(side_values(op, e, t).astype(np.float64))
        y = np.full(shape, self.b, np.float64)
        for ak, f in zip(self.a, feats):
            y = y + ak * f
        return y

    def __repr__(self):
        return "QualityFusion(a=%r, b=%r, ops=%r, prior=%r, cllr_after=%r, converged=%r, separable=%r)" % (
            self.a.tolist(), self.b, self.ops, self.prior, self.cllr_after, self.converged, self.separable)


def _quality_fusion(raw, k, sides, prior):
    f = _fusion(raw, k + len(sides), prior)
    return QualityFusion(f.a, f.b, [s.code for s in sides], prior=f.prior, cllr_after=f.cllr_after, converged=f.converged,
                         separable=f.separable, objective=f.objective, lambda2=f.lambda2, iterations=f.iterations, passes=f.passes)


def pass_with_sides_dev(engine, dscores, ld, sides, m, nt, denrol_spk, dtest_spk, a, c=0.0, theta=0.0):
    """One pass over K HBM-resident matrices and Q sides (`Side`s with device vectors); a has K + Q weights.  Bit-identical
    to `pass_from_matrices_dev` over K + Q matrices with the sides materialised by `side_values`."""
    k, ptrs, lds = _matrix_args(dscores, ld)
    q, sraw, keep = _side_args(sides, m, nt)
    a = _weights(a, k + q)
    raw = np.zeros(1, RECORD_DTYPE)
    N.check(engine._h, engine._lib.plda_fusion_side_pass_dev(engine._h, k, _vp(ptrs), _vp(lds), q, _vp(sraw), int(m), int(nt),
                                                             _p(denrol_spk), _p(dtest_spk), _vp(a), float(c), float(theta), _vp(raw)))
    del keep
    return _record(raw)


def fit_with_sides_dev(engine, dscores, ld, sides, m, nt, denrol_spk, dtest_spk, prior=0.5, tol=0.0, max_iter=0):
    """The fusion fit over K matrices and Q sides -> `QualityFusion`."""
    k, ptrs, lds = _matrix_args(dscores, ld)
    sides = list(sides)
    q, sraw, keep = _side_args(sides, m, nt)
    raw = np.zeros(1, FIT_DTYPE)
    N.check(engine._h, engine._lib.plda_fusion_side_fit_dev(engine._h, k, _vp(ptrs), _vp(lds), q, _vp(sraw), int(m), int(nt),
                                                            _p(denrol_spk), _p(dtest_spk), float(prior), float(tol), int(max_iter), _vp(raw)))
    del keep
    return _quality_fusion(raw, k, sides, prior)


def apply_with_sides_dev(engine, dscores, ld, sides, m, nt, fusion, dout, ld_out):
    """out[i, j] = (float)(the FMA chain from b over the K systems and the Q sides); dout may be one of the K matrices with
    ld_out equal to its pitch.  Enqueued on the engine's stream (no synchronisation): the side vectors must stay alive
    until the stream has run it."""
    k, ptrs, lds = _matrix_args(dscores, ld)
    q, sraw, keep = _side_args(sides, m, nt)
    a = _weights(fusion.a, k + q)
    N.check(engine._h, engine._lib.plda_fusion_side_map_dev(engine._h, k, _vp(ptrs), _vp(lds), q, _vp(sraw), int(m), int(nt), _vp(a),
                                                            float(fusion.b), _p(dout), int(ld_out)))
    return keep


def fit_from_operands_with_sides_dev(engine, du, dn, n_uniform, m, dv, nt, dzmean, dzstd, denrol_spk, dtest_spk, sides, prior=0.5,
                                     tol=0.0, max_iter=0):
    """The operand form: system 0 is the engine's own score matrix of (du, dn | n_uniform, dv, z-norm), produced slab by slab
    and never held (the arguments of plda_score_calib_fit_dev) -> `QualityFusion` over 1 system and Q sides."""
    sides = list(sides)
    q, sraw, keep = _side_args(sides, m, nt)
    raw = np.zeros(1, FIT_DTYPE)
    N.check(engine._h, engine._lib.plda_score_fusion_side_fit_dev(engine._h, _p(du), _p(dn), int(n_uniform), int(m), _p(dv), int(nt),
                                                                  _p(dzmean), _p(dzstd), _p(denrol_spk), _p(dtest_spk), q, _vp(sraw),
                                                                  float(prior), float(tol), int(max_iter), _vp(raw)))
    del keep
    return _quality_fusion(raw, 1, sides, prior)


def pass_from_operands_with_sides_dev(engine, du, dn, n_uniform, m, dv, nt, dzmean, dzstd, denrol_spk, dtest_spk, sides, a, c=0.0,
                                      theta=0.0):
    """One pass of the operand form; a has 1 + Q weights."""
    q, sraw, keep = _side_args(sides, m, nt)
    a = _weights(a, 1 + q)
    raw = np.zeros(1, RECORD_DTYPE)
    N.check(engine._h, engine._lib.plda_score_fusion_side_pass_dev(engine._h, _p(du), _p(dn), int(n_uniform), int(m), _p(dv), int(nt),
                                                                   _p(dzmean), _p(dzstd), _p(denrol_spk), _p(dtest_spk), q, _vp(sraw),
                                                                   _vp(a), float(c), float(theta), _vp(raw)))
    del keep
    return _record(raw)
