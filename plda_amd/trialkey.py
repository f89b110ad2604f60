"""plda_amd/trialkey.py -- trial keys: masked trials and per-condition metrics on the GPU (csrc/partition.hip; the
definitions are in include/plda_hip.h, "trial keys").  A `TrialKey` says which (enrol, test) pairs are trials and which
condition bucket each belongs to; `partition_matrix_dev` / `partition_from_operands_dev` turn a trials matrix (resident, or
scored slab by slab) into per-(bucket, class) score lists on the device, in an order that depends on the key and the
speaker ids alone; `metrics` runs the device-list forms of the consumers on them, per bucket, pooled and equalised."""
import ctypes as C

import numpy as np

from . import _native as N

MAX_CODES = 128      # PLDA_KEY_MAX_CODES
MAX_BUCKETS = 8      # PLDA_KEY_MAX_BUCKETS
STRIP = 256          # PLDA_PARTITION_STRIP
# struct plda_partition_record of include/plda_hip.h: [bucket][class], class 1 = targets
RECORD_DTYPE = np.dtype([("count", np.int64, (MAX_BUCKETS, 2)), ("offset", np.int64, (MAX_BUCKETS, 2)), ("total", np.int64, (2,))],
                        align=True)
assert RECORD_DTYPE.itemsize == 272


class _Key(C.Structure):
    """struct plda_trial_key"""
    _fields_ = [("enrol_code", C.c_void_p), ("test_code", C.c_void_p), ("table", C.c_void_p), ("n_enrol_codes", C.c_int32),
                ("n_test_codes", C.c_int32), ("n_buckets", C.c_int32), ("reserved", C.c_int32)]


def _labels(*sides):
    """the distinct labels of the sides: sorted where they compare, else in order of first appearance"""
    seen = {}
    for side in sides:
        for v in side:
            seen.setdefault(v, None)
    try:
        return sorted(seen)
    except TypeError:
        return list(seen)


def _as_labels(cond):
    a = cond.tolist() if isinstance(cond, np.ndarray) else list(cond)
    return [tuple(v) if isinstance(v, list) else v for v in a]


class TrialKey(object):
    """Which pairs are trials, and their condition buckets.  `enrol_cond` / `test_cond`: one hashable label per enrol row /
    test column.  rule:
      "same"    a pair is a trial iff its two labels are equal; one bucket per label present on both sides (gender-matched);
      "all"     one bucket, every pair is a trial (the labels are not looked at; both may be lengths);
      mapping   {(enrol label, test label): bucket name}; pairs it does not name are not trials.
    Holds `enrol_code` / `test_code` (uint8), `table` (int8 [n_enrol_codes, n_test_codes], -1: not a trial) and
    `bucket_names`."""

    def __init__(self, enrol_cond, test_cond, rule="same"):
        if isinstance(rule, str) and rule == "all":
            m = int(enrol_cond) if np.isscalar(enrol_cond) else len(enrol_cond)
            nt = int(test_cond) if np.isscalar(test_cond) else len(test_cond)
            self._set(np.zeros(m, np.uint8), np.zeros(nt, np.uint8), np.zeros((1, 1), np.int8), ["all"])
            return
        el, tl = _as_labels(enrol_cond), _as_labels(test_cond)
        ecodes, tcodes = _labels(el), _labels(tl)
        if len(ecodes) > MAX_CODES or len(tcodes) > MAX_CODES:
            raise ValueError("TrialKey: %d enrol and %d test labels (at most %d per side)" % (len(ecodes), len(tcodes), MAX_CODES))
        eidx, tidx = {v: i for i, v in enumerate(ecodes)}, {v: i for i, v in enumerate(tcodes)}
        table = np.full((max(len(ecodes), 1), max(len(tcodes), 1)), -1, np.int8)
        names = []
        if isinstance(rule, str):
            if rule != "same":
                raise ValueError("TrialKey: rule must be 'same', 'all' or a {(enrol label, test label): bucket} mapping")
            for v in ecodes:
                if v in tidx:
                    table[eidx[v], tidx[v]] = len(names)
                    names.append(v)
        else:
            for (e, t), name in rule.items():
                if name not in names:
                    names.append(name)
                if e in eidx and t in tidx:
                    table[eidx[e], tidx[t]] = names.index(name)
        if not names:
            names = ["none"]          # (a key that selects nothing is a key: every count is 0)
        if len(names) > MAX_BUCKETS:
            raise ValueError("TrialKey: %d buckets (at most %d)" % (len(names), MAX_BUCKETS))
        self._set(np.array([eidx[v] for v in el], np.uint8), np.array([tidx[v] for v in tl], np.uint8), table, names)

    def _set(self, enrol_code, test_code, table, names):
        self.enrol_code = np.ascontiguousarray(enrol_code, np.uint8)
        self.test_code = np.ascontiguousarray(test_code, np.uint8)
        self.table = np.ascontiguousarray(table, np.int8)
        self.bucket_names = list(names)
        self._dev = {}

    @classmethod
    def from_codes(cls, enrol_code, test_code, table, bucket_names=None):
        """A key from its parts, unchecked (the library checks them): codes (uint8), table (int8 [Ce, Ct])."""
        table = np.asarray(table, np.int8)
        k = cls.__new__(cls)
        k._set(enrol_code, test_code, table, bucket_names if bucket_names is not None else list(range(max(int(table.max()) + 1, 1))))
        return k

    @classmethod
    def product(cls, k1, k2):
        """The cross of two keys over the same rows and columns (gender x language): a pair is a trial iff it is one under
        both, its bucket the pair of buckets.  Raises where the cross exceeds the limits."""
        if k1.enrol_code.shape != k2.enrol_code.shape or k1.test_code.shape != k2.test_code.shape:
            raise ValueError("TrialKey.product: the keys cover different rows or columns")
        (ce1, ct1), (ce2, ct2) = k1.table.shape, k2.table.shape
        if ce1 * ce2 > MAX_CODES or ct1 * ct2 > MAX_CODES or k1.n_buckets * k2.n_buckets > MAX_BUCKETS:
            raise ValueError("TrialKey.product: %d x %d codes and %d buckets (at most %d codes per side, %d buckets)"
                             % (ce1 * ce2, ct1 * ct2, k1.n_buckets * k2.n_buckets, MAX_CODES, MAX_BUCKETS))
        t1 = k1.table.astype(np.int64)[:, None, :, None]
        t2 = k2.table.astype(np.int64)[None, :, None, :]
        table = np.where((t1 >= 0) & (t2 >= 0), t1 * k2.n_buckets + t2, -1).reshape(ce1 * ce2, ct1 * ct2)
        names = [(a, b) for a in k1.bucket_names for b in k2.bucket_names]
        return cls.from_codes(k1.enrol_code.astype(np.int64) * ce2 + k2.enrol_code, k1.test_code.astype(np.int64) * ct2 + k2.test_code,
                              table, names)

    @property
    def n_buckets(self):
        return len(self.bucket_names)

    @property
    def shape(self):
        return self.enrol_code.shape[0], self.test_code.shape[0]

    def mask(self):
        """The bucket of every pair (int8 [M, Nt], -1: not a trial) on the host -- for small keys and tests."""
        return self.table[self.enrol_code[:, None], self.test_code[None, :]]

    def _struct(self, enrol_code_ptr, test_code_ptr):
        return _Key(enrol_code_ptr, test_code_ptr, self.table.ctypes.data, self.table.shape[0], self.table.shape[1], self.n_buckets, 0)

    def plan(self, enrol_spk, test_spk):
        """`plda_partition_plan` on the host (no GPU): the record (RECORD_DTYPE array of one) for these speaker ids."""
        es, ts = np.ascontiguousarray(enrol_spk, np.int64), np.ascontiguousarray(test_spk, np.int64)
        if es.shape != self.enrol_code.shape or ts.shape != self.test_code.shape:
            raise ValueError("TrialKey.plan: %d / %d speaker ids for a key of %d rows and %d columns"
                             % (es.shape[0], ts.shape[0], self.shape[0], self.shape[1]))
        rec = np.zeros(1, RECORD_DTYPE)
        key = self._struct(self.enrol_code.ctypes.data, self.test_code.ctypes.data)
        rc = N.load().plda_partition_plan(C.c_void_p(es.ctypes.data), es.shape[0], C.c_void_p(ts.ctypes.data), ts.shape[0],
                                          C.cast(C.byref(key), C.c_void_p), C.c_void_p(rec.ctypes.data))
        N.check(None, rc)
        return rec

    def device_codes(self, device):
        """the two code arrays as torch uint8 tensors on `device` (kept)"""
        import torch
        dev = torch.device(device)
        if dev not in self._dev:
            self._dev[dev] = (torch.from_numpy(self.enrol_code).to(dev), torch.from_numpy(self.test_code).to(dev))
        return self._dev[dev]


class Partition(object):
    """The lists of a partition: two torch fp32 device buffers and the plan.  `tar(b)` / `non(b)`: views of bucket b's (an
    index or a bucket name) target / non-target list; `pooled()`: the (targets, non-targets) of all buckets, which are the
    buffers themselves; `counts`: int64 [n_buckets, 2], column 1 = targets."""

    def __init__(self, key, record, dtar, dnon):
        self.key, self.record, self.dtar, self.dnon = key, record, dtar, dnon
        self.bucket_names = list(key.bucket_names)

    @property
    def counts(self):
        return self.record[0]["count"][:len(self.bucket_names)].copy()

    @property
    def totals(self):
        return int(self.record[0]["total"][1]), int(self.record[0]["total"][0])

    def _bucket(self, b):
        if isinstance(b, (int, np.integer)) and not isinstance(b, bool) and b not in self.bucket_names:
            return int(b)
        return self.bucket_names.index(b)

    def _view(self, buf, b, cls):
        b = self._bucket(b)
        off, n = int(self.record[0]["offset"][b][cls]), int(self.record[0]["count"][b][cls])
        return buf[off:off + n]

    def tar(self, b):
        return self._view(self.dtar, b, 1)

    def non(self, b):
        return self._view(self.dnon, b, 0)

    def pooled(self):
        nt, nn = self.totals
        return self.dtar[:nt], self.dnon[:nn]


def _buffers(record, device, guard=0):
    import torch
    nt, nn = int(record[0]["total"][1]), int(record[0]["total"][0])
    return (torch.empty(max(nt + guard, 1), dtype=torch.float32, device=device),
            torch.empty(max(nn + guard, 1), dtype=torch.float32, device=device))


def partition_matrix_dev(engine, key, S, denrol_spk, dtest_spk):
    """Partition the HBM-resident fp32 trials matrix `S` (a torch device tensor [M, Nt] with contiguous rows; its row stride is
    the pitch) under `key`; `denrol_spk` / `dtest_spk`: int64 torch device tensors.  Returns a `Partition`.  The partition
    kernel is enqueued on the engine's stream; consumers called through the same engine are ordered behind it."""
    m, nt = int(S.shape[0]), int(S.shape[1])
    if (m, nt) != key.shape:
        raise ValueError("partition: a %d x %d matrix under a key of %d rows and %d columns" % ((m, nt) + key.shape))
    rec = key.plan(denrol_spk.cpu().numpy(), dtest_spk.cpu().numpy())
    dtar, dnon = _buffers(rec, S.device)
    dec, dtc = key.device_codes(S.device)
    ks = key._struct(dec.data_ptr(), dtc.data_ptr())
    out = np.zeros(1, RECORD_DTYPE)
    ld = int(S.stride(0)) if m > 1 else max(nt, int(S.stride(0)))
    N.check(engine._h, engine._lib.plda_partition_matrix_dev(
        engine._h, C.c_void_p(S.data_ptr()), ld, m, nt, C.c_void_p(denrol_spk.data_ptr()), C.c_void_p(dtest_spk.data_ptr()),
        C.cast(C.byref(ks), C.c_void_p), C.c_void_p(dtar.data_ptr()), int(rec[0]["total"][1]), C.c_void_p(dnon.data_ptr()),
        int(rec[0]["total"][0]), C.c_void_p(out.ctypes.data)))
    return Partition(key, out, dtar, dnon)


def partition_from_operands_dev(engine, key, dU, dn, n_uniform, dV, denrol_spk, dtest_spk, dzmean=None, dzstd=None):
    """The same lists without the matrix (`plda_score_partition_dev`): dU [M, D] / dV [Nt, D] fp64 torch device tensors of
    transformed vectors, dn the int32 enrol counts (None: n_uniform), the z-norm statistics or None.  Bit-identical to
    scoring the matrix and partitioning it."""
    m, nt = int(dU.shape[0]), int(dV.shape[0])
    if (m, nt) != key.shape:
        raise ValueError("partition: %d x %d operands under a key of %d rows and %d columns" % ((m, nt) + key.shape))
    rec = key.plan(denrol_spk.cpu().numpy(), dtest_spk.cpu().numpy())
    dtar, dnon = _buffers(rec, dU.device)
    dec, dtc = key.device_codes(dU.device)
    ks = key._struct(dec.data_ptr(), dtc.data_ptr())
    out = np.zeros(1, RECORD_DTYPE)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    N.check(engine._h, engine._lib.plda_score_partition_dev(
        engine._h, p(dU), p(dn), int(n_uniform), m, p(dV), nt, p(dzmean), p(dzstd), p(denrol_spk), p(dtest_spk),
        C.cast(C.byref(ks), C.c_void_p), p(dtar), int(rec[0]["total"][1]), p(dnon), int(rec[0]["total"][0]),
        C.c_void_p(out.ctypes.data)))
    engine.synchronize()             # (the operands may be freed when this returns)
    return Partition(key, out, dtar, dnon)


# ---------------------------------------------------------------------------------------------- the consumers on device lists
def _args(tar, non):
    return [C.c_void_p(tar.data_ptr()), int(tar.shape[0]), C.c_void_p(non.data_ptr()), int(non.shape[0])]


def eer_lists_dev(engine, tar, non):
    """`plda_eer_lists_dev`: the 6-vector (threshold, FAR, FRR, EER, #targets, #impostors) of two torch device lists."""
    out = np.zeros(6)
    N.check(engine._h, engine._lib.plda_eer_lists_dev(engine._h, *(_args(tar, non) + [C.c_void_p(out.ctypes.data)])))
    return out


def det_lists_dev(engine, tar, non, n_points=100):
    far, frr, thr = np.zeros(n_points), np.zeros(n_points), np.zeros(n_points)
    N.check(engine._h, engine._lib.plda_det_lists_dev(engine._h, *(_args(tar, non) + [int(n_points), C.c_void_p(far.ctypes.data),
                                                                                      C.c_void_p(frr.ctypes.data), C.c_void_p(thr.ctypes.data)])))
    return thr, far, frr


def min_dcf_lists_dev(engine, tar, non, points=((0.01, 1.0, 1.0),)):
    from . import dcf as DC
    return DC._call(engine, engine._lib.plda_min_dcf_lists_dev, _args(tar, non), points)


def calib_pass_lists_dev(engine, tar, non, a=1.0, c=0.0, theta=0.0):
    from . import calibration as CB
    raw = np.zeros(1, CB.RECORD_DTYPE)
    N.check(engine._h, engine._lib.plda_calib_pass_lists_dev(engine._h, *(_args(tar, non) + [float(a), float(c), float(theta),
                                                                                             C.c_void_p(raw.ctypes.data)])))
    return CB._record(raw)


def calib_fit_lists_dev(engine, tar, non, prior=0.5, tol=0.0, max_iter=0):
    from . import calibration as CB
    raw = np.zeros(1, CB.FIT_DTYPE)
    N.check(engine._h, engine._lib.plda_calib_fit_lists_dev(engine._h, *(_args(tar, non) + [float(prior), float(tol), int(max_iter),
                                                                                            C.c_void_p(raw.ctypes.data)])))
    return CB._calibration(raw, prior)


def rocch_lists_dev(engine, tar, non, points=False, cap_vertices=None):
    from . import rocch as RC
    return RC._call(engine, engine._lib.plda_rocch_lists_dev, _args(tar, non), points, min(int(tar.shape[0]), int(non.shape[0])),
                    cap_vertices)


def _fusion_args(tars, nons):
    k = len(tars)
    if k != len(nons) or k < 1 or any(t.shape != tars[0].shape for t in tars) or any(n.shape != nons[0].shape for n in nons):
        raise ValueError("fusion lists: K target and K non-target lists of equal lengths")
    pp = (C.c_void_p * k)(*[t.data_ptr() for t in tars])
    pn = (C.c_void_p * k)(*[n.data_ptr() for n in nons])
    return k, pp, pn


def fusion_pass_lists_dev(engine, tars, nons, a, c=0.0, theta=0.0):
    """`plda_fusion_pass_lists_dev` on K aligned pairs of torch device lists (K systems partitioned with one key)."""
    from . import fusion as FU
    k, pp, pn = _fusion_args(tars, nons)
    w = FU._weights(a, k)
    raw = np.zeros(1, FU.RECORD_DTYPE)
    N.check(engine._h, engine._lib.plda_fusion_pass_lists_dev(engine._h, k, C.cast(pp, C.c_void_p), int(tars[0].shape[0]),
                                                              C.cast(pn, C.c_void_p), int(nons[0].shape[0]), C.c_void_p(w.ctypes.data),
                                                              float(c), float(theta), C.c_void_p(raw.ctypes.data)))
    return FU._record(raw)


def fusion_fit_lists_dev(engine, tars, nons, prior=0.5, tol=0.0, max_iter=0):
    """`plda_fusion_fit_lists_dev`: a `plda_amd.fusion.Fusion`, as `fusion.fit_from_lists` returns it."""
    from . import fusion as FU
    k, pp, pn = _fusion_args(tars, nons)
    raw = np.zeros(1, FU.FIT_DTYPE)
    N.check(engine._h, engine._lib.plda_fusion_fit_lists_dev(engine._h, k, C.cast(pp, C.c_void_p), int(tars[0].shape[0]),
                                                             C.cast(pn, C.c_void_p), int(nons[0].shape[0]), float(prior), float(tol),
                                                             int(max_iter), C.c_void_p(raw.ctypes.data)))
    return FU._fusion(raw, k, prior)


# ---------------------------------------------------------------------------------------------- per-condition metrics
def _figures(engine, tar, non, points, prior):
    from . import calibration as CB
    out = {"n_tar": int(tar.shape[0]), "n_non": int(non.shape[0]), "eer": None, "min_dcf": None, "act_dcf": None, "cllr": None,
           "min_cllr": None}
    if out["n_tar"] == 0 or out["n_non"] == 0:
        return out
    out["eer"] = float(eer_lists_dev(engine, tar, non)[3])
    out["min_dcf"] = [r["min_dcf"] for r in min_dcf_lists_dev(engine, tar, non, points)[0]]
    out["act_dcf"] = [CB.act_dcf(lambda th: calib_pass_lists_dev(engine, tar, non, theta=th), float(p), float(cm), float(cf))
                      for p, cm, cf in points]
    out["cllr"] = CB.objective(calib_pass_lists_dev(engine, tar, non), prior) / CB.LN2
    out["min_cllr"] = rocch_lists_dev(engine, tar, non)[0]["min_cllr"]
    return out


def metrics(engine, part, points=((0.01, 1.0, 1.0),), prior=0.5):
    """Per bucket, pooled and equalised figures of a `Partition`, all through the device-list entry points:
    {"buckets": {name: f}, "pooled": f, "equalised": g} with f = {n_tar, n_non, eer, min_dcf [per point], act_dcf [per point:
    the actual DCF of the scores as LLRs at the point's Bayes threshold], cllr (prior-weighted; prior = 0.5: Cllr), min_cllr}.
    A bucket without a target or without a non-target has its counts and None figures and is named in
    equalised["skipped"]; `equalised` is the unweighted mean of the other buckets' figures (NIST's equalisation; None where
    no bucket counts)."""
    points = tuple(tuple(float(v) for v in pt) for pt in points)
    buckets = {}
    for b, name in enumerate(part.bucket_names):
        buckets[name] = _figures(engine, part.tar(b), part.non(b), points, prior)
    pooled = _figures(engine, *(part.pooled() + (points, prior)))
    used = [n for n in part.bucket_names if buckets[n]["eer"] is not None]
    eq = {"skipped": [n for n in part.bucket_names if buckets[n]["eer"] is None], "n_buckets": len(used)}
    for k in ("eer", "cllr", "min_cllr"):
        eq[k] = float(np.mean([buckets[n][k] for n in used])) if used else None
    for k in ("min_dcf", "act_dcf"):
        eq[k] = [float(np.mean([buckets[n][k][i] for n in used])) for i in range(len(points))] if used else None
    return {"buckets": buckets, "pooled": pooled, "equalised": eq}
