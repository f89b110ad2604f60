"""plda_amd/rocch.py -- the ROC convex hull of labelled trials on the GPU: minCllr, the ROCCH-EER and the PAV calibration
map (csrc/rocch.hip; the definitions are in include/plda_hip.h, "ROC convex hull").  Thin ctypes glue in the manner of
plda_amd/dcf.py.  Every call returns `(result, pav, info)`: the figures as a dict (Np, Nn, n_vertices, min_cllr, eer and
the rates of the two vertices around it), a `Pav` holding the vertices and the segment llrs, and the call's
`plda_rocch_info` as a dict (with `points=True`: plus "points", the reduced points every rank of which a test can check).
The calibration loss of a system is `cllr - result["min_cllr"]`."""
import ctypes as C

import numpy as np

from . import _native as N

# the structures of include/plda_hip.h
VERTEX_DTYPE = np.dtype([("x", np.uint64), ("y", np.uint64), ("fa", np.uint64), ("miss", np.uint64), ("threshold", np.float64),
                         ("key", np.uint32), ("has_key", np.int32)], align=True)
RESULT_DTYPE = np.dtype([("np", np.uint64), ("nn", np.uint64), ("n_vertices", np.int64), ("min_cllr", np.float64), ("eer", np.float64),
                         ("eer_far_lo", np.float64), ("eer_far_hi", np.float64), ("eer_frr_lo", np.float64), ("eer_frr_hi", np.float64)],
                        align=True)
INFO_DTYPE = np.dtype([("np", np.uint64), ("nn", np.uint64), ("t_raw", np.uint64), ("t_distinct", np.uint64), ("n_lds", np.uint64),
                       ("n_global_atomic", np.uint64), ("n_register", np.uint64), ("window_start", np.int64), ("window_size", np.int64),
                       ("reads", np.int32), ("launches", np.int32), ("edge_class", np.int32), ("coarse_read", np.int32),
                       ("neighbour_reads", np.int32), ("reserved", np.int32)], align=True)
assert (VERTEX_DTYPE.itemsize, RESULT_DTYPE.itemsize, INFO_DTYPE.itemsize) == (48, 72, 96)
MAX_PAV_VERTICES = 4097      # the device map's table: PLDA_E_CAPACITY above


class _Points(C.Structure):
    _fields_ = [("cap", C.c_int64), ("T", C.c_int64), ("edge_class", C.c_int32), ("reserved", C.c_int32), ("edge_key", C.c_void_p),
                ("other_lt", C.c_void_p), ("other_le", C.c_void_p), ("edge_lt", C.c_void_p), ("edge_le", C.c_void_p)]


def _p(x):
    return C.c_void_p(int(x)) if x else None


def score_keys(scores):
    """The order-preserving uint32 key of fp32 scores (-0.0 == +0.0), as csrc/trial_source.hpp forms it."""
    u = np.ascontiguousarray(scores, np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    neg = (u & 0x80000000) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


class Pav:
    """The PAV map of a ROCCH: `vertices` (VERTEX_DTYPE array) and `llr` (float64, one per segment).  Segment i covers the
    keys in (key(V_i), key(V_i+1)], the first also everything below, the last everything above.  Calling it maps NumPy
    scores on the host by the rule, table and roundings of the device kernel (`apply_dev`), bit for bit."""

    def __init__(self, vertices, llr):
        self.vertices = np.ascontiguousarray(vertices, VERTEX_DTYPE)
        self.llr = np.ascontiguousarray(llr, np.float64)
        assert self.llr.shape[0] == self.vertices.shape[0] - 1 >= 1

    def table(self, bound=0.0):
        t = self.llr if not bound > 0.0 else np.clip(self.llr, -bound, bound)
        return t.astype(np.float32)

    def __call__(self, scores, bound=0.0):
        s = np.ascontiguousarray(scores, np.float32)
        seg = np.searchsorted(self.vertices["key"][1:-1], score_keys(s.reshape(-1)), side="left")
        out = self.table(bound)[seg].reshape(s.shape)
        nan = np.isnan(s)
        out[nan] = s[nan]
        return out

    def apply_dev(self, engine, dscores, ld, m, nt, dout=None, ld_out=None, bound=0.0):
        """`plda_pav_map_dev` on an HBM-resident fp32 matrix; in place when `dout` is None.  Enqueues the map on the
        engine's stream (the call waits only for its table's upload)."""
        if dout is None:
            dout, ld_out = dscores, ld
        N.check(engine._h, engine._lib.plda_pav_map_dev(engine._h, _p(dscores), int(ld), int(m), int(nt), self.vertices.shape[0],
                                                        C.c_void_p(self.vertices.ctypes.data), C.c_void_p(self.llr.ctypes.data),
                                                        float(bound), _p(dout), int(ld_out if ld_out is not None else nt)))


def _result(raw):
    r = raw[0]
    return {"Np": int(r["np"]), "Nn": int(r["nn"]), "n_vertices": int(r["n_vertices"]), "min_cllr": float(r["min_cllr"]),
            "eer": float(r["eer"]), "eer_far_lo": float(r["eer_far_lo"]), "eer_far_hi": float(r["eer_far_hi"]),
            "eer_frr_lo": float(r["eer_frr_lo"]), "eer_frr_hi": float(r["eer_frr_hi"])}


def _info(raw):
    r = raw[0]
    return {k: int(r[k]) for k in ("t_raw", "t_distinct", "n_lds", "n_global_atomic", "n_register", "window_start", "window_size", "reads",
                                   "launches", "edge_class", "coarse_read", "neighbour_reads")}


def _call(engine, fn, args, points, points_bound, cap_vertices):
    cap = 8192 if cap_vertices is None else int(cap_vertices)
    pts = arrays = None
    if points:
        n = max(int(points_bound), 1)
        arrays = {"edge_key": np.zeros(n, np.uint32), "other_lt": np.zeros(n, np.uint64), "other_le": np.zeros(n, np.uint64),
                  "edge_lt": np.zeros(n, np.uint64), "edge_le": np.zeros(n, np.uint64)}
        pts = _Points(n, 0, 0, 0, *[a.ctypes.data for a in arrays.values()])
    while True:
        out, info = np.zeros(1, RESULT_DTYPE), np.zeros(1, INFO_DTYPE)
        verts, llr = np.zeros(max(cap, 1), VERTEX_DTYPE), np.zeros(max(cap, 1), np.float64)
        rc = fn(engine._h, *(list(args) + [cap, C.c_void_p(out.ctypes.data), C.c_void_p(verts.ctypes.data), C.c_void_p(llr.ctypes.data),
                                          C.byref(pts) if pts is not None else None, C.c_void_p(info.ctypes.data)]))
        need = int(out[0]["n_vertices"])
        if rc == N.PLDA_E_CAPACITY and cap_vertices is None and need > cap:
            cap = need          # (the whole call again: hulls of more than 8192 vertices are not expected)
            continue
        N.check(engine._h, rc)
        break
    inf = _info(info)
    if points:
        inf["points"] = dict({k: a[:pts.T].copy() for k, a in arrays.items()}, T=int(pts.T), edge_class=int(pts.edge_class))
    return _result(out), Pav(verts[:need].copy(), llr[:need - 1].copy()), inf


def rocch_from_lists(engine, truescores, impostscores, points=False, cap_vertices=None):
    """The ROCCH of target / non-target score arrays on the host."""
    pos = np.ascontiguousarray(truescores, np.float32)
    neg = np.ascontiguousarray(impostscores, np.float32)
    return _call(engine, engine._lib.plda_rocch_lists, [C.c_void_p(pos.ctypes.data), pos.shape[0], C.c_void_p(neg.ctypes.data), neg.shape[0]],
                 points, min(pos.shape[0], neg.shape[0]), cap_vertices)


def rocch_from_matrix_dev(engine, dscores, ld, m, nt, denrol_spk, dtest_spk, points=False, cap_vertices=None):
    """Same on an HBM-resident fp32 trials matrix; trial (i, j) is a target iff enrol_spk[i] == test_spk[j] (int64 device
    arrays)."""
    return _call(engine, engine._lib.plda_rocch_matrix_dev, [_p(dscores), int(ld), int(m), int(nt), _p(denrol_spk), _p(dtest_spk)],
                 points, (int(m) * int(nt)) // 2 + 1, cap_vertices)


def rocch_from_operands_dev(engine, dU, dn, n_uniform, m, dV, nt, denrol_spk, dtest_spk, dzmean=None, dzstd=None, points=False,
                            cap_vertices=None):
    """Same without the matrix (arguments as `eer.eer_from_operands_dev`); the slabs are re-scored once per read."""
    return _call(engine, engine._lib.plda_score_rocch_dev,
                 [_p(dU), _p(dn), int(n_uniform), int(m), _p(dV), int(nt), _p(dzmean), _p(dzstd), _p(denrol_spk), _p(dtest_spk)],
                 points, (int(m) * int(nt)) // 2 + 1, cap_vertices)


# ---------------------------------------------------------------------------------------------- the host steps (no GPU)
def host_hull(edge_key, other_lt, other_le, edge_lt, edge_le, edge_class, n_pos, n_neg, cap_vertices=None):
    """`plda_rocch_hull`: the reduced points -> (status, result dict, vertices, llr).  A vertex's `key` is the edge of its
    cut and its threshold NaN until `host_finish`."""
    lib = N.load()
    ek = np.ascontiguousarray(edge_key, np.uint32)
    arrs = [np.ascontiguousarray(a, np.uint64) for a in (other_lt, other_le, edge_lt, edge_le)]
    T = ek.shape[0]
    assert all(a.shape == (T,) for a in arrs)
    cap = 2 * T + 2 if cap_vertices is None else int(cap_vertices)
    out = np.zeros(1, RESULT_DTYPE)
    verts, llr = np.zeros(max(cap, 1), VERTEX_DTYPE), np.zeros(max(cap, 1), np.float64)
    rc = lib.plda_rocch_hull(T, C.c_void_p(ek.ctypes.data), *[C.c_void_p(a.ctypes.data) for a in arrs], int(edge_class), int(n_pos),
                             int(n_neg), cap, C.c_void_p(out.ctypes.data), C.c_void_p(verts.ctypes.data), C.c_void_p(llr.ctypes.data))
    n = int(out[0]["n_vertices"]) if rc == N.PLDA_OK else 0
    return rc, _result(out), verts[:n].copy(), llr[:max(n - 1, 0)].copy()


def host_finish(vertices, below, above):
    """`plda_rocch_finish`: the vertices' keys and thresholds from the keys next to their cuts.  Returns (status, vertices)."""
    lib = N.load()
    v = np.ascontiguousarray(vertices, VERTEX_DTYPE).copy()
    lo, hi = np.ascontiguousarray(below, np.uint32), np.ascontiguousarray(above, np.uint32)
    assert lo.shape == hi.shape == v.shape
    rc = lib.plda_rocch_finish(v.shape[0], C.c_void_p(v.ctypes.data), C.c_void_p(lo.ctypes.data), C.c_void_p(hi.ctypes.data))
    return rc, v
