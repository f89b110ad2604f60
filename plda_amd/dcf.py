"""plda_amd/dcf.py -- exact minimum detection cost (minDCF) at several operating points on the GPU (csrc/dcf.hip; the
definition is in include/plda_hip.h, "exact minimum detection cost").  Thin ctypes glue in the manner of plda_amd/eer.py.
Every call returns `(results, info)`: one dict per operating point (min_dcf, threshold, far, frr, miss, fa) and the
call's `plda_min_dcf_info` as a dict.  The calibration loss of a system at a point is
`calibration.act_dcf(...) - results[i]["min_dcf"]` (a plain subtraction: both are normalised by the same constant)."""
import ctypes as C

import numpy as np

from . import _native as N

MAX_POINTS = 8
# the structures of include/plda_hip.h
POINT_DTYPE = np.dtype([("prior", np.float64), ("c_miss", np.float64), ("c_fa", np.float64)], align=True)
RESULT_DTYPE = np.dtype([("min_dcf", np.float64), ("threshold", np.float64), ("far", np.float64), ("frr", np.float64),
                         ("miss", np.uint64), ("fa", np.uint64)], align=True)
INFO_DTYPE = np.dtype([("np", np.uint64), ("nn", np.uint64), ("reads", np.int32), ("launches", np.int32), ("lists_used", np.int32),
                       ("neighbour_reads", np.int32), ("level_launches", np.int32, (3,)), ("reserved", np.int32),
                       ("level_bins", np.int64, (3,)), ("level_trials", np.uint64, (3,))], align=True)
NODE_DTYPE = np.dtype([("prefix", np.uint32), ("reserved", np.uint32), ("miss_below", np.uint64), ("nn_below", np.uint64),
                       ("n_pos", np.uint64), ("n_neg", np.uint64)], align=True)
CUT_DTYPE = np.dtype([("value", np.float64), ("miss", np.uint64), ("fa", np.uint64), ("edge", np.uint32), ("has_edge", np.int32)],
                     align=True)
STATE_DTYPE = np.dtype([("np", np.uint64), ("nn", np.uint64), ("nonfinite", np.uint64), ("best", CUT_DTYPE, (MAX_POINTS,))], align=True)
assert (POINT_DTYPE.itemsize, RESULT_DTYPE.itemsize, INFO_DTYPE.itemsize, NODE_DTYPE.itemsize, CUT_DTYPE.itemsize,
        STATE_DTYPE.itemsize) == (24, 48, 96, 40, 32, 280)


def _p(x):
    return C.c_void_p(int(x)) if x else None


def _points(points):
    pts = np.zeros(len(points), POINT_DTYPE)
    for i, pt in enumerate(points):
        pts[i] = tuple(float(v) for v in pt)
    if not 1 <= len(pts) <= MAX_POINTS:
        raise ValueError("min_dcf: 1 .. %d operating points (prior, c_miss, c_fa)" % MAX_POINTS)
    return pts


def _results(raw):
    return [{"min_dcf": float(r["min_dcf"]), "threshold": float(r["threshold"]), "far": float(r["far"]), "frr": float(r["frr"]),
             "miss": int(r["miss"]), "fa": int(r["fa"])} for r in raw]


def _info(raw):
    r = raw[0]
    return {"Np": int(r["np"]), "Nn": int(r["nn"]), "reads": int(r["reads"]), "launches": int(r["launches"]),
            "lists_used": bool(r["lists_used"]), "neighbour_reads": int(r["neighbour_reads"]),
            "level_launches": [int(v) for v in r["level_launches"]], "level_bins": [int(v) for v in r["level_bins"]],
            "level_trials": [int(v) for v in r["level_trials"]]}


def _call(engine, fn, args, points):
    pts = _points(points)
    out, info = np.zeros(len(pts), RESULT_DTYPE), np.zeros(1, INFO_DTYPE)
    N.check(engine._h, fn(engine._h, *(list(args) + [len(pts), C.c_void_p(pts.ctypes.data), C.c_void_p(out.ctypes.data),
                                                    C.c_void_p(info.ctypes.data)])))
    return _results(out), _info(info)


def min_dcf_from_lists(engine, truescores, impostscores, points=((0.01, 1.0, 1.0),)):
    """minDCF at `points` = ((prior, c_miss, c_fa), ...) from target / non-target score arrays on the host."""
    pos = np.ascontiguousarray(truescores, np.float32)
    neg = np.ascontiguousarray(impostscores, np.float32)
    return _call(engine, engine._lib.plda_min_dcf_lists,
                 [C.c_void_p(pos.ctypes.data), pos.shape[0], C.c_void_p(neg.ctypes.data), neg.shape[0]], points)


def min_dcf_from_matrix_dev(engine, dscores, ld, m, nt, denrol_spk, dtest_spk, points=((0.01, 1.0, 1.0),)):
    """Same on an HBM-resident fp32 trials matrix; trial (i, j) is a target iff enrol_spk[i] == test_spk[j] (int64 device
    arrays)."""
    return _call(engine, engine._lib.plda_min_dcf_matrix_dev, [_p(dscores), int(ld), int(m), int(nt), _p(denrol_spk), _p(dtest_spk)],
                 points)


def min_dcf_from_matrix_comm_dev(engine, dscores, ld, m, nt, denrol_spk, dtest_spk, points=((0.01, 1.0, 1.0),)):
    """The row-sharded form: this rank's rows of the matrix (m may be 0), every histogram summed through the engine's
    communicator; every rank gets the global result."""
    return _call(engine, engine._lib.plda_min_dcf_matrix_comm_dev,
                 [_p(dscores), int(ld), int(m), int(nt), _p(denrol_spk), _p(dtest_spk)], points)


def min_dcf_from_operands_dev(engine, dU, dn, n_uniform, m, dV, nt, denrol_spk, dtest_spk, dzmean=None, dzstd=None,
                              points=((0.01, 1.0, 1.0),)):
    """Same without the matrix (arguments as `eer.eer_from_operands_dev`); the slabs are re-scored once per read."""
    return _call(engine, engine._lib.plda_score_min_dcf_dev,
                 [_p(dU), _p(dn), int(n_uniform), int(m), _p(dV), int(nt), _p(dzmean), _p(dzstd), _p(denrol_spk), _p(dtest_spk)], points)


# ---------------------------------------------------------------------------------------------- the host step (no GPU)
def host_step(level, nodes, hist, points, state, cap_next):
    """`plda_min_dcf_step`: nodes (NODE_DTYPE array), hist (uint64 [n_nodes, 2, 2048]), state (STATE_DTYPE array of one,
    updated in place).  Returns (status, surviving nodes)."""
    lib = N.load()
    pts = _points(points)
    nodes = np.ascontiguousarray(nodes, NODE_DTYPE)
    hist = np.ascontiguousarray(hist, np.uint64)
    assert hist.shape == (len(nodes), 2, 2048) and state.dtype == STATE_DTYPE
    nxt = np.zeros(max(int(cap_next), 1), NODE_DTYPE)
    n_next = C.c_int64(0)
    rc = lib.plda_min_dcf_step(int(level), len(nodes), C.c_void_p(nodes.ctypes.data), C.c_void_p(hist.ctypes.data), len(pts),
                               C.c_void_p(pts.ctypes.data), C.c_void_p(state.ctypes.data), int(cap_next),
                               C.c_void_p(nxt.ctypes.data), C.byref(n_next))
    return rc, nxt[:n_next.value].copy()


def host_finish(state, points, below, above):
    """`plda_min_dcf_finish`: the reported figures from the incumbents and the keys next to their edges."""
    lib = N.load()
    pts = _points(points)
    lo, hi = np.zeros(MAX_POINTS, np.uint32), np.full(MAX_POINTS, 0xffffffff, np.uint32)
    lo[:len(pts)], hi[:len(pts)] = below, above
    out = np.zeros(len(pts), RESULT_DTYPE)
    rc = lib.plda_min_dcf_finish(C.c_void_p(state.ctypes.data), len(pts), C.c_void_p(pts.ctypes.data), C.c_void_p(lo.ctypes.data),
                                 C.c_void_p(hi.ctypes.data), C.c_void_p(out.ctypes.data))
    return rc, _results(out)
