"""Host model of the side-information terms of a quality-aware calibration (include/plda_hip.h, "quality-aware
calibration"; csrc/fusion.hip).  A side is ONE IEEE fp32 operation on a per-enrol-row and a per-test-column number;
everything after it -- the chain, the record, the Newton fit -- is tests/fusion_model.py on the MATERIALISED side, which is
the contract the device is held to bit for bit.  Written from the header's table alone (plda_amd/fusion.py has its own)."""
import numpy as np

OPS = ("min", "max", "sum", "absdiff", "prod")


def side_values(op, e, t):
    """op as a name or its code 0 .. 4; e and t broadcast against each other; fp32 in, one fp32 operation, fp32 out."""
    code = OPS.index(op) if isinstance(op, str) else int(op)
    if not 0 <= code < len(OPS):
        raise ValueError("op outside 0 .. 4")
    e, t = np.asarray(e, np.float32), np.asarray(t, np.float32)
    e, t = np.broadcast_arrays(e, t)
    out = np.empty(e.shape, np.float32)
    with np.errstate(all="ignore"):
        if code == 0:
            lt = e < t                         # e < t ? e : t  (a tie, a NaN: t)
            out[...] = t
            out[lt] = e[lt]
        elif code == 1:
            gt = e > t                         # e > t ? e : t
            out[...] = t
            out[gt] = e[gt]
        elif code == 2:
            out[...] = e + t
        elif code == 3:
            out[...] = np.fabs(e - t)
        else:
            out[...] = e * t
    assert out.dtype == np.float32
    return out


def materialise(sides, m, nt):
    """[(op, enrol[M], test[Nt]), ...] -> the fp32 [M, Nt] matrix of every side."""
    out = []
    for op, e, t in sides:
        e, t = np.asarray(e, np.float32), np.asarray(t, np.float32)
        assert e.shape == (m,) and t.shape == (nt,)
        out.append(side_values(op, e[:, None], t[None, :]))
    return out


def planted_case():
    """The planted case of K25: 300 x 500 trials, speakers drawn from 60, log-durations qe / qt, and a score whose class
    means move with min(qe, qt) -- so the score alone cannot be calibrated as well as the score with its quality.
    Returns (es, ts, s fp32 [M, Nt], qe fp32 [M], qt fp32 [Nt])."""
    rng = np.random.default_rng(7)
    m, nt = 300, 500
    es, ts = rng.integers(0, 60, m).astype(np.int64), rng.integers(0, 60, nt).astype(np.int64)
    qe = np.log(rng.uniform(2, 40, m)).astype(np.float32)
    qt = np.log(rng.uniform(2, 40, nt)).astype(np.float32)
    tgt = es[:, None] == ts[None, :]
    qmin = np.minimum(qe[:, None], qt[None, :]).astype(np.float64)
    s = rng.normal(0.0, 1.5, (m, nt)) + np.where(tgt, 1.0 + 1.2 * qmin, -2.0 + 0.6 * qmin)
    return es, ts, s.astype(np.float32), qe, qt
