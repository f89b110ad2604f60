"""plda_amd/der.py -- diarisation error rate on the device (csrc/der.hip; include/plda_hip.h, "diarisation error rate"):
segment-level miss, false alarm and speaker confusion under the optimal one-to-one mapping of reference to hypothesis
speakers, and the sweep of ONE full AHC merge record over Q thresholds.

    der(engine, ref, hyp, offsets, dur=None)              counts [R, 4], per-recording and pooled DER[, the speaker map]
    sweep(engine, merges, offsets, ref, thresholds, ...)  counts [Q, R, 4], n_clusters [Q, R], pooled DER [Q], the best q
    plan(engine, sr, sh)                                  the dispatch class of a recording of sr x sh speakers
    MPlda.der / MPlda.tune_threshold                      the same from an engine; tune_threshold clusters once, then sweeps

Labels: ref in [-1, 64), hyp in [-1, 4096), -1 = non-speech; dur int32 >= 0 in ticks (None: 1 everywhere).  Everything on the
device is an integer and the counts are exact; the divisions are done here, the pooled ones from Python ints.

The Jaccard error rate (include/plda_hip.h, "Jaccard error rate and per-speaker figures") comes from the same calls with
jer=True: der, der_timed return a DerResult that also carries jer, jer_counts, jer_map and speakers; sweep, sweep_timed a
SweepResult with jer_counts, jer and best_jer.  jer_rates(jer_counts) and pooled_jer(jer_counts) are the divisions.

The time-based form (csrc/der_time.hip; include/plda_hip.h, "time-based diarisation error rate") scores TIME, with overlapped
reference speech, a collar and UEM regions -- md-eval's definition on integer ticks:

    der_timed(engine, turns, seg_start, seg_dur, hyp, offsets, collar=0, uem=None, skip_overlap=False, hyp2=None)   a DerResult
    sweep_timed(engine, merges, turns, seg_start, seg_dur, offsets, thresholds, ...)                     a SweepResult
    plan_timed(engine, n_turns, n_seg, n_uem=0, collar=0)                                                the event-sort class

turns = (turn_start, turn_dur, turn_spk, turn_off), what rttm.pack_turns returns first; uem = (uem_start, uem_dur, uem_off).
hyp2 int [T] (K21) is the second hypothesis speaker of every segment, -1 = none: a segment then carries up to two labels
(diarize.vbx(..., return_second=True) and diarize.apply_overlap make one; rttm.pack_hyp cuts one from RTTM turns).
"""
import ctypes as C

import numpy as np

from . import _native as N
from . import diarize

MAX_REF = 64            # PLDA_DER_MAX_REF
MAX_HYP = diarize.AHC_MAX
MAX_TURNS = 16384       # PLDA_DER_MAX_TURNS
MAX_UEM = 1024          # PLDA_DER_MAX_UEM
MAX_TIME = 1 << 30
MAX_COLLAR = 1 << 20
SKIP_OVERLAP = 1        # PLDA_DER_SKIP_OVERLAP

_p = diarize._p


class DerResult:
    """counts int64 [R, 4] = {speech, miss, fa, confusion}; der float64 [R] (NaN where speech = 0); total = the pooled
    sum of errors / sum of speech (NaN when there is no speech); map int32 [R, 64] or None.
    With jer=True also: jer_counts int64 [R, 2] = {n_ref, jsum}; jer float64 [R] (NaN where n_ref = 0); jer_total, pooled
    over all reference speakers; jer_map int32 [R, 64]; speakers, per recording a list of (ref_label, hyp_label or -1,
    ref_ticks, intersect, union, jer) for every reference speaker that counts, ascending by ref_label.  Otherwise None."""

    def __init__(self, counts, map_=None, jer_counts=None, jer_map=None, spk=None):
        self.counts = counts
        self.map = map_
        self.der = rates(counts)
        self.total = pooled(counts)
        self.jer_counts = jer_counts
        self.jer_map = jer_map
        self.jer = jer_rates(jer_counts) if jer_counts is not None else None
        self.jer_total = pooled_jer(jer_counts) if jer_counts is not None else None
        self.speakers = _speakers(jer_map, spk) if spk is not None else None

    def __repr__(self):
        return "DerResult(total=%r, recordings=%d)" % (self.total, len(self.counts))


class SweepResult:
    """counts int64 [Q, R, 4]; n_clusters int32 [Q, R]; der float64 [Q], pooled over the recordings; best = the index of the
    lowest pooled DER (ties: the lowest index; NaN never wins); thresholds float64 [Q].
    With jer=True also: jer_counts int64 [Q, R, 2]; jer float64 [Q], pooled; best_jer = the index of the lowest pooled JER
    (the same tie rule).  Otherwise None."""

    def __init__(self, thresholds, counts, n_clusters, jer_counts=None):
        self.thresholds = thresholds
        self.counts = counts
        self.n_clusters = n_clusters
        self.der = np.asarray([pooled(c) for c in counts], np.float64)
        self.best = best_index(counts)
        self.jer_counts = jer_counts
        self.jer = np.asarray([pooled_jer(c) for c in jer_counts], np.float64) if jer_counts is not None else None
        self.best_jer = best_jer_index(jer_counts) if jer_counts is not None else None

    def __repr__(self):
        return "SweepResult(best=%d, threshold=%r, der=%r)" % (self.best, float(self.thresholds[self.best]), float(self.der[self.best]))


def rates(counts):
    """(miss + fa + confusion) / speech of every row of counts [..., 4]; NaN where speech = 0."""
    c = np.asarray(counts, np.int64)
    err = (c[..., 1] + c[..., 2] + c[..., 3]).astype(np.float64)
    sp = c[..., 0].astype(np.float64)
    out = np.full(err.shape, np.nan)
    np.divide(err, sp, out=out, where=sp > 0)
    return out


def _sums(counts):
    c = np.asarray(counts, np.int64).reshape(-1, 4)
    speech = sum(int(v) for v in c[:, 0])
    err = sum(int(v) for v in c[:, 1:].ravel())
    return err, speech


def pooled(counts):
    """sum of errors / sum of speech over counts [R, 4], from Python ints; NaN when there is no speech."""
    err, speech = _sums(counts)
    return err / speech if speech > 0 else float("nan")


def best_index(counts):
    """argmin over q of the pooled DER of counts [Q, R, 4], compared as exact fractions; ties go to the lowest q."""
    best, be, bs = 0, None, None
    for q, c in enumerate(counts):
        err, speech = _sums(c)
        if speech <= 0:
            continue
        if be is None or err * bs < be * speech:         # err / speech < be / bs
            best, be, bs = q, err, speech
    return best


JER_ONE = 1 << 32       # the weight of a Jaccard index of 1


def jer_rates(jer_counts):
    """1 - jsum / (n_ref 2^32) of every row of jer_counts [..., 2]; NaN where n_ref = 0."""
    c = np.asarray(jer_counts, np.int64)
    out = np.full(c.shape[:-1], np.nan)
    for idx in np.ndindex(*c.shape[:-1]):
        n, js = int(c[idx + (0,)]), int(c[idx + (1,)])
        if n > 0:
            out[idx] = (n * JER_ONE - js) / (n * JER_ONE)
    return out


def _jer_sums(jer_counts):
    c = np.asarray(jer_counts, np.int64).reshape(-1, 2)
    return sum(int(v) for v in c[:, 0]), sum(int(v) for v in c[:, 1])


def pooled_jer(jer_counts):
    """1 - sum jsum / (2^32 sum n_ref) over jer_counts [R, 2], from Python ints: the mean over all reference speakers of all
    recordings (a recording with n_ref = 0 adds nothing); NaN when there is no reference speaker."""
    n, js = _jer_sums(jer_counts)
    return (n * JER_ONE - js) / (n * JER_ONE) if n > 0 else float("nan")


def best_jer_index(jer_counts):
    """argmin over q of the pooled JER of jer_counts [Q, R, 2], compared as exact fractions; ties go to the lowest q."""
    best, bj, bn = 0, None, None
    for q, c in enumerate(jer_counts):
        n, js = _jer_sums(c)
        if n <= 0:
            continue
        if bj is None or js * bn > bj * n:               # js / n > bj / bn: a larger mean index is a smaller JER
            best, bj, bn = q, js, n
    return best


def _speakers(jer_map, spk):
    out = []
    for r in range(len(spk)):
        rows = []
        for i in np.flatnonzero(spk[r, :, 0] > 0):
            rt, inter, union = (int(v) for v in spk[r, i])
            rows.append((int(i), int(jer_map[r, i]), rt, inter, union, 1.0 - inter / union))
        out.append(rows)
    return out


def _jer_out(r, q=None):
    """The buffers of a JER call: (jer_counts, jer_map, spk); a sweep (q given) has jer_counts [Q, R, 2] alone."""
    if q is not None:
        return np.empty((q, r, 2), np.int64), None, None
    return np.empty((r, 2), np.int64), np.empty((r, MAX_REF), np.int32), np.empty((r, MAX_REF, 3), np.int64)


def _call(engine, name, args):
    """The one library call of a DER function: entry point `name` on args, arrays (None: NULL) as pointers."""
    N.check(engine._h, getattr(engine._lib, name)(engine._h, *[a if isinstance(a, int) else _p(a) for a in args]))


def plan(engine, sr, sh):
    """{"cls": 0 (matrix in LDS) or 1 (in handle scratch), "scratch_bytes": per recording, "lds_max": the widest matrix,
    max(sr, sh), of the LDS class at this sr}."""
    out = (C.c_int32 * 3)()
    N.check(engine._h, engine._lib.plda_der_plan(engine._h, int(sr), int(sh), out))
    return {"cls": int(out[0]), "scratch_bytes": int(out[1]), "lds_max": int(out[2])}


def _jer_ticks(dur, offsets):
    """The segment forms of the JER calls: the durations of a recording add up to at most 2^30 (dur None: its segment count)."""
    if dur is not None and (np.add.reduceat(dur.astype(np.int64), offsets[:-1]) > MAX_TIME).any():
        raise ValueError("with jer=True the durations of a recording must add up to at most 2^30")


def plan_jer(engine, sr, sh):
    """plan() under the LDS accounting of the JER form (plda_der_jer_plan)."""
    out = (C.c_int32 * 3)()
    N.check(engine._h, engine._lib.plda_der_jer_plan(engine._h, int(sr), int(sh), out))
    return {"cls": int(out[0]), "scratch_bytes": int(out[1]), "lds_max": int(out[2])}


def _offsets(offsets):
    offsets = np.ascontiguousarray(offsets, np.int64)
    if offsets.ndim != 1 or len(offsets) < 2:
        raise ValueError("offsets must hold R + 1 >= 2 entries")
    if offsets[0] != 0:
        raise ValueError("offsets must start at 0")
    sizes = np.diff(offsets)
    if (sizes < 1).any() or (sizes > MAX_HYP).any():
        raise ValueError("every recording must hold 1 ... %d segments (offsets must ascend)" % MAX_HYP)
    return offsets


def _labels(a, t, name, limit):
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        raise ValueError("%s must be an integer array" % name)
    if a.shape != (t,):
        raise ValueError("%s must hold one entry per segment (%d), got %r" % (name, t, a.shape))
    if a.size and (a.min() < -1 or a.max() >= limit):
        raise ValueError("%s must lie in [-1, %d)" % (name, limit))
    return np.ascontiguousarray(a, np.int32)


def _dur(dur, t):
    if dur is None:
        return None
    d = np.asarray(dur)
    if d.dtype.kind not in "iu":
        raise ValueError("dur must be an integer array of ticks")
    if d.shape != (t,):
        raise ValueError("dur must hold one entry per segment (%d), got %r" % (t, d.shape))
    if d.size and (d.min() < 0 or d.max() > 0x7fffffff):
        raise ValueError("dur must lie in [0, 2^31)")
    return np.ascontiguousarray(d, np.int32)


def der_args(ref, hyp, offsets, dur):
    """The argument check of der / MPlda.der, before any device work -> (ref, hyp, offsets, dur).  ValueError on anything the
    C ABI would answer with PLDA_E_INVAL."""
    offsets = _offsets(offsets)
    t = int(offsets[-1])
    return _labels(ref, t, "ref", MAX_REF), _labels(hyp, t, "hyp", MAX_HYP), offsets, _dur(dur, t)


def sweep_args(merges, offsets, ref, thresholds, dur, num_speakers):
    """The argument check of sweep -> (merge_a, merge_b, merge_cost, offsets, ref, thresholds, dur, min_clusters)."""
    offsets = _offsets(offsets)
    r, t = len(offsets) - 1, int(offsets[-1])
    if len(merges) != 3:
        raise ValueError("merges must be (merge_a, merge_b, merge_cost)")
    ma, mb = (np.ascontiguousarray(a, np.int32) for a in merges[:2])
    mc = np.ascontiguousarray(merges[2], np.float64)
    for a, name in ((ma, "merge_a"), (mb, "merge_b"), (mc, "merge_cost")):
        if a.shape != (t - r,):
            raise ValueError("%s must hold T - R = %d entries, got %r" % (name, t - r, a.shape))
    thresholds = np.ascontiguousarray(thresholds, np.float64)
    if thresholds.ndim != 1 or len(thresholds) < 1:
        raise ValueError("thresholds must hold Q >= 1 entries")
    if np.isnan(thresholds).any():
        raise ValueError("thresholds must not hold NaN")
    _, _, minc = diarize.stop_args(offsets, 0.0, num_speakers)
    if minc is not None and (minc < 1).any():
        raise ValueError("num_speakers must be >= 1")
    return ma, mb, mc, offsets, _labels(ref, t, "ref", MAX_REF), thresholds, _dur(dur, t), minc


def der(engine, ref, hyp, offsets, dur=None, return_map=False, jer=False):
    """Score R recordings: ref, hyp int [T] (-1 = non-speech), recording r owning segments offsets[r] .. offsets[r+1], dur
    int [T] ticks (None: 1).  jer=True: the Jaccard error rate and the per-speaker figures from the same call (the durations
    of a recording then add up to at most 2^30).  Returns a DerResult."""
    ref, hyp, offsets, dur = der_args(ref, hyp, offsets, dur)
    r = len(offsets) - 1
    counts = np.empty((r, 4), np.int64)
    map_ = np.empty((r, MAX_REF), np.int32) if return_map else None
    if jer:
        _jer_ticks(dur, offsets)
    jout = _jer_out(r) if jer else ()
    _call(engine, "plda_der_jer" if jer else "plda_der", [ref, hyp, dur, offsets, r, counts, map_] + list(jout))
    return DerResult(counts, map_, *jout)


def sweep(engine, merges, offsets, ref, thresholds, dur=None, num_speakers=None, jer=False):
    """Score the clusterings that a FULL merge record (diarize.ahc / MPlda.cluster with threshold=None, num_speakers=1,
    return_merges=True) yields at every one of `thresholds`, with at least `num_speakers` clusters left (None: 1): what
    diarize.cut at that threshold followed by der returns, for all Q in one device run.  Returns a SweepResult."""
    ma, mb, mc, offsets, ref, thresholds, dur, minc = sweep_args(merges, offsets, ref, thresholds, dur, num_speakers)
    r, q = len(offsets) - 1, len(thresholds)
    counts, ncl = np.empty((q, r, 4), np.int64), np.empty((q, r), np.int32)
    if jer:
        _jer_ticks(dur, offsets)
    jout = _jer_out(r, q)[:1] if jer else ()
    _call(engine, "plda_der_jer_sweep" if jer else "plda_der_sweep",
          [ma, mb, mc, offsets, r, ref, dur, thresholds, q, minc, counts, ncl] + list(jout))
    return SweepResult(thresholds, counts, ncl, *jout)


# ------------------------------------------------------------------------------------------- the time-based form
def _counted(off, r, name, limit):
    off = np.ascontiguousarray(off, np.int64)
    if off.shape != (r + 1,):
        raise ValueError("%s must hold R + 1 = %d entries, got %r" % (name, r + 1, off.shape))
    if off[0] != 0:
        raise ValueError("%s must start at 0" % name)
    sizes = np.diff(off)
    if (sizes < 0).any() or (sizes > limit).any():
        raise ValueError("every recording must hold 0 ... %d entries of %s (it must ascend)" % (limit, name))
    return off


def _times(start, dur, n, name):
    out = []
    for a, what in ((start, "start"), (dur, "dur")):
        a = np.asarray(a)
        if a.dtype.kind not in "iu":
            raise ValueError("%s_%s must be an integer array of ticks" % (name, what))
        if a.shape != (n,):
            raise ValueError("%s_%s must hold %d entries, got %r" % (name, what, n, a.shape))
        out.append(a.astype(np.int64))
    if n and (out[0].min() < 0 or out[1].min() < 0 or (out[0] + out[1]).max() > MAX_TIME):
        raise ValueError("%s times must satisfy 0 <= start, 0 <= dur, start + dur <= 2^30" % name)
    return np.ascontiguousarray(out[0], np.int32), np.ascontiguousarray(out[1], np.int32)


def _second(hyp, hyp2, t):
    """hyp2 int32 [T] checked against hyp: in [-1, MAX_HYP), and a second label needs a first one and differs from it."""
    hyp2 = _labels(hyp2, t, "hyp2", MAX_HYP)
    hyp = _labels(hyp, t, "hyp", MAX_HYP)
    if ((hyp2 >= 0) & (hyp < 0)).any():
        raise ValueError("hyp2 >= 0 needs hyp >= 0: a second speaker without a first")
    if ((hyp2 >= 0) & (hyp2 == hyp)).any():
        raise ValueError("hyp2 must differ from hyp where it is >= 0")
    return hyp2


def timed_args(turns, seg_start, seg_dur, offsets, collar, uem, skip_overlap, hyp=None, hyp2=None):
    """The argument check shared by der_timed and sweep_timed, before any device work ->
    (turn_start, turn_dur, turn_spk, turn_off, seg_start, seg_dur, offsets, uem_start, uem_dur, uem_off, collar, flags); the
    three uem entries are None without a UEM.  Disjointness (same-speaker turns, segments) is the device's check.  With hyp2
    (and hyp) the tuple is followed by hyp2 as int32 [T]: its shape, dtype and range, hyp2 >= 0 only where hyp >= 0, hyp2 != hyp."""
    if hyp2 is not None:
        if hyp is None:
            raise ValueError("hyp2 needs hyp")
        base = timed_args(turns, seg_start, seg_dur, offsets, collar, uem, skip_overlap)
        return base + (_second(hyp, hyp2, int(base[6][-1])),)
    offsets = _offsets(offsets)
    r, t = len(offsets) - 1, int(offsets[-1])
    if turns is None or len(turns) != 4:
        raise ValueError("turns must be (turn_start, turn_dur, turn_spk, turn_off)")
    toff = _counted(turns[3], r, "turn_off", MAX_TURNS)
    ts, td = _times(turns[0], turns[1], int(toff[-1]), "turn")
    tk = _labels(turns[2], int(toff[-1]), "turn_spk", MAX_REF)
    if tk.size and tk.min() < 0:
        raise ValueError("turn_spk must lie in [0, %d)" % MAX_REF)
    ss, sd = _times(seg_start, seg_dur, t, "seg")
    us = ud = uoff = None
    if uem is not None:
        if len(uem) != 3:
            raise ValueError("uem must be (uem_start, uem_dur, uem_off)")
        uoff = _counted(uem[2], r, "uem_off", MAX_UEM)
        us, ud = _times(uem[0], uem[1], int(uoff[-1]), "uem")
    if isinstance(collar, bool) or not isinstance(collar, (int, np.integer)) or not 0 <= collar <= MAX_COLLAR:
        raise ValueError("collar must be an integer number of ticks in [0, 2^20]")
    return ts, td, tk, toff, ss, sd, offsets, us, ud, uoff, int(collar), SKIP_OVERLAP if skip_overlap else 0


def plan_timed(engine, n_turns, n_seg, n_uem=0, collar=0):
    """{"cls": 0 (events sorted in LDS) or 1 (in handle scratch), "scratch_bytes": per recording, "lds_max": the largest
    event-slot count of the LDS class, "events": the event slots of this recording}."""
    out = (C.c_int32 * 3)()
    N.check(engine._h, engine._lib.plda_der_timed_plan(engine._h, int(n_turns), int(n_seg), int(n_uem), int(collar), out))
    return {"cls": int(out[0]), "scratch_bytes": int(out[1]), "lds_max": int(out[2]),
            "events": (6 if collar > 0 else 2) * int(n_turns) + 2 * int(n_seg) + 2 * int(n_uem)}


def der_timed(engine, turns, seg_start, seg_dur, hyp, offsets, collar=0, uem=None, skip_overlap=False, return_map=False, hyp2=None,
              jer=False):
    """Time-based DER of R recordings: reference turns (they may overlap across speakers), disjoint hypothesis segments
    seg_start, seg_dur, hyp int [T] (-1 = non-speech), recording r owning segments offsets[r] .. offsets[r+1]; collar in
    ticks; uem the scored regions or None; skip_overlap: md-eval's -1; hyp2 int [T] or None: the second speaker of every
    segment (-1 = none; plda_der_timed_ovl).  Returns a DerResult."""
    targs = timed_args(turns, seg_start, seg_dur, offsets, collar, uem, skip_overlap, hyp, hyp2)
    ts, td, tk, toff, ss, sd, offsets, us, ud, uoff, collar, flags = targs[:12]
    hyp = _labels(hyp, int(offsets[-1]), "hyp", MAX_HYP)
    r = len(offsets) - 1
    counts = np.empty((r, 4), np.int64)
    map_ = np.empty((r, MAX_REF), np.int32) if return_map else None
    jout = _jer_out(r) if jer else ()
    # the two-label entry points take hyp2 behind hyp; the JER one also where there is none (NULL), plda_der_timed has no such argument
    second = [targs[12] if hyp2 is not None else None] if jer or hyp2 is not None else []
    _call(engine, "plda_der_timed_jer" if jer else "plda_der_timed_ovl" if hyp2 is not None else "plda_der_timed",
          [ts, td, tk, toff, ss, sd, hyp] + second + [offsets, r, us, ud, uoff, collar, flags, counts, map_] + list(jout))
    return DerResult(counts, map_, *jout)


def sweep_timed_args(merges, turns, seg_start, seg_dur, offsets, thresholds, num_speakers, collar, uem, skip_overlap):
    """The argument check of sweep_timed -> (merge_a, merge_b, merge_cost, thresholds, min_clusters) + timed_args' tuple."""
    targs = timed_args(turns, seg_start, seg_dur, offsets, collar, uem, skip_overlap)
    ref = np.zeros(int(targs[6][-1]), np.int32)
    ma, mb, mc, _, _, thresholds, _, minc = sweep_args(merges, targs[6], ref, thresholds, None, num_speakers)
    return (ma, mb, mc, thresholds, minc) + targs


def sweep_timed(engine, merges, turns, seg_start, seg_dur, offsets, thresholds, num_speakers=None, collar=0, uem=None,
                skip_overlap=False, jer=False):
    """sweep() on time: the clusterings a FULL merge record yields at every threshold, each scored as der_timed scores the
    labels of diarize.cut at that threshold.  The time line is cut once per recording.  Returns a SweepResult."""
    ma, mb, mc, thresholds, minc, ts, td, tk, toff, ss, sd, offsets, us, ud, uoff, collar, flags = sweep_timed_args(
        merges, turns, seg_start, seg_dur, offsets, thresholds, num_speakers, collar, uem, skip_overlap)
    r, q = len(offsets) - 1, len(thresholds)
    counts, ncl = np.empty((q, r, 4), np.int64), np.empty((q, r), np.int32)
    jout = _jer_out(r, q)[:1] if jer else ()
    _call(engine, "plda_der_timed_jer_sweep" if jer else "plda_der_timed_sweep",
          [ma, mb, mc, ts, td, tk, toff, ss, sd, offsets, r, us, ud, uoff, collar, flags, thresholds, q, minc, counts, ncl] + list(jout))
    return SweepResult(thresholds, counts, ncl, *jout)
