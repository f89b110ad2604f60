"""plda_amd/rttm.py -- RTTM files (NIST Rich Transcription Time Marked; the SPEAKER lines diarisation tools exchange) and the
step from reference turns to the per-segment labels plda_amd/der.py scores.  Pure Python / NumPy, no device.

    write(file, rec_ids, offsets, labels, start, dur, tick=0.01)   one SPEAKER line per maximal run of abutting segments
    read(file, tick=0.01)                                          {recording: [(start, dur, speaker)]}, times in ticks
    segment_labels(turns, seg_start, seg_dur)                      the reference speaker of every segment, by greatest overlap

Times are integer ticks of `tick` seconds (0.01 s by default), so that a file written here reads back exactly.
"""
import numpy as np

MAX_REF = 64            # PLDA_DER_MAX_REF


def _open(file, mode):
    return (open(file, mode), True) if isinstance(file, (str, bytes)) or hasattr(file, "__fspath__") else (file, False)


def _decimals(tick):
    d = 0
    while d < 9 and abs(round(tick * 10 ** d) - tick * 10 ** d) > 1e-9:
        d += 1
    return d


def write(file, rec_ids, offsets, labels, start, dur, tick=0.01):
    """Write the segments of R recordings: recording r, named rec_ids[r], owns segments offsets[r] .. offsets[r+1] with
    labels[t] (-1: non-speech, not written), start[t] and dur[t] in ticks.  Consecutive segments of one label that abut
    (start + dur of one = start of the next) are one SPEAKER line; the speaker of label k is named "spk<k>"."""
    offsets = np.asarray(offsets, np.int64)
    labels, start, dur = (np.asarray(a, np.int64) for a in (labels, start, dur))
    if len(rec_ids) != len(offsets) - 1:
        raise ValueError("rec_ids must name every recording")
    if not (labels.shape == start.shape == dur.shape == (int(offsets[-1]),)):
        raise ValueError("labels, start and dur must hold one entry per segment")
    nd = _decimals(tick)
    f, close = _open(file, "w")
    try:
        for r, rec in enumerate(rec_ids):
            run = None                                   # [label, start, end]
            for t in list(range(int(offsets[r]), int(offsets[r + 1]))) + [None]:
                if t is not None and run is not None and labels[t] == run[0] and start[t] == run[2]:
                    run[2] = int(start[t] + dur[t])
                    continue
                if run is not None and run[0] >= 0:
                    f.write("SPEAKER %s 1 %.*f %.*f <NA> <NA> spk%d <NA> <NA>\n"
                            % (rec, nd, run[1] * tick, nd, (run[2] - run[1]) * tick, run[0]))
                run = None if t is None else [int(labels[t]), int(start[t]), int(start[t] + dur[t])]
    finally:
        if close:
            f.close()


def read(file, tick=0.01):
    """{recording: [(start, dur, speaker)]} of the SPEAKER lines of an RTTM file, in file order; start and dur rounded to
    integer ticks."""
    out = {}
    f, close = _open(file, "r")
    try:
        for line in f:
            p = line.split()
            if not p or p[0] != "SPEAKER":
                continue
            if len(p) < 8:
                raise ValueError("short SPEAKER line: %r" % line)
            out.setdefault(p[1], []).append((int(round(float(p[3]) / tick)), int(round(float(p[4]) / tick)), p[7]))
    finally:
        if close:
            f.close()
    return out


def segment_labels(turns, seg_start, seg_dur):
    """The reference label of every segment [seg_start[t], seg_start[t] + seg_dur[t]) of ONE recording from its reference
    turns [(start, dur, speaker)]: the speaker whose turns overlap the segment longest; ties go to the first speaker in
    sorted name order; no overlap gives -1.  Returns (labels int32 [T] in [-1, 64), names): label k is names[k], the
    sorted speaker names."""
    names = sorted({s for _, _, s in turns})
    if len(names) > MAX_REF:
        raise ValueError("%d reference speakers (at most %d)" % (len(names), MAX_REF))
    index = {s: k for k, s in enumerate(names)}
    seg_start, seg_dur = np.asarray(seg_start, np.int64), np.asarray(seg_dur, np.int64)
    if seg_start.shape != seg_dur.shape or seg_start.ndim != 1:
        raise ValueError("seg_start and seg_dur must be 1-D arrays of one length")
    seg_end = seg_start + seg_dur
    ov = np.zeros((max(len(names), 1), len(seg_start)), np.int64)
    for st, du, s in turns:
        ov[index[s]] += np.clip(np.minimum(seg_end, st + du) - np.maximum(seg_start, st), 0, None)
    labels = np.argmax(ov, 0).astype(np.int32)           # (the first maximum: the first name in sorted order)
    labels[ov.max(0) <= 0] = -1
    return labels, names
