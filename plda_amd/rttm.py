"""plda_amd/rttm.py -- RTTM files (NIST Rich Transcription Time Marked; the SPEAKER lines diarisation tools exchange) and the
step from reference turns to the per-segment labels plda_amd/der.py scores.  Pure Python / NumPy, no device.

    write(file, rec_ids, offsets, labels, start, dur, tick=0.01, labels2=None)   one SPEAKER line per maximal run of abutting
                                                                   segments of a speaker; labels2: a second speaker per segment
    read(file, tick=0.01)                                          {recording: [(start, dur, speaker)]}, times in ticks
    segment_labels(turns, seg_start, seg_dur)                      the reference speaker of every segment, by greatest overlap
    pack_turns(turns_by_recording, rec_ids)                        the packed turn arrays of der.der_timed, + sorted names
    pack_hyp(turns_by_recording, rec_ids)                          hypothesis turns cut into disjoint segments of at most two
                                                                   speakers: der.der_timed's seg_start, seg_dur, hyp, hyp2, offsets
    read_uem(file, tick=0.01)                                      {recording: [(start, dur)]} of a UEM file
    cut_windows(start, dur, offsets)                               overlapping sliding windows -> disjoint segments

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


def write(file, rec_ids, offsets, labels, start, dur, tick=0.01, labels2=None):
    """Write the segments of R recordings: recording r, named rec_ids[r], owns segments offsets[r] .. offsets[r+1] with
    labels[t] (-1: non-speech, not written), start[t] and dur[t] in ticks.  Consecutive segments of one label that abut
    (start + dur of one = start of the next) are one SPEAKER line; the speaker of label k is named "spk<k>".
    labels2 (None, or one entry per segment, -1: none) is a second speaker of the segment: the segment then contributes to
    both speakers' lines, abutting segments are merged per speaker, and a recording's lines come in order of their start
    (ties: the lower label).  With labels2=None the output is what it was without the argument."""
    offsets = np.asarray(offsets, np.int64)
    labels, start, dur = (np.asarray(a, np.int64) for a in (labels, start, dur))
    if len(rec_ids) != len(offsets) - 1:
        raise ValueError("rec_ids must name every recording")
    if not (labels.shape == start.shape == dur.shape == (int(offsets[-1]),)):
        raise ValueError("labels, start and dur must hold one entry per segment")
    if labels2 is not None:
        labels2 = np.asarray(labels2, np.int64)
        if labels2.shape != labels.shape:
            raise ValueError("labels2 must hold one entry per segment")
    nd = _decimals(tick)
    f, close = _open(file, "w")
    try:
        for r, rec in enumerate(rec_ids):
            if labels2 is not None:
                runs = {}                                # label -> [[start, end]], the segments in their given order
                for t in range(int(offsets[r]), int(offsets[r + 1])):
                    for k in {int(labels[t]), int(labels2[t])}:
                        if k < 0:
                            continue
                        mine = runs.setdefault(k, [])
                        if mine and mine[-1][1] == start[t]:
                            mine[-1][1] = int(start[t] + dur[t])
                        else:
                            mine.append([int(start[t]), int(start[t] + dur[t])])
                for s, k, e in sorted((s, k, e) for k, mine in runs.items() for s, e in mine):
                    f.write("SPEAKER %s 1 %.*f %.*f <NA> <NA> spk%d <NA> <NA>\n" % (rec, nd, s * tick, nd, (e - s) * tick, k))
                continue
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


def pack_turns(turns_by_recording, rec_ids):
    """The reference turns {recording: [(start, dur, speaker)]} (read's result) of the recordings rec_ids, packed for
    der.der_timed: ((turn_start, turn_dur, turn_spk int32, turn_off int64 [R + 1]), names) with names[r] the sorted speaker
    names of recording r (turn_spk indexes them).  Empty turns are dropped; turns of one speaker that overlap or abut become
    one turn; a recording absent from the dict has no turn.  More than 64 speakers in a recording: ValueError."""
    ts, td, tk, off, names_out = [], [], [], [0], []
    for rec in rec_ids:
        turns = [(int(s), int(d), k) for s, d, k in turns_by_recording.get(rec, ()) if int(d) > 0]
        names = sorted({k for _, _, k in turns})
        if len(names) > MAX_REF:
            raise ValueError("%s: %d reference speakers (at most %d)" % (rec, len(names), MAX_REF))
        for idx, name in enumerate(names):
            run = None                                   # [start, end]
            for s, d in sorted((s, d) for s, d, k in turns if k == name):
                if run is not None and s <= run[1]:
                    run[1] = max(run[1], s + d)
                    continue
                if run is not None:
                    ts.append(run[0]); td.append(run[1] - run[0]); tk.append(idx)
                run = [s, s + d]
            if run is not None:
                ts.append(run[0]); td.append(run[1] - run[0]); tk.append(idx)
        off.append(len(ts))
        names_out.append(names)
    return (np.asarray(ts, np.int32), np.asarray(td, np.int32), np.asarray(tk, np.int32), np.asarray(off, np.int64)), names_out


def pack_hyp(turns_by_recording, rec_ids):
    """Hypothesis turns {recording: [(start, dur, speaker)]} (read's result; they may overlap across speakers) of the
    recordings rec_ids, cut into disjoint segments for der.der_timed(..., hyp2=): (seg_start, seg_dur, hyp, hyp2 int32 [T],
    offsets int64 [R + 1]); hyp and hyp2 index the sorted speaker names of their recording.  A segment is a stretch between two
    consecutive turn boundaries with one or two speakers talking; the lower label is hyp, hyp2 = -1 with one speaker.  Empty
    turns are dropped; turns of one speaker that overlap count once.
    A recording with no speech gets one empty segment (hyp = -1): der.der_timed takes no recording without a segment.  A
    stretch with three or more simultaneous speakers: ValueError, naming the recording and the tick."""
    ss, sd, h1, h2, off = [], [], [], [], [0]
    for rec in rec_ids:
        turns = [(int(s), int(d), k) for s, d, k in turns_by_recording.get(rec, ()) if int(d) > 0]
        names = sorted({k for _, _, k in turns})
        index = {k: i for i, k in enumerate(names)}
        bounds = sorted({b for s, d, _ in turns for b in (s, s + d)})
        n0 = len(ss)
        for a, b in zip(bounds[:-1], bounds[1:]):
            talk = sorted({index[k] for s, d, k in turns if s <= a and b <= s + d})
            if len(talk) > 2:
                raise ValueError("%s: %d hypothesis speakers at tick %d (at most 2)" % (rec, len(talk), a))
            if talk:
                ss.append(a); sd.append(b - a); h1.append(talk[0]); h2.append(talk[1] if len(talk) > 1 else -1)
        if len(ss) == n0:
            ss.append(0); sd.append(0); h1.append(-1); h2.append(-1)
        off.append(len(ss))
    i32 = lambda a: np.asarray(a, np.int32)
    return i32(ss), i32(sd), i32(h1), i32(h2), np.asarray(off, np.int64)


def read_uem(file, tick=0.01):
    """{recording: [(start, dur)]} of a UEM file ("<recording> <channel> <start> <end>" per line, seconds; lines that are
    empty or start with ';' or '#' are skipped), in file order, times rounded to integer ticks; an interval that ends before
    it starts is an error."""
    out = {}
    f, close = _open(file, "r")
    try:
        for line in f:
            p = line.split()
            if not p or p[0][0] in ";#":
                continue
            if len(p) < 4:
                raise ValueError("short UEM line: %r" % line)
            a, b = int(round(float(p[2]) / tick)), int(round(float(p[3]) / tick))
            if b < a:
                raise ValueError("UEM interval ends before it starts: %r" % line)
            out.setdefault(p[0], []).append((a, b - a))
    finally:
        if close:
            f.close()
    return out


def pack_uem(uem_by_recording, rec_ids):
    """(uem_start, uem_dur int32, uem_off int64 [R + 1]) of read_uem's result for the recordings rec_ids (a recording absent
    from the dict gets no interval: nothing of it is scored)."""
    us, ud, off = [], [], [0]
    for rec in rec_ids:
        for s, d in uem_by_recording.get(rec, ()):
            us.append(int(s)); ud.append(int(d))
        off.append(len(us))
    return np.asarray(us, np.int32), np.asarray(ud, np.int32), np.asarray(off, np.int64)


def cut_windows(start, dur, offsets):
    """Overlapping sliding windows -> disjoint segments, the rule of Kaldi's make_rttm.py: where window t + 1 of a recording
    starts before window t ends, both are cut at the midpoint of the overlap; an odd overlap gives the extra tick to the
    earlier window.  The windows of a recording (offsets[r] .. offsets[r+1]) must be in time order (starts and ends ascending).
    Returns (start, dur) int32 [T]."""
    offsets = np.asarray(offsets, np.int64)
    start, dur = np.asarray(start, np.int64), np.asarray(dur, np.int64)
    if not (start.shape == dur.shape == (int(offsets[-1]),)):
        raise ValueError("start and dur must hold one entry per window")
    lo, hi = start.copy(), start + dur
    for r in range(len(offsets) - 1):
        a, b = int(offsets[r]), int(offsets[r + 1])
        if (np.diff(start[a:b]) < 0).any() or (np.diff(hi[a:b]) < 0).any() or (dur[a:b] < 0).any():
            raise ValueError("the windows of recording %d are not in time order" % r)
        for t in range(a, b - 1):
            ov = int(hi[t] - lo[t + 1])
            if ov > 0:
                cut = int(lo[t + 1]) + (ov + 1) // 2
                hi[t] = cut
                lo[t + 1] = cut
    if (hi < lo).any():
        raise ValueError("a window lies inside its neighbours' overlap")
    return lo.astype(np.int32), (hi - lo).astype(np.int32)
