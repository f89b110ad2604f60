"""The host models of the time-based diarisation error rate (include/plda_hip.h, "time-based diarisation error rate";
csrc/der_time.hip), and seeded generators of input that is valid by construction.

    score_ticks   the definition, tick by tick, in Python ints: every tick from min - collar to max + collar is looked at
    score_atoms   the same by intervals (np.unique of the boundaries, +-1 prefix sums), for recordings too long to walk

A recording is a dict: ts, td, tk (reference turns: start, dur, speaker), ss, sd (hypothesis segments), hyp (their labels,
-1 = non-speech), us, ud (UEM intervals) or None for both.  Both models return ([speech, miss, fa, confusion], C, ref labels,
hyp labels) with C the matrix of Python ints over the labels of the whole recording (rows: the reference speakers of any turn
with dur > 0; columns: the hypothesis labels >= 0 of any segment), sorted.  The optimum comes
from der_model.assign."""
import numpy as np

import der_model as M

MAX_REF = 64
SKIP_OVERLAP = 1


def rec(ts=(), td=(), tk=(), ss=(), sd=(), hyp=(), us=None, ud=None):
    i32 = lambda a: np.asarray(a, np.int32).reshape(-1)
    return {"ts": i32(ts), "td": i32(td), "tk": i32(tk), "ss": i32(ss), "sd": i32(sd), "hyp": i32(hyp),
            "us": None if us is None else i32(us), "ud": None if us is None else i32(ud)}


def _labels(r):
    rl = sorted({int(k) for k, d in zip(r["tk"], r["td"]) if d > 0})
    hl = sorted({int(b) for b in r["hyp"] if b >= 0})
    return rl, hl


def _finish(C, rl, hl, speech, miss, fa, both, assign=None):
    correct, _ = (assign or M.assign)(C)
    return [speech, miss, fa, both - correct], C, rl, hl


def score_ticks(r, collar=0, skip_overlap=False):
    """The definition, one tick at a time."""
    rl, hl = _labels(r)
    ri, hi = {v: k for k, v in enumerate(rl)}, {v: k for k, v in enumerate(hl)}
    C = np.zeros((len(rl), len(hl)), object)
    C[...] = 0
    ends = [int(s) + int(d) for s, d in zip(r["ts"], r["td"])] + [int(s) + int(d) for s, d in zip(r["ss"], r["sd"])]
    starts = [int(s) for s in r["ts"]] + [int(s) for s in r["ss"]]
    if r["us"] is not None:
        starts += [int(s) for s in r["us"]]
        ends += [int(s) + int(d) for s, d in zip(r["us"], r["ud"])]
    if not starts:
        return _finish(C, rl, hl, 0, 0, 0, 0)
    t0, t1 = min(starts) - collar, max(ends) + collar
    n = t1 - t0
    ref = [set() for _ in range(n)]
    hyp = [[] for _ in range(n)]
    out = [False] * n                                   # inside a collar zone
    inside = [r["us"] is None] * n                      # inside the UEM
    for s, d, k in zip(r["ts"].tolist(), r["td"].tolist(), r["tk"].tolist()):
        if d == 0:
            continue
        for t in range(s, s + d):
            assert k not in ref[t - t0], "generator: same-speaker turns overlap"
            ref[t - t0].add(k)
        for b in (s, s + d):
            for t in range(b - collar, b + collar):
                out[t - t0] = True
    for s, d, b in zip(r["ss"].tolist(), r["sd"].tolist(), r["hyp"].tolist()):
        for t in range(s, s + d):
            hyp[t - t0].append(b)
    if r["us"] is not None:
        for s, d in zip(r["us"].tolist(), r["ud"].tolist()):
            for t in range(s, s + d):
                inside[t - t0] = True
    speech = miss = fa = both = 0
    for t in range(n):
        assert len(hyp[t]) <= 1, "generator: hypothesis segments overlap"
        if out[t] or not inside[t]:
            continue
        nref = len(ref[t])
        if skip_overlap and nref > 1:
            continue
        j = hyp[t][0] if hyp[t] else -1
        nhyp = 1 if j >= 0 else 0
        speech += nref
        miss += max(0, nref - nhyp)
        fa += max(0, nhyp - nref)
        both += min(nref, nhyp)
        if nhyp:
            for i in ref[t]:
                C[ri[i], hi[j]] += 1
    return _finish(C, rl, hl, speech, miss, fa, both)


def score_atoms(r, collar=0, skip_overlap=False, assign=None):
    """The same by intervals: the boundaries cut the time line into atoms, depths are prefix sums of +-1 at the boundaries.
    assign: another solver in place of der_model.assign (scripts/der_time_bench.py times scipy's)."""
    rl, hl = _labels(r)
    ts, td, tk = (r[k].astype(np.int64) for k in ("ts", "td", "tk"))
    ss, sd, hyp = (r[k].astype(np.int64) for k in ("ss", "sd", "hyp"))
    keep = td > 0
    ts, td, tk = ts[keep], td[keep], tk[keep]
    keep = sd > 0
    ss, sd, hyp = ss[keep], sd[keep], hyp[keep]
    zs = np.concatenate([ts - collar, ts + td - collar]) if collar > 0 else np.zeros(0, np.int64)
    ze = zs + 2 * collar
    has_uem = r["us"] is not None
    us = r["us"].astype(np.int64) if has_uem else np.zeros(0, np.int64)
    ue = us + r["ud"].astype(np.int64) if has_uem else us
    b = np.unique(np.concatenate([ts, ts + td, ss, ss + sd, zs, ze, us, ue]))
    C = np.zeros((len(rl), len(hl)), object)
    C[...] = 0
    if len(b) < 2:
        return _finish(C, rl, hl, 0, 0, 0, 0, assign)
    na = len(b) - 1
    ticks = np.diff(b)

    def depth(starts, ends, weight=None):
        d = np.zeros(na + 1, np.int64)
        np.add.at(d, np.searchsorted(b, starts), 1 if weight is None else weight)
        np.add.at(d, np.searchsorted(b, ends), -1 if weight is None else -weight)
        return np.cumsum(d)[:na]

    scored = depth(zs, ze) == 0
    if has_uem:
        scored &= depth(us, ue) > 0
    talk = np.zeros((len(rl), na), bool)
    for i, k in enumerate(rl):
        sel = tk == k
        d = depth(ts[sel], ts[sel] + td[sel])
        assert d.max(initial=0) <= 1, "generator: same-speaker turns overlap"
        talk[i] = d > 0
    nref = talk.sum(0)
    assert depth(ss, ss + sd).max(initial=0) <= 1, "generator: hypothesis segments overlap"
    lab = depth(ss, ss + sd, hyp + 1) - 1                # the label of the one open segment, -1 where none (or non-speech)
    if skip_overlap:
        scored &= nref <= 1
    nhyp = (lab >= 0).astype(np.int64)
    w = np.where(scored, ticks, 0)
    tot = lambda v: sum(int(x) for x in (v * w).tolist())
    speech, miss, fa = tot(nref), tot(np.maximum(0, nref - nhyp)), tot(np.maximum(0, nhyp - nref))
    both = tot(np.minimum(nref, nhyp))
    hi = {v: k for k, v in enumerate(hl)}
    col = np.asarray([hi.get(j, 0) for j in range(int(lab.max(initial=-1)) + 1)], np.int64)
    for i in range(len(rl)):
        sel = talk[i] & (lab >= 0) & (w > 0)
        row = np.zeros(len(hl), np.int64)                # (a cell is at most 2^30 ticks: no overflow)
        np.add.at(row, col[lab[sel]], w[sel])
        for j, x in enumerate(row.tolist()):
            C[i, j] = int(x)
    return _finish(C, rl, hl, speech, miss, fa, both, assign)


def counts(recs, collar=0, skip_overlap=False, model=score_ticks):
    """counts int64 [R, 4] of a list of recordings."""
    return np.asarray([model(r, collar, skip_overlap)[0] for r in recs], np.int64).reshape(len(recs), 4)


def check_map(row, r, collar=0, skip_overlap=False, model=score_atoms):
    """The properties the contract gives the map row int32 [64] (der_model.check_map, on the atom matrix)."""
    _, C, rl, hl = model(r, collar, skip_overlap)
    row = np.asarray(row)
    assert row.shape == (MAX_REF,)
    mapped = [(i, int(row[i])) for i in range(MAX_REF) if row[i] != -1]
    assert all(i in rl for i, _ in mapped) and all(j in hl for _, j in mapped), "an absent label is mapped"
    assert len({j for _, j in mapped}) == len(mapped), "the map is not one-to-one"
    weight = 0
    for i, j in mapped:
        c = C[rl.index(i), hl.index(j)]
        assert c > 0, "a zero-weight pair is reported"
        weight += c
    assert weight == M.assign(C)[0], "the map does not attain the optimum"
    return weight


# ------------------------------------------------------------------------------------------- generators and packing
def _disjoint(rng, count, span, p_touch=0.3):
    """count intervals in [0, span], pairwise disjoint (some abut, some are empty), in random order -> (start, dur)"""
    if count == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    pts = np.sort(rng.integers(0, span + 1, 2 * count))
    for k in range(1, count):                            # make some neighbours abut
        if rng.random() < p_touch:
            pts[2 * k] = pts[2 * k - 1]
    s, e = pts[0::2], pts[1::2]
    p = rng.permutation(count)
    return s[p].astype(np.int32), (e - s)[p].astype(np.int32)


def random_recording(rng, n_seg, n_turns, n_spk=4, span=300, n_hyp=5, p_ns=0.15, n_uem=0):
    """n_turns reference turns over up to n_spk speakers (disjoint per speaker, overlapping across speakers), n_seg disjoint
    hypothesis segments with labels in [-1, n_hyp), n_uem UEM intervals (they may overlap; 0: no UEM)."""
    spk = rng.integers(0, max(n_spk, 1), n_turns)
    ts, td, tk = [], [], []
    for k in sorted(set(spk.tolist())):
        s, d = _disjoint(rng, int((spk == k).sum()), span)
        ts.append(s); td.append(d); tk.append(np.full(len(s), k, np.int32))
    cat = lambda a: np.concatenate(a) if a else np.zeros(0, np.int32)
    ts, td, tk = cat(ts), cat(td), cat(tk)
    p = rng.permutation(len(ts))
    ss, sd = _disjoint(rng, n_seg, span)
    hyp = rng.integers(0, n_hyp, n_seg).astype(np.int32)
    hyp[rng.random(n_seg) < p_ns] = -1
    us = ud = None
    if n_uem:
        us = rng.integers(0, span, n_uem).astype(np.int32)
        ud = rng.integers(0, span // 2 + 1, n_uem).astype(np.int32)
    return rec(ts[p], td[p], tk[p], ss, sd, hyp, us, ud)


def pack(recs):
    """The arrays of a call: (turns = (ts, td, tk, turn_off), ss, sd, hyp, offsets, uem = (us, ud, uem_off) or None); a UEM is
    packed when any recording has one (a recording without then gets one interval over everything)."""
    off = lambda sizes: np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cat = lambda k: np.concatenate([r[k] for r in recs]).astype(np.int32)
    uem = None
    if any(r["us"] is not None for r in recs):
        us = [r["us"] if r["us"] is not None else np.zeros(1, np.int32) for r in recs]
        ud = [r["ud"] if r["us"] is not None else np.full(1, 1 << 30, np.int32) for r in recs]
        uem = (np.concatenate(us).astype(np.int32), np.concatenate(ud).astype(np.int32), off([len(u) for u in us]))
    return ((cat("ts"), cat("td"), cat("tk"), off([len(r["ts"]) for r in recs])), cat("ss"), cat("sd"), cat("hyp"),
            off([len(r["ss"]) for r in recs]), uem)
