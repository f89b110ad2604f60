"""The host models of the time-based diarisation error rate with up to TWO hypothesis labels per segment (include/plda_hip.h,
"time-based diarisation error rate", TWO HYPOTHESIS LABELS PER SEGMENT; plda_der_timed_ovl), and a seeded generator.

    score_ticks   the definition, tick by tick, in Python ints with label sets; `correct` by exhaustion over the one-to-one
                  partial maps (small speaker counts only: it asserts them)
    score_atoms   the same by intervals, `correct` from scipy.optimize.linear_sum_assignment (exact while every cell is
                  below 2^53: asserted)

A recording is der_time_model's dict plus "hyp2": int32 per segment, -1 = no second speaker; where hyp2 >= 0, hyp >= 0 and
hyp2 != hyp.  Both return ([speech, miss, fa, confusion], C, ref labels, hyp labels) as der_time_model's do, the hypothesis
labels ranging over both arrays."""
import numpy as np

import der_time_model as T

MAX_REF = T.MAX_REF


def rec(ts=(), td=(), tk=(), ss=(), sd=(), hyp=(), hyp2=None, us=None, ud=None):
    r = T.rec(ts, td, tk, ss, sd, hyp, us, ud)
    r["hyp2"] = np.full(len(r["hyp"]), -1, np.int32) if hyp2 is None else np.asarray(hyp2, np.int32).reshape(-1)
    assert r["hyp2"].shape == r["hyp"].shape
    assert not ((r["hyp2"] >= 0) & ((r["hyp"] < 0) | (r["hyp2"] == r["hyp"]))).any(), "generator: a bad second label"
    return r


def without_second(r):
    """the recording der_time_model scores: hyp alone"""
    return {k: v for k, v in r.items() if k != "hyp2"}


def _labels(r):
    rl = sorted({int(k) for k, d in zip(r["tk"], r["td"]) if d > 0})
    hl = sorted({int(b) for b in r["hyp"] if b >= 0} | {int(b) for b in r["hyp2"] if b >= 0})
    return rl, hl


def best_map_exhaustive(C):
    """the maximum of sum_i C[i][m(i)] over all one-to-one partial maps m, every map tried: row i stays unmapped or takes any
    column no earlier row took"""
    nr = len(C)
    nc = len(C[0]) if nr else 0
    assert nr <= 5 and nc <= 8, "exhaustion is for small speaker counts"

    def go(i, used):
        if i == nr:
            return 0
        best = go(i + 1, used)
        for j in range(nc):
            if not used >> j & 1:
                best = max(best, int(C[i][j]) + go(i + 1, used | 1 << j))
        return best
    return go(0, 0)


def best_map_scipy(C):
    from scipy.optimize import linear_sum_assignment
    if C.shape[0] == 0 or C.shape[1] == 0:
        return 0
    a = np.asarray(C.tolist(), np.int64)
    assert a.max(initial=0) < 1 << 53, "linear_sum_assignment works in float64"
    rows, cols = linear_sum_assignment(a, maximize=True)
    return sum(int(a[i, j]) for i, j in zip(rows, cols))


def _matrix(rl, hl):
    C = np.zeros((len(rl), len(hl)), object)
    C[...] = 0
    return C


def score_ticks(r, collar=0, skip_overlap=False):
    """The definition, one tick at a time: J(t) is the label set of the segment over tick t."""
    rl, hl = _labels(r)
    ri, hi = {v: k for k, v in enumerate(rl)}, {v: k for k, v in enumerate(hl)}
    C = _matrix(rl, hl)
    starts = [int(s) for s in r["ts"]] + [int(s) for s in r["ss"]]
    ends = [int(s) + int(d) for s, d in zip(r["ts"], r["td"])] + [int(s) + int(d) for s, d in zip(r["ss"], r["sd"])]
    if r["us"] is not None:
        starts += [int(s) for s in r["us"]]
        ends += [int(s) + int(d) for s, d in zip(r["us"], r["ud"])]
    if not starts:
        return [0, 0, 0, 0], C, rl, hl
    t0, t1 = min(starts) - collar, max(ends) + collar
    n = t1 - t0
    ref = [set() for _ in range(n)]
    seg = [[] for _ in range(n)]
    out = [False] * n
    inside = [r["us"] is None] * n
    for s, d, k in zip(r["ts"].tolist(), r["td"].tolist(), r["tk"].tolist()):
        if d == 0:
            continue
        for t in range(s, s + d):
            assert k not in ref[t - t0], "generator: same-speaker turns overlap"
            ref[t - t0].add(k)
        for b in (s, s + d):
            for t in range(b - collar, b + collar):
                out[t - t0] = True
    for s, d, b, b2 in zip(r["ss"].tolist(), r["sd"].tolist(), r["hyp"].tolist(), r["hyp2"].tolist()):
        for t in range(s, s + d):
            seg[t - t0].append({x for x in (b, b2) if x >= 0})
    if r["us"] is not None:
        for s, d in zip(r["us"].tolist(), r["ud"].tolist()):
            for t in range(s, s + d):
                inside[t - t0] = True
    speech = miss = fa = both = 0
    for t in range(n):
        assert len(seg[t]) <= 1, "generator: hypothesis segments overlap"
        if out[t] or not inside[t]:
            continue
        nref = len(ref[t])
        if skip_overlap and nref > 1:
            continue
        J = seg[t][0] if seg[t] else set()
        nhyp = len(J)
        speech += nref
        miss += max(0, nref - nhyp)
        fa += max(0, nhyp - nref)
        both += min(nref, nhyp)
        for i in ref[t]:
            for j in J:
                C[ri[i], hi[j]] += 1
    return [speech, miss, fa, both - best_map_exhaustive(C.tolist())], C, rl, hl


def score_atoms(r, collar=0, skip_overlap=False):
    """The same by intervals (der_time_model.score_atoms with a second label): the boundaries cut the time line into atoms,
    depths are prefix sums of +-1 at the boundaries; at most one segment is open over an atom, so a prefix sum of label + 1
    at its boundaries is that segment's label + 1, for either label."""
    rl, hl = _labels(r)
    ts, td, tk = (r[k].astype(np.int64) for k in ("ts", "td", "tk"))
    ss, sd, hyp, hyp2 = (r[k].astype(np.int64) for k in ("ss", "sd", "hyp", "hyp2"))
    keep = td > 0
    ts, td, tk = ts[keep], td[keep], tk[keep]
    keep = sd > 0
    ss, sd, hyp, hyp2 = ss[keep], sd[keep], hyp[keep], hyp2[keep]
    zs = np.concatenate([ts - collar, ts + td - collar]) if collar > 0 else np.zeros(0, np.int64)
    ze = zs + 2 * collar
    has_uem = r["us"] is not None
    us = r["us"].astype(np.int64) if has_uem else np.zeros(0, np.int64)
    ue = us + r["ud"].astype(np.int64) if has_uem else us
    b = np.unique(np.concatenate([ts, ts + td, ss, ss + sd, zs, ze, us, ue]))
    C = _matrix(rl, hl)
    if len(b) < 2:
        return [0, 0, 0, 0], C, rl, hl
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
    lab = [depth(ss, ss + sd, h + 1) - 1 for h in (hyp, hyp2)]
    if skip_overlap:
        scored &= nref <= 1
    nhyp = (lab[0] >= 0).astype(np.int64) + (lab[1] >= 0)
    w = np.where(scored, ticks, 0)
    tot = lambda v: sum(int(x) for x in (v * w).tolist())
    speech, miss, fa = tot(nref), tot(np.maximum(0, nref - nhyp)), tot(np.maximum(0, nhyp - nref))
    both = tot(np.minimum(nref, nhyp))
    col = np.full(max(hl, default=-1) + 1, 0, np.int64)
    col[hl] = np.arange(len(hl))
    for i in range(len(rl)):
        row = np.zeros(len(hl), np.int64)                # (a cell is at most 2 * 2^30 ticks: no overflow)
        for l in lab:
            sel = talk[i] & (l >= 0) & (w > 0)
            np.add.at(row, col[l[sel]], w[sel])
        for j, x in enumerate(row.tolist()):
            C[i, j] = int(x)
    return [speech, miss, fa, both - best_map_scipy(C)], C, rl, hl


def counts(recs, collar=0, skip_overlap=False, model=score_atoms):
    """counts int64 [R, 4] of a list of recordings."""
    return np.asarray([model(r, collar, skip_overlap)[0] for r in recs], np.int64).reshape(len(recs), 4)


def check_map(row, r, collar=0, skip_overlap=False):
    """The properties plda_der's contract gives the map row int32 [64], on the two-label matrix."""
    _, C, rl, hl = score_atoms(r, collar, skip_overlap)
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
    assert weight == best_map_scipy(C), "the map does not attain the optimum"


# ------------------------------------------------------------------------------------------- generator and packing
def add_second(rng, r, n_hyp, p_second=0.2):
    """der_time_model's recording with a second label, another one in [0, n_hyp), on about p_second of its speech segments"""
    hyp = r["hyp"]
    hyp2 = np.full(len(hyp), -1, np.int32)
    if n_hyp >= 2:
        pick = (rng.random(len(hyp)) < p_second) & (hyp >= 0)
        other = (hyp + 1 + rng.integers(0, n_hyp - 1, len(hyp))) % n_hyp          # uniform over the labels that are not hyp
        hyp2[pick] = other[pick]
    out = dict(r)
    out["hyp2"] = hyp2
    assert not ((hyp2 >= 0) & ((hyp < 0) | (hyp2 == hyp))).any()
    return out


def random_recording(rng, n_seg, n_turns, n_spk=4, span=300, n_hyp=5, p_ns=0.15, n_uem=0, p_second=0.2):
    return add_second(rng, T.random_recording(rng, n_seg, n_turns, n_spk, span, n_hyp, p_ns, n_uem), n_hyp, p_second)


def pack(recs):
    """der_time_model.pack's tuple with hyp2 behind it"""
    return T.pack(recs) + (np.concatenate([r["hyp2"] for r in recs]).astype(np.int32),)
