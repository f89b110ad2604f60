"""The host models of the Jaccard error rate and the per-speaker figures (include/plda_hip.h, "Jaccard error rate and
per-speaker figures"; the JER form of csrc/der.hip's solve).

    atoms_ticks      the definition tick by tick: [speech, miss, fa, both], C, rt, ht over a recording of der_overlap_model's
                     kind (turns, segments with up to two labels, UEM), a collar and the skip-overlap switch
    atoms_intervals  the same by intervals
    atoms_segments   the segment form (ref, hyp, dur per segment)
    weights          w[i][j] = floor(C 2^32 / (rt[i] + ht[j] - C)) in Python ints
    best_exhaustive  the optimum of sum_i w[i][m(i)] with every one-to-one partial map tried (small matrices: asserted)
    best_scipy       the same from scipy.optimize.linear_sum_assignment on -w: w <= 2^32 and at most 64 rows, so every value
                     it adds is an integer below 2^53 and the result is exact
    jer              [n_ref, jsum] of a recording, from either optimum
    check_outputs    the laws the contract gives jer, jmap and spk of one recording

Everything is a Python int; nothing here is taken from the device."""
import numpy as np

import der_model as M
import der_overlap_model as O

ONE = 1 << 32
MAX_REF = O.MAX_REF


def _empty(rl, hl):
    return O._matrix(rl, hl), [0] * len(rl), [0] * len(hl)


def atoms_ticks(r, collar=0, skip_overlap=False):
    """([speech, miss, fa, both], C, rt, ht, ref labels, hyp labels), one tick at a time (der_overlap_model.score_ticks'
    walk, with rt and ht beside C)"""
    rl, hl = O._labels(r)
    ri, hi = {v: k for k, v in enumerate(rl)}, {v: k for k, v in enumerate(hl)}
    C, rt, ht = _empty(rl, hl)
    starts = [int(s) for s in r["ts"]] + [int(s) for s in r["ss"]]
    ends = [int(s) + int(d) for s, d in zip(r["ts"], r["td"])] + [int(s) + int(d) for s, d in zip(r["ss"], r["sd"])]
    if r["us"] is not None:
        starts += [int(s) for s in r["us"]]
        ends += [int(s) + int(d) for s, d in zip(r["us"], r["ud"])]
    if not starts:
        return [0, 0, 0, 0], C, rt, ht, rl, hl
    t0, t1 = min(starts) - collar, max(ends) + collar
    n = t1 - t0
    ref = [set() for _ in range(n)]
    seg = [set() for _ in range(n)]
    out = [False] * n
    inside = [r["us"] is None] * n
    for s, d, k in zip(r["ts"].tolist(), r["td"].tolist(), r["tk"].tolist()):
        if d == 0:
            continue
        for t in range(s, s + d):
            ref[t - t0].add(k)
        for b in (s, s + d):
            for t in range(b - collar, b + collar):
                out[t - t0] = True
    for s, d, b, b2 in zip(r["ss"].tolist(), r["sd"].tolist(), r["hyp"].tolist(), r["hyp2"].tolist()):
        for t in range(s, s + d):
            seg[t - t0] |= {x for x in (b, b2) if x >= 0}
    if r["us"] is not None:
        for s, d in zip(r["us"].tolist(), r["ud"].tolist()):
            for t in range(s, s + d):
                inside[t - t0] = True
    speech = miss = fa = both = 0
    for t in range(n):
        if out[t] or not inside[t] or (skip_overlap and len(ref[t]) > 1):
            continue
        nref, nhyp = len(ref[t]), len(seg[t])
        speech += nref
        miss += max(0, nref - nhyp)
        fa += max(0, nhyp - nref)
        both += min(nref, nhyp)
        for i in ref[t]:
            rt[ri[i]] += 1
            for j in seg[t]:
                C[ri[i], hi[j]] += 1
        for j in seg[t]:
            ht[hi[j]] += 1
    return [speech, miss, fa, both], C, rt, ht, rl, hl


def atoms_intervals(r, collar=0, skip_overlap=False):
    """The same by intervals: the boundaries cut the time line into atoms, depths are prefix sums of +-1 at the boundaries
    (der_overlap_model.score_atoms' construction)."""
    rl, hl = O._labels(r)
    C, rt, ht = _empty(rl, hl)
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
    if len(b) < 2:
        return [0, 0, 0, 0], C, rt, ht, rl, hl
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
        talk[i] = depth(ts[sel], ts[sel] + td[sel]) > 0
    nref = talk.sum(0)
    lab = [depth(ss, ss + sd, h + 1) - 1 for h in (hyp, hyp2)]
    if skip_overlap:
        scored &= nref <= 1
    nhyp = (lab[0] >= 0).astype(np.int64) + (lab[1] >= 0)
    w = np.where(scored, ticks, 0)
    tot = lambda v: sum(int(x) for x in (v * w).tolist())
    four = [tot(nref), tot(np.maximum(0, nref - nhyp)), tot(np.maximum(0, nhyp - nref)), tot(np.minimum(nref, nhyp))]
    hi = {v: k for k, v in enumerate(hl)}
    for a in np.flatnonzero(w > 0).tolist():
        d = int(w[a])
        J = [hi[int(l[a])] for l in lab if l[a] >= 0]
        for j in J:
            ht[j] += d
        for i in np.flatnonzero(talk[:, a]).tolist():
            rt[i] += d
            for j in J:
                C[i, j] += d
    return four, C, rt, ht, rl, hl


def atoms_segments(ref, hyp, dur=None):
    """The segment form: every segment weighted by dur (None: 1); ref = -1 / hyp = -1 is no speaker on that side."""
    C, rl, hl, speech, miss, fa, both = M.confusion(ref, hyp, dur)
    dur = np.ones(len(ref), np.int64) if dur is None else np.asarray(dur, np.int64)
    rt = [sum(int(d) for a, d in zip(ref, dur) if a == i) for i in rl]
    ht = [sum(int(d) for b, d in zip(hyp, dur) if b == j) for j in hl]
    return [speech, miss, fa, both], C, rt, ht, rl, hl


def weights(C, rt, ht):
    """w as a list of rows of Python ints; a pair with an empty union (rt = ht = 0) weighs 0"""
    out = []
    for i in range(len(rt)):
        row = []
        for j in range(len(ht)):
            c = int(C[i, j])
            u = rt[i] + ht[j] - c
            assert 0 <= c <= min(rt[i], ht[j])
            row.append(c * ONE // u if u > 0 else 0)
            assert 0 <= row[-1] <= ONE
        out.append(row)
    return out


def best_exhaustive(w):
    return O.best_map_exhaustive(w) if w and w[0] else 0


def best_scipy(w):
    """(jsum, column of every row or -1): scipy on integer-valued doubles, exact below 2^53"""
    from scipy.optimize import linear_sum_assignment
    if not w or not w[0]:
        return 0, [-1] * len(w)
    a = np.asarray(w, np.float64)
    assert len(w) * ONE < 1 << 53
    rows, cols = linear_sum_assignment(-a)
    col = [-1] * len(w)
    for i, j in zip(rows.tolist(), cols.tolist()):
        col[i] = j
    return sum(w[i][j] for i, j in enumerate(col) if j >= 0), col


def jer(C, rt, ht, best=None):
    """[n_ref, jsum] (Python ints)"""
    w = weights(C, rt, ht)
    jsum = best(w) if best else best_scipy(w)[0]
    return [sum(1 for v in rt if v > 0), jsum]


def jer_float(C, rt, ht):
    """the mean of 1 - I / U over the counting speakers under scipy's optimum on the EXACT Jaccard indices, in float64; NaN
    without a counting speaker"""
    from scipy.optimize import linear_sum_assignment
    n_ref = sum(1 for v in rt if v > 0)
    if n_ref == 0:
        return float("nan")
    if not ht:
        return 1.0
    a = np.zeros((len(rt), len(ht)))
    for i in range(len(rt)):
        for j in range(len(ht)):
            u = rt[i] + ht[j] - int(C[i, j])
            a[i, j] = int(C[i, j]) / u if u > 0 else 0.0
    rows, cols = linear_sum_assignment(-a)
    return 1.0 - float(a[rows, cols].sum()) / n_ref


def rate(pair):
    n, js = int(pair[0]), int(pair[1])
    return (n * ONE - js) / (n * ONE) if n > 0 else float("nan")


def score(r, collar=0, skip_overlap=False, atoms=atoms_intervals):
    """(counts [speech, miss, fa, confusion], [n_ref, jsum]) of a time-based recording"""
    four, C, rt, ht, rl, hl = atoms(r, collar, skip_overlap)
    return four[:3] + [four[3] - O.best_map_scipy(C)], jer(C, rt, ht)


def check_outputs(jer_row, jmap_row, spk_rows, C, rt, ht, rl, hl):
    """The contract of one recording's jer int64 [2], jmap int32 [64] and spk int64 [64, 3] against the model's matrices."""
    w = weights(C, rt, ht)
    want = jer(C, rt, ht)
    assert [int(v) for v in jer_row] == want, "jer %r, model %r" % (list(jer_row), want)
    jmap_row, spk_rows = np.asarray(jmap_row), np.asarray(spk_rows)
    assert jmap_row.shape == (MAX_REF,) and spk_rows.shape == (MAX_REF, 3)
    mapped = [(i, int(jmap_row[i])) for i in range(MAX_REF) if jmap_row[i] != -1]
    assert all(i in rl for i, _ in mapped) and all(j in hl for _, j in mapped), "an absent label is mapped"
    assert len({j for _, j in mapped}) == len(mapped), "jmap is not one-to-one"
    total = 0
    for i, j in mapped:
        assert C[rl.index(i), hl.index(j)] > 0, "a pair without a common tick is reported"
        total += w[rl.index(i)][hl.index(j)]
    assert total == want[1], "jmap does not attain jsum"
    law = 0
    for lab in range(MAX_REF):
        got = [int(v) for v in spk_rows[lab]]
        k = rl.index(lab) if lab in rl else -1
        if k < 0 or rt[k] == 0:
            assert got == [0, 0, 0] and jmap_row[lab] == -1, "label %d is absent: %r" % (lab, got)
            continue
        j = int(jmap_row[lab])
        inter = int(C[k, hl.index(j)]) if j >= 0 else 0
        union = rt[k] + (ht[hl.index(j)] if j >= 0 else 0) - inter
        assert got == [rt[k], inter, union], "label %d: spk %r, model %r" % (lab, got, [rt[k], inter, union])
        law += inter * ONE // union
    assert law == want[1], "the floor-sum law"
