"""The host model of the diarisation error rate (include/plda_hip.h, "diarisation error rate"; csrc/der.hip): confusion
counts in Python ints, an assignment solver (shortest augmenting paths, the column scan vectorised in NumPy so that 64 x 4096
stays in seconds), a brute-force optimum for small matrices, and input builders shared by the CPU and GPU tests.

The optimum VALUE is unique, so counts compare with ==.  The map is not canonical among equal-weight optima: the tests check
its properties (one-to-one, original label values, no zero-weight pair, attains `correct`), never its identity."""
import itertools

import numpy as np

MAX_REF = 64
MAX_HYP = 4096


def confusion(ref, hyp, dur=None):
    """(C, ref_labels, hyp_labels, speech, miss, fa, both) of one recording: C an object array of Python ints over the
    labels present, sorted."""
    ref, hyp = np.asarray(ref, np.int64), np.asarray(hyp, np.int64)
    dur = np.ones(len(ref), np.int64) if dur is None else np.asarray(dur, np.int64)
    rl, hl = sorted(set(ref[ref >= 0].tolist())), sorted(set(hyp[hyp >= 0].tolist()))
    ri, hi = {v: k for k, v in enumerate(rl)}, {v: k for k, v in enumerate(hl)}
    C = np.zeros((len(rl), len(hl)), object)
    C[...] = 0
    speech = miss = fa = both = 0
    for a, b, d in zip(ref.tolist(), hyp.tolist(), dur.tolist()):
        if a >= 0:
            speech += d
            if b < 0:
                miss += d
            else:
                both += d
                C[ri[a], hi[b]] += d
        elif b >= 0:
            fa += d
    return C, rl, hl, speech, miss, fa, both


def assign(C):
    """Maximum-weight one-to-one partial map of the rows of C (non-negative integers, any shape) to its columns ->
    (weight as a Python int, col_of_row int list, -1 = unmapped).  Shortest augmenting paths on cost = -C with int64
    potentials, over the orientation with fewer rows; zero columns pad a matrix with more rows than columns."""
    C = np.asarray(C)
    nr, nc = C.shape
    if nr == 0 or nc == 0:
        return 0, [-1] * nr
    if nr > nc:
        w, row_of_col = assign(C.T)
        col_of_row = [-1] * nr
        for j, i in enumerate(row_of_col):
            if i >= 0:
                col_of_row[i] = j
        return w, col_of_row
    cost = -C.astype(np.int64)
    INF = np.int64(1) << 62
    u = np.zeros(nr + 1, np.int64)
    v = np.zeros(nc + 1, np.int64)
    own = np.zeros(nc + 1, np.int64)            # row (1-based) holding column j; column 0 is virtual
    way = np.zeros(nc + 1, np.int64)
    for i in range(1, nr + 1):
        own[0] = i
        minv = np.full(nc + 1, INF, np.int64)
        used = np.zeros(nc + 1, bool)
        j0 = 0
        while True:
            used[j0] = True
            i0 = own[j0]
            free = ~used
            free[0] = False
            cur = np.full(nc + 1, INF, np.int64)
            cur[1:] = cost[i0 - 1] - u[i0] - v[1:]
            better = free & (cur < minv)
            minv[better] = cur[better]
            way[better] = j0
            cand = np.where(free, minv, INF)
            j1 = int(np.argmin(cand))            # the first minimum
            delta = cand[j1]
            u[own[used]] += delta
            v[used] -= delta
            minv[free] -= delta
            j0 = j1
            if own[j0] == 0:
                break
        while j0:
            j1 = int(way[j0])
            own[j0] = own[j1]
            j0 = j1
    col_of_row = [-1] * nr
    weight = 0
    for j in range(1, nc + 1):
        if own[j]:
            col_of_row[int(own[j]) - 1] = j - 1
            weight += int(C[int(own[j]) - 1, j - 1])
    return weight, col_of_row


def brute(C):
    """The optimum weight over all one-to-one partial maps, by enumeration (both sides <= 6)."""
    C = np.asarray(C)
    nr, nc = C.shape
    assert nr <= 6 and nc <= 6
    if nr > nc:
        C, nr, nc = C.T, nc, nr
    best = 0
    for perm in itertools.permutations(range(nc), nr):       # C >= 0: a full map of the shorter side loses nothing
        best = max(best, sum(int(C[i, perm[i]]) for i in range(nr)))
    return best


def score_one(ref, hyp, dur=None):
    """[speech, miss, fa, confusion] (Python ints), the map {ref label: hyp label} (zero-weight pairs dropped), C, labels."""
    C, rl, hl, speech, miss, fa, both = confusion(ref, hyp, dur)
    correct, col = assign(C)
    m = {rl[i]: hl[j] for i, j in enumerate(col) if j >= 0 and C[i, j] > 0}
    return [speech, miss, fa, both - correct], m, C, rl, hl


def score(ref, hyp, offsets, dur=None):
    """counts int64 [R, 4] of the recordings of a call."""
    ref, hyp = np.asarray(ref), np.asarray(hyp)
    out = np.zeros((len(offsets) - 1, 4), np.int64)
    for r in range(len(offsets) - 1):
        a, b = int(offsets[r]), int(offsets[r + 1])
        out[r] = score_one(ref[a:b], hyp[a:b], None if dur is None else np.asarray(dur)[a:b])[0]
    return out


def check_map(row, ref, hyp, dur=None):
    """The properties the contract gives the map row int32 [64] of one recording; returns the weight it attains."""
    C, rl, hl, speech, miss, fa, both = confusion(ref, hyp, dur)
    row = np.asarray(row)
    assert row.shape == (MAX_REF,)
    mapped = [(i, int(row[i])) for i in range(MAX_REF) if row[i] != -1]
    assert all(i in rl for i, _ in mapped), "a reference label that is absent is mapped"
    assert all(j in hl for _, j in mapped), "a hypothesis label that is absent is mapped to"
    assert len({j for _, j in mapped}) == len(mapped), "the map is not one-to-one"
    weight = 0
    for i, j in mapped:
        c = C[rl.index(i), hl.index(j)]
        assert c > 0, "a zero-weight pair is reported"
        weight += c
    correct, _ = assign(C)
    assert weight == correct, "the map attains %d, the optimum is %d" % (weight, correct)
    return weight


# ------------------------------------------------------------------------------------------- input builders
def from_matrix(C, seed=0, unit=None):
    """(ref, hyp, dur) of one recording whose confusion matrix over labels 0.. is C: one segment per non-zero cell (dur = the
    cell), shuffled; `unit`: instead C[i, j] segments of that duration."""
    C = np.asarray(C, np.int64)
    ref, hyp, dur = [], [], []
    for i in range(C.shape[0]):
        for j in range(C.shape[1]):
            if C[i, j] > 0:
                k = 1 if unit is None else int(C[i, j])
                ref += [i] * k
                hyp += [j] * k
                dur += [int(C[i, j]) if unit is None else unit] * k
    p = np.random.default_rng(seed).permutation(len(ref))
    return np.asarray(ref, np.int32)[p], np.asarray(hyp, np.int32)[p], np.asarray(dur, np.int32)[p]


def greedy_trap(k):
    """A 2k x 2k matrix of k diagonal blocks [[10, 9], [9, 0]] (weights growing by block so that no two blocks tie): a greedy
    largest-cell map takes 10 + 0 in every block where the optimum takes 9 + 9."""
    C = np.zeros((2 * k, 2 * k), np.int64)
    for b in range(k):
        s = b + 1
        C[2 * b:2 * b + 2, 2 * b:2 * b + 2] = [[10 * s, 9 * s], [9 * s, 0]]
    return C


def random_case(rng, n, sr, sh, p_ref_ns=0.1, p_hyp_ns=0.1, max_dur=5, gap=1):
    """n segments, labels drawn from sr / sh values spaced `gap` apart (the reference's closer where 64 values do not hold
    that), -1 with the given probabilities."""
    ref = (rng.integers(0, sr, n) * min(gap, (MAX_REF - 1) // max(sr - 1, 1))).astype(np.int32)
    hyp = (rng.integers(0, sh, n) * gap).astype(np.int32)
    ref[rng.random(n) < p_ref_ns] = -1
    hyp[rng.random(n) < p_hyp_ns] = -1
    dur = rng.integers(0, max_dur + 1, n).astype(np.int32)
    return ref, hyp, dur


def exact_shape(rng, n, sr, sh):
    """n >= max(sr, sh) segments in which exactly sr reference and sh hypothesis labels occur (0 .. sr-1, 0 .. sh-1)."""
    assert n >= max(sr, sh)
    ref = np.concatenate([np.arange(sr), rng.integers(0, sr, n - sr)]).astype(np.int32)
    hyp = np.concatenate([np.arange(sh), rng.integers(0, sh, n - sh)]).astype(np.int32)
    rng.shuffle(ref)
    rng.shuffle(hyp)
    return ref, hyp, rng.integers(1, 8, n).astype(np.int32)


def planted_block(sizes, seed, noise=0.3):
    """A square fp32 score block of planted speakers (+1 inside, -1 across, Gaussian noise) and the speaker of every
    segment, interleaved at random."""
    rng = np.random.default_rng(seed)
    g = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    S = np.where(g[:, None] == g[None, :], 1.0, -1.0) + noise * rng.standard_normal((len(g), len(g)))
    return S.astype(np.float32), g.astype(np.int32)
