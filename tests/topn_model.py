"""Host model of top-N selection with indices (plda_amd/csrc/topn.hip), for the tests: the definition of include/plda_hip.h
("top-N retrieval with indices") restated in NumPy, independent of the product's arithmetic.

  score_key(S32)        the order-preserving uint32 key of fp32 scores: a < b <=> key(a) < key(b), -0.0 == +0.0, a total
                        order on all bit patterns (NaNs included: they sort where their bits put them)
  top_n(S32, n, axis)   (scores float32 [L, n], index int64 [L, n]): per line (axis 0: row, candidates = columns; axis 1:
                        column, candidates = rows) the first n candidates in the order (key descending, index ascending);
                        the scores are the matrix entries at those indices, bit for bit
  content(kind, m, nt, rng)   the crafted matrices of the tests: ties, signed zeros, one binade, non-finite values, planted
                        duplicates where wave shares and pieces meet
"""
import numpy as np


def score_key(S32):
    u = np.ascontiguousarray(S32, np.float32).view(np.uint32)
    u = np.where(u == np.uint32(0x80000000), np.uint32(0), u)
    return np.where((u & np.uint32(0x80000000)) != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def top_n(S32, n, axis):
    S32 = np.asarray(S32, np.float32)
    assert S32.ndim == 2 and axis in (0, 1)
    lines = np.ascontiguousarray(S32 if axis == 0 else S32.T)
    assert 1 <= n <= lines.shape[1]
    key = score_key(lines).astype(np.int64)
    index = np.argsort(-key, axis=1, kind="stable")[:, :n].astype(np.int64)       # stable: equal keys keep ascending index
    bits = np.take_along_axis(lines.view(np.uint32), index, axis=1)              # (moved as integers: a NaN keeps its payload)
    return bits.view(np.float32), index


def content(kind, m, nt, rng):
    if kind == "gaussian":
        return (10.0 * rng.standard_normal((m, nt))).astype(np.float32)
    if kind == "equal":
        return np.full((m, nt), 1.25, np.float32)
    if kind == "zeros":                       # -0.0 and +0.0 are one value: the order is the index order, the bits are kept
        s = np.zeros((m, nt), np.float32)
        s[rng.random((m, nt)) < 0.5] = -0.0
        return s
    if kind in ("ascending", "descending"):   # every column ascends (descends) with the row: the column filter's worst (best) case
        s = (np.arange(m, dtype=np.float64)[:, None] + 0.125 * (np.arange(nt) % 7)[None, :]).astype(np.float32)
        return s if kind == "ascending" else -s
    if kind == "binade":                      # [1, 1.25): the first 11 key bits of all elements are equal -- one level-0 bin
        return (1.0 + 0.2499 * rng.random((m, nt))).astype(np.float32)
    if kind == "nonfinite":
        s = (10.0 * rng.standard_normal((m, nt))).astype(np.float32)
        u = rng.random((m, nt))
        s[u < 0.02] = np.inf
        s[(u >= 0.02) & (u < 0.04)] = -np.inf
        s[(u >= 0.04) & (u < 0.07)] = np.float32(1e-42)
        s[(u >= 0.07) & (u < 0.10)] = np.float32(-3e-45)
        s[(u >= 0.10) & (u < 0.12)] = 0.0
        return s
    assert kind == "duplicates"
    # one value above everything else planted where wave shares (a 16th of a row) and pieces (128 rows) meet, a second value
    # on a twentieth of all entries: ties at the top and at the n-th place that only the index order decides
    s = (10.0 * rng.standard_normal((m, nt))).astype(np.float32)
    s[rng.random((m, nt)) < 0.05] = 45.0
    seg = -(-nt // 16)
    seg4 = 4 * -(-(-(-nt // 4)) // 16)
    cols = sorted({c for c in (0, 1, seg - 1, seg, seg + 1, seg4 - 1, seg4, 2 * seg4, nt // 2, nt - 2, nt - 1) if 0 <= c < nt})
    rows = sorted({r for r in (0, 1, 63, 64, 127, 128, 129, 255, 256, 257, m // 2, m - 2, m - 1) if 0 <= r < m})
    s[np.ix_(rows, cols)] = 60.0
    return s
