"""Host model of top-N selection with indices (plda_amd/csrc/topn.hip), for the tests: the definition of include/plda_hip.h
("top-N retrieval with indices") restated in NumPy, independent of the product's arithmetic.

  score_key(S32)        the order-preserving uint32 key of fp32 scores: a < b <=> key(a) < key(b), -0.0 == +0.0, a total
                        order on all bit patterns (NaNs included: they sort where their bits put them)
  top_n(S32, n, axis)   (scores float32 [L, n], index int64 [L, n]): per line (axis 0: row, candidates = columns; axis 1:
                        column, candidates = rows) the first n candidates in the order (key descending, index ascending);
                        the scores are the matrix entries at those indices, bit for bit
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
