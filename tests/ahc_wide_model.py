"""tests/ahc_wide_model.py -- host models of what the corpus-scale clustering (include/plda_hip.h, "corpus-scale clustering";
K28) adds on top of tests/ahc_model.py, which is the model of the clustering itself (the wide class is held to it with R = 1).

    keep_clusters(labels, m)     the filter and renumber step of MPlda.adapt_clustered, written as the plain loop
    with_row_stride(S, ld)       a block laid out with row stride ld, the padding NaN (it must never be read)
    threshold_after(costs, m)    a threshold at which a run with the full record `costs` stops after exactly m merges
"""
import numpy as np


def keep_clusters(labels, min_cluster_size):
    """-> (rows kept, ascending; their new labels; clusters kept): clusters of at least min_cluster_size members survive and
    are renumbered 0 .. in the order of their old numbers."""
    labels = [int(v) for v in labels]
    count = {}
    for v in labels:
        count[v] = count.get(v, 0) + 1
    new = {}
    for v in sorted(count):
        if count[v] >= min_cluster_size:
            new[v] = len(new)
    rows = [i for i, v in enumerate(labels) if v in new]
    return np.asarray(rows, np.int64), np.asarray([new[labels[i]] for i in rows], np.int64), len(new)


def with_row_stride(S, ld):
    """the (n - 1) * ld + n floats of the block S [n, n] at row stride ld >= n; every padding float is NaN"""
    n = S.shape[0]
    assert ld >= n
    full = np.full((n, ld), np.nan, np.float32)
    full[:, :n] = S
    return full.ravel()[:(n - 1) * ld + n].copy()


def threshold_after(costs, m):
    """the score threshold halfway between merge m - 1 and merge m of a full record whose costs ascend strictly there: a run
    with it makes exactly m merges (v <= -threshold holds for the first m, fails for the next)"""
    assert 0 < m < len(costs) and costs[m - 1] < costs[m] and (m < 2 or costs[:m].max() == costs[m - 1])
    thr = -(costs[m - 1] + costs[m]) / 2.0
    assert costs[m - 1] <= -thr < costs[m]
    return float(thr)
