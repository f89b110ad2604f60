"""tests/trialkey_model.py -- the NumPy statement of a trial key (include/plda_hip.h, "trial keys"; csrc/partition.hip).

A key is (enrol_code [M], test_code [Nt], table [Ce, Ct]): pair (i, j) is a trial iff table[enrol_code[i], test_code[j]] >= 0,
that entry is its bucket, and it is a target iff enrol_spk[i] == test_spk[j].  Its list is L = 2 * bucket + class.  Within a
list the trials lie by (column strip j // 256, row i, column j)."""
import numpy as np

STRIP = 256
MAX_BUCKETS = 8


def bucket_and_class(enrol_code, test_code, table, enrol_spk, test_spk):
    """(bucket int64 [M, Nt], -1: not a trial; class bool [M, Nt])"""
    table = np.asarray(table, np.int64)
    bucket = table[np.asarray(enrol_code, np.int64)[:, None], np.asarray(test_code, np.int64)[None, :]]
    cls = np.asarray(enrol_spk, np.int64)[:, None] == np.asarray(test_spk, np.int64)[None, :]
    return bucket, cls


def one_list(S, mask):
    """the scores of the pairs in `mask`, in the contract's order"""
    nt = S.shape[1]
    parts = [S[:, s:s + STRIP][mask[:, s:s + STRIP]] for s in range(0, nt, STRIP)]
    return np.concatenate(parts) if parts else S[:0, 0]


def plan(enrol_code, test_code, table, n_buckets, enrol_spk, test_spk):
    """(count, offset: int64 [8, 2]; total: int64 [2]) -- [bucket][class], class 1 = targets"""
    bucket, cls = bucket_and_class(enrol_code, test_code, table, enrol_spk, test_spk)
    count, offset, total = np.zeros((MAX_BUCKETS, 2), np.int64), np.zeros((MAX_BUCKETS, 2), np.int64), np.zeros(2, np.int64)
    for b in range(MAX_BUCKETS):
        for c in (0, 1):
            offset[b, c] = total[c]
            if b < n_buckets:
                count[b, c] = int(np.count_nonzero((bucket == b) & (cls == bool(c))))
            total[c] += count[b, c]
    return count, offset, total


def lists(S, enrol_code, test_code, table, n_buckets, enrol_spk, test_spk):
    """{(bucket, class): fp32 list}, and the two class buffers (targets, non-targets): the buckets' lists in bucket order"""
    S = np.asarray(S, np.float32)
    bucket, cls = bucket_and_class(enrol_code, test_code, table, enrol_spk, test_spk)
    out = {(b, c): one_list(S, (bucket == b) & (cls == bool(c))) for b in range(n_buckets) for c in (0, 1)}
    tar = np.concatenate([out[(b, 1)] for b in range(n_buckets)])
    non = np.concatenate([out[(b, 0)] for b in range(n_buckets)])
    return out, tar, non


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
