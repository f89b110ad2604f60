"""The host model of VBx's second speaker (include/plda_hip.h, "VBx resegmentation", SECOND SPEAKER; plda_vbx_top2): the rule
applied to a gamma array, in NumPy.  It selects and compares, it does not compute: its post2 is an entry of gamma, bit for bit.

    top2(gamma) -> (labels, k, labels2, post2) of ONE recording, gamma [T, S] in the initial numbering
"""
import numpy as np


def _argmax(row, allowed):
    """the first maximum of row over the allowed columns (ties: the smallest s), -1 when none is allowed"""
    best = -1
    for s in range(len(row)):
        if allowed[s] and (best < 0 or row[s] > row[best]):
            best = s
    return best


def top2(gamma):
    gamma = np.asarray(gamma, np.float64)
    t_n, s_n = gamma.shape
    every = np.ones(s_n, bool)
    first = np.asarray([_argmax(gamma[t], every) for t in range(t_n)], np.int64)
    alive = np.zeros(s_n, bool)
    alive[first] = True                                                   # A: somebody's first choice
    order = sorted(np.flatnonzero(alive), key=lambda s: int(np.flatnonzero(first == s)[0]))
    rank = {int(s): k for k, s in enumerate(order)}                       # 0 .. k-1 by ascending smallest first-member
    labels = np.asarray([rank[int(s)] for s in first], np.int32)
    labels2 = np.full(t_n, -1, np.int32)
    post2 = np.zeros(t_n, np.float64)
    for t in range(t_n):
        allowed = alive.copy()
        allowed[first[t]] = False
        s = _argmax(gamma[t], allowed)
        if s >= 0:
            labels2[t] = rank[s]
            post2[t] = gamma[t, s]
    return labels, len(order), labels2, post2
