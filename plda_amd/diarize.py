"""plda_amd/diarize.py -- speaker clustering of the segments of recordings (csrc/ahc.hip; the contract is in
include/plda_hip.h, "speaker clustering"): batched average-linkage agglomerative clustering on PLDA score blocks, the
diarisation use of a PLDA back-end (Kaldi: ivector-plda-scoring-dense + agglomerative-cluster).

    ahc(engine, blocks, ...)          clusters R square fp32 score blocks on the device, one workgroup per recording
    plan(engine, n)                   the dispatch class a recording of n segments takes
    cut(merges, offsets, ...)         pure NumPy: labels at another threshold / speaker count from ONE full merge record
    MPlda.cluster(x, offsets, ...)    raw segment vectors in, labels out (the blocks are scored on the device and dropped)

A recording is merged bottom-up while the best pair's average score is at least `threshold` (None: no threshold) and more than
`num_speakers` clusters are left (None: 1).  Out of scope, on purpose: Kaldi's per-recording mean subtraction and PCA before
scoring, its two-pass clustering of very long recordings, RTTM output, DER.
"""
import ctypes as C

import numpy as np

from . import _native as N

AHC_MAX = 4096          # PLDA_AHC_MAX


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def offsets_of(sizes):
    """int64 [R + 1] offsets of recordings of the given sizes."""
    off = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(np.asarray(sizes, np.int64), out=off[1:])
    return off


def stop_args(offsets, threshold, num_speakers):
    """(has_threshold, threshold, min_clusters int32 [R] or None) of the C ABI from the Python arguments."""
    r = len(offsets) - 1
    if threshold is None and num_speakers is None:
        raise ValueError("threshold=None needs num_speakers (nothing would stop the merging)")
    minc = None
    if num_speakers is not None:
        minc = np.ascontiguousarray(np.broadcast_to(np.asarray(num_speakers), (r,)), np.int32)
    return (0 if threshold is None else 1), (0.0 if threshold is None else float(threshold)), minc


def merge_slices(offsets):
    """[(start, stop)] of every recording's entries in a merge record of length T - R."""
    return [(int(offsets[r]) - r, int(offsets[r + 1]) - r - 1) for r in range(len(offsets) - 1)]


def _outputs(t, r, return_merges):
    labels, ncl = np.empty(t, np.int32), np.empty(r, np.int32)
    if not return_merges:
        return labels, ncl, None, None, None
    return labels, ncl, np.empty(t - r, np.int32), np.empty(t - r, np.int32), np.empty(t - r, np.float64)


def plan(engine, n):
    """{"cls": 0 (sums in LDS) or 1 (sums in HBM scratch), "scratch_bytes": per recording, "lds_max": largest n of class 0}."""
    out = (C.c_int32 * 3)()
    N.check(engine._h, engine._lib.plda_ahc_plan(engine._h, int(n), out))
    return {"cls": int(out[0]), "scratch_bytes": int(out[1]), "lds_max": int(out[2])}


def pack(blocks):
    """(scores float32 [sum n_r^2], block_off int64 [R + 1], offsets int64 [R + 1]) of a list of square arrays."""
    blocks = [np.ascontiguousarray(b, np.float32) for b in blocks]
    for b in blocks:
        if b.ndim != 2 or b.shape[0] != b.shape[1]:
            raise ValueError("every block must be a square 2-D array, got shape %r" % (b.shape,))
    sizes = [b.shape[0] for b in blocks]
    block_off = offsets_of([n * n for n in sizes])
    scores = np.concatenate([b.ravel() for b in blocks]) if blocks else np.zeros(0, np.float32)
    return scores, block_off, offsets_of(sizes)


def ahc(engine, blocks, threshold=0.0, num_speakers=None, return_merges=False):
    """Cluster the recordings whose square fp32 score blocks are `blocks`.  Returns (labels int32 [T], n_clusters int32 [R]
    [, (merge_a, merge_b, merge_cost)]): T the total number of segments, labels 0 .. k-1 per recording by ascending smallest
    member; the merge record as include/plda_hip.h lays it out (merge_slices(offsets) cuts it per recording)."""
    scores, block_off, offsets = pack(blocks)
    has_t, thr, minc = stop_args(offsets, threshold, num_speakers)
    r, t = len(offsets) - 1, int(offsets[-1])
    labels, ncl, ma, mb, mc = _outputs(t, r, return_merges)
    N.check(engine._h, engine._lib.plda_ahc_matrix(engine._h, _p(scores), _p(block_off), _p(offsets), r, has_t, thr, _p(minc),
                                                   _p(labels), _p(ncl), _p(ma), _p(mb), _p(mc)))
    return (labels, ncl, (ma, mb, mc)) if return_merges else (labels, ncl)


def ahc_vectors(engine, vecs, offsets, threshold=0.0, num_speakers=None, return_merges=False):
    """The operand form: `vecs` [T, Dout] are already-transformed segment vectors (num_examples = 1); every recording's block
    is scored on the device exactly as score_matrix_dev would write it, clustered and dropped."""
    vecs = np.ascontiguousarray(vecs, np.float64)
    offsets = np.ascontiguousarray(offsets, np.int64)
    if offsets.ndim != 1 or len(offsets) < 2:
        raise ValueError("offsets must hold R + 1 >= 2 entries")
    if vecs.ndim != 2 or vecs.shape[0] != int(offsets[-1]):
        raise ValueError("vecs must be [offsets[-1], Dout], got %r" % (vecs.shape,))
    dout, _ = engine.dims()
    if vecs.shape[1] != dout:
        raise ValueError("vecs have dimension %d, the model's output dimension is %d" % (vecs.shape[1], dout))
    has_t, thr, minc = stop_args(offsets, threshold, num_speakers)
    r, t = len(offsets) - 1, int(offsets[-1])
    labels, ncl, ma, mb, mc = _outputs(t, r, return_merges)
    N.check(engine._h, engine._lib.plda_score_ahc(engine._h, _p(vecs), _p(offsets), r, has_t, thr, _p(minc), _p(labels), _p(ncl),
                                                  _p(ma), _p(mb), _p(mc)))
    return (labels, ncl, (ma, mb, mc)) if return_merges else (labels, ncl)


def cut(merges, offsets, threshold=None, num_speakers=None):
    """Labels at (threshold, num_speakers) from a FULL merge record (one taken with threshold=None, num_speakers=1), without
    the device: the record's prefix is replayed and stops at the first merge whose cost fails the device's own stop rule --
    k <= max(1, num_speakers), or !(cost <= -threshold) -- so the result equals a device run with those arguments exactly.
    Returns (labels int32 [T], n_clusters int32 [R]).  A threshold can so be tuned on a development set from one device run."""
    ma, mb, mc = (np.asarray(a) for a in merges)
    offsets = np.asarray(offsets, np.int64)
    has_t, thr, minc = stop_args(offsets, threshold, num_speakers)
    r, t = len(offsets) - 1, int(offsets[-1])
    labels, ncl = np.empty(t, np.int32), np.empty(r, np.int32)
    neg_thr = -np.float64(thr)
    for q, (m0, m1) in enumerate(merge_slices(offsets)):
        n = int(offsets[q + 1] - offsets[q])
        stop_k = max(1, int(minc[q])) if minc is not None else 1
        slot = np.arange(n)
        k = n
        e = m0
        while k > stop_k:
            if e >= m1 or ma[e] < 0:
                raise ValueError("the merge record of recording %d ends at %d clusters: not a full record" % (q, k))
            if has_t and not (mc[e] <= neg_thr):
                break
            slot[slot == mb[e]] = ma[e]
            k -= 1
            e += 1
        live = np.unique(slot)
        labels[offsets[q]:offsets[q + 1]] = np.searchsorted(live, slot)
        ncl[q] = k
    return labels, ncl
