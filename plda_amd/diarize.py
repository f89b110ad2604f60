"""plda_amd/diarize.py -- speaker diarisation of the segments of recordings: batched average-linkage agglomerative clustering
on PLDA score blocks (csrc/ahc.hip; include/plda_hip.h, "speaker clustering"; Kaldi: ivector-plda-scoring-dense +
agglomerative-cluster), then VBx resegmentation, a variational-Bayes HMM over the segment sequence with the PLDA model as its
emission model, initialised from the clustering (csrc/vbx.hip; include/plda_hip.h, "VBx resegmentation"; Landini et al. 2022).

    ahc(engine, blocks, ...)          clusters R square fp32 score blocks on the device, one workgroup per recording
    plan(engine, n)                   the dispatch class a recording of n segments takes
    cut(merges, offsets, ...)         pure NumPy: labels at another threshold / speaker count from ONE full merge record
    MPlda.cluster(x, offsets, ...)    raw segment vectors in, labels out (the blocks are scored on the device and dropped)
    ahc_wide(engine, block, ...)      ONE problem of up to AHC_WIDE_MAX = 32768 vectors on the whole device, the same contract
                                      (K28, "corpus-scale clustering"); ahc_wide_vectors: its operand form; plan_wide(engine, n);
                                      MPlda.cluster_corpus(x, ...) takes raw vectors, MPlda.adapt_clustered(x, ...) fits an
                                      in-domain model on the pseudo-labels (keep_clusters: its filter) and blends it in
    score_dense_pca(engine, x, offsets, t)   every recording's block scored in the PCA subspace of its own segment vectors
                                      (Kaldi's --target-energy=t; csrc/dense_pca.hip), one workgroup per recording
    spectral(engine, blocks, ...)     clusters the same blocks without a threshold: spectral clustering on a pruned
                                      nearest-neighbour graph, the pruning value by the normalised-maximum-eigengap rule, the
                                      speaker count from the largest eigengap (csrc/spectral.hip; MPlda.cluster(method="spectral"))
    spectral_vectors(engine, vecs, offsets, ...)   its operand form; spectral_plan(engine, n, k): its dispatch classes
    ahc_dense_pca(engine, x, offsets, t, ...)   the same blocks clustered and dropped (MPlda.cluster(..., target_energy=t))
    dense_pca_plan(engine, n, d)      the dispatch class a recording of n segments at dimension d takes there
    vbx(engine, y, offsets, labels)   resegments R recordings of projected vectors from initial labels, one workgroup each;
                                      return_second=True: + every segment's second most likely speaker and its posterior
    apply_overlap(labels2, post2, ...)   pure NumPy: where to keep the second speaker (a detector's mask, a posterior floor)
    vbx_plan(engine, t, s, d)         the dispatch class a recording of t segments, s initial speakers, dimension d takes
    MPlda.resegment(x, offsets, labels, ...)   raw segment vectors in: plda_project_rows, then vbx
    MPlda.diarize(x, offsets, ...)    cluster, then resegment

A recording is merged bottom-up while the best pair's average score is at least `threshold` (None: no threshold) and more than
`num_speakers` clusters are left (None: 1).  Out of scope, on purpose: Kaldi's per-recording mean subtraction, its two-pass
clustering of very long recordings; for VBx: more than 64 initial speakers, several workgroups on one
recording, an overlap detector, a third speaker.  The diarisation error rate, and the threshold sweep that cut() serves on the host, live in
plda_amd/der.py; RTTM files in plda_amd/rttm.py.  Length normalisation and the LDA fit before the model are the embedding
chain's (K18: plda_amd/embed.py, MPlda.fit_embedding / set_embedding): with one attached, cluster / resegment / diarize take
the extractor's output as it is.
"""
import ctypes as C

import numpy as np

from . import _native as N

AHC_MAX = 4096          # PLDA_AHC_MAX
VBX_MAX_SPK = 64        # PLDA_VBX_MAX_SPK


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


# ------------------------------------------------------------------------------------------- corpus-scale clustering (K28)
AHC_WIDE_MAX = 32768    # PLDA_AHC_WIDE_MAX


def plan_wide(engine, n):
    """{"scratch_bytes": the wide class's state for n vectors (the operand form adds 4 n^2), "launches_per_step",
    "steps_per_check": the steps enqueued between two host reads of the stop word, "pieces": the column pieces of a row scan}."""
    out = (C.c_int64 * 4)()
    N.check(engine._h, engine._lib.plda_ahc_wide_plan(engine._h, int(n), out))
    return {"scratch_bytes": int(out[0]), "launches_per_step": int(out[1]), "steps_per_check": int(out[2]), "pieces": int(out[3])}


def wide_args(n, threshold, num_speakers):
    """The argument check of ahc_wide / ahc_wide_vectors / MPlda.cluster_corpus, before any device work ->
    (has_threshold, threshold, min_clusters) of the C ABI.  ONE problem: num_speakers is one integer >= 1 or None."""
    if isinstance(n, bool) or int(n) != n or not 1 <= n <= AHC_WIDE_MAX:
        raise ValueError("one problem must hold 1 ... %d vectors, got %r" % (AHC_WIDE_MAX, n))
    if num_speakers is not None:
        if isinstance(num_speakers, (bool, np.bool_)) or np.ndim(num_speakers) != 0 or not isinstance(num_speakers, (int, np.integer)):
            raise ValueError("num_speakers must be one integer >= 1 (the corpus is one problem), got %r" % (num_speakers,))
        if not 1 <= int(num_speakers) <= 0x7fffffff:
            raise ValueError("num_speakers must be >= 1, got %r" % (num_speakers,))
    if threshold is not None:
        if isinstance(threshold, (bool, np.bool_)) or not isinstance(threshold, (int, float, np.integer, np.floating)):
            raise ValueError("threshold must be a number or None, got %r" % (threshold,))
        if np.isnan(threshold):
            raise ValueError("threshold is NaN")
    has_t, thr, minc = stop_args(np.asarray([0, int(n)], np.int64), threshold, num_speakers)
    return has_t, thr, (1 if minc is None else int(minc[0]))


def ahc_wide(engine, block, threshold=0.0, num_speakers=None, return_merges=False):
    """Cluster ONE problem of n <= AHC_WIDE_MAX vectors whose square fp32 score block is `block`, on the whole device
    (include/plda_hip.h, "corpus-scale clustering"): the contract of ahc() with one recording, for every n from 1 up.  Returns
    (labels int32 [n], n_clusters int[, (merge_a, merge_b, merge_cost)])."""
    block = np.asarray(block)
    if block.ndim != 2 or block.shape[0] != block.shape[1]:
        raise ValueError("the block must be a square 2-D array, got shape %r" % (block.shape,))
    n = block.shape[0]
    has_t, thr, minc = wide_args(n, threshold, num_speakers)
    block = np.ascontiguousarray(block, np.float32)
    labels, ncl, ma, mb, mc = _outputs(n, 1, return_merges)
    N.check(engine._h, engine._lib.plda_ahc_wide_matrix(engine._h, _p(block), n, n, has_t, thr, minc, _p(labels), _p(ncl), _p(ma), _p(mb),
                                                        _p(mc)))
    return (labels, int(ncl[0]), (ma, mb, mc)) if return_merges else (labels, int(ncl[0]))


def ahc_wide_vectors(engine, y, threshold=0.0, num_speakers=None, return_merges=False):
    """The operand form: `y` [n, Dout] are already-transformed vectors (num_examples = 1); the block is scored on the device
    exactly as score_matrix_dev would write it, clustered and dropped."""
    y = np.asarray(y)
    if y.ndim != 2:
        raise ValueError("y must be [n, Dout], got %r" % (y.shape,))
    has_t, thr, minc = wide_args(y.shape[0], threshold, num_speakers)
    y = np.ascontiguousarray(y, np.float64)
    dout, _ = engine.dims()
    if y.shape[1] != dout:
        raise ValueError("y has dimension %d, the model's output dimension is %d" % (y.shape[1], dout))
    n = y.shape[0]
    labels, ncl, ma, mb, mc = _outputs(n, 1, return_merges)
    N.check(engine._h, engine._lib.plda_score_ahc_wide(engine._h, _p(y), n, has_t, thr, minc, _p(labels), _p(ncl), _p(ma), _p(mb), _p(mc)))
    return (labels, int(ncl[0]), (ma, mb, mc)) if return_merges else (labels, int(ncl[0]))


def keep_clusters(labels, min_cluster_size=2):
    """The filter and renumber step of MPlda.adapt_clustered, pure NumPy: (rows int64 [m], the rows of clusters with at least
    min_cluster_size members, ascending; new_labels int64 [m], those clusters renumbered 0 .. kept - 1 in their old order;
    kept)."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.dtype.kind not in "iu" or (labels.size and labels.min() < 0):
        raise ValueError("labels must be a 1-D array of integers >= 0")
    if isinstance(min_cluster_size, bool) or int(min_cluster_size) != min_cluster_size or min_cluster_size < 1:
        raise ValueError("min_cluster_size must be an integer >= 1, got %r" % (min_cluster_size,))
    counts = np.bincount(labels) if labels.size else np.zeros(0, np.int64)
    keep = counts >= int(min_cluster_size)
    new_id = np.cumsum(keep) - 1
    rows = np.nonzero(keep[labels])[0].astype(np.int64)
    return rows, new_id[labels[rows]].astype(np.int64), int(keep.sum())


# ------------------------------------------------------------------------------------------- spectral clustering
SPECTRAL_MAX = 2048         # PLDA_SPECTRAL_MAX
SPECTRAL_MAX_SPK = 64       # PLDA_SPECTRAL_MAX_SPK
SPECTRAL_MAX_P = 16         # PLDA_SPECTRAL_MAX_P
P_FRACTIONS = (0.03, 0.05, 0.08, 0.12, 0.16, 0.2, 0.25, 0.3)


def spectral_plan(engine, n, k=1):
    """{"select_class": keys per lane of the neighbour selection for n segments, "select_max": the largest n of that class,
    "kmeans_cls": 0 (embedding in LDS) or 1 (in scratch) for k columns, "kmeans_lds_max": the largest n of class 0 at this k,
    "scratch_bytes": the working set of one eigenproblem of order n}."""
    out = (C.c_int32 * 5)()
    N.check(engine._h, engine._lib.plda_spectral_plan(engine._h, int(n), int(k), out))
    return {"select_class": int(out[0]), "select_max": int(out[1]), "kmeans_cls": int(out[2]), "kmeans_lds_max": int(out[3]),
            "scratch_bytes": int(out[4])}


def spectral_args(offsets, p=None, p_fractions=P_FRACTIONS, max_speakers=16, num_speakers=None, max_iters=20):
    """(p_table int32 [R, P], num_speakers int32 [R] or None) of the C ABI from the Python arguments, checked before any device
    work.  p=None: p = min(N - 1, max(2, ceil(f N))) per recording for every f of p_fractions (1 at least); an int: that value
    for every recording; a list: those values for every recording; an [R, P] array: as given."""
    offsets = np.asarray(offsets, np.int64)
    if offsets.ndim != 1 or len(offsets) < 2:
        raise ValueError("offsets must hold R + 1 >= 2 entries")
    r = len(offsets) - 1
    sizes = np.diff(offsets)
    if offsets[0] != 0 or (sizes < 1).any() or (sizes > SPECTRAL_MAX).any():
        raise ValueError("every recording must hold 1 ... %d segments (offsets must ascend from 0)" % SPECTRAL_MAX)
    if isinstance(max_speakers, bool) or int(max_speakers) != max_speakers or not 1 <= max_speakers <= SPECTRAL_MAX_SPK:
        raise ValueError("max_speakers must be an integer in 1 ... %d" % SPECTRAL_MAX_SPK)
    if isinstance(max_iters, bool) or int(max_iters) != max_iters or not 1 <= max_iters <= 1000:
        raise ValueError("max_iters must be an integer in 1 ... 1000")
    if p is None:
        f = np.asarray(p_fractions, np.float64)
        if f.ndim != 1 or not 1 <= len(f) <= SPECTRAL_MAX_P or not (np.isfinite(f).all() and (f > 0).all()):
            raise ValueError("p_fractions must hold 1 ... %d positive fractions" % SPECTRAL_MAX_P)
        table = np.maximum(1, np.minimum(sizes[:, None] - 1, np.maximum(2, np.ceil(f[None, :] * sizes[:, None]).astype(np.int64))))
    else:
        table = np.asarray(p)
        if table.dtype.kind not in "iu":
            raise ValueError("p must be an integer, a list of integers or an [R, P] integer array")
        table = np.broadcast_to(table.reshape(1, -1) if table.ndim < 2 else table, (r, table.shape[-1] if table.ndim else 1))
        if not 1 <= table.shape[1] <= SPECTRAL_MAX_P or (table < 1).any() or (table > 0x7fffffff).any():
            raise ValueError("p must hold 1 ... %d values >= 1 per recording" % SPECTRAL_MAX_P)
    ns = None
    if num_speakers is not None:
        ns = np.ascontiguousarray(np.broadcast_to(np.asarray(num_speakers), (r,)), np.int32)
        if (ns < 0).any() or (ns > max_speakers).any():
            raise ValueError("num_speakers must lie in 0 ... max_speakers = %d (0: the eigengap's count)" % max_speakers)
    return np.ascontiguousarray(table, np.int32), ns


def _spectral_call(engine, fn, head, offsets, table, ns, max_speakers, max_iters, return_info):
    r, t, ms = len(offsets) - 1, int(offsets[-1]), int(max_speakers)
    labels, ncl = np.empty(t, np.int32), np.empty(r, np.int32)
    pu = kg = eig = emb = d2 = None
    if return_info:
        pu, kg, d2 = np.empty(r, np.int32), np.empty(r, np.int32), np.empty(t, np.int32)
        eig, emb = np.empty((r, table.shape[1], ms + 2), np.float64), np.empty((t, ms), np.float64)
    N.check(engine._h, fn(engine._h, *head, _p(offsets), r, _p(table), table.shape[1], ms, _p(ns), int(max_iters), _p(labels), _p(ncl),
                          _p(pu), _p(kg), _p(eig), _p(emb), _p(d2)))
    if not return_info:
        return labels, ncl
    return labels, ncl, {"p_used": pu, "k_gap": kg, "eig": eig, "embed": emb, "deg2": d2, "p_table": table}


def spectral(engine, blocks, p=None, p_fractions=P_FRACTIONS, max_speakers=16, num_speakers=None, max_iters=20, return_info=False):
    """Cluster the recordings whose square fp32 score blocks are `blocks` by spectral clustering with auto-tuned pruning
    (include/plda_hip.h, "spectral clustering with auto-tuned pruning"): no threshold, the speaker count from the largest
    eigengap (at most max_speakers) unless num_speakers (an int or one per recording; 0: the eigengap's) gives it.  Returns
    (labels int32 [T], n_clusters int32 [R][, info]): labels 0 .. per recording by first occurrence; info = {"p_used", "k_gap"
    int32 [R], "eig" [R, P, max_speakers + 2], "embed" [T, max_speakers], "deg2" int32 [T], "p_table" int32 [R, P]}."""
    scores, block_off, offsets = pack(blocks)
    table, ns = spectral_args(offsets, p, p_fractions, max_speakers, num_speakers, max_iters)
    return _spectral_call(engine, engine._lib.plda_spectral_matrix, (_p(scores), _p(block_off)), offsets, table, ns, max_speakers,
                          max_iters, return_info)


def spectral_vectors(engine, vecs, offsets, p=None, p_fractions=P_FRACTIONS, max_speakers=16, num_speakers=None, max_iters=20,
                     return_info=False):
    """The operand form: `vecs` [T, Dout] are already-transformed segment vectors (num_examples = 1); every recording's block
    is scored on the device exactly as score_matrix_dev would write it, clustered and dropped."""
    vecs = np.ascontiguousarray(vecs, np.float64)
    offsets = np.ascontiguousarray(offsets, np.int64)
    table, ns = spectral_args(offsets, p, p_fractions, max_speakers, num_speakers, max_iters)
    if vecs.ndim != 2 or vecs.shape[0] != int(offsets[-1]):
        raise ValueError("vecs must be [offsets[-1], Dout], got %r" % (vecs.shape,))
    dout, _ = engine.dims()
    if vecs.shape[1] != dout:
        raise ValueError("vecs have dimension %d, the model's output dimension is %d" % (vecs.shape[1], dout))
    return _spectral_call(engine, engine._lib.plda_score_spectral, (_p(vecs),), offsets, table, ns, max_speakers, max_iters, return_info)


# ------------------------------------------------------------------------------------------- dense scoring behind a PCA
DENSE_PCA_MAX_DIM = 512     # PLDA_DENSE_PCA_MAX_DIM


def dense_pca_plan(engine, n, d):
    """{"cls": 0 (working matrix in LDS) or 1 (in HBM scratch), "scratch_bytes": per recording, "m": min(n, d), "lds_max": the
    largest m of class 0} of a recording of n segments at model dimension d."""
    out = (C.c_int32 * 4)()
    N.check(engine._h, engine._lib.plda_dense_pca_plan(engine._h, int(n), int(d), out))
    return {"cls": int(out[0]), "scratch_bytes": int(out[1]), "m": int(out[2]), "lds_max": int(out[3])}


def dense_pca_args(engine, x, offsets, target_energy):
    """The argument check of score_dense_pca / ahc_dense_pca, before any device work -> (x, offsets).  ValueError on anything
    the C ABI would answer with PLDA_E_INVAL and that the host can see."""
    x = np.ascontiguousarray(x, np.float64)
    offsets = np.ascontiguousarray(offsets, np.int64)
    if not (isinstance(target_energy, (int, float, np.floating)) and 0.0 < float(target_energy) < 1.0):
        raise ValueError("target_energy must lie in (0, 1), got %r" % (target_energy,))
    if offsets.ndim != 1 or len(offsets) < 2:
        raise ValueError("offsets must hold R + 1 >= 2 entries")
    if offsets[0] != 0:
        raise ValueError("offsets must start at 0")
    sizes = np.diff(offsets)
    if (sizes < 1).any() or (sizes > AHC_MAX).any():
        raise ValueError("every recording must hold 1 ... %d segments (offsets must ascend)" % AHC_MAX)
    if x.ndim != 2 or x.shape[0] != int(offsets[-1]):
        raise ValueError("x must be [offsets[-1], D], got %r" % (x.shape,))
    dout, din = engine.dims()
    if dout != din:
        raise ValueError("the model is truncated (transform %d x %d): the PCA projects the untruncated model" % (dout, din))
    if din > DENSE_PCA_MAX_DIM:
        raise ValueError("model dimension %d: dense PCA scoring is supported up to %d" % (din, DENSE_PCA_MAX_DIM))
    if x.shape[1] != din:
        raise ValueError("x has dimension %d, the model's input dimension is %d" % (x.shape[1], din))
    if not np.isfinite(x).all():
        raise ValueError("x holds non-finite values")
    return x, offsets


def score_dense_pca(engine, x, offsets, target_energy, return_info=False):
    """Score every recording's segment pairs in the PCA subspace of its own segment vectors (include/plda_hip.h, "dense scoring
    in a recording's PCA subspace"): x [T, D] rows in the model's input space, recording r owning rows offsets[r] ..
    offsets[r+1].  Returns a list of [N_r, N_r] float32 blocks (S[i, j]: enrol i, test j)[, {"dims": int32 [R], the retained
    dimensions, "eigenvalues": a list of [min(N_r, D)] arrays, descending}]."""
    x, offsets = dense_pca_args(engine, x, offsets, target_energy)
    r, t = len(offsets) - 1, int(offsets[-1])
    sizes = np.diff(offsets)
    block_off = offsets_of(sizes * sizes)
    scores = np.empty(int(block_off[-1]), np.float32)
    dims = np.empty(r, np.int32) if return_info else None
    eig = np.empty(t, np.float64) if return_info else None
    N.check(engine._h, engine._lib.plda_score_dense_pca(engine._h, _p(x), _p(offsets), r, float(target_energy), _p(scores),
                                                        _p(block_off), _p(dims), _p(eig)))
    blocks = [scores[block_off[q]:block_off[q + 1]].reshape(int(sizes[q]), int(sizes[q])) for q in range(r)]
    if not return_info:
        return blocks
    m = np.minimum(sizes, x.shape[1])
    return blocks, {"dims": dims, "eigenvalues": [eig[offsets[q]:offsets[q] + m[q]] for q in range(r)]}


def ahc_dense_pca(engine, x, offsets, target_energy, threshold=0.0, num_speakers=None, return_merges=False):
    """score_dense_pca's blocks clustered on the device and dropped: (labels, n_clusters[, merges]) as ahc() returns them on
    those blocks."""
    has_t, thr, minc = stop_args(np.ascontiguousarray(offsets, np.int64), threshold, num_speakers)
    x, offsets = dense_pca_args(engine, x, offsets, target_energy)
    r, t = len(offsets) - 1, int(offsets[-1])
    labels, ncl, ma, mb, mc = _outputs(t, r, return_merges)
    N.check(engine._h, engine._lib.plda_score_dense_pca_ahc(engine._h, _p(x), _p(offsets), r, float(target_energy), has_t, thr,
                                                            _p(minc), _p(labels), _p(ncl), _p(ma), _p(mb), _p(mc)))
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


# ------------------------------------------------------------------------------------------- VBx resegmentation
def vbx_plan(engine, t, s, d):
    """{"cls": 0 (state in LDS) or 1 (state in HBM scratch), "scratch_bytes": per recording, "lds_doubles": the LDS class's
    limit in doubles of state} of a recording of t segments, s initial speakers and dimension d."""
    out = (C.c_int32 * 3)()
    N.check(engine._h, engine._lib.plda_vbx_plan(engine._h, int(t), int(s), int(d), out))
    return {"cls": int(out[0]), "scratch_bytes": int(out[1]), "lds_doubles": int(out[2])}


def vbx_args(y, offsets, labels, phi, Fa, Fb, loop_prob, max_iters):
    """The argument check of vbx / MPlda.resegment, before any device work -> (y, offsets, labels, phi, S of every recording).
    ValueError on anything the C ABI would answer with PLDA_E_INVAL and that the host can see."""
    y = np.ascontiguousarray(y, np.float64)
    offsets = np.ascontiguousarray(offsets, np.int64)
    labels = np.ascontiguousarray(labels, np.int32)
    if offsets.ndim != 1 or len(offsets) < 2:
        raise ValueError("offsets must hold R + 1 >= 2 entries")
    if offsets[0] != 0:
        raise ValueError("offsets must start at 0")
    sizes = np.diff(offsets)
    if (sizes < 1).any() or (sizes > AHC_MAX).any():
        raise ValueError("every recording must hold 1 ... %d segments (offsets must ascend)" % AHC_MAX)
    if y.ndim != 2 or y.shape[0] != int(offsets[-1]) or y.shape[1] < 1:
        raise ValueError("y must be [offsets[-1], D], got %r" % (y.shape,))
    if labels.shape != (y.shape[0],):
        raise ValueError("labels must hold one entry per row of y, got %r" % (labels.shape,))
    if (labels < 0).any() or (labels >= VBX_MAX_SPK).any():
        raise ValueError("labels must lie in [0, %d)" % VBX_MAX_SPK)
    if not np.isfinite(y).all():
        raise ValueError("y holds non-finite values")
    if phi is not None:
        phi = np.ascontiguousarray(phi, np.float64)
        if phi.shape != (y.shape[1],):
            raise ValueError("phi must hold D = %d entries, got %r" % (y.shape[1], phi.shape))
        if not (np.isfinite(phi).all() and (phi >= 0).all()):
            raise ValueError("phi must be finite and >= 0")
    if not (Fa > 0 and np.isfinite(Fa)):
        raise ValueError("Fa must be > 0")
    if not (Fb > 0 and np.isfinite(Fb)):
        raise ValueError("Fb must be > 0")
    if not 0 <= loop_prob < 1:
        raise ValueError("loop_prob must lie in [0, 1)")
    if int(max_iters) != max_iters or max_iters < 1:
        raise ValueError("max_iters must be an integer >= 1")
    spk = np.maximum.reduceat(labels, offsets[:-1]).astype(np.int64) + 1
    return y, offsets, labels, phi, spk


def vbx(engine, y, offsets, labels, phi=None, Fa=0.3, Fb=17.0, loop_prob=0.99, init_smoothing=5.0, max_iters=40, epsilon=1e-4,
        return_posteriors=False, return_second=False):
    """VBx resegmentation of R recordings: y [T, D] segment vectors in the model's diagonalised space WITHOUT length
    normalisation (MPlda.project_rows), recording r owning rows offsets[r] .. offsets[r+1], `labels` the initial labels (the
    AHC's), phi [D] the between-class variance (None: the model's psi).  Returns (labels int32 [T], n_clusters int32 [R][, info]),
    labels 0 .. k-1 per recording by ascending smallest member; info = {"gamma": a list of [T_r, S_r] arrays (columns in the
    initial numbering), "pi": a list of [S_r] arrays, "elbo": [R, max_iters] (NaN from iters[r] on), "iters": int32 [R]}.
    return_second=True: (labels, n_clusters, labels2 int32 [T], post2 float64 [T][, info]) -- the second most likely speaker
    of every segment among those that are some segment's first choice, numbered as labels, and its posterior; -1 and 0 in a
    recording with one speaker (plda_vbx_top2; the VBx recipe's --output-2nd).  apply_overlap decides where to use it."""
    y, offsets, labels, phi, spk = vbx_args(y, offsets, labels, phi, Fa, Fb, loop_prob, max_iters)
    r, t = len(offsets) - 1, int(offsets[-1])
    out_l, out_k = np.empty(t, np.int32), np.empty(r, np.int32)
    gamma = goff = pi = poff = elbo = iters = None
    if return_posteriors:
        goff, poff = offsets_of(np.diff(offsets) * spk), offsets_of(spk)
        gamma, pi = np.empty(int(goff[-1]), np.float64), np.empty(int(poff[-1]), np.float64)
        elbo, iters = np.empty((r, int(max_iters)), np.float64), np.empty(r, np.int32)
    args = (engine._h, _p(y), y.shape[1], _p(phi), _p(labels), _p(offsets), r, float(Fa), float(Fb), float(loop_prob),
            float(init_smoothing), int(max_iters), float(epsilon), _p(out_l), _p(out_k), _p(gamma), _p(goff), _p(pi), _p(poff), _p(elbo),
            _p(iters))
    out = (out_l, out_k)
    if return_second:
        out_l2, out_p2 = np.empty(t, np.int32), np.empty(t, np.float64)
        N.check(engine._h, engine._lib.plda_vbx_top2(*args, _p(out_l2), _p(out_p2)))
        out += (out_l2, out_p2)
    else:
        N.check(engine._h, engine._lib.plda_vbx(*args))
    if not return_posteriors:
        return out
    sizes = np.diff(offsets)
    info = {"gamma": [gamma[goff[q]:goff[q + 1]].reshape(int(sizes[q]), int(spk[q])) for q in range(r)],
            "pi": [pi[poff[q]:poff[q + 1]] for q in range(r)], "elbo": elbo, "iters": iters}
    return out + (info,)


def apply_overlap(labels2, post2, overlap=None, min_posterior=None):
    """Where the second speaker of vbx(..., return_second=True) is kept: labels2[t] where overlap[t] holds (an external
    overlap detector's per-segment bool mask), and also where post2[t] >= min_posterior; -1 everywhere else.  At least one of
    the two must be given.  Returns int32 [T], what der.der_timed takes as hyp2 and rttm.write as labels2.  Pure NumPy."""
    if overlap is None and min_posterior is None:
        raise ValueError("apply_overlap needs overlap, min_posterior or both")
    labels2 = np.asarray(labels2)
    post2 = np.asarray(post2, np.float64)
    if labels2.ndim != 1 or labels2.dtype.kind not in "iu" or post2.shape != labels2.shape:
        raise ValueError("labels2 (integer) and post2 must be 1-D arrays of one length")
    keep = np.zeros(labels2.shape, bool)
    if overlap is not None:
        overlap = np.asarray(overlap)
        if overlap.dtype != np.bool_ or overlap.shape != labels2.shape:
            raise ValueError("overlap must be a bool mask with one entry per segment")
        keep |= overlap
    if min_posterior is not None:
        if isinstance(min_posterior, bool) or not isinstance(min_posterior, (int, float, np.integer, np.floating)) or np.isnan(min_posterior):
            raise ValueError("min_posterior must be a number")
        keep |= post2 >= float(min_posterior)
    return np.where(keep & (labels2 >= 0), labels2, -1).astype(np.int32)
