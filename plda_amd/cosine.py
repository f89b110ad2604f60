"""plda_amd/cosine.py -- `Cosine`: the cosine back-end behind MPlda's scoring interface (K27; csrc/cosine.hip).

A Cosine object is an MPlda whose handle was switched with plda_backend_set(h, PLDA_BACKEND_COSINE, dim): it holds no PLDA
model, a score is the cosine of the two vectors (length-normalised on the device, in fp64, before the one rounding to the
trials GEMM's fp32 operands), and everything behind the score is MPlda's own: score_matrix, score_trials,
score_matrix_asnorm, top_n, min_dcf, min_cllr, calibrate*, fuse, evaluate, partition, cluster (AHC and spectral), cluster_corpus and the
*_dev methods, unchanged.
"""
import ctypes as C

import numpy as np

from .libplda import MPlda, Transformed, _labels, _npz_path

BACKEND_PLDA, BACKEND_COSINE = 0, 1
_NEEDS_MODEL = "%s needs a PLDA model; this is a cosine back-end, which has none (use MPlda)"


class Cosine(MPlda):
    """Cosine scoring of `dim`-dimensional embeddings on GPU `device`."""

    def __init__(self, dim, device=0, diag=None):
        MPlda.__init__(self, device, diag)
        self._ck(self._lib.plda_backend_set(self._h, BACKEND_COSINE, int(dim)))
        self.dim = int(dim)

    def backend(self):
        """(kind, dim) of the handle: (1, dim)."""
        k, d = C.c_int32(), C.c_int32()
        self._ck(self._lib.plda_backend_get(self._h, C.byref(k), C.byref(d)))
        return k.value, d.value

    # ------------------------------------------------------------------ what needs a PLDA model
    def fit(self, *a, **kw):
        raise ValueError(_NEEDS_MODEL % "fit")

    def adapt(self, *a, **kw):
        raise ValueError(_NEEDS_MODEL % "adapt")

    def adapt_clustered(self, *a, **kw):
        raise ValueError(_NEEDS_MODEL % "adapt_clustered")

    def resegment(self, *a, **kw):
        raise ValueError(_NEEDS_MODEL % "resegment")

    def diarize(self, *a, **kw):
        raise ValueError(_NEEDS_MODEL % "diarize")

    def score_dense(self, *a, **kw):
        raise ValueError(_NEEDS_MODEL % "score_dense")

    # ------------------------------------------------------------------ embedding chain
    def fit_embedding(self, x, y=None, kind="lda", dim=None, len_in=0.0, len_out=None):
        """MPlda.fit_embedding, and kind="wccn": within-class covariance normalisation, A with A W A^T = I.  Under a cosine
        score WCCN and full-rank LDA differ by a rotation, to which a cosine is invariant, so "wccn" fits kind "lda" at
        dim = Din (a `dim` below Din is refused: that would be LDA, not WCCN)."""
        if kind == "wccn":
            if not isinstance(x, np.ndarray) or x.ndim != 2:
                raise ValueError("Input features must be 2-dimensional (nsamples, featdim)")
            if dim is not None and int(dim) != x.shape[1]:
                raise ValueError("fit_embedding: kind 'wccn' keeps every dimension (dim = %d, Din = %d); use kind 'lda' to reduce" % (int(dim), x.shape[1]))
            kind, dim = "lda", x.shape[1]
        return MPlda.fit_embedding(self, x, y, kind, dim, len_in, len_out)

    # ------------------------------------------------------------------ enrolment
    def transform(self, x, y):
        """{label: (n, ndarray f64[dim])} in ascending label order, as MPlda.transform returns it: a label's model is the mean
        of its length-normalised rows (the usual multi-session enrolment), n its number of rows.  The rows are stable-sorted
        by label on the host and pooled on the device (plda_dvector_pool: mean, l2norm).  An all-zero row makes its label's
        model NaN, as the pooling defines it."""
        if not isinstance(x, np.ndarray):
            raise TypeError("argument 1 must be numpy.ndarray, not %s" % type(x).__name__)
        X = np.ascontiguousarray(x, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("Input features must be 2-dimensional (nsamples, featdim)")
        X = self._embedded(x, X)
        n, d = X.shape
        if d != self.dim:
            raise ValueError("transform: rows have %d features, the back-end was created for %d" % (d, self.dim))
        Y = _labels(y, n, allow_strings_msg=True)
        order = np.argsort(Y, kind="stable")
        labels, counts = np.unique(Y, return_counts=True)
        g = labels.shape[0]
        offsets = np.zeros(g + 1, np.int64)
        np.cumsum(counts, out=offsets[1:])
        rows = np.ascontiguousarray(X[order])
        vecs = np.empty((g, d), np.float64)
        if g:
            self._ck(self._lib.plda_dvector_pool(self._h, C.c_void_p(rows.ctypes.data), 1, n, d, C.c_void_p(offsets.ctypes.data), g, 0, 1,
                                                 C.c_void_p(vecs.ctypes.data)))
        res = Transformed(zip(labels.tolist(), zip(counts.tolist(), vecs)))
        res._packed = (labels.astype(np.int64), counts.astype(np.int32), vecs)
        return res

    def transform_array(self, xbar, num_examples=1):
        """The rows themselves, float64 [R, dim]: a cosine model vector needs no projection (the scoring entry points
        length-normalise).  What `cluster` calls on its segment vectors."""
        return self._check_dim(np.ascontiguousarray(xbar, np.float64))

    # ------------------------------------------------------------------ z-norm
    def norm(self, vectors, enrol, numutts=0):
        """Z-norm statistics of every model of `enrol` (transform()'s dict) against the cohort rows `vectors` [Nb, dim]: mean
        and population std of its cosines with ALL of them -- cohort_stats(enrol, vectors, top_k=None) -- stored insert-once
        as MPlda.norm stores them.  numutts: the first `numutts` rows of a fixed-seed permutation, as there.  Returns None."""
        if not isinstance(vectors, np.ndarray):
            raise TypeError("argument 1 must be numpy.ndarray, not %s" % type(vectors).__name__)
        if not isinstance(enrol, dict):
            raise TypeError("argument 2 must be dict, not %s" % type(enrol).__name__)
        bkg = self._embedded(vectors, np.ascontiguousarray(vectors, np.float64))
        if bkg.ndim != 2 or bkg.shape[1] != self.dim:
            raise ValueError("norm: cohort vectors must be [rows, %d], got %s" % (self.dim, tuple(bkg.shape)))
        if numutts and int(numutts) < bkg.shape[0]:
            sel = np.sort(np.random.default_rng(0).permutation(bkg.shape[0])[: int(numutts)])
            bkg = np.ascontiguousarray(bkg[sel])
        if not enrol:
            return None
        ids = self._unpack(enrol)[0]
        mean, std = self.cohort_stats(enrol, bkg, top_k=None)
        for k, m, s in zip(ids.tolist(), mean.tolist(), std.tolist()):
            if k not in self._meanz:
                self._meanz[k] = m
                self._stdvz[k] = s
        return None

    # ------------------------------------------------------------------ persistence
    def save(self, path):
        """Back-end, dimension, z-norm statistics, calibration and embedding chain to .npz (MPlda.save without the model)."""
        ids = np.array(sorted(self._meanz), dtype=np.int64)
        extra = {}
        if self._calibration is not None:
            c = self._calibration
            extra = {"calib_a": np.float64(c.a), "calib_b": np.float64(c.b), "calib_prior": np.float64(c.prior)}
        if self._embedding is not None:
            e = self._embedding
            none = np.zeros(0)
            extra.update(embed_m_in=none if e.m_in is None else e.m_in, embed_len_in=np.float64(e.len_in),
                         embed_A=np.zeros((0, e.din)) if e.A is None else e.A, embed_m_out=none if e.m_out is None else e.m_out,
                         embed_len_out=np.float64(e.len_out))
        np.savez(_npz_path(path), backend=np.array("cosine"), dim=np.int64(self.dim), zn_ids=ids,
                 zn_mean=np.array([self._meanz[i] for i in ids], dtype=np.float64),
                 zn_std=np.array([self._stdvz[i] for i in ids], dtype=np.float64), **extra)

    def load(self, path):
        z = np.load(_npz_path(path, for_load=True))
        if "backend" not in z.files or str(z["backend"]) != "cosine":
            raise ValueError("load: %s does not hold a cosine back-end (a PLDA model file belongs to MPlda.load)" % (path,))
        if int(z["dim"]) != self.dim:
            raise ValueError("load: the file's dimension %d is not this back-end's %d" % (int(z["dim"]), self.dim))
        self._meanz = {int(i): float(v) for i, v in zip(z["zn_ids"], z["zn_mean"])}
        self._stdvz = {int(i): float(v) for i, v in zip(z["zn_ids"], z["zn_std"])}
        self._zn_tag = None
        self._calibration = None
        if "calib_a" in z.files:
            from .calibration import Calibration
            self._calibration = Calibration(float(z["calib_a"]), float(z["calib_b"]), float(z["calib_prior"]))
        chain = None
        if "embed_A" in z.files:
            from .embed import EmbeddingChain
            A, m_in, m_out = z["embed_A"], z["embed_m_in"], z["embed_m_out"]
            chain = EmbeddingChain(m_in if m_in.size else None, float(z["embed_len_in"]), A if A.size else None,
                                   m_out if m_out.size else None, float(z["embed_len_out"]), dim=A.shape[1])
        self.set_embedding(chain)
        return self
