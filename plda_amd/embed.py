"""plda_amd/embed.py -- the embedding chain in front of a PLDA model (K18; include/plda_hip.h, "embedding chain"):

    v = x - m_in;  v <- v len_in / |v|;  u = A v;  u <- u - m_out;  u <- u len_out / |u|          (each part optional)

`EmbeddingChain` is the plain host object; `MPlda.set_embedding` / `fit_embedding` / `embed` put it on the device.
"""
import math

import numpy as np

MAX_DIN = 4096     # PLDA_EMBED_MAX_DIN
MAX_DOUT = 2048    # PLDA_EMBED_MAX_DOUT

KINDS = {"centre": 0, "whiten": 1, "lda": 2}

# name -> (kind, len_in, len_out); len_out None = sqrt(dim)
_RECIPES = {
    "centre-norm": ("centre", 0.0, None),    # subtract the mean, length-normalise to sqrt(D)
    "kaldi-lda": ("lda", 0.0, None),         # ivector-subtract-global-mean | transform-vec lda | ivector-normalize-length
    "kaldi-whiten": ("whiten", 0.0, None),   # the same with a whitening (PCA) matrix
    "vbx": ("lda", 1.0, 1.0),                # l2(LDA l2(x - m1) - m2)
}


def recipe(name):
    """-> (kind, len_in, len_out) of "centre-norm", "kaldi-lda", "kaldi-whiten" or "vbx" (len_out None: sqrt(dim))."""
    try:
        return _RECIPES[name]
    except KeyError:
        raise ValueError("unknown embedding recipe %r (one of %s)" % (name, ", ".join(sorted(_RECIPES))))


def _vec(a, name):
    if a is None:
        return None
    a = np.array(a, dtype=np.float64, order="C", copy=True)
    if a.ndim != 1 or a.shape[0] == 0:
        raise ValueError("EmbeddingChain: %s must be a non-empty 1-dimensional array" % name)
    if not np.all(np.isfinite(a)):
        raise ValueError("EmbeddingChain: %s has a non-finite element" % name)
    return a


def _length(v, name):
    v = float(v)
    if not math.isfinite(v) or v < 0.0:
        raise ValueError("EmbeddingChain: %s must be finite and >= 0, got %r" % (name, v))
    return v


class EmbeddingChain(object):
    """(m_in [Din] | None, len_in, A [Dout, Din] | None, m_out [Dout] | None, len_out); `din`, `dout`.  At least one of
    m_in, A, m_out must be given (it fixes the dimension), or `dim`."""

    def __init__(self, m_in=None, len_in=0.0, A=None, m_out=None, len_out=0.0, dim=None):
        self.m_in = _vec(m_in, "m_in")
        self.m_out = _vec(m_out, "m_out")
        self.len_in = _length(len_in, "len_in")
        self.len_out = _length(len_out, "len_out")
        self.A = None
        self.eig = None        # eigenvalues of the fit that made the chain (MPlda.fit_embedding), else None
        if A is not None:
            A = np.array(A, dtype=np.float64, order="C", copy=True)
            if A.ndim != 2 or A.shape[0] == 0 or A.shape[1] == 0:
                raise ValueError("EmbeddingChain: A must be a non-empty 2-dimensional array [Dout, Din]")
            if not np.all(np.isfinite(A)):
                raise ValueError("EmbeddingChain: A has a non-finite element")
            self.A = A
            self.dout, self.din = A.shape
        else:
            d = self.m_in.shape[0] if self.m_in is not None else self.m_out.shape[0] if self.m_out is not None else dim
            if d is None:
                raise ValueError("EmbeddingChain: without m_in, A and m_out the dimension `dim` is needed")
            self.din = self.dout = int(d)
        if dim is not None and int(dim) != self.din:
            raise ValueError("EmbeddingChain: dim %d != the input dimension %d" % (int(dim), self.din))
        if self.m_in is not None and self.m_in.shape[0] != self.din:
            raise ValueError("EmbeddingChain: m_in has %d elements, the input dimension is %d" % (self.m_in.shape[0], self.din))
        if self.m_out is not None and self.m_out.shape[0] != self.dout:
            raise ValueError("EmbeddingChain: m_out has %d elements, the output dimension is %d" % (self.m_out.shape[0], self.dout))
        if not 1 <= self.din <= MAX_DIN:
            raise ValueError("EmbeddingChain: input dimension %d outside 1 ... %d" % (self.din, MAX_DIN))
        if not 1 <= self.dout <= MAX_DOUT:
            raise ValueError("EmbeddingChain: output dimension %d outside 1 ... %d" % (self.dout, MAX_DOUT))

    @classmethod
    def from_kaldi(cls, mean_path, transform_path=None, normalize_length=True):
        """Kaldi's ivector-subtract-global-mean mean.vec | transform-vec transform.mat | ivector-normalize-length: m_in from
        `mean_path`, A from `transform_path` (None: no matrix); a matrix with Din + 1 columns carries an offset column,
        which becomes m_out = -offset; normalize_length: len_out = sqrt(Dout)."""
        from . import kaldi_io
        m_in = kaldi_io.read_vector(mean_path)
        A, m_out = None, None
        if transform_path is not None:
            A = kaldi_io.read_matrix(transform_path)
            if A.ndim != 2 or A.shape[1] not in (m_in.shape[0], m_in.shape[0] + 1):
                raise ValueError("from_kaldi: the transform has %s columns, the mean %d elements" % (A.shape[1:], m_in.shape[0]))
            if A.shape[1] == m_in.shape[0] + 1:
                m_out = -A[:, -1]
                A = A[:, :-1]
        dout = A.shape[0] if A is not None else m_in.shape[0]
        return cls(m_in, 0.0, A, m_out, math.sqrt(dout) if normalize_length else 0.0)

    def __repr__(self):
        return "EmbeddingChain(din=%d, dout=%d, m_in=%s, len_in=%r, A=%s, m_out=%s, len_out=%r)" % (
            self.din, self.dout, self.m_in is not None, self.len_in, self.A is not None, self.m_out is not None, self.len_out)
