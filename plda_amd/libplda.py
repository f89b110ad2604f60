"""plda_amd/libplda.py -- `MPlda`, counterpart of the reference's CPython type
`libplda.MPlda` (/root/reference/src/pldamodule.cpp:280-295: fit / transform / norm /
score), calling the C ABI of libplda_hip.so through ctypes.

Same method names, argument meaning, defaults, return shapes and error behaviour as
the reference (file:line cited per method); the arithmetic runs in hand-written HIP
kernels on an MI355X.  Batched extensions (`transform_array`, `score_matrix`,
`score_trials`) expose what the reference's callers loop over in Python.
"""
import ctypes as C
import threading

import numpy as np

from . import _native as N

_ERR_LABELS_UNSIGNED = "Given labels (argument 2) are not an unsigned! Set the dtype to uint!"  # pldamodule.cpp:56,134
_ERR_X_FLOAT = "Given Input features (argument 1) are not floats! Set the dtype to float!"      # pldamodule.cpp:60
_ERR_LABELS_STR = "Labels need to be numpy array of uints, not strings!"                         # pldamodule.cpp:129
_ERR_ONE_SPK = ("Number of speakers is 1. Aborting PLDA esimation, at least two speakers are "   # pldamodule.cpp:84
                "required!")


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _vp(x):
    """A raw device address as a void pointer; None (or 0): NULL."""
    return C.c_void_p(int(x)) if x else None


def _features(x, what="Input features"):
    if not isinstance(x, np.ndarray):
        raise TypeError("argument 1 must be numpy.ndarray, not %s" % type(x).__name__)  # "O!" parse
    if x.dtype.kind != "f":
        raise ValueError(_ERR_X_FLOAT)
    if x.ndim != 2:
        raise ValueError("%s must be 2-dimensional (nsamples, featdim)" % what)
    # the reference reads the buffer as C-contiguous f64 regardless of dtype/strides
    # (kaldi-utils.hpp:99-111, quirk Q12); coercing is a strict superset of that
    return np.ascontiguousarray(x, dtype=np.float64)


def _labels(y, n, allow_strings_msg=False):
    if not isinstance(y, np.ndarray):
        raise TypeError("argument 2 must be numpy.ndarray, not %s" % type(y).__name__)
    if allow_strings_msg and y.dtype.kind in "SU":
        raise ValueError(_ERR_LABELS_STR)
    if y.dtype.kind != "u":
        raise ValueError(_ERR_LABELS_UNSIGNED)
    y = np.ascontiguousarray(y).reshape(-1).astype(np.uint64, copy=False)
    if y.shape[0] != n:
        raise ValueError("labels and features disagree on the number of samples")  # assert at :68,137
    return np.ascontiguousarray(y)


def _npz_path(path, for_load=False):
    """np.savez appends '.npz' to a path without that suffix and np.load does not: normalise, so that
    save('model') / load('model') round-trip.  On load an existing file of exactly that name wins (a model
    written through a file object may have any name).  File objects pass through."""
    if isinstance(path, (str, bytes)) or hasattr(path, "__fspath__"):
        import os
        p = os.fspath(path)
        if isinstance(p, bytes):
            p = p.decode()
        if for_load and os.path.exists(p):
            return p
        return p if p.endswith(".npz") else p + ".npz"
    return path


def _compact_labels(Y):
    """Labels -> dense 0..K-1 in ascending label order (what np.unique(return_inverse=True) gives), and K.  np.unique
    sorts: 4.2 ms for 100k labels, more than the fit itself.  Labels are small integers in practice (the reference
    indexes an array by them), so count instead: 0.2 ms, and already-dense labels pass through untouched."""
    n = Y.shape[0]
    if n == 0:
        return Y, 0                                   # plda_fit reports the empty input (PLDA_E_INVAL), not NumPy's max()
    top = int(Y.max())
    if top < 16 * n + 1024:
        signed = Y.view(np.int64)                     # (top < 2^63: same values)
        present = np.bincount(signed, minlength=top + 1) > 0
        k = int(np.count_nonzero(present))
        if k == top + 1:
            return Y, k
        remap = np.cumsum(present, dtype=np.int64) - 1
        return np.ascontiguousarray(remap[signed].astype(np.uint64)), k
    uniq, inv = np.unique(Y, return_inverse=True)
    return np.ascontiguousarray(inv.astype(np.uint64)), int(uniq.shape[0])


class Transformed(dict):
    """What `transform()` returns: the reference's dict {label: (n, ndarray f64[D])} (pldamodule.cpp:162-191), which also
    remembers the three arrays it was built from -- labels, counts and the [Ku, D] block the row views point into -- so that
    `score_matrix` / `score_trials` / `norm` take them as they are instead of re-stacking Ku rows in Python (2 000 entries: ~1 ms,
    more than the GPU call).  Any change of the KEYS drops the memory and the dict is unpacked like any other; the rows are
    views, so writing into a vector is seen either way."""
    __slots__ = ("_packed",)

    def _forget(self):
        self._packed = None

    def __setitem__(self, k, v):
        self._forget(); dict.__setitem__(self, k, v)

    def __delitem__(self, k):
        self._forget(); dict.__delitem__(self, k)

    def pop(self, *a):
        self._forget(); return dict.pop(self, *a)

    def popitem(self):
        self._forget(); return dict.popitem(self)

    def clear(self):
        self._forget(); dict.clear(self)

    def update(self, *a, **kw):
        self._forget(); dict.update(self, *a, **kw)

    def setdefault(self, *a):
        self._forget(); return dict.setdefault(self, *a)

    def __ior__(self, other):
        self._forget(); return dict.__ior__(self, other)

    def __reduce__(self):          # pickles and deep copies are ordinary dicts (the block and its row views would part)
        return (dict, (dict(self),))


class MPlda(object):
    """GPU-resident PLDA model + z-norm statistics (MPlda struct, pldamodule.cpp:27-34)."""

    def __init__(self, device=0, diag=None):
        self._lib = N.load(diag)        # diag=True: the diagnostic build (measurement arms; profiling scripts only)
        h = C.c_void_p()
        rc = self._lib.plda_create(int(device), C.byref(h))
        if rc != N.PLDA_OK:
            msg = self._lib.plda_last_error(None)      # (this library's own thread-local message: it may be the diagnostic build)
            raise N.PldaError(rc, msg.decode("utf-8", "replace") if msg else "")
        self._h = h
        self.device = int(device)
        # std::unordered_map<long,double> *meanz, *stdvz (pldamodule.cpp:33)
        self._meanz = {}
        self._stdvz = {}
        self._calibration = None      # plda_amd.calibration.Calibration of the last calibrate() / load()
        self.pav = None               # plda_amd.rocch.Pav of the last calibrate_pav()
        self._embedding = None        # plda_amd.embed.EmbeddingChain in front of the raw-row methods (set_embedding / fit_embedding)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._lib.plda_destroy(h)
            except Exception:
                pass
            self._h = None

    def _ck(self, rc):
        N.check(self._h, rc)

    # ------------------------------------------------------------------ embedding chain (csrc/embed.hip)
    def set_embedding(self, chain):
        """Attach an EmbeddingChain (plda_amd/embed.py), or None to remove it.  While one is attached, the raw-row methods --
        fit, transform, norm (its `vectors`), adapt, adapt_accumulate, cluster, resegment, diarize, project_rows,
        tune_threshold -- pass their rows through it first, on the device: centre, length-normalise, project, re-centre,
        length-normalise (K18).  The host-array methods go through the host entry point, which costs one extra PCIe round
        trip (the embedded rows come back and go down again); callers with rows in HBM chain embed_dev into the _dev entry
        points and never leave it.  The _dev methods never apply the chain themselves."""
        if chain is None:
            self._ck(self._lib.plda_embed_clear(self._h))
            self._embedding = None
            return
        from .embed import EmbeddingChain
        if not isinstance(chain, EmbeddingChain):
            raise TypeError("set_embedding: an EmbeddingChain or None is needed, not %s" % type(chain).__name__)
        self._ck(self._lib.plda_embed_set(self._h, chain.din, chain.dout, _ptr(chain.m_in), chain.len_in, _ptr(chain.A),
                                          _ptr(chain.m_out), chain.len_out))
        self._embedding = chain

    @property
    def embedding(self):
        """The attached EmbeddingChain, or None."""
        return self._embedding

    def _read_embedding(self):
        from .embed import EmbeddingChain
        a, b, f = C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._lib.plda_embed_dims(self._h, C.byref(a), C.byref(b), C.byref(f)))
        din, dout, flags = a.value, b.value, f.value
        m_in = np.zeros(din) if flags & 1 else None
        A = np.zeros((dout, din)) if flags & 2 else None
        m_out = np.zeros(dout) if flags & 4 else None
        li, lo = C.c_double(), C.c_double()
        self._ck(self._lib.plda_embed_get(self._h, _ptr(m_in), C.byref(li), _ptr(A), _ptr(m_out), C.byref(lo)))
        return EmbeddingChain(m_in, li.value, A, m_out, lo.value, dim=din)

    def fit_embedding(self, x, y=None, kind="lda", dim=None, len_in=0.0, len_out=None):
        """Estimate a chain from rows x [N, Din] on the device and attach it: m_in = the column mean, then kind "centre"
        (m_out = the mean after the first length normalisation), "whiten" (A = the `dim` leading principal directions scaled
        to unit variance) or "lda" (labels y; A W A^T = I, A B A^T diagonal, the `dim` leading directions).  dim None: Din;
        len_out None: sqrt(dim).  fp32 rows go down as fp32.  Returns the EmbeddingChain; its `eig` holds the eigenvalues
        (None for "centre").  On an error the attached chain stays as it was."""
        from .embed import KINDS
        if kind not in KINDS:
            raise ValueError("fit_embedding: kind %r (one of %s)" % (kind, ", ".join(sorted(KINDS))))
        X, dtype = self._embed_input(x)
        n, d = X.shape
        dim = d if dim is None else int(dim)
        lo = float(np.sqrt(dim)) if len_out is None else float(len_out)
        dense = None
        if KINDS[kind] == 2:
            if y is None:
                raise ValueError("fit_embedding: kind 'lda' needs labels y")
            dense, _ = _compact_labels(_labels(y, n))
        eig = np.zeros(max(dim, 1))
        self._ck(self._lib.plda_embed_fit(self._h, _ptr(X), dtype, n, d, _ptr(dense), KINDS[kind], dim, float(len_in), lo, _ptr(eig)))
        chain = self._read_embedding()
        chain.eig = eig[:dim].copy() if KINDS[kind] else None
        self._embedding = chain
        return chain

    @staticmethod
    def _embed_input(x):
        if not isinstance(x, np.ndarray):
            raise TypeError("argument 1 must be numpy.ndarray, not %s" % type(x).__name__)
        if x.dtype.kind != "f":
            raise ValueError(_ERR_X_FLOAT)
        if x.ndim != 2:
            raise ValueError("Input features must be 2-dimensional (nsamples, featdim)")
        if x.dtype == np.float32:
            return np.ascontiguousarray(x), 1            # fp32 goes down as fp32: the kernel widens it at the load
        return np.ascontiguousarray(x, dtype=np.float64), 0

    def embed(self, x):
        """The attached chain applied to rows x [R, Din] (fp32 or fp64) -> float64 [R, Dout]."""
        if self._embedding is None:
            raise ValueError("embed: no embedding is set (set_embedding / fit_embedding)")
        X, dtype = self._embed_input(x)
        r, d = X.shape
        if d != self._embedding.din:
            raise ValueError("embed: rows have %d features, the embedding takes %d" % (d, self._embedding.din))
        out = np.empty((r, self._embedding.dout), np.float64)
        self._ck(self._lib.plda_embed_apply(self._h, _ptr(X), dtype, r, d, _ptr(out)))
        return out

    def embed_dev(self, dX, dtype, R, Din, dout):
        """The same on HBM-resident rows (raw device addresses): dX [R, Din] of dtype (0 fp64, 1 fp32), dout fp64 [R, Dout]."""
        self._ck(self._lib.plda_embed_apply_dev(self._h, C.c_void_p(int(dX)), int(dtype), int(R), int(Din), C.c_void_p(int(dout))))

    def _embedded(self, x, X, check_model=True):
        """The one hook of the raw-row methods: X (the float64 rows the method made of its argument x) as it is when no chain
        is attached, else the chain applied to x (as fp32 if x is fp32)."""
        chain = self._embedding
        if chain is None:
            return X
        if check_model:
            try:
                din = self.dims()[1]
            except N.PldaError:
                din = None           # no model yet: the method's own call reports it
            if din is not None and chain.dout != din:
                raise ValueError("the embedding's output dimension %d is not the model's input dimension %d" % (chain.dout, din))
        fp32 = isinstance(x, np.ndarray) and x.dtype == np.float32 and x.ndim == 2
        return self.embed(x if fp32 else X)

    def _rows(self, x, what="Input features", check_model=True):
        return self._embedded(x, _features(x, what), check_model)

    # ------------------------------------------------------------------ fit
    def fit(self, x, y, iters=10):
        """MPlda_fit (pldamodule.cpp:42-109).  Returns None."""
        self._dout = None            # the model dimension may change
        X = self._rows(x, check_model=False)
        n, d = X.shape
        Y = _labels(y, n)
        # the reference indexes a VLA by label value (:88-92, quirk Q2): labels must be
        # dense 0..K-1.  Compacting with unique() is the same thing for dense labels.
        dense, k = _compact_labels(Y)
        if k == 1:
            raise ValueError(_ERR_ONE_SPK)
        rc = self._lib.plda_fit(self._h, _ptr(X), n, d, _ptr(dense), int(iters))
        if rc == N.PLDA_E_ONE_SPEAKER:
            raise ValueError(_ERR_ONE_SPK)
        self._ck(rc)
        return None

    def fit_timings(self):
        """ms of the last fit: dict(stats, em, output, iters)."""
        t = np.zeros(4)
        self._ck(self._lib.plda_fit_timings(self._h, _ptr(t)))
        return dict(stats_ms=t[0], em_ms=t[1], output_ms=t[2], iters=int(t[3]))

    def fit_plan(self):
        """How the EM of the last fit ran: dict(groups = distinct utterance counts, form = "basis" | "moments" | "rows")."""
        p = np.zeros(2, np.int32)
        self._ck(self._lib.plda_fit_plan(self._h, _ptr(p)))
        return dict(groups=int(p[0]), form=("basis", "moments", "rows")[int(p[1])])

    def fit_internals(self):
        """means/counts/scatter/sum/W/B of the last fit (parity tests)."""
        k = C.c_int64()
        self._ck(self._lib.plda_fit_num_classes(self._h, C.byref(k)))
        K = k.value
        _, d = self.dims()
        means, counts = np.zeros((K, d)), np.zeros(K, np.int64)
        scatter, s, W, B = np.zeros((d, d)), np.zeros(d), np.zeros((d, d)), np.zeros((d, d))
        self._ck(self._lib.plda_fit_get_stats(self._h, _ptr(means), _ptr(counts), _ptr(scatter), _ptr(s),
                                              _ptr(W), _ptr(B)))
        return dict(means=means, counts=counts, scatter=scatter, sum=s, W=W, B=B)

    # ---------------------------------------------------------------- model
    def dims(self):
        a, b = C.c_int32(), C.c_int32()
        self._ck(self._lib.plda_get_dims(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def get_model(self):
        dout, din = self.dims()
        mean, T, psi, off = np.zeros(din), np.zeros((dout, din)), np.zeros(dout), np.zeros(dout)
        self._ck(self._lib.plda_get_model(self._h, _ptr(mean), _ptr(T), _ptr(psi), _ptr(off)))
        return dict(mean=mean, transform=T, psi=psi, offset=off)

    def set_model(self, mean, transform, psi):
        self._dout = None            # the model dimension may change
        mean = np.ascontiguousarray(mean, np.float64)
        T = np.ascontiguousarray(transform, np.float64)
        psi = np.ascontiguousarray(psi, np.float64)
        dout, din = T.shape
        if mean.shape != (din,) or psi.shape != (dout,):
            raise ValueError("set_model: shapes disagree")
        self._ck(self._lib.plda_set_model(self._h, dout, din, _ptr(mean), _ptr(T), _ptr(psi)))

    def save(self, path):
        """Model + z-norm statistics to .npz (the reference has no persistence)."""
        m = self.get_model()
        ids = np.array(sorted(self._meanz), dtype=np.int64)
        extra = {}
        if self._calibration is not None:      # three more keys, only when a calibration is stored
            c = self._calibration
            extra = {"calib_a": np.float64(c.a), "calib_b": np.float64(c.b), "calib_prior": np.float64(c.prior)}
        if self._embedding is not None:        # five more keys, only when a chain is attached; absent arrays are saved empty
            e = self._embedding
            none = np.zeros(0)
            extra.update(embed_m_in=none if e.m_in is None else e.m_in, embed_len_in=np.float64(e.len_in),
                         embed_A=np.zeros((0, e.din)) if e.A is None else e.A, embed_m_out=none if e.m_out is None else e.m_out,
                         embed_len_out=np.float64(e.len_out))
        np.savez(_npz_path(path), mean=m["mean"], transform=m["transform"], psi=m["psi"], zn_ids=ids,
                 zn_mean=np.array([self._meanz[i] for i in ids], dtype=np.float64),
                 zn_std=np.array([self._stdvz[i] for i in ids], dtype=np.float64), **extra)

    def load(self, path):
        z = np.load(_npz_path(path, for_load=True))
        self.set_model(z["mean"], z["transform"], z["psi"])
        self._meanz = {int(i): float(v) for i, v in zip(z["zn_ids"], z["zn_mean"])}
        self._stdvz = {int(i): float(v) for i, v in zip(z["zn_ids"], z["zn_std"])}
        self._zn_tag = None         # the sorted copy of _zn_arrays belongs to the dicts just replaced (id() of a new dict may repeat)
        self._calibration = None    # replaced like the z-norm dictionaries: a file without the keys clears it
        if "calib_a" in z.files:
            from .calibration import Calibration
            self._calibration = Calibration(float(z["calib_a"]), float(z["calib_b"]), float(z["calib_prior"]))
        chain = None                # a file without the keys clears the chain, like the calibration
        if "embed_A" in z.files:
            from .embed import EmbeddingChain
            A, m_in, m_out = z["embed_A"], z["embed_m_in"], z["embed_m_out"]
            chain = EmbeddingChain(m_in if m_in.size else None, float(z["embed_len_in"]), A if A.size else None,
                                   m_out if m_out.size else None, float(z["embed_len_out"]), dim=A.shape[1])
        self.set_embedding(chain)

    def save_kaldi(self, path, binary=True):
        """Write the model as a Kaldi `Plda` file (plda_amd/kaldi_io.py: format restated, not pinned)."""
        from . import kaldi_io
        m = self.get_model()
        if m["transform"].shape[0] != m["transform"].shape[1]:
            # Kaldi's Plda::Read / TransformIvector assume a square transform (Dim() = mean.Dim() = psi.Dim())
            raise ValueError("save_kaldi: a model truncated with targetdim (transform %d x %d) has no Kaldi Plda "
                             "representation; use save()" % m["transform"].shape)
        kaldi_io.write_plda(path, m["mean"], m["transform"], m["psi"], binary)

    def load_kaldi(self, path):
        """Load a Kaldi `Plda` file (binary or text), e.g. one written by ivector-compute-plda."""
        from . import kaldi_io
        mean, transform, psi = kaldi_io.read_plda(path)
        self.set_model(mean, transform, psi)
        return self

    def truncate(self, targetdim):
        """Build extension 'targetdim' (SURVEY.md Appendix B Q3): keep the top-psi rows."""
        self._dout = None            # the model dimension may change
        self._ck(self._lib.plda_truncate(self._h, int(targetdim)))

    def smooth(self, factor):
        """Plda::SmoothWithinClassCovariance (reached at pldamodule.cpp:158-160)."""
        self._ck(self._lib.plda_smooth(self._h, float(factor)))

    # ------------------------------------------------- domain adaptation (csrc/adapt.hip)
    def _model_replaced(self):
        """The z-norm maps, their sorted copy and the stored calibration describe the scores of the model that was just
        replaced; the maps are insert-once, so a later norm() could not overwrite them: they are cleared."""
        self._meanz = {}
        self._stdvz = {}
        self._zn_tag = None
        self._calibration = None

    def adapt_reset(self):
        """Forget the adaptation statistics; the next accumulation takes the model mean as its pilot anew."""
        self._ck(self._lib.plda_adapt_reset(self._h))

    def adapt_accumulate(self, x, weights=None):
        """Add the rows x [N, D] (weights [N] >= 0, None: 1) to the adaptation statistics: total weight, sum and second
        moments about the pilot (the model mean at the first accumulation after a reset).  The rows are read once, slab by
        slab.  A non-finite row or a bad weight raises and leaves the statistics as they were."""
        X = self._rows(x)
        n, d = X.shape
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, np.float64).reshape(-1)
            if w.shape[0] != n:
                raise ValueError("adapt_accumulate: one weight per row")
        self._ck(self._lib.plda_adapt_accumulate(self._h, _ptr(X), n, d, _ptr(w)))

    def adapt_accumulate_dev(self, dX, n, d, dweights=None):
        """The same on rows already in this GPU's memory: dX / dweights are device addresses (ints) of fp64 [n, d] / [n]."""
        self._ck(self._lib.plda_adapt_accumulate_dev(self._h, C.c_void_p(int(dX)), int(n), int(d),
                                                     C.c_void_p(int(dweights)) if dweights else None))

    def adapt_stats(self):
        """dict(tot_weight, rows, pilot [D], s1 [D], s2 [D, D]): the record as it stands (sums about the pilot)."""
        _, d = self.dims()
        tw, rows = C.c_double(), C.c_int64()
        pilot, s1, s2 = np.zeros(d), np.zeros(d), np.zeros((d, d))
        self._ck(self._lib.plda_adapt_get_stats(self._h, C.byref(tw), C.byref(rows), _ptr(pilot), _ptr(s1), _ptr(s2)))
        return dict(tot_weight=tw.value, rows=rows.value, pilot=pilot, s1=s1, s2=s2)

    def adapt_add_stats(self, tot_weight, rows, pilot, s1, s2):
        """Add the record of another handle or rank (the fields of adapt_stats()).  Its pilot must equal this record's bit
        for bit; an empty record adopts it only if it equals the model mean."""
        _, d = self.dims()
        pilot = np.ascontiguousarray(pilot, np.float64)
        s1 = np.ascontiguousarray(s1, np.float64)
        s2 = np.ascontiguousarray(s2, np.float64)
        if pilot.shape != (d,) or s1.shape != (d,) or s2.shape != (d, d):
            raise ValueError("adapt_add_stats: pilot / s1 must be [%d], s2 [%d, %d]" % (d, d, d))
        self._ck(self._lib.plda_adapt_add_stats(self._h, float(tot_weight), int(rows), _ptr(pilot), _ptr(s1), _ptr(s2)))

    def adapt_update(self, within_scale=0.3, between_scale=0.7, mean_diff_scale=1.0):
        """Replace the model by its unsupervised adaptation to the accumulated statistics (Kaldi's PldaUnsupervisedAdaptor
        restated, defaults included; PARITY UNPINNED): the variance the data shows beyond the model's total covariance is
        added to the within- and between-class covariances in the given proportions and the mean moves to the data's.
        Returns a plda_amd.adaptation.Adaptation.  On failure the old model stays.  On success the z-norm statistics and
        the stored calibration are CLEARED: they describe the scores of the old model (and the z-norm maps are
        insert-once, so a later norm() could not overwrite them).  Vectors transformed before the update belong to the
        old model too."""
        from .adaptation import Adaptation
        _, d = self.dims()
        eig = np.zeros(d)
        info = N.AdaptInfo()
        self._ck(self._lib.plda_adapt_update(self._h, float(within_scale), float(between_scale), float(mean_diff_scale),
                                             _ptr(eig), C.byref(info)))
        self._model_replaced()
        return Adaptation(eig, info.n_excess, info.tot_weight, info.rows, info.mean_shift)

    def adapt(self, x, weights=None, within_scale=0.3, between_scale=0.7, mean_diff_scale=1.0):
        """Unsupervised domain adaptation in one call: adapt_reset, adapt_accumulate(x, weights), adapt_update(...).
        Clears the z-norm statistics and the stored calibration like adapt_update."""
        self.adapt_reset()
        self.adapt_accumulate(x, weights)
        return self.adapt_update(within_scale, between_scale, mean_diff_scale)

    def blend(self, other, alpha, alpha_mean=None):
        """Supervised adaptation by interpolation: within- and between-class covariances become (1 - alpha) this model's +
        alpha `other`'s, the mean (1 - alpha_mean) this + alpha_mean other's (alpha_mean=None: alpha).  `other` is an MPlda,
        a liblda.PLDA or a (mean, transform, psi) triple of the same dimension.  On success the z-norm statistics and the
        stored calibration are cleared, as by adapt_update."""
        inner = getattr(other, "_instance", other)
        if isinstance(inner, MPlda):
            m = inner.get_model()
            mean2, T2, psi2 = m["mean"], m["transform"], m["psi"]
        else:
            mean2, T2, psi2 = other
        mean2 = np.ascontiguousarray(mean2, np.float64)
        T2 = np.ascontiguousarray(T2, np.float64)
        psi2 = np.ascontiguousarray(psi2, np.float64)
        if T2.ndim != 2 or T2.shape[0] != T2.shape[1] or mean2.shape != (T2.shape[0],) or psi2.shape != (T2.shape[0],):
            raise ValueError("blend: the other model must be square: mean [D], transform [D, D], psi [D]")
        am = float(alpha) if alpha_mean is None else float(alpha_mean)
        self._ck(self._lib.plda_blend_model(self._h, T2.shape[0], _ptr(mean2), _ptr(T2), _ptr(psi2), float(alpha), am))
        self._model_replaced()

    # ------------------------------------------------------------ transform
    def transform(self, x, y, targetdim=0, smoothfactor=1.0):
        """Mplda_transform (pldamodule.cpp:111-194): {label: (n, ndarray f64[D])},
        ascending label order (:164).  `targetdim`/`smoothfactor` are the C layer's
        optional "|kf" arguments (:117): smoothing is applied on every call where it is
        != 1.0, cumulatively (:158-160, quirk Q5); targetdim is the build's working
        replacement for the reference's broken one (quirk Q3)."""
        if not isinstance(x, np.ndarray):
            raise TypeError("argument 1 must be numpy.ndarray, not %s" % type(x).__name__)
        X = np.ascontiguousarray(x, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("Input features must be 2-dimensional (nsamples, featdim)")
        X = self._embedded(x, X)
        n, d = X.shape
        Y = _labels(y, n, allow_strings_msg=True)
        if targetdim and int(targetdim) != self.dims()[0]:
            self.truncate(int(targetdim))
        if float(smoothfactor) != 1.0:
            self.smooth(float(smoothfactor))
        dout, _ = self.dims()
        cap = C.c_int64(n)
        out_labels = np.empty(n, np.uint64)
        out_counts = np.empty(n, np.int64)
        out_vecs = np.empty((n, dout), np.float64)
        self._ck(self._lib.plda_transform_groups(self._h, _ptr(X), n, d, _ptr(Y), _ptr(out_labels),
                                                 _ptr(out_counts), _ptr(out_vecs), C.byref(cap)))
        g = cap.value
        vecs = out_vecs[:g].copy()
        # keys / counts as Python ints and one row view per label, all built by C-level iteration
        res = Transformed(zip(out_labels[:g].tolist(), zip(out_counts[:g].tolist(), vecs)))
        res._packed = (out_labels[:g].astype(np.int64), out_counts[:g].astype(np.int32), vecs)
        return res

    def transform_plan(self, r):
        """What K4 runs for r rows on the installed model (plda_transform_plan): {"arm": "fused" (the one-pass kernel) or "pair"
        (GEMM + length-norm pass), "cls": the dimension class 0 .. 4 (Dout <= 128 / 208 / 256 / 384 / 512; -1 on the pair arm),
        "main_rows", "main_block": the rows of the main launch and the rows of one of its blocks, "tail_rows", "tail_block": the
        same of the tail launch (0, 0 without one), "cus": the compute units the split was made for}."""
        out = (C.c_int64 * 8)()
        self._ck(self._lib.plda_transform_plan(self._h, int(r), out))
        return {"arm": "pair" if out[0] else "fused", "cls": int(out[1]), "main_rows": int(out[2]), "main_block": int(out[3]),
                "tail_rows": int(out[4]), "tail_block": int(out[5]), "cus": int(out[6])}

    def transform_array(self, xbar, num_examples=1):
        """Batched Plda::TransformIvector on already-averaged rows -> ndarray [R, D].  ValueError when a count is <= 0."""
        X = np.ascontiguousarray(xbar, np.float64)
        r, d = X.shape
        dout, _ = self.dims()
        out = np.zeros((r, dout), np.float64)
        if np.ndim(num_examples) == 0:
            self._ck(self._lib.plda_transform_rows(self._h, _ptr(X), r, d, None, int(num_examples), _ptr(out)))
        else:
            ne = np.ascontiguousarray(num_examples, np.int32)
            if ne.shape != (r,):
                raise ValueError("num_examples must have one entry per row")
            if (ne <= 0).any():
                raise ValueError("num_examples must be > 0: %d of %d rows are not" % (int((ne <= 0).sum()), r))
            self._ck(self._lib.plda_transform_rows(self._h, _ptr(X), r, d, _ptr(ne), 0, _ptr(out)))
        return out

    # ----------------------------------------------------------------- speaker clustering (csrc/ahc.hip)
    def cluster(self, x, offsets, threshold=0.0, num_speakers=None, return_merges=False, target_energy=None, method="ahc", p=None,
                p_fractions=None, max_speakers=16, max_iters=20, return_info=False):
        """Cluster the segments of R recordings (diarisation; plda_amd/diarize.py): x [T, Din] raw segment vectors, recording
        r owning rows offsets[r] .. offsets[r+1].  Every row is transformed with num_examples = 1, every recording's segments
        are scored against each other on the device and merged bottom-up (average linkage) while the best pair's average
        score is at least `threshold` (None: no threshold) and more than `num_speakers` (an int or one per recording; None: 1)
        clusters are left.  target_energy=t (0 < t < 1; Kaldi's --target-energy): every recording is scored in the PCA subspace
        of its own segment vectors instead (score_dense).  Returns (labels int32 [T], n_clusters int32 [R][, (merge_a, merge_b,
        merge_cost)]).
        method="spectral": spectral clustering with auto-tuned pruning instead (diarize.spectral: no threshold; p, p_fractions,
        max_speakers, max_iters and return_info as there; num_speakers None: the eigengap's count).  A non-default threshold or
        return_merges=True is a ValueError; with target_energy the blocks of score_dense are clustered.  Returns (labels,
        n_clusters[, info])."""
        from . import diarize
        offsets = np.ascontiguousarray(offsets, np.int64)
        if method == "spectral":
            if return_merges or not (isinstance(threshold, (int, float)) and not isinstance(threshold, bool) and threshold == 0.0):
                raise ValueError('method="spectral" has no threshold and no merge record')
            fr = diarize.P_FRACTIONS if p_fractions is None else p_fractions
            diarize.spectral_args(offsets, p, fr, max_speakers, num_speakers, max_iters)       # (before any device work)
            X = self._rows(x, "Segment vectors")
            if X.shape[0] != int(offsets[-1]):
                raise ValueError("offsets must hold R + 1 >= 2 entries ending at the number of rows of x")
            if target_energy is not None:
                return diarize.spectral(self, diarize.score_dense_pca(self, X, offsets, target_energy), p, fr, max_speakers, num_speakers,
                                        max_iters, return_info)
            return diarize.spectral_vectors(self, self.transform_array(X, 1), offsets, p, fr, max_speakers, num_speakers, max_iters,
                                            return_info)
        if method != "ahc":
            raise ValueError('method must be "ahc" or "spectral", got %r' % (method,))
        if p is not None or p_fractions is not None or max_speakers != 16 or max_iters != 20 or return_info:
            raise ValueError('p, p_fractions, max_speakers, max_iters and return_info belong to method="spectral"')
        diarize.stop_args(offsets, threshold, num_speakers)     # (threshold=None without num_speakers: ValueError, before any work)
        X = self._rows(x, "Segment vectors")
        if offsets.ndim != 1 or len(offsets) < 2 or X.shape[0] != int(offsets[-1]):
            raise ValueError("offsets must hold R + 1 >= 2 entries ending at the number of rows of x")
        if target_energy is not None:
            return diarize.ahc_dense_pca(self, X, offsets, target_energy, threshold, num_speakers, return_merges)
        return diarize.ahc_vectors(self, self.transform_array(X, 1), offsets, threshold, num_speakers, return_merges)

    # ----------------------------------------------------------------- corpus-scale clustering (csrc/ahc.hip, the wide class)
    def cluster_corpus(self, x, threshold=0.0, num_speakers=None, return_merges=False):
        """Cluster a whole unlabelled corpus into pseudo-speakers: x [N, Din] raw vectors, ONE problem of up to
        diarize.AHC_WIDE_MAX = 32768 rows on the whole device (include/plda_hip.h, "corpus-scale clustering").  Every row is
        transformed with num_examples = 1, all rows are scored against each other on the device and merged bottom-up (average
        linkage, the contract of cluster() with one recording) while the best pair's average score is at least `threshold`
        (None: no threshold) and more than `num_speakers` (None: 1) clusters are left.  Returns (labels int32 [N],
        n_clusters[, (merge_a, merge_b, merge_cost)])."""
        from . import diarize
        if not isinstance(x, np.ndarray) or x.ndim != 2:
            raise ValueError("Corpus vectors must be a 2-dimensional ndarray (nsamples, featdim)")
        diarize.wide_args(x.shape[0], threshold, num_speakers)       # (before any device work)
        X = self._rows(x, "Corpus vectors")
        return diarize.ahc_wide_vectors(self, self.transform_array(X, 1), threshold, num_speakers, return_merges)

    def adapt_clustered(self, x, threshold=0.0, num_speakers=None, alpha=0.5, alpha_mean=None, min_cluster_size=2, iters=10):
        """Clustering-based domain adaptation (Garcia-Romero et al. 2014) in one call: cluster_corpus(x, threshold,
        num_speakers) with this (out-of-domain) model; the rows of clusters smaller than `min_cluster_size` are dropped and the
        rest renumbered (diarize.keep_clusters); an in-domain model is fitted on those pseudo-labels on a second handle of the
        same device (`iters` EM iterations); blend(that model, alpha, alpha_mean).  Returns a
        plda_amd.adaptation.ClusteredAdaptation(labels, n_clusters, rows_kept, clusters_kept).  ValueError, before the fit and
        with the model untouched, if fewer than two clusters survive.  Clears the z-norm statistics and the stored calibration,
        as blend does."""
        from . import diarize
        from .adaptation import ClusteredAdaptation
        if isinstance(min_cluster_size, bool) or not isinstance(min_cluster_size, (int, np.integer)) or min_cluster_size < 1:
            raise ValueError("min_cluster_size must be an integer >= 1, got %r" % (min_cluster_size,))
        if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 1:
            raise ValueError("iters must be an integer >= 1, got %r" % (iters,))
        for name, v in (("alpha", alpha), ("alpha_mean", alpha if alpha_mean is None else alpha_mean)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) <= 1.0:
                raise ValueError("%s must lie in [0, 1], got %r" % (name, v))
        labels, ncl = self.cluster_corpus(x, threshold, num_speakers)
        rows, new_labels, kept = diarize.keep_clusters(labels, min_cluster_size)
        if kept < 2:
            raise ValueError("adapt_clustered: %d of %d clusters have at least %d members; an in-domain model needs two"
                             % (kept, ncl, int(min_cluster_size)))
        X = self._rows(x, "Corpus vectors")
        other = MPlda(self.device)
        other.fit(np.ascontiguousarray(X[rows]), new_labels.astype(np.uint64), int(iters))
        self.blend(other, alpha, alpha_mean)
        return ClusteredAdaptation(labels, ncl, int(rows.shape[0]), kept)

    def score_dense(self, x, offsets, target_energy, return_info=False):
        """Every recording's segment pairs scored in the PCA subspace of its own segment vectors (Kaldi's
        ivector-plda-scoring-dense --target-energy; plda_amd/diarize.py: score_dense_pca): x [T, Din] raw segment vectors.
        Returns a list of [N_r, N_r] float32 blocks[, {"dims", "eigenvalues"}]."""
        from . import diarize
        return diarize.score_dense_pca(self, self._rows(x, "Segment vectors"), offsets, target_energy, return_info)

    # ----------------------------------------------------------------- VBx resegmentation (csrc/vbx.hip)
    def project_rows(self, x):
        """transform . x + offset of every row of x [R, Din] -> [R, Dout]: TransformIvector without its normalisation factor,
        the space VBx works in."""
        return self._project(self._rows(x, "Segment vectors"))

    def _project(self, X):
        dout, _ = self.dims()
        out = np.zeros((X.shape[0], dout), np.float64)
        self._ck(self._lib.plda_project_rows(self._h, _ptr(X), X.shape[0], X.shape[1], _ptr(out)))
        return out

    def project_rows_dev(self, dX, R, Din, dout):
        """The same on HBM-resident rows (raw device addresses)."""
        self._ck(self._lib.plda_project_rows_dev(self._h, C.c_void_p(int(dX)), int(R), int(Din), C.c_void_p(int(dout))))

    def resegment(self, x, offsets, labels, Fa=0.3, Fb=17.0, loop_prob=0.99, init_smoothing=5.0, max_iters=40, epsilon=1e-4,
                  return_posteriors=False, return_second=False):
        """VBx resegmentation (plda_amd/diarize.py: vbx): x [T, Din] raw segment vectors, recording r owning rows offsets[r] ..
        offsets[r+1], `labels` the initial labels (cluster()'s).  The rows are projected into the model's diagonalised space
        (project_rows), the between-class variance is the model's psi.  Returns (labels, n_clusters[, info]);
        return_second=True: (labels, n_clusters, labels2, post2[, info]), every segment's second speaker and its posterior."""
        from . import diarize
        X = self._rows(x, "Segment vectors")
        offsets = np.ascontiguousarray(offsets, np.int64)
        if offsets.ndim != 1 or len(offsets) < 2 or X.shape[0] != int(offsets[-1]):
            raise ValueError("offsets must hold R + 1 >= 2 entries ending at the number of rows of x")
        diarize.vbx_args(np.zeros((X.shape[0], 1)), offsets, labels, None, Fa, Fb, loop_prob, max_iters)   # (before any device work)
        return diarize.vbx(self, self._project(X), offsets, labels, None, Fa, Fb, loop_prob, init_smoothing, max_iters, epsilon,
                           return_posteriors, return_second)

    def diarize(self, x, offsets, threshold=0.0, num_speakers=None, target_energy=None, overlap=None, min_posterior=None, method="ahc",
                p=None, p_fractions=None, max_speakers=16, **vbx):
        """cluster(x, offsets, threshold, num_speakers), then resegment(x, offsets, its labels, **vbx).  target_energy goes to
        the clustering only: VBx keeps working on the full model.  With overlap (a per-segment bool mask) or min_posterior the
        return is (labels, n_clusters, labels2): the second speaker where diarize.apply_overlap keeps it, -1 elsewhere.
        method="spectral" (with p, p_fractions, max_speakers as cluster takes them): the spectral clustering's labels start VBx."""
        if (overlap is not None or min_posterior is not None) and (vbx.get("return_second") or vbx.get("return_posteriors")):
            raise ValueError("overlap / min_posterior return (labels, n_clusters, labels2): call resegment for the posteriors")
        if method != "ahc" or p is not None or p_fractions is not None or max_speakers != 16:
            labels, _ = self.cluster(x, offsets, threshold, num_speakers, target_energy=target_energy, method=method, p=p,
                                     p_fractions=p_fractions, max_speakers=max_speakers)
        elif target_energy is None:
            labels, _ = self.cluster(x, offsets, threshold, num_speakers)
        else:
            labels, _ = self.cluster(x, offsets, threshold, num_speakers, target_energy=target_energy)
        if overlap is None and min_posterior is None:
            return self.resegment(x, offsets, labels, **vbx)
        from . import diarize
        labels, ncl, labels2, post2 = self.resegment(x, offsets, labels, return_second=True, **vbx)
        return labels, ncl, diarize.apply_overlap(labels2, post2, overlap, min_posterior)

    def vbx_dev(self, dY, D, dPhi, dlabels_in, offsets, dlabels, dn_clusters, Fa=0.3, Fb=17.0, loop_prob=0.99, init_smoothing=5.0,
                max_iters=40, epsilon=1e-4, dgamma=None, gamma_off=None, dpi=None, pi_off=None, delbo=None, diters=None):
        """VBx on HBM-resident projected rows and labels (raw device addresses); offsets, gamma_off and pi_off (int64) are HOST
        arrays."""
        self._ck(self._lib.plda_vbx_dev(
            self._h, _vp(dY), int(D), _vp(dPhi), _vp(dlabels_in), _ptr(offsets), len(offsets) - 1, float(Fa), float(Fb), float(loop_prob),
            float(init_smoothing), int(max_iters), float(epsilon), _vp(dlabels), _vp(dn_clusters), _vp(dgamma),
            _ptr(gamma_off) if gamma_off is not None else None, _vp(dpi), _ptr(pi_off) if pi_off is not None else None, _vp(delbo),
            _vp(diters)))

    def vbx_top2_dev(self, dY, D, dPhi, dlabels_in, offsets, dlabels, dn_clusters, dlabels2=None, dpost2=None, Fa=0.3, Fb=17.0,
                     loop_prob=0.99, init_smoothing=5.0, max_iters=40, epsilon=1e-4, dgamma=None, gamma_off=None, dpi=None, pi_off=None,
                     delbo=None, diters=None):
        """vbx_dev with the second speaker: dlabels2 int32 [T] and dpost2 float64 [T] (raw device addresses, each may be None)."""
        self._ck(self._lib.plda_vbx_top2_dev(
            self._h, _vp(dY), int(D), _vp(dPhi), _vp(dlabels_in), _ptr(offsets), len(offsets) - 1, float(Fa), float(Fb), float(loop_prob),
            float(init_smoothing), int(max_iters), float(epsilon), _vp(dlabels), _vp(dn_clusters), _vp(dgamma),
            _ptr(gamma_off) if gamma_off is not None else None, _vp(dpi), _ptr(pi_off) if pi_off is not None else None, _vp(delbo),
            _vp(diters), _vp(dlabels2), _vp(dpost2)))

    def ahc_matrix_dev(self, dscores, block_off, offsets, has_threshold, threshold, min_clusters, dlabels, dn_clusters,
                       dmerge_a=None, dmerge_b=None, dmerge_cost=None):
        """Cluster packed HBM-resident fp32 score blocks (raw device addresses); block_off, offsets (int64) and min_clusters
        (int32 or None) are HOST arrays."""
        self._ck(self._lib.plda_ahc_matrix_dev(
            self._h, _vp(dscores), _ptr(block_off), _ptr(offsets), len(offsets) - 1, int(has_threshold), float(threshold),
            _ptr(min_clusters) if min_clusters is not None else None, _vp(dlabels), _vp(dn_clusters), _vp(dmerge_a), _vp(dmerge_b),
            _vp(dmerge_cost)))

    def score_ahc_dev(self, dX, offsets, has_threshold, threshold, min_clusters, dlabels, dn_clusters, dmerge_a=None,
                      dmerge_b=None, dmerge_cost=None):
        """The same on HBM-resident transformed segment vectors dX [T, Dout]: the blocks are scored and dropped."""
        self._ck(self._lib.plda_score_ahc_dev(
            self._h, _vp(dX), _ptr(offsets), len(offsets) - 1, int(has_threshold), float(threshold),
            _ptr(min_clusters) if min_clusters is not None else None, _vp(dlabels), _vp(dn_clusters), _vp(dmerge_a), _vp(dmerge_b),
            _vp(dmerge_cost)))

    def ahc_wide_matrix_dev(self, dscores, n, ld, has_threshold, threshold, min_clusters, dlabels, dn_clusters, dmerge_a=None,
                            dmerge_b=None, dmerge_cost=None):
        """Cluster ONE HBM-resident fp32 score block [n, n] at row stride ld on the whole device (raw device addresses;
        plda_ahc_wide_matrix_dev); min_clusters is one int >= 1."""
        self._ck(self._lib.plda_ahc_wide_matrix_dev(
            self._h, _vp(dscores), int(n), int(ld), int(has_threshold), float(threshold), int(min_clusters), _vp(dlabels),
            _vp(dn_clusters), _vp(dmerge_a), _vp(dmerge_b), _vp(dmerge_cost)))

    def score_ahc_wide_dev(self, dX, n, has_threshold, threshold, min_clusters, dlabels, dn_clusters, dmerge_a=None, dmerge_b=None,
                           dmerge_cost=None):
        """The same on HBM-resident transformed vectors dX [n, Dout]: the block is scored and dropped."""
        self._ck(self._lib.plda_score_ahc_wide_dev(
            self._h, _vp(dX), int(n), int(has_threshold), float(threshold), int(min_clusters), _vp(dlabels), _vp(dn_clusters),
            _vp(dmerge_a), _vp(dmerge_b), _vp(dmerge_cost)))

    def spectral_matrix_dev(self, dscores, block_off, offsets, p_table, max_speakers, num_speakers, max_iters, dlabels, dn_clusters,
                            dp_used=None, dk_gap=None, deig=None, dembed=None, ddeg2=None):
        """Spectral clustering of packed HBM-resident fp32 score blocks (raw device addresses; plda_spectral_matrix_dev);
        block_off, offsets (int64), p_table (int32 [R, P]) and num_speakers (int32 [R] or None) are HOST arrays."""
        self._ck(self._lib.plda_spectral_matrix_dev(
            self._h, _vp(dscores), _ptr(block_off), _ptr(offsets), len(offsets) - 1, _ptr(p_table), p_table.shape[1], int(max_speakers),
            _ptr(num_speakers) if num_speakers is not None else None, int(max_iters), _vp(dlabels), _vp(dn_clusters), _vp(dp_used),
            _vp(dk_gap), _vp(deig), _vp(dembed), _vp(ddeg2)))

    def score_spectral_dev(self, dX, offsets, p_table, max_speakers, num_speakers, max_iters, dlabels, dn_clusters, dp_used=None,
                           dk_gap=None, deig=None, dembed=None, ddeg2=None):
        """The same on HBM-resident transformed segment vectors dX [T, Dout]: the blocks are scored and dropped."""
        self._ck(self._lib.plda_score_spectral_dev(
            self._h, _vp(dX), _ptr(offsets), len(offsets) - 1, _ptr(p_table), p_table.shape[1], int(max_speakers),
            _ptr(num_speakers) if num_speakers is not None else None, int(max_iters), _vp(dlabels), _vp(dn_clusters), _vp(dp_used),
            _vp(dk_gap), _vp(deig), _vp(dembed), _vp(ddeg2)))

    def score_dense_pca_dev(self, dX, offsets, target_energy, dscores, block_off, ddims=None, deig=None):
        """plda_score_dense_pca_dev on HBM-resident rows dX [T, Din] (raw device addresses): block r row-major at dscores +
        block_off[r] floats; offsets and block_off (int64) are HOST arrays; ddims int32 [R] and deig float64 [T] may be None."""
        self._ck(self._lib.plda_score_dense_pca_dev(self._h, _vp(dX), _ptr(offsets), len(offsets) - 1, float(target_energy),
                                                    _vp(dscores), _ptr(block_off), _vp(ddims), _vp(deig)))

    def score_dense_pca_ahc_dev(self, dX, offsets, target_energy, has_threshold, threshold, min_clusters, dlabels, dn_clusters,
                                dmerge_a=None, dmerge_b=None, dmerge_cost=None):
        """The same blocks clustered and dropped (plda_score_dense_pca_ahc_dev); the outputs as score_ahc_dev's."""
        self._ck(self._lib.plda_score_dense_pca_ahc_dev(
            self._h, _vp(dX), _ptr(offsets), len(offsets) - 1, float(target_energy), int(has_threshold), float(threshold),
            _ptr(min_clusters) if min_clusters is not None else None, _vp(dlabels), _vp(dn_clusters), _vp(dmerge_a), _vp(dmerge_b),
            _vp(dmerge_cost)))

    # ----------------------------------------------------------------- diarisation error rate (csrc/der.hip)
    def der(self,ref, hyp, offsets, dur=None, return_map=False, jer=False):
        """Diarisation error rate of R recordings (plda_amd/der.py): ref, hyp int [T] per-segment speaker labels (-1 =
        non-speech), recording r owning segments offsets[r] .. offsets[r+1], dur int [T] ticks (None: 1 everywhere).  Miss,
        false alarm and confusion under the optimal one-to-one speaker mapping, exact integers from the device.  Returns a
        plda_amd.der.DerResult (counts [R, 4], der [R], total[, map [R, 64]]); jer=True: also the Jaccard error rate and the
        per-speaker figures (jer, jer_counts, jer_map, speakers)."""
        from . import der
        return der.der(self, ref, hyp, offsets, dur, return_map, jer)

    def tune_threshold(self, x, offsets, ref, thresholds, dur=None, target_energy=None, turns=None, seg_start=None, seg_dur=None,
                       collar=0, uem=None, skip_overlap=False, metric="der"):
        """The clustering threshold with the lowest pooled DER (metric="jer": the lowest pooled JER) on a development set: ONE cluster(x, offsets, threshold=None,
        num_speakers=1, return_merges=True[, target_energy=target_energy]), then one der.sweep of its full merge record over
        `thresholds`.  With `turns` (and seg_start, seg_dur; collar, uem, skip_overlap as in der_timed) the sweep is the
        time-based one, der.sweep_timed, and ref and dur must be None.  Returns (the best threshold -- the first of equal
        ones --, the plda_amd.der.SweepResult; under metric="jer" it carries jer_counts, jer and best_jer)."""
        from . import der
        if metric not in ("der", "jer"):
            raise ValueError("metric must be 'der' or 'jer'")
        jer = metric == "jer"
        offsets = np.ascontiguousarray(offsets, np.int64)
        X = self._rows(x, "Segment vectors")
        if offsets.ndim != 1 or len(offsets) < 2 or X.shape[0] != int(offsets[-1]):
            raise ValueError("offsets must hold R + 1 >= 2 entries ending at the number of rows of x")
        t, r = int(offsets[-1]), len(offsets) - 1
        empty = (np.zeros(t - r, np.int32), np.zeros(t - r, np.int32), np.zeros(t - r))
        if turns is not None:
            if ref is not None or dur is not None:
                raise ValueError("with turns, ref and dur must be None (the reference is the turns)")
            der.sweep_timed_args(empty, turns, seg_start, seg_dur, offsets, thresholds, None, collar, uem, skip_overlap)
        else:
            sargs = der.sweep_args(empty, offsets, ref, thresholds, dur, None)        # (before any device work)
            if jer:
                der._jer_ticks(sargs[6], sargs[3])
        from . import diarize
        diarize.stop_args(offsets, None, 1)
        if target_energy is not None:
            _, _, merges = diarize.ahc_dense_pca(self, X, offsets, target_energy, None, 1, True)
        else:
            _, _, merges = diarize.ahc_vectors(self, self.transform_array(X, 1), offsets, None, 1, True)   # cluster() on embedded rows
        if turns is not None:
            res = der.sweep_timed(self, merges, turns, seg_start, seg_dur, offsets, thresholds, None, collar, uem, skip_overlap, jer)
        else:
            res = der.sweep(self, merges, offsets, ref, thresholds, dur, None, jer)
        return float(res.thresholds[res.best_jer if jer else res.best]), res

    def der_timed(self, turns, seg_start, seg_dur, hyp, offsets, collar=0, uem=None, skip_overlap=False, return_map=False, hyp2=None,
                  jer=False):
        """Time-based DER of R recordings (plda_amd/der.py: der_timed): reference turns (turn_start, turn_dur, turn_spk,
        turn_off) that may overlap across speakers, disjoint hypothesis segments, a collar in ticks, UEM regions, md-eval's
        skip-overlap switch; hyp2: the second speaker of every segment, -1 = none; jer=True: also the Jaccard error rate and
        the per-speaker figures.  Returns a plda_amd.der.DerResult."""
        from . import der
        return der.der_timed(self, turns, seg_start, seg_dur, hyp, offsets, collar, uem, skip_overlap, return_map, hyp2, jer)

    # the four call shapes of the DER *_dev methods; jer: the outputs the JER entry point of that shape takes behind the rest
    def _der_seg_dev(self, name, dref, dhyp, ddur, offsets, dcounts, dmap, *jer):
        self._ck(getattr(self._lib, name)(self._h, _vp(dref), _vp(dhyp), _vp(ddur), _ptr(offsets), len(offsets) - 1, _vp(dcounts), _vp(dmap),
                                          *map(_vp, jer)))

    def _der_seg_sweep_dev(self, name, dmerges, offsets, dref, ddur, thresholds, min_clusters, dcounts, dn_clusters, *jer):
        self._ck(getattr(self._lib, name)(
            self._h, _vp(dmerges[0]), _vp(dmerges[1]), _vp(dmerges[2]), _ptr(offsets), len(offsets) - 1, _vp(dref), _vp(ddur),
            _ptr(thresholds), len(thresholds), _ptr(min_clusters), _vp(dcounts), _vp(dn_clusters), *map(_vp, jer)))

    def _der_timed_dev(self, name, dturns, turn_off, dseg_start, dseg_dur, dhyps, offsets, duem, uem_off, collar, flags, dcounts, dmap, *jer):
        du = duem if duem is not None else (None, None)      # dhyps: (dhyp,), or (dhyp, dhyp2) where the entry point takes two labels
        self._ck(getattr(self._lib, name)(
            self._h, _vp(dturns[0]), _vp(dturns[1]), _vp(dturns[2]), _ptr(turn_off), _vp(dseg_start), _vp(dseg_dur), *map(_vp, dhyps),
            _ptr(offsets), len(offsets) - 1, _vp(du[0]), _vp(du[1]), _ptr(uem_off), int(collar), int(flags), _vp(dcounts), _vp(dmap),
            *map(_vp, jer)))

    def _der_timed_sweep_dev(self, name, dmerges, dturns, turn_off, dseg_start, dseg_dur, offsets, duem, uem_off, collar, flags, thresholds,
                             min_clusters, dcounts, dn_clusters, *jer):
        du = duem if duem is not None else (None, None)
        self._ck(getattr(self._lib, name)(
            self._h, _vp(dmerges[0]), _vp(dmerges[1]), _vp(dmerges[2]), _vp(dturns[0]), _vp(dturns[1]), _vp(dturns[2]), _ptr(turn_off),
            _vp(dseg_start), _vp(dseg_dur), _ptr(offsets), len(offsets) - 1, _vp(du[0]), _vp(du[1]), _ptr(uem_off), int(collar), int(flags),
            _ptr(thresholds), len(thresholds), _ptr(min_clusters), _vp(dcounts), _vp(dn_clusters), *map(_vp, jer)))

    def der_timed_jer_dev(self, dturns, turn_off, dseg_start, dseg_dur, dhyp, dhyp2, offsets, dcounts, djer, dmap=None, djmap=None,
                          dspk=None, duem=None, uem_off=None, collar=0, flags=0):
        """plda_der_timed_jer_dev: der_timed_ovl_dev (dhyp2 may be None), then djer int64 [R, 2], djmap int32 [R, 64] or None,
        dspk int64 [R, 64, 3] or None."""
        self._der_timed_dev("plda_der_timed_jer_dev", dturns, turn_off, dseg_start, dseg_dur, (dhyp, dhyp2), offsets, duem, uem_off, collar,
                            flags, dcounts, dmap, djer, djmap, dspk)

    def der_timed_jer_sweep_dev(self, dmerges, dturns, turn_off, dseg_start, dseg_dur, offsets, thresholds, min_clusters, dcounts,
                                dn_clusters, djer, duem=None, uem_off=None, collar=0, flags=0):
        """plda_der_timed_jer_sweep_dev: der_timed_sweep_dev, then djer int64 [Q, R, 2]."""
        self._der_timed_sweep_dev("plda_der_timed_jer_sweep_dev", dmerges, dturns, turn_off, dseg_start, dseg_dur, offsets, duem, uem_off,
                                  collar, flags, thresholds, min_clusters, dcounts, dn_clusters, djer)

    def der_jer_dev(self, dref, dhyp, ddur, offsets, dcounts, djer, dmap=None, djmap=None, dspk=None):
        """plda_der_jer_dev: der_dev, then djer int64 [R, 2], djmap int32 [R, 64] or None, dspk int64 [R, 64, 3] or None."""
        self._der_seg_dev("plda_der_jer_dev", dref, dhyp, ddur, offsets, dcounts, dmap, djer, djmap, dspk)

    def der_jer_sweep_dev(self, dmerge_a, dmerge_b, dmerge_cost, offsets, dref, ddur, thresholds, min_clusters, dcounts, dn_clusters,
                          djer):
        """plda_der_jer_sweep_dev: der_sweep_dev, then djer int64 [Q, R, 2]."""
        self._der_seg_sweep_dev("plda_der_jer_sweep_dev", (dmerge_a, dmerge_b, dmerge_cost), offsets, dref, ddur, thresholds, min_clusters,
                                dcounts, dn_clusters, djer)

    def der_timed_ovl_dev(self, dturns, turn_off, dseg_start, dseg_dur, dhyp, dhyp2, offsets, dcounts, dmap=None, duem=None,
                          uem_off=None, collar=0, flags=0):
        """plda_der_timed_ovl_dev: der_timed_dev with dhyp2 int32 [T], the second label of every segment (None: der_timed_dev)."""
        self._der_timed_dev("plda_der_timed_ovl_dev", dturns, turn_off, dseg_start, dseg_dur, (dhyp, dhyp2), offsets, duem, uem_off, collar,
                            flags, dcounts, dmap)

    def der_timed_dev(self, dturns, turn_off, dseg_start, dseg_dur, dhyp, offsets, dcounts, dmap=None, duem=None, uem_off=None,
                      collar=0, flags=0):
        """plda_der_timed_dev on HBM-resident int32 arrays (raw device addresses): dturns = (turn_start, turn_dur, turn_spk),
        duem = (uem_start, uem_dur) or None; turn_off, offsets, uem_off (int64) are HOST arrays; dcounts int64 [R, 4], dmap
        int32 [R, 64] or None."""
        self._der_timed_dev("plda_der_timed_dev", dturns, turn_off, dseg_start, dseg_dur, (dhyp,), offsets, duem, uem_off, collar, flags,
                            dcounts, dmap)

    def der_timed_sweep_dev(self, dmerges, dturns, turn_off, dseg_start, dseg_dur, offsets, thresholds, min_clusters, dcounts,
                            dn_clusters, duem=None, uem_off=None, collar=0, flags=0):
        """plda_der_timed_sweep_dev on an HBM-resident full merge record dmerges = (merge_a, merge_b, merge_cost) and the
        arrays of der_timed_dev; thresholds (float64) and min_clusters (int32 or None) are HOST arrays; dcounts int64
        [Q, R, 4], dn_clusters int32 [Q, R]."""
        self._der_timed_sweep_dev("plda_der_timed_sweep_dev", dmerges, dturns, turn_off, dseg_start, dseg_dur, offsets, duem, uem_off, collar,
                                  flags, thresholds, min_clusters, dcounts, dn_clusters)

    def der_dev(self, dref, dhyp, ddur, offsets, dcounts, dmap=None):
        """plda_der_dev on HBM-resident int32 labels and durations (raw device addresses; ddur and dmap may be None);
        offsets (int64) is a HOST array; dcounts int64 [R, 4], dmap int32 [R, 64]."""
        self._der_seg_dev("plda_der_dev", dref, dhyp, ddur, offsets, dcounts, dmap)

    def der_sweep_dev(self, dmerge_a, dmerge_b, dmerge_cost, offsets, dref, ddur, thresholds, min_clusters, dcounts, dn_clusters):
        """plda_der_sweep_dev on an HBM-resident full merge record, labels and durations (raw device addresses); offsets
        (int64), thresholds (float64) and min_clusters (int32 or None) are HOST arrays; dcounts int64 [Q, R, 4], dn_clusters
        int32 [Q, R]."""
        self._der_seg_sweep_dev("plda_der_sweep_dev", (dmerge_a, dmerge_b, dmerge_cost), offsets, dref, ddur, thresholds, min_clusters,
                                dcounts, dn_clusters)

    # ----------------------------------------------------------------- norm
    def norm(self, vectors, transformedvecs, numutts=0):
        """MPlda_norm (pldamodule.cpp:196-256): z-norm statistics of every enrol model
        against the cohort `vectors`; stored insert-once like unordered_map::insert
        (:245,250, quirk Q8).  Returns None (quirk Q9)."""
        if not isinstance(vectors, np.ndarray):
            raise TypeError("argument 1 must be numpy.ndarray, not %s" % type(vectors).__name__)
        if not isinstance(transformedvecs, dict):
            raise TypeError("argument 2 must be dict, not %s" % type(transformedvecs).__name__)
        bkg = self._embedded(vectors, np.ascontiguousarray(vectors, np.float64))
        nb, d = bkg.shape
        rows = bkg
        if numutts and int(numutts) < nb:
            # the reference takes the first `numutts` rows of an unseeded shuffle (:204-216);
            # here: a fixed-seed permutation (quirk Q10)
            sel = np.sort(np.random.default_rng(0).permutation(nb)[: int(numutts)])
            rows = np.ascontiguousarray(bkg[sel])
        ids = list(transformedvecs.keys())
        if not ids:
            return None
        packed = getattr(transformedvecs, "_packed", None) if isinstance(transformedvecs, Transformed) else None
        if packed is not None and packed[0].shape[0] == len(ids):
            models = self._check_dim(packed[2], "norm: model vectors")       # transform()'s own block, as it is
        else:
            for k in ids:
                if not isinstance(k, (int, np.integer)) or not isinstance(transformedvecs[k], tuple):
                    return None  # the reference bails out with NULL (:229-230)
            models = self._check_dim(np.ascontiguousarray(np.stack([np.asarray(transformedvecs[k][1], np.float64) for k in ids])),
                                     "norm: model vectors")
        if d != self.dims()[1]:
            raise ValueError("norm: cohort vectors have %d features, the model expects %d" % (d, self.dims()[1]))
        mean, std = np.zeros(len(ids)), np.zeros(len(ids))
        self._ck(self._lib.plda_znorm_stats(self._h, _ptr(rows), rows.shape[0], nb, d, _ptr(models), len(ids),
                                            _ptr(mean), _ptr(std)))
        # insert-once, as unordered_map::insert (:245,250): only the labels without statistics yet (C-level loops: 50 000
        # models are 8 ms of per-key setdefault calls otherwise)
        fresh = [i for i, k in enumerate(ids) if k not in self._meanz] if self._meanz else None
        if fresh is None:
            keys = [int(k) for k in ids]
            self._meanz.update(zip(keys, mean.tolist()))
            self._stdvz.update(zip(keys, std.tolist()))
        elif fresh:
            keys = [int(ids[i]) for i in fresh]
            self._meanz.update(zip(keys, mean[fresh].tolist()))
            self._stdvz.update(zip(keys, std[fresh].tolist()))
        return None

    def znorm_stats(self):
        return dict(self._meanz), dict(self._stdvz)

    # ---------------------------------------------------------------- score
    def score(self, target, xvec, yvec):
        """MPlda_score (pldamodule.cpp:258-277): LLR of enrol model `xvec=(n, vec)`
        against test `yvec=(n, vec)`, z-normalised if `target` has statistics.

        One trial per call is latency, not throughput: plda_score_one evaluates it on the handle's host
        mirror of psi (a GPU round trip costs ten times the arithmetic); batches belong on score_matrix /
        score_trials."""
        if not isinstance(xvec, tuple) or not isinstance(yvec, tuple):
            raise TypeError("score(target, (n, vec), (n, vec)): enrol model and test must be tuples")
        u, v = xvec[1], yvec[1]
        if not (type(u) is np.ndarray and u.dtype == np.float64 and u.ndim == 1 and u.flags.c_contiguous):
            u = np.ascontiguousarray(np.asarray(u, np.float64).reshape(-1))
        if not (type(v) is np.ndarray and v.dtype == np.float64 and v.ndim == 1 and v.flags.c_contiguous):
            v = np.ascontiguousarray(np.asarray(v, np.float64).reshape(-1))
        dout = self._dout_cached()
        if u.shape[0] != dout or v.shape[0] != dout:
            raise ValueError("score: vectors must have the model dimension %d" % dout)
        tl = self.__dict__.get("_score_tls")
        if tl is None:
            tl = self._score_tls = threading.local()      # per thread: ctypes drops the GIL inside the call
        out = getattr(tl, "out", None)
        if out is None:
            out = tl.out = C.c_double()
        zm = self._meanz.get(int(target))
        if zm is None:
            rc = self._lib.plda_score_one(self._h, u.ctypes.data, int(xvec[0]), v.ctypes.data, 0, 0.0, 0.0, out)
        else:
            rc = self._lib.plda_score_one(self._h, u.ctypes.data, int(xvec[0]), v.ctypes.data, 1, zm,
                                          self._stdvz[int(target)], out)
        if rc:
            self._ck(rc)
        return out.value

    def score_on_device(self, target, xvec, yvec):
        """The same trial through the GPU's fp64 trial-list kernel (plda_score_pairs with P = 1): ~30 us per
        call; kept for parity tests of the two paths."""
        n = np.array([int(xvec[0])], np.int32)
        zero, out = np.zeros(1, np.int64), np.zeros(1)
        u = np.ascontiguousarray(np.asarray(xvec[1], np.float64).reshape(-1))
        v = np.ascontiguousarray(np.asarray(yvec[1], np.float64).reshape(-1))
        dout = self._dout_cached()
        if u.shape[0] != dout or v.shape[0] != dout:
            raise ValueError("score: vectors must have the model dimension %d" % dout)
        t = int(target)
        has_z = t in self._meanz
        zm, zs = np.array([self._meanz.get(t, 0.0)]), np.array([self._stdvz.get(t, 0.0)])
        self._ck(self._lib.plda_score_pairs(self._h, _ptr(u), _ptr(n), 1, _ptr(v), 1, _ptr(zero), _ptr(zero), 1,
                                            _ptr(zm) if has_z else None, _ptr(zs) if has_z else None, _ptr(out)))
        return float(out[0])

    def _dout_cached(self):
        d = self.__dict__.get("_dout")
        if d is None:
            d = self._dout = self.dims()[0]
        return d

    def _unpack(self, side):
        """dict {id: (n, vec)} or (counts, vecs[, ids]) -> ids, counts(int32), vecs."""
        if isinstance(side, Transformed):
            packed = getattr(side, "_packed", None)
            if packed is not None and packed[0].shape[0] == len(side):
                return packed[0], packed[1], self._check_dim(packed[2])
        if isinstance(side, dict):
            ids = np.array(list(side.keys()), dtype=np.int64)
            counts = np.array([int(side[k][0]) for k in side], np.int32)
            vecs = np.ascontiguousarray(np.stack([np.asarray(side[k][1], np.float64) for k in side]))
            return ids, counts, self._check_dim(vecs)
        counts, vecs = side[0], np.ascontiguousarray(side[1], np.float64)
        counts = np.ascontiguousarray(np.broadcast_to(np.asarray(counts), (vecs.shape[0],)), np.int32)
        ids = np.asarray(side[2], np.int64) if len(side) > 2 else None
        return ids, counts, self._check_dim(vecs)

    def _check_dim(self, vecs, what="vectors"):
        """The C side reads rows of exactly the model's current dimension: vectors transformed before a
        later truncate() / transform(targetdim=...) / load() / refit would be re-strided silently."""
        dout = self._dout_cached()
        if vecs.ndim != 2 or vecs.shape[1] != dout:
            raise ValueError("%s must be [rows, %d] (the model's current dimension), got %s"
                             % (what, dout, tuple(vecs.shape)))
        return vecs

    def _zn_arrays(self, ids, znorm):
        if not znorm or ids is None or not self._meanz:
            return None, None
        if len(ids) < 256:
            zm = np.array([self._meanz.get(int(k), 0.0) for k in ids])
            zs = np.array([self._stdvz.get(int(k), 0.0) if int(k) in self._meanz else 0.0 for k in ids])
            return zm, zs  # std 0 => that row is left un-normalised (engine convention)
        # many models: one sorted copy of the statistics (rebuilt when the dicts are replaced or grow -- entries are
        # insert-once, their values never change) and a vectorised lookup instead of two dict probes per model
        tag = (id(self._meanz), len(self._meanz), id(self._stdvz), len(self._stdvz))
        if getattr(self, "_zn_tag", None) != tag:
            keys = np.fromiter(self._meanz.keys(), np.int64, len(self._meanz))
            order = np.argsort(keys, kind="stable")
            self._zn_keys = keys[order]
            self._zn_mean = np.fromiter(self._meanz.values(), np.float64, len(self._meanz))[order]
            self._zn_std = np.fromiter((self._stdvz.get(k, 0.0) for k in self._meanz), np.float64, len(self._meanz))[order]
            self._zn_tag = tag
        ids = np.asarray(ids, np.int64)
        pos = np.minimum(np.searchsorted(self._zn_keys, ids), len(self._zn_keys) - 1)
        hit = self._zn_keys[pos] == ids
        return np.where(hit, self._zn_mean[pos], 0.0), np.where(hit, self._zn_std[pos], 0.0)

    def score_matrix(self, enrol, test, znorm=True, calibrate=False):
        """Dense trials matrix: float32 [M, Nt] of score(id_i, enrol_i, test_j) -- the nested
        loop of scoring/scorePLDA.py:302-318 / tests/pldatest.py:29-33 as one GEMM.  calibrate=True: mapped with the
        stored calibration (`calibrate`), (float)fma(a, (double)score, b)."""
        cal = self._stored_calibration(calibrate)
        ids, counts, U = self._unpack(enrol)
        _, _, V = self._unpack(test)
        m, nt = U.shape[0], V.shape[0]
        out = np.empty((m, nt), np.float32)   # every element is written; the pages are first touched by the copy threads
        if m == 0 or nt == 0:
            return out
        zm, zs = self._zn_arrays(ids, znorm)
        uniform = int(counts[0]) if np.all(counts == counts[0]) else 0
        if cal is not None:
            S = self._trials_matrix_on_device(counts, U, V, zn=(zm, zs))
            self._affine_map_on_device(S, cal)
            return S.cpu().numpy()
        self._ck(self._lib.plda_score_matrix(self._h, _ptr(U), None if uniform else _ptr(counts), uniform, m,
                                             _ptr(V), nt, _ptr(zm), _ptr(zs), _ptr(out), nt))
        return out

    def score_trials(self, enrol, test, e_idx, t_idx, znorm=True, calibrate=False):
        """Sparse trial list in fp64: out[p] = score(enrol[e_idx[p]], test[t_idx[p]]).  calibrate=True: a * score + b of the
        stored calibration, in fp64 on the host."""
        cal = self._stored_calibration(calibrate)
        if cal is not None:
            return cal(self.score_trials(enrol, test, e_idx, t_idx, znorm))
        ids, counts, U = self._unpack(enrol)
        _, _, V = self._unpack(test)
        e = np.ascontiguousarray(e_idx, np.int64).reshape(-1)
        t = np.ascontiguousarray(t_idx, np.int64).reshape(-1)
        out = np.zeros(e.shape[0])
        if e.shape[0] == 0:
            return out
        zm, zs = self._zn_arrays(ids, znorm)
        self._ck(self._lib.plda_score_pairs(self._h, _ptr(U), _ptr(counts), U.shape[0], _ptr(V), V.shape[0],
                                            _ptr(e), _ptr(t), e.shape[0], _ptr(zm), _ptr(zs), _ptr(out)))
        return out

    # ------------------------------------------------- S-norm / adaptive S-norm (csrc/snorm.hip)
    def _cohort_rows(self, cohort):
        """[Nc, Dout] array, or a dict / (counts, vecs) as `_unpack` takes (its counts are ignored: a cohort vector is one
        utterance)."""
        if isinstance(cohort, (dict, tuple, list)):
            return self._unpack(cohort)[2]
        return self._check_dim(np.ascontiguousarray(cohort, np.float64), "cohort")

    def _cohort_stats(self, counts, X, Cv, top_k):
        r, nc = X.shape[0], Cv.shape[0]
        k = nc if top_k is None else int(top_k)
        mean, std = np.empty(r), np.empty(r)
        if r == 0:
            return mean, std
        uniform = int(counts[0]) if np.all(counts == counts[0]) else 0
        self._ck(self._lib.plda_cohort_stats(self._h, _ptr(X), None if uniform else _ptr(counts), uniform, r, _ptr(Cv), nc, k,
                                             _ptr(mean), _ptr(std)))
        return mean, std

    def cohort_stats(self, side, cohort, top_k=None):
        """(mean, std) float64 [R] in the order of `side`: mean and population std of the top_k LARGEST scores of every
        row of `side` against the already-transformed `cohort` (top_k=None: all of it -- plain S-norm statistics)."""
        _, counts, X = self._unpack(side)
        return self._cohort_stats(counts, X, self._cohort_rows(cohort), top_k)

    def score_matrix_asnorm(self, enrol, test, cohort, top_k=None, calibrate=False):
        """float32 [M, Nt]: every trial normalised on both sides, 0.5 ((s - mean_e) / std_e + (s - mean_t) / std_t), the
        enrol model and the test vector each against the top_k closest vectors of `cohort` (a side whose std is 0 contributes
        the raw score).  The test side is scored with n = 1 whatever counts `test` stores, as in score_matrix.
        calibrate=True: mapped with the stored calibration as in score_matrix."""
        cal = self._stored_calibration(calibrate)
        _, counts, U = self._unpack(enrol)
        _, _, V = self._unpack(test)
        Cv = self._cohort_rows(cohort)
        m, nt = U.shape[0], V.shape[0]
        out = np.empty((m, nt), np.float32)
        if m == 0 or nt == 0:
            return out
        em, es = self._cohort_stats(counts, U, Cv, top_k)
        tm, ts = self._cohort_stats(np.ones(nt, np.int32), V, Cv, top_k)
        if cal is not None:
            S = self._trials_matrix_on_device(counts, U, V, sn=(em, es, tm, ts))
            self._affine_map_on_device(S, cal)
            return S.cpu().numpy()
        uniform = int(counts[0]) if np.all(counts == counts[0]) else 0
        self._ck(self._lib.plda_score_matrix_snorm(self._h, _ptr(U), None if uniform else _ptr(counts), uniform, m, _ptr(V), nt,
                                                   _ptr(em), _ptr(es), _ptr(tm), _ptr(ts), _ptr(out), nt))
        return out

    def score_trials_asnorm(self, enrol, test, e_idx, t_idx, cohort, top_k=None, calibrate=False):
        """The fp64 trial-list scores of score_trials(..., znorm=False) with the same two-sided map, applied on the host.
        calibrate=True: then a * score + b of the stored calibration."""
        cal = self._stored_calibration(calibrate)
        if cal is not None:
            return cal(self.score_trials_asnorm(enrol, test, e_idx, t_idx, cohort, top_k))
        _, counts, U = self._unpack(enrol)
        _, _, V = self._unpack(test)
        Cv = self._cohort_rows(cohort)
        e = np.ascontiguousarray(e_idx, np.int64).reshape(-1)
        t = np.ascontiguousarray(t_idx, np.int64).reshape(-1)
        raw = self.score_trials((counts, U), (np.ones(V.shape[0], np.int32), V), e, t, znorm=False)
        if e.shape[0] == 0:
            return raw
        em, es = self._cohort_stats(counts, U, Cv, top_k)
        tm, ts = self._cohort_stats(np.ones(V.shape[0], np.int32), V, Cv, top_k)

        def side(m, s):
            ok = s != 0.0
            return np.where(ok, (raw - m) / np.where(ok, s, 1.0), raw)
        return 0.5 * (side(em[e], es[e]) + side(tm[t], ts[t]))

    # ------------------------------------------------- top-N retrieval / rank-N identification (csrc/topn.hip)
    def top_n(self, enrol, test, n=10, per="test", znorm=True, cohort=None, top_k=None, calibrate=False):
        """(scores float32 [L, n], ids int64 [L, n]): per="test" -- for each of the L test entries its n best-scoring enrol
        models (closed-set identification); per="enrol" -- for each of the L enrol models its n best-scoring test entries
        (watch-list retrieval).  Best first; equal scores in the order of the other side.  The ids are the other side's keys,
        or positions where that side has none.  The scores are those of score_matrix (znorm) or, with a cohort, of
        score_matrix_asnorm; the matrix is never held (include/plda_hip.h, "top-N retrieval").  calibrate=True: the n scores
        are mapped with the stored calibration on the host, (float)fma(a, (double)score, b); a map with a <= 0 would not keep
        the order and is refused."""
        cal = self._stored_calibration(calibrate)
        if cal is not None and not cal.a > 0.0:
            raise ValueError("top_n: the stored calibration has a = %r; a map with a <= 0 does not keep the order of the scores" % cal.a)
        if per not in ("test", "enrol"):
            raise ValueError("top_n: per must be 'test' or 'enrol', got %r" % (per,))
        ids, counts, U = self._unpack(enrol)
        tids, _, V = self._unpack(test)
        m, nt = U.shape[0], V.shape[0]
        axis, lines, other = (1, nt, ids) if per == "test" else (0, m, tids)
        if m == 0 or nt == 0:
            raise ValueError("top_n: no trials")
        n = int(n)
        if n < 1:
            raise ValueError("top_n: n = %d (must be >= 1)" % n)
        scores, index = np.empty((lines, n), np.float32), np.empty((lines, n), np.int64)
        zm = zs = em = es = tm = ts = None
        if cohort is None:
            zm, zs = self._zn_arrays(ids, znorm)
        else:
            Cv = self._cohort_rows(cohort)
            em, es = self._cohort_stats(counts, U, Cv, top_k)
            tm, ts = self._cohort_stats(np.ones(nt, np.int32), V, Cv, top_k)
        uniform = int(counts[0]) if np.all(counts == counts[0]) else 0
        self._ck(self._lib.plda_score_topn(self._h, _ptr(U), None if uniform else _ptr(counts), uniform, m, _ptr(V), nt,
                                           _ptr(zm), _ptr(zs), _ptr(em), _ptr(es), _ptr(tm), _ptr(ts), axis, n,
                                           _ptr(scores), _ptr(index)))
        if cal is not None:
            from . import identify as ID
            scores = ID.affine_f32(cal.a, scores, cal.b)
        return scores, (index if other is None else np.asarray(other, np.int64)[index])

    # ------------------------------------------------- score calibration (csrc/calib.hip, plda_amd/calibration.py)
    def _stored_calibration(self, calibrate):
        if not calibrate:
            return None
        if self._calibration is None:
            raise ValueError("calibrate=True needs a stored calibration: call calibrate() (or load a file that holds one) first")
        return self._calibration

    def _to_device(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", self.device))

    def _trials_matrix_on_device(self, counts, U, V, zn=(None, None), sn=None):
        """The fp32 [M, Nt] matrix of score_matrix (zn: z-norm statistics or Nones) or score_matrix_asnorm (sn: the four
        cohort statistics) as a device tensor."""
        import torch
        m, nt = U.shape[0], V.shape[0]
        uniform = int(counts[0]) if np.all(counts == counts[0]) else 0
        dU, dV = self._to_device(U), self._to_device(V)
        dn = None if uniform else self._to_device(counts)
        S = torch.empty((m, nt), dtype=torch.float32, device=dU.device)
        ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
        if sn is not None:
            st = [self._to_device(x) for x in sn]
            self.score_matrix_snorm_dev(dU.data_ptr(), ptr(dn), uniform, m, dV.data_ptr(), nt, S.data_ptr(), nt,
                                        st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(), st[3].data_ptr())
        else:
            st = [self._to_device(x) if x is not None else None for x in zn]
            self.score_matrix_dev(dU.data_ptr(), ptr(dn), uniform, m, dV.data_ptr(), nt, S.data_ptr(), nt, ptr(st[0]), ptr(st[1]))
        self.synchronize()           # (the operands may be freed when this returns)
        return S

    def _affine_map_on_device(self, S, cal):
        from . import calibration as CB
        CB.apply_dev(self, S.data_ptr(), S.shape[1], S.shape[0], S.shape[1], cal)
        self.synchronize()

    def _labelled_trials(self, enrol, test, test_speaker, what):
        """(enrol ids, counts, U, V, int64 speaker of every test entry) of the labelled trials between two transform()
        results: the argument handling `calibrate` and `min_dcf` share."""
        ids, counts, U = self._unpack(enrol)
        tids, _, V = self._unpack(test)
        m, nt = U.shape[0], V.shape[0]
        if ids is None:
            raise ValueError("%s: the enrol side needs its speaker ids (a transform() result or (counts, vecs, ids))" % what)
        if hasattr(test_speaker, "keys"):
            if tids is None:
                raise ValueError("%s: a test_speaker mapping needs test keys" % what)
            tspk = np.array([int(test_speaker[int(k)]) for k in tids], np.int64)
        else:
            tspk = np.ascontiguousarray(test_speaker, np.int64).reshape(-1)
        if tspk.shape[0] != nt:
            raise ValueError("%s: test_speaker must name the speaker of each of the %d test entries" % (what, nt))
        if m == 0 or nt == 0:
            raise ValueError("%s: no trials" % what)
        return ids, counts, U, V, tspk

    def min_dcf(self, enrol, test, test_speaker, points=((0.01, 1.0, 1.0),), znorm=True, cohort=None, top_k=None, calibrate=False):
        """The exact minimum detection cost of the trials between two transform() results at the operating points
        `points` = ((prior, c_miss, c_fa), ...), at most 8 (include/plda_hip.h, "exact minimum detection cost").  Arguments
        as `calibrate`; the scores are those of score_matrix (znorm) or, with a cohort, score_matrix_asnorm, and with
        calibrate=True they are mapped with the stored calibration first.  Without a cohort and without the map the matrix
        is never held (the trials are re-scored slab by slab once per read); otherwise it is.  Returns (one dict per point:
        min_dcf, threshold, far, frr, miss, fa; the call's info dict).  The calibration loss at a point is
        `calibration.act_dcf(...) - min_dcf`."""
        from . import dcf as DC
        cal = self._stored_calibration(calibrate)
        ids, counts, U, V, tspk = self._labelled_trials(enrol, test, test_speaker, "min_dcf")
        m, nt = U.shape[0], V.shape[0]
        despk, dtspk = self._to_device(np.ascontiguousarray(ids, np.int64)), self._to_device(tspk)
        if cohort is None and cal is None:
            zm, zs = self._zn_arrays(ids, znorm)
            uniform = int(counts[0]) if np.all(counts == counts[0]) else 0
            dU, dV = self._to_device(U), self._to_device(V)
            dn = None if uniform else self._to_device(counts)
            dzm, dzs = (self._to_device(zm), self._to_device(zs)) if zm is not None else (None, None)
            ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
            return DC.min_dcf_from_operands_dev(self, dU.data_ptr(), ptr(dn), uniform, m, dV.data_ptr(), nt, despk.data_ptr(),
                                                dtspk.data_ptr(), ptr(dzm), ptr(dzs), points=points)
        if cohort is None:
            S = self._trials_matrix_on_device(counts, U, V, zn=self._zn_arrays(ids, znorm))
        else:
            Cv = self._cohort_rows(cohort)
            em, es = self._cohort_stats(counts, U, Cv, top_k)
            tm, ts = self._cohort_stats(np.ones(nt, np.int32), V, Cv, top_k)
            S = self._trials_matrix_on_device(counts, U, V, sn=(em, es, tm, ts))
        if cal is not None:
            self._affine_map_on_device(S, cal)
        return DC.min_dcf_from_matrix_dev(self, S.data_ptr(), nt, m, nt, despk.data_ptr(), dtspk.data_ptr(), points=points)

    # ------------------------------------------------- trial keys (csrc/partition.hip, plda_amd/trialkey.py)
    def partition(self, enrol, test, test_speaker, key=None, znorm=True, cohort=None, top_k=None, calibrate=False):
        """The per-(bucket, class) score lists of the trials between two transform() results under a
        `plda_amd.trialkey.TrialKey` (None: every pair is a trial, one bucket), on the device: a
        `plda_amd.trialkey.Partition` (include/plda_hip.h, "trial keys"), for a DET plot or a score file.  Arguments as
        `min_dcf`.  Without a cohort and without the map the matrix is never held (the trials are scored slab by slab and
        only the selected ones are written); otherwise it is."""
        from . import trialkey as TK
        cal = self._stored_calibration(calibrate)
        ids, counts, U, V, tspk = self._labelled_trials(enrol, test, test_speaker, "partition")
        m, nt = U.shape[0], V.shape[0]
        if key is None:
            key = TK.TrialKey(m, nt, "all")
        if key.shape != (m, nt):
            raise ValueError("partition: the key covers %d x %d pairs, the trials are %d x %d" % (key.shape + (m, nt)))
        despk, dtspk = self._to_device(np.ascontiguousarray(ids, np.int64)), self._to_device(tspk)
        if cohort is None and cal is None:
            zm, zs = self._zn_arrays(ids, znorm)
            uniform = int(counts[0]) if np.all(counts == counts[0]) else 0
            dU, dV = self._to_device(U), self._to_device(V)
            dn = None if uniform else self._to_device(counts)
            dzm, dzs = (self._to_device(zm), self._to_device(zs)) if zm is not None else (None, None)
            return TK.partition_from_operands_dev(self, key, dU, dn, uniform, dV, despk, dtspk, dzm, dzs)
        S = self._own_matrix_on_device(ids, counts, U, V, znorm, cohort, top_k)
        if cal is not None:
            self._affine_map_on_device(S, cal)
        part = TK.partition_matrix_dev(self, key, S, despk, dtspk)
        self.synchronize()           # (the matrix may be freed when this returns)
        return part

    def evaluate(self, enrol, test, test_speaker, key=None, points=((0.01, 1.0, 1.0),), znorm=True, cohort=None, top_k=None,
                 calibrate=False, prior=0.5):
        """Per-condition, pooled and equalised figures of the trials between two transform() results under a trial key
        (None: every pair, one bucket): `plda_amd.trialkey.metrics` of `partition(...)` -- EER, minDCF and actual DCF at
        `points`, Cllr and minCllr per bucket, over all trials, and as the unweighted mean over the buckets that hold both
        classes (NIST's equalisation).  Nothing leaves the device but the figures."""
        from . import trialkey as TK
        part = self.partition(enrol, test, test_speaker, key, znorm, cohort, top_k, calibrate)
        return TK.metrics(self, part, points=points, prior=prior)

    def min_cllr(self, enrol, test, test_speaker, znorm=True, cohort=None, top_k=None):
        """minCllr, the ROC convex hull and the PAV map of the trials between two transform() results (include/plda_hip.h,
        "ROC convex hull").  Arguments as `min_dcf`; the scores are those of score_matrix (znorm) or, with a cohort,
        score_matrix_asnorm.  Without a cohort the matrix is never held (the trials are re-scored slab by slab once per
        read).  Returns (result dict: Np, Nn, n_vertices, min_cllr, eer, ...; a plda_amd.rocch.Pav).  The calibration loss of
        a calibration is its `cllr_after - min_cllr`."""
        from . import rocch as RC
        ids, counts, U, V, tspk = self._labelled_trials(enrol, test, test_speaker, "min_cllr")
        m, nt = U.shape[0], V.shape[0]
        despk, dtspk = self._to_device(np.ascontiguousarray(ids, np.int64)), self._to_device(tspk)
        if cohort is None:
            zm, zs = self._zn_arrays(ids, znorm)
            uniform = int(counts[0]) if np.all(counts == counts[0]) else 0
            dU, dV = self._to_device(U), self._to_device(V)
            dn = None if uniform else self._to_device(counts)
            dzm, dzs = (self._to_device(zm), self._to_device(zs)) if zm is not None else (None, None)
            ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
            res, pav, _ = RC.rocch_from_operands_dev(self, dU.data_ptr(), ptr(dn), uniform, m, dV.data_ptr(), nt, despk.data_ptr(),
                                                     dtspk.data_ptr(), ptr(dzm), ptr(dzs))
            return res, pav
        Cv = self._cohort_rows(cohort)
        em, es = self._cohort_stats(counts, U, Cv, top_k)
        tm, ts = self._cohort_stats(np.ones(nt, np.int32), V, Cv, top_k)
        S = self._trials_matrix_on_device(counts, U, V, sn=(em, es, tm, ts))
        res, pav, _ = RC.rocch_from_matrix_dev(self, S.data_ptr(), nt, m, nt, despk.data_ptr(), dtspk.data_ptr())
        return res, pav

    def calibrate_pav(self, enrol, test, test_speaker, znorm=True, cohort=None, top_k=None):
        """`min_cllr`, and the PAV map is stored as `self.pav` (the non-parametric reference beside `calibrate`'s affine map:
        apply it with `self.pav(scores)` or `self.pav.apply_dev(...)`).  The affine calibration, `score_matrix` and their
        `calibrate=True` paths are not touched.  Returns the Pav."""
        _, self.pav = self.min_cllr(enrol, test, test_speaker, znorm, cohort, top_k)
        return self.pav

    def calibrate(self, enrol, test, test_speaker, prior=0.5, znorm=True, cohort=None, top_k=None):
        """Fit the linear calibration llr = a * score + b (prior-weighted logistic regression, include/plda_hip.h) on the
        trials between two transform() results and store it.  The enrol keys are the model speakers; `test_speaker` gives
        the speaker of every test entry, as a mapping {test key: speaker} or a sequence in the order of `test`.  The
        scores are normalised first exactly as score_matrix (znorm) or, with a cohort, score_matrix_asnorm would.  Without a
        cohort the matrix is never held (the trials are re-scored slab by slab once per pass); with one it is.  Returns the
        `plda_amd.calibration.Calibration`; a separable or unconverged fit raises a RuntimeWarning."""
        from . import calibration as CB
        ids, counts, U, V, tspk = self._labelled_trials(enrol, test, test_speaker, "calibrate")
        m, nt = U.shape[0], V.shape[0]
        despk, dtspk = self._to_device(np.ascontiguousarray(ids, np.int64)), self._to_device(tspk)
        if cohort is None:
            zm, zs = self._zn_arrays(ids, znorm)
            uniform = int(counts[0]) if np.all(counts == counts[0]) else 0
            dU, dV = self._to_device(U), self._to_device(V)
            dn = None if uniform else self._to_device(counts)
            dzm, dzs = (self._to_device(zm), self._to_device(zs)) if zm is not None else (None, None)
            ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
            cal = CB.fit_from_operands_dev(self, dU.data_ptr(), ptr(dn), uniform, m, dV.data_ptr(), nt, despk.data_ptr(),
                                           dtspk.data_ptr(), ptr(dzm), ptr(dzs), prior=prior)
        else:
            Cv = self._cohort_rows(cohort)
            em, es = self._cohort_stats(counts, U, Cv, top_k)
            tm, ts = self._cohort_stats(np.ones(nt, np.int32), V, Cv, top_k)
            S = self._trials_matrix_on_device(counts, U, V, sn=(em, es, tm, ts))
            cal = CB.fit_from_matrix_dev(self, S.data_ptr(), nt, m, nt, despk.data_ptr(), dtspk.data_ptr(), prior=prior)
        self._calibration = cal
        return cal

    @property
    def calibration(self):
        """The stored `plda_amd.calibration.Calibration`, or None."""
        return self._calibration

    # ------------------------------------------------- multi-system score fusion (csrc/fusion.hip, plda_amd/fusion.py)
    def _own_matrix_on_device(self, ids, counts, U, V, znorm, cohort, top_k):
        """This model's fp32 [M, Nt] trials matrix as a device tensor, normalised as score_matrix (znorm) or, with a cohort,
        score_matrix_asnorm would."""
        if cohort is None:
            return self._trials_matrix_on_device(counts, U, V, zn=self._zn_arrays(ids, znorm))
        Cv = self._cohort_rows(cohort)
        em, es = self._cohort_stats(counts, U, Cv, top_k)
        tm, ts = self._cohort_stats(np.ones(V.shape[0], np.int32), V, Cv, top_k)
        return self._trials_matrix_on_device(counts, U, V, sn=(em, es, tm, ts))

    def _other_matrices_on_device(self, others, m, nt, what):
        """The other systems' fp32 [M, Nt] matrices as device tensors (NumPy arrays are uploaded; torch device tensors are
        taken as they are, last dimension contiguous) and their row pitches."""
        import torch
        if len(others) < 1 or len(others) > 7:
            raise ValueError("%s: 1 .. 7 other systems (a fusion has at most 8)" % what)
        out = []
        for i, o in enumerate(others):
            if not isinstance(o, torch.Tensor):
                o = self._to_device(np.ascontiguousarray(o, np.float32))
            if o.dtype != torch.float32 or tuple(o.shape) != (m, nt) or not o.is_cuda or (nt > 1 and o.stride(1) != 1):
                raise ValueError("%s: others[%d] must be an fp32 [%d, %d] matrix (NumPy, or a torch device tensor with "
                                 "contiguous rows)" % (what, i, m, nt))
            out.append(o)
        return out, [int(o.stride(0)) if m > 1 else nt for o in out]

    def fuse(self, enrol, test, test_speaker, others, prior=0.5, znorm=True, cohort=None, top_k=None):
        """Fit the linear fusion llr = b + a_0 * (this model's score) + sum_k a_k * others[k-1] by prior-weighted logistic
        regression (include/plda_hip.h, "multi-system score fusion") on the trials between two transform() results.  This
        model's matrix is normalised exactly as `calibrate` would; `others` is a sequence of fp32 [M, Nt] matrices of other
        systems in the same row / column order, NumPy or torch device tensors (e.g. the transposed LDA.predict_log_proba
        columns of the enrolled speakers).  Returns the `plda_amd.fusion.Fusion`; it is NOT stored and not written by save():
        its weights belong to a set of systems, not to this model.  A separable or unconverged fit raises a RuntimeWarning."""
        from . import fusion as FU
        ids, counts, U, V, tspk = self._labelled_trials(enrol, test, test_speaker, "fuse")
        m, nt = U.shape[0], V.shape[0]
        oth, lds = self._other_matrices_on_device(others, m, nt, "fuse")
        despk, dtspk = self._to_device(np.ascontiguousarray(ids, np.int64)), self._to_device(tspk)
        S = self._own_matrix_on_device(ids, counts, U, V, znorm, cohort, top_k)
        import torch
        torch.cuda.synchronize(S.device)     # (uploads and the callers' tensors live on torch's streams)
        return FU.fit_from_matrices_dev(self, [S.data_ptr()] + [o.data_ptr() for o in oth], [nt] + lds, m, nt, despk.data_ptr(),
                                        dtspk.data_ptr(), prior=prior)

    def score_matrix_fused(self, enrol, test, others, fusion, znorm=True, cohort=None, top_k=None, quality=None):
        """float32 [M, Nt]: the fused value of `fusion` (a `plda_amd.fusion.Fusion` over this model's matrix, normalised as in
        `fuse`, followed by `others`), the FMA chain of the header rounded once to fp32.  With `quality` (the argument of
        `calibrate_quality`) `fusion` is that call's `QualityFusion`, and `others` may be empty."""
        from . import fusion as FU
        ids, counts, U = self._unpack(enrol)
        tids, _, V = self._unpack(test)
        m, nt = U.shape[0], V.shape[0]
        if m == 0 or nt == 0:
            return np.empty((m, nt), np.float32)
        if quality is None:
            oth, lds = self._other_matrices_on_device(others, m, nt, "score_matrix_fused")
            sides = []
        else:
            oth, lds = self._other_matrices_on_device(others, m, nt, "score_matrix_fused") if len(others) else ([], [])
            sides = self._quality_sides(quality, ids, tids, m, nt, "score_matrix_fused")
            if getattr(fusion, "n_sides", 0) != len(sides) or tuple(fusion.ops) != tuple(s.op for s in sides):
                raise ValueError("score_matrix_fused: the fusion was fitted on the sides %r, got %r"
                                 % (getattr(fusion, "ops", ()), tuple(s.op for s in sides)))
        if fusion.n_systems != 1 + len(oth) or (quality is None and getattr(fusion, "n_sides", 0)):
            raise ValueError("score_matrix_fused: the fusion was fitted on %d systems%s, got %d" % (
                fusion.n_systems, " and %d sides" % fusion.n_sides if getattr(fusion, "n_sides", 0) else "", 1 + len(oth)))
        S = self._own_matrix_on_device(ids, counts, U, V, znorm, cohort, top_k)
        import torch
        torch.cuda.synchronize(S.device)
        ptrs, pitches = [S.data_ptr()] + [o.data_ptr() for o in oth], [nt] + lds
        if sides:
            keep = FU.apply_with_sides_dev(self, ptrs, pitches, sides, m, nt, fusion, S.data_ptr(), nt)
        else:
            FU.apply_dev(self, ptrs, pitches, m, nt, fusion, S.data_ptr(), nt)
        self.synchronize()
        keep = None     # noqa: F841  (the side vectors had to outlive the enqueued map)
        return S.cpu().numpy()

    # ------------------------------------------------- quality-aware calibration (K25; csrc/fusion.hip)
    def _quality_sides(self, quality, ids, tids, m, nt, what):
        """`quality` = ((op, enrol_values, test_values), ...) -> `plda_amd.fusion.Side`s with device vectors.  Each values
        argument is a mapping {key: value} (looked up by the enrol / test keys) or a sequence in the order of enrol / test:
        the convention of `test_speaker`."""
        from . import fusion as FU

        def values(v, keys, n, which, q):
            if hasattr(v, "keys"):
                if keys is None:
                    raise ValueError("%s: quality %d: a mapping of %s values needs %s keys" % (what, q, which, which))
                v = [float(v[int(k)]) for k in keys]
            v = np.ascontiguousarray(v, np.float32).reshape(-1)
            if v.shape[0] != n:
                raise ValueError("%s: quality %d: %d %s values for %d %s entries" % (what, q, v.shape[0], which, n, which))
            return v
        sides = []
        for q, item in enumerate(quality):
            if len(item) != 3:
                raise ValueError("%s: quality %d is not (op, enrol_values, test_values)" % (what, q))
            op, ev, tv = item
            sides.append(FU.Side(op, values(ev, ids, m, "enrol", q), values(tv, tids, nt, "test", q)))
        import torch
        dev = torch.device("cuda", self.device)
        return [s.on(dev) for s in sides]

    def calibrate_quality(self, enrol, test, test_speaker, quality, others=(), prior=0.5, znorm=True, cohort=None, top_k=None):
        """Quality-aware calibration (include/plda_hip.h, "quality-aware calibration"): fit llr = b + a_0 * (this model's
        score) + sum a_k * others[k-1] + sum a_q * side_q, where side q = op(enrol quality of the row, test quality of the
        column) -- `quality` is a sequence of (op, enrol_values, test_values), op one of "min" | "max" | "sum" | "absdiff" |
        "prod", each values argument a mapping {key: value} or a sequence in the order of `enrol` / `test` (the convention of
        `test_speaker`).  A side's [M, Nt] values are formed in registers, never in memory.  Other arguments as `fuse`; at
        most 8 systems and sides together.  With no `others` and no cohort this model's matrix is never held either (the
        operand form, as `calibrate`); otherwise it is.  Returns the `plda_amd.fusion.QualityFusion`; it is NOT stored,
        like `fuse`'s result.  Apply it with `score_matrix_fused(..., quality=quality)`."""
        from . import fusion as FU
        ids, counts, U, V, tspk = self._labelled_trials(enrol, test, test_speaker, "calibrate_quality")
        tids = self._unpack(test)[0]
        m, nt = U.shape[0], V.shape[0]
        quality = list(quality)
        if 1 + len(others) + len(quality) > FU.MAX_SYSTEMS:
            raise ValueError("calibrate_quality: at most %d systems and sides together" % FU.MAX_SYSTEMS)
        sides = self._quality_sides(quality, ids, tids, m, nt, "calibrate_quality")
        despk, dtspk = self._to_device(np.ascontiguousarray(ids, np.int64)), self._to_device(tspk)
        import torch
        if cohort is None and not len(others):
            zm, zs = self._zn_arrays(ids, znorm)
            uniform = int(counts[0]) if np.all(counts == counts[0]) else 0
            dU, dV = self._to_device(U), self._to_device(V)
            dn = None if uniform else self._to_device(counts)
            dzm, dzs = (self._to_device(zm), self._to_device(zs)) if zm is not None else (None, None)
            ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
            torch.cuda.synchronize(dU.device)
            return FU.fit_from_operands_with_sides_dev(self, dU.data_ptr(), ptr(dn), uniform, m, dV.data_ptr(), nt, ptr(dzm), ptr(dzs),
                                                       despk.data_ptr(), dtspk.data_ptr(), sides, prior=prior)
        oth, lds = self._other_matrices_on_device(others, m, nt, "calibrate_quality") if len(others) else ([], [])
        S = self._own_matrix_on_device(ids, counts, U, V, znorm, cohort, top_k)
        torch.cuda.synchronize(S.device)
        return FU.fit_with_sides_dev(self, [S.data_ptr()] + [o.data_ptr() for o in oth], [nt] + lds, sides, m, nt, despk.data_ptr(),
                                     dtspk.data_ptr(), prior=prior)

    # ------------------------------------------------- device-resident path
    def set_stream(self, hip_stream):
        """Enqueue on this hipStream_t (an int handle, e.g. torch.cuda.current_stream().cuda_stream;
        0 is HIP's default stream).  None returns to the handle's own stream."""
        if hip_stream is None:
            self._ck(self._lib.plda_reset_stream(self._h))
        else:
            self._ck(self._lib.plda_set_stream(self._h, C.c_void_p(int(hip_stream))))

    def synchronize(self):
        self._ck(self._lib.plda_synchronize(self._h))

    def trace_enable(self, on=True):
        """Per-stage timing spans (include/plda_hip.h: plda_trace_*; PLDA_HIP_TRACE=1 turns it on from creation)."""
        self._ck(self._lib.plda_trace_enable(self._h, 1 if on else 0))

    def trace_read(self, reset=True):
        """list of dict(name, calls, ms, work, unit) aggregated by stage name."""
        import json
        buf = C.create_string_buffer(1 << 16)
        self._ck(self._lib.plda_trace_read(self._h, buf, len(buf), 1 if reset else 0))
        return json.loads(buf.value.decode())

    def sym_eig(self, G, method=0):
        """Eigen-decomposition of a symmetric matrix by the GetOutput eigensolver (diagnostics / tests):
        (eigenvalues descending, eigenvectors in ROWS, method used: 1 = block Jacobi, 2 = direct)."""
        G = np.ascontiguousarray(G, dtype=np.float64)
        if G.ndim != 2 or G.shape[0] != G.shape[1]:
            raise ValueError("sym_eig: square matrix expected")
        d = G.shape[0]
        lam, vec, used = np.zeros(d), np.zeros((d, d)), C.c_int32(0)
        self._ck(self._lib.plda_sym_eig(self._h, _ptr(G), d, int(method), _ptr(lam), _ptr(vec), C.byref(used)))
        return lam, vec, used.value

    def gemm_f64(self, A, B, alpha=1.0, beta=0.0, C_in=None, transA=False, transB=False, kw=None):
        """alpha op(A) op(B) + beta C by the engine's fp64 GEMM (diagnostics / tests); A, B 2-D, or 3-D for a batch."""
        A = np.ascontiguousarray(A, np.float64); B = np.ascontiguousarray(B, np.float64)
        batch = A.shape[0] if A.ndim == 3 else 1
        a2, b2 = A.shape[-2:], B.shape[-2:]
        m, k = (a2[1], a2[0]) if transA else a2
        k2, n = (b2[1], b2[0]) if transB else b2
        if k != k2 or (B.ndim == 3) != (A.ndim == 3) or (B.ndim == 3 and B.shape[0] != batch):
            raise ValueError("gemm_f64: shapes disagree")
        shape = (batch, m, n) if A.ndim == 3 else (m, n)
        out = np.zeros(shape) if C_in is None else np.ascontiguousarray(C_in, np.float64).reshape(shape).copy()
        w = None if kw is None else np.ascontiguousarray(kw, np.float64)
        self._ck(self._lib.plda_gemm_f64(self._h, m, n, k, float(alpha), _ptr(A), int(transA), _ptr(B), int(transB),
                                         _ptr(w) if w is not None else None, float(beta), _ptr(out), batch))
        return out

    def spd_inverse(self, A):
        """Inverse of a symmetric positive definite matrix by the E-step's kernels (diagnostics / tests)."""
        A = np.ascontiguousarray(A, dtype=np.float64)
        if A.ndim != 2 or A.shape[0] != A.shape[1]:
            raise ValueError("spd_inverse: square matrix expected")
        out = np.empty_like(A)
        self._ck(self._lib.plda_spd_inverse(self._h, _ptr(A), A.shape[0], _ptr(out)))
        return out

    def profile_enable(self, on=True):
        self._ck(self._lib.plda_profile_enable(self._h, 1 if on else 0))

    def profile_read(self, reset=True):
        """(GEMM ms, launches, algorithmic flop) accumulated by HIP events on the kernel's stream."""
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        self._ck(self._lib.plda_profile_read(self._h, C.byref(ms), C.byref(n), C.byref(fl), 1 if reset else 0))
        return ms.value, n.value, fl.value

    def fit_dev(self, dX, n, d, dlabels, k, iters=10):
        self._dout = None            # the model dimension may change
        self._ck(self._lib.plda_fit_dev(self._h, C.c_void_p(int(dX)), int(n), int(d), C.c_void_p(int(dlabels)),
                                        int(k), int(iters)))

    def fit_stats_dev(self, dX, n, d, dlabels, k):
        """Statistics pass only (pldamodule.cpp:76-100) over this handle's share of the speakers."""
        self._ck(self._lib.plda_fit_stats_dev(self._h, C.c_void_p(int(dX)), int(n), int(d),
                                              C.c_void_p(int(dlabels)), int(k)))

    def fit_get_stats_dev(self, dmeans, dcounts, dscatter):
        self._ck(self._lib.plda_fit_get_stats_dev(self._h, C.c_void_p(int(dmeans)) if dmeans else None,
                                                  C.c_void_p(int(dcounts)) if dcounts else None,
                                                  C.c_void_p(int(dscatter)) if dscatter else None))

    def fit_em_dev(self, dmeans, dcounts, k, dscatter, d, iters=10):
        """EM + GetOutput (pldamodule.cpp:102-106) on merged statistics."""
        self._dout = None            # the model dimension may change
        rc = self._lib.plda_fit_em_dev(self._h, C.c_void_p(int(dmeans)), C.c_void_p(int(dcounts)), int(k),
                                       C.c_void_p(int(dscatter)), int(d), int(iters))
        if rc == -2:
            raise ValueError(self._lib.plda_last_error(self._h).decode())
        self._ck(rc)

    def transform_rows_dev(self, dX, r, d, dn, n_uniform, dout):
        self._ck(self._lib.plda_transform_rows_dev(self._h, C.c_void_p(int(dX)), int(r), int(d),
                                                   C.c_void_p(int(dn)) if dn else None, int(n_uniform),
                                                   C.c_void_p(int(dout))))

    def score_last_kernel(self):
        """Name of the trials-GEMM kernel the last score_matrix* call launched."""
        buf = C.create_string_buffer(128)
        self._ck(self._lib.plda_score_last_kernel(self._h, buf, 128))
        return buf.value.decode()

    def linalg_last_kernels(self):
        """The kernels (template arguments included) that the fp64 building blocks dispatched since the last sym_eig,
        gemm_f64 or spd_inverse call began, each once, in the order of first launch (tests pin dispatch classes by it)."""
        buf = C.create_string_buffer(1024)
        self._ck(self._lib.plda_linalg_last_kernels(self._h, buf, 1024))
        return [k for k in buf.value.decode().split(";") if k]

    def score_last_shape(self):
        """(M, Nt, algorithmic GEMM depth) of the last score_matrix* call: depth Dout (uniform count), Dout + G - 1
        (mixed counts, bucketed by the G distinct counts) or 2 Dout (mixed counts, depth-2D form)."""
        m, nt, k = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        self._ck(self._lib.plda_score_last_shape(self._h, C.byref(m), C.byref(nt), C.byref(k)))
        return int(m.value), int(nt.value), int(k.value)

    def score_matrix_dev(self, dU, dn, n_uniform, m, dV, nt, dout, ld, dzmean=None, dzstd=None):
        """Enqueue one trials block on HBM-resident operands (raw device addresses)."""
        self._ck(self._lib.plda_score_matrix_dev(
            self._h, C.c_void_p(int(dU)), C.c_void_p(int(dn)) if dn else None, int(n_uniform), int(m),
            C.c_void_p(int(dV)), int(nt), C.c_void_p(int(dzmean)) if dzmean else None,
            C.c_void_p(int(dzstd)) if dzstd else None, C.c_void_p(int(dout)), int(ld)))

    def cohort_stats_dev(self, dX, dn, n_uniform, r, dC, nc, top_k, dmean, dstd):
        """Enqueue the top_k cohort statistics of r HBM-resident rows (raw device addresses; dmean, dstd: float64 [r])."""
        self._ck(self._lib.plda_cohort_stats_dev(
            self._h, C.c_void_p(int(dX)), C.c_void_p(int(dn)) if dn else None, int(n_uniform), int(r), C.c_void_p(int(dC)),
            int(nc), int(top_k), C.c_void_p(int(dmean)) if dmean else None, C.c_void_p(int(dstd)) if dstd else None))

    def score_matrix_snorm_dev(self, dU, dn, n_uniform, m, dV, nt, dout, ld, demean=None, destd=None, dtmean=None, dtstd=None):
        """Enqueue one trials block normalised with per-row (demean, destd) and / or per-column (dtmean, dtstd) statistics."""
        self._ck(self._lib.plda_score_matrix_snorm_dev(
            self._h, _vp(dU), _vp(dn), int(n_uniform), int(m), _vp(dV), int(nt), _vp(demean), _vp(destd), _vp(dtmean), _vp(dtstd),
            _vp(dout), int(ld)))

    def topn_matrix_dev(self, dscores, ld, m, nt, axis, top_n, dout_scores, dout_index):
        """Enqueue the top_n selection with indices on an HBM-resident fp32 matrix [m, nt] (row pitch ld): per row (axis 0) or
        per column (axis 1); dout_scores float32, dout_index int64, both [lines, top_n]."""
        self._ck(self._lib.plda_topn_matrix_dev(self._h, _vp(dscores), int(ld), int(m), int(nt), int(axis), int(top_n),
                                                _vp(dout_scores), _vp(dout_index)))

    def score_topn_dev(self, dU, dn, n_uniform, m, dV, nt, axis, top_n, dout_scores, dout_index, dzmean=None, dzstd=None,
                       demean=None, destd=None, dtmean=None, dtstd=None):
        """The same selection on the trials of HBM-resident operands, the matrix never held: the scores of score_matrix_dev
        (dzmean, dzstd) or, with demean / destd and / or dtmean / dtstd, of score_matrix_snorm_dev."""
        self._ck(self._lib.plda_score_topn_dev(
            self._h, _vp(dU), _vp(dn), int(n_uniform), int(m), _vp(dV), int(nt), _vp(dzmean), _vp(dzstd), _vp(demean), _vp(destd),
            _vp(dtmean), _vp(dtstd), int(axis), int(top_n), _vp(dout_scores), _vp(dout_index)))

    def score_prepare_dev(self, dV, nt, mixed_counts=False, n_uniform=1):
        """Pack the test side [nt, Dout] (HBM-resident fp64) once; later score_matrix_dev / sharded calls with the same
        dV, nt, model and kind of enrol counts skip the repacking.  The rows behind dV must not change meanwhile."""
        self._ck(self._lib.plda_score_prepare_dev(self._h, C.c_void_p(int(dV)), int(nt), 1 if mixed_counts else 0, int(n_uniform)))

    def score_prepare_counts_dev(self, dV, nt, counts):
        """Pack the test side for mixed enrol counts in the bucketed form (GEMM depth Dout + G - 1): `counts` = the enrol
        counts the later calls will bring (any order, duplicates allowed; a host array)."""
        c = np.ascontiguousarray(np.asarray(counts).ravel(), dtype=np.int32)
        self._ck(self._lib.plda_score_prepare_counts_dev(self._h, C.c_void_p(int(dV)), int(nt), _ptr(c), int(c.shape[0])))

    def score_unprepare(self):
        self._ck(self._lib.plda_score_unprepare(self._h))

    # ------------------------------------------------- several GPUs (csrc/comm.hip)
    @staticmethod
    def comm_unique_id():
        """128 bytes for rank 0 to hand to every rank's comm_init (ncclGetUniqueId)."""
        buf = C.create_string_buffer(128)
        rc = N.load().plda_comm_unique_id(buf, 128)
        if rc != N.PLDA_OK:
            raise N.PldaError(rc, "plda_comm_unique_id failed")
        return buf.raw

    def comm_init(self, nranks, rank, unique_id):
        """Collective: RCCL communicator of this handle (one process per GPU)."""
        uid = C.create_string_buffer(bytes(unique_id), 128)
        self._ck(self._lib.plda_comm_init(self._h, int(nranks), int(rank), uid))

    def comm_init_host(self, nranks, rank, table):
        """Collectives over a HOST transport: `table` is a _native.HostCollectives (two callbacks on host buffers,
        e.g. plda_amd.sharding.TorchHostTransport over gloo); the library stages device data through a pinned
        bounce buffer.  The callbacks must stay alive as long as the communicator: they are kept on this object."""
        self._comm_table = table
        self._ck(self._lib.plda_comm_init_host(self._h, int(nranks), int(rank), C.byref(table)))

    def comm_init_peer(self, nranks, rank, table):
        """Direct-write collectives over HIP IPC (plda_comm_init_peer); `table`: a HostCollectives used for the handles
        and the rendezvous only.  It must outlive the communicator."""
        self._ck(self._lib.plda_comm_init_peer(self._h, int(nranks), int(rank), C.byref(table)))

    def comm_init_custom(self, nranks, rank, table):
        """Collectives through a caller-supplied device-level table (_native.Collectives)."""
        self._comm_table = table
        self._ck(self._lib.plda_comm_init_custom(self._h, int(nranks), int(rank), C.byref(table)))

    def comm_destroy(self):
        self._ck(self._lib.plda_comm_destroy(self._h))
        self._comm_table = None

    def comm_emulate(self, nranks, rank):
        self._ck(self._lib.plda_comm_emulate(self._h, int(nranks), int(rank)))

    def comm_info(self):
        a, b = C.c_int32(), C.c_int32()
        self._ck(self._lib.plda_comm_info(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def comm_describe(self):
        """dict(transport, nranks, rank, device, pci_bus_id, rccl_version) as the transport itself reports it
        (RCCL: ncclCommCount / ncclCommUserRank / ncclCommCuDevice)."""
        import json
        buf = C.create_string_buffer(512)
        self._ck(self._lib.plda_comm_describe(self._h, buf, len(buf)))
        return json.loads(buf.value.decode())

    @staticmethod
    def shard_plan(m, nranks, rank, block_rows=4096):
        """This rank's blocks [(first row, stop row), ...] of the row partition of the trials matrix
        (plda_shard_plan: a pure function of the library, no GPU needed) -- their order is also the order of
        the rows in the rank's compact slab."""
        lib = N.load()
        nb, rows = C.c_int64(), C.c_int64()
        rc = lib.plda_shard_plan(int(m), int(nranks), int(rank), int(block_rows), None, None, 0, C.byref(nb), C.byref(rows))
        if rc != N.PLDA_OK:
            raise N.PldaError(rc, "plda_shard_plan: bad argument")
        st, ct = np.zeros(max(nb.value, 1), np.int64), np.zeros(max(nb.value, 1), np.int64)
        rc = lib.plda_shard_plan(int(m), int(nranks), int(rank), int(block_rows), _ptr(st), _ptr(ct), nb.value,
                                 C.byref(nb), C.byref(rows))
        if rc != N.PLDA_OK:
            raise N.PldaError(rc, "plda_shard_plan failed")
        return [(int(a), int(a + c)) for a, c in zip(st[:nb.value], ct[:nb.value])]

    def score_matrix_sharded_dev(self, dU, dn, n_uniform, m, dV, nt, dout, ld, block_rows=4096, gather=False,
                                 dzmean=None, dzstd=None):
        """Row-sharded trials matrix on replicated HBM-resident inputs: this rank's blocks (block b -> rank
        b mod R) written in place into the full [M, ld] matrix; gather=True assembles it on every rank."""
        self._ck(self._lib.plda_score_matrix_sharded_dev(
            self._h, C.c_void_p(int(dU)), C.c_void_p(int(dn)) if dn else None, int(n_uniform), int(m),
            C.c_void_p(int(dV)), int(nt), C.c_void_p(int(dzmean)) if dzmean else None,
            C.c_void_p(int(dzstd)) if dzstd else None, C.c_void_p(int(dout)), int(ld), int(block_rows),
            1 if gather else 0))

    def score_matrix_sharded_local_dev(self, dU, dn, n_uniform, m, dV, nt, dlocal, ld_local, block_rows=4096,
                                       dfull=None, ld_full=0, dzmean=None, dzstd=None):
        """The same partition with COMPACT output: this rank's blocks back to back in dlocal[local_rows, ld_local]
        (row map: shard_plan); dfull, if given, additionally receives the assembled [M, ld_full] matrix."""
        self._ck(self._lib.plda_score_matrix_sharded_local_dev(
            self._h, C.c_void_p(int(dU)), C.c_void_p(int(dn)) if dn else None, int(n_uniform), int(m),
            C.c_void_p(int(dV)), int(nt), C.c_void_p(int(dzmean)) if dzmean else None,
            C.c_void_p(int(dzstd)) if dzstd else None, C.c_void_p(int(dlocal)), int(ld_local), int(block_rows),
            C.c_void_p(int(dfull)) if dfull else None, int(ld_full)))

    def eer_matrix_comm_dev(self, dscores, ld, m, nt, denrol_spk, dtest_spk):
        """EER of a row-sharded trials matrix (this rank's slab [m, ld] with the speaker ids of ITS rows, all test
        speaker ids), the histogram counters summed over the ranks through the handle's collectives.  Returns
        the 6-vector (threshold, FAR, FRR, EER, #targets, #impostors), identical on every rank."""
        out = np.zeros(6)
        self._ck(self._lib.plda_eer_matrix_comm_dev(self._h, C.c_void_p(int(dscores)) if dscores else None, int(ld), int(m),
                                                    int(nt), C.c_void_p(int(denrol_spk)) if denrol_spk else None,
                                                    C.c_void_p(int(dtest_spk)), _ptr(out)))
        return out

    def znorm_stats_sharded_dev(self, dbkg, nb, num_examples, d, dmodels, m, dmean, dstd):
        self._ck(self._lib.plda_znorm_stats_sharded_dev(self._h, C.c_void_p(int(dbkg)), int(nb), int(num_examples), int(d),
                                                        C.c_void_p(int(dmodels)), int(m), C.c_void_p(int(dmean)),
                                                        C.c_void_p(int(dstd))))

    def cohort_stats_sharded_dev(self, dX, dn, n_uniform, r, dC, nc, top_k, dmean, dstd):
        self._ck(self._lib.plda_cohort_stats_sharded_dev(
            self._h, C.c_void_p(int(dX)), C.c_void_p(int(dn)) if dn else None, int(n_uniform), int(r), C.c_void_p(int(dC)),
            int(nc), int(top_k), C.c_void_p(int(dmean)), C.c_void_p(int(dstd))))

    def fit_sharded_dev(self, dX, n, d, dlabels, k, iters=10):
        """Fit with the statistics pass over THIS rank's speakers (local dense labels 0..k-1)."""
        self._dout = None
        rc = self._lib.plda_fit_sharded_dev(self._h, C.c_void_p(int(dX)), int(n), int(d), C.c_void_p(int(dlabels)),
                                            int(k), int(iters))
        if rc == N.PLDA_E_ONE_SPEAKER:
            raise ValueError(_ERR_ONE_SPK)
        self._ck(rc)

    def znorm_stats_dev(self, dbkg, nb, num_examples, d, dmodels, m, dmean, dstd):
        self._ck(self._lib.plda_znorm_stats_dev(self._h, C.c_void_p(int(dbkg)), int(nb), int(num_examples), int(d),
                                                C.c_void_p(int(dmodels)), int(m), C.c_void_p(int(dmean)),
                                                C.c_void_p(int(dstd))))
