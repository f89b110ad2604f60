"""tests/history_cases.py -- the probe registry of the handle-history tests.

The law (include/plda_hip.h, "a long-lived handle"): after ANY sequence of earlier successful or refused calls on a handle, a
call's outputs equal, bit for bit, the outputs of the same call on a fresh handle that holds the same model.

    PROBES[name]            a Probe: a named pure function `probe(eng) -> {key: ndarray}`.  Its inputs are built from a seed
                            fixed by its name (and the dimensions of the handle's model where it reads one); every probe ASSERTS
                            the dispatch or padding class it landed in (plan functions, plda_score_last_shape / _kernel,
                            plda_linalg_last_kernels), so that "large then small" cannot quietly become one path twice.  The
                            dispatch record is also part of the outputs: history must not change the kernel either.
    FAMILIES[family]        {"large": name, "small": name[, "third": name]}: small is strictly smaller in every dimension and,
                            where the family has classes, in another class; third is small's class at another size
    MODELS[key]             (din, dout, seed) of the synthetic models the families install (Probe.home names one; None: the
                            probe needs no PLDA model)
    BUFFERS[member]         every plda::DevBuf of plda_handle (plda_amd/csrc/common.hpp) -> the probes that use it, the largest
                            use first, or one line saying why no probe on one GPU can reach it
    ROUTES, REFUSALS        the ways a model is replaced, and the documented refusals that come AFTER device work began
    same_bits / Harness     the comparison (np.array_equal on the uint8 views, as test_gpu_scratch_poison._twice) and the
                            sequence runner of tests/test_gpu_handle_history.py; tests/test_history_cases.py runs the same
                            harness against fake engines written in Python, to show that it can fail

Imports on the CPU: NumPy only at import time; torch and the library are imported inside the probes.
"""
import ctypes as C
import zlib

import numpy as np

E_INVAL, E_NUMERIC, E_NOT_FITTED, E_CAPACITY = -1, -3, -4, -7


def seed_of(name):
    return zlib.crc32(name.encode())


def rng_of(name, *more):
    return np.random.default_rng([seed_of(name)] + [int(v) for v in more])


def _c(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _text(s):
    return np.frombuffer(s.encode(), np.uint8).copy()


# =========================================================================================== models
MODELS = {"A200": (200, 200, 11), "B33": (33, 33, 12), "C7": (7, 7, 13), "D104": (104, 104, 14), "E16": (16, 16, 15),
          "L300": (300, 300, 16), "T150": (200, 150, 17), "F104": (104, 104, 18), "G94": (94, 94, 19)}


def model(key):
    """(mean [din], transform [dout, din], psi [dout]) of MODELS[key]: an orthogonal matrix with scaled rows (the model of
    tests/test_gpu_scratch_poison.py::_model), cut to its leading dout rows."""
    din, dout, seed = MODELS[key]
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((din, din)))
    t = q * (0.5 + rng.random(din))[:, None]
    psi = np.sort(rng.random(din) * 3.0 + 0.05)[::-1].copy()
    return rng.random(din), np.ascontiguousarray(t[:dout]), np.ascontiguousarray(psi[:dout])


# =========================================================================================== the registry
class Probe(object):
    def __init__(self, name, module, build, run, home=None, switches=None):
        self.name, self.module, self.home = name, module, home
        self.switches = dict(switches or {})       # creation-time switches the probe's handle must be made under
        self._build, self._run, self._inputs = build, run, {}

    def inputs(self, din=0, dout=0, cached=True):
        """the probe's host inputs: a function of (name, din, dout) alone"""
        key = (int(din), int(dout))
        if not cached:
            return self._build(rng_of(self.name, *key), *key)
        if key not in self._inputs:
            self._inputs[key] = self._build(rng_of(self.name, *key), *key)
        return self._inputs[key]

    def dims(self, eng):
        if self.home is None:
            return 0, 0
        dout, din = eng.dims()
        return din, dout

    def __call__(self, eng):
        out = self._run(eng, self.inputs(*self.dims(eng)))
        return {k: np.ascontiguousarray(np.asarray(v)).copy() for k, v in out.items()}


PROBES = {}
FAMILIES = {}


def _add(name, module, build, run, home=None, switches=None):
    assert name not in PROBES, name
    PROBES[name] = Probe(name, module, build, run, home, switches)
    return name


def _family(family, large, small, third=None):
    FAMILIES[family] = {"large": large, "small": small}
    if third is not None:
        FAMILIES[family]["third"] = third


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _sync():
    import torch
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- the trials GEMM (score.hip)
BF16X3 = {"PLDA_SCORE_DTYPE": "bf16x3"}      # the contraction as three bf16 terms (s_A16, s_B16)
BT4 = {"PLDA_GEMM_VARIANT": "40"}            # the one-wave-per-SIMD kernel wherever its guards hold (GEMM depth >= 72)


def switches_of(eng):
    return dict(getattr(eng, "history_switches", ()))


def expected_gemm_kernel(eng, kq8):
    """the trials-GEMM kernel a handle runs at these probes' shapes (fewer than 512 tiles of 256 x 256: the 128 x 128 kernel by
    shape): PLDA_SCORE_DTYPE=bf16x3 goes in front of every arm; arm 40 takes the one-wave-per-SIMD kernel from three stages of
    four 8-k steps on, i.e. a packed depth of at least 72 (score.hip: choose_gemm_kernel)"""
    sw = switches_of(eng)
    if sw.get("PLDA_SCORE_DTYPE") == "bf16x3":
        return "trials_gemm_bf16x3_kernel"
    if sw.get("PLDA_GEMM_VARIANT") == "40" and kq8 >= 72:
        return "trials_gemm_bt4_kernel"
    return "trials_gemm_kernel"


def packed_depth(kind, dout):
    """the packed GEMM depth: the algorithmic depth's model part rounded up to 8 (at least 16), the bucket columns to 8"""
    dp = max(16, (dout + 7) // 8 * 8)
    return {"u1": dp, "u7": dp, "bucketed": dp + 8, "deep": 2 * dp}[kind]
COUNT_KINDS = ("u1", "u7", "bucketed", "deep")


def score_counts(rng, kind, m):
    """uniform n = 1 / n = 7, bucketed counts 1..5 (all five present), a count above 4095 (the depth-2D form)"""
    if kind == "u1":
        return 1
    if kind == "u7":
        return 7
    if kind == "bucketed":
        n = rng.integers(1, 6, m).astype(np.int32)
        n[:5] = np.arange(1, 6)
        return n
    n = rng.choice(np.array([1, 3, 5000], np.int32), m).astype(np.int32)
    n[0], n[1] = 5000, 3
    return n


def score_depth(kind, dout):
    return {"u1": dout, "u7": dout, "bucketed": dout + 5 - 1, "deep": 2 * dout}[kind]


def score_matrix(eng, U, n, V, zm=None, zs=None):
    m, nt = U.shape[0], V.shape[0]
    out = np.empty((m, nt), np.float32)
    uniform = int(n) if np.ndim(n) == 0 else 0
    eng._ck(eng._lib.plda_score_matrix(eng._h, _c(U), None if uniform else _c(n), uniform, m, _c(V), nt, _c(zm), _c(zs), _c(out), nt))
    return out


def _score_probe(name, home, m, nt):
    def build(rng, din, dout):
        inp = dict(U=rng.standard_normal((m, dout)), V=rng.standard_normal((nt, dout)), zm=rng.standard_normal(m) * 3.0,
                   zs=rng.random(m) * 2.0 + 0.5)
        for kind in COUNT_KINDS:
            inp["n_" + kind] = score_counts(rng, kind, m)
        return inp

    def run(eng, inp):
        dout = inp["U"].shape[1]
        out = {}
        for kind in COUNT_KINDS:
            for z in (False, True):
                key = "%s%s" % (kind, "_z" if z else "")
                out[key] = score_matrix(eng, inp["U"], inp["n_" + kind], inp["V"], inp["zm"] if z else None, inp["zs"] if z else None)
                shape, kernel = eng.score_last_shape(), eng.score_last_kernel()
                assert shape == (m, nt, score_depth(kind, dout)), (name, key, shape)
                if packed_depth(kind, dout) >= 72 or not switches_of(eng).get("PLDA_GEMM_VARIANT"):
                    assert kernel == expected_gemm_kernel(eng, packed_depth(kind, dout)), (name, key, kernel)
                out[key + "_kernel"] = _text(kernel)
        return out

    return _add(name, "score", build, run, home)


_family("score", _score_probe("score.large", "A200", 300, 517), _score_probe("score.small", "B33", 129, 257),
        _score_probe("score.third", "C7", 65, 64))


def _bt4_probe(name, grids):
    """The one-wave-per-SIMD kernel under PLDA_GEMM_VARIANT=40 at D = 94 over `grids` = [(M, Nt)]: every (ceil(M / 256), ceil(Nt /
    256)) is a tile grid of its own with its own table in the handle's six-entry cache (score.hip: bt4_schedule), matrices that
    end inside a tile go through the fringe scratch, and the queue counters must be back at zero after every launch.  The
    first grid is scored again at the end: with more than six grids its table was evicted and is rebuilt."""
    def build(rng, din, dout):
        m, nt = max(g[0] for g in grids), max(g[1] for g in grids)
        return dict(U=rng.standard_normal((m, dout)), V=rng.standard_normal((nt, dout)), n_bucketed=score_counts(rng, "bucketed", m),
                    zm=rng.standard_normal(m), zs=rng.random(m) + 0.5)

    def run(eng, inp):
        import torch
        assert len({((m + 255) // 256, (nt + 255) // 256) for m, nt in grids}) == len(grids), name
        dU, dV, dn, dzm, dzs = (_dev(inp[k]) for k in ("U", "V", "n_bucketed", "zm", "zs"))
        out = {}
        for i, (m, nt) in enumerate(list(grids) + [grids[0]]):
            mixed = i % 2 == 1
            S = torch.empty((m, nt), dtype=torch.float32, device=dU.device)
            _sync()
            eng.score_matrix_dev(dU.data_ptr(), dn.data_ptr() if mixed else None, 0 if mixed else 2, m, dV.data_ptr(), nt, S.data_ptr(), nt,
                                 dzm.data_ptr() if i % 3 == 2 else None, dzs.data_ptr() if i % 3 == 2 else None)
            eng.synchronize()
            assert eng.score_last_kernel() == "trials_gemm_bt4_kernel", (name, i, eng.score_last_kernel())
            out["S%d" % i] = S.cpu().numpy()
        return out

    return _add(name, "bt4", build, run, "G94", BT4)


_family("bt4", _bt4_probe("bt4.large", [(700, 1299), (300, 517), (1000, 800), (300, 1299), (1000, 517), (700, 800), (300, 800), (1000, 1299)]),
        _bt4_probe("bt4.small", [(290, 500), (600, 257)]))


def _score_dev(eng, d, kind, z=False, prepared=None):
    """score_matrix_dev on device copies of the operands d (a dict of torch tensors) -> the fp32 matrix on the host"""
    import torch
    m, nt = d["U"].shape[0], d["V"].shape[0]
    S = torch.empty((m, nt), dtype=torch.float32, device=d["U"].device)
    n = d["n_" + kind]
    _sync()
    eng.score_matrix_dev(d["U"].data_ptr(), None if isinstance(n, int) else n.data_ptr(), n if isinstance(n, int) else 0, m,
                         d["V"].data_ptr(), nt, S.data_ptr(), nt, d["zm"].data_ptr() if z else None, d["zs"].data_ptr() if z else None)
    eng.synchronize()
    return S.cpu().numpy()


def _prepared_probe(name, home, m, nt, keep):
    """The prepared test side in both forms (plda_score_prepare_dev: uniform and depth-2D; plda_score_prepare_counts_dev: the
    bucketed form), each scored twice (the second call reuses the packed side).  keep: the handle is left prepared, with a
    pointer the caching allocator hands to whoever asks next -- the cache is keyed on the pointer, the model epoch and a
    content fingerprint."""
    def build(rng, din, dout):
        inp = dict(U=rng.standard_normal((m, dout)), V=rng.standard_normal((nt, dout)), zm=rng.standard_normal(m), zs=rng.random(m) + 0.5)
        for kind in COUNT_KINDS:
            inp["n_" + kind] = score_counts(rng, kind, m)
        return inp

    def run(eng, inp):
        dout = inp["U"].shape[1]
        d = {k: (v if np.ndim(v) == 0 else _dev(v)) for k, v in inp.items()}
        out = {}
        for kind, prepare in (("u7", lambda: eng.score_prepare_dev(d["V"].data_ptr(), nt, False, 7)),
                              ("bucketed", lambda: eng.score_prepare_counts_dev(d["V"].data_ptr(), nt, inp["n_bucketed"])),
                              ("deep", lambda: eng.score_prepare_dev(d["V"].data_ptr(), nt, True))):
            _sync()
            prepare()
            for again in (0, 1):
                out["%s_%d" % (kind, again)] = _score_dev(eng, d, kind, z=bool(again))
                assert eng.score_last_shape() == (m, nt, score_depth(kind, dout)), (name, kind, eng.score_last_shape())
        if not keep:
            eng.score_unprepare()
        out["plain"] = _score_dev(eng, d, "u1")
        return out

    return _add(name, "prepared", build, run, home)


_family("prepared", _prepared_probe("prepared.large", "A200", 300, 517, True), _prepared_probe("prepared.small", "B33", 129, 257, True),
        _prepared_probe("prepared.third", "C7", 65, 64, False))


# ------------------------------------------------------------------------------------------- trial lists and the one-trial score
PAIRS_TAB_MIN = 16384          # score.hip: from this many trials on the list runs on per-count tables (pair_tab)


def score_pairs(eng, U, n, V, e, t, zm=None, zs=None):
    out = np.zeros(e.shape[0])
    eng._ck(eng._lib.plda_score_pairs(eng._h, _c(U), _c(n), U.shape[0], _c(V), V.shape[0], _c(e), _c(t), e.shape[0], _c(zm), _c(zs), _c(out)))
    return out


def _pairs_probe(name, home, m, nt, p):
    def build(rng, din, dout):
        return dict(U=rng.standard_normal((m, dout)), V=rng.standard_normal((nt, dout)), n=rng.integers(1, 5, m).astype(np.int32),
                    e=rng.integers(0, m, p), t=rng.integers(0, nt, p), zm=rng.standard_normal(m), zs=rng.random(m) + 0.5)

    def run(eng, inp):
        args = (eng, inp["U"], inp["n"], inp["V"], inp["e"], inp["t"])
        return dict(raw=score_pairs(*args), z=score_pairs(*args, inp["zm"], inp["zs"]))

    return _add(name, "pairs", build, run, home)


_family("pairs", _pairs_probe("pairs.long", "A200", 57, 91, PAIRS_TAB_MIN + 3), _pairs_probe("pairs.short", "B33", 23, 40, PAIRS_TAB_MIN - 1),
        _pairs_probe("pairs.third", "C7", 9, 17, 501))


def _one_probe(name, home):
    def build(rng, din, dout):
        return dict(u=rng.standard_normal(dout), v=rng.standard_normal(dout))

    def run(eng, inp):
        out = {}
        for n in (1, 7, 1):                       # (the host cache is per count: 1, then 7, then 1 again)
            for z in (0, 1):
                s = C.c_double()
                eng._ck(eng._lib.plda_score_one(eng._h, _c(inp["u"]), n, _c(inp["v"]), z, 0.25, 1.5, C.byref(s)))
                out["n%d_z%d" % (n, z)] = np.array([s.value])
        eng._dout = None
        out["device"] = np.array([eng.score_on_device(3, (2, inp["u"]), (1, inp["v"]))])
        return out

    return _add(name, "one", build, run, home)


_family("one", _one_probe("one.large", "A200"), _one_probe("one.small", "B33"), _one_probe("one.third", "C7"))


# ------------------------------------------------------------------------------------------- K4, project_rows, the grouped transform, norm
def transform_class(dout):
    """the dimension class of the one-pass K4 kernel: Dout <= 128 / 208 / 256 / 384 / 512 (include/plda_hip.h: plda_transform_plan)"""
    return sum(dout > edge for edge in (128, 208, 256, 384))


def _transform_probe(name, home, r):
    def build(rng, din, dout):
        return dict(x=rng.standard_normal((r, din)) + 0.3, n=rng.integers(1, 9, r).astype(np.int32))

    def run(eng, inp):
        plan = eng.transform_plan(r)
        assert plan["arm"] == "fused" and plan["cls"] == transform_class(eng.dims()[0]), (name, plan)
        return dict(u=eng.transform_array(inp["x"], 3), m=eng.transform_array(inp["x"], inp["n"]), p=eng._project(inp["x"]),
                    plan=np.array([plan["cls"], plan["main_block"], plan["tail_block"], plan["main_rows"], plan["tail_rows"]]))

    return _add(name, "transform", build, run, home)


_family("transform", _transform_probe("transform.large", "A200", 1029), _transform_probe("transform.small", "B33", 129),
        _transform_probe("transform.third", "C7", 17))
_transform_probe("transform.truncated", "T150", 257)
_transform_probe("transform.L300", "L300", 300)


def _groups_probe(name, home, r, k, nb, nm):
    """transform_groups (the grouping of fit.hip, the centroids, K4) and norm() (the z-norm statistics by moments)"""
    def build(rng, din, dout):
        return dict(x=rng.random((r, din)), y=rng.integers(0, k, r).astype(np.uint64), bkg=rng.random((nb, din)),
                    models=rng.standard_normal((nm, dout)))

    def run(eng, inp):
        eng._dout = None
        tr = eng.transform(inp["x"], inp["y"])
        keys = sorted(tr)
        eng._meanz, eng._stdvz, eng._zn_tag = {}, {}, None
        eng.norm(inp["bkg"], {i: (1, inp["models"][i]) for i in range(nm)})
        zm, zs = eng.znorm_stats()
        eng._meanz, eng._stdvz, eng._zn_tag = {}, {}, None
        return dict(tv=np.stack([tr[i][1] for i in keys]), tc=np.array([tr[i][0] for i in keys]), keys=np.array(keys),
                    zm=np.array([zm[i] for i in range(nm)]), zs=np.array([zs[i] for i in range(nm)]))

    return _add(name, "groups", build, run, home)


_family("groups", _groups_probe("groups.large", "A200", 900, 60, 301, 13), _groups_probe("groups.small", "B33", 120, 9, 40, 5),
        _groups_probe("groups.third", "L300", 400, 30, 120, 7))          # (D > 208: norm's model pass on the general GEMM + row kernel)


# ------------------------------------------------------------------------------------------- the PLDA fit (fit.hip)
def _fit_data(rng, n, d, k, skew):
    if skew:
        y = np.concatenate([np.arange(k), rng.integers(0, k, n - k)]).astype(np.uint64)
    else:
        y = (np.arange(n) % k).astype(np.uint64)
    return rng.random((n, d)) + 0.5 * rng.standard_normal((k, d))[y.astype(np.int64)], y


def _fit_probe(name, n, d, k, skew, form, split=False):
    """A PLDA fit (it REPLACES the handle's model: it is also a model route).  skew: many distinct class counts (the row form
    of the grouped EM), else equal counts (the moment form).  split: plda_fit_stats_dev, then plda_fit_em_dev on the statistics
    read back."""
    def build(rng, din, dout):
        x, y = _fit_data(rng, n, d, k, skew)
        return dict(x=x, y=y)

    def run(eng, inp):
        import torch
        eng._dout = None
        if split:
            dx, dy = _dev(inp["x"]), _dev(inp["y"].view(np.int64))
            dm = torch.empty((k, d), dtype=torch.float64, device=dx.device)
            dc = torch.empty(k, dtype=torch.int64, device=dx.device)
            ds = torch.empty((d, d), dtype=torch.float64, device=dx.device)
            _sync()
            eng.fit_stats_dev(dx.data_ptr(), n, d, dy.data_ptr(), k)
            eng.fit_get_stats_dev(dm.data_ptr(), dc.data_ptr(), ds.data_ptr())
            eng.synchronize()
            eng.fit_em_dev(dm.data_ptr(), dc.data_ptr(), k, ds.data_ptr(), d, 3)
            eng.synchronize()
        else:
            eng.fit(inp["x"], inp["y"], 3)
        plan, it, g = eng.fit_plan(), eng.fit_internals(), eng.get_model()
        assert plan["form"] == form, (name, plan)
        return dict(W=it["W"], B=it["B"], means=it["means"], scatter=it["scatter"], psi=g["psi"], transform=g["transform"], mean=g["mean"],
                    offset=g["offset"], plan=np.array([plan["groups"]]))

    return _add(name, "fit", build, run)


_family("fit", _fit_probe("fit.large", 700, 209, 41, True, "rows"), _fit_probe("fit.small", 240, 33, 12, False, "moments"),
        _fit_probe("fit.third", 120, 17, 8, False, "moments"))
_fit_probe("fit.split", 300, 48, 20, True, "rows", split=True)


# ------------------------------------------------------------------------------------------- LDA (lda.hip)
def _lda_probe(name, n, d, k):
    def build(rng, din, dout):
        x, y = _fit_data(rng, n, d, k, True)
        return dict(x=x, y=y)

    def run(eng, inp):
        from plda_amd.lda import LDA
        out = {}
        for solver in ("svd", "eigen", "lsqr"):
            lda = LDA(solver, engine=eng)
            lda.fit(inp["x"], inp["y"])
            out[solver + "_lp"] = lda.predict_log_proba(inp["x"][:67])
            if solver != "lsqr":
                out[solver + "_tr"] = lda.transform(inp["x"][:67])
        return out

    return _add(name, "lda", build, run)


_family("lda", _lda_probe("lda.large", 900, 120, 23), _lda_probe("lda.small", 150, 9, 5))


# ------------------------------------------------------------------------------------------- the embedding chain (embed.hip)
def _embed_plan(eng, din, dout, has_a, dtype):
    out = np.zeros(3, np.int32)
    eng._ck(eng._lib.plda_embed_plan(eng._h, din, dout, int(has_a), dtype, _c(out)))
    return int(out[0])


def _embed_apply_probe(name, din, dout, r, has_a, cls):
    """embed_set + embed_apply + embed_clear: class 0 (no matrix), 1 (the fused kernel, Dout <= 512), 2 (row pass + GEMM + row pass)"""
    def build(rng, _din, _dout):
        inp = dict(m_in=rng.standard_normal(din), x64=rng.standard_normal((r, din)), x32=rng.standard_normal((r, din)).astype(np.float32))
        if has_a:
            inp.update(A=rng.standard_normal((dout, din)) / np.sqrt(din), m_out=rng.standard_normal(dout) * 0.1)
        return inp

    def run(eng, inp):
        from plda_amd.embed import EmbeddingChain
        ch = EmbeddingChain(inp["m_in"], 1.0, inp.get("A"), inp.get("m_out"), float(np.sqrt(dout)), dim=din)
        eng.set_embedding(ch)
        try:
            assert _embed_plan(eng, din, dout if has_a else din, has_a, 0) == cls, name
            return dict(f64=eng.embed(inp["x64"]), f32=eng.embed(inp["x32"]), one=eng.embed(inp["x64"][:1]))
        finally:
            eng.set_embedding(None)

    return _add(name, "embed", build, run)


_family("embed", _embed_apply_probe("embed.large", 520, 513, 129, True, 2), _embed_apply_probe("embed.small", 65, 64, 33, True, 1),
        _embed_apply_probe("embed.third", 17, 17, 5, True, 1))
_embed_apply_probe("embed.centre", 200, 200, 65, False, 0)


def _embed_fit_probe(name, n, d, k, dim):
    def build(rng, _din, _dout):
        x, y = _fit_data(rng, n, d, k, True)
        return dict(x=x, y=y, x32=x.astype(np.float32))

    def run(eng, inp):
        out = {}
        try:
            for kind, x in (("lda", inp["x"]), ("whiten", inp["x32"]), ("centre", inp["x"])):
                ch = eng.fit_embedding(x, inp["y"] if kind == "lda" else None, kind, None if kind == "centre" else dim, 1.0)
                out[kind + "_m_in"] = ch.m_in
                if ch.A is not None:
                    out[kind + "_A"], out[kind + "_eig"] = ch.A, ch.eig
                if ch.m_out is not None:
                    out[kind + "_m_out"] = ch.m_out
                out[kind + "_rows"] = eng.embed(inp["x"][:9])
        finally:
            eng.set_embedding(None)
        return out

    return _add(name, "embed_fit", build, run)


_family("embed_fit", _embed_fit_probe("embed_fit.large", 600, 130, 21, 64), _embed_fit_probe("embed_fit.small", 90, 9, 5, 4))


# ------------------------------------------------------------------------------------------- VBx (vbx.hip)
VBX_LDS_DOUBLES = 19456


def _vbx_probe(name, shapes, d, classes, second=False):
    """diarize.vbx on given Phi (the handle only has to hold SOME model), posteriors included; second: plda_vbx_top2"""
    def build(rng, din, dout):
        import vbx_model as M
        recs = [M.generate(t, d, max(1, min(4, s)), s, int(rng.integers(1 << 30)))[:2] for t, s in shapes]
        return dict(y=np.concatenate([r[0] for r in recs]), labels=np.concatenate([r[1] for r in recs]),
                    phi=30.0 * np.exp(-4.0 * np.arange(d) / d))

    def run(eng, inp):
        from plda_amd import diarize
        got = [diarize.vbx_plan(eng, t, s, d)["cls"] for t, s in shapes]
        assert got == list(classes), (name, got)
        off = diarize.offsets_of([t for t, _ in shapes])
        res = diarize.vbx(eng, inp["y"], off, inp["labels"], inp["phi"], max_iters=8, epsilon=-np.inf, return_posteriors=True,
                          return_second=second)
        info = res[-1]
        out = dict(labels=res[0], ncl=res[1], elbo=info["elbo"], iters=info["iters"], gamma=np.concatenate([g.ravel() for g in info["gamma"]]),
                   pi=np.concatenate(info["pi"]))
        if second:
            out.update(labels2=res[2], post2=res[3])
        return out

    return _add(name, "vbx", build, run, "E16")


_family("vbx", _vbx_probe("vbx.large", [(130, 64), (65, 8)], 33, (1, 0)), _vbx_probe("vbx.small", [(64, 8)], 16, (0,)),
        _vbx_probe("vbx.third", [(9, 3), (5, 2)], 7, (0, 0)))
_family("vbx2", _vbx_probe("vbx2.large", [(130, 64), (65, 8)], 33, (1, 0), True), _vbx_probe("vbx2.small", [(64, 8)], 16, (0,), True))


# ------------------------------------------------------------------------------------------- AHC (ahc.hip)
def ahc_lds_max():
    n = 1
    while 8 * (n + 1) * n // 2 + 28 * (n + 1) + 512 <= 160 * 1024:
        n += 1
    return n


def _ahc_probe(name, sizes, classes):
    def build(rng, din, dout):
        import ahc_model
        return {"b%d" % i: ahc_model.gaussian(n, int(rng.integers(1 << 30))) for i, n in enumerate(sizes)}

    def run(eng, inp):
        from plda_amd import diarize
        got = [diarize.plan(eng, n)["cls"] for n in sizes]
        assert got == list(classes) and diarize.plan(eng, 1)["lds_max"] == ahc_lds_max(), (name, got)
        lab, ncl, mer = diarize.ahc(eng, [inp["b%d" % i] for i in range(len(sizes))], None, 1, True)
        lab2, ncl2 = diarize.ahc(eng, [inp["b%d" % i] for i in range(len(sizes))], 0.0, 2)
        return dict(lab=lab, ncl=ncl, ma=mer[0], mb=mer[1], mc=mer[2], lab2=lab2, ncl2=ncl2)

    return _add(name, "ahc", build, run)


_family("ahc", _ahc_probe("ahc.large", [ahc_lds_max() + 1, 65], (1, 0)), _ahc_probe("ahc.small", [64, 3], (0, 0)),
        _ahc_probe("ahc.third", [5], (0,)))


def _ahc_operand_probe(name, home, sizes):
    """plda_score_ahc: the blocks scored into the slab (sn_slab), clustered and dropped"""
    def build(rng, din, dout):
        spk = rng.standard_normal((6, dout)) * 1.5
        return dict(v=np.concatenate([spk[rng.integers(0, 6, n)] + rng.standard_normal((n, dout)) for n in sizes]))

    def run(eng, inp):
        from plda_amd import diarize
        lab, ncl, mer = diarize.ahc_vectors(eng, inp["v"], diarize.offsets_of(sizes), None, 1, True)
        return dict(lab=lab, ncl=ncl, ma=mer[0], mb=mer[1], mc=mer[2])

    return _add(name, "ahc", build, run, home)


_family("ahc_operand", _ahc_operand_probe("ahc_operand.large", "A200", [ahc_lds_max() + 1, 40]), _ahc_operand_probe("ahc_operand.small", "B33", [33, 7]))


# ------------------------------------------------------------------------------------------- dense PCA scoring (dense_pca.hip)
DENSE_PCA_LDS_MAX = 100        # dense_pca.hip: 16 m^2 + 20 ceil(m / 2) + 76 bytes of LDS <= 160 KiB


def dense_pca_case(x, offsets, target):
    """the case of test_gpu_dense_pca.py::test_poisoned_scratch_is_bit_identical: the blocks with their dimensions and
    eigenvalues, then the clustering form's five outputs"""
    def case(eng):
        from plda_amd import diarize
        blocks, info = diarize.score_dense_pca(eng, x, offsets, target, return_info=True)
        lab, ncl, mer = diarize.ahc_dense_pca(eng, x, offsets, target, None, 1, True)
        return dict(blocks=np.concatenate([b.ravel() for b in blocks]), dims=info["dims"], eig=np.concatenate(info["eigenvalues"]), lab=lab,
                    ncl=ncl, ma=mer[0], mb=mer[1], mc=mer[2])
    return case


def _dense_probe(name, home, sizes):
    def build(rng, din, dout):
        import dense_pca_model as dm
        return dict(x=np.concatenate([dm.planted_rows(rng, n, din) for n in sizes]))

    def run(eng, inp):
        from plda_amd import diarize
        dout, din = eng.dims()
        got = [diarize.dense_pca_plan(eng, n, din)["cls"] for n in sizes]
        assert got == [int(min(n, din) > DENSE_PCA_LDS_MAX) for n in sizes], (name, got)
        return dense_pca_case(inp["x"], diarize.offsets_of(sizes), 0.5)(eng)

    return _add(name, "dense_pca", build, run, home)


_family("dense_pca", _dense_probe("dense_pca.large", "A200", [130, 40, 9]), _dense_probe("dense_pca.small", "B33", [20, 3]),
        _dense_probe("dense_pca.third", "D104", [101, 5]))      # classes under their home models: (1, 0, 0), (0, 0), (1, 0)


# ------------------------------------------------------------------------------------------- DER (der.hip, der_time.hip)
def der_lds_max(sr):
    fixed = 8 * (4 + 16 + 1 + 65 + 64) + 4 * (64 + 64 + 4)
    w = 1
    while w < 4096 and 8 * sr * (w + 1) + 32 * (w + 2) + fixed <= 160 * 1024:
        w += 1
    return w


def _distinct(rng, n, count, limit):
    vals = np.sort(rng.choice(limit, count, replace=False))
    lab = np.concatenate([np.arange(count), rng.integers(0, count, n - count)])
    rng.shuffle(lab)
    return vals[lab].astype(np.int32)


def _der_probe(name, shapes, classes):
    """shapes: (n, sr, sh) per recording"""
    def build(rng, din, dout):
        ref = np.concatenate([_distinct(rng, n, sr, 64) for n, sr, _ in shapes])
        hyp = np.concatenate([_distinct(rng, n, sh, 4096) for n, _, sh in shapes])
        return dict(ref=ref, hyp=hyp, dur=rng.integers(0, 1000, len(ref)).astype(np.int32))

    def run(eng, inp):
        from plda_amd import der, diarize
        got = [der.plan(eng, sr, sh)["cls"] for _, sr, sh in shapes]
        assert got == list(classes), (name, got)
        res = der.der(eng, inp["ref"], inp["hyp"], diarize.offsets_of([s[0] for s in shapes]), inp["dur"], return_map=True)
        return dict(counts=res.counts, map=res.map)

    return _add(name, "der", build, run)


_family("der", _der_probe("der.large", [(300, 64, 300), (65, 9, 30)], (1, 0)), _der_probe("der.small", [(64, 5, 9)], (0,)),
        _der_probe("der.third", [(5, 2, 3), (2, 1, 1)], (0, 0)))


def _merges(rng, sizes):
    """a full merge record of drawn blocks from the host model of the clustering (tests/ahc_model.py)"""
    import ahc_model
    blocks = [ahc_model.gaussian(n, int(rng.integers(1 << 30))) for n in sizes]
    full = ahc_model.cluster(blocks, None, 1)
    return full[2], full[3], full[4]


def _der_sweep_probe(name, sizes, q):
    def build(rng, din, dout):
        ma, mb, mc = _merges(rng, sizes)
        t = int(sum(sizes))
        ref = rng.integers(-1, 6, t).astype(np.int32)
        thr = np.sort(-np.asarray(mc)[rng.integers(0, len(mc), q)]) if len(mc) else np.zeros(q)
        return dict(ma=ma, mb=mb, mc=mc, ref=ref, dur=rng.integers(1, 50, t).astype(np.int32), thr=np.asarray(thr, np.float64))

    def run(eng, inp):
        from plda_amd import der, diarize
        res = der.sweep(eng, (inp["ma"], inp["mb"], inp["mc"]), diarize.offsets_of(sizes), inp["ref"], inp["thr"], inp["dur"])
        return dict(counts=res.counts, ncl=res.n_clusters)

    return _add(name, "der", build, run)


_family("der_sweep", _der_sweep_probe("der_sweep.large", [150, 40], 7), _der_sweep_probe("der_sweep.small", [17], 3))


def _timed_recs(rng, shapes, second):
    import der_overlap_model as OV
    import der_time_model as T
    recs = []
    for nt, n, nu in shapes:
        kw = dict(n_spk=8, span=40 * (nt + n) + 100, n_hyp=12, n_uem=nu)
        recs.append(OV.random_recording(rng, n, nt, **kw) if second else T.random_recording(rng, n, nt, **kw))
    return (OV if second else T).pack(recs)


def _timed_probe(name, shapes, collar, classes, second=False, sweep=0):
    """shapes: (turns, segments, UEM intervals) per recording; second: plda_der_timed_ovl; sweep: plda_der_timed_sweep over that
    many thresholds of a drawn merge record"""
    def build(rng, din, dout):
        p = _timed_recs(rng, shapes, second)
        inp = dict(ts=p[0][0], td=p[0][1], tk=p[0][2], toff=p[0][3], ss=p[1], sd=p[2], hyp=p[3], off=p[4])
        if p[5] is not None:
            inp.update(us=p[5][0], ud=p[5][1], uoff=p[5][2])
        if second:
            inp["hyp2"] = p[6]
        if sweep:
            ma, mb, mc = _merges(rng, [s[1] for s in shapes])
            inp.update(ma=ma, mb=mb, mc=mc, thr=np.sort(-np.asarray(mc)[rng.integers(0, len(mc), sweep)]).astype(np.float64))
        return inp

    def run(eng, inp):
        from plda_amd import der
        got = [der.plan_timed(eng, nt, n, nu, collar)["cls"] for nt, n, nu in shapes]
        assert got == list(classes), (name, got)
        turns = (inp["ts"], inp["td"], inp["tk"], inp["toff"])
        uem = (inp["us"], inp["ud"], inp["uoff"]) if "us" in inp else None
        if sweep:
            res = der.sweep_timed(eng, (inp["ma"], inp["mb"], inp["mc"]), turns, inp["ss"], inp["sd"], inp["off"], inp["thr"], None, collar, uem)
            return dict(counts=res.counts, ncl=res.n_clusters)
        res = der.der_timed(eng, turns, inp["ss"], inp["sd"], inp["hyp"], inp["off"], collar, uem, False, True, inp.get("hyp2"))
        return dict(counts=res.counts, map=res.map)

    return _add(name, "der_timed", build, run)


# (6 events a turn under a collar: 2750 turns and 60 segments are 16 620 event slots, above the 16 384 of the LDS class)
_family("der_timed", _timed_probe("der_timed.large", [(2750, 60, 2), (40, 20, 0)], 9, (1, 0)), _timed_probe("der_timed.small", [(30, 12, 0)], 0, (0,)),
        _timed_probe("der_timed.third", [(5, 3, 1)], 2, (0,)))
_family("der_timed_ovl", _timed_probe("der_timed_ovl.large", [(2750, 60, 2), (40, 20, 0)], 9, (1, 0), second=True),
        _timed_probe("der_timed_ovl.small", [(30, 12, 0)], 0, (0,), second=True))
_family("der_timed_sweep", _timed_probe("der_timed_sweep.large", [(2750, 60, 0), (40, 20, 0)], 9, (1, 0), sweep=5),
        _timed_probe("der_timed_sweep.small", [(30, 12, 0)], 0, (0,), sweep=2))


# ------------------------------------------------------------------------------------------- AS-norm and top-N (snorm.hip, topn.hip)
def _asnorm_probe(name, home, r, nc, k, m, nt):
    """the cohort statistics of r rows (both count kinds), then the S-normalised matrix of m x nt trials"""
    def build(rng, din, dout):
        return dict(X=rng.standard_normal((r, dout)), Cv=rng.standard_normal((nc, dout)), n=rng.choice(np.array([2, 5], np.int32), r).astype(np.int32),
                    V=rng.standard_normal((nt, dout)))

    def run(eng, inp):
        eng._dout = None
        mu, sd = eng._cohort_stats(np.full(r, 3, np.int32), inp["X"], inp["Cv"], k)
        mm, sm = eng._cohort_stats(inp["n"], inp["X"], inp["Cv"], nc)
        S = eng.score_matrix_asnorm((inp["n"][:m], inp["X"][:m]), (1, inp["V"]), inp["Cv"], k)
        return dict(mu=mu, sd=sd, mm=mm, sm=sm, S=S)

    return _add(name, "asnorm", build, run, home)


_family("asnorm", _asnorm_probe("asnorm.large", "A200", 130, 4097, 300, 65, 129), _asnorm_probe("asnorm.small", "B33", 3, 65, 5, 3, 17))


def _topn_probe(name, home, m, nt, top):
    def build(rng, din, dout):
        return dict(U=rng.standard_normal((m, dout)), V=rng.standard_normal((nt, dout)), n=rng.choice(np.array([2, 5], np.int32), m).astype(np.int32),
                    Cv=rng.standard_normal((40, dout)), S=rng.standard_normal((m, nt)).astype(np.float32))

    def run(eng, inp):
        import torch
        eng._dout = None
        eng._meanz, eng._stdvz, eng._zn_tag = {}, {}, None
        out = {}
        for per in ("test", "enrol"):
            n = min(top, m if per == "test" else nt)
            s, i = eng.top_n((inp["n"], inp["U"]), (1, inp["V"]), n, per)
            out[per + "_s"], out[per + "_i"] = s, i
            s, i = eng.top_n((inp["n"], inp["U"]), (1, inp["V"]), n, per, cohort=inp["Cv"], top_k=9)
            out[per + "_cs"], out[per + "_ci"] = s, i
        dS = _dev(inp["S"])
        for axis in (0, 1):
            n = min(top, nt if axis == 0 else m)
            lines = m if axis == 0 else nt
            ds = torch.empty((lines, n), dtype=torch.float32, device=dS.device)
            di = torch.empty((lines, n), dtype=torch.int64, device=dS.device)
            _sync()
            eng.topn_matrix_dev(dS.data_ptr(), nt, m, nt, axis, n, ds.data_ptr(), di.data_ptr())
            eng.synchronize()
            out["m%d_s" % axis], out["m%d_i" % axis] = ds.cpu().numpy(), di.cpu().numpy()
        return out

    return _add(name, "topn", build, run, home)


_family("topn", _topn_probe("topn.large", "A200", 257, 1025, 100), _topn_probe("topn.small", "B33", 63, 65, 10))


# ------------------------------------------------------------------------------------------- EER, DET, minDCF, calibration, fusion
def _labelled(rng, m, nt, spk):
    es, ts = rng.integers(0, spk, m), rng.integers(0, spk, nt)
    ts[0], ts[-1] = es[0], spk
    S = (rng.standard_normal((m, nt)) + 2.0 * (es[:, None] == ts[None, :])).astype(np.float32)
    return S, es.astype(np.int64), ts.astype(np.int64)


def _trials_probe(name, home, m, nt, spk):
    """One labelled matrix through every reduction that shares trial_hist -- EER (default: by size), DET, minDCF --, their list
    forms, and the operand forms (slabs of scores in flight: eer_slab, eer_smp)"""
    def build(rng, din, dout):
        S, es, ts = _labelled(rng, m, nt, spk)
        c = rng.standard_normal((spk + 1, dout)) * 1.2
        return dict(S=S, es=es, ts=ts, U=c[es] + rng.standard_normal((m, dout)), V=c[ts] + rng.standard_normal((nt, dout)))

    def run(eng, inp):
        from plda_amd import dcf, eer
        pts = ((0.01, 1.0, 1.0), (0.05, 1.0, 1.0), (0.001, 1.0, 1.0), (0.5, 1.0, 1.0), (0.005, 10.0, 1.0))
        tgt = inp["es"][:, None] == inp["ts"][None, :]
        pos, neg = inp["S"][tgt], inp["S"][~tgt]
        dS, des, dts, dU, dV = (_dev(inp[k]) for k in ("S", "es", "ts", "U", "V"))
        _sync()
        a = (dS.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr())
        o = (dU.data_ptr(), None, 2, m, dV.data_ptr(), nt, des.data_ptr(), dts.data_ptr())
        out = dict(eer=np.asarray(eer.eer_from_matrix_dev(eng, *a), np.float64), eer_l=np.asarray(eer.eer_from_lists(eng, pos, neg), np.float64),
                   eer_o=np.asarray(eer.eer_from_operands_dev(eng, *o), np.float64))
        out["thr"], out["far"], out["frr"] = eer.det_from_matrix_dev(eng, *a, 50)
        for key, (res, info) in (("dcf", dcf.min_dcf_from_matrix_dev(eng, *a, pts)), ("dcf_l", dcf.min_dcf_from_lists(eng, pos, neg, pts)),
                                 ("dcf_o", dcf.min_dcf_from_operands_dev(eng, *o, points=pts))):
            out[key] = _text(repr(res))
        return out

    return _add(name, "trials", build, run, home)


_family("trials", _trials_probe("trials.large", "A200", 257, 2049, 16), _trials_probe("trials.small", "B33", 37, 255, 6),
        _trials_probe("trials.third", "C7", 5, 64, 3))


def _reduction_probe(name, module, home, m, nt, spk):
    """ONE reduction of a labelled matrix -- module "eer", "det", "mindcf" or "calib_pass" -- in its matrix, list and operand
    forms (a DET has no operand form): the four share trial_hist, eer_list and the operand slabs, so each is the other's
    neighbour"""
    def build(rng, din, dout):
        S, es, ts = _labelled(rng, m, nt, spk)
        c = rng.standard_normal((spk + 1, dout)) * 1.2
        return dict(S=S, es=es, ts=ts, U=c[es] + rng.standard_normal((m, dout)), V=c[ts] + rng.standard_normal((nt, dout)),
                    n=rng.integers(1, 4, m).astype(np.int32))

    def run(eng, inp):
        from plda_amd import calibration as CB, dcf, eer
        tgt = inp["es"][:, None] == inp["ts"][None, :]
        pos, neg = inp["S"][tgt], inp["S"][~tgt]
        dS, des, dts, dU, dV, dn = (_dev(inp[k]) for k in ("S", "es", "ts", "U", "V", "n"))
        _sync()
        a = (dS.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr())
        o = (dU.data_ptr(), dn.data_ptr(), 0, m, dV.data_ptr(), nt, des.data_ptr(), dts.data_ptr())
        if module == "eer":
            return dict(m=np.asarray(eer.eer_from_matrix_dev(eng, *a)), l=np.asarray(eer.eer_from_lists(eng, pos, neg)),
                        o=np.asarray(eer.eer_from_operands_dev(eng, *o)))
        if module == "det":
            t1, fa1, fr1 = eer.det_from_matrix_dev(eng, *a, 50)
            t2, fa2, fr2 = eer.det_from_lists(eng, pos, neg, 30)
            return dict(t1=t1, fa1=fa1, fr1=fr1, t2=t2, fa2=fa2, fr2=fr2)
        if module == "mindcf":
            pts = ((0.01, 1.0, 1.0), (0.5, 1.0, 1.0), (0.005, 10.0, 1.0))
            return {k: _text(repr(r[0])) for k, r in (("m", dcf.min_dcf_from_matrix_dev(eng, *a, pts)), ("l", dcf.min_dcf_from_lists(eng, pos, neg, pts)),
                                                      ("o", dcf.min_dcf_from_operands_dev(eng, *o, points=pts)))}
        recs = (CB.pass_from_matrix_dev(eng, *a, 0.7, -0.3, 0.5), CB.pass_from_lists(eng, pos, neg, 0.7, -0.3, 0.5),
                CB.pass_from_operands_dev(eng, *o, None, None, 0.7, -0.3, 0.5))
        return {k: _text(repr(sorted(r.items()))) for k, r in zip("mlo", recs)}

    return _add(name, module, build, run, home)


for _module in ("eer", "det", "mindcf", "calib_pass"):
    _family(_module, _reduction_probe(_module + ".large", _module, "A200", 300, 1025, 16), _reduction_probe(_module + ".small", _module, "B33", 37, 255, 6))


def _calib_probe(name, m, nt, spk, k):
    """the calibration pass and fit (calib_part) and the fusion pass and fit of k systems (fusion_part), list forms"""
    def build(rng, din, dout):
        S, es, ts = _labelled(rng, m, nt, spk)
        inp = dict(S=S, es=es, ts=ts)
        for j in range(1, k):
            inp["S%d" % j] = (S * np.float32(1.0 + 0.5 * j) + rng.standard_normal((m, nt)).astype(np.float32)).astype(np.float32)
        return inp

    def run(eng, inp):
        from plda_amd import calibration as CB, fusion as FU
        tgt = inp["es"][:, None] == inp["ts"][None, :]
        sys_ = [inp["S"]] + [inp["S%d" % j] for j in range(1, k)]
        pos, neg = inp["S"][tgt], inp["S"][~tgt]
        rec = CB.pass_from_lists(eng, pos, neg, 0.7, -0.3, 0.5)
        f = CB.fit_from_lists(eng, pos, neg, 0.5, 1e-18, 100)
        frec = FU.pass_from_lists(eng, [s[tgt] for s in sys_], [s[~tgt] for s in sys_], np.full(k, 1.0 / k), 0.1, 0.2)
        ff = FU.fit_from_lists(eng, [s[tgt] for s in sys_], [s[~tgt] for s in sys_], 0.5, 1e-18, 100)
        return dict(rec=_text(repr(sorted(rec.items()))), fit=np.array([f.a, f.b, f.cllr_after]),
                    frec=_text(repr(sorted((kk, np.asarray(v).tolist()) for kk, v in frec.items()))), ffit=np.concatenate([np.ravel(ff.a), [ff.b, ff.cllr_after]]))

    return _add(name, "calibration", build, run)


_family("calibration", _calib_probe("calibration.large", 129, 1025, 11, 4), _calib_probe("calibration.small", 17, 64, 4, 2))


# ------------------------------------------------------------------------------------------- adaptation (adapt.hip)
def _adapt_probe(name, home, n):
    """the statistics record of n rows (non-destructive: adapt_reset, accumulate in two pieces, read)"""
    def build(rng, din, dout):
        return dict(x=rng.standard_normal((n, din)) * 1.3 + 0.2, w=rng.random(n) + 0.05)

    def run(eng, inp):
        eng.adapt_reset()
        eng.adapt_accumulate(inp["x"][:n // 2], inp["w"][:n // 2])
        eng.adapt_accumulate(inp["x"][n // 2:], inp["w"][n // 2:])
        s = eng.adapt_stats()
        eng.adapt_reset()
        return dict(tw=np.array([s["tot_weight"]]), rows=np.array([s["rows"]]), pilot=s["pilot"], s1=s["s1"], s2=s["s2"])

    return _add(name, "adapt", build, run, home)


def adapt_and_blend_case(model, other, x, w):
    """the case of test_gpu_adapt.py::test_adapt_and_blend_on_poisoned_scratch: the record in two pieces, the update, the blend"""
    def case(eng):
        eng.set_model(*model)
        eng.adapt_accumulate(x[:100], w[:100])
        eng.adapt_accumulate(x[100:], w[100:])
        st = eng.adapt_stats()
        res = eng.adapt_update()
        g = eng.get_model()
        eng.blend(other, 0.3, 0.6)
        b = eng.get_model()
        return dict(s2=st["s2"], s1=st["s1"], tw=np.array([st["tot_weight"]]), s=res.eigenvalues, T=g["transform"], psi=g["psi"],
                    mean=g["mean"], off=g["offset"], bT=b["transform"], bpsi=b["psi"], bmean=b["mean"])
    return case


def _adapt_chain_probe(name, d, n):
    """record -> adapt_update -> blend under a model of its own (it REPLACES the handle's model twice: ad_work, the solvers)"""
    def build(rng, din, dout):
        import adapt_model as AM
        model, other = AM.synthetic_model(d, int(rng.integers(1 << 30))), AM.synthetic_model(d, int(rng.integers(1 << 30)))
        x = AM.sample(*model, n, int(rng.integers(1 << 30)), scale=1.4, offset=0.1 * np.ones(d))
        return dict(mean=model[0], T=model[1], psi=model[2], mean2=other[0], T2=other[1], psi2=other[2], x=x, w=rng.random(n))

    def run(eng, inp):
        eng._dout = None
        eng.adapt_reset()
        out = adapt_and_blend_case((inp["mean"], inp["T"], inp["psi"]), (inp["mean2"], inp["T2"], inp["psi2"]), inp["x"], inp["w"])(eng)
        eng.adapt_reset()
        return out

    return _add(name, "adapt", build, run)


_family("adapt_chain", _adapt_chain_probe("adapt_chain.large", 257, 333), _adapt_chain_probe("adapt_chain.small", 24, 120))
_family("adapt", _adapt_probe("adapt.large", "A200", 650), _adapt_probe("adapt.small", "B33", 40), _adapt_probe("adapt.third", "C7", 9))


# ------------------------------------------------------------------------------------------- the fp64 building blocks (linalg.hip, eig_dc.hip)
def sym_eig_case(G, methods=(0, 1, 2)):
    """the case of test_gpu_scratch_poison.py::test_sym_eig_on_poisoned_scratch: default, block Jacobi and the direct method"""
    def case(eng):
        out = {}
        for method in methods:
            lam, V, used = eng.sym_eig(G, method)
            out["lam%d" % method], out["V%d" % method], out["used%d" % method] = lam, V, np.array([used])
        return out
    return case


def spd_inverse_case(A):
    """the case of test_gpu_scratch_poison.py::test_spd_inverse_on_poisoned_scratch"""
    def case(eng):
        return dict(x=eng.spd_inverse(A))
    return case


def gemm_f64_case(A, B, w, Cin, batch):
    """the case of test_gpu_scratch_poison.py::test_gemm_f64_on_poisoned_scratch: a batch, or one product with A transposed and
    weights along k"""
    def case(eng):
        if batch > 1:
            return dict(c=eng.gemm_f64(A, B, alpha=0.5, beta=2.0, C_in=Cin))
        return dict(c=eng.gemm_f64(A, B, alpha=0.5, beta=2.0, C_in=Cin, transA=True, kw=w))
    return case


def _eig_probe(name, n):
    def build(rng, din, dout):
        a = rng.standard_normal((n, n))
        return dict(G=a @ a.T / n + np.diag(rng.random(n)))

    def run(eng, inp):
        out = {}
        for method in (0, 1, 2):
            out.update(sym_eig_case(inp["G"], (method,))(eng))
            kernels = eng.linalg_last_kernels()
            assert kernels, name
            if method:
                assert out["used%d" % method][0] == method, (name, method, out["used%d" % method])
            out["kernels%d" % method] = _text(";".join(kernels))
        return out

    return _add(name, "sym_eig", build, run)


_family("sym_eig", _eig_probe("sym_eig.large", 333), _eig_probe("sym_eig.small", 65), _eig_probe("sym_eig.third", 7))


def _inv_probe(name, d):
    def build(rng, din, dout):
        a = rng.standard_normal((d, d + 5))
        return dict(A=a @ a.T + 0.5 * np.eye(d))

    def run(eng, inp):
        out = spd_inverse_case(inp["A"])(eng)
        kernels = eng.linalg_last_kernels()
        assert kernels, name
        out["kernels"] = _text(";".join(kernels))
        return out

    return _add(name, "spd_inverse", build, run)


# (D <= 256: block sweeps on the fp64 matrix cores; above: blocked whitening)
_family("spd_inverse", _inv_probe("spd_inverse.large", 300), _inv_probe("spd_inverse.small", 33), _inv_probe("spd_inverse.third", 200))


def _gemm_probe(name, m, n, k, batch):
    def build(rng, din, dout):
        if batch > 1:
            return dict(A=rng.standard_normal((batch, m, k)), B=rng.standard_normal((batch, k, n)), Cin=rng.standard_normal((batch, m, n)))
        return dict(A=rng.standard_normal((k, m)), B=rng.standard_normal((k, n)), w=rng.random(k), Cin=rng.standard_normal((m, n)))

    def run(eng, inp):
        out = gemm_f64_case(inp["A"], inp["B"], inp.get("w"), inp["Cin"], batch)(eng)
        kernels = eng.linalg_last_kernels()
        assert kernels, name
        out["kernels"] = _text(";".join(kernels))
        return out

    return _add(name, "gemm_f64", build, run)


# (64 x 64 x 20000: split-K with its second-stage reduction over linalg_part)
_family("gemm_f64", _gemm_probe("gemm_f64.large", 64, 64, 20000, 1), _gemm_probe("gemm_f64.small", 17, 33, 9, 1),
        _gemm_probe("gemm_f64.third", 200, 200, 200, 3))


# =========================================================================================== the buffers of the handle
def _p(*names):
    for n in names:
        assert n in PROBES, n
    return tuple(names)


_MODEL = _p("transform.large", "transform.small")
_FIT = _p("fit.large", "fit.small")
_GROUP = _p("fit.large", "groups.large", "lda.large", "embed_fit.large", "embed_fit.small", "lda.small", "groups.small", "fit.small")
_LDA = _p("lda.large", "lda.small")
_SCORE = _p("score.large", "topn.large", "asnorm.large", "trials.large", "ahc_operand.large", "prepared.large", "prepared.small", "ahc_operand.small",
            "trials.small", "asnorm.small", "topn.small", "score.small")
_EIG = _p("fit.large", "lda.large", "embed_fit.large", "sym_eig.large", "sym_eig.small", "embed_fit.small", "lda.small", "fit.small")
_LINALG = _p("fit.large", "lda.large", "embed_fit.large", "sym_eig.large", "spd_inverse.large", "gemm_f64.large", "dense_pca.large",
             "dense_pca.small", "gemm_f64.small", "spd_inverse.small", "sym_eig.small", "embed_fit.small", "lda.small", "fit.small")
_NO_RANKS = "needs several ranks (tests/test_gpu_comm_procs.py)"
BUFFERS = {
    "d_mean": _MODEL, "d_transform": _MODEL, "d_psi": _p("score.large", "score.small"), "d_offset": _MODEL,
    "f_means": _FIT, "f_counts": _FIT, "f_scatter": _FIT, "f_sum": _FIT, "f_W": _FIT, "f_B": _FIT, "fit_flag": _FIT,
    "fit_sort": _GROUP, "fit_offsets": _GROUP, "fit_hist": _GROUP, "fit_roww": _GROUP,
    "fit_xc": _FIT, "fit_mu": _FIT, "fit_csum": _FIT, "em_rows": _FIT, "em_mats": _FIT, "em_chunks": _FIT,
    "grp_pos": _p("groups.large", "groups.small"), "grp_uniq": _p("groups.large", "groups.small"),
    "l_means": _LDA, "l_priors": _LDA, "l_xbar": _LDA, "l_scalings": _LDA, "l_coef": _LDA, "l_intercept": _LDA, "l_evr": _LDA, "lda_work": _LDA,
    "hio_O": _p("score.large", "score.small"),
    "s_Apk": _SCORE, "s_Bpk": _SCORE, "s_rbias": _SCORE, "s_rscale": _SCORE, "s_cbias": _SCORE, "s_rpair": _SCORE, "s_cpair": _SCORE,
    "s_A16": _p("score.large", "asnorm.large", "asnorm.small", "score.small"), "s_B16": _p("score.large", "asnorm.large", "asnorm.small", "score.small"),
    "host_flag": _p("pairs.long", "prepared.large", "prepared.small"), "pair_tab": _p("pairs.long", "pairs.third"),
    "zn_pilot_rows": _p("groups.large", "groups.third", "groups.small"),
    "zn_pilot_sums": "only PLDA_ZNORM_VARIANT=1 uses it, and that arm sums with floating-point atomics: two fresh handles differ in bits (test_gpu_scratch_poison.py holds it to the oracle only)",
    "tf_pad": _p("transform.L300", "transform.large", "transform.truncated", "transform.small", "transform.third"),
    "jac_work": _EIG, "simdiag_state": _p("fit.large", "lda.large", "embed_fit.large", "embed_fit.small", "lda.small", "fit.small"),
    "linalg_part": _LINALG, "syrk_wts": _FIT, "eigdc": _EIG,
    "coef_cache": _SCORE, "bt4_cnt": _p("bt4.large", "score.large", "score.small", "bt4.small"),
    "bt4_fringe": _p("bt4.large", "score.large", "score.small", "bt4.small"),
    "cs_work": _p("prepared.large", "asnorm.large", "prepared.small", "asnorm.small"),
    "timeline": "exists in the diagnostic build only",
    "comm_mm": _NO_RANKS, "comm_mc": _NO_RANKS, "comm_counts": _NO_RANKS, "comm_hist": _NO_RANKS,
    "zn_rows": _p("groups.large", "groups.third", "groups.small"), "zn_y": _p("groups.large", "groups.third", "groups.small"),
    "zn_small": _p("groups.large", "groups.third", "groups.small"), "zn_cpad": _p("groups.large", "groups.small"),
    "eer_slab": _p("trials.large", "eer.large", "mindcf.large", "calib_pass.large", "calib_pass.small", "mindcf.small", "eer.small", "trials.small"),
    "eer_smp": _p("trials.large", "eer.large", "eer.small", "trials.small"),
    "trial_hist": _p("trials.large", "eer.large", "det.large", "mindcf.large", "mindcf.small", "det.small", "eer.small", "trials.third"),
    "eer_list": _p("trials.large", "eer.large", "mindcf.large", "mindcf.small", "eer.small", "trials.third"),
    "calib_part": _p("calibration.large", "calib_pass.large", "calib_pass.small", "calibration.small"), "fusion_part": _p("calibration.large", "calibration.small"),
    "sn_slab": _p("asnorm.large", "topn.large", "ahc_operand.large", "dense_pca.large", "dense_pca.small", "ahc_operand.small", "topn.small", "asnorm.small"),
    "ad_rec": _p("adapt.large", "adapt.small"), "ad_slab": _p("adapt.large", "adapt.small"), "ad_stage": _p("adapt.large", "adapt.small"),
    "ad_work": _p("adapt_chain.large", "adapt_chain.small"),
    "ahc_scratch": _p("ahc.large", "ahc_operand.large", "ahc.small"), "ahc_tab": _p("ahc.large", "ahc.small"), "ahc_slot": _p("ahc.large", "ahc.small"),
    "ahc_stat": _p("ahc.large", "ahc.small"),
    "dp_scratch": _p("dense_pca.large", "dense_pca.third", "dense_pca.small"), "dp_tab": _p("dense_pca.large", "dense_pca.small"),
    "dp_stat": _p("dense_pca.large", "dense_pca.small"), "dp_model": _p("dense_pca.large", "dense_pca.third", "dense_pca.small"),
    "vbx_scratch": _p("vbx.large", "vbx2.large", "vbx.small"), "vbx_tab": _p("vbx.large", "vbx.small"), "vbx_stat": _p("vbx.large", "vbx.small"),
    "der_scratch": _p("der.large", "der_timed.large", "der.small"), "der_tab": _p("der.large", "der_sweep.large", "der_timed.large", "der.small"),
    "der_stat": _p("der.large", "der_sweep.large", "der_timed.large", "der_timed.small", "der.small"),
    "der_atoms": _p("der_timed.large", "der_timed_ovl.large", "der_timed_sweep.large", "der_timed.small"),
    "der_events": _p("der_timed.large", "der_timed_sweep.large", "der_timed.small"),
    "em_min": _p("embed.large", "embed.small"), "em_A": _p("embed.large", "embed.small"), "em_mout": _p("embed.large", "embed.small"),
    "em_apad": _p("embed.small", "embed.third"), "em_v": _p("embed.large", "embed.small"), "em_g": _p("embed.large", "embed.small"),
    "em_fit": _p("embed_fit.large", "embed_fit.small"),
}
# the creation-time switches under which a buffer is reached (its probes run on handles made with them, against fresh
# handles made the same way)
UNDER = {"s_A16": BF16X3, "s_B16": BF16X3, "bt4_cnt": BT4, "bt4_fringe": BT4}
# shared by two modules by attribution, yet without neighbour pairs of their own, each with its reason
NOT_NEIGHBOURS = {
    "d_mean": "model arrays: written by the model routes only, which family (d) follows with every consumer",
    "d_transform": "model arrays: written by the model routes only, which family (d) follows with every consumer",
    "d_psi": "model arrays: written by the model routes only, which family (d) follows with every consumer",
    "d_offset": "model arrays: written by the model routes only, which family (d) follows with every consumer",
}


def _modules(buf):
    use = BUFFERS[buf]
    return set() if isinstance(use, str) else {PROBES[n].module for n in use}


# the buffers several modules share (derived: every buffer whose probes come from two modules or more): the neighbours
# family runs every ordered pair of different modules over each
SHARED = tuple(b for b in BUFFERS if len(_modules(b)) >= 2 and b not in NOT_NEIGHBOURS)


def handle_buffers(text):
    """the plda::DevBuf members of `struct plda_handle` in the text of plda_amd/csrc/common.hpp (arrays by their name)"""
    import re
    body = text[text.index("struct plda_handle {"):]
    body = body[:body.index("\n};")]
    names = []
    for decl in re.findall(r"^\s*plda::DevBuf\s+([^;]+);", body, re.M):
        for part in decl.split(","):
            names.append(re.sub(r"\[\d+\]", "", part).strip())
    return names


def neighbour_pairs():
    """[(buffer, X, Y)]: for every shared buffer and every ordered pair of different modules that use it, the first module's
    probe with the largest use (its first in BUFFERS) and the second module's with the smallest (its last); a pair that an
    earlier buffer already gave (under the same switches) is not repeated"""
    out, seen = [], set()
    for buf in SHARED:
        by_module = {}
        for name in BUFFERS[buf]:
            by_module.setdefault(PROBES[name].module, []).append(name)
        under = tuple(sorted(UNDER.get(buf, {}).items()))
        for a in by_module:
            for b in by_module:
                key = (by_module[a][0], by_module[b][-1], under)
                if a != b and key not in seen:
                    seen.add(key)
                    out.append((buf, by_module[a][0], by_module[b][-1]))
    return out


# =========================================================================================== model routes and refusals
def _route_set(key):
    return lambda eng: eng.set_model(*model(key))


def _route_fit(name):
    return lambda eng: PROBES[name](eng)


def _route_adapt(eng):
    dout, din = eng.dims()
    x = rng_of("route.adapt", din).standard_normal((3 * din + 50, din)) * 1.4 + 0.1
    eng.adapt(x, None, 0.3, 0.7, 1.0)


def _route_blend(eng):
    dout, din = eng.dims()
    rng = rng_of("route.blend", din)
    q, _ = np.linalg.qr(rng.standard_normal((din, din)))
    eng.blend((rng.random(din), q * (0.6 + rng.random(din))[:, None], np.sort(rng.random(din) * 2.0 + 0.1)[::-1].copy()), 0.25, 0.5)


def _route_truncate(eng):
    eng._dout = None
    dout = eng.dims()[0]
    eng.truncate(max(min(dout, 5), (dout * 3) // 4))         # (never below 5 dimensions, however often the walk draws it)


# name -> (apply(eng), square: the route needs a square model and leaves one)
ROUTES = {
    "set_model.same": (_route_set("F104"), False), "set_model.smaller": (_route_set("B33"), False), "set_model.larger": (_route_set("A200"), False),
    "fit": (_route_fit("fit.small"), False), "fit_stats_em": (_route_fit("fit.split"), False),
    "truncate": (_route_truncate, False), "smooth": (lambda eng: eng.smooth(0.5), False),
    "adapt_update": (_route_adapt, True), "blend": (_route_blend, True),
}


class Refused(AssertionError):
    pass


def expect_status(eng, code, call, match=None):
    """call() must end in a PldaError of exactly this status (and, with match, a message that holds it)"""
    from plda_amd._native import PldaError
    try:
        call()
    except PldaError as e:
        assert e.code == code, "status %d where %d is documented: %s" % (e.code, code, e)
        assert match is None or match in str(e), "refused for another reason than %r: %s" % (match, e)
        return
    raise Refused("the call was accepted where status %d is documented" % code)


def _raw(eng, fn, *args):
    from plda_amd._native import check
    check(eng._h, getattr(eng._lib, fn)(eng._h, *args))


def _refuse_vbx_nan(eng):
    """a NaN row of y: found by the device (include/plda_hip.h: "a non-finite y ... " after the argument checks)"""
    d, t = 16, 40
    rng = rng_of("refuse.vbx")
    y = rng.standard_normal((t, d))
    y[17, 3] = np.nan
    lab = (np.arange(t) % 3).astype(np.int32)
    off = np.array([0, t], np.int64)
    phi = np.ones(d)
    ol, ok = np.empty(t, np.int32), np.empty(1, np.int32)
    expect_status(eng, E_INVAL, lambda: _raw(eng, "plda_vbx", _c(y), d, _c(phi), _c(lab), _c(off), 1, 0.3, 17.0, 0.99, 5.0, 5, 1e-4, _c(ol), _c(ok),
                                              None, None, None, None, None, None))


def _refuse_dense_nan(eng):
    dout, din = eng.dims()
    x = rng_of("refuse.dense", din).standard_normal((12, din))
    x[5, 0] = np.nan
    off, boff = np.array([0, 12], np.int64), np.array([0, 144], np.int64)
    s = np.zeros(144, np.float32)
    expect_status(eng, E_INVAL, lambda: _raw(eng, "plda_score_dense_pca", _c(x), _c(off), 1, 0.5, _c(s), _c(boff), None, None))


def _refuse_dense_singular(eng):
    """Dense PCA under a model whose transform is all zero: T^T T is not positive definite, found by the factorisation's flag
    after the covariances were formed on the device (PLDA_E_NUMERIC; the input of test_gpu_adapt.py's singular blend, through
    the same model_covariances_f64).  It leaves the covariance cache of the handle half-built."""
    dout, din = eng.dims()
    m = eng.get_model()
    eng.set_model(m["mean"], np.zeros((din, din)), np.ones(din))
    x = rng_of("refuse.dense", din).standard_normal((12, din))
    off, boff = np.array([0, 12], np.int64), np.array([0, 144], np.int64)
    s = np.zeros(144, np.float32)
    expect_status(eng, E_NUMERIC, lambda: _raw(eng, "plda_score_dense_pca", _c(x), _c(off), 1, 0.5, _c(s), _c(boff), None, None), "singular")
    eng.set_model(m["mean"], m["transform"], m["psi"])          # the model it had: what follows runs under a sound one


def refuse_dense_truncated(eng):
    """dense PCA on a truncated model (Dout < Din): PLDA_E_INVAL"""
    dout, din = eng.dims()
    assert dout < din
    x = rng_of("refuse.dense", din).standard_normal((12, din))
    off, boff = np.array([0, 12], np.int64), np.array([0, 144], np.int64)
    s = np.zeros(144, np.float32)
    expect_status(eng, E_INVAL, lambda: _raw(eng, "plda_score_dense_pca", _c(x), _c(off), 1, 0.5, _c(s), _c(boff), None, None))


def _refuse_ahc_nonfinite(eng):
    import ahc_model
    b = ahc_model.gaussian(40, 5).astype(np.float32)
    b[7, 9] = b[9, 7] = np.inf
    from plda_amd import diarize
    expect_status(eng, E_INVAL, lambda: diarize.ahc(eng, [b], None, 1))


def _refuse_pairs_index(eng):
    dout, din = eng.dims()
    rng = rng_of("refuse.pairs", dout)
    m, nt, p = 23, 40, PAIRS_TAB_MIN + 5
    U, V = rng.standard_normal((m, dout)), rng.standard_normal((nt, dout))
    n = rng.integers(1, 4, m).astype(np.int32)
    e, t = rng.integers(0, m, p), rng.integers(0, nt, p)
    t[p - 7] = nt                                    # one index past the test side: found by the device's check of a long list
    expect_status(eng, E_INVAL, lambda: score_pairs(eng, U, n, V, e, t))


def _refuse_groups_capacity(eng):
    dout, din = eng.dims()
    rng = rng_of("refuse.groups", din)
    x, y = rng.random((60, din)), rng.integers(0, 9, 60).astype(np.uint64)
    y[:9] = np.arange(9)
    cap = C.c_int64(4)                               # nine groups into room for four
    ol, oc, ov = np.empty(4, np.uint64), np.empty(4, np.int64), np.empty((4, dout))
    expect_status(eng, E_CAPACITY, lambda: _raw(eng, "plda_transform_groups", _c(x), 60, din, _c(y), _c(ol), _c(oc), _c(ov), C.byref(cap)))


def _refuse_der_label(eng):
    """a reference label at its limit (64): found by the device, after the host-side argument checks"""
    ref = np.array([0, 1, 64, 2], np.int32)
    hyp = np.array([0, 1, 1, 2], np.int32)
    off, counts = np.array([0, 4], np.int64), np.empty((1, 4), np.int64)
    expect_status(eng, E_INVAL, lambda: _raw(eng, "plda_der", _c(ref), _c(hyp), None, _c(off), 1, _c(counts), None))


def _refuse_der_timed_overlap(eng):
    """two hypothesis segments that overlap: the device's disjointness check"""
    ts, td, tk = np.array([0, 50], np.int32), np.array([40, 30], np.int32), np.array([0, 1], np.int32)
    ss, sd, hyp = np.array([0, 10], np.int32), np.array([20, 20], np.int32), np.array([0, 1], np.int32)
    toff, off, counts = np.array([0, 2], np.int64), np.array([0, 2], np.int64), np.empty((1, 4), np.int64)
    expect_status(eng, E_INVAL, lambda: _raw(eng, "plda_der_timed", _c(ts), _c(td), _c(tk), _c(toff), _c(ss), _c(sd), _c(hyp), _c(off), 1, None, None,
                                              None, 0, 0, _c(counts), None))


def _refuse_fit_singular(eng):
    """the input of test_gpu_api_edges.py::test_singular_within_class_covariance_is_reported_by_the_deferred_check: EM keeps W
    positive definite for finite data, so the failing input is a NaN feature; GetOutput's Cholesky fails at the end of the fit"""
    x = rng_of("refuse.fit").random((400, 24))
    x[7, 3] = np.nan
    y = np.repeat(np.arange(40, dtype=np.uint64), 10)
    eng._dout = None
    expect_status(eng, E_NUMERIC, lambda: eng.fit(x, y, 1))


def _refuse_adapt_epoch(eng):
    """a record taken under one model, the update asked for under the next: PLDA_E_INVAL"""
    dout, din = eng.dims()
    x = rng_of("refuse.adapt", din).standard_normal((din + 20, din))
    eng.adapt_reset()
    eng.adapt_accumulate(x)
    m = eng.get_model()
    eng.set_model(m["mean"], m["transform"], m["psi"])          # the same numbers: a new epoch
    expect_status(eng, E_INVAL, lambda: eng.adapt_update(), "taken under an earlier model")
    eng.adapt_reset()


# name -> (call(eng), the module's own next valid probe, a probe of a module that shares a buffer with it, needs a model)
REFUSALS = {
    "vbx.nan_row": (_refuse_vbx_nan, "vbx.small", "ahc.small", "E16"),
    "dense_pca.nan_row": (_refuse_dense_nan, "dense_pca.small", "asnorm.small", "B33"),
    "dense_pca.singular_model": (_refuse_dense_singular, "dense_pca.small", "adapt.small", "B33"),
    "ahc.nonfinite": (_refuse_ahc_nonfinite, "ahc.small", "dense_pca.small", "B33"),
    "pairs.index": (_refuse_pairs_index, "pairs.long", "prepared.small", "B33"),
    "groups.capacity": (_refuse_groups_capacity, "groups.small", "fit.small", "B33"),
    "der.label": (_refuse_der_label, "der.small", "der_timed.small", None),
    "der_timed.overlap": (_refuse_der_timed_overlap, "der_timed.small", "der.small", None),
    "fit.singular": (_refuse_fit_singular, "fit.small", "lda.small", None),
    "adapt.epoch": (_refuse_adapt_epoch, "adapt.small", "transform.small", "B33"),
}


# =========================================================================================== the comparison and the runner
def same_bits(got, want, what=""):
    """np.array_equal on the uint8 views of every output, shapes and dtypes included"""
    assert sorted(got) == sorted(want), "%s: outputs %s against %s" % (what, sorted(got), sorted(want))
    for k in sorted(want):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, "%s: %s is %s %s, fresh %s %s" % (what, k, a.dtype, a.shape, b.dtype, b.shape)
        if not np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)):
            differ = int((a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8)).sum())
            raise AssertionError("%s: %s differs from the fresh handle's in %d of %d bytes" % (what, k, differ, a.nbytes))


def model_key(eng):
    """the installed model as bytes (None without one): what `the same model` means"""
    from_engine = getattr(eng, "history_model", None)
    if from_engine is not None:
        return from_engine()
    try:
        m = eng.get_model()
    except Exception as e:       # noqa: BLE001
        if getattr(e, "code", E_NOT_FITTED) != E_NOT_FITTED:      # (a device error is not "no model")
            raise
        return None
    return (m["transform"].shape, m["mean"].tobytes(), m["transform"].tobytes(), m["psi"].tobytes())


def _triple(key):
    (dout, din), mean, t, psi = key
    return np.frombuffer(mean), np.frombuffer(t).reshape(dout, din), np.frombuffer(psi)


class Harness(object):
    """Runs probes on long-lived engines and holds each result to a fresh engine's.  make(): a fresh engine.  Fresh results
    are computed once per (probe, model) and kept."""

    def __init__(self, make, probes=None, models=None):
        self.make, self.probes, self.fresh = make, PROBES if probes is None else probes, {}
        self.model = model if models is None else models        # home -> (mean, transform, psi)
        self.log = []

    def expected(self, name, key, switches=()):
        """the probe's result on a fresh handle made under `switches` and given the model `key`: once per (probe, model,
        creation-time switches)"""
        if (name, key, switches) not in self.fresh:
            eng = self.make(**dict(switches)) if switches else self.make()
            if key is not None:
                eng.set_model(*_triple(key))
            self.fresh[(name, key, switches)] = self.probes[name](eng)
        return self.fresh[(name, key, switches)]

    def install(self, eng, home):
        if home is not None:
            eng._dout = None
            eng.set_model(*self.model(home))
        self.log.append("model %s" % home)

    def check(self, eng, name, what=""):
        """the probe on eng (its home model installed first, where it has one) against the fresh handle's"""
        probe = self.probes[name]
        if probe.home is not None:
            self.install(eng, probe.home)
        self.check_here(eng, name, what)

    def check_here(self, eng, name, what=""):
        """the probe on eng under whatever model eng holds"""
        self.log.append(name)
        key = model_key(eng)
        got = self.probes[name](eng)
        same_bits(got, self.expected(name, key, tuple(sorted(switches_of(eng).items()))), "%s [%s]" % (name, what or " -> ".join(self.log[-6:])))
        return got

    def shrink_and_regrow(self, eng, family):
        f = FAMILIES[family] if isinstance(family, str) else family
        orders = [("large", "small", "large"), ("small", "large", "small")]
        if "third" in f:
            orders += [("small", "third", "small"), ("third", "large", "third")]
        for order in orders:
            for size in order:
                self.check(eng, f[size], "%s" % (order,))

    def neighbours(self, eng, x, y):
        """X then Y on one handle: Y equals fresh (X is held to the law as well: it costs nothing more)"""
        self.check(eng, x, "neighbours, first")
        self.check(eng, y, "after %s" % x)

    def route(self, eng, home, warm, route, consumers, before=None, after=None):
        """under model `home` every cache is warmed (the probes `warm`, held to the law too), `before(eng)` leaves what the
        route must invalidate, route(eng) replaces the model, `after(eng)` asserts the documented refusals, and every consumer
        equals a fresh handle given get_model() through set_model"""
        self.install(eng, home)
        for name in warm:
            self.check_here(eng, name, "warming under %s" % home)
        if before is not None:
            before(eng)
        route(eng)
        self.log.append("route")
        if after is not None:
            after(eng)
        for name in consumers:
            self.check_here(eng, name, "after the route")

    def after_refusal(self, eng, home, refuse, own, other):
        """refuse(eng) asserts its status code itself; the next valid call of the same module and of a module that shares a
        buffer with it equal fresh"""
        for nxt in (own, other):
            self.install(eng, home)
            refuse(eng)
            self.log.append("refused")
            self.check(eng, nxt, "after a refused call")

    def walk(self, engines, steps, routes, refusals, roaming=(), stream=None, square="D104"):
        """steps: walk_steps()'s list.  A probe in `roaming` runs under whatever model its handle holds, every other one under
        its home model; a route that needs a square model gets `square` installed first where the handle's is not; stream(eng,
        on): moves the handle to a side stream and back."""
        for i, (which, kind, name) in enumerate(steps):
            eng = engines[which]
            what = "step %d of %s" % (i, steps)
            if kind == "probe":
                (self.check_here if name in roaming and model_key(eng) is not None else self.check)(eng, name, what)
            elif kind == "route":
                apply, needs_square = routes[name]
                key = model_key(eng)
                if key is None or (needs_square and key[0][0] != key[0][1]):
                    self.install(eng, square)
                apply(eng)
            elif kind == "refuse":
                call, _, _, home = refusals[name]
                if home is not None:
                    self.install(eng, home)
                call(eng)
            elif kind == "stream" and stream is not None:
                stream(eng, name == "side")
            self.log.append("%s %s" % (kind, name))


# the probes of the walk: those that run on a handle made without a creation-time switch
WALK_PROBES = sorted(n for n, p in PROBES.items() if not p.switches)


def walk_steps(seed, count, probes, routes, refusals, handles=2):
    """[(handle, kind, name)]: a function of the seed alone.  The handles alternate; about two steps in three are probes, the
    rest routes, refused calls and moves of the stream."""
    rng = np.random.default_rng([seed_of("walk"), int(seed)])
    probes, routes, refusals = sorted(probes), sorted(routes), sorted(refusals)
    steps, side = [], [False] * handles
    for i in range(int(count)):
        which, u = i % handles, rng.random()
        if u < 0.58 or not (routes or refusals):
            steps.append((which, "probe", probes[int(rng.integers(len(probes)))]))
        elif u < 0.72 and routes:
            steps.append((which, "route", routes[int(rng.integers(len(routes)))]))
        elif u < 0.82 and refusals:
            steps.append((which, "refuse", refusals[int(rng.integers(len(refusals)))]))
        else:
            side[which] = not side[which]
            steps.append((which, "stream", "side" if side[which] else "own"))
    return steps
