"""GPU: the C-ABI glue of csrc/api.hip, through ctypes alone -- what every host-pointer entry point refuses (status code and
plda_last_error text, in the order of its checks), that a host form computes bit for bit what its device form computes with
every optional argument present and absent, the 4 MiB threshold of the pinned ring, and the values plda_create refuses.
No call may leave device memory behind (plda_device_bytes_held)."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_data

pytestmark = pytest.mark.gpu

OK, INVAL, NOT_FITTED, LABELS, CAPACITY = 0, -1, -4, -6, -7
D = 20
OFFSETS = np.array([0, 5, 6, 13], np.int64)      # recordings of 5, 1 and 7 rows
R, T = 3, 13
M, NT, TOP_N, Q = 5, 7, 2, 3
BLOCK_OFF = np.array([0, 25, 26, 75], np.int64)  # N_r^2 floats per recording, packed


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx():
    import torch
    from plda_amd import MPlda, _native as N
    c = Ctx()
    c.torch, c.N, c.lib = torch, N, N.load()
    x, y = make_data(41, 900, D, 30, skew=True, scale_between=0.5)
    c.eng = MPlda(0)
    c.eng.fit(x, y, 4)
    c.fresh = MPlda(0)
    c.h, c.f = c.eng._h, c.fresh._h
    c.x = x
    rng = np.random.default_rng(7)
    c.U, c.V = rng.standard_normal((M, D)), rng.standard_normal((NT, D))
    c.n = np.array([1, 2, 3, 2, 1], np.int32)
    c.zm, c.zs = rng.standard_normal(M), rng.random(M) + 0.5
    c.em, c.es = rng.standard_normal(M), rng.random(M) + 0.5
    c.tm, c.ts = rng.standard_normal(NT), rng.random(NT) + 0.5
    c.X = np.ascontiguousarray(x[:T])                       # raw rows of the three recordings
    c.Y = rng.standard_normal((T, D))                       # PLDA-space rows of the three recordings
    c.nT = (np.arange(T) % 3 + 1).astype(np.int32)
    # an LDA model and an embedding chain on the fitted handle
    lx = rng.standard_normal((60, D)) + np.repeat(rng.standard_normal((4, D)), 15, 0)
    ll = np.repeat(np.arange(4, dtype=np.uint64), 15)
    assert c.lib.plda_lda_fit(c.h, lx.ctypes.data, 60, D, ll.ctypes.data, 0, None) == OK, N.last_error(c.h)
    c.m_in, c.A, c.m_out = rng.standard_normal(D), rng.standard_normal((8, D)), rng.standard_normal(8)
    assert c.lib.plda_embed_set(c.h, D, 8, c.m_in.ctypes.data, 1.0, c.A.ctypes.data, c.m_out.ctypes.data, 1.0) == OK, N.last_error(c.h)
    c.zero = np.zeros(1 << 14, np.int64)                    # a valid pointer for arguments no refused call reads far into
    return c


def _hp(a):
    return None if a is None else a.ctypes.data


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _call(c, fn, dev, args, ins, outs, strict=True):
    """One call of `fn`.  args: a list whose str entries name arrays of ins / outs (device tensors for dev, host arrays
    otherwise; None stays NULL), every other entry is passed as it is.  Returns {output name: array}.  Asserts PLDA_OK and that
    (strict) the call holds no device memory afterwards that it did not hold before."""
    torch, lib = c.torch, c.lib
    keep, res = {}, {}
    for k, v in ins.items():
        keep[k] = None if v is None else (torch.from_numpy(np.ascontiguousarray(v)).cuda() if dev else np.ascontiguousarray(v))
    for k, v in outs.items():
        keep[k] = None if v is None else (torch.zeros(v[0], dtype=getattr(torch, v[1])).cuda() if dev else np.zeros(v[0], getattr(np, v[1])))
    ptr = lambda t: None if t is None else (t.data_ptr() if dev else t.ctypes.data)
    a = [ptr(keep[x]) if isinstance(x, str) else x for x in args]
    torch.cuda.synchronize()
    held = lib.plda_device_bytes_held()
    rc = getattr(lib, fn)(c.h, *a)
    assert rc == OK, "%s: status %d: %s" % (fn, rc, c.N.last_error(c.h))
    assert lib.plda_synchronize(c.h) == OK
    assert not strict or lib.plda_device_bytes_held() == held, "%s left %d bytes on the device" % (fn, lib.plda_device_bytes_held() - held)
    for k in outs:
        if keep[k] is not None:
            res[k] = keep[k].cpu().numpy() if dev else keep[k]
    return res


def _parity(c, name, dev_args, host_args, ins, outs):
    """device form twice (bit-equal), host form once (bit-equal to them); one unchecked call of each first, so that the
    handle's own scratch has its final size.  Returns the host form's outputs."""
    _call(c, name + "_dev", True, dev_args, ins, outs, strict=False)
    _call(c, name, False, host_args, ins, outs, strict=False)
    d1 = _call(c, name + "_dev", True, dev_args, ins, outs)
    d2 = _call(c, name + "_dev", True, dev_args, ins, outs)
    hh = _call(c, name, False, host_args, ins, outs)
    assert set(d1) == set(d2) == set(hh)
    for k in d1:
        assert _same(d1[k], d2[k]), "%s_dev: %s differs between two runs" % (name, k)
        assert _same(d1[k], hh[k]), "%s: %s differs between the host and the device form" % (name, k)
    return hh


def _common_equal(name, a, b):
    for k in set(a) & set(b):
        assert _same(a[k], b[k]), "%s: %s changes when an optional argument is left out" % (name, k)


# ---------------------------------------------------------------- form parity
@pytest.mark.parametrize("counts", [True, False])
def test_parity_transform_rows(ctx, counts):
    a = ["X", T, D, "n", 0 if counts else 2, "out"]
    _parity(ctx, "plda_transform_rows", a, a, {"X": ctx.X, "n": ctx.nT if counts else None}, {"out": ((T, D), "float64")})


def test_parity_project_rows(ctx):
    a = ["X", T, D, "out"]
    _parity(ctx, "plda_project_rows", a, a, {"X": ctx.X}, {"out": ((T, D), "float64")})


def test_parity_znorm_stats(ctx):
    a = ["bkg", T, 2, D, "models", M, "mean", "std"]
    _parity(ctx, "plda_znorm_stats", a, a, {"bkg": ctx.X, "models": ctx.U}, {"mean": ((M,), "float64"), "std": ((M,), "float64")})


@pytest.mark.parametrize("counts", [True, False])
def test_parity_cohort_stats(ctx, counts):
    a = ["X", "n", 0 if counts else 2, M, "C", NT, TOP_N, "mean", "std"]
    _parity(ctx, "plda_cohort_stats", a, a, {"X": ctx.U, "n": ctx.n if counts else None, "C": ctx.V},
            {"mean": ((M,), "float64"), "std": ((M,), "float64")})


@pytest.mark.parametrize("counts", [True, False])
@pytest.mark.parametrize("znorm", [True, False])
def test_parity_score_matrix(ctx, counts, znorm):
    a = ["U", "n", 0 if counts else 2, M, "V", NT, "zm", "zs", "out", NT]
    _parity(ctx, "plda_score_matrix", a, a, {"U": ctx.U, "n": ctx.n if counts else None, "V": ctx.V, "zm": ctx.zm if znorm else None,
                                             "zs": ctx.zs if znorm else None}, {"out": ((M, NT), "float32")})


@pytest.mark.parametrize("counts", [True, False])
@pytest.mark.parametrize("sides", ["both", "enrol", "test"])
def test_parity_score_matrix_snorm(ctx, counts, sides):
    e, t = sides != "test", sides != "enrol"
    a = ["U", "n", 0 if counts else 2, M, "V", NT, "em", "es", "tm", "ts", "out", NT]
    _parity(ctx, "plda_score_matrix_snorm", a, a,
            {"U": ctx.U, "n": ctx.n if counts else None, "V": ctx.V, "em": ctx.em if e else None, "es": ctx.es if e else None,
             "tm": ctx.tm if t else None, "ts": ctx.ts if t else None}, {"out": ((M, NT), "float32")})


@pytest.mark.parametrize("stats", ["", "z", "et", "e", "t"])      # (the library refuses z-norm together with S-norm statistics)
@pytest.mark.parametrize("counts", [True, False])
@pytest.mark.parametrize("axis", [0, 1])
def test_parity_score_topn(ctx, stats, counts, axis):
    L = M if axis == 0 else NT
    pair = lambda k, a, b: (a, b) if k in stats else (None, None)
    (zm, zs), (em, es), (tm, ts) = pair("z", ctx.zm, ctx.zs), pair("e", ctx.em, ctx.es), pair("t", ctx.tm, ctx.ts)
    a = ["U", "n", 0 if counts else 2, M, "V", NT, "zm", "zs", "em", "es", "tm", "ts", axis, TOP_N, "os", "oi"]
    _parity(ctx, "plda_score_topn", a, a, {"U": ctx.U, "n": ctx.n if counts else None, "V": ctx.V, "zm": zm, "zs": zs, "em": em,
                                           "es": es, "tm": tm, "ts": ts}, {"os": ((L, TOP_N), "float32"), "oi": ((L, TOP_N), "int64")})


@pytest.mark.parametrize("dtype", [0, 1])
def test_parity_dvector_pool(ctx, dtype):
    frames = ctx.Y.astype(np.float32) if dtype == 0 else ctx.Y
    a = ["frames", dtype, T, D, "off", R, 0, 1, "out"]
    _parity(ctx, "plda_dvector_pool", a, a, {"frames": frames, "off": OFFSETS}, {"out": ((R, D), "float64")})


def test_parity_lda_predict(ctx):
    _parity(ctx, "plda_lda_predict", ["X", T, 0, "out"], ["X", T, D, 0, "out"], {"X": ctx.X}, {"out": ((T, 4), "float64")})


def test_parity_lda_transform(ctx):
    _parity(ctx, "plda_lda_transform", ["X", T, 2, "out"], ["X", T, D, 2, "out"], {"X": ctx.X}, {"out": ((T, 2), "float64")})


def test_parity_htk_frames(ctx):
    blob = np.random.default_rng(3).standard_normal(T * 4).astype(">f4").view(np.uint8)     # 16-byte samples, three files back to back
    file_off = np.array([0, 20, 24], np.int64)
    _parity(ctx, "plda_htk_frames", ["blob", "fo", "off", R, T, 16, 1, "out"], ["blob", blob.size, "fo", "off", R, 16, 1, "out"],
            {"blob": blob, "fo": file_off, "off": OFFSETS}, {"out": ((T, 3 * 4), "float32")})


def _ahc_outs(merges):
    o = {"labels": ((T,), "int32"), "ncl": ((R,), "int32"), "ma": None, "mb": None, "mc": None}
    if merges:
        o.update(ma=((T - R,), "int32"), mb=((T - R,), "int32"), mc=((T - R,), "float64"))
    return o


def _ahc_scores():
    rng = np.random.default_rng(5)
    blocks = []
    for r in range(R):
        n = int(OFFSETS[r + 1] - OFFSETS[r])
        s = rng.standard_normal((n, n))
        blocks.append((s + s.T).astype(np.float32).ravel())
    return np.concatenate(blocks)


MINC = np.array([2, 1, 3], np.int32)
AHC_TAIL = ["labels", "ncl", "ma", "mb", "mc"]


@pytest.mark.parametrize("minc", [True, False])
def test_parity_ahc_matrix(ctx, minc):
    a = ["S", _hp(BLOCK_OFF), _hp(OFFSETS), R, 1, 0.0, _hp(MINC) if minc else None] + AHC_TAIL
    res = [_parity(ctx, "plda_ahc_matrix", a, a, {"S": _ahc_scores()}, _ahc_outs(m)) for m in (True, False)]
    _common_equal("plda_ahc_matrix", *res)


@pytest.mark.parametrize("minc", [True, False])
def test_parity_score_ahc(ctx, minc):
    a = ["X", _hp(OFFSETS), R, 1, 0.0, _hp(MINC) if minc else None] + AHC_TAIL
    res = [_parity(ctx, "plda_score_ahc", a, a, {"X": ctx.Y}, _ahc_outs(m)) for m in (True, False)]
    _common_equal("plda_score_ahc", *res)


def test_parity_score_dense_pca(ctx):
    res = []
    for dims, eig in ((True, True), (False, True), (True, False), (False, False)):
        a = ["X", _hp(OFFSETS), R, 0.9, "S", _hp(BLOCK_OFF), "dims", "eig"]
        res.append(_parity(ctx, "plda_score_dense_pca", a, a, {"X": ctx.X},
                           {"S": ((75,), "float32"), "dims": ((R,), "int32") if dims else None, "eig": ((T,), "float64") if eig else None}))
    for other in res[1:]:
        _common_equal("plda_score_dense_pca", res[0], other)


@pytest.mark.parametrize("minc", [True, False])
def test_parity_score_dense_pca_ahc(ctx, minc):
    a = ["X", _hp(OFFSETS), R, 0.9, 1, 0.0, _hp(MINC) if minc else None] + AHC_TAIL
    res = [_parity(ctx, "plda_score_dense_pca_ahc", a, a, {"X": ctx.X}, _ahc_outs(m)) for m in (True, False)]
    _common_equal("plda_score_dense_pca_ahc", *res)


REF = np.array([0, 0, 1, 1, 2, 0, 0, 1, 1, 1, 2, 2, 0], np.int32)
HYP = np.array([1, 1, 0, 0, 0, 3, 0, 0, 1, 1, 2, 1, 0], np.int32)
DUR = (np.arange(T) % 4 + 1).astype(np.int32)


@pytest.mark.parametrize("dur", [True, False])
def test_parity_der(ctx, dur):
    a = ["ref", "hyp", "dur", _hp(OFFSETS), R, "counts", "map"]
    res = [_parity(ctx, "plda_der", a, a, {"ref": REF, "hyp": HYP, "dur": DUR if dur else None},
                   {"counts": ((R, 4), "int64"), "map": ((R, 64), "int32") if m else None}) for m in (True, False)]
    _common_equal("plda_der", *res)


@pytest.mark.parametrize("dur", [True, False])
@pytest.mark.parametrize("minc", [True, False])
def test_parity_der_sweep(ctx, dur, minc):
    # the full merge record of the three recordings: no threshold, down to one cluster
    a = ["X", _hp(OFFSETS), R, 0, 0.0, None] + AHC_TAIL
    rec = _call(ctx, "plda_score_ahc", False, a, {"X": ctx.Y}, _ahc_outs(True), strict=False)
    thr = np.array([-5.0, 0.0, 5.0])
    a = ["ma", "mb", "mc", _hp(OFFSETS), R, "ref", "dur", _hp(thr), Q, _hp(MINC) if minc else None, "counts", "ncl"]
    _parity(ctx, "plda_der_sweep", a, a, {"ma": rec["ma"], "mb": rec["mb"], "mc": rec["mc"], "ref": REF, "dur": DUR if dur else None},
            {"counts": ((Q, R, 4), "int64"), "ncl": ((Q, R), "int32")})


def test_parity_vbx(ctx):
    lin = np.array([0, 1, 0, 1, 0, 0, 0, 1, 2, 0, 1, 2, 0], np.int32)       # S_r = 2, 1, 3
    goff, poff = np.array([0, 10, 11, 32], np.int64), np.array([0, 2, 3, 6], np.int64)
    phi = np.random.default_rng(9).random(D) + 0.5
    iters = 3
    res = []
    for absent in ("none", "Phi", "gamma", "pi", "elbo", "iters"):
        g, p = absent != "gamma", absent != "pi"
        a = ["Y", D, "Phi", "lin", _hp(OFFSETS), R, 0.3, 17.0, 0.9, 5.0, iters, 1e-4, "labels", "ncl", "gamma", _hp(goff) if g else None, "pi",
             _hp(poff) if p else None, "elbo", "iters"]
        out = _parity(ctx, "plda_vbx", a, a, {"Y": ctx.Y, "Phi": None if absent == "Phi" else phi, "lin": lin},
                      {"labels": ((T,), "int32"), "ncl": ((R,), "int32"), "gamma": ((32,), "float64") if g else None,
                       "pi": ((6,), "float64") if p else None, "elbo": ((R, iters), "float64") if absent != "elbo" else None,
                       "iters": ((R,), "int32") if absent != "iters" else None})
        if absent != "Phi":
            res.append(out)
    for other in res[1:]:
        _common_equal("plda_vbx", res[0], other)


@pytest.mark.parametrize("dtype", [0, 1])
def test_parity_embed_apply(ctx, dtype):
    a = ["X", dtype, T, D, "out"]
    _parity(ctx, "plda_embed_apply", a, a, {"X": ctx.X.astype(np.float32) if dtype == 1 else ctx.X}, {"out": ((T, 8), "float64")})


@pytest.mark.parametrize("rows", [26214, 26215])
def test_ring_threshold_of_transform_rows(ctx, rows):
    """rows * 20 * 8 bytes: 4 194 240 stay under the 4 MiB threshold (plain copies), 4 194 400 pass it (the pinned ring, both ways)"""
    X = np.random.default_rng(rows).standard_normal((rows, D))
    a = ["X", rows, D, "n", 3, "out"]
    _parity(ctx, "plda_transform_rows", a, a, {"X": X, "n": None}, {"out": ((rows, D), "float64")})


# ---------------------------------------------------------------- refusals
DER_SEG = ["ref", "hyp", "dur", "offsets", "R", "counts", "map"]
DER_SWEEP = ["ma", "mb", "mc", "offsets", "R", "ref", "dur", "thr", "Q", "minc", "counts", "ncl"]
DER_TIMED = ["tstart", "tdur", "tspk", "turn_off", "sstart", "sdur", "hyp", "offsets", "R", "ustart", "udur", "uem_off", "collar",
             "flags", "counts", "map"]
DER_TIMED_OVL = DER_TIMED[:7] + ["hyp2"] + DER_TIMED[7:]
DER_TIMED_SWEEP = ["ma", "mb", "mc"] + DER_TIMED[:6] + DER_TIMED[7:14] + ["thr", "Q", "minc", "counts", "ncl"]
# entry point (and its _dev form, which takes the same arguments) -> (the text's prefix, argument order, sweep, timed, JER)
DER_FORMS = {
    "plda_der": ("der", DER_SEG, False, False, False),
    "plda_der_sweep": ("der_sweep", DER_SWEEP, True, False, False),
    "plda_der_jer": ("der_jer", DER_SEG + ["jer", "jmap", "spk"], False, False, True),
    "plda_der_jer_sweep": ("der_jer_sweep", DER_SWEEP + ["jer"], True, False, True),
    "plda_der_timed": ("der_timed", DER_TIMED, False, True, False),
    "plda_der_timed_ovl": ("der_timed_ovl", DER_TIMED_OVL, False, True, False),
    "plda_der_timed_sweep": ("der_timed_sweep", DER_TIMED_SWEEP, True, True, False),
    "plda_der_timed_jer": ("der_timed_jer", DER_TIMED_OVL + ["jer", "jmap", "spk"], False, True, True),
    "plda_der_timed_jer_sweep": ("der_timed_jer_sweep", DER_TIMED_SWEEP + ["jer"], True, True, True),
}


def _der_refusals(c):
    """The whole refusal ladder of every DER entry point, host and device form (plda_der and plda_der_sweep: the device form; their
    host forms are in the table below).  A ladder starts with every argument in the state its check refuses and mends ONE
    argument per row, in the order of the library's checks: each row fails on the check behind the previous row's, while
    everything a later check looks at is still wrong.  No row gets as far as a launch or an allocation."""
    P = c.zero.ctypes.data
    off, off1, offgap = _hp(OFFSETS), np.array([1, 5, 6, 13], np.int64), np.array([0, 5, 5, 13], np.int64)
    desc = np.array([0, 5, 2, 6], np.int64)
    thr, thr_nan, minc0 = np.array([0.0, 1.0]), np.array([0.0, float("nan")]), np.array([1, 0, 1], np.int32)
    c.keep_der = [off1, offgap, desc, thr, thr_nan, minc0]
    rows = []
    for name, (pfx, order, sweep, timed, jer) in DER_FORMS.items():
        st = dict.fromkeys(order)                 # every pointer NULL ...
        st.update(R=0, Q=0, collar=-1, flags=2, minc=_hp(minc0), mb=P, mc=P, tdur=P, tspk=P, udur=P, uem_off=_hp(off1))
        ladder = []
        if timed:
            ladder += [("turn_off is NULL", "turn_off", _hp(off1)), ("seg_start is NULL", "sstart", P), ("seg_dur is NULL", "sdur", P)]
            ladder += [] if sweep else [("hyp is NULL", "hyp", P)]
            ladder += [("counts is NULL", "counts", P)]
            ladder += [("jer is NULL", "jer", P)] if jer else []
            ladder += [("n_clusters is NULL", "ncl", P)] if sweep else []
        else:
            ladder += [("ref is NULL", "ref", P)]
            ladder += [] if sweep else [("hyp is NULL", "hyp", P)]
            ladder += [("counts is NULL", "counts", P)]
            ladder += [("n_clusters is NULL", "ncl", P)] if sweep else []
            ladder += [("jer is NULL", "jer", P)] if jer else []
        ladder += [("R = 0 (must be >= 1)", "R", 1 << 31), ("R = 2147483648 (at most 2^31 - 1)", "R", R),
                   ("offsets is NULL", "offsets", _hp(off1)), ("offsets[0] = 1 (must be 0)", "offsets", _hp(offgap)),
                   ("recording 1 has 0 segments (must be 1 ... PLDA_AHC_MAX = 4096; offsets must ascend)", "offsets", off)]
        if sweep:
            ladder += [("Q = 0 (must be >= 1)", "Q", 65536), ("Q = 65536 (at most 65535)", "Q", 2), ("thresholds is NULL", "thr", _hp(thr_nan)),
                       ("thresholds[1] is NaN", "thr", _hp(thr)), ("min_clusters[1] = 0 (must be >= 1)", "minc", None)]
        if timed:
            ladder += [("turn_off[0] = 1 (must be 0)", "turn_off", _hp(desc)),
                       ("recording 1 has -3 turns (must be 0 ... PLDA_DER_MAX_TURNS = 16384; turn_off must ascend)", "turn_off", off),
                       ("turn_start, turn_dur or turn_spk is NULL", "tstart", P),
                       ("uem_off[0] = 1 (must be 0)", "uem_off", _hp(desc)),
                       ("recording 1 has -3 UEM intervals (must be 0 ... PLDA_DER_MAX_UEM = 1024; uem_off must ascend)", "uem_off", off),
                       ("uem_start or uem_dur is NULL", "uem_off", None),      # (the UEM arrays without their offsets: udur is still given)
                       ("uem_off is NULL", "udur", None),
                       ("collar = -1 (must be 0 ... 2^20)", "collar", 0),
                       ("flags = 2 (bit 0, PLDA_DER_SKIP_OVERLAP, is the only one)", "flags", 0)]
        if sweep:
            ladder += [("merge_a, merge_b or merge_cost is NULL", "ma", P)]
        fns = [name + "_dev"] if name in ("plda_der", "plda_der_sweep") else [name, name + "_dev"]
        for text, key, mended in ladder:
            assert key in st, (name, key)
            rows += [(fn, c.h, [st[k] for k in order], INVAL, "%s: %s" % (pfx, text)) for fn in fns]
            st[key] = mended
    return rows


def _refusals(c):
    """(entry point, handle, arguments, status, plda_last_error text or None).  Texts are the library's, letter for letter."""
    h, f, P = c.h, c.f, c.zero.ctypes.data
    off, boff = _hp(OFFSETS), _hp(BLOCK_OFF)
    gap = np.array([0, 0, 2, 2, 7, 7], np.uint64)
    badn = np.array([1, 0, -1], np.int32)
    ones = np.ones(4, np.int32)
    eidx, good = np.array([0, 5], np.int64), np.array([0, 1], np.int64)
    boffs = np.array([0, 7, 3], np.int64)
    off1, offgap = np.array([1, 5, 6, 13], np.int64), np.array([0, 5, 5, 13], np.int64)
    minc0 = np.array([1, 0, 1], np.int32)
    bo_short = np.array([0, 25, 25, 75], np.int64)
    fr5, fr23, fr00 = np.array([0, 5], np.int64), np.array([2, 3], np.int64), np.array([0, 0], np.int64)
    gdesc = np.array([10, 8, 4, 0], np.int64)
    thr = np.array([0.0, 1.0, 2.0])
    cap, cap0 = C.c_int64(4), C.c_int64(0)
    c.keep = [gap, badn, ones, eidx, good, boffs, off1, offgap, minc0, bo_short, fr5, fr23, fr00, gdesc, thr, cap, cap0]
    nan = float("nan")
    ahc_ok = [P, P, None, None, None]
    vbx = lambda **k: [k.get("Y", P), k.get("D", D), None, k.get("lin", P), k.get("off", off), k.get("R", R), k.get("Fa", 0.3), 17.0,
                       k.get("lp", 0.9), 5.0, k.get("mi", 3), 1e-4, k.get("labels", P), P, k.get("gamma"), k.get("goff"), None, None, None, None]
    rows = [
        ("plda_fit", h, [None, 6, D, _hp(gap), 2], INVAL, "fit: bad argument"),
        ("plda_fit", f, [P, 6, D, _hp(gap), 2], LABELS, "fit: labels must be dense 0..K-1"),
        ("plda_lda_fit", f, [None, 6, D, _hp(gap), 0, None], INVAL, "lda_fit: bad argument"),
        ("plda_lda_fit", f, [P, 6, D, _hp(gap), 0, None], LABELS, "lda_fit: labels must be dense 0..K-1"),
        ("plda_set_model", f, [0, D, None, P, P], INVAL, "set_model: bad argument"),
        ("plda_lda_set_model", f, [3, 0, D, 1, None, None, None, None, None, None], INVAL, "lda_set_model: bad argument"),
        ("plda_lda_set_model", f, [0, 2, D, 1, None, None, None, None, P, P], INVAL, "lda_set_model: scalings required"),
        ("plda_lda_set_model", f, [0, 2, D, 1, None, None, None, P, P, P], INVAL, "lda_set_model: xbar required for the svd solver"),

        ("plda_transform_rows", f, [None, 3, D, None, 0, None], NOT_FITTED, "transform: model not fitted"),
        ("plda_transform_rows", h, [None, 0, D, None, 0, None], OK, None),
        ("plda_transform_rows", h, [None, 3, D, None, 0, P], INVAL, "transform_rows: bad argument"),
        ("plda_transform_rows", h, [P, 3, D, None, 0, P], INVAL, "transform_rows: need num_examples or n_uniform > 0"),
        ("plda_transform_rows", h, [P, 3, D, _hp(badn), 0, P], INVAL, "transform_rows: 2 of 3 rows have num_examples <= 0 (the first is row 1)"),

        ("plda_transform_groups", f, [None, 4, D, None, None, None, None, None], NOT_FITTED, "transform: model not fitted"),
        ("plda_transform_groups", h, [None, 4, D, None, None, None, None, None], INVAL, "transform_groups: Ku is NULL"),
        ("plda_transform_groups", h, [None, 0, D, None, None, None, None, C.byref(cap)], OK, None),
        ("plda_transform_groups", h, [None, 4, 7, P, P, P, P, C.byref(cap)], INVAL, "transform_groups: bad argument"),
        ("plda_transform_groups", h, [P, 4, 7, P, P, P, P, C.byref(cap0)], INVAL, "transform: feature dim 7 != model dim 20"),
        ("plda_transform_groups", h, [P, 4, D, P, P, P, P, C.byref(cap0)], CAPACITY, "transform_groups: capacity must be > 0"),

        ("plda_score_matrix", f, [None, None, 0, 2, None, 2, None, None, None, 1], NOT_FITTED, "score_matrix: model not fitted"),
        ("plda_score_matrix", h, [None, None, 0, 0, None, 2, None, None, None, 1], OK, None),
        ("plda_score_matrix", h, [None, None, 0, 2, None, 0, None, None, None, 1], OK, None),
        ("plda_score_matrix", h, [None, None, 0, 2, P, 2, None, None, P, 2], INVAL, "score_matrix: bad argument"),
        ("plda_score_matrix", h, [P, None, 0, 2, P, 2, None, None, P, 1], INVAL, "score_matrix: bad argument"),
        ("plda_score_matrix", h, [P, None, 0, 2, P, 2, None, None, P, 2], INVAL, "score_matrix: n_uniform must be > 0 when n_enrol is NULL"),

        ("plda_score_pairs", f, [None, None, 0, None, 0, None, None, 3, None, None, None], NOT_FITTED, "score: model not fitted"),
        ("plda_score_pairs", h, [None, None, 0, None, 0, None, None, 0, None, None, None], OK, None),
        ("plda_score_pairs", h, [None, P, 2, P, 2, P, P, 3, None, None, None], INVAL, "score_pairs: bad argument"),
        ("plda_score_pairs", h, [P, P, 2, P, 2, _hp(eidx), _hp(good), 2, None, None, P], INVAL, "score_pairs: trial 1 indexes outside the enrol/test sets"),
        ("plda_score_pairs", h, [P, P, 2, P, 2, _hp(good), _hp(good), 2, None, None, P], INVAL, "score_pairs: num_examples must be > 0"),

        ("plda_znorm_stats", f, [None, 3, 1, 7, None, 2, None, None], NOT_FITTED, "norm: model not fitted"),
        ("plda_znorm_stats", h, [None, 3, 1, 7, P, 2, P, P], INVAL, "norm: bad argument"),
        ("plda_znorm_stats", h, [P, 3, 1, 7, P, 2, P, P], INVAL, "norm: feature dim 7 != model dim 20"),

        ("plda_cohort_stats", f, [None, None, 0, 0, None, 0, 1, None, None], NOT_FITTED, "cohort_stats: model not fitted"),
        ("plda_cohort_stats", h, [None, None, 0, 0, None, 0, 1, None, None], INVAL, "cohort_stats: R = 0, Nc = 0 (both must be >= 1)"),
        ("plda_cohort_stats", h, [None, None, 0, 3, P, 4, 5, P, P], INVAL, "cohort_stats: top_k = 5 (must be in 1 ... Nc = 4)"),
        ("plda_cohort_stats", h, [P, None, 0, 3, None, 4, 2, P, P], INVAL, "cohort_stats: cohort is NULL"),
        ("plda_cohort_stats", h, [P, None, 0, 3, P, 4, 2, P, None], INVAL, "cohort_stats: std is NULL"),
        ("plda_cohort_stats", h, [P, None, 0, 3, P, 4, 2, P, P], INVAL, "cohort_stats: n_uniform must be > 0 when n is NULL"),

        ("plda_score_matrix_snorm", f, [None, None, 0, 0, None, 0, P, None, None, None, None, 0], NOT_FITTED, "score_matrix_snorm: model not fitted"),
        ("plda_score_matrix_snorm", h, [None, None, 0, 0, None, 0, P, None, None, None, None, 0], INVAL, "score_matrix_snorm: estd is NULL but its partner is not"),
        ("plda_score_matrix_snorm", h, [None, None, 0, 0, None, 0, None, None, None, P, None, 0], INVAL, "score_matrix_snorm: tmean is NULL but its partner is not"),
        ("plda_score_matrix_snorm", h, [None, None, 0, 0, None, 0, None, None, None, None, None, 0], INVAL,
         "score_matrix_snorm: both statistic pairs are NULL (emean/estd or tmean/tstd must be given)"),
        ("plda_score_matrix_snorm", h, [None, None, 0, 0, None, 2, P, P, None, None, None, 0], INVAL, "score_matrix_snorm: M = 0, Nt = 2 (both must be >= 1)"),
        ("plda_score_matrix_snorm", h, [P, None, 0, 2, None, 2, P, P, None, None, None, 0], INVAL, "score_matrix_snorm: V is NULL"),
        ("plda_score_matrix_snorm", h, [P, None, 0, 2, P, 2, P, P, None, None, P, 1], INVAL, "score_matrix_snorm: ld_out = 1 < Nt = 2"),
        ("plda_score_matrix_snorm", h, [P, None, 0, 2, P, 2, P, P, None, None, P, 2], INVAL, "score_matrix_snorm: n_uniform must be > 0 when n_enrol is NULL"),

        ("plda_score_topn", f, [None, None, 0, 0, None, 0, None, None, None, None, None, None, 5, 0, None, None], NOT_FITTED, "score_topn: model not fitted"),
        ("plda_score_topn", h, [None, None, 0, 0, None, 0, None, None, None, None, None, None, 5, 0, None, None], INVAL, "score_topn: M = 0, Nt = 0 (both must be >= 1)"),
        ("plda_score_topn", h, [None, None, 0, 2, None, 2, None, None, None, None, None, None, 5, 0, None, None], INVAL,
         "score_topn: axis = 5 (must be 0: per row, or 1: per column)"),
        ("plda_score_topn", h, [None, None, 0, 2, None, 2, None, None, None, None, None, None, 0, 257, None, None], INVAL, "score_topn: top_n = 257 (must be in 1 ... 256)"),
        ("plda_score_topn", h, [P, None, 0, 2, P, 2, P, None, None, None, None, None, 0, 2, None, None], INVAL, "score_topn: out_scores is NULL"),
        ("plda_score_topn", h, [P, None, 0, 2, P, 2, P, None, None, P, None, None, 0, 2, P, P], INVAL, "score_topn: zstd is NULL but its partner is not"),
        ("plda_score_topn", h, [P, None, 0, 2, P, 2, None, None, None, P, P, None, 0, 2, P, P], INVAL, "score_topn: emean is NULL but its partner is not"),
        ("plda_score_topn", h, [P, None, 0, 2, P, 2, None, None, None, None, P, None, 0, 2, P, P], INVAL, "score_topn: tstd is NULL but its partner is not"),
        ("plda_score_topn", h, [P, None, 0, 2, P, 2, None, None, None, None, None, None, 0, 2, P, P], INVAL, "score_topn: n_uniform must be > 0 when n_enrol is NULL"),

        ("plda_dvector_pool", h, [None, 0, -1, 0, None, 0, 0, 0, None], OK, None),
        ("plda_dvector_pool", h, [None, 0, 5, 4, _hp(boffs), 2, 0, 0, P], INVAL, "dvector_pool: bad argument"),
        ("plda_dvector_pool", h, [P, 2, 5, 4, _hp(boffs), 2, 0, 0, P], INVAL, "dvector_pool: bad argument"),
        ("plda_dvector_pool", h, [P, 1, 5, 4, _hp(boffs), 2, 0, 0, P], INVAL, "dvector_pool: offsets must be non-decreasing within [0, T]"),

        ("plda_lda_predict", f, [None, 3, 7, 0, None], NOT_FITTED, "This LDA instance is not fitted yet"),
        ("plda_lda_predict", h, [None, 3, 7, 0, None], INVAL, "X has 7 features per sample; expecting 20"),
        ("plda_lda_predict", h, [None, 0, D, 0, None], OK, None),
        ("plda_lda_predict", h, [None, 3, D, 0, P], INVAL, "lda_predict: bad argument"),
        ("plda_lda_transform", f, [None, 3, 7, 2, None], NOT_FITTED, "This LDA instance is not fitted yet"),
        ("plda_lda_transform", h, [None, 3, 7, 2, None], INVAL, "X has 7 features per sample; expecting 20"),
        ("plda_lda_transform", h, [None, 3, D, 0, None], OK, None),
        ("plda_lda_transform", h, [None, 0, D, 2, None], OK, None),
        ("plda_lda_transform", h, [None, 3, D, 2, P], INVAL, "lda_transform: bad argument"),

        ("plda_htk_frames", h, [None, -1, None, None, 0, 6, -1, None], OK, None),
        ("plda_htk_frames", h, [None, -1, P, P, 1, 6, 0, P], INVAL, "htk_frames: bad argument"),
        ("plda_htk_frames", h, [P, 16, P, _hp(fr5), 1, 6, 0, P], INVAL, "htk_frames: samplesize 6 is not a multiple of 4"),
        ("plda_htk_frames", h, [P, 16, P, _hp(fr5), 1, 16, 0, P], INVAL, "htk_frames: file 0 does not fit the blob (pad short files with zeros)"),
        ("plda_htk_frames", h, [P, 1000, P, _hp(fr23), 1, 16, 0, P], INVAL, "htk_frames: frame_off[0] must be 0"),
        ("plda_htk_frames", h, [P, 1000, P, _hp(fr00), 1, 16, 0, P], OK, None),

        ("plda_ahc_matrix", h, [None, None, None, 0, 0, 0.0, None, None, None, None, None, None], INVAL, "ahc_matrix: scores is NULL"),
        ("plda_ahc_matrix", h, [P, boff, None, 0, 0, 0.0, None] + ahc_ok, INVAL, "ahc_matrix: R = 0 (must be >= 1)"),
        ("plda_ahc_matrix", h, [P, boff, None, R, 0, 0.0, None, None, None, None, None, None], INVAL, "ahc_matrix: offsets is NULL"),
        ("plda_ahc_matrix", h, [P, boff, off, R, 0, 0.0, None, None, None, P, None, None], INVAL, "ahc_matrix: labels is NULL"),
        ("plda_ahc_matrix", h, [P, boff, off, R, 0, 0.0, None, P, None, P, None, None], INVAL, "ahc_matrix: n_clusters is NULL"),
        ("plda_ahc_matrix", h, [P, boff, off, R, 1, nan, None, P, P, P, None, None], INVAL,
         "ahc_matrix: merge_a, merge_b and merge_cost must be given together or not at all"),
        ("plda_ahc_matrix", h, [P, boff, _hp(off1), R, 1, nan, None] + ahc_ok, INVAL, "ahc_matrix: threshold is NaN"),
        ("plda_ahc_matrix", h, [P, None, _hp(off1), R, 0, 0.0, None] + ahc_ok, INVAL, "ahc_matrix: offsets[0] = 1 (must be 0)"),
        ("plda_ahc_matrix", h, [P, None, _hp(offgap), R, 0, 0.0, None] + ahc_ok, INVAL,
         "ahc_matrix: recording 1 has 0 segments (must be 1 ... PLDA_AHC_MAX = 4096; offsets must ascend)"),
        ("plda_ahc_matrix", h, [P, None, off, R, 0, 0.0, _hp(minc0)] + ahc_ok, INVAL, "ahc_matrix: min_clusters[1] = 0 (must be >= 1)"),
        ("plda_ahc_matrix", h, [P, None, off, R, 0, 0.0, None] + ahc_ok, INVAL, "ahc_matrix: block_off is NULL"),
        ("plda_ahc_matrix", h, [P, _hp(bo_short), off, R, 0, 0.0, None] + ahc_ok, INVAL, "ahc_matrix: block 1 holds 0 floats, its recording needs 1 x 1"),

        ("plda_score_ahc", f, [None, None, 0, 0, 0.0, None, None, None, None, None, None], NOT_FITTED, "score_ahc: model not fitted"),
        ("plda_score_ahc", h, [None, None, 0, 0, 0.0, None, None, None, None, None, None], INVAL, "score_ahc: X is NULL"),
        ("plda_score_ahc", h, [P, None, 0, 0, 0.0, None, None, None, None, None, None], INVAL, "score_ahc: R = 0 (must be >= 1)"),
        ("plda_score_ahc", h, [P, None, R, 0, 0.0, None, None, None, None, None, None], INVAL, "score_ahc: offsets is NULL"),
        ("plda_score_ahc", h, [P, off, R, 0, 0.0, _hp(minc0), None, P, None, None, None], INVAL, "score_ahc: labels is NULL"),
        ("plda_score_ahc", h, [P, off, R, 0, 0.0, _hp(minc0)] + ahc_ok, INVAL, "score_ahc: min_clusters[1] = 0 (must be >= 1)"),

        ("plda_score_dense_pca", f, [None, None, 0, 1.5, None, None, None, None], NOT_FITTED, "score_dense_pca: model not fitted"),
        ("plda_score_dense_pca", h, [None, None, 0, 1.5, None, None, None, None], INVAL, "score_dense_pca: target_energy = 1.5 (must lie in (0, 1))"),
        ("plda_score_dense_pca", h, [None, None, 0, 0.9, None, None, None, None], INVAL, "score_dense_pca: R = 0 (must be 1 ... 2^31 - 1)"),
        ("plda_score_dense_pca", h, [None, None, R, 0.9, None, None, None, None], INVAL, "score_dense_pca: offsets is NULL"),
        ("plda_score_dense_pca", h, [None, _hp(off1), R, 0.9, None, None, None, None], INVAL, "score_dense_pca: offsets[0] = 1 (must be 0)"),
        ("plda_score_dense_pca", h, [None, off, R, 0.9, None, None, None, None], INVAL, "score_dense_pca: block_off is NULL"),
        ("plda_score_dense_pca", h, [None, off, R, 0.9, None, _hp(bo_short), None, None], INVAL,
         "score_dense_pca: block 1 holds 0 floats, its recording needs 1 x 1"),
        ("plda_score_dense_pca", h, [None, off, R, 0.9, None, boff, None, None], INVAL, "score_dense_pca: X is NULL"),
        ("plda_score_dense_pca", h, [P, off, R, 0.9, None, boff, None, None], INVAL, "score_dense_pca: scores is NULL"),

        ("plda_score_dense_pca_ahc", f, [None, None, 0, 0.0, 0, 0.0, None, None, None, None, None, None], NOT_FITTED, "score_dense_pca_ahc: model not fitted"),
        ("plda_score_dense_pca_ahc", h, [None, off, R, 0.0, 0, 0.0, None, None, None, None, None, None], INVAL,
         "score_dense_pca_ahc: target_energy = 0 (must lie in (0, 1))"),
        ("plda_score_dense_pca_ahc", h, [None, off, R, 0.9, 0, 0.0, None, None, None, None, None, None], INVAL, "score_dense_pca_ahc: X is NULL"),
        ("plda_score_dense_pca_ahc", h, [P, off, R, 0.9, 0, 0.0, None, None, None, None, None, None], INVAL, "score_dense_pca_ahc: labels is NULL"),
        ("plda_score_dense_pca_ahc", h, [P, off, R, 0.9, 1, nan, None] + ahc_ok, INVAL, "score_dense_pca_ahc: threshold is NaN"),

        ("plda_der", h, [None, None, None, None, 0, None, None], INVAL, "der: ref is NULL"),
        ("plda_der", h, [P, None, None, None, 0, None, None], INVAL, "der: hyp is NULL"),
        ("plda_der", h, [P, P, None, None, 0, None, None], INVAL, "der: counts is NULL"),
        ("plda_der", h, [P, P, None, None, 0, P, None], INVAL, "der: R = 0 (must be >= 1)"),
        ("plda_der", h, [P, P, None, None, R, P, None], INVAL, "der: offsets is NULL"),
        ("plda_der", h, [P, P, None, _hp(offgap), R, P, None], INVAL,
         "der: recording 1 has 0 segments (must be 1 ... PLDA_AHC_MAX = 4096; offsets must ascend)"),

        ("plda_der_sweep", h, [None, None, None, None, 0, None, None, None, 0, None, None, None], INVAL, "der_sweep: ref is NULL"),
        ("plda_der_sweep", h, [None, None, None, None, 0, P, None, None, 0, None, None, None], INVAL, "der_sweep: counts is NULL"),
        ("plda_der_sweep", h, [None, None, None, None, 0, P, None, None, 0, None, P, None], INVAL, "der_sweep: n_clusters is NULL"),
        ("plda_der_sweep", h, [None, None, None, None, 0, P, None, None, 0, None, P, P], INVAL, "der_sweep: R = 0 (must be >= 1)"),
        ("plda_der_sweep", h, [None, None, None, off, R, P, None, None, 0, None, P, P], INVAL, "der_sweep: Q = 0 (must be >= 1)"),
        ("plda_der_sweep", h, [None, None, None, off, R, P, None, None, Q, None, P, P], INVAL, "der_sweep: thresholds is NULL"),
        ("plda_der_sweep", h, [None, None, None, off, R, P, None, _hp(thr), Q, _hp(minc0), P, P], INVAL, "der_sweep: min_clusters[1] = 0 (must be >= 1)"),
        ("plda_der_sweep", h, [P, P, None, off, R, P, None, _hp(thr), Q, None, P, P], INVAL, "der_sweep: merge_a, merge_b or merge_cost is NULL"),

    ] + _der_refusals(c) + [
        ("plda_vbx", f, vbx(Y=None, R=0), NOT_FITTED, "vbx: model not fitted"),
        ("plda_vbx", h, vbx(Y=None, lin=None), INVAL, "vbx: Y is NULL"),
        ("plda_vbx", h, vbx(lin=None, R=0), INVAL, "vbx: labels_in is NULL"),
        ("plda_vbx", h, vbx(R=0, D=0), INVAL, "vbx: R = 0 (must be 1 ... 2^31 - 1)"),
        ("plda_vbx", h, vbx(D=0, off=None), INVAL, "vbx: D = 0 (must be 1 ... 4096)"),
        ("plda_vbx", h, vbx(off=None, labels=None), INVAL, "vbx: offsets is NULL"),
        ("plda_vbx", h, vbx(labels=None, Fa=0.0), INVAL, "vbx: labels is NULL"),
        ("plda_vbx", h, vbx(Fa=0.0, lp=1.0), INVAL, "vbx: Fa = 0 (must be > 0)"),
        ("plda_vbx", h, vbx(lp=1.0, mi=0), INVAL, "vbx: loop_prob = 1 (must be in [0, 1))"),
        ("plda_vbx", h, vbx(mi=0, gamma=P), INVAL, "vbx: max_iters = 0 (must be >= 1)"),
        ("plda_vbx", h, vbx(gamma=P, off=_hp(off1)), INVAL, "vbx: gamma and gamma_off must be given together"),
        ("plda_vbx", h, vbx(off=_hp(off1)), INVAL, "vbx: offsets[0] = 1 (must be 0)"),
        ("plda_vbx", h, vbx(gamma=P, goff=_hp(gdesc)), INVAL, "vbx: gamma_off / pi_off must ascend"),

        ("plda_project_rows", f, [None, -1, 7, None], NOT_FITTED, "project_rows: model not fitted"),
        ("plda_project_rows", h, [None, -1, 7, None], INVAL, "project_rows: feature dim 7 != model dim 20"),
        ("plda_project_rows", h, [None, -1, D, None], INVAL, "project_rows: R = -1"),
        ("plda_project_rows", h, [None, 0, D, None], OK, None),
        ("plda_project_rows", h, [None, 3, D, P], INVAL, "project_rows: bad argument"),

        ("plda_embed_apply", f, [None, 2, 3, 7, None], NOT_FITTED, "embed_apply: no embedding chain is set"),
        ("plda_embed_apply", h, [None, 2, 3, 7, None], INVAL, "embed_apply: dtype 2 (0 fp64, 1 fp32)"),
        ("plda_embed_apply", h, [None, 0, 3, 7, None], INVAL, "embed_apply: feature dim 7 != the chain's input dim 20"),
        ("plda_embed_apply", h, [None, 0, 0, D, None], OK, None),
        ("plda_embed_apply", h, [None, 0, 3, D, P], INVAL, "embed_apply: bad argument"),

        ("plda_embed_fit", h, [None, 2, 6, D, _hp(gap), 2, D, 1.0, 1.0, None], LABELS, "embed_fit: labels must be dense 0..K-1"),
        ("plda_embed_fit", h, [None, 2, 10, D, None, 0, D, 1.0, 1.0, None], INVAL, "embed_fit: dtype 2 (0 fp64, 1 fp32)"),
        ("plda_embed_fit", h, [None, 0, 10, D, None, 3, D, 1.0, 1.0, None], INVAL, "embed_fit: kind 3 (0 centre, 1 whiten, 2 lda)"),
        ("plda_embed_fit", h, [None, 0, 10, D, None, 2, D, 1.0, 1.0, None], INVAL, "embed_fit: kind 2 (lda) needs labels"),
        ("plda_embed_fit", h, [None, 0, 10, D, None, 0, D, 1.0, 1.0, None], INVAL, "embed_fit: X is NULL"),

        ("plda_gemm_f64", h, [0, 2, 2, 1.0, None, 0, P, 0, None, 0.0, P, 1], INVAL, "gemm_f64: bad argument"),
        ("plda_gemm_f64", h, [2, 2, 2, 1.0, P, 0, P, 0, P, 0.0, P, 2], INVAL, "gemm_f64: bad argument"),
        ("plda_spd_inverse", h, [None, 2049, None], INVAL, "spd_inverse: bad argument"),
        ("plda_sym_eig", h, [None, 4, 3, P, P, None], INVAL, "sym_eig: bad argument"),
        ("plda_sym_eig", h, [P, 1025, 3, P, P, None], INVAL, "sym_eig: method must be 0 (default), 1 (Jacobi) or 2 (direct)"),
        ("plda_sym_eig", h, [P, 1025, 1, P, P, None], INVAL, "sym_eig: the block Jacobi solver (method 1) stops at D = 1024; D = 1025 needs method 0 or 2"),

        ("plda_eer_lists", h, [None, 0, P, 4, None], INVAL, "eer: need at least one target and one impostor score"),
        ("plda_det_lists", h, [P, 4, P, 4, 8, None, P, P], INVAL, "det: need at least one target and one impostor score"),
        ("plda_min_dcf_lists", h, [P, 4, P, 0, 1, P, None, None], INVAL, "min_dcf: need at least one target and one non-target score"),
        ("plda_calib_pass_lists", h, [P, 0, None, 4, 1.0, 0.0, 0.0, None], INVAL, "calib_pass: need at least one target and one non-target score"),
        ("plda_calib_fit_lists", h, [P, 4, None, 0, 0.5, 1e-6, 10, None], INVAL, "calib_fit: need at least one target and one non-target score"),
        ("plda_fusion_pass_lists", h, [99, None, 0, None, 0, None, 0.0, 0.0, P], INVAL, "plda_fusion_pass_lists: the output structure or the weight array is NULL"),
        ("plda_fusion_fit_lists", h, [99, None, 0, None, 0, 0.5, 1e-6, 10, None], INVAL, "plda_fusion_fit_lists: the output structure or the weight array is NULL"),
    ]
    return rows


def test_refusals_status_text_and_order(ctx):
    lib, N = ctx.lib, ctx.N
    rows = _refusals(ctx)
    seen = set()
    for fn, h, args, status, text in rows:
        if fn not in seen:      # a NULL handle, whatever else is wrong with the call
            seen.add(fn)
            assert getattr(lib, fn)(None, *args) == INVAL, fn
        held = lib.plda_device_bytes_held()
        before = N.last_error(h)
        rc = getattr(lib, fn)(h, *args)
        got = N.last_error(h)
        assert rc == status, "%s%r: status %d (%s), expected %d (%s)" % (fn, args, rc, got, status, text)
        assert got == (before if text is None else text), "%s%r" % (fn, args)
        assert lib.plda_device_bytes_held() == held, "%s%r left device memory behind" % (fn, args)
    host_forms = {"plda_fit", "plda_lda_fit", "plda_transform_rows", "plda_transform_groups", "plda_score_matrix", "plda_score_pairs",
                  "plda_znorm_stats", "plda_cohort_stats", "plda_score_matrix_snorm", "plda_score_topn", "plda_dvector_pool",
                  "plda_lda_predict", "plda_lda_transform", "plda_htk_frames", "plda_ahc_matrix", "plda_score_ahc", "plda_score_dense_pca",
                  "plda_score_dense_pca_ahc", "plda_der", "plda_der_sweep", "plda_vbx", "plda_project_rows", "plda_embed_apply",
                  "plda_embed_fit", "plda_gemm_f64", "plda_spd_inverse", "plda_sym_eig", "plda_eer_lists", "plda_det_lists",
                  "plda_min_dcf_lists", "plda_calib_pass_lists", "plda_calib_fit_lists", "plda_fusion_pass_lists", "plda_fusion_fit_lists"}
    host_forms |= set(DER_FORMS)
    assert host_forms <= seen and {fn + "_dev" for fn in DER_FORMS} <= seen
    assert ctx.eng.dims() == (D, D)     # the handles still work
    assert lib.plda_adapt_accumulate(None, None, 0, D, None) == INVAL


def test_silent_refusals_keep_the_error_text(ctx):
    lib, N, h = ctx.lib, ctx.N, ctx.h
    assert lib.plda_project_rows(h, None, 3, D, None) == INVAL
    text = N.last_error(h)
    assert text == "project_rows: bad argument"
    assert lib.plda_fit_timings(h, None) == INVAL and N.last_error(h) == text
    assert lib.plda_fit_plan(h, None) == INVAL and N.last_error(h) == text
    assert lib.plda_fit_num_classes(h, None) == INVAL and N.last_error(h) == text
    for fn in ("plda_fit_timings", "plda_fit_plan", "plda_fit_num_classes"):
        assert getattr(lib, fn)(None, None) == INVAL
    ms = (C.c_double * 4)()
    assert lib.plda_fit_timings(h, C.addressof(ms)) == OK and N.last_error(h) == text


@pytest.mark.parametrize("name,value,text", [
    ("PLDA_SCORE_DTYPE", "f16", "plda_create: PLDA_SCORE_DTYPE=f16 (f32 or bf16x3)"),
    ("PLDA_EMBED_CUS", "5000", "plda_create: PLDA_EMBED_CUS=5000 (a whole number 1 ... 4096; 0 or empty: the device's count)"),
    ("PLDA_EMBED_VARIANT", "2", "plda_create: PLDA_EMBED_VARIANT=2 (0: by shape, 1: row pass + GEMM + row pass always)"),
])
def test_create_refuses_bad_settings(ctx, monkeypatch, name, value, text):
    lib = ctx.lib
    held = lib.plda_device_bytes_held()
    monkeypatch.setenv(name, value)
    h = C.c_void_p()
    assert lib.plda_create(0, C.byref(h)) == INVAL and not h.value
    assert lib.plda_last_error(None).decode() == text
    monkeypatch.delenv(name)
    from plda_amd import MPlda
    eng = MPlda(0)
    assert lib.plda_fit_timings(eng._h, None) == INVAL
    del eng
    assert lib.plda_device_bytes_held() == held
