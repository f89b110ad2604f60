"""GPU: quality-aware calibration -- side-information terms in the fusion (csrc/fusion.hip; include/plda_hip.h
"quality-aware calibration"), every call through the C ABI.

THE CONTRACT under test: a side pass, fit or map is BIT-IDENTICAL to the existing plda_fusion_pass_matrices_dev /
_fit_matrices_dev / _map_dev over K + Q matrices in which every side has been materialised with its fp32 operation
(tests/fusion_side_model.py), at any pitch or alignment of the materialised matrices.

  1. the pass: all 1024 bytes of the record against the matrix pass on materialised sides, for all 28 (K, Q) with K, Q >= 1 on
     37 x 1023 and for (1,1) (1,3) (1,7) (2,1) (2,3) (4,1) (4,4) (7,1) -- both sides of the rows-in-flight classes T <= 2, <= 4,
     > 4 -- on the other shapes (one row, one column, ragged strips, several strips, 5 rows per workgroup); every op; the
     matrices misaligned none / one / all; side vectors at a base offset of 0 and 1 float; three label layouts; theta between
     two chain values.  And independently of the matrix kernel: tests/fusion_model.py on the materialised arrays within the
     fusion's band (1e-12 of sum|term|, integers equal);
  2. the map against plda_fusion_map_dev on materialised sides and against the exact chain; in place; guard columns;
  3. the fit on the planted case: the plda_fusion_fit bytes, and Cllr below the score's own;
  4. the operand form against the matrix form on plda_score_matrix_dev's output, across slab boundaries;
  5. refusals by name; Q = 0 is the existing path;
  6. poisoned scratch, a long-lived handle, create / calibrate_quality / destroy;
  7. liblda.PLDA.calibrate_quality / score_matrix_fused(quality=...) end to end.

Run with -s to see the measured figures next to each bound.  Nothing here provokes a fault."""
import ctypes as C
import gc
import warnings

import numpy as np
import pytest

import fusion_model as fm
import fusion_side_model as sm
import test_gpu_fusion as tgf
from test_gpu_fusion import Placed, _dev, _t

pytestmark = pytest.mark.gpu

OPS = sm.OPS
vp = lambda arr: C.c_void_p(arr.ctypes.data)                                        # noqa: E731


def _engine(monkeypatch, poison=False, slab=None, model_d=None):
    from plda_amd import MPlda
    env = tgf.ENV + ("PLDA_EER_SLAB_ROWS",)
    for name in env:
        monkeypatch.delenv(name, raising=False)
    if poison:
        monkeypatch.setenv("PLDA_SCRATCH_POISON", "1")
    if slab:
        monkeypatch.setenv("PLDA_EER_SLAB_ROWS", str(slab))
    eng = MPlda(0)
    for name in env:
        monkeypatch.delenv(name, raising=False)
    if model_d:
        rng = np.random.default_rng(model_d)
        q, _ = np.linalg.qr(rng.standard_normal((model_d, model_d)))
        eng.set_model(rng.random(model_d), q * (1.0 + rng.random(model_d))[:, None], np.sort(0.05 + rng.random(model_d) * 4.0)[::-1].copy())
    return eng


class Sides(object):
    """Q sides: host vectors (log-durations and the like, some negative), their device copies at a base offset of `off`
    floats between guard floats, the `plda_amd.fusion.Side`s over them and the materialised fp32 matrices."""
    G = 16

    def __init__(self, rng, m, nt, ops, off):
        from plda_amd import fusion as FU
        self.ops, self.host, self.bufs, self.sides = list(ops), [], [], []
        for op in ops:
            e = (np.log(rng.uniform(2, 40, m)) - 1.0).astype(np.float32)
            t = (np.log(rng.uniform(2, 40, nt)) - 1.0).astype(np.float32)
            self.add(FU, op, e, t, off)
        self.mats = sm.materialise([(op, e, t) for op, (e, t) in zip(self.ops, self.host)], m, nt)

    def add(self, FU, op, e, t, off):
        pair = []
        for v in (e, t):
            flat = np.full(self.G + off + v.shape[0] + self.G, Placed.SENTINEL, np.float32)
            flat[self.G + off:self.G + off + v.shape[0]] = v
            d = _t(flat)
            assert d.data_ptr() % 16 == 0
            self.bufs.append((d, flat))
            pair.append(d[self.G + off:self.G + off + v.shape[0]])
        self.host.append((e, t))
        self.sides.append(FU.Side(op, pair[0], pair[1]))

    def unchanged(self):
        return all(np.array_equal(d.cpu().numpy().view(np.int32), h.view(np.int32)) for d, h in self.bufs)


def _raw_side_pass(eng, ptrs, lds, sides, m, nt, des, dts, a, c, theta):
    from plda_amd import fusion as FU
    k, p, l = FU._matrix_args(ptrs, lds)
    q, sraw, keep = FU._side_args(sides, m, nt)
    a = np.ascontiguousarray(a, np.float64)
    assert a.shape == (k + q,)
    raw = np.zeros(1, FU.RECORD_DTYPE)
    rc = eng._lib.plda_fusion_side_pass_dev(eng._h, k, vp(p), vp(l), q, vp(sraw), m, nt, C.c_void_p(des.data_ptr()),
                                            C.c_void_p(dts.data_ptr()), vp(a), float(c), float(theta), vp(raw))
    del keep
    return rc, raw


def _raw_matrix_pass(eng, ptrs, lds, m, nt, des, dts, a, c, theta):
    from plda_amd import fusion as FU
    k, p, l = FU._matrix_args(ptrs, lds)
    a = np.ascontiguousarray(a, np.float64)
    raw = np.zeros(1, FU.RECORD_DTYPE)
    rc = eng._lib.plda_fusion_pass_matrices_dev(eng._h, k, vp(p), vp(l), m, nt, C.c_void_p(des.data_ptr()), C.c_void_p(dts.data_ptr()),
                                                vp(a), float(c), float(theta), vp(raw))
    return rc, raw


def _weights(rng, t):
    return np.round(rng.uniform(0.1, 0.5, t) * np.where(np.arange(t) % 2, -1.0, 1.0), 6), 0.125


# ------------------------------------------------------------------------------------------- 1. the pass record
ALL_PAIRS = [(k, q) for k in range(1, 8) for q in range(1, 9 - k)]
SAMPLE = [(1, 1), (1, 3), (1, 7), (2, 1), (2, 3), (4, 1), (4, 4), (7, 1)]
OTHER_SHAPES = [(300, 500), (1, 2000), (700, 1), (5, 4099), (513, 1025), (17001, 130)]     # 17001 x 130: 5 rows per workgroup
assert len(ALL_PAIRS) == 28
PASS_CASES = [(37, 1023, k, q, i) for i, (k, q) in enumerate(ALL_PAIRS)]
PASS_CASES += [(m, nt, k, q, 3 * j + i) for j, (m, nt) in enumerate(OTHER_SHAPES) for i, (k, q) in enumerate(SAMPLE)]


def _pass_case(m, nt, k, q, i):
    """what rotates with the case index: the ops (every op appears in every Q >= 5 case and across the Q = 1 cases), the
    placement of the matrices, the side vectors' base offset, the label layout"""
    ops = [OPS[(i + j) % 5] for j in range(q)]
    return ops, ("none", "one", "all")[i % 3], (i // 3) % 2, ("random", "sparse", "blocks")[(i + i // 3) % 3]


def test_the_pass_cases_cover_what_they_claim():
    seen_ops, seen = set(), set()
    for m, nt, k, q, i in PASS_CASES:
        ops, mode, off, layout = _pass_case(m, nt, k, q, i)
        seen_ops.update(ops)
        seen.add((mode, off, layout))
    assert seen_ops == set(OPS)
    assert {s[0] for s in seen} == {"none", "one", "all"} and {s[1] for s in seen} == {0, 1} and {s[2] for s in seen} == {"random", "sparse", "blocks"}
    assert {(k, q) for m, nt, k, q, i in PASS_CASES if (m, nt) == (37, 1023)} == set(ALL_PAIRS)
    assert -(-17001 // min(17001, 4096)) == 5                               # rows per workgroup of the tall shape


@pytest.mark.parametrize("m,nt,k,q,i", PASS_CASES)
def test_side_pass_is_the_matrix_pass_on_materialised_sides(monkeypatch, m, nt, k, q, i):
    from plda_amd import fusion as FU
    ops, mode, off, layout = _pass_case(m, nt, k, q, i)
    eng = _engine(monkeypatch)
    rng = np.random.default_rng(m * 7919 + nt * 31 + k * 9 + q)
    es, ts = tgf._labels(rng, m, nt, layout)
    if m > 10000 and layout == "sparse":
        es[::97] = ts[3]
    tgt = es[:, None] == ts[None, :]
    S = tgf._systems(rng, m, nt, k, tgt)
    sd = Sides(rng, m, nt, ops, off)
    feats = S + sd.mats
    lds, offs = tgf._placement(k + q, nt, mode)
    P = Placed(feats, lds, offs)                                          # the K systems AND the materialised sides
    des, dts = _t(es), _t(ts)
    a, c = _weights(rng, k + q)
    theta = tgf._theta(feats, a, c)
    rc_m, mat = _raw_matrix_pass(eng, P.ptrs, P.lds, m, nt, des, dts, a, c, theta)
    rc_s, side = _raw_side_pass(eng, P.ptrs[:k], P.lds[:k], sd.sides, m, nt, des, dts, a, c, theta)
    assert rc_m == 0 and rc_s == 0, eng._lib.plda_last_error(eng._h)
    assert side.tobytes() == mat.tobytes(), [n for n in FU.RECORD_DTYPE.names if side[n].tobytes() != mat[n].tobytes()]
    assert _raw_side_pass(eng, P.ptrs[:k], P.lds[:k], sd.sides, m, nt, des, dts, a, c, theta)[1].tobytes() == side.tobytes()
    got = FU._record(side)
    assert got["K"] == k + q and got["Np"] == int(tgt.sum()) and got["Np"] + got["Nn"] == m * nt
    # independently of the matrix kernel: the host model on the materialised arrays
    tgf._compare("%dx%d K %d Q %d %s %s off %d %s" % (m, nt, k, q, ops, mode, off, layout), got, fm.pass_matrices(feats, es, ts, a, c, theta))
    for j, mat_j in enumerate(sd.mats):
        assert got["smin"][k + j] == mat_j.min() and got["smax"][k + j] == mat_j.max()
    # the wrapper gives the same record
    tgf._same_bits(FU.pass_with_sides_dev(eng, P.ptrs[:k], P.lds[:k], sd.sides, m, nt, des.data_ptr(), dts.data_ptr(), a, c, theta), got)
    assert P.unchanged() and sd.unchanged()


# ------------------------------------------------------------------------------------------- 2. the map
@pytest.mark.parametrize("m,nt,k,q,mode,off,ld_out,off_out", [(37, 500, 1, 2, "none", 0, 500, 0), (19, 1023, 3, 5, "all", 1, 1030, 1),
                                                              (1, 5, 2, 1, "none", 1, 8, 0), (33, 515, 1, 7, "one", 0, 516, 0),
                                                              (40, 2050, 4, 4, "one", 1, 2052, 0), (300, 1, 7, 1, "all", 0, 1, 0)])
def test_side_map_is_the_matrix_map_and_the_exact_chain(monkeypatch, m, nt, k, q, mode, off, ld_out, off_out):
    import torch
    from plda_amd import fusion as FU
    eng = _engine(monkeypatch)
    rng = np.random.default_rng(m + nt + 10 * k + q)
    S = [(rng.standard_normal((m, nt)) * 10.0 ** rng.integers(-1, 3)).astype(np.float32) for _ in range(k)]
    ops = [OPS[(m + j) % 5] for j in range(q)]
    sd = Sides(rng, m, nt, ops, off)
    feats = S + sd.mats
    lds, offs = tgf._placement(k + q, nt, mode)
    P = Placed(feats, lds, offs)
    fus = FU.QualityFusion(rng.standard_normal(k + q) * [0.0371234567891234, 1.7, 0.3, 1.0, 2.0, 0.01, 0.5, 1.1][:k + q], -1.23456789012345, ops)
    exp = fm.map_exact([f.ravel() for f in feats], fus.a, fus.b).reshape(m, nt)
    G = 4096
    outs = []
    for sided in (False, True):
        dO = torch.full((G + off_out + m * ld_out + G,), float(P.SENTINEL), dtype=torch.float32, device=_dev())
        if sided:
            FU.apply_with_sides_dev(eng, P.ptrs[:k], P.lds[:k], sd.sides, m, nt, fus, dO.data_ptr() + 4 * (G + off_out), ld_out)
        else:
            FU.apply_dev(eng, P.ptrs, P.lds, m, nt, FU.Fusion(fus.a, fus.b), dO.data_ptr() + 4 * (G + off_out), ld_out)
        eng.synchronize()
        O = dO.cpu().numpy()
        body = O[G + off_out:G + off_out + m * ld_out].reshape(m, ld_out)
        # the guard band: nothing before, nothing after, nothing right of column Nt
        assert (O[:G + off_out] == P.SENTINEL).all() and (O[G + off_out + m * ld_out:] == P.SENTINEL).all() and (body[:, nt:] == P.SENTINEL).all()
        outs.append(np.ascontiguousarray(body[:, :nt]).view(np.int32))
    assert np.array_equal(outs[1], outs[0])                                # the matrix map on materialised sides
    assert np.array_equal(outs[1], exp.view(np.int32))                     # the exact chain, rounded once
    assert P.unchanged() and sd.unchanged()
    # in place over system k - 1: the same bits, its columns beyond Nt and its guards untouched, everything else unchanged
    j = k - 1
    FU.apply_with_sides_dev(eng, P.ptrs[:k], P.lds[:k], sd.sides, m, nt, fus, P.ptrs[j], P.lds[j])
    eng.synchronize()
    flat = P.dev[j].cpu().numpy()
    inplace = flat[P.G + offs[j]:P.G + offs[j] + m * lds[j]].reshape(m, lds[j])
    assert np.array_equal(np.ascontiguousarray(inplace[:, :nt]).view(np.int32), exp.view(np.int32))
    assert (inplace[:, nt:] == P.SENTINEL).all() and (flat[:P.G + offs[j]] == P.SENTINEL).all() and (flat[P.G + offs[j] + m * lds[j]:] == P.SENTINEL).all()
    for i in range(k + q):
        if i != j:
            assert np.array_equal(P.dev[i].cpu().numpy().view(np.int32), P.host[i].view(np.int32))
    assert sd.unchanged()


# ------------------------------------------------------------------------------------------- 3. the fit
def _raw_fits(eng, P, k, sides, m, nt, des, dts, prior):
    from plda_amd import fusion as FU
    fits = []
    for sided in (False, True):
        kk, p, l = FU._matrix_args(P.ptrs[:k] if sided else P.ptrs, P.lds[:k] if sided else P.lds)
        raw = np.zeros(1, FU.FIT_DTYPE)
        if sided:
            q, sraw, keep = FU._side_args(sides, m, nt)
            rc = eng._lib.plda_fusion_side_fit_dev(eng._h, kk, vp(p), vp(l), q, vp(sraw), m, nt, C.c_void_p(des.data_ptr()),
                                                   C.c_void_p(dts.data_ptr()), prior, 0.0, 0, vp(raw))
        else:
            rc = eng._lib.plda_fusion_fit_matrices_dev(eng._h, kk, vp(p), vp(l), m, nt, C.c_void_p(des.data_ptr()), C.c_void_p(dts.data_ptr()),
                                                       prior, 0.0, 0, vp(raw))
        assert rc == 0, eng._lib.plda_last_error(eng._h)
        fits.append(raw)
    return fits


@pytest.mark.parametrize("ops,prior,off", [(("min", "max"), 0.5, 0), (("min", "absdiff"), 0.1, 1)])
def test_fit_on_the_planted_case(monkeypatch, ops, prior, off):
    from plda_amd import fusion as FU
    eng = _engine(monkeypatch)
    es, ts, s, qe, qt = sm.planted_case()
    m, nt = s.shape
    rng = np.random.default_rng(5)
    sd = Sides(rng, m, nt, [], off)
    for op in ops:
        sd.add(FU, op, qe, qt, off)
    mats = sm.materialise([(op, qe, qt) for op in ops], m, nt)
    P = Placed([s] + mats, *tgf._placement(1 + len(ops), nt, "one"))
    des, dts = _t(es), _t(ts)
    mat, side = _raw_fits(eng, P, 1, sd.sides, m, nt, des, dts, prior)
    assert side.tobytes() == mat.tobytes()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        f = FU.fit_with_sides_dev(eng, P.ptrs[:1], P.lds[:1], sd.sides, m, nt, des.data_ptr(), dts.data_ptr(), prior)
        alone = FU.fit_from_matrices_dev(eng, P.ptrs[:1], P.lds[:1], m, nt, des.data_ptr(), dts.data_ptr(), prior)
    assert isinstance(f, FU.QualityFusion) and f.n_systems == 1 and f.n_sides == 2 and f.ops == tuple(ops)
    assert f.converged and not f.separable and alone.converged
    assert np.array_equal(f.a, side["a"][0][:3]) and f.b == float(side["b"][0])
    pos, neg = fm.split([s] + mats, es, ts)
    lam2 = tgf._assert_fit_is_optimal(f_as_fusion(f), pos, neg, 3, prior)
    print("planted %s prior %g: Cllr %.4f with sides, %.4f alone; %d iterations, %d passes; model lambda2 = %.3g"
          % (ops, prior, f.cllr_after, alone.cllr_after, f.iterations, f.passes, lam2))
    assert f.cllr_after < alone.cllr_after
    assert P.unchanged() and sd.unchanged()


def f_as_fusion(f):
    """a QualityFusion as the plain Fusion over K + Q features that the existing optimality helper takes"""
    from plda_amd import fusion as FU
    return FU.Fusion(f.a, f.b, f.prior, f.cllr_after, f.converged, f.separable, f.objective, f.lambda2, f.iterations, f.passes)


# ------------------------------------------------------------------------------------------- 4. the operand form
def _score_matrix(eng, dU, dn, nu, m, dV, nt, dzm=None, dzs=None):
    import torch
    S = torch.empty((m, nt), dtype=torch.float32, device=_dev())
    eng.score_matrix_dev(dU.data_ptr(), dn.data_ptr() if dn is not None else None, nu, m, dV.data_ptr(), nt, S.data_ptr(), nt,
                         dzm.data_ptr() if dzm is not None else None, dzs.data_ptr() if dzs is not None else None)
    eng.synchronize()
    return S


@pytest.mark.parametrize("mixed,zn,m,nt,ops,off", [(False, False, 900, 1300, ("min",), 0), (True, True, 513, 1025, ("absdiff", "prod", "sum"), 1)])
def test_operand_form_agrees_with_the_matrix_form(monkeypatch, mixed, zn, m, nt, ops, off):
    """Slabs of 256 rows: 900 rows are four slabs, 513 rows three with a last slab of ONE row -- the enrol vectors and the
    speaker ids of a slab start at its row offset.  The record sums across slabs, so it is not the matrix form's bits:
    integers and extremes equal at a theta between two chain values, sums within the band, two runs the same bytes."""
    from plda_amd import fusion as FU
    d = 48
    eng = _engine(monkeypatch, slab=256, model_d=d)
    rng = np.random.default_rng(31 + mixed)
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    n = rng.integers(1, 4, m).astype(np.int32) if mixed else 2
    es, ts = tgf._labels(rng, m, nt, "random")
    dU, dV, des, dts = _t(U), _t(V), _t(es), _t(ts)
    dn, nu = (_t(n), 0) if mixed else (None, int(n))
    dzm, dzs = (_t(rng.standard_normal(m)), _t(0.5 + rng.random(m))) if zn else (None, None)
    ptr = lambda t: t.data_ptr() if t is not None else None                         # noqa: E731
    S = _score_matrix(eng, dU, dn, nu, m, dV, nt, dzm, dzs)
    Sh = S.cpu().numpy()
    sd = Sides(rng, m, nt, ops, off)
    feats = [Sh] + sd.mats
    a = np.array([50.0 / float(np.abs(Sh).max()), 0.3, -0.2, 0.1][:1 + len(ops)])      # |a_0 s| <= 50: inside the band's range
    c = -0.25
    theta = tgf._theta(feats, a, c)
    ref = fm.pass_matrices(feats, es, ts, a, c, theta)
    mat = FU.pass_with_sides_dev(eng, [S.data_ptr()], [nt], sd.sides, m, nt, des.data_ptr(), dts.data_ptr(), a, c, theta)
    opr = [FU.pass_from_operands_with_sides_dev(eng, dU.data_ptr(), ptr(dn), nu, m, dV.data_ptr(), nt, ptr(dzm), ptr(dzs), des.data_ptr(),
                                                dts.data_ptr(), sd.sides, a, c, theta) for _ in range(2)]
    tgf._same_bits(opr[0], opr[1])
    tgf._compare("matrix form", mat, ref)
    tgf._compare("operand form, slabs of 256 rows", opr[0], ref)
    for key in tgf.INTS + ("ymin_t", "ymax_t", "ymin_n", "ymax_n"):
        assert opr[0][key] == mat[key], key
    assert np.array_equal(opr[0]["smin"], mat["smin"]) and np.array_equal(opr[0]["smax"], mat["smax"])
    # the fits: both optimal by the model's own derivatives (which is what pins them to each other)
    pos, neg = fm.split(feats, es, ts)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        fo = FU.fit_from_operands_with_sides_dev(eng, dU.data_ptr(), ptr(dn), nu, m, dV.data_ptr(), nt, ptr(dzm), ptr(dzs), des.data_ptr(),
                                                 dts.data_ptr(), sd.sides, prior=0.2)
        fmx = FU.fit_with_sides_dev(eng, [S.data_ptr()], [nt], sd.sides, m, nt, des.data_ptr(), dts.data_ptr(), prior=0.2)
    for f in (fo, fmx):
        assert f.n_systems == 1 and f.n_sides == len(ops)
        tgf._assert_fit_is_optimal(f_as_fusion(f), pos, neg, 1 + len(ops), 0.2)
    # Q = 0 in the operand form: this model's score alone, the K = 1 fusion
    o0 = FU.pass_from_operands_with_sides_dev(eng, dU.data_ptr(), ptr(dn), nu, m, dV.data_ptr(), nt, ptr(dzm), ptr(dzs), des.data_ptr(),
                                              dts.data_ptr(), [], a[:1], c, 0.0)
    tgf._compare("operand form, Q = 0", o0, fm.pass_matrices([Sh], es, ts, a[:1], c, 0.0))
    assert sd.unchanged()


# ------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_by_name_and_q0(monkeypatch):
    from plda_amd import fusion as FU
    from plda_amd._native import PLDA_E_INVAL, PldaError
    eng = _engine(monkeypatch)
    lib, h = eng._lib, eng._h
    rng = np.random.default_rng(12)
    m, nt, k = 60, 90, 2
    es, ts = tgf._labels(rng, m, nt, "random")
    tgt = es[:, None] == ts[None, :]
    S = tgf._systems(rng, m, nt, k, tgt)
    dS = [_t(s) for s in S]
    des, dts, dO = _t(es), _t(ts), _t(np.zeros((m, nt), np.float32))
    sd = Sides(rng, m, nt, ["min", "sum", "prod", "max", "absdiff", "min", "max"], 0)
    ptrs = np.array([d.data_ptr() for d in dS] + [dS[0].data_ptr()] * 6, np.uint64)
    ld = np.full(8, nt, np.int64)
    a = np.full(9, 0.01)
    rec, fit = np.zeros(1, FU.RECORD_DTYPE), np.zeros(1, FU.FIT_DTYPE)
    tp = lambda t: C.c_void_p(t.data_ptr())                                         # noqa: E731
    _, sraw, keep = FU._side_args(sd.sides, m, nt)

    def call(which="pass", K=k, Q=2, sides=sraw, A=a):
        s = vp(sides) if sides is not None else None
        if which == "pass":
            return lib.plda_fusion_side_pass_dev(h, K, vp(ptrs), vp(ld), Q, s, m, nt, tp(des), tp(dts), vp(A) if A is not None else None, 0.0, 0.0, vp(rec))
        if which == "fit":
            return lib.plda_fusion_side_fit_dev(h, K, vp(ptrs), vp(ld), Q, s, m, nt, tp(des), tp(dts), 0.5, 0.0, 0, vp(fit))
        return lib.plda_fusion_side_map_dev(h, K, vp(ptrs), vp(ld), Q, s, m, nt, vp(A), 0.0, tp(dO), nt)

    def refused(text, **kw):
        for which in ("pass", "fit", "map"):
            assert call(which, **kw) == PLDA_E_INVAL, (which, kw)
            assert text in lib.plda_last_error(h).decode(), (which, lib.plda_last_error(h).decode())

    refused("n_systems must be 1 .. 8", K=0)
    refused("n_systems must be 1 .. 8", K=9, Q=0)
    refused("n_systems + n_sides must be at most 8", K=2, Q=7)
    refused("n_systems + n_sides must be at most 8", K=8, Q=1)
    refused("n_systems + n_sides must be at most 8", K=2, Q=-1)
    refused("the array of sides is NULL", sides=None)
    for bad_op in (5, -1):
        bad = sraw.copy()
        bad[1]["op"] = bad_op
        refused("side 1 has op %d" % bad_op, sides=bad)
    bad = sraw.copy()
    bad[1]["enrol"] = 0
    refused("the enrol vector of side 1 is NULL", sides=bad)
    bad = sraw.copy()
    bad[0]["test"] = 0
    refused("the test vector of side 0 is NULL", sides=bad)
    assert call("pass", A=None) == PLDA_E_INVAL
    # the operand form checks its sides the same way (before it looks at the model)
    assert lib.plda_score_fusion_side_pass_dev(h, None, None, 1, m, None, nt, None, None, tp(des), tp(dts), 8, vp(sraw), vp(a), 0.0, 0.0, vp(rec)) == PLDA_E_INVAL
    assert "n_systems + n_sides must be at most 8" in lib.plda_last_error(h).decode()
    assert lib.plda_score_fusion_side_fit_dev(h, None, None, 1, m, None, nt, None, None, tp(des), tp(dts), 1, vp(sraw), 0.5, 0.0, 0, vp(fit)) != 0
    assert "not fitted" in lib.plda_last_error(h).decode()
    eng.synchronize()
    assert np.array_equal(dO.cpu().numpy(), np.zeros((m, nt), np.float32))          # no refused map wrote anything

    # Q = 0 is the existing path: the existing record bytes, the existing map bits
    w = np.array([0.3, -0.2])
    theta = tgf._theta(S, w, 0.1)
    rc0, r0 = _raw_side_pass(eng, ptrs[:k], ld[:k], [], m, nt, des, dts, w, 0.1, theta)
    rc1, r1 = _raw_matrix_pass(eng, ptrs[:k], ld[:k], m, nt, des, dts, w, 0.1, theta)
    assert rc0 == 0 and rc1 == 0 and r0.tobytes() == r1.tobytes()
    assert lib.plda_fusion_side_map_dev(h, k, vp(ptrs), vp(ld), 0, None, m, nt, vp(w), 0.1, tp(dO), nt) == 0
    eng.synchronize()
    exp = fm.map_exact([s.ravel() for s in S], w, 0.1).reshape(m, nt)
    assert np.array_equal(dO.cpu().numpy().view(np.int32), exp.view(np.int32))

    # a NaN in a side vector: the status, the count, and the record written all the same.  Side 1 is SUM: a NaN enrol value
    # makes its whole row non-finite (nt trials), and one trial of them also has an infinite score -- counted once
    nan_e = sd.host[1][0].copy()
    nan_e[7] = np.nan
    inf_s = S[0].copy()
    inf_s[7, 3] = np.inf
    d_inf = _t(inf_s)
    sd2 = Sides(rng, m, nt, [], 1)
    sd2.add(FU, "min", *sd.host[0], 1)
    sd2.add(FU, "sum", nan_e, sd.host[1][1], 1)
    rc, r = _raw_side_pass(eng, [d_inf.data_ptr(), dS[1].data_ptr()], [nt, nt], sd2.sides, m, nt, des, dts, a[:4], 0.0, 0.0)
    assert rc == PLDA_E_INVAL and "%d trials with a non-finite score or side value" % nt in lib.plda_last_error(h).decode()
    assert int(r["nonfinite"][0]) == nt and int(r["np"][0]) == int(tgt.sum()) and int(r["np"][0] + r["nn"][0]) == m * nt and int(r["n_systems"][0]) == 4
    # ... and MIN with a NaN enrol value returns the test value, by the written comparison: nothing non-finite
    sd3 = Sides(rng, m, nt, [], 0)
    sd3.add(FU, "min", nan_e, sd.host[1][1], 0)
    rc, r = _raw_side_pass(eng, ptrs[:k], ld[:k], sd3.sides, m, nt, des, dts, a[:3], 0.0, 0.0)
    assert rc == 0 and int(r["nonfinite"][0]) == 0

    # a constant side, a duplicated side, dependent sides: refused by name
    const = Sides(rng, m, nt, [], 0)
    const.add(FU, "min", *sd.host[0], 0)
    const.add(FU, "sum", np.full(m, 1.5, np.float32), np.full(nt, -0.25, np.float32), 0)
    cases = ((const.sides, "side 1 is constant"),
             ([sd.sides[0], sd.sides[0]], "Cholesky pivot of side 1"),
             ([sd.sides[0], FU.Side("max", sd.sides[0].enrol, sd.sides[0].test), FU.Side("sum", sd.sides[0].enrol, sd.sides[0].test)],
              "Cholesky pivot of side 2"))                # min + max = sum but for one fp32 rounding
    for sides, msg in cases:
        with pytest.raises(PldaError, match=msg) as ei:
            FU.fit_with_sides_dev(eng, ptrs[:k], ld[:k], sides, m, nt, des.data_ptr(), dts.data_ptr())
        assert ei.value.code == PLDA_E_INVAL
    # a duplicated SYSTEM is still named as a system
    with pytest.raises(PldaError, match="Cholesky pivot of system 1"):
        FU.fit_with_sides_dev(eng, [ptrs[0], ptrs[0]], ld[:2], sd.sides[:1], m, nt, des.data_ptr(), dts.data_ptr())
    # and the handle still works
    got = FU.pass_with_sides_dev(eng, ptrs[:k], ld[:k], sd.sides[:2], m, nt, des.data_ptr(), dts.data_ptr(), a[:4], 0.1, theta)
    tgf._compare("after the refusals", got, fm.pass_matrices(S + sd.mats[:2], es, ts, a[:4], 0.1, theta))
    del keep


# ------------------------------------------------------------------------------------------- 6. hygiene
def _hygiene_run(eng, S, sd, es, ts, k):
    import torch
    from plda_amd import fusion as FU
    m, nt = S[0].shape
    P = Placed(S, *tgf._placement(k, nt, "one"))
    des, dts = _t(es), _t(ts)
    a = np.array([0.2, -0.1, 0.05, 0.3, -0.2][:k + len(sd.sides)])
    rc, rec = _raw_side_pass(eng, P.ptrs, P.lds, sd.sides, m, nt, des, dts, a, 0.1, 0.5)
    assert rc == 0
    fit = FU.fit_with_sides_dev(eng, P.ptrs, P.lds, sd.sides, m, nt, des.data_ptr(), dts.data_ptr())
    out = torch.zeros((m, nt), dtype=torch.float32, device=_dev())
    torch.cuda.synchronize()
    FU.apply_with_sides_dev(eng, P.ptrs, P.lds, sd.sides, m, nt, fit, out.data_ptr(), nt)
    eng.synchronize()
    assert np.all(np.isfinite(FU._record(rec)["H_n"]))
    return rec.tobytes(), (fit.a.tobytes(), fit.b, fit.cllr_after, fit.passes), out.cpu().numpy().tobytes()


def _hygiene_case():
    rng = np.random.default_rng(8)
    m, nt, k = 520, 1100, 2
    es, ts = tgf._labels(rng, m, nt, "random")
    S = tgf._systems(rng, m, nt, k, es[:, None] == ts[None, :])
    return rng, m, nt, k, es, ts, S


def test_poisoned_scratch_gives_the_same_bits(monkeypatch):
    from plda_amd import MPlda
    rng, m, nt, k, es, ts, S = _hygiene_case()
    runs = []
    for poison in (False, True):
        eng = _engine(monkeypatch, poison=poison)
        sd = Sides(np.random.default_rng(80), m, nt, ["absdiff", "min", "prod"], 1)
        runs.append(_hygiene_run(eng, S, sd, es, ts, k))
        del eng
    MPlda(0)                                   # the poison switch off again for whatever runs next in this process
    assert runs[0] == runs[1]


def test_a_long_lived_handle_gives_a_fresh_handles_bits(monkeypatch):
    """The same calls on a fresh handle, and on one that earlier ran a LARGER K = 8 fusion pass (its partial records still in
    the handle's scratch) and a refused side call."""
    from plda_amd import fusion as FU
    from plda_amd._native import PldaError
    rng, m, nt, k, es, ts, S = _hygiene_case()
    sd = Sides(np.random.default_rng(80), m, nt, ["absdiff", "min", "prod"], 1)
    fresh = _hygiene_run(_engine(monkeypatch), S, sd, es, ts, k)
    eng = _engine(monkeypatch)
    M2, N2 = 1500, 2300
    es2, ts2 = tgf._labels(rng, M2, N2, "random")
    S2 = tgf._systems(rng, M2, N2, 8, es2[:, None] == ts2[None, :])
    d2 = [_t(s) for s in S2]
    FU.pass_from_matrices_dev(eng, [d.data_ptr() for d in d2], [N2] * 8, M2, N2, _t(es2).data_ptr(), _t(ts2).data_ptr(), np.full(8, 0.01), 0.0, 0.0)
    with pytest.raises(PldaError, match="Cholesky pivot of side 1"):
        FU.fit_with_sides_dev(eng, [d2[0].data_ptr()], [N2], [sd_dup(sd, M2, N2)] * 2, M2, N2, _t(es2).data_ptr(), _t(ts2).data_ptr())
    assert _hygiene_run(eng, S, sd, es, ts, k) == fresh


def sd_dup(sd, m, nt):
    from plda_amd import fusion as FU
    rng = np.random.default_rng(81)
    return FU.Side("min", _t(rng.standard_normal(m).astype(np.float32)), _t(rng.standard_normal(nt).astype(np.float32)))


def _small_model():
    from conftest import make_data
    from liblda import PLDA
    x, y = make_data(61, 3000, 32, 60, scale_between=0.15)
    p = PLDA(0)
    p.fit(x, y, 5)
    enrol = p.transform(x[:180], y[:180])                                # 60 models of 3 utterances
    test = p.transform(x[1200:2400], np.arange(1200, dtype=np.uint64))   # 1200 single-utterance tests
    test_speaker = {int(i): int(s) for i, s in zip(range(1200), y[1200:2400])}
    p.norm(x[2400:], enrol)
    rng = np.random.default_rng(4)
    qe = {int(k): float(v) for k, v in zip(enrol.keys(), np.log(rng.uniform(2, 40, 60)))}       # a mapping by key ...
    qt = np.log(rng.uniform(2, 40, 1200)).astype(np.float32)                                     # ... and a sequence
    return p, enrol, test, test_speaker, qe, qt


def test_create_calibrate_quality_destroy_gives_back_every_byte():
    import torch
    from plda_amd import _native
    lib = _native.load()
    p, enrol, test, test_speaker, qe, qt = _small_model()
    quality = [("min", qe, qt), ("absdiff", qe, qt)]
    del p
    gc.collect()
    torch.cuda.synchronize()
    before = lib.plda_device_bytes_held()
    from liblda import PLDA
    from conftest import make_data
    x, y = make_data(61, 3000, 32, 60, scale_between=0.15)
    for _ in range(2):
        p = PLDA(0)
        p.fit(x, y, 5)
        p.norm(x[2400:], enrol)
        f = p.calibrate_quality(enrol, test, test_speaker, quality)
        assert f.n_sides == 2 and lib.plda_device_bytes_held() > before
        p.score_matrix_fused(enrol, test, (), f, quality=quality)
        del p
        gc.collect()
        torch.cuda.synchronize()
        assert lib.plda_device_bytes_held() == before


# ------------------------------------------------------------------------------------------- 7. end to end
def test_end_to_end_calibrate_quality():
    from plda_amd import fusion as FU
    p, enrol, test, test_speaker, qe, qt = _small_model()
    plain = p.score_matrix(enrol, test)
    quality = [("min", qe, qt), ("absdiff", qe, qt)]
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        f = p.calibrate_quality(enrol, test, test_speaker, quality, prior=0.5)                    # the operand form
        rng = np.random.default_rng(3)
        other = (0.02 * plain.astype(np.float64) + 0.5 * rng.standard_normal(plain.shape) - 20.0).astype(np.float32)
        f2 = p.calibrate_quality(enrol, test, test_speaker, quality, others=[other], prior=0.5)   # the matrix form
    assert isinstance(f, FU.QualityFusion) and f.n_systems == 1 and f.n_sides == 2 and f.ops == ("min", "absdiff") and f.converged
    assert f2.n_systems == 2 and f2.n_sides == 2 and f2.converged
    assert np.array_equal(p.score_matrix(enrol, test).view(np.int32), plain.view(np.int32))      # nothing stored, defaults unchanged
    qev = np.array([qe[int(k)] for k in enrol.keys()], np.float32)
    es = np.array(list(enrol.keys()), np.int64)
    ts = np.array([test_speaker[int(k)] for k in test.keys()], np.int64)
    mats = sm.materialise([("min", qev, qt), ("absdiff", qev, qt)], 60, 1200)
    pos, neg = fm.split([plain] + mats, es, ts)
    lam2 = fm.newton(fm.pass_record(pos, neg, f.a, f.b), 0.5)[2]
    cal = p.calibrate(enrol, test, test_speaker)
    print("end to end: a = %s, b = %.6g, Cllr with qualities %.4f, calibrated alone %.4f, model lambda2 = %.3g" % (f.a, f.b, f.cllr_after, cal.cllr_after, lam2))
    assert lam2 <= 1e-17
    assert f.cllr_after <= cal.cllr_after + 1e-12                        # nested models, the same objective at prior 0.5
    fused = p.score_matrix_fused(enrol, test, (), f, quality=quality)
    host = f([plain], [(qev, qt), (qev, qt)])
    assert fused.dtype == np.float32 and fused.shape == plain.shape
    # within one fp32 rounding of the fp64 host map (which adds products, where the device chains fused multiply-adds)
    assert np.all(np.abs(fused.astype(np.float64) - host) <= np.spacing(np.abs(host).astype(np.float32)).astype(np.float64))
    exp = fm.map_exact([plain.ravel()] + [x.ravel() for x in mats], f.a, f.b).reshape(plain.shape)
    assert np.array_equal(fused.view(np.int32), exp.view(np.int32))
    fused2 = p.score_matrix_fused(enrol, test, [other], f2, quality=quality)
    exp2 = fm.map_exact([plain.ravel(), other.ravel()] + [x.ravel() for x in mats], f2.a, f2.b).reshape(plain.shape)
    assert np.array_equal(fused2.view(np.int32), exp2.view(np.int32))
    # the checks that come before any device call
    with pytest.raises(ValueError, match="unknown side op"):
        p.calibrate_quality(enrol, test, test_speaker, [("mean", qe, qt)])
    with pytest.raises(ValueError, match="1199 test values"):
        p.calibrate_quality(enrol, test, test_speaker, [("min", qe, qt[:-1])])
    with pytest.raises(ValueError, match="at most 8"):
        p.calibrate_quality(enrol, test, test_speaker, [("min", qe, qt)] * 8)
    with pytest.raises(ValueError):
        p.score_matrix_fused(enrol, test, (), f, quality=[("max", qe, qt), ("absdiff", qe, qt)])   # not the fitted ops
    with pytest.raises(ValueError):
        p.score_matrix_fused(enrol, test, [other], f2)                                            # a quality fusion without its qualities
