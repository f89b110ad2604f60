"""GPU: top-N selection with indices (csrc/topn.hip; include/plda_hip.h "top-N retrieval with indices").

The reference of every check is code older than the feature: the full fp32 matrix (crafted, or written by score_matrix_dev /
score_matrix_snorm_dev for the same inputs) fed to tests/topn_model.top_n.  Equality is EXACT, for the indices and for the
bits of the scores; there is no tolerance anywhere.

  1. the matrix form on crafted matrices, both axes, every top_n, with row padding, with pieces of the default height and of 128;
  2. the operand form against the materialised matrix: three GEMM depths, no statistics / z-norm / S-norm pairs, slabs of 128;
  3. two calls bit-identical, the host form equal to the device form;
  4. liblda.PLDA.top_n end to end, with the rank-1 rate of plda_amd.identify;
  5. API edges; 6. guard bands, poisoned scratch, leaks, the memory a call holds.

Nothing here provokes a fault: stray accesses would land in memory the test owns."""
import numpy as np
import pytest

import topn_model as tm
from conftest import make_data

pytestmark = pytest.mark.gpu

ENV = ("PLDA_SNORM_SLAB_ROWS", "PLDA_SCRATCH_POISON", "PLDA_MIXED_VARIANT")
TOPN_MAX = 256


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _engine(monkeypatch, d=None, slab=None, poison=False):
    """An MPlda whose pieces / slabs are `slab` rows high (None: by size); with a model of dimension d when d is given."""
    from plda_amd import MPlda
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    if slab:
        monkeypatch.setenv("PLDA_SNORM_SLAB_ROWS", str(slab))
    if poison:
        monkeypatch.setenv("PLDA_SCRATCH_POISON", "1")
    eng = MPlda(0)
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    if d is not None:
        rng = np.random.default_rng(d)
        q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        eng.set_model(rng.random(d), q * (1.0 + rng.random(d))[:, None], np.sort(0.05 + 4.0 * rng.random(d))[::-1].copy())
    return eng


def _ns(length):
    return sorted({min(n, length) for n in (1, 2, 10, 100, TOPN_MAX)})


def _same(label, got, ref):
    """(scores, index) pairs equal: the indices, and the scores as bit patterns."""
    assert got[1].dtype == np.int64 and got[0].dtype == np.float32, label
    assert np.array_equal(got[1], ref[1]), (label, "index", int((got[1] != ref[1]).sum()))
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), (label, "score bits")


def _matrix_topn(eng, dS, ld, m, nt, axis, n):
    """topn_matrix_dev on a device matrix; the outputs start as a pattern no result holds."""
    import torch
    lines = m if axis == 0 else nt
    os_ = torch.full((lines, n), float("nan"), dtype=torch.float32, device=_dev())
    oi = torch.full((lines, n), -7, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize()                   # (the handle's stream does not wait for torch's fills and copies)
    eng.topn_matrix_dev(dS.data_ptr(), ld, m, nt, axis, n, os_.data_ptr(), oi.data_ptr())
    eng.synchronize()
    return os_.cpu().numpy(), oi.cpu().numpy()


# ------------------------------------------------------------------------------------------- 1. matrix form, crafted
SHAPES = [(1, 1), (1, 63), (130, 1), (130, 1000), (1025, 4097), (257, 20011)]
CONTENTS = ["gaussian", "equal", "zeros", "ascending", "descending", "binade", "nonfinite", "duplicates"]


_content = tm.content


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("m,nt", SHAPES)
def test_matrix_form_on_crafted_matrices(monkeypatch, m, nt, kind):
    import torch
    rng = np.random.default_rng(m + nt)
    S = _content(kind, m, nt, rng)
    engines = [("default", _engine(monkeypatch)), ("pieces of 128", _engine(monkeypatch, slab=128))]
    pad4 = (nt + 3) // 4 * 4
    refs = [tm.top_n(S, _ns(nt if axis == 0 else m)[-1], axis) for axis in (0, 1)]
    for ld in sorted({nt, pad4 + 4, nt + 1}):          # contiguous; 16-byte rows with padding; unaligned rows with padding
        dS = torch.full((m, ld), float("nan"), dtype=torch.float32, device=_dev())       # (a NaN has the highest key of all)
        dS[:, :nt] = _t(S)
        for axis in (0, 1):
            length = nt if axis == 0 else m
            ref = refs[axis]
            for n in _ns(length):
                want = (ref[0][:, :n], ref[1][:, :n])
                for name, eng in engines:
                    got = _matrix_topn(eng, dS, ld, m, nt, axis, n)
                    _same("%s %dx%d ld %d axis %d n %d, %s" % (kind, m, nt, ld, axis, n, name), got, want)
                if kind in ("equal", "zeros"):
                    assert np.array_equal(want[1], np.broadcast_to(np.arange(n), want[1].shape))


# ------------------------------------------------------------------------------------------- 2. operand form
def _counts(kind, r, rng):
    """The three GEMM depths of tests/test_gpu_asnorm.py::_counts."""
    if kind == "uniform":
        return 3
    if kind == "two":
        return rng.choice(np.array([2, 5], np.int32), r).astype(np.int32)
    n = rng.choice(np.array([1, 3, 5000], np.int32), r).astype(np.int32)       # a count above 4095: the depth-2D form
    n[0] = 5000
    return n


def _full_matrix(eng, U, n, V, zn=None, sn=None):
    """The materialised fp32 matrix: score_matrix_dev (zn: (zmean, zstd) or None) or score_matrix_snorm_dev (sn: four arrays, a
    pair may be None)."""
    import torch
    m, nt = U.shape[0], V.shape[0]
    dU, dV = _t(U), _t(V)
    dn = None if np.isscalar(n) else _t(np.asarray(n, np.int32))
    nptr, nu = (dn.data_ptr(), 0) if dn is not None else (None, int(n))
    out = torch.full((m, nt), float("nan"), dtype=torch.float32, device=_dev())
    torch.cuda.synchronize()
    if sn is not None:
        st = [None if a is None else _t(a) for a in sn]
        eng.score_matrix_snorm_dev(dU.data_ptr(), nptr, nu, m, dV.data_ptr(), nt, out.data_ptr(), nt,
                                   *[None if a is None else a.data_ptr() for a in st])
    else:
        st = [None, None] if zn is None else [_t(a) for a in zn]
        eng.score_matrix_dev(dU.data_ptr(), nptr, nu, m, dV.data_ptr(), nt, out.data_ptr(), nt,
                             *[None if a is None else a.data_ptr() for a in st])
    eng.synchronize()
    return out.cpu().numpy()


def _operand_topn(eng, U, n, V, axis, top_n, zn=None, sn=None):
    import torch
    m, nt = U.shape[0], V.shape[0]
    lines = m if axis == 0 else nt
    dU, dV = _t(U), _t(V)
    dn = None if np.isscalar(n) else _t(np.asarray(n, np.int32))
    nptr, nu = (dn.data_ptr(), 0) if dn is not None else (None, int(n))
    st = [None if a is None else _t(a) for a in (tuple(zn) if zn is not None else (None, None)) + (tuple(sn) if sn is not None else (None,) * 4)]
    os_ = torch.full((lines, top_n), float("nan"), dtype=torch.float32, device=_dev())
    oi = torch.full((lines, top_n), -7, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize()
    eng.score_topn_dev(dU.data_ptr(), nptr, nu, m, dV.data_ptr(), nt, axis, top_n, os_.data_ptr(), oi.data_ptr(),
                       *[None if a is None else a.data_ptr() for a in st])
    eng.synchronize()
    return os_.cpu().numpy(), oi.cpu().numpy()


def _operands(d, kind, m=300, nt=517):
    """Operands with exact ties: a third of the test rows are copies of others (axis 0), a third of the enrol rows are copies
    of others WITH their counts and statistics (axis 1)."""
    rng = np.random.default_rng(d + len(kind))
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    n = _counts(kind, m, rng)
    src_v, src_u = rng.integers(0, nt, nt // 3), rng.integers(0, m, m // 3)
    dst_v, dst_u = rng.permutation(nt)[:nt // 3], rng.permutation(m)[:m // 3]
    stats = dict(zm=rng.standard_normal(m) * 10 - 20, zs=0.5 + 5 * rng.random(m), em=rng.standard_normal(m) * 10 - 20,
                 es=0.5 + 5 * rng.random(m), tm=rng.standard_normal(nt) * 10 - 20, ts=0.5 + 5 * rng.random(nt))
    stats["zs"][::7] = 0.0                    # a zero std leaves the row un-normalised
    stats["es"][::11] = 0.0
    stats["ts"][::5] = 0.0
    for dst, src in zip(dst_v, src_v):
        V[dst] = V[src]
        stats["tm"][dst], stats["ts"][dst] = stats["tm"][src], stats["ts"][src]
    for dst, src in zip(dst_u, src_u):
        U[dst] = U[src]
        if not np.isscalar(n):
            n[dst] = n[src]
        for k in ("zm", "zs", "em", "es"):
            stats[k][dst] = stats[k][src]
    if kind == "big":
        n[0] = 5000
    return U, n, V, stats


MODES = ["raw", "znorm", "snorm both", "snorm enrol", "snorm test"]


def _mode_args(mode, st):
    if mode == "raw":
        return None, None
    if mode == "znorm":
        return (st["zm"], st["zs"]), None
    if mode == "snorm both":
        return None, (st["em"], st["es"], st["tm"], st["ts"])
    if mode == "snorm enrol":
        return None, (st["em"], st["es"], None, None)
    return None, (None, None, st["tm"], st["ts"])


@pytest.mark.parametrize("kind", ["uniform", "two", "big"])
@pytest.mark.parametrize("d", [48, 200, 257])
def test_operand_form_equals_the_materialised_matrix(monkeypatch, d, kind):
    U, n, V, st = _operands(d, kind)
    m, nt = U.shape[0], V.shape[0]
    eng, small = _engine(monkeypatch, d), _engine(monkeypatch, d, slab=128)
    for mode in MODES:
        zn, sn = _mode_args(mode, st)
        S = _full_matrix(eng, U, n, V, zn=zn, sn=sn)
        dS = _t(S)
        by_row, by_col = np.sort(S, axis=1), np.sort(S, axis=0)
        assert (by_row[:, 1:] == by_row[:, :-1]).any() and (by_col[1:] == by_col[:-1]).any(), mode   # the copies do tie, along both axes
        for axis in (0, 1):
            length = nt if axis == 0 else m
            ref = tm.top_n(S, _ns(length)[-1], axis)
            for top in (1, 10, 100, _ns(length)[-1]):
                want = (ref[0][:, :top], ref[1][:, :top])
                label = "D %d %s %s axis %d n %d" % (d, kind, mode, axis, top)
                _same(label + " matrix form", _matrix_topn(eng, dS, nt, m, nt, axis, top), want)
                _same(label + " operand form", _operand_topn(eng, U, n, V, axis, top, zn=zn, sn=sn), want)
                _same(label + " operand form, slabs of 128", _operand_topn(small, U, n, V, axis, top, zn=zn, sn=sn), want)


# ------------------------------------------------------------------------------------------- 3. repeatable; host form
@pytest.mark.parametrize("axis", [0, 1])
def test_two_calls_identical_and_host_form_equals_device_form(monkeypatch, axis):
    from plda_amd.libplda import _ptr
    d, top = 200, 50
    U, n, V, st = _operands(d, "two", m=333, nt=777)
    m, nt = U.shape[0], V.shape[0]
    lines = m if axis == 0 else nt
    eng = _engine(monkeypatch, d, slab=128)
    for mode in MODES:
        zn, sn = _mode_args(mode, st)
        first = _operand_topn(eng, U, n, V, axis, top, zn=zn, sn=sn)
        _same(mode + ": second call", _operand_topn(eng, U, n, V, axis, top, zn=zn, sn=sn), first)
        hs, hi = np.full((lines, top), np.nan, np.float32), np.full((lines, top), -7, np.int64)
        host = [None if a is None else np.ascontiguousarray(a, np.float64) for a in (zn or (None, None)) + (sn or (None,) * 4)]
        eng._ck(eng._lib.plda_score_topn(eng._h, _ptr(U), _ptr(n), 0, m, _ptr(V), nt, *[_ptr(a) for a in host], axis, top,
                                         _ptr(hs), _ptr(hi)))
        _same(mode + ": host form", (hs, hi), first)


# ------------------------------------------------------------------------------------------- 4. end to end
def test_plda_top_n_end_to_end():
    from liblda import PLDA
    from plda_amd import identify
    x, y = make_data(61, 3000, 32, 60, scale_between=0.15)               # real speaker structure, classes that overlap
    p = PLDA(0)
    p.fit(x, y, 5)
    enrol = p.transform(x[:180], y[:180])                                # 60 models of 3 utterances
    test = p.transform(x[1200:1900], np.arange(700, dtype=np.uint64) + 1000)      # 700 single-utterance tests, keys 1000 ...
    truth = y[1200:1900].astype(np.int64)
    p.norm(x[2400:], enrol)
    cohort = p.transform_array(x[2400:], 1)
    ekeys = np.array(list(enrol.keys()), np.int64)
    tkeys = np.array(list(test.keys()), np.int64)
    plain = p.score_matrix(enrol, test)
    asn = p.score_matrix_asnorm(enrol, test, cohort, top_k=100)
    assert not np.array_equal(plain, p.score_matrix(enrol, test, znorm=False))            # the z-norm statistics are in use
    for S, kw in ((plain, {}), (p.score_matrix(enrol, test, znorm=False), dict(znorm=False)), (asn, dict(cohort=cohort, top_k=100))):
        for per, axis, keys, n in (("test", 1, ekeys, 10), ("enrol", 0, tkeys, 25), ("test", 1, ekeys, 60)):
            ref = tm.top_n(S, n, axis)
            scores, ids = p.top_n(enrol, test, n=n, per=per, **kw)
            _same("%s per %s n %d" % (sorted(kw), per, n), (scores, ids), (ref[0], keys[ref[1]]))
    # rank-N identification: the rate from the ids equals the one from the full matrix
    scores, ids = p.top_n(enrol, test, n=10)
    best = ekeys[np.array([int(np.argmax(plain[:, j])) for j in range(plain.shape[1])])]
    rates = identify.rank_rates(ids, truth)
    assert rates[1] == float((best == truth).mean())
    order = np.argsort(-plain.astype(np.float64), axis=0, kind="stable")
    assert rates[5] == float((ekeys[order[:5]] == truth[None, :]).any(axis=0).mean())
    assert 1.0 / 60 < rates[1] <= rates[5] <= rates[10] <= 1.0                            # (above chance: 60 models)
    assert np.array_equal(identify.cmc(ids, truth)[[0, 4, 9]], [rates[1], rates[5], rates[10]])
    # the stored calibration: the same ids, the scores of the calibrated matrix at those ids, bit for bit
    with pytest.raises(ValueError, match="stored calibration"):
        p.top_n(enrol, test, calibrate=True)
    cal = p.calibrate(enrol, test, {int(k): int(s) for k, s in zip(tkeys, truth)})
    assert cal.a > 0
    mapped = p.score_matrix(enrol, test, calibrate=True)
    ref = tm.top_n(plain, 10, 1)
    cs, cids = p.top_n(enrol, test, n=10, calibrate=True)
    assert np.array_equal(cids, ekeys[ref[1]])
    assert np.array_equal(cs.view(np.uint32), np.take_along_axis(np.ascontiguousarray(mapped.T), ref[1], axis=1).view(np.uint32))
    mapped_as = p.score_matrix_asnorm(enrol, test, cohort, top_k=100, calibrate=True)
    ref = tm.top_n(asn, 7, 0)
    cs, cids = p.top_n(enrol, test, n=7, per="enrol", cohort=cohort, top_k=100, calibrate=True)
    assert np.array_equal(cids, tkeys[ref[1]])
    assert np.array_equal(cs.view(np.uint32), np.take_along_axis(mapped_as, ref[1], axis=1).view(np.uint32))
    # a side without keys: positions
    _, counts, Uv = p._instance._unpack(enrol)
    _, _, Vv = p._instance._unpack(test)
    s2, i2 = p.top_n((counts, Uv), (1, Vv), n=3, znorm=False)
    ref = tm.top_n(p.score_matrix(enrol, test, znorm=False), 3, 1)
    _same("no keys", (s2, i2), ref)
    # a map that would reverse the order is refused
    from plda_amd.calibration import Calibration
    p._instance._calibration = Calibration(-1.0, 0.0, 0.5)
    with pytest.raises(ValueError, match="a <= 0"):
        p.top_n(enrol, test, calibrate=True)
    with pytest.raises(ValueError, match="per must be"):
        p.top_n(enrol, test, per="column")


# ------------------------------------------------------------------------------------------- 5. API edges
def test_api_edges(monkeypatch):
    import torch
    from plda_amd import MPlda
    from plda_amd._native import PLDA_E_INVAL, PLDA_E_NOT_FITTED, PldaError
    d, m, nt = 48, 10, 20
    rng = np.random.default_rng(1)
    Uh, Vh = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    U, V = _t(Uh), _t(Vh)
    S = _t(rng.standard_normal((m, nt)).astype(np.float32))
    st = torch.ones((6, nt), dtype=torch.float64, device=_dev())
    os_ = torch.zeros((nt, nt), dtype=torch.float32, device=_dev())
    oi = torch.zeros((nt, nt), dtype=torch.int64, device=_dev())
    fresh = MPlda(0)
    torch.cuda.synchronize()
    with pytest.raises(PldaError, match="score_topn: model not fitted") as ei:
        fresh.score_topn_dev(U.data_ptr(), None, 1, m, V.data_ptr(), nt, 0, 5, os_.data_ptr(), oi.data_ptr())
    assert ei.value.code == PLDA_E_NOT_FITTED
    with pytest.raises(PldaError, match="score_topn: model not fitted"):
        hs, hi = np.zeros((m, 5), np.float32), np.zeros((m, 5), np.int64)
        from plda_amd.libplda import _ptr
        fresh._ck(fresh._lib.plda_score_topn(fresh._h, _ptr(Uh), None, 1, m, _ptr(Vh), nt, None, None, None, None, None, None, 0, 5,
                                             _ptr(hs), _ptr(hi)))
    eng = _engine(monkeypatch, d)
    base_m = dict(dscores=S.data_ptr(), ld=nt, m=m, nt=nt, axis=0, top_n=5, dout_scores=os_.data_ptr(), dout_index=oi.data_ptr())
    bad_matrix = [
        (dict(axis=2), r"axis = 2 \(must be 0"), (dict(axis=-1), "axis = -1"), (dict(top_n=0), "top_n = 0"),
        (dict(top_n=nt + 1), r"top_n = 21 \(must be in 1 ... min\(256, Nt = 20\)\)"),
        (dict(axis=1, top_n=m + 1), r"top_n = 11 \(must be in 1 ... min\(256, M = 10\)\)"),
        (dict(top_n=257), "top_n = 257"), (dict(m=0), "M = 0"), (dict(nt=0), "Nt = 0"), (dict(nt=(1 << 30) + 1, ld=(1 << 30) + 1), "at most 2\\^30"),
        (dict(ld=nt - 1), "ld = 19 < Nt = 20"), (dict(dscores=None), "scores is NULL"), (dict(dout_scores=None), "out_scores is NULL"),
        (dict(dout_index=None), "out_index is NULL"),
    ]
    for kw, text in bad_matrix:
        a = dict(base_m)
        a.update(kw)
        with pytest.raises(PldaError, match="topn_matrix: .*" + text) as ei:
            eng.topn_matrix_dev(**a)
        assert ei.value.code == PLDA_E_INVAL, kw
    base_o = dict(dU=U.data_ptr(), dn=None, n_uniform=1, m=m, dV=V.data_ptr(), nt=nt, axis=1, top_n=5, dout_scores=os_.data_ptr(),
                  dout_index=oi.data_ptr())
    p = [st[i].data_ptr() for i in range(6)]
    bad_operand = [
        (dict(axis=3), "axis = 3"), (dict(top_n=0), "top_n = 0"), (dict(top_n=m + 1), r"min\(256, M = 10\)"),
        (dict(axis=0, top_n=nt + 1), r"min\(256, Nt = 20\)"), (dict(m=0), "M = 0"), (dict(nt=0), "Nt = 0"),
        (dict(dU=None), "U is NULL"), (dict(dV=None), "V is NULL"), (dict(dout_scores=None), "out_scores is NULL"),
        (dict(dout_index=None), "out_index is NULL"), (dict(n_uniform=0), "n_uniform must be > 0"),
        (dict(dzmean=p[0]), "zstd is NULL but its partner is not"), (dict(dzstd=p[1]), "zmean is NULL"),
        (dict(demean=p[2]), "estd is NULL"), (dict(destd=p[3]), "emean is NULL"), (dict(dtmean=p[4]), "tstd is NULL"),
        (dict(dtstd=p[5]), "tmean is NULL"),
        (dict(dzmean=p[0], dzstd=p[1], demean=p[2], destd=p[3]), "z-norm statistics .* together with S-norm statistics"),
        (dict(dzmean=p[0], dzstd=p[1], dtmean=p[4], dtstd=p[5]), "together with S-norm"),
    ]
    for kw, text in bad_operand:
        a = dict(base_o)
        a.update(kw)
        with pytest.raises(PldaError, match="score_topn: .*" + text) as ei:
            eng.score_topn_dev(**a)
        assert ei.value.code == PLDA_E_INVAL, kw
    # the handle is still usable; top_n equal to the length of a line, along both axes: the whole line, sorted
    full = _full_matrix(eng, Uh, 1, Vh)
    for axis, length in ((0, nt), (1, m)):
        _same("whole line, axis %d" % axis, _operand_topn(eng, Uh, 1, Vh, axis, length), tm.top_n(full, length, axis))
        _same("whole line, matrix form", _matrix_topn(eng, _t(full), nt, m, nt, axis, length), tm.top_n(full, length, axis))
    with pytest.raises(ValueError, match=r"must be \[rows, 48\] \(the model's current dimension\)"):
        eng.top_n((1, rng.standard_normal((3, d - 1))), (1, rng.standard_normal((3, d))), n=2)
    with pytest.raises(PldaError, match="top_n = 4"):
        eng.top_n((1, rng.standard_normal((3, d))), (1, rng.standard_normal((5, d))), n=4)          # three models only
    with pytest.raises(ValueError, match="no trials"):
        eng.top_n((1, np.zeros((0, d))), (1, rng.standard_normal((5, d))), n=1)


# ------------------------------------------------------------------------------------------- 6. guards, poison, leaks
GUARD_BYTES = 64 << 10
PAYLOAD = 0x7FC0DEAD


def _input(a, nan, ld=None):
    """`a` placed in a buffer with GUARD_BYTES of NaN (or zero; -1 / 0 for integers) on both sides and in the tail of every
    row when a pitch is given."""
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a)
    g = GUARD_BYTES // a.itemsize
    rows, cols = (a.shape[0], a.shape[1]) if a.ndim == 2 else (1, a.shape[0])
    ld = ld or cols
    buf = torch.empty(g + rows * ld + g, dtype=t.dtype, device=_dev())
    if t.dtype.is_floating_point:
        buf.fill_(float("nan") if nan else 0.0)
    else:
        buf.fill_(-1 if nan else 0)
    body = buf[g:g + rows * ld].view(rows, ld)[:, :cols]
    body.copy_(t.reshape(rows, cols).to(_dev()))
    return buf, body


class _Output:
    """An output [rows, cols] inside a buffer filled with the payload."""

    def __init__(self, rows, cols, dtype):
        import torch
        self.rows, self.cols = rows, cols
        self.itemsize = torch.empty(0, dtype=dtype).element_size()
        self.g = GUARD_BYTES // self.itemsize
        n = self.g + rows * cols + self.g
        self.words = torch.full((n * self.itemsize // 4,), PAYLOAD, dtype=torch.int32, device=_dev())
        self.buf = self.words.view(dtype)
        self.body = self.buf[self.g:self.g + rows * cols].view(rows, cols)

    def ptr(self):
        return self.body.data_ptr()

    def check(self, what):
        import torch
        torch.cuda.synchronize()
        w = self.words.cpu().numpy().reshape(-1, self.itemsize // 4)
        wg = self.g
        guard = np.concatenate([w[:wg], w[wg + self.rows * self.cols:]])
        bad = np.nonzero((guard != np.int32(PAYLOAD)).any(1))[0]
        assert bad.size == 0, "%s: %d guard elements overwritten" % (what, bad.size)
        left = int((w[wg:wg + self.rows * self.cols] == np.int32(PAYLOAD)).all(1).sum())
        assert left == 0, "%s: %d output elements never written" % (what, left)
        return self.body.cpu().numpy().copy()


@pytest.mark.parametrize("d,m,nt,ld,kind", [(48, 63, 517, 519, "uniform"), (200, 333, 1029, 1032, "two"), (257, 130, 260, 260, "big")])
def test_guard_bands_and_poisoned_scratch(monkeypatch, d, m, nt, ld, kind):
    import torch
    rng = np.random.default_rng(m)
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    n = _counts(kind, m, rng)
    em, es = rng.standard_normal(m), 0.5 + rng.random(m)
    tmn, tsd = rng.standard_normal(nt), 0.5 + rng.random(nt)
    S = (10.0 * rng.standard_normal((m, nt))).astype(np.float32)
    top = 40
    runs = {}
    for poison in (False, True):
        for nan in (True, False):
            eng = _engine(monkeypatch, d, poison=poison, slab=128)
            keep = [_input(a, nan) for a in (U, V, em, es, tmn, tsd)] + [_input(S, nan, ld)]
            dU, dV, dem, des, dtm, dts, dS = [b for _, b in keep]
            dn = None if np.isscalar(n) else _input(n, nan)
            nptr = dn[1].data_ptr() if dn is not None else None
            nu = int(n) if np.isscalar(n) else 0
            run = {}
            for axis in (0, 1):
                lines = m if axis == 0 else nt
                outs = [(_Output(lines, top, torch.float32), _Output(lines, top, torch.int64)) for _ in range(4)]
                torch.cuda.synchronize()
                eng.topn_matrix_dev(dS.data_ptr(), ld, m, nt, axis, top, outs[0][0].ptr(), outs[0][1].ptr())
                eng.score_topn_dev(dU.data_ptr(), nptr, nu, m, dV.data_ptr(), nt, axis, top, outs[1][0].ptr(), outs[1][1].ptr())
                eng.score_topn_dev(dU.data_ptr(), nptr, nu, m, dV.data_ptr(), nt, axis, top, outs[2][0].ptr(), outs[2][1].ptr(),
                                   dzmean=dem.data_ptr(), dzstd=des.data_ptr())
                eng.score_topn_dev(dU.data_ptr(), nptr, nu, m, dV.data_ptr(), nt, axis, top, outs[3][0].ptr(), outs[3][1].ptr(),
                                   demean=dem.data_ptr(), destd=des.data_ptr(), dtmean=dtm.data_ptr(), dtstd=dts.data_ptr())
                eng.synchronize()
                for name, (o_s, o_i) in zip(("matrix", "raw", "znorm", "snorm"), outs):
                    run["%s scores axis %d" % (name, axis)] = o_s.check("%s scores" % name)
                    run["%s index axis %d" % (name, axis)] = o_i.check("%s index" % name)
            runs[(poison, nan)] = run
            del eng
    from plda_amd import MPlda
    MPlda(0)                                   # the poison switch off again for whatever runs next in this process
    first = runs[(False, True)]
    for key, run in runs.items():
        for k in first:
            assert np.array_equal(first[k].view(np.uint8), run[k].view(np.uint8)), (key, k)
    eng = _engine(monkeypatch, d)
    for axis in (0, 1):
        _same("guarded matrix", (first["matrix scores axis %d" % axis], first["matrix index axis %d" % axis]), tm.top_n(S, top, axis))
        full = _full_matrix(eng, U, n, V, sn=(em, es, tmn, tsd))
        _same("guarded operands", (first["snorm scores axis %d" % axis], first["snorm index axis %d" % axis]), tm.top_n(full, top, axis))


def test_repeated_calls_hold_no_more_and_destroy_gives_back_every_byte(monkeypatch):
    import gc
    import torch
    from plda_amd import _native
    lib = _native.load()
    rng = np.random.default_rng(2)
    d, m, nt = 64, 300, 700
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    S = _t(rng.standard_normal((m, nt)).astype(np.float32))
    gc.collect()
    torch.cuda.synchronize()
    before = lib.plda_device_bytes_held()
    for _ in range(2):
        eng = _engine(monkeypatch, d)
        held = None
        for rep in range(3):
            for axis in (0, 1):
                _operand_topn(eng, U, 2, V, axis, 20)
                _matrix_topn(eng, S, nt, m, nt, axis, 20)
                eng.top_n((2, U), (1, V), n=5, per="test" if axis else "enrol", znorm=False)
            eng.synchronize()
            if held is None:
                held = lib.plda_device_bytes_held()
            assert lib.plda_device_bytes_held() == held                 # the second and third rounds allocate nothing new
        assert held > before
        del eng
        gc.collect()
        assert lib.plda_device_bytes_held() == before


@pytest.mark.parametrize("axis", [0, 1])
def test_a_call_holds_one_slab_whatever_the_matrix(monkeypatch, axis):
    """4096 x 20 000 with slabs of 256 rows: the call's peak stays below the slab and the packed operands.  The O(L top_n)
    term is ZERO bytes: axis 0 needs no state across slabs and the state of axis 1 lives in the caller's outputs."""
    import torch
    from plda_amd import _native
    lib = _native.load()
    D, M, Nt, top = 200, 4096, 20000, 100
    eng = _engine(monkeypatch, D, slab=256)
    g = torch.Generator(device=_dev())
    g.manual_seed(9)
    U = torch.randn((M, D), dtype=torch.float64, device=_dev(), generator=g)
    V = torch.randn((Nt, D), dtype=torch.float64, device=_dev(), generator=g)
    lines = M if axis == 0 else Nt
    os_ = torch.full((lines, top), float("nan"), dtype=torch.float32, device=_dev())
    oi = torch.full((lines, top), -7, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize()
    before = lib.plda_device_bytes_held()
    lib.plda_device_bytes_peak(1)
    eng.score_topn_dev(U.data_ptr(), None, 1, M, V.data_ptr(), Nt, axis, top, os_.data_ptr(), oi.data_ptr())
    eng.synchronize()
    rose = lib.plda_device_bytes_peak(0) - before
    pad = lambda v, q: (v + q - 1) // q * q                                         # noqa: E731
    kpad = pad(D, 4) + 32                                                          # k-quads + the bias planes of a packed row
    slab = 256 * pad(Nt, 4) * 4
    operands = (256 + pad(Nt, 256)) * kpad * 4 + (256 + pad(Nt, 256)) * 4 * 8
    cap = (slab + operands) + (slab + operands) // 8 + (1 << 20)                   # the buffers' growth slack
    scratch = 0 * lines * top
    print("axis %d: device bytes rose by %.1f MiB (slab %.1f MiB, packed operands %.1f MiB; the matrix is %.1f MiB)"
          % (axis, rose / 2 ** 20, slab / 2 ** 20, operands / 2 ** 20, M * Nt * 4 / 2 ** 20))
    assert rose <= cap + scratch
    assert rose < M * Nt * 4 // 4
    # and the result is the materialised matrix's, on 64 lines spread over it
    S = torch.empty((M, Nt), dtype=torch.float32, device=_dev())
    eng.score_matrix_dev(U.data_ptr(), None, 1, M, V.data_ptr(), Nt, S.data_ptr(), Nt)
    eng.synchronize()
    pick = np.unique(np.linspace(0, lines - 1, 64).astype(np.int64))
    sub = S.cpu().numpy()
    sub = sub[pick] if axis == 0 else sub[:, pick]
    _same("4096 x 20000 axis %d" % axis, (os_.cpu().numpy()[pick], oi.cpu().numpy()[pick]), tm.top_n(sub, top, axis))
