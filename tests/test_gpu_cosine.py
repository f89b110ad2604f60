"""The cosine back-end (K27; plda_amd/csrc/cosine.hip, plda_amd/cosine.py) on the GPU.

A cosine handle reaches the trials GEMM through the same seam as a PLDA handle, so its fp32 scores are held to the same
yardstick: tests/cosine_model.py rebuilds the operands the prep kernel packs, tests/fp32_chain.py the GEMM's chain of fp32
fused multiply-adds, and a case passes when at least 99.9 % of the checked elements are bit-identical to that model, every
other one lies within fp32_chain.allowance, and every one within fp32_chain.budget of the fp64 value.  The trial lists are
held to bounds derived below.  Every test needs plda_backend_set, which the library did not have before K27.
Run with -s to see the per-case figures.
"""
import ctypes as C

import numpy as np
import pytest

import asnorm_model as am
import cosine_model as cm
import fp32_chain as fc

pytestmark = pytest.mark.gpu

LIMIT = 20000
ENV = ("PLDA_GEMM_VARIANT", "PLDA_PREP_VARIANT", "PLDA_SNORM_SLAB_ROWS", "PLDA_SCRATCH_POISON")
U53 = 2.0 ** -53


def _engine(monkeypatch, d, variant=None, prep=None, slab=None, poison=None, cls=None):
    for name, val in zip(ENV, (variant, prep, slab, poison)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    if cls is not None:
        return cls(0)
    from plda_amd import Cosine
    return Cosine(d)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _matrix_dev(eng, U, V, zm=None, zs=None, pad=0, fill=float("nan"), n_uniform=1, dV=None):
    """score_matrix_dev on fresh device copies -> the whole [M, Nt + pad] array, padding included."""
    import torch
    dU = _dev(U)
    dV = _dev(V) if dV is None else dV
    m, nt = U.shape[0], V.shape[0]
    o = torch.full((m, nt + pad), fill, dtype=torch.float32, device=dU.device)
    z = zm is not None
    dzm, dzs = (_dev(zm), _dev(zs)) if z else (None, None)
    torch.cuda.synchronize()
    eng.score_matrix_dev(dU.data_ptr(), None, n_uniform, m, dV.data_ptr(), nt, o.data_ptr(), nt + pad, dzm.data_ptr() if z else None,
                         dzs.data_ptr() if z else None)
    eng.synchronize()
    return o.cpu().numpy()


def _expect_kernel(variant, M, Nt, Kg):
    """launch_gemm's choice (score.hip) for a small-enough operand, as tests/test_gpu_score_model.py states it."""
    btM, btN = -(-M // 256), -(-Nt // 256)
    tiles = btM * btN
    nst = ((Kg // 4 >> 1) + 3) >> 2
    full = tiles >= 0.85 * (-(-btM // 4) * 4) * (-(-btN // 8) * 8)
    big = tiles >= 1700
    big2 = tiles >= 1700 or (tiles >= 512 and full)
    if nst >= 3 and (variant in (40, 48, 49) or (variant == 0 and big)):
        return "trials_gemm_bt4_kernel"
    if variant == 30 or (variant == 0 and big2):
        return "trials_gemm_bt2_kernel"
    return "trials_gemm_kernel"


def _verify(eng, got, op, label, variant=0):
    """The bit check of tests/test_gpu_score_model.py::_verify (without its score_tol line), and every element within budget."""
    M, N = got.shape
    pairs = fc.sample_pairs(M, N, LIMIT)
    kernel = _expect_kernel(variant, M, N, op.Kg)
    assert eng.score_last_kernel() == kernel, (label, eng.score_last_kernel(), kernel)
    last = eng.score_last_shape()
    assert last[2] == op.depth and last[:2] == (M, N), (label, last, op.depth)
    g = got[pairs]
    ex = fc.exact(op, pairs)
    allow = fc.allowance(op, pairs)
    model = fc.chain(op.A32, op.B32, pairs)
    ok, frac, ulp = fc.check(g, model, allow)
    err, bud = np.abs(g.astype(np.float64) - ex), fc.budget(op, pairs)
    over = np.where(bud > 0, err / np.where(bud > 0, bud, 1.0), np.where(err > 0, np.inf, 0.0))     # (a zero row: 0 of 0)
    print("\nCOS %-34s %-24s identical %.5f  max ulp %d  max |err| / budget %.3f  (%d elements)" % (label, kernel, frac, ulp, over.max(), len(g)))
    assert ok, "%s: %.5f of %d elements bit-identical, max %d ulp" % (label, frac, len(g), ulp)
    assert (over <= 1.0).all(), (label, float(over.max()))


def _set_zn(eng, zm, zs):
    """The statistics as the engine's dictionaries (rows with zstd = 0 have none: left raw); the ids of the rows."""
    ids = np.arange(len(zm), dtype=np.int64)
    eng._meanz = {int(k): float(zm[k]) for k in ids if zs[k] != 0.0}
    eng._stdvz = {int(k): float(zs[k]) for k in ids if zs[k] != 0.0}
    eng._zn_tag = None
    return ids


# ---------------------------------------------------------------- 1. matrix bits
@pytest.mark.parametrize("stats", [False, True], ids=["raw", "znorm"])
@pytest.mark.parametrize("shape", cm.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_matrix_bits(monkeypatch, shape, stats):
    M, Nt, D = shape
    U, V, zm, zs = cm.case(M, Nt, D, stats=stats)
    op = cm.operands(U, V, zm, zs)
    first = None
    for prep in (None, 2, 3):
        eng = _engine(monkeypatch, D, prep=prep)
        assert eng.dims() == (D, D) and eng.backend() == (1, D)
        if stats:
            ids = _set_zn(eng, zm, zs)
            host = eng.score_matrix((1, U, ids), (1, V))
        else:
            host = eng.score_matrix((1, U), (1, V))
        if first is None:
            first = host
            _verify(eng, host, op, "%dx%dx%d %s host" % (M, Nt, D, "zn" if stats else "raw"))
        dev = _matrix_dev(eng, U, V, zm, zs, pad=5, fill=-77.0, n_uniform=3)      # (a count is checked, then ignored)
        assert (dev[:, Nt:] == -77.0).all(), "padding columns written"
        assert eng.score_last_shape() == (M, Nt, D)
        for name, got in (("host", host), ("device", dev[:, :Nt])):
            assert np.array_equal(got.view(np.uint32), first.view(np.uint32)), "PLDA_PREP_VARIANT=%s %s entry: other bytes" % (prep, name)
    row = first[M // 2]
    assert np.array_equal(row, np.zeros(Nt, np.float32)) if not stats or zs[M // 2] == 0 else np.all(row == row[0])   # the zero row


# ---------------------------------------------------------------- 2. big tiles
@pytest.mark.parametrize("variant", [30, 40])
def test_big_tiles(monkeypatch, variant):
    M, Nt, D = 1024, 768, 200
    U, V, zm, zs = cm.case(M, Nt, D, stats=True)
    eng = _engine(monkeypatch, D, variant=variant)
    got = _matrix_dev(eng, U, V, zm, zs)
    assert eng.score_last_kernel() == {30: "trials_gemm_bt2_kernel", 40: "trials_gemm_bt4_kernel"}[variant]
    _verify(eng, got, cm.operands(U, V, zm, zs), "1024x768x200 variant %d" % variant, variant)


# ---------------------------------------------------------------- 3. one side at a time
def test_prepared_test_side(monkeypatch):
    M, Nt, D = 130, 257, 65
    U1, V, _, _ = cm.case(M, Nt, D, seed=1)
    U2 = cm.case(M + 7, Nt, D, seed=2)[0]
    eng = _engine(monkeypatch, D)
    want1, want2 = _matrix_dev(eng, U1, V), _matrix_dev(eng, U2, V)
    dV = _dev(V)
    eng.score_prepare_dev(dV.data_ptr(), Nt, n_uniform=4)
    got1, got2 = _matrix_dev(eng, U1, V, dV=dV), _matrix_dev(eng, U2, V, dV=dV)
    assert np.array_equal(got1.view(np.uint32), want1.view(np.uint32)) and np.array_equal(got2.view(np.uint32), want2.view(np.uint32))
    _verify(eng, got2, cm.operands(U2, V), "prepared test side")


def test_snorm_slabs_enrol_only_and_reuse(monkeypatch):
    import torch
    M, Nt, D = 300, 260, 64
    U, V, _, _ = cm.case(M, Nt, D, seed=3)
    rng = np.random.default_rng(9)
    em, es = rng.normal(0.0, 0.05, M), rng.uniform(0.05, 0.3, M)
    tm, ts = rng.normal(0.0, 0.05, Nt), rng.uniform(0.05, 0.3, Nt)
    es[::7] = 0.0
    ts[::5] = 0.0
    raw = _matrix_dev(_engine(monkeypatch, D), U, V)                   # the one-call matrix
    eng = _engine(monkeypatch, D, slab=128)                            # three slabs: the later ones pack the enrol side only
    dU, dV, o = _dev(U), _dev(V), torch.full((M, Nt + 3), 5.0, dtype=torch.float32, device="cuda:0")
    d = [_dev(a) for a in (em, es, tm, ts)]
    torch.cuda.synchronize()
    eng.score_matrix_snorm_dev(dU.data_ptr(), None, 1, M, dV.data_ptr(), Nt, o.data_ptr(), Nt + 3, *[t.data_ptr() for t in d])
    eng.synchronize()
    got = o.cpu().numpy()
    assert (got[:, Nt:] == 5.0).all()
    ref = am.snorm_apply(raw, em, es, tm, ts).astype(np.float32)
    same = got[:, :Nt].view(np.uint32) == ref.view(np.uint32)
    print("\nsnorm slabs: %.6f of %d elements equal the host map's bytes" % (same.mean(), same.size))
    assert same.all()
    # statistics (0, 1): the raw scores, bit for bit
    ident = [_dev(a) for a in (np.zeros(M), np.ones(M), np.zeros(Nt), np.ones(Nt))]
    eng.score_matrix_snorm_dev(dU.data_ptr(), None, 1, M, dV.data_ptr(), Nt, o.data_ptr(), Nt + 3, *[t.data_ptr() for t in ident])
    eng.synchronize()
    assert np.array_equal(o.cpu().numpy()[:, :Nt].view(np.uint32), raw.view(np.uint32))


def test_batch_equals_rows_one_at_a_time(monkeypatch):
    import torch
    M, Nt, D = 300, 33, 200
    U, V, zm, zs = cm.case(M, Nt, D, seed=4, stats=True)
    eng = _engine(monkeypatch, D)
    batch = _matrix_dev(eng, U, V, zm, zs)
    dU, dV, dzm, dzs = _dev(U), _dev(V), _dev(zm), _dev(zs)
    o = torch.empty((M, Nt), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    for i in range(M):
        eng.score_matrix_dev(dU[i].data_ptr(), None, 1, 1, dV.data_ptr(), Nt, o[i].data_ptr(), Nt, dzm[i:].data_ptr(), dzs[i:].data_ptr())
    eng.synchronize()
    assert np.array_equal(o.cpu().numpy().view(np.uint32), batch.view(np.uint32))


# ---------------------------------------------------------------- 4. containment
def test_nan_stays_in_its_row_or_column(monkeypatch):
    M, Nt, D = 65, 130, 64
    U, V, zm, zs = cm.case(M, Nt, D, seed=5, stats=True)
    eng = _engine(monkeypatch, D)
    clean = _matrix_dev(eng, U, V, zm, zs)
    Ub = U.copy()
    Ub[17, 40] = np.nan
    got = _matrix_dev(eng, Ub, V, zm, zs)
    assert np.isnan(got[17]).all()
    keep = np.arange(M) != 17
    assert np.array_equal(got[keep].view(np.uint32), clean[keep].view(np.uint32))
    Vb = V.copy()
    Vb[101, 3] = np.nan
    got = _matrix_dev(eng, U, Vb, zm, zs)
    assert np.isnan(got[:, 101]).all()
    keep = np.arange(Nt) != 101
    assert np.array_equal(got[:, keep].view(np.uint32), clean[:, keep].view(np.uint32))


# ---------------------------------------------------------------- 5. every consumer: operand form == matrix form
@pytest.fixture()
def consumer_case(monkeypatch):
    import torch
    M, Nt, D = 300, 260, 64
    rng = np.random.default_rng(21)
    centres = rng.standard_normal((10, D))
    espk = np.arange(M, dtype=np.int64) % 10
    tspk = rng.integers(0, 10, Nt).astype(np.int64)             # about 10 % targets
    U = centres[espk] + 1.5 * rng.standard_normal((M, D))
    V = centres[tspk] + 1.5 * rng.standard_normal((Nt, D))
    eng = _engine(monkeypatch, D)
    t = dict(U=_dev(U), V=_dev(V), es=_dev(espk), ts=_dev(tspk))
    S = torch.empty((M, Nt), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    eng.score_matrix_dev(t["U"].data_ptr(), None, 1, M, t["V"].data_ptr(), Nt, S.data_ptr(), Nt)
    eng.synchronize()
    return eng, M, Nt, D, U, V, espk, tspk, t, S


def test_consumers_equal_their_matrix_forms(consumer_case):
    import torch
    from plda_amd import dcf, eer, trialkey as TK
    eng, M, Nt, D, U, V, espk, tspk, t, S = consumer_case
    pU, pV, pe, pt = (t[k].data_ptr() for k in ("U", "V", "es", "ts"))
    a = eer.eer_from_operands_dev(eng, pU, None, 1, M, pV, Nt, pe, pt)
    b = eer.eer_from_matrix_dev(eng, S.data_ptr(), Nt, M, Nt, pe, pt)
    assert np.array_equal(a, b) and 0.0 < a[3] < 0.5 and a[4] + a[5] == M * Nt, (a, b)
    pts = ((0.01, 1.0, 1.0), (0.05, 1.0, 1.0))
    a = dcf.min_dcf_from_operands_dev(eng, pU, None, 1, M, pV, Nt, pe, pt, points=pts)[0]
    b = dcf.min_dcf_from_matrix_dev(eng, S.data_ptr(), Nt, M, Nt, pe, pt, points=pts)[0]
    assert a == b, (a, b)
    for axis, lines in ((0, M), (1, Nt)):
        outs = [(torch.empty((lines, 5), dtype=torch.float32, device="cuda:0"), torch.empty((lines, 5), dtype=torch.int64, device="cuda:0"))
                for _ in range(2)]
        eng.score_topn_dev(pU, None, 1, M, pV, Nt, axis, 5, outs[0][0].data_ptr(), outs[0][1].data_ptr())
        eng.topn_matrix_dev(S.data_ptr(), Nt, M, Nt, axis, 5, outs[1][0].data_ptr(), outs[1][1].data_ptr())
        eng.synchronize()
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), axis
    key = TK.TrialKey(np.arange(M) % 2, np.arange(Nt) % 3 % 2, "same")
    pa = TK.partition_from_operands_dev(eng, key, t["U"], None, 1, t["V"], t["es"], t["ts"])
    pb = TK.partition_matrix_dev(eng, key, S, t["es"], t["ts"])
    eng.synchronize()
    assert pa.record.tobytes() == pb.record.tobytes() and sum(pa.totals) > 0
    nt_, nn_ = pa.totals
    assert torch.equal(pa.dtar[:nt_], pb.dtar[:nt_]) and torch.equal(pa.dnon[:nn_], pb.dnon[:nn_])


def test_cohort_stats_against_the_model(consumer_case):
    eng, M, Nt, D, U, V, espk, tspk, t, S = consumer_case
    S32 = eng.score_matrix((1, U), (1, V), znorm=False)              # V as the cohort
    for K in (20, Nt):
        mean, std = eng.cohort_stats((3, U), V, top_k=K)
        ref_m, ref_s = am.topk_stats(S32, K)
        tol_m, tol_s = am.stats_tolerance(S32, K, ref_m, ref_s)
        dm, ds = np.abs(mean - ref_m), np.abs(std - ref_s)
        print("\ncohort stats K = %d: max |dmean| / bound %.3g, max |dstd| / bound %.3g" % (K, (dm / tol_m).max(), (ds / tol_s).max()))
        assert np.isfinite(mean).all() and np.isfinite(std).all()
        assert (dm <= tol_m).all() and (ds <= tol_s).all()


def test_score_ahc_equals_ahc_on_the_cosine_blocks(monkeypatch):
    import torch
    D, sizes = 64, (5, 40, 130)
    rng = np.random.default_rng(31)
    X = np.concatenate([rng.standard_normal((3, D))[rng.integers(0, 3, n)] + 0.8 * rng.standard_normal((n, D)) for n in sizes])
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    T, R = int(offsets[-1]), len(sizes)
    eng = _engine(monkeypatch, D)
    dX = _dev(X)
    out = [(torch.full((T,), -1, dtype=torch.int32, device="cuda:0"), torch.full((R,), -1, dtype=torch.int32, device="cuda:0")) for _ in range(2)]
    blocks = []
    torch.cuda.synchronize()
    for r, n in enumerate(sizes):
        b = torch.empty((n, n), dtype=torch.float32, device="cuda:0")
        p = dX[int(offsets[r])].data_ptr()
        eng.score_matrix_dev(p, None, 1, n, p, n, b.data_ptr(), n)
        blocks.append(b.ravel())
    eng.synchronize()
    scores = torch.cat(blocks)
    block_off = np.concatenate([[0], np.cumsum([n * n for n in sizes])]).astype(np.int64)
    eng.score_ahc_dev(dX.data_ptr(), offsets, 1, 0.3, None, out[0][0].data_ptr(), out[0][1].data_ptr())
    eng.ahc_matrix_dev(scores.data_ptr(), block_off, offsets, 1, 0.3, None, out[1][0].data_ptr(), out[1][1].data_ptr())
    eng.synchronize()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    ncl = out[0][1].cpu().numpy()
    assert (ncl >= 1).all() and (ncl <= np.array(sizes)).all() and ncl[2] < 130


# ---------------------------------------------------------------- 6. trial lists
@pytest.mark.parametrize("P", [1, 1000, 20000])
@pytest.mark.parametrize("D", [7, 200, 513])
def test_trial_lists(monkeypatch, D, P):
    """Bounds, derived.  c = (u . v) inv(u) inv(v): the dot product of D terms carries at most D 2^-53 sum |u_d v_d| <=
    D 2^-53 |u| |v| (Cauchy-Schwarz), each sum of squares D 2^-53 relative and its inverse square root three more roundings
    (sqrt, division; half of the sum's error), the two products two more: |c_dev - c| <= (D + 2 (D / 2 + 3) + 2) 2^-53 =
    (2 D + 8) 2^-53 for |c| <= 1.  The map (c - zmean) / zstd is a subtraction and a division: two roundings of at most
    2^-53 (|c| + |zmean|) / zstd each, twice that allowed."""
    M, Nt = (1, 1) if P == 1 else (40, 50)
    U, V, zm, zs = cm.case(M, Nt, D, seed=6, stats=True)
    if P == 1:
        U = cm.case(3, 1, D, seed=6)[0][:1]                       # (row M / 2 = 0 would be the zero row,
        zs[0] = 0.125                                             #  and row 0 the one without statistics)
    rng = np.random.default_rng(P + D)
    e, t = rng.integers(0, M, P), rng.integers(0, Nt, P)
    eng = _engine(monkeypatch, D)
    counts = np.full(M, 2, np.int32)
    c_dev = eng.score_trials((counts, U), (1, V), e, t, znorm=False)
    want, c = cm.pairs(U, V, e, t, zm, zs)
    err = np.abs(c_dev.astype(np.longdouble) - c).astype(np.float64)
    print("\npairs D %d P %d: max |device - longdouble| / bound = %.3f" % (D, P, err.max() / ((2 * D + 8) * U53)))
    assert (err <= (2 * D + 8) * U53).all()
    if M > 1:
        zero = e == M // 2
        assert zero.any() and (c_dev[zero] == 0.0).all()           # a pair with a zero row scores 0
    ids = _set_zn(eng, zm, zs)
    z_dev = eng.score_trials((counts, U, ids), (1, V), e, t, znorm=True)
    has = zs[e] != 0.0
    host = np.where(has, (c_dev - zm[e]) / np.where(has, zs[e], 1.0), c_dev)
    bound = np.where(has, 4 * U53 * (np.abs(c_dev) + np.abs(zm[e])) / np.where(has, zs[e], 1.0), 0.0)
    assert (np.abs(z_dev - host) <= bound).all(), float(np.abs(z_dev - host).max())
    # one trial on the host (plda_score_one), the same bounds
    for p in range(min(P, 25)):
        i, j = int(e[p]), int(t[p])
        eng._meanz, eng._stdvz = {}, {}
        one = eng.score(i, (2, U[i]), (1, V[j]))
        assert abs(float(np.longdouble(one) - c[p])) <= (2 * D + 8) * U53
        if zs[i] != 0.0:
            eng._meanz, eng._stdvz = {i: float(zm[i])}, {i: float(zs[i])}
            onez = eng.score(i, (2, U[i]), (1, V[j]))
            assert abs(onez - (one - zm[i]) / zs[i]) <= 4 * U53 * (abs(one) + abs(zm[i])) / zs[i]
    if P == 1:
        eng._meanz, eng._stdvz = {}, {}
        assert eng.score_on_device(0, (2, U[0]), (1, V[0])) == c_dev[0]      # the mapped-host path, the same kernel


def test_trial_list_indices_are_validated(monkeypatch):
    from plda_amd._native import PldaError
    D = 7
    U, V, _, _ = cm.case(40, 50, D)
    eng = _engine(monkeypatch, D)
    for P in (100, 20000):
        e, t = np.zeros(P, np.int64), np.zeros(P, np.int64)
        t[P - 3] = 50
        with pytest.raises(PldaError) as ei:
            eng.score_trials((np.ones(40, np.int32), U), (1, V), e, t)
        assert ei.value.code == -1 and "trial %d" % (P - 3) in ei.value.message


# ---------------------------------------------------------------- 7. state
def _plda_model(D, seed=0):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    return rng.random(D), q * (1.0 + rng.random(D))[:, None], np.sort(0.05 + 4 * rng.random(D))[::-1].copy()


def test_refusals_and_dims(monkeypatch):
    from plda_amd import MPlda
    from plda_amd._native import PldaError
    D = 24
    eng = _engine(monkeypatch, D)
    lib, h = eng._lib, eng._h
    assert eng.dims() == (D, D) and eng.backend() == (1, D)
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal((60, D)), (np.arange(60) % 6).astype(np.uint64)
    mean, T, psi = _plda_model(D)

    def refused(code, text, fn, *a, **kw):
        with pytest.raises(PldaError) as ei:
            fn(*a, **kw)
        assert ei.value.code == code and text in ei.value.message, (fn, ei.value.code, ei.value.message)

    # what installs a model: PLDA_E_INVAL, and the message says why
    refused(-1, "cosine back-end", MPlda.fit, eng, x, y)
    refused(-1, "cosine back-end", MPlda.set_model, eng, mean, T, psi)
    dx, dy = _dev(x), _dev(y.view(np.int64))
    refused(-1, "cosine back-end", eng.fit_dev, dx.data_ptr(), 60, D, dy.data_ptr(), 6)
    refused(-1, "cosine back-end", eng.fit_sharded_dev, dx.data_ptr(), 60, D, dy.data_ptr(), 6)
    # what needs the model proper: PLDA_E_NOT_FITTED, and the wrapper's one sentence
    why = "(cosine back-end selected: this entry point needs a PLDA model)"
    refused(-4, why, MPlda.transform, eng, x, y)
    refused(-4, why, MPlda.transform_array, eng, x, 1)
    refused(-4, why, eng.get_model)
    refused(-4, why, eng.truncate, 8)
    refused(-4, why, eng.smooth, 0.5)
    refused(-4, why, eng.project_rows, x)
    refused(-4, why, MPlda.norm, eng, x, {0: (1, x[0])})
    refused(-4, why, eng.adapt_accumulate, x)
    refused(-4, why, MPlda.score_dense, eng, x, np.array([0, 60]), 0.5)
    assert eng.dims() == (D, D)
    with pytest.raises(ValueError, match="PLDA model"):
        eng.fit(x, y)
    # the switch itself
    assert lib.plda_backend_set(h, 2, D) == -1 and lib.plda_backend_set(h, 1, 0) == -1 and lib.plda_backend_set(h, 1, 2049) == -1
    assert lib.plda_backend_set(h, 0, D) == -1 and lib.plda_backend_set(h, -1, 0) == -1
    assert eng.backend() == (1, D)
    m = MPlda(0)
    m.set_model(mean, T, psi)
    assert lib.plda_backend_set(m._h, 1, D) == -1                      # cosine after set_model
    assert "PLDA model" in m._lib.plda_last_error(m._h).decode()
    k, d = C.c_int32(-1), C.c_int32(-1)
    assert lib.plda_backend_get(m._h, C.byref(k), C.byref(d)) == 0 and (k.value, d.value) == (0, 0)
    assert lib.plda_backend_set(m._h, 0, 0) == 0 and m.dims() == (D, D)  # a PLDA handle stays as it is


def test_back_to_plda_scores_like_a_fresh_handle(monkeypatch):
    from plda_amd import MPlda
    D, M, Nt = 65, 130, 257
    U, V, _, _ = cm.case(M, Nt, D, seed=7)
    mean, T, psi = _plda_model(D, 3)
    fresh = _engine(monkeypatch, D, cls=MPlda)
    fresh.set_model(mean, T, psi)
    want = _matrix_dev(fresh, U, V, n_uniform=2)
    eng = _engine(monkeypatch, D)
    cos = _matrix_dev(eng, U, V, n_uniform=2)
    dV = _dev(V)
    eng.score_prepare_dev(dV.data_ptr(), Nt, n_uniform=2)              # a cosine test side, prepared before the switch
    eng._ck(eng._lib.plda_backend_set(eng._h, 0, 0))
    with pytest.raises(Exception):
        eng.dims()                                                     # the empty PLDA state
    MPlda.set_model(eng, mean, T, psi)
    got = _matrix_dev(eng, U, V, n_uniform=2, dV=dV)                   # same pointer, same size, same count: not reused
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got, cos)
    assert eng.score_last_shape() == (M, Nt, D)


def test_scratch_poison_leaves_the_matrix_unchanged(monkeypatch):
    M, Nt, D = 130, 257, 65
    U, V, zm, zs = cm.case(M, Nt, D, stats=True)
    poisoned = _engine(monkeypatch, D, poison=1)
    got = _matrix_dev(poisoned, U, V, zm, zs)
    del poisoned
    clean = _engine(monkeypatch, D)                                    # (the switch is process-wide: the latest plda_create's)
    want = _matrix_dev(clean, U, V, zm, zs)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    _verify(clean, want, cm.operands(U, V, zm, zs), "after a poisoned handle")


# ---------------------------------------------------------------- 8. Python
def _speakers(rng, D, n_spk, per, spread=0.5):
    centres = rng.standard_normal((n_spk, D))
    y = np.repeat(np.arange(n_spk), per)
    return centres[y] + spread * rng.standard_normal((len(y), D)), y.astype(np.uint64)


def test_transform_is_the_mean_of_unit_rows(monkeypatch):
    D = 48
    rng = np.random.default_rng(41)
    sessions = np.array([1, 2, 3, 4, 2, 1, 4, 3])
    y = np.repeat(np.arange(len(sessions)) * 3 + 5, sessions).astype(np.uint64)
    perm = rng.permutation(len(y))
    y = y[perm]
    x = rng.standard_normal((len(y), D)) * rng.uniform(0.2, 9.0, (len(y), 1))
    eng = _engine(monkeypatch, D)
    tv = eng.transform(x, y)
    assert list(tv) == sorted(set(y.tolist()))
    unit = x / np.linalg.norm(x, axis=1, keepdims=True)
    for k, (n, vec) in tv.items():
        rows = unit[y == k]
        assert n == len(rows) and np.abs(vec - rows.mean(0)).max() <= 1e-12
    ids, counts, vecs = eng._unpack(tv)
    assert counts.tolist() == [int((y == k).sum()) for k in ids] and vecs.shape == (len(sessions), D)


def test_norm_then_znorm_scores(monkeypatch):
    D = 64
    rng = np.random.default_rng(43)
    x, y = _speakers(rng, D, 12, 3)
    tx, ty = _speakers(rng, D, 12, 2)
    cohort = rng.standard_normal((150, D))
    eng = _engine(monkeypatch, D)
    enrol, test = eng.transform(x, y), eng.transform(tx, np.arange(len(ty)).astype(np.uint64))
    assert eng.norm(cohort, enrol) is None
    zmd, zsd = eng.znorm_stats()
    ids, _, U = eng._unpack(enrol)
    V = eng._unpack(test)[2]
    zm, zs = np.array([zmd[int(k)] for k in ids]), np.array([zsd[int(k)] for k in ids])
    cc = cm.cosine_matrix(U, cohort)
    assert np.abs(zm - cc.mean(1)).max() <= 1e-6 and np.abs(zs - cc.std(1)).max() <= 1e-6      # fp32 scores behind the statistics
    got = eng.score_matrix(enrol, test, znorm=True)
    op = cm.operands(U, V, zm, zs)
    pairs = fc.sample_pairs(len(U), len(V), LIMIT)
    zn = ((cm.cosine_matrix(U, V) - zm[:, None]) / zs[:, None])[pairs]
    # the budget is about the operands' own fp64 value, which carries s_i = fp32(1 / zstd_i): one more 2^-24 on the cosine term
    slack = 2.0 ** -23 * (np.abs(cm.cosine_matrix(U, V)) / zs[:, None])[pairs]
    assert (np.abs(got[pairs].astype(np.float64) - zn) <= fc.budget(op, pairs) + slack).all()
    raw = eng.score_matrix(enrol, test, znorm=False)
    assert np.abs(raw - cm.cosine_matrix(U, V)).max() <= 1e-5


def test_inherited_methods_agree_with_the_resident_matrix(monkeypatch):
    import torch
    from plda_amd import calibration as CB, trialkey as TK
    D = 64
    rng = np.random.default_rng(47)
    centres = rng.standard_normal((15, D))
    ye = np.arange(15).astype(np.uint64)
    x = centres + 0.6 * rng.standard_normal((15, D))
    tspk = rng.integers(0, 15, 120)
    tx = centres[tspk] + 2.5 * rng.standard_normal((120, D))
    cohort = rng.standard_normal((90, D))
    eng = _engine(monkeypatch, D)
    enrol, test = eng.transform(x, ye), eng.transform(tx, np.arange(120).astype(np.uint64))
    ids, counts, U = eng._unpack(enrol)
    V = eng._unpack(test)[2]
    raw = eng.score_matrix(enrol, test, znorm=False)
    # AS-norm: the host map of asnorm_model on the raw matrix, to the rounding tests/test_gpu_asnorm.py holds the PLDA form to
    em, es = eng.cohort_stats(enrol, cohort, top_k=20)
    tm, ts = eng.cohort_stats(test, cohort, top_k=20)
    got = eng.score_matrix_asnorm(enrol, test, cohort, top_k=20)
    ref = am.snorm_apply(raw, em, es, tm, ts)
    se, st = am.snorm_sides(raw, em, es, tm, ts)
    assert (np.abs(got.astype(np.float64) - ref) <= am.ulp32(ref) + 2.0 ** -50 * (np.abs(se) + np.abs(st))).all()
    # top-N: the selection on the resident matrix
    S = _dev(raw)
    sc, who = eng.top_n(enrol, test, n=5, per="test", znorm=False)
    o = (torch.empty((120, 5), dtype=torch.float32, device="cuda:0"), torch.empty((120, 5), dtype=torch.int64, device="cuda:0"))
    torch.cuda.synchronize()
    eng.topn_matrix_dev(S.data_ptr(), 120, 15, 120, 1, 5, o[0].data_ptr(), o[1].data_ptr())
    eng.synchronize()
    assert np.array_equal(sc, o[0].cpu().numpy()) and np.array_equal(who, ids[o[1].cpu().numpy()])
    assert (who[:, 0] == tspk).mean() > 0.5                               # and it identifies
    # evaluate under a two-bucket key, calibrate: the matrix forms on the resident matrix
    key = TK.TrialKey(np.arange(15) % 2, np.arange(120) % 2, "same")
    res = eng.evaluate(enrol, test, tspk, key, znorm=False)
    des, dts = _dev(np.ascontiguousarray(ids, np.int64)), _dev(tspk.astype(np.int64))
    res2 = TK.metrics(eng, TK.partition_matrix_dev(eng, key, S, des, dts))
    assert res == res2 and len(res["buckets"]) == 2 and 0.0 <= res["pooled"]["eer"] < 0.3
    cal = eng.calibrate(enrol, test, tspk, znorm=False)
    cal2 = CB.fit_from_matrix_dev(eng, S.data_ptr(), 120, 15, 120, des.data_ptr(), dts.data_ptr())
    assert np.isclose(cal.a, cal2.a, rtol=1e-9, atol=0) and np.isclose(cal.b, cal2.b, rtol=1e-9, atol=1e-12) and cal.a > 0
    mapped = eng.score_matrix(enrol, test, znorm=False, calibrate=True)
    assert np.abs(mapped - (cal.a * raw.astype(np.float64) + cal.b)).max() <= 1e-5 * (abs(cal.a) + abs(cal.b))


@pytest.mark.parametrize("method", ["ahc", "spectral"])
def test_cluster_separates_two_speakers(monkeypatch, method):
    """Two speakers whose directions are orthogonal (90 degrees > 60), segments within 15 degrees of their speaker's: a
    cosine above 0.5 within a speaker, below it across."""
    D = 64
    rng = np.random.default_rng(53)
    dirs = np.linalg.qr(rng.standard_normal((D, 2)))[0].T
    sizes = (40, 64)
    truth, rows = [], []
    for n in sizes:
        spk = np.concatenate([[0, 1], rng.integers(0, 2, n - 2)])       # labels count from the smallest member
        noise = rng.standard_normal((n, D))
        noise -= (noise @ dirs.T) @ dirs
        noise *= np.tan(np.radians(15)) * rng.random((n, 1)) / np.linalg.norm(noise, axis=1, keepdims=True)
        rows.append((dirs[spk] + noise) * rng.uniform(0.5, 20.0, (n, 1)))
        truth.append(spk)
    x, offsets = np.concatenate(rows), np.array([0, 40, 104])
    eng = _engine(monkeypatch, D)
    if method == "ahc":
        labels, ncl = eng.cluster(x, offsets, threshold=0.5)
    else:
        labels, ncl = eng.cluster(x, offsets, method="spectral")
    assert ncl.tolist() == [2, 2] and np.array_equal(labels, np.concatenate(truth))


def test_save_load_round_trip(monkeypatch, tmp_path):
    D = 32
    rng = np.random.default_rng(59)
    x, y = _speakers(rng, D, 8, 10)
    eng = _engine(monkeypatch, D)
    enrol = eng.transform(x, y)
    eng.norm(rng.standard_normal((50, D)), enrol)
    from plda_amd.calibration import Calibration
    eng._calibration = Calibration(1.5, -0.25, 0.5)
    eng.fit_embedding(x, y, kind="wccn")
    assert eng.embedding.dout == D
    eng.save(tmp_path / "cos")
    other = _engine(monkeypatch, D)
    assert other.load(tmp_path / "cos") is other
    assert other.znorm_stats() == eng.znorm_stats() and (other.calibration.a, other.calibration.b) == (1.5, -0.25)
    assert np.array_equal(other.embedding.A, eng.embedding.A)
    v = rng.standard_normal((9, D))
    eng.set_embedding(None)
    other.set_embedding(None)
    assert np.array_equal(other.score_matrix(enrol, (1, v)), eng.score_matrix(enrol, (1, v)))
    from plda_amd import Cosine, MPlda
    with pytest.raises(ValueError):
        Cosine(D + 1).load(tmp_path / "cos")
    with pytest.raises(Exception):
        MPlda(0).load(tmp_path / "cos")
