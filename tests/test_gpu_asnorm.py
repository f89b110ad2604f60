"""GPU: adaptive symmetric score normalisation (csrc/snorm.hip; include/plda_hip.h "S-norm / adaptive S-norm").

  1. cohort statistics against the exact definition: topk_stats (tests/asnorm_model.py) of the fp32 scores that
     score_matrix_dev writes for the same inputs, within the DERIVED bounds of asnorm_model.stats_tolerance (fp64 sums of K
     fp32 values); exactly (std == 0, mean == the value) where a row's top-K values are all equal; bit-identical between
     slab heights and between two calls;
  2. the same statistics against the fp64 oracle's scores, within the project's score band carried through the Lipschitz
     facts of tests/test_asnorm_model.py;
  3. the two-sided map's rounding contract: fp64 evaluation of the finished fp32 score, one rounding to fp32;
  4. liblda.PLDA.score_matrix_asnorm / score_trials_asnorm end to end against the oracle's fp64 AS-norm;
  5. the large shape (50 000 x 200 000), sampled, with the slab cap asserted through plda_device_bytes_peak;
  6. API edges; 7. guard bands, poisoned scratch, leaks; 8. rows sharded over emulated ranks.

Run with -s to see the measured figures next to each bound.  Nothing here provokes a fault: stray accesses would land in
memory the test owns."""

import numpy as np
import pytest

import asnorm_model as am
from conftest import score_tol

pytestmark = pytest.mark.gpu

ENV = ("PLDA_SNORM_SLAB_ROWS", "PLDA_SCRATCH_POISON", "PLDA_MIXED_VARIANT")


def _dev():
    import torch
    return torch.device("cuda", 0)


def _psi(d, seed=3, lo=0.05, hi=4.05, log=False):
    rng = np.random.default_rng(seed)
    p = np.exp(rng.uniform(np.log(lo), np.log(hi), d)) if log else lo + rng.random(d) * (hi - lo)
    return np.sort(p)[::-1].copy()


def _engine(monkeypatch, d, psi=None, slab=None, poison=False):
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
    rng = np.random.default_rng(d)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    eng.set_model(rng.random(d), q * (1.0 + rng.random(d))[:, None], _psi(d) if psi is None else psi)
    return eng


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _scores(eng, U, n, V):
    """fp32 [M, Nt] of plda_score_matrix_dev without statistics (n: int, or int32 array)."""
    import torch
    dU, dV = _t(U), _t(V)
    dn = None if np.isscalar(n) else _t(np.asarray(n, np.int32))
    out = torch.empty((U.shape[0], V.shape[0]), dtype=torch.float32, device=_dev())
    eng.score_matrix_dev(dU.data_ptr(), dn.data_ptr() if dn is not None else None, int(n) if np.isscalar(n) else 0, U.shape[0],
                         dV.data_ptr(), V.shape[0], out.data_ptr(), V.shape[0])
    eng.synchronize()
    return out.cpu().numpy()


def _stats(eng, X, n, Cv, K):
    import torch
    dX, dC = _t(X), _t(Cv)
    dn = None if np.isscalar(n) else _t(np.asarray(n, np.int32))
    res = torch.full((2, X.shape[0]), float("nan"), dtype=torch.float64, device=_dev())
    eng.cohort_stats_dev(dX.data_ptr(), dn.data_ptr() if dn is not None else None, int(n) if np.isscalar(n) else 0, X.shape[0],
                         dC.data_ptr(), Cv.shape[0], K, res[0].data_ptr(), res[1].data_ptr())
    eng.synchronize()
    r = res.cpu().numpy()
    return r[0].copy(), r[1].copy()


def _counts(kind, r, rng):
    if kind == "uniform":
        return 3
    if kind == "two":
        return rng.choice(np.array([2, 5], np.int32), r).astype(np.int32)
    n = rng.choice(np.array([1, 3, 5000], np.int32), r).astype(np.int32)       # a count above 4095: the depth-2D form
    n[0] = 5000
    return n


def _expected_depth(kind, d, n):
    if kind == "uniform" or len(np.unique(n)) == 1:
        return d
    return d + len(np.unique(n)) - 1 if kind == "two" else 2 * d


def _check_exact(label, S32, K, mean, std):
    ref_m, ref_s = am.topk_stats(S32, K)
    tol_m, tol_s = am.stats_tolerance(S32, K, ref_m, ref_s)
    dm, ds = np.abs(mean - ref_m), np.abs(std - ref_s)
    w = am.topk_width(S32, K)
    flat = w == 0
    print("%s: K = %d, rows %d (all-equal top-K: %d); max |dmean| / bound = %.3g, max |dstd| / bound = %.3g" % (
        label, K, S32.shape[0], int(flat.sum()),
        float((dm[~flat] / tol_m[~flat]).max()) if (~flat).any() else 0.0,
        float((ds[~flat] / tol_s[~flat]).max()) if (~flat).any() else 0.0))
    assert np.isfinite(mean).all() and np.isfinite(std).all(), label
    assert (dm <= tol_m).all(), (label, float(dm.max()))
    assert (ds <= tol_s).all(), (label, float(ds.max()))
    assert np.array_equal(mean[flat], ref_m[flat]) and (std[flat] == 0.0).all(), label


def _ks(nc):
    return sorted({min(k, nc) for k in (1, 2, 300, nc - 1, nc) if min(k, nc) >= 1})


# ------------------------------------------------------------------------------------------- 1. statistics, exact
CASES = [
    # d, Nc, R, counts
    (48, 1, 130, "uniform"), (48, 63, 1, "two"), (48, 1000, 1025, "uniform"), (200, 4097, 130, "two"),
    (200, 20011, 130, "uniform"), (257, 1000, 130, "big"), (257, 4097, 1, "uniform"), (200, 1000, 1025, "big"),
    (48, 20011, 130, "two"),
]


@pytest.mark.parametrize("d,nc,r,kind", CASES)
def test_statistics_match_the_definition(monkeypatch, d, nc, r, kind):
    rng = np.random.default_rng(d + nc + r)
    X, Cv = rng.standard_normal((r, d)), rng.standard_normal((nc, d))
    n = _counts(kind, r, rng)
    eng = _engine(monkeypatch, d)
    small = _engine(monkeypatch, d, slab=128)
    S32 = _scores(eng, X, n, Cv)
    assert eng.score_last_shape()[2] == _expected_depth(kind, d, n)
    for K in _ks(nc):
        mean, std = _stats(eng, X, n, Cv, K)
        assert eng.score_last_shape() == (r, nc, _expected_depth(kind, d, n))
        _check_exact("D %d Nc %d R %d %s" % (d, nc, r, kind), S32, K, mean, std)
        again = _stats(eng, X, n, Cv, K)
        assert np.array_equal(mean, again[0]) and np.array_equal(std, again[1])            # two calls: bit-identical
        m2, s2 = _stats(small, X, n, Cv, K)
        assert np.array_equal(mean, m2) and np.array_equal(std, s2)                        # slabs of 128 rows: bit-identical


@pytest.mark.parametrize("what", ["tripled", "identical", "psi_extreme", "zeros", "clustered"])
def test_statistics_ties_and_extremes(monkeypatch, what):
    d, r, nc = 200, 130, 1500
    rng = np.random.default_rng(5)
    X, Cv = rng.standard_normal((r, d)), rng.standard_normal((nc, d))
    psi = None
    if what == "tripled":                     # every cohort vector three times: ties at every boundary
        Cv = np.repeat(Cv[:nc // 3], 3, axis=0)[rng.permutation(nc // 3 * 3)]
    elif what == "identical":                 # all scores of a row equal: std exactly 0 for every K
        Cv = np.repeat(Cv[:1], nc, axis=0)
    elif what == "psi_extreme":
        psi = _psi(d, lo=1e-6, hi=1e4, log=True)
    elif what == "zeros":                     # rows of zeros: the GEMM part of their scores vanishes, the biases remain
        X[::2] = 0.0
        Cv = Cv / np.linalg.norm(Cv, axis=1, keepdims=True)
    elif what == "clustered":                 # the closest cohort vectors sit side by side in the first 3000 of 20 011 columns:
        x0 = rng.standard_normal(d)           # the share of the row that one wave compacts holds more candidates than its list
        X = x0 + 0.05 * rng.standard_normal((r, d))
        Cv = np.concatenate([x0 + 0.05 * rng.standard_normal((3000, d)), rng.standard_normal((17011, d))])
    nc = Cv.shape[0]
    eng = _engine(monkeypatch, d, psi=psi)
    small = _engine(monkeypatch, d, psi=psi, slab=128)
    for n in (1, _counts("two", r, rng)):
        S32 = _scores(eng, X, n, Cv)
        if what == "clustered":
            assert (np.argsort(S32, axis=1)[:, -2000:] < 3000).all()
        for K in _ks(nc) + ([1500, 2000, 2900] if what == "clustered" else [4, 5, 6]):
            mean, std = _stats(eng, X, n, Cv, K)
            _check_exact(what, S32, K, mean, std)
            if what == "identical":
                assert (std == 0.0).all() and np.array_equal(mean, S32[:, 0].astype(np.float64))
            m2, s2 = _stats(small, X, n, Cv, K)
            assert np.array_equal(mean, m2) and np.array_equal(std, s2)


# ------------------------------------------------------------------------------------------- 2. against the fp64 oracle
@pytest.mark.parametrize("d,nc,r,kind", [(48, 1000, 130, "two"), (200, 4097, 130, "uniform"), (257, 1000, 130, "big")])
def test_statistics_against_the_fp64_oracle(monkeypatch, oracle, d, nc, r, kind):
    rng = np.random.default_rng(d + nc)
    X, Cv = rng.standard_normal((r, d)), rng.standard_normal((nc, d))
    n = _counts(kind, r, rng)
    eng = _engine(monkeypatch, d)
    S_ref = oracle.score_block(eng.get_model()["psi"], X, n, Cv)
    eps = score_tol(S_ref).max(axis=1)
    for K in _ks(nc):
        mean, std = _stats(eng, X, n, Cv, K)
        top = np.sort(S_ref, axis=1)[:, ::-1][:, :K]
        dm, ds = np.abs(mean - top.mean(axis=1)), np.abs(std - top.std(axis=1))
        print("oracle D %d Nc %d %s K %d: max |dmean| / eps = %.3g, max |dstd| / eps = %.3g" % (d, nc, kind, K, (dm / eps).max(), (ds / eps).max()))
        assert (dm <= eps).all() and (ds <= eps).all()


# ------------------------------------------------------------------------------------------- 3. apply, rounding contract
def _snorm(eng, U, n, V, em, es, tm, ts, ld=None, fill=None):
    import torch
    m, nt = U.shape[0], V.shape[0]
    ld = ld or nt
    dU, dV = _t(U), _t(V)
    dn = None if np.isscalar(n) else _t(np.asarray(n, np.int32))
    dv = [None if a is None else _t(np.asarray(a, np.float64)) for a in (em, es, tm, ts)]
    out = torch.full((m, ld), float("nan") if fill is None else fill, dtype=torch.float32, device=_dev())
    eng.score_matrix_snorm_dev(dU.data_ptr(), dn.data_ptr() if dn is not None else None, int(n) if np.isscalar(n) else 0, m,
                               dV.data_ptr(), nt, out.data_ptr(), ld, *[None if a is None else a.data_ptr() for a in dv])
    eng.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("sides", ["both", "enrol", "test"])
@pytest.mark.parametrize("d,m,nt,ld,kind", [(48, 300, 517, 517, "uniform"), (200, 1025, 777, 800, "two"), (257, 130, 1030, 1031, "big"),
                                            (200, 512, 1024, 1024, "uniform")])
def test_apply_rounding_contract(monkeypatch, sides, d, m, nt, ld, kind):
    rng = np.random.default_rng(m + nt)
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    n = _counts(kind, m, rng)
    for slab in (None, 128):
        eng = _engine(monkeypatch, d, slab=slab)
        raw32 = _scores(eng, U, n, V)
        em, es = rng.standard_normal(m) * 10 - 20, 0.5 + 5 * rng.random(m)
        tm, ts = rng.standard_normal(nt) * 10 - 20, 0.5 + 5 * rng.random(nt)
        es[::7] = 0.0
        ts[::5] = 0.0
        if sides == "enrol":
            tm = ts = None
        if sides == "test":
            em = es = None
        got = _snorm(eng, U, n, V, em, es, tm, ts, ld=ld, fill=123.0)
        assert (got[:, nt:] == 123.0).all()                                   # the padding columns are not touched
        ref = am.snorm_apply(raw32, em, es, tm, ts)
        se, st = am.snorm_sides(raw32, em, es, tm, ts)
        mag = (np.abs(se) if se is not None else 0.0) + (np.abs(st) if st is not None else 0.0)
        err = np.abs(got[:, :nt].astype(np.float64) - ref)
        tol = am.ulp32(ref) + 2.0 ** -50 * mag
        print("apply %s D %d %dx%d ld %d %s slab %s: max err / bound = %.3g, bit-equal to float32(ref): %.4f" % (
            sides, d, m, nt, ld, kind, slab, (err / tol).max(), (got[:, :nt] == ref.astype(np.float32)).mean()))
        assert (err <= tol).all(), float((err / tol).max())
        # statistics (0, 1) on both sides: the raw scores, bit for bit
        ident = _snorm(eng, U, n, V, np.zeros(m), np.ones(m), np.zeros(nt), np.ones(nt), ld=ld, fill=123.0)
        assert np.array_equal(ident[:, :nt].view(np.uint32), raw32.view(np.uint32))


# ------------------------------------------------------------------------------------------- 4. end to end
def _oracle_asnorm(oracle, psi, U, n, V, Cv, K):
    """fp64 AS-norm from the oracle's scores: raw [M, Nt], the four statistic vectors and the normalised matrix."""
    def stats(X, cnt):
        top = np.sort(oracle.score_block(psi, X, cnt, Cv), axis=1)[:, ::-1][:, :K]
        return top.mean(axis=1), top.std(axis=1)
    raw = oracle.score_block(psi, U, n, V)
    em, es = stats(U, n)
    tm, ts = stats(V, 1)
    out = 0.5 * ((raw - em[:, None]) / es[:, None] + (raw - tm[None, :]) / ts[None, :])
    return raw, (em, es, tm, ts), out


def _asnorm_bound(raw, st, eps_raw, eps_stat):
    """sum over the sides of 0.5 [(eps + |dmean|) / std + |raw - mean| |dstd| / std^2] with |dmean|, |dstd| <= eps_stat."""
    em, es, tm, ts = st
    side = lambda m, s: 0.5 * ((eps_raw + eps_stat) / s + np.abs(raw - m) * eps_stat / (s * s))     # noqa: E731
    return side(em[:, None], es[:, None]) + side(tm[None, :], ts[None, :])


def test_end_to_end_asnorm_against_the_oracle(oracle):
    from liblda import PLDA
    rng = np.random.default_rng(0)
    n, d, k = 1200, 48, 40
    y = (np.arange(n) % k).astype(np.uint64)
    x = rng.random((n, d)) + 0.4 * rng.standard_normal((k, d))[y.astype(np.int64)]
    p = PLDA(0)
    p.fit(x[:900], y[:900], 5)                                                   # rows 900 .. 1199 are held out: the cohort
    model = p._instance.get_model()
    enrol = p.transform(x[:210], y[:210])
    test = p.transform(x[210:340], np.arange(130, dtype=np.uint64))
    cohort = p.transform_array(x[900:1200], 1)                                   # 300 held-out rows
    _, counts, U = p._instance._unpack(enrol)
    _, _, V = p._instance._unpack(test)
    K = 50
    raw, st, ref = _oracle_asnorm(oracle, model["psi"], U, counts, V, cohort, K)
    eps = score_tol(raw)
    eps_stat = max(score_tol(oracle.score_block(model["psi"], X, c, cohort)).max() for X, c in ((U, counts), (V, 1)))
    got = p.score_matrix_asnorm(enrol, test, cohort, top_k=K)
    assert got.dtype == np.float32 and got.shape == ref.shape
    bound = _asnorm_bound(raw, st, eps, eps_stat) + am.ulp32(ref)
    err = np.abs(got - ref)
    print("end to end matrix: max err / bound = %.3g (max err %.3g)" % ((err / bound).max(), err.max()))
    assert (err <= bound).all()
    mean, std = p.cohort_stats(enrol, cohort, top_k=K)
    assert np.abs(mean - st[0]).max() <= eps_stat and np.abs(std - st[1]).max() <= eps_stat
    # the trial list: fp64 raw scores (the trial-list path's own 1e-11), the same statistics
    e = rng.integers(0, U.shape[0], 1000)
    t = rng.integers(0, V.shape[0], 1000)
    gt = p.score_trials_asnorm(enrol, test, e, t, cohort, top_k=K)
    bt = _asnorm_bound(raw, st, 1e-11 * np.maximum(np.abs(raw), np.abs(raw).mean()), eps_stat)[e, t]
    et = np.abs(gt - ref[e, t])
    print("end to end trials: max err / bound = %.3g" % (et / bt).max())
    assert gt.dtype == np.float64 and (et <= bt).all()
    # top_k=None is plain S-norm: the whole cohort
    full = p.cohort_stats(test, cohort)
    all_k = p.cohort_stats(test, cohort, top_k=cohort.shape[0])
    assert np.array_equal(full[0], all_k[0]) and np.array_equal(full[1], all_k[1])


# ------------------------------------------------------------------------------------------- 5. large shape, sampled
def test_large_shape_sampled_and_slab_cap(monkeypatch):
    import torch
    from plda_amd import _native
    lib = _native.load()
    dev = _dev()
    D, R, Nc, K = 200, 50000, 200000, 300
    eng = _engine(monkeypatch, D)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator(device=dev)
    g.manual_seed(9)
    X = torch.randn((R, D), dtype=torch.float64, device=dev, generator=g)
    Cv = torch.randn((Nc, D), dtype=torch.float64, device=dev, generator=g)
    res = torch.full((2, R), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    before = lib.plda_device_bytes_held()
    lib.plda_device_bytes_peak(1)
    eng.cohort_stats_dev(X.data_ptr(), None, 1, R, Cv.data_ptr(), Nc, K, res[0].data_ptr(), res[1].data_ptr())
    eng.synchronize()
    rose = lib.plda_device_bytes_peak(0) - before
    m_last, nt_last, gemm_k = eng.score_last_shape()
    assert (m_last, nt_last, gemm_k) == (R, Nc, D)
    pad = lambda v, q: (v + q - 1) // q * q                                         # noqa: E731
    kpad = pad(gemm_k, 4) + 32                                                     # k-quads + the bias planes of a packed row
    slab_rows = pad(min(R, (4 << 30) // 4 // Nc), 256)
    operands = (slab_rows + pad(Nc, 256)) * kpad * 4 + (slab_rows + pad(Nc, 256)) * 4 * 8
    operands += operands // 8 + (1 << 20)                                          # the buffers' growth slack
    print("large shape: device bytes rose by %.1f MiB over the call (cap: 4 GiB + %.1f MiB of packed operands; the matrix is %.1f GB)"
          % (rose / 2 ** 20, operands / 2 ** 20, R * Nc * 4 / 1e9))
    assert rose <= (4 << 30) + operands
    got = res.cpu().numpy()
    assert np.isfinite(got).all()
    rows = np.unique(np.linspace(0, R - 1, 64).astype(np.int64))
    sub = torch.empty((rows.size, Nc), dtype=torch.float32, device=dev)
    Xs = X[torch.from_numpy(rows).to(dev)].contiguous()
    eng.score_matrix_dev(Xs.data_ptr(), None, 1, rows.size, Cv.data_ptr(), Nc, sub.data_ptr(), Nc)
    eng.synchronize()
    _check_exact("50k x 200k sampled", sub.cpu().numpy(), K, got[0][rows], got[1][rows])


# ------------------------------------------------------------------------------------------- 6. API edges
def test_api_edges(monkeypatch):
    import torch
    from plda_amd import MPlda
    from plda_amd._native import PLDA_E_INVAL, PLDA_E_NOT_FITTED, PldaError
    d, r, nc = 48, 10, 20
    rng = np.random.default_rng(1)
    X, Cv = _t(rng.standard_normal((r, d))), _t(rng.standard_normal((nc, d)))
    res = torch.zeros((4, max(r, nc)), dtype=torch.float64, device=_dev())
    out = torch.zeros((r, nc), dtype=torch.float32, device=_dev())
    fresh = MPlda(0)
    with pytest.raises(PldaError, match="not fitted") as ei:
        fresh.cohort_stats_dev(X.data_ptr(), None, 1, r, Cv.data_ptr(), nc, 5, res[0].data_ptr(), res[1].data_ptr())
    assert ei.value.code == PLDA_E_NOT_FITTED
    with pytest.raises(PldaError, match="not fitted"):
        fresh.score_matrix_snorm_dev(X.data_ptr(), None, 1, r, Cv.data_ptr(), nc, out.data_ptr(), nc, res[0].data_ptr(), res[1].data_ptr())
    eng = _engine(monkeypatch, d)
    x, c, m_, s_ = X.data_ptr(), Cv.data_ptr(), res[0].data_ptr(), res[1].data_ptr()
    bad_stats = [
        (dict(top_k=0), "top_k"), (dict(top_k=nc + 1), "top_k"), (dict(r=0), "R = 0"), (dict(nc=0), "Nc = 0"),
        (dict(dmean=None), "mean is NULL"), (dict(dstd=None), "std is NULL"), (dict(n_uniform=0), "n_uniform"),
    ]
    for kw, text in bad_stats:
        a = dict(dX=x, dn=None, n_uniform=1, r=r, dC=c, nc=nc, top_k=5, dmean=m_, dstd=s_)
        a.update(kw)
        with pytest.raises(PldaError, match=text) as ei:
            eng.cohort_stats_dev(**a)
        assert ei.value.code == PLDA_E_INVAL, kw
    t_, u_ = res[2].data_ptr(), res[3].data_ptr()
    bad_apply = [
        (dict(), "both statistic pairs are NULL"), (dict(demean=m_), "estd is NULL"), (dict(destd=s_), "emean is NULL"),
        (dict(dtmean=t_), "tstd is NULL"), (dict(dtstd=u_, demean=m_, destd=s_), "tmean is NULL"),
        (dict(demean=m_, destd=s_, ld=nc - 1), "ld_out"), (dict(demean=m_, destd=s_, m=0), "M = 0"),
    ]
    for kw, text in bad_apply:
        a = dict(dU=x, dn=None, n_uniform=1, m=r, dV=c, nt=nc, dout=out.data_ptr(), ld=nc)
        a.update(kw)
        with pytest.raises(PldaError, match=text) as ei:
            eng.score_matrix_snorm_dev(**a)
        assert ei.value.code == PLDA_E_INVAL, kw
    # the handle is still usable
    mean, std = _stats(eng, X.cpu().numpy(), 1, Cv.cpu().numpy(), 5)
    _check_exact("after the refused calls", _scores(eng, X.cpu().numpy(), 1, Cv.cpu().numpy()), 5, mean, std)
    # host wrappers: the dimension check speaks like _check_dim
    with pytest.raises(ValueError, match=r"must be \[rows, 48\] \(the model's current dimension\)"):
        eng.cohort_stats((1, rng.standard_normal((3, d))), rng.standard_normal((5, d + 1)))
    with pytest.raises(ValueError, match=r"must be \[rows, 48\] \(the model's current dimension\)"):
        eng.score_matrix_asnorm((1, rng.standard_normal((3, d - 1))), (1, rng.standard_normal((3, d))), rng.standard_normal((5, d)))
    with pytest.raises(PldaError, match="top_k"):
        eng.cohort_stats((1, rng.standard_normal((3, d))), rng.standard_normal((5, d)), top_k=6)


# ------------------------------------------------------------------------------------------- 7. guards, poison, leaks
GUARD_BYTES = 64 << 10
PAYLOAD = 0x7FC0DEAD


def _input(a, nan):
    """`a` placed in a buffer with GUARD_BYTES of NaN (or zero; -1 / 0 for integers) on both sides."""
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a)
    g = GUARD_BYTES // a.itemsize
    buf = torch.empty(g + a.size + g, dtype=t.dtype, device=_dev())
    if t.dtype.is_floating_point:
        buf.fill_(float("nan") if nan else 0.0)
    else:
        buf.fill_(-1 if nan else 0)
    body = buf[g:g + a.size].view(a.shape)
    body.copy_(t.to(_dev()))
    return buf, body


class _Output:
    """An output [rows, cols] with row pitch ld inside a buffer filled with the payload."""

    def __init__(self, rows, cols, dtype, ld=None):
        import torch
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.itemsize = torch.empty(0, dtype=dtype).element_size()
        self.g = GUARD_BYTES // self.itemsize
        n = self.g + rows * self.ld + self.g
        self.words = torch.full((n * self.itemsize // 4,), PAYLOAD, dtype=torch.int32, device=_dev())
        self.buf = self.words.view(dtype)
        self.body = self.buf[self.g:self.g + rows * self.ld].view(rows, self.ld)[:, :self.cols]

    def ptr(self):
        return self.body.data_ptr()

    def check(self, what):
        import torch
        torch.cuda.synchronize()
        w = self.words.cpu().numpy().reshape(-1, self.itemsize // 4)
        inside = np.zeros(w.shape[0], bool)
        idx = self.g + np.arange(self.rows)[:, None] * self.ld + np.arange(self.cols)[None, :]
        inside[idx.ravel()] = True
        bad = np.nonzero((w[~inside] != np.int32(PAYLOAD)).any(1))[0]
        assert bad.size == 0, "%s: %d guard elements overwritten" % (what, bad.size)
        left = int((w[idx.ravel()] == np.int32(PAYLOAD)).all(1).sum())
        assert left == 0, "%s: %d output elements never written" % (what, left)
        return self.body.cpu().numpy().copy()


@pytest.mark.parametrize("d,r,nc,ld,kind", [(48, 63, 517, 519, "uniform"), (200, 333, 1029, 1032, "two"), (257, 130, 260, 260, "big")])
def test_guard_bands_and_poisoned_scratch(monkeypatch, d, r, nc, ld, kind):
    import torch
    rng = np.random.default_rng(r)
    X, Cv = rng.standard_normal((r, d)), rng.standard_normal((nc, d))
    n = _counts(kind, r, rng)
    em, es = rng.standard_normal(r), 0.5 + rng.random(r)
    tm, ts = rng.standard_normal(nc), 0.5 + rng.random(nc)
    K = min(50, nc)
    runs = {}
    for poison in (False, True):
        for nan in (True, False):
            eng = _engine(monkeypatch, d, poison=poison)
            keep = [_input(a, nan) for a in (X, Cv, em, es, tm, ts)]
            dX, dC, dem, des, dtm, dts = [b for _, b in keep]
            dn = None if np.isscalar(n) else _input(n, nan)
            nptr = dn[1].data_ptr() if dn is not None else None
            nu = int(n) if np.isscalar(n) else 0
            o_mean, o_std = _Output(1, r, torch.float64), _Output(1, r, torch.float64)
            o_s, o_e = _Output(r, nc, torch.float32, ld), _Output(r, nc, torch.float32, ld)
            torch.cuda.synchronize()
            eng.cohort_stats_dev(dX.data_ptr(), nptr, nu, r, dC.data_ptr(), nc, K, o_mean.ptr(), o_std.ptr())
            eng.score_matrix_snorm_dev(dX.data_ptr(), nptr, nu, r, dC.data_ptr(), nc, o_s.ptr(), ld, dem.data_ptr(), des.data_ptr(),
                                       dtm.data_ptr(), dts.data_ptr())
            eng.score_matrix_snorm_dev(dX.data_ptr(), nptr, nu, r, dC.data_ptr(), nc, o_e.ptr(), ld, dem.data_ptr(), des.data_ptr())
            eng.synchronize()
            runs[(poison, nan)] = dict(mean=o_mean.check("mean"), std=o_std.check("std"), both=o_s.check("snorm both sides"),
                                       enrol=o_e.check("snorm enrol side"))
            del eng
    from plda_amd import MPlda
    MPlda(0)                                   # the poison switch off again for whatever runs next in this process
    first = runs[(False, True)]
    for key, run in runs.items():
        for k in first:
            assert np.array_equal(first[k].view(np.uint8), run[k].view(np.uint8)), (key, k)
    eng = _engine(monkeypatch, d)
    _check_exact("guarded inputs", _scores(eng, X, n, Cv), K, first["mean"][0], first["std"][0])


def test_create_use_destroy_gives_back_every_byte(monkeypatch):
    import gc
    import torch
    from plda_amd import _native
    lib = _native.load()
    rng = np.random.default_rng(2)
    d, r, nc = 64, 300, 700
    X, Cv = rng.standard_normal((r, d)), rng.standard_normal((nc, d))
    gc.collect()
    torch.cuda.synchronize()
    before = lib.plda_device_bytes_held()
    for _ in range(3):
        eng = _engine(monkeypatch, d)
        mean, std = _stats(eng, X, 2, Cv, 40)
        _snorm(eng, X, 2, Cv, mean, std, None, None)
        eng.cohort_stats((2, X), Cv, top_k=40)
        eng.score_matrix_asnorm((2, X), (1, Cv[:50]), Cv, top_k=40)
        assert lib.plda_device_bytes_held() > before
        eng.synchronize()
        del eng
        gc.collect()
        assert lib.plda_device_bytes_held() == before


# ------------------------------------------------------------------------------------------- 8. sharded by row
@pytest.mark.parametrize("kind", ["uniform", "two"])
def test_sharded_rows_tile_the_single_rank_result(monkeypatch, kind):
    import torch
    d, r, nc, K, world = 64, 1000, 1500, 100, 3
    rng = np.random.default_rng(4)
    X, Cv = rng.standard_normal((r, d)), rng.standard_normal((nc, d))
    n = _counts(kind, r, rng)
    eng = _engine(monkeypatch, d)
    ref = _stats(eng, X, n, Cv, K)
    dX, dC = _t(X), _t(Cv)
    dn = None if np.isscalar(n) else _t(n)
    got = torch.full((2, r), float("nan"), dtype=torch.float64, device=_dev())
    covered = np.zeros(r, np.int32)
    for rank in range(world):
        mine = torch.full((2, r), float("nan"), dtype=torch.float64, device=_dev())
        eng.comm_emulate(world, rank)
        eng.cohort_stats_sharded_dev(dX.data_ptr(), dn.data_ptr() if dn is not None else None, int(n) if np.isscalar(n) else 0, r,
                                     dC.data_ptr(), nc, K, mine[0].data_ptr(), mine[1].data_ptr())
        eng.synchronize()
        rows = torch.isfinite(mine[0])
        assert torch.equal(rows, torch.isfinite(mine[1]))
        covered += rows.cpu().numpy()
        got[:, rows] = mine[:, rows]
    eng.comm_emulate(1, 0)
    assert (covered == 1).all()                                  # every row by exactly one rank
    g = got.cpu().numpy()
    assert np.array_equal(g[0], ref[0]) and np.array_equal(g[1], ref[1])
