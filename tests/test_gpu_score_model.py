"""The fp32 trials GEMM against its exact host model, bit for bit (tests/fp32_chain.py).

Every fp32 trials score is determined: fp64 prep arithmetic rounded once to fp32, then a k-ordered chain of
fp32 fmas (v_mfma_f32_32x32x2_f32) from the rank-2 bias pair.  `fp32_chain` predicts each score's bits on
the host; a case passes when

  * at least 99.9 % of the checked elements are bit-identical to the model, and
  * every other element lies within `fp32_chain.allowance` (2 ulp of sum_k |a_k b_k|: one operand rounding
    flipped by the prep kernels' fp64 evaluation order or fma contraction, and what that does to the later
    partial sums), an allowance asserted to be at least 10x tighter than `score_tol` on every checked element.

Each case also asserts the kernel and depth that ran (score_last_kernel / score_last_shape), so a dispatch
change cannot quietly make it test something else.  Covered: the library's arms PLDA_GEMM_VARIANT 0, 20, 30,
40, 48, 49; the host and device entries (ld > Nt), prepared test sides, the sharded entries;
PLDA_PREP_VARIANT 1-3 and PLDA_MIXED_VARIANT=1; depths 1 .. 2048, ragged rows and columns, uniform, bucketed
and depth-2D counts, z-norm (with zstd == 0 rows), extreme psi, a targetdim-truncated model, near-cancelling
scores and a row whose operands and partial sums are all subnormal.  The opt-in bf16x3 arm is held to its
error SIZE (the bf16 MFMA's internal order is not documented): the split-model bound on the max error and
an RMS error within 2x that of the fp32 chain on the same operands.

The existing score_tol checks against the fp64 oracle stay where they are; this module adds the tight ones.
Run with -s to see the per-case bit-identical fraction, largest ulp deviation and bf16x3 RMS ratio.
"""
import numpy as np
import pytest

import fp32_chain as fc
from conftest import score_tol

pytestmark = pytest.mark.gpu

LIMIT = 20000             # elements emulated per case (the chain costs LIMIT x depth fp32 fmas on the host)
K_BUDGET = 2e6            # ... and at most this many element-columns
ENV = ("PLDA_GEMM_VARIANT", "PLDA_PREP_VARIANT", "PLDA_MIXED_VARIANT", "PLDA_SCORE_DTYPE")


def _psi(d, seed=3, lo=0.05, hi=4.05, log=False):
    rng = np.random.default_rng(seed)
    p = np.exp(rng.uniform(np.log(lo), np.log(hi), d)) if log else lo + rng.random(d) * (hi - lo)
    return np.sort(p)[::-1].copy()


def _engine(monkeypatch, d, psi, variant=0, prep=None, mixed=None, dtype=None):
    from plda_amd import MPlda
    for name, val in zip(ENV, (variant or None, prep, mixed, dtype)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    eng = MPlda(0)
    rng = np.random.default_rng(d)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    eng.set_model(rng.random(d), q * (1.0 + rng.random(d))[:, None], psi)
    return eng


def _expect_kernel(variant, M, Nt, Kg, dtype=None):
    """launch_gemm's choice (score.hip) for a small-enough operand (fits4g, ld < 2^22)."""
    if dtype == "bf16x3":
        return "trials_gemm_bf16x3_kernel"
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


def _pairs(M, N, Kt, limit=LIMIT, seed=0):
    return fc.sample_pairs(M, N, int(min(limit, K_BUDGET / Kt)), seed)


def _verify(eng, got, op, label, variant=0, dtype=None, pairs=None, shape=True, limit=LIMIT):
    """The bit check of one case (or, for the bf16x3 arm, its error-size check)."""
    M, N = got.shape
    pairs = _pairs(M, N, op.A32.shape[1], limit) if pairs is None else pairs
    kernel = _expect_kernel(variant, M, N, op.Kg, dtype)
    assert eng.score_last_kernel() == kernel, (label, eng.score_last_kernel(), kernel)
    last = eng.score_last_shape()
    assert last[2] == op.depth and (not shape or last[:2] == (M, N)), (label, last, op.depth)
    g = got[pairs]
    ex = fc.exact(op, pairs)
    if dtype == "bf16x3":
        err = g.astype(np.float64) - ex
        bound = fc.bf16x3_bound(op, pairs)
        e32 = fc.chain(op.A32, op.B32, pairs).astype(np.float64) - ex
        ratio = fc.rms(err) / fc.rms(e32)
        print("\nBF16X3 %-34s rms ratio %.3f  max err / bound %.3f  max |err| %.2e (fp32 chain %.2e)  max |score| %.1f"
              % (label, ratio, np.max(np.abs(err) / bound), np.abs(err).max(), np.abs(e32).max(), np.abs(ex).max()))
        assert (np.abs(err) <= bound).all(), (label, np.max(np.abs(err) / bound))
        assert ratio <= 2.0, (label, ratio)
        return
    allow = fc.allowance(op, pairs)
    assert (allow <= 0.1 * score_tol(ex)).all(), (label, np.max(allow / score_tol(ex)))
    model = fc.chain(op.A32, op.B32, pairs)
    ok, frac, ulp = fc.check(g, model, allow)
    print("\nFP32 %-36s %-26s identical %.5f  max ulp %d  (%d elements)" % (label, kernel, frac, ulp, len(g)))
    assert ok, "%s: %.5f of %d elements bit-identical, max %d ulp, worst |delta| / allowance %.3g" % (
        label, frac, len(g), ulp, np.max(np.abs(g.astype(np.float64) - model) / allow))


def _zn(eng, m, rng, zstd_zero_every=7):
    """z-norm statistics on the engine (some rows without: zstd 0, left raw); the arrays the model wants."""
    zm = rng.standard_normal(m) * 20.0
    zs = rng.random(m) * 5.0 + 0.5
    zs[::zstd_zero_every] = 0.0
    zm = np.where(zs == 0.0, 0.0, zm)
    ids = np.arange(m, dtype=np.int64)
    eng._meanz = {int(k): float(zm[k]) for k in ids if zs[k] != 0.0}
    eng._stdvz = {int(k): float(zs[k]) for k in ids if zs[k] != 0.0}
    return ids, zm, zs


def _counts(rng, m, values):
    values = np.asarray(values, np.int32)
    c = values[rng.integers(0, len(values), m)]
    c[:len(values)] = values[:m]
    return c.astype(np.int32)


def _host_case(monkeypatch, d, m, nt, n, variant=0, seed=0, psi=None, zn=False, label="", **env):
    eng = _engine(monkeypatch, d, _psi(d) if psi is None else psi, variant, **env)
    psi = eng.get_model()["psi"]
    rng = np.random.default_rng(1000 + seed)
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    if zn:
        ids, zm, zs = _zn(eng, m, rng)
        got = eng.score_matrix((n, U, ids), (1, V))
    else:
        zm = zs = None
        got = eng.score_matrix((n, U), (1, V))
    form = fc.pick_form(d, n, env.get("mixed") or 0)
    op = fc.operands(psi, U, V, n, zm, zs, form=form)
    _verify(eng, got, op, label, variant, env.get("dtype"))
    return eng, op


# ---------------------------------------------------------------- depths (default dispatch; bt2 / bt4 forced)
DEPTHS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, 63, 64, 65, 129, 200, 255, 256, 257, 512, 1024, 2048]


@pytest.mark.parametrize("d", DEPTHS)
def test_depths_default(monkeypatch, d):
    n = (1, 7, 100, 4095)[DEPTHS.index(d) % 4]
    _host_case(monkeypatch, d, 65, 127, n, seed=d, label="depth %d n=%d" % (d, n))


@pytest.mark.parametrize("variant", [30, 40])
@pytest.mark.parametrize("d", [1, 9, 65, 72, 200, 257, 1024])
def test_depths_big_tile(monkeypatch, variant, d):
    _host_case(monkeypatch, d, 257, 300, 7, variant, seed=d, label="v%d depth %d" % (variant, d))


# ---------------------------------------------------------------- ragged rows and columns
SIDES = [1, 31, 32, 33, 127, 128, 129, 255, 256, 257]


@pytest.mark.parametrize("variant", [20, 30, 40])
@pytest.mark.parametrize("m,nt", list(zip(SIDES, SIDES[::-1])) + [(257, 257), (1, 1)])
def test_rows_and_columns(monkeypatch, variant, m, nt):
    _host_case(monkeypatch, 72, m, nt, 3, variant, seed=m, label="v%d %dx%d" % (variant, m, nt))


# ---------------------------------------------------------------- every arm of the library, every operand form
FORMS = {
    "uniform": (200, 7, False),
    "buckets": (96, [1, 2, 3, 4, 5], False),
    "znorm_uniform": (120, 3, True),
    "znorm_buckets": (120, [1, 2, 3, 4, 5], True),
    "depth2d": (96, [1, 17, 4096], False),
}


@pytest.mark.parametrize("variant", [0, 20, 30, 40, 48, 49])
@pytest.mark.parametrize("form", list(FORMS))
def test_arms(monkeypatch, variant, form):
    d, vals, zn = FORMS[form]
    m, nt = 300, 517
    n = vals if np.ndim(vals) == 0 else _counts(np.random.default_rng(5), m, vals)
    _host_case(monkeypatch, d, m, nt, n, variant, seed=7, zn=zn, label="v%d %s" % (variant, form))


# ---------------------------------------------------------------- counts
@pytest.mark.parametrize("variant", [20, 40])
@pytest.mark.parametrize("name,d,values", [
    ("n1", 200, 1), ("n7", 200, 7), ("n100", 200, 100), ("n4095", 200, 4095),
    ("G2", 96, [1, 3]), ("G5", 96, [1, 2, 3, 4, 5]), ("G9", 96, list(range(1, 10))), ("G10", 96, list(range(1, 11))),
    ("G40", 96, list(range(1, 80, 2))), ("adjacent", 200, [1, 4094, 4095]), ("n200_201", 200, [200, 201]),
    ("past_range", 96, [1, 17, 4096]), ("too_many_G", 24, list(range(1, 15))), ("G70", 200, list(range(1, 71))),
])
def test_counts(monkeypatch, variant, name, d, values):
    m, nt = 300, 260
    n = values if np.ndim(values) == 0 else _counts(np.random.default_rng(len(name)), m, values)
    _, op = _host_case(monkeypatch, d, m, nt, n, variant, seed=11, label="v%d counts %s" % (variant, name))
    want = {"past_range": "depth2d", "too_many_G": "depth2d", "G70": "depth2d"}.get(name)
    assert want is None or op.form == want


def test_mixed_variant_depth2d(monkeypatch):
    m, nt = 300, 517
    n = _counts(np.random.default_rng(3), m, [1, 2, 3, 4, 5])
    _, op = _host_case(monkeypatch, 96, m, nt, n, 20, mixed=1, label="PLDA_MIXED_VARIANT=1")
    assert op.form == "depth2d"


# ---------------------------------------------------------------- models and data
@pytest.mark.parametrize("counts", ["uniform", "mixed"])
def test_psi_extremes(monkeypatch, counts):
    d, m, nt = 200, 200, 260
    psi = _psi(d, lo=1e-6, hi=1e4, log=True)
    n = 4 if counts == "uniform" else _counts(np.random.default_rng(1), m, [1, 2, 5, 40, 4095])
    _host_case(monkeypatch, d, m, nt, n, 0, psi=psi, label="psi 1e-6..1e4 %s" % counts)


def test_targetdim_model(monkeypatch):
    eng = _engine(monkeypatch, 64, _psi(64))
    eng.truncate(40)
    psi = eng.get_model()["psi"]
    assert psi.shape == (40,)
    rng = np.random.default_rng(2)
    U, V = rng.standard_normal((130, 40)), rng.standard_normal((250, 40))
    got = eng.score_matrix((5, U), (1, V))
    _verify(eng, got, fc.operands(psi, U, V, 5), "targetdim 64 -> 40")


def _cancelling(psi, n, U, V, rows, rng):
    """Rescale enrol rows i in `rows` along a random direction so that S_ii = r_i + q_i + A1_i . v_i ~ 0."""
    c, var = fc._coef(float(n), psi)
    L = np.sum(np.log(var) - np.log(1 + psi))
    g = 1 / var - 1 / (1 + psi)
    done = []
    for i in rows:
        w = rng.standard_normal(psi.shape[0])
        a = np.sum(c / var * w * V[i])
        b = -0.5 * np.sum(c * c / var * w * w)
        C = -0.5 * L - 0.5 * np.sum(g * V[i] * V[i])
        disc = a * a - 4 * b * C
        if disc > 0:
            U[i] = w * (-a - np.sqrt(disc)) / (2 * b)
            done.append(i)
    return done


@pytest.mark.parametrize("variant", [20, 40])
def test_near_cancellation(monkeypatch, variant):
    d, m, nt = 200, 64, 300
    eng = _engine(monkeypatch, d, _psi(d), variant)
    psi = eng.get_model()["psi"]
    rng = np.random.default_rng(4)
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    rows = _cancelling(psi, 3, U, V, range(32), rng)
    assert len(rows) >= 16
    got = eng.score_matrix((3, U), (1, V))
    op = fc.operands(psi, U, V, 3)
    ex = fc.exact(op, (np.array(rows), np.array(rows)))
    assert (np.abs(ex) < 1e-6 * fc.magnitude(op, (np.array(rows), np.array(rows)))).all()
    _verify(eng, got, op, "v%d near-cancellation" % variant, variant)
    diag = (np.array(rows), np.array(rows))           # the cancelling elements themselves, all of them
    ok, frac, ulp = fc.check(got[diag], fc.chain(op.A32, op.B32, diag), fc.allowance(op, diag), min_identical=0.9)
    assert ok, (frac, ulp)


@pytest.mark.parametrize("variant", [20, 30, 40])
@pytest.mark.parametrize("mixed", [False, True])
def test_subnormal_row(monkeypatch, variant, mixed):
    """Row 0 gets zstd = 1e40: s_0 = fp32(1e-40) is subnormal, so are its packed A operand, its one-hot entry,
    r'_0 and every partial sum of its scores -- a flush of subnormal MFMA inputs would zero them."""
    d, m, nt = 96, 257, 300
    eng = _engine(monkeypatch, d, _psi(d), variant)
    psi = eng.get_model()["psi"]
    rng = np.random.default_rng(8)
    U, V = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    n = _counts(rng, m, [1, 2, 3, 4, 5]) if mixed else 2
    ids, zm, zs = _zn(eng, m, rng)
    zs[0], zm[0] = 1e40, 3.0
    eng._meanz[0], eng._stdvz[0] = 3.0, 1e40
    got = eng.score_matrix((n, U, ids), (1, V))
    op = fc.operands(psi, U, V, n, zm, zs)
    assert 0 < abs(op.A32[0, 1]) < np.finfo(np.float32).tiny and (np.abs(op.A32[0, 2:]) < np.finfo(np.float32).tiny).all()
    row0 = (np.zeros(nt, np.int64), np.arange(nt))
    model0 = fc.chain(op.A32, op.B32, row0)
    assert (np.abs(model0) < np.finfo(np.float32).tiny).all() and (model0 != 0).all()
    assert np.array_equal(got[0], model0), np.count_nonzero(got[0] != model0)
    _verify(eng, got, op, "v%d subnormal row %s" % (variant, "mixed" if mixed else "uniform"), variant)


# ---------------------------------------------------------------- prep variants
@pytest.mark.parametrize("prep", [1, 2, 3])
@pytest.mark.parametrize("form", ["uniform", "znorm_uniform", "znorm_buckets", "depth2d"])
def test_prep_variants(monkeypatch, prep, form):
    d, vals, zn = FORMS[form]
    m, nt = 300, 517
    n = vals if np.ndim(vals) == 0 else _counts(np.random.default_rng(5), m, vals)
    _host_case(monkeypatch, d, m, nt, n, 20, seed=9, zn=zn, prep=prep, label="prep%d %s" % (prep, form))


# ---------------------------------------------------------------- device entries
def _dev_setup(monkeypatch, d, m, nt, seed, variant=0):
    import torch
    dev = torch.device("cuda", 0)
    eng = _engine(monkeypatch, d, _psi(d), variant)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    psi = eng.get_model()["psi"]
    rng = np.random.default_rng(seed)
    Uh, Vh = rng.standard_normal((m, d)), rng.standard_normal((nt, d))
    return torch, dev, eng, psi, rng, Uh, Vh, torch.from_numpy(Uh).to(dev), torch.from_numpy(Vh).to(dev)


@pytest.mark.parametrize("mixed", [False, True])
def test_device_entry_ld_and_znorm(monkeypatch, mixed):
    d, m, nt, ld = 128, 300, 517, 533
    torch, dev, eng, psi, rng, Uh, Vh, U, V = _dev_setup(monkeypatch, d, m, nt, 31)
    counts = _counts(rng, m, [1, 2, 3, 4, 5]) if mixed else None
    dn = torch.from_numpy(counts).to(dev) if mixed else None
    zm, zs = rng.standard_normal(m) * 20, rng.random(m) * 5 + 0.5
    zs[::5] = 0.0
    for z in (False, True):
        o = torch.full((m, ld), float("nan"), dtype=torch.float32, device=dev)
        dzm, dzs = (torch.from_numpy(zm).to(dev), torch.from_numpy(zs).to(dev)) if z else (None, None)
        eng.score_matrix_dev(U.data_ptr(), dn.data_ptr() if mixed else 0, 0 if mixed else 4, m, V.data_ptr(), nt,
                             o.data_ptr(), ld, dzm.data_ptr() if z else None, dzs.data_ptr() if z else None)
        torch.cuda.synchronize()
        full = o.cpu().numpy()
        assert np.isnan(full[:, nt:]).all()
        op = fc.operands(psi, Uh, Vh, counts if mixed else 4, zm if z else None, zs if z else None)
        _verify(eng, np.ascontiguousarray(full[:, :nt]), op, "dev ld>Nt %s%s" % ("mixed" if mixed else "uniform", " z" if z else ""))
    eng.set_stream(None)


def test_device_prepared_sides(monkeypatch):
    """A prepared test side is reused: uniform (score_prepare_dev), bucketed for a WIDER count set than the call
    brings (score_prepare_counts_dev: the prepared set decides the buckets and the depth) and depth-2D."""
    d, m, nt = 56, 400, 700
    torch, dev, eng, psi, rng, Uh, Vh, U, V = _dev_setup(monkeypatch, d, m, nt, 41)

    def score(counts, n_uniform=0):
        o = torch.empty((m, nt), dtype=torch.float32, device=dev)
        dn = torch.from_numpy(counts).to(dev) if counts is not None else None
        eng.score_matrix_dev(U.data_ptr(), dn.data_ptr() if dn is not None else 0, n_uniform, m, V.data_ptr(), nt, o.data_ptr(), nt)
        torch.cuda.synchronize()
        return o.cpu().numpy()

    eng.score_prepare_dev(V.data_ptr(), nt, n_uniform=6)
    _verify(eng, score(None, 6), fc.operands(psi, Uh, Vh, 6), "prepared uniform")
    c15 = _counts(rng, m, [1, 2, 3, 4, 5])
    eng.score_prepare_counts_dev(V.data_ptr(), nt, [6, 5, 4, 3, 2, 1])
    op = fc.operands(psi, Uh, Vh, c15, form="buckets", cs=np.arange(1, 7))
    assert op.depth == d + 5
    _verify(eng, score(c15), op, "prepared buckets {1..6}, call {1..5}")
    c24 = _counts(rng, m, [2, 4])
    _verify(eng, score(c24), fc.operands(psi, Uh, Vh, c24, form="buckets", cs=np.arange(1, 7)), "prepared buckets, call {2,4}")
    eng.score_prepare_dev(V.data_ptr(), nt, mixed_counts=True)
    _verify(eng, score(c15), fc.operands(psi, Uh, Vh, c15, form="depth2d"), "prepared depth-2D")
    eng.score_unprepare()
    eng.set_stream(None)


@pytest.mark.parametrize("mixed", [False, True])
def test_sharded_entries(monkeypatch, mixed):
    d, m, nt, R = 72, 700, 300, 3
    torch, dev, eng, psi, rng, Uh, Vh, U, V = _dev_setup(monkeypatch, d, m, nt, 51)
    counts = np.sort(_counts(rng, m, [1, 2, 5, 9])).astype(np.int32) if mixed else None
    dn = torch.from_numpy(counts).to(dev) if mixed else None
    op = fc.operands(psi, Uh, Vh, counts if mixed else 3)
    full = torch.full((m, nt), float("nan"), dtype=torch.float32, device=dev)
    for r in range(R):
        eng.comm_emulate(R, r)
        eng.score_matrix_sharded_dev(U.data_ptr(), dn.data_ptr() if mixed else None, 0 if mixed else 3, m, V.data_ptr(), nt,
                                     full.data_ptr(), nt, block_rows=256)
        rows = np.concatenate([np.arange(a, b) for a, b in eng.shard_plan(m, R, r, 256)])
        slab = torch.full((len(rows), nt), float("nan"), dtype=torch.float32, device=dev)
        eng.score_matrix_sharded_local_dev(U.data_ptr(), dn.data_ptr() if mixed else None, 0 if mixed else 3, m, V.data_ptr(), nt,
                                           slab.data_ptr(), nt, block_rows=256)
        torch.cuda.synchronize()
        sub = fc.Operands(op.A64[rows], op.B64, op.A32[rows], op.B32, op.form, op.depth)
        _verify(eng, slab.cpu().numpy(), sub, "sharded_local rank %d/%d" % (r, R), shape=False)
    _verify(eng, full.cpu().numpy(), op, "sharded_dev R=%d" % R, shape=False)
    eng.comm_emulate(1, 0)
    eng.set_stream(None)


# ---------------------------------------------------------------- the 8192 x 8192 default-dispatch shapes, sampled
@pytest.mark.parametrize("name,d,n,zn", [("C2", 200, 1, False), ("C3", 512, 100, False), ("C4", 256, "1..5", False),
                                         ("C5", 200, 1, True)])
def test_large_default_dispatch(monkeypatch, name, d, n, zn):
    """One device call each (the host entry scores in row slabs): bt2 at exactly 1024 tiles of 256 x 256."""
    m = nt = 8192
    torch, dev, eng, psi, rng, Uh, Vh, U, V = _dev_setup(monkeypatch, d, m, nt, 61)
    counts = _counts(rng, m, [1, 2, 3, 4, 5]) if n == "1..5" else None
    dn = torch.from_numpy(counts).to(dev) if counts is not None else None
    zm = zs = None
    if zn:
        zm, zs = rng.standard_normal(m) * 20, rng.random(m) * 5 + 0.5
        zs[::7] = 0.0
    dzm, dzs = (torch.from_numpy(zm).to(dev), torch.from_numpy(zs).to(dev)) if zn else (None, None)
    out = torch.full((m, nt), float("nan"), dtype=torch.float32, device=dev)
    eng.score_matrix_dev(U.data_ptr(), dn.data_ptr() if dn is not None else None, 0 if dn is not None else n, m, V.data_ptr(), nt,
                         out.data_ptr(), nt, dzm.data_ptr() if zn else None, dzs.data_ptr() if zn else None)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    op = fc.operands(psi, Uh, Vh, counts if counts is not None else n, zm, zs)
    _verify(eng, got, op, "%s 8192x8192 D=%d" % (name, d), limit=3600)
    eng.set_stream(None)


# ---------------------------------------------------------------- the opt-in bf16x3 arm: error size
@pytest.mark.parametrize("form", ["uniform", "buckets", "znorm_uniform", "znorm_buckets"])
def test_bf16x3_error_size(monkeypatch, form):
    d, vals, zn = FORMS[form]
    d = 200
    m, nt = 255, 257
    n = vals if np.ndim(vals) == 0 else _counts(np.random.default_rng(5), m, vals)
    _host_case(monkeypatch, d, m, nt, n, 0, seed=13, zn=zn, dtype="bf16x3", label="bf16x3 %s" % form)
