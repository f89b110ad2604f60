"""GPU: the fp64 GEMM behind fit, GetOutput and the LDA (Kaldi / ATLAS dgemm in the reference, reached through
pldamodule.cpp:76-106) on its own, through plda_gemm_f64: every dispatch class -- one 16 x 16 tile per workgroup
(M, N, K <= 256), the panel kernel, the 64 x 64 and 128 x 128 tiles with and without split-K -- both operand layouts,
alpha / beta, batches, k-weights, ragged sizes, against NumPy in fp64."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _check(eng, rng, m, n, k, ta, tb, alpha, beta, batch=None, kw=False):
    sa = (k, m) if ta else (m, k)
    sb = (n, k) if tb else (k, n)
    if batch:
        sa, sb = (batch,) + sa, (batch,) + sb
    A, B = rng.standard_normal(sa), rng.standard_normal(sb)
    C0 = rng.standard_normal(((batch,) if batch else ()) + (m, n))
    w = rng.random(k) + 0.5 if kw else None
    got = eng.gemm_f64(A, B, alpha, beta, C0, ta, tb, w)
    opA = np.swapaxes(A, -1, -2) if ta else A
    opB = np.swapaxes(B, -1, -2) if tb else B
    if w is not None:
        opA = opA * w
    want = alpha * (opA @ opB) + beta * C0
    tol = 4e-16 * k * max(1.0, np.abs(opA).max() * np.abs(opB).max()) * abs(alpha) + 1e-15 * np.abs(beta * C0).max() + 1e-15
    assert np.abs(got - want).max() <= tol, (m, n, k, ta, tb, np.abs(got - want).max(), tol)


def test_small_products_every_layout():
    from plda_amd import MPlda
    eng = MPlda(0)
    rng = np.random.default_rng(0)
    for (m, n, k) in ((1, 1, 1), (3, 5, 2), (16, 16, 4), (17, 33, 5), (64, 64, 64), (200, 200, 200), (199, 201, 203),
                      (256, 256, 256), (255, 1, 256), (1, 256, 255), (40, 200, 13)):
        for ta in (False, True):
            for tb in (False, True):
                _check(eng, rng, m, n, k, ta, tb, 1.0, 0.0)
    _check(eng, rng, 200, 200, 200, False, True, -1.0, 1.0)
    _check(eng, rng, 100, 120, 77, True, False, 0.37, -2.5)


def test_batches_share_nothing():
    from plda_amd import MPlda
    eng = MPlda(0)
    rng = np.random.default_rng(1)
    _check(eng, rng, 200, 200, 200, False, False, 1.0, 0.0, batch=5)
    _check(eng, rng, 64, 48, 200, False, True, -1.0, 1.0, batch=35)
    _check(eng, rng, 300, 300, 300, True, False, 1.0, 0.0, batch=3)       # panel kernel, batched
    _check(eng, rng, 512, 512, 512, False, False, 1.0, 1.0, batch=2)


def test_deep_and_large_products():
    from plda_amd import MPlda
    eng = MPlda(0)
    rng = np.random.default_rng(2)
    _check(eng, rng, 200, 200, 5000, True, False, 1.0, 0.0)               # X^T X shape: panel kernel in chunks
    _check(eng, rng, 512, 512, 10000, True, False, 1.0, 0.0)              # tiles + split-K
    _check(eng, rng, 1000, 300, 700, False, True, 2.0, 0.5)
    _check(eng, rng, 130, 2000, 129, False, False, 1.0, 0.0)
    _check(eng, rng, 200, 200, 40000, True, False, 1.0, 0.0, kw=True)     # the scatter's weighted contraction
    _check(eng, rng, 260, 260, 3000, True, False, 1.0, 0.0, kw=True)


@pytest.mark.parametrize("d", [210, 256, 300, 320, 384, 450, 512])
def test_symmetric_products_one_read_kernel(d):
    """X^T diag(w) X with both operands the SAME array (what fit's statistics pass computes, pldamodule.cpp:94-98): for
    208 < D <= 512 the block kernel of round 4 (csrc/syrk_blk.inc: 64 x 64 blocks dealt to the waves of up to four
    workgroups, full rows staged once by LDS DMA).  Row counts around the 16-row stage and the group split (fewer
    stages than groups, ragged last stage, one row), with and without weights, alpha / beta; exactly symmetric output."""
    from plda_amd import MPlda
    eng = MPlda(0)
    rng = np.random.default_rng(d)
    for k in (2048, 2049, 2063, 5000, 40000):
        for kw in (False, True):
            X = rng.standard_normal((k, d))
            w = rng.random(k) + 0.5 if kw else None
            C0 = rng.standard_normal((d, d)); C0 = C0 + C0.T
            alpha, beta = (1.0, 0.0) if k != 5000 else (-0.5, 2.0)
            got = eng.gemm_f64(X, X, alpha, beta, C0, True, False, w)
            want = alpha * ((X.T * w) @ X if kw else X.T @ X) + beta * C0
            tol = 4e-16 * k * max(1.0, np.abs(X).max() ** 2) * abs(alpha) * 1.5 + 1e-15 * np.abs(beta * C0).max() + 1e-15
            assert np.abs(got - want).max() <= tol, (d, k, kw, np.abs(got - want).max(), tol)
            assert np.array_equal(got, got.T)


# ---- every dispatch class of gemm_f64_batched / syrk_f64 (csrc/linalg.hip), pinned by the kernel the library reports ----
#
# _check keeps its tolerance; the helpers below add the assertion of WHICH kernel formed the product
# (MPlda.linalg_last_kernels), so that a moved dispatch threshold fails a test instead of emptying it.

_LAYOUTS = [(ta, tb) for ta in (False, True) for tb in (False, True)]


def _panel(ta, tb, k):
    """the panel instantiation of a product: <A contiguous along k, B contiguous along k, 64-deep stages per chunk>"""
    return "gemm_f64_panel_kernel<%d,%d,%d>" % (not ta, tb, min(4, -(-k // 64)))


def _general(ta, tb, tile, splitk):
    return "gemm_f64_kernel<%d,%d,%d>%s" % (not ta, tb, tile, "+splitk" if splitk else "")


def _assert_union(seen, expected, what):
    assert seen == expected, "%s: never ran %s; ran unexpectedly %s" % (what, sorted(expected - seen), sorted(seen - expected))


_PANEL_K = [1, 3, 4, 5, 8, 63, 64, 65, 100, 128, 129, 190, 192, 193, 255, 256,      # one chunk of 1, 2, 3, 4 stages
            257, 300, 511, 512, 513, 2047, 2048]                                     # chunks of 256, ragged and full last chunk


@pytest.mark.parametrize("m,n,batch", [(300, 40, None), (40, 300, None), (257, 257, 3)])
def test_panel_kernel_every_instantiation(m, n, batch):
    """gemm_f64_panel_kernel<AKC, BKC, NB>: all 16 instantiations (NB = 1, 2, 3 are reached only with M or N above 256,
    the tile-16 kernel taking the rest), every tail of the K walk: K % 8 == 4 (the lone MFMA after the pairs), K not a
    multiple of 4, a partial and a full last chunk of a K above 256."""
    from plda_amd import MPlda
    eng = MPlda(0)
    rng = np.random.default_rng(m * 1000 + n)
    seen = set()
    for k in _PANEL_K:
        for ta, tb in _LAYOUTS:
            alpha, beta = (1.0, 0.0) if k % 5 else (-0.75, 1.5)
            _check(eng, rng, m, n, k, ta, tb, alpha, beta, batch=batch)
            assert eng.linalg_last_kernels() == [_panel(ta, tb, k)], (m, n, k, ta, tb, eng.linalg_last_kernels())
            seen |= set(eng.linalg_last_kernels())
    _assert_union(seen, {"gemm_f64_panel_kernel<%d,%d,%d>" % (a, b, nb) for a in (0, 1) for b in (0, 1) for nb in (1, 2, 3, 4)},
                  "panel kernel")


@pytest.mark.parametrize("ta,tb", [(True, True), (False, False)])
def test_tile16_kernel_every_depth(ta, tb):
    """gemm_f64_tile16_kernel: K split over the waves of a workgroup, every K from 1 to 70 at a ragged 17 x 33."""
    from plda_amd import MPlda
    eng = MPlda(0)
    rng = np.random.default_rng(17 + ta)
    for k in range(1, 71):
        alpha, beta = (1.0, 0.0) if k % 5 else (0.37, -2.5)
        _check(eng, rng, 17, 33, k, ta, tb, alpha, beta)
        assert eng.linalg_last_kernels() == ["gemm_f64_tile16_kernel"], (k, eng.linalg_last_kernels())


@pytest.mark.parametrize("m,n,k,batch,variant,tile,splitk", [
    (130, 2000, 129, None, None, 64, False),     # N above the panel's 1024; 32 tiles of 128 would leave the chip idle
    (2000, 130, 700, None, None, 64, False),
    (130, 130, 3000, None, None, 64, True),      # K above the panel's 2048: 9 tiles x 12 splits
    (384, 384, 5632, None, None, 128, True),     # 9 tiles of 128 x 22 chunks of 256 = 198 >= 192 workgroups
    (300, 300, 300, 48, "4", 128, False),        # PLDA_GEMM64_VARIANT=4 (no tile-16, no panel): the batch fills the chip
])
def test_general_kernel_both_tiles_with_and_without_split_k(m, n, k, batch, variant, tile, splitk, monkeypatch):
    """gemm_f64_kernel<AKC, BKC, 64 | 128>, with and without the split-K second stage, every layout (shapes derived from
    gemm_f64_batched: `big` needs M, N >= 128 and tiles128 * min(ceil(K / 256), 64) * batch >= 192)."""
    if variant:
        monkeypatch.setenv("PLDA_GEMM64_VARIANT", variant)
    from plda_amd import MPlda
    eng = MPlda(0)
    rng = np.random.default_rng(m + n + k)
    for ta, tb in _LAYOUTS:
        _check(eng, rng, m, n, k, ta, tb, 1.0, 0.0, batch=batch)
        assert eng.linalg_last_kernels() == [_general(ta, tb, tile, splitk)], (m, n, k, ta, tb, eng.linalg_last_kernels())
    _check(eng, rng, m, n, k, False, True, -0.5, 2.0, batch=batch)


@pytest.mark.parametrize("m,n,k,splitk", [(40, 50, 100, False), (200, 200, 1500, True), (130, 70, 3000, True)])
def test_row_weights_every_layout(m, n, k, splitk):
    """kw with A stored [M, K] as well as [K, M]: the weight of a k is one value per fetched ROW of a transposed A but one
    per COLUMN of the tile (w[0] of the AKC = true path of fetch_tile / store_tile) otherwise."""
    from plda_amd import MPlda
    eng = MPlda(0)
    rng = np.random.default_rng(k)
    for ta, tb in _LAYOUTS:
        _check(eng, rng, m, n, k, ta, tb, 1.0, 0.0, kw=True)
        assert eng.linalg_last_kernels() == [_general(ta, tb, 64, splitk)], (m, n, k, ta, tb, eng.linalg_last_kernels())
    _check(eng, rng, m, n, k, False, False, 2.0, 0.5, kw=True)


def _syrk_kernels(d):
    """what X^T diag(w) X of one array [K >= 2048, d] runs (syrk_f64)"""
    if d <= 208:
        return ["syrk_tri_kernel"]
    if d <= 512 and d % 2 == 0:
        return ["syrk_blk_kernel"]
    return ["syrk_lower_kernel<1>", "syrk_lower_kernel<0>"]      # the diagonal, then the strictly-lower super-tiles


def _same_array(eng, rng, d, k, kw, alpha, beta, nan_c=False):
    X = rng.standard_normal((k, d))
    w = rng.random(k) + 0.5 if kw else None
    C0 = rng.standard_normal((d, d)); C0 = C0 + C0.T
    got = eng.gemm_f64(X, X, alpha, beta, np.full((d, d), np.nan) if nan_c else C0, True, False, w)
    want = alpha * ((X.T * w) @ X if kw else X.T @ X) + beta * C0
    tol = 4e-16 * k * max(1.0, np.abs(X).max() ** 2) * abs(alpha) * 1.5 + 1e-15 * np.abs(beta * C0).max() + 1e-15
    assert np.isfinite(got).all(), (d, k, kw)
    assert np.abs(got - want).max() <= tol, (d, k, kw, np.abs(got - want).max(), tol)
    assert np.array_equal(got, got.T), (d, k, kw)
    return got


@pytest.mark.parametrize("d", [32, 33, 47, 48, 49, 64, 80, 96, 112, 128, 144, 160, 176, 192, 200, 207, 208])
def test_symmetric_products_tri_kernel(d):
    """syrk_tri_kernel on its own (the same-array product of D <= 208; through a fit it is reached at few sizes): the tile
    rows of the triangle are dealt to eight waves as {w, nt - 1 - w}, nt = ceil(D / 16) = 2 .. 13 here."""
    from plda_amd import MPlda
    eng = MPlda(0)
    rng = np.random.default_rng(d)
    for k in (2048, 2063, 5000):
        for kw in (False, True):
            alpha, beta = (1.0, 0.0) if k != 5000 else (-0.5, 2.0)
            _same_array(eng, rng, d, k, kw, alpha, beta)
            assert eng.linalg_last_kernels() == _syrk_kernels(d) == ["syrk_tri_kernel"], (d, k, eng.linalg_last_kernels())


def test_tri_kernel_sizes_cover_every_tile_count():
    sizes = [32, 33, 47, 48, 49, 64, 80, 96, 112, 128, 144, 160, 176, 192, 200, 207, 208]
    assert {-(-d // 16) for d in sizes} == set(range(2, 14))


@pytest.mark.parametrize("d", [513, 640, 700, 1000, 1024])
def test_symmetric_products_super_tile_kernel(d):
    """syrk_lower_kernel (D > 512, otherwise reached only through a whole fit): 128 x 128 super-tiles, the diagonal ones
    and the strictly-lower ones in a launch each, ragged last super-tile."""
    from plda_amd import MPlda
    eng = MPlda(0)
    rng = np.random.default_rng(d)
    for k in (2048, 2063, 5000):
        for kw in (False, True):
            alpha, beta = (1.0, 0.0) if k != 5000 else (-0.5, 2.0)
            _same_array(eng, rng, d, k, kw, alpha, beta)
            assert eng.linalg_last_kernels() == _syrk_kernels(d), (d, k, eng.linalg_last_kernels())
            assert len(eng.linalg_last_kernels()) == 2


def test_beta_zero_never_reads_c():
    """beta == 0: C is output only (the library's own products land in scratch that holds anything).  One shape per
    dispatch class, C_in all NaN; the result is finite and within the usual tolerance."""
    from plda_amd import MPlda
    eng = MPlda(0)
    rng = np.random.default_rng(11)
    for (m, n, k, want) in ((64, 64, 64, "gemm_f64_tile16_kernel"), (300, 40, 100, _panel(False, False, 100)),
                            (130, 2000, 129, _general(False, False, 64, False)), (384, 384, 5632, _general(False, False, 128, True))):
        A, B = rng.standard_normal((m, k)), rng.standard_normal((k, n))
        got = eng.gemm_f64(A, B, 1.0, 0.0, np.full((m, n), np.nan))
        assert eng.linalg_last_kernels() == [want], (m, n, k, eng.linalg_last_kernels())
        tol = 4e-16 * k * max(1.0, np.abs(A).max() * np.abs(B).max()) + 1e-15
        assert np.isfinite(got).all() and np.abs(got - A @ B).max() <= tol, (m, n, k)
    for d in (100, 256, 640):        # syrk_tri, syrk_blk, syrk_lower
        _same_array(eng, rng, d, 2048, False, 1.0, 0.0, nan_c=True)
        assert eng.linalg_last_kernels() == _syrk_kernels(d), (d, eng.linalg_last_kernels())
    assert [_syrk_kernels(d)[0] for d in (100, 256, 640)] == ["syrk_tri_kernel", "syrk_blk_kernel", "syrk_lower_kernel<1>"]


def _family(eng, kind):
    """one product of each family, seeded: (result, reference, tolerance)"""
    rng = np.random.default_rng(99)
    if kind[0] == "gemm":
        _, m, n, k = kind
        A, B = rng.standard_normal((m, k)), rng.standard_normal((k, n))
        return eng.gemm_f64(A, B), A @ B, 4e-16 * k * max(1.0, np.abs(A).max() * np.abs(B).max()) + 1e-15
    _, d, k = kind
    X = rng.standard_normal((k, d))
    return eng.gemm_f64(X, X, 1.0, 0.0, None, True, False), X.T @ X, 4e-16 * k * max(1.0, np.abs(X).max() ** 2) * 1.5 + 1e-15


@pytest.mark.parametrize("variant,kind,default_kernels,arm_kernels", [
    ("1", ("gemm", 384, 384, 5632), [_general(False, False, 128, True)], [_general(False, False, 64, True)]),      # 64 x 64 tiles always
    ("2", ("syrk", 100, 2048), ["syrk_tri_kernel"], [_panel(True, False, 2048)]),                                  # same array: the general path
    ("3", ("syrk", 200, 2048), ["syrk_tri_kernel"], ["syrk_lower_kernel<1>", "syrk_lower_kernel<0>"]),             # super-tiles always
    ("4", ("gemm", 64, 64, 64), ["gemm_f64_tile16_kernel"], [_general(False, False, 64, False)]),                  # neither tile-16 nor panel
    ("4", ("gemm", 300, 40, 100), [_panel(False, False, 100)], [_general(False, False, 64, False)]),
    ("5", ("gemm", 64, 64, 64), ["gemm_f64_tile16_kernel"], [_panel(False, False, 64)]),                           # panel for tile-16
    ("6", ("syrk", 256, 2048), ["syrk_blk_kernel"], ["syrk_lower_kernel<1>", "syrk_lower_kernel<0>"]),             # no one-read block kernel
])
def test_variant_arms_agree_with_the_default(variant, kind, default_kernels, arm_kernels, monkeypatch):
    """PLDA_GEMM64_VARIANT=1..6 are kept in the library as A/B arms: each must really switch the kernel and form the same
    product (to _check's tolerance, against NumPy and against the default arm)."""
    from plda_amd import MPlda
    monkeypatch.delenv("PLDA_GEMM64_VARIANT", raising=False)
    eng0 = MPlda(0)
    got0, want, tol = _family(eng0, kind)
    assert eng0.linalg_last_kernels() == default_kernels, eng0.linalg_last_kernels()
    monkeypatch.setenv("PLDA_GEMM64_VARIANT", variant)
    eng1 = MPlda(0)
    got1, _, _ = _family(eng1, kind)
    assert eng1.linalg_last_kernels() == arm_kernels, eng1.linalg_last_kernels()
    assert np.abs(got0 - want).max() <= tol and np.abs(got1 - want).max() <= tol and np.abs(got1 - got0).max() <= tol, \
        (variant, kind, np.abs(got0 - want).max(), np.abs(got1 - want).max(), tol)
