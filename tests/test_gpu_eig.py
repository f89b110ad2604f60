"""GPU: the symmetric eigensolver of GetOutput (csrc/eig_dc.hip: Householder tridiagonalisation + divide and
conquer + back-transformation; csrc/linalg.hip: block Jacobi) through plda_sym_eig, against numpy.linalg.eigh.
The reference reaches this step through Kaldi's SpMatrix::Eig inside PldaEstimator::GetOutput
(pldamodule.cpp:102-106); what GetOutput needs of it is: eigenvalues, an ORTHONORMAL set of eigenvectors
(any basis inside a cluster), small residual.  Hard cases: rank-deficient (the between-class covariance of fewer
speakers than dimensions), clusters, graded spectra, already-tridiagonal and diagonal input, extreme scales."""
import numpy as np
import pytest

import eig_hard_cases as hc

pytestmark = pytest.mark.gpu


def _cases(n, rng):
    A = rng.standard_normal((n, n))
    yield "gaussian", A + A.T
    B = rng.standard_normal((n, max(n // 3, 1)))
    yield "rank-deficient PSD", B @ B.T
    yield "identity", np.eye(n)
    yield "zero", np.zeros((n, n))
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.concatenate([np.ones(n // 2), np.full(n - n // 2, 2.0)])
    yield "two clusters", (q * lam) @ q.T
    yield "graded", (q * 10.0 ** (-np.arange(n) * 16.0 / n)) @ q.T
    yield "tridiagonal", (np.diag(np.abs(np.arange(n) - n // 2).astype(float)) + np.diag(np.ones(n - 1), 1)
                          + np.diag(np.ones(n - 1), -1))
    yield "diag + tiny coupling", np.diag(rng.random(n)) + 1e-12 * (A + A.T)
    yield "scaled 1e150", (A + A.T) * 1e150
    yield "scaled 1e-150", (A + A.T) * 1e-150


def _check(eng, name, G, method, expect_method=None, tol=5e-13):
    n = G.shape[0]
    G = 0.5 * (G + G.T)
    lam, V, used = eng.sym_eig(G, method)
    if expect_method is not None:
        assert used == expect_method, (name, n, used)
    ref = np.linalg.eigvalsh(G)[::-1]
    nrm = max(np.abs(ref).max(), 1e-300)
    assert np.all(np.diff(lam) <= 0), (name, n)
    e_val = np.abs(lam - ref).max() / nrm
    e_orth = np.abs(V @ V.T - np.eye(n)).max()
    Gs = G / nrm
    e_res = np.abs(V @ Gs - (lam / nrm)[:, None] * V).max()
    assert e_val < tol and e_orth < tol and e_res < tol, (name, n, method, e_val, e_orth, e_res)
    return e_val, e_orth, e_res


@pytest.mark.parametrize("n", [1, 2, 3, 5, 16, 17, 33, 64, 100, 200, 224, 256])
def test_direct_method_against_numpy(n):
    from plda_amd import MPlda
    eng = MPlda(0)
    rng = np.random.default_rng(n)
    for name, G in _cases(n, rng):
        _check(eng, name, G, method=2, expect_method=2)


@pytest.mark.parametrize("n", [161, 225, 257, 320, 512, 513, 1000, 1024, 1025, 1536, 2048])
def test_direct_method_large(n):
    """n > 160: the tridiagonalisation runs on ceil(n / 8) cooperating workgroups (register layouts of 7, 8, 16, 32 and
    64 elements per lane: the sizes straddle their limits; 2048 is the largest supported -- 256 workgroups, one per CU;
    above 1024 the row registers spill and only the direct method exists, the block Jacobi fallback stops at 1024)."""
    from plda_amd import MPlda
    eng = MPlda(0)
    rng = np.random.default_rng(n)
    for name, G in _cases(n, rng):
        _check(eng, name, G, method=2, expect_method=2, tol=2e-12)
        assert set(_expected_kernels(n, "default")) <= set(eng.linalg_last_kernels()), (n, name, eng.linalg_last_kernels())


@pytest.mark.parametrize("variant", ["2", "3"])
def test_both_tridiagonalisation_kernels(variant, monkeypatch):
    """PLDA_EIG_VARIANT=2: one workgroup, matrix in registers (n <= 256); 3: rows over cooperating workgroups."""
    monkeypatch.setenv("PLDA_EIG_VARIANT", variant)
    from plda_amd import MPlda
    eng = MPlda(0)
    for n in (3, 17, 100, 200, 256):
        rng = np.random.default_rng(1000 + n)
        for name, G in _cases(n, rng):
            _check(eng, name, G, method=2, expect_method=2)


def test_back_transformation_two_row_arm(monkeypatch):
    """PLDA_EIG_VARIANT=4: the default kernels with the two-rows-per-wave back-transformation of rounds 2-3 (the A/B arm of
    the one-row kernel with the eight-sums-at-once reduction that n <= 512 takes since round 4)."""
    monkeypatch.setenv("PLDA_EIG_VARIANT", "4")
    from plda_amd import MPlda
    eng = MPlda(0)
    for n in (9, 64, 200, 257, 512):
        rng = np.random.default_rng(2000 + n)
        for name, G in _cases(n, rng):
            _check(eng, name, G, method=2, expect_method=2, tol=2e-12)


@pytest.mark.parametrize("n", [5, 64, 200])
def test_jacobi_against_numpy(n):
    from plda_amd import MPlda
    eng = MPlda(0)
    rng = np.random.default_rng(100 + n)
    for name, G in _cases(n, rng):
        if name.startswith("scaled") or (name == "graded" and n > 64):
            # the Jacobi arm (fallback + warm starts of the per-iteration EM arm) is used unscaled and works on the
            # rows of G itself: with a spectrum graded over 16 decades the rows of the smallest eigenvalues are
            # rounding noise and its relative stopping test is never met (40 sweeps -> PLDA_E_NUMERIC).  The
            # direct method above covers these inputs.
            continue
        _check(eng, name, G, method=1, expect_method=1, tol=2e-11)   # stops at |cos| <= 4 eps sqrt(D) between rows


def test_default_dispatch_and_plda_like_input():
    """what fit uses: whitened between-class covariance of a PLDA-like problem, D = 200."""
    from plda_amd import MPlda
    eng = MPlda(0)
    rng = np.random.default_rng(7)
    D, K = 200, 1000
    W = np.cov(rng.standard_normal((D, 5000)))
    Bm = rng.standard_normal((D, K)) * (np.arange(D)[:, None] + 1.0) ** -1.0
    T1 = np.linalg.inv(np.linalg.cholesky(W))
    G = T1 @ (Bm @ Bm.T / K) @ T1.T
    _check(eng, "plda-like", G, method=0, expect_method=2)
    # fewer speakers than dimensions: D - K + 1 zero eigenvalues
    Bm = rng.standard_normal((D, 40))
    G = T1 @ (Bm @ Bm.T / 40) @ T1.T
    _check(eng, "plda-like rank 40", G, method=0, expect_method=2)


def test_non_finite_input_falls_back_or_fails_cleanly():
    from plda_amd import MPlda
    eng = MPlda(0)
    G = np.eye(8)
    G[2, 3] = G[3, 2] = np.nan
    with pytest.raises(Exception):
        eng.sym_eig(G, 2)


# ---- every dispatch class of the direct method, pinned by the kernels the library reports (linalg_last_kernels) ----
#
# The arms are read when the handle is created.  _expected_kernels restates the host-side switch of sym_eig_dc_f64
# (csrc/eig_dc.hip); when a threshold moves there, the sweeps below fail on the kernel name instead of quietly testing
# another class.

_ARMS = {"default": {}, "sweep2": {"PLDA_SWEEP_VARIANT": "2"}, "eig2": {"PLDA_EIG_VARIANT": "2"},
         "eig3": {"PLDA_EIG_VARIANT": "3"}, "eig4": {"PLDA_EIG_VARIANT": "4"}}
_RANGES = {"default": (1, 272), "sweep2": (1, 224), "eig2": (1, 256), "eig3": (3, 272), "eig4": (3, 272)}


def _names(kernel, args):
    return {"%s<%d>" % (kernel, a) for a in args}


_DEFAULT_TRIDIAG = (_names("tridiag_reg16_kernel", (1, 2, 14)) | _names("tridiag_full_kernel", range(3, 14))
                    | _names("tridiag_rows_kernel", (8, 16)))
# what each arm's sweep must have run, in full
_FULL = {
    "default": _DEFAULT_TRIDIAG | _names("householder_row1_kernel", (1, 2, 4, 8)),
    "sweep2": _names("tridiag_reg16_kernel", range(1, 15)) | _names("householder_row1_kernel", (1, 2, 4)),
    "eig2": _names("tridiag_reg_kernel", range(1, 9)) | _names("householder_row1_kernel", (1, 2, 4)),
    "eig3": _names("tridiag_rows_kernel", (7, 8, 16)) | _names("householder_row1_kernel", (1, 2, 4, 8)),
    "eig4": _DEFAULT_TRIDIAG | _names("householder_rows_kernel", (1, 2, 4, 8)),
}


def _ceil_div(a, b):
    return -(-a // b)


def _expected_kernels(n, arm):
    """(tridiagonalisation kernel, back-transformation kernel) of an n x n decomposition on `arm`."""
    ev0 = arm in ("default", "sweep2", "eig4")
    if arm in ("default", "eig4") and 32 < n <= 208:
        tri = "tridiag_full_kernel<%d>" % _ceil_div(n, 16)
    elif ev0 and n <= 224:
        tri = "tridiag_reg16_kernel<%d>" % _ceil_div(n, 16)
    elif (arm == "eig2" and n <= 256) or (arm not in ("eig2", "eig3") and n <= 160):
        tri = "tridiag_reg_kernel<%d>" % _ceil_div(n, 32)
    else:
        e = _ceil_div(n, 32)
        tri = "tridiag_rows_kernel<%d>" % (7 if e <= 7 else 8 if e <= 8 else 16 if e <= 16 else 32 if e <= 32 else 64)
    e = _ceil_div(n, 64)
    ee = 1 if e <= 1 else 2 if e <= 2 else 4 if e <= 4 else 8 if e <= 8 else 16 if e <= 16 else 32
    back = "householder_row%s_kernel<%d>" % ("1" if arm != "eig4" and ee <= 8 else "s", ee)
    return tri, back


def _assert_union(seen, expected, what):
    """the kernels a sweep reported are exactly the instantiations it claims to cover"""
    assert seen == expected, "%s: never ran %s; ran unexpectedly %s" % (what, sorted(expected - seen), sorted(seen - expected))


def _sweep_matrices(n):
    """the two matrices of a size sweep: the seeded Gaussian A + A^T and the hard case n mod 13"""
    rng = np.random.default_rng(7000 + n)
    A = rng.standard_normal((n, n))
    return [("gaussian", A + A.T), hc.hard_cases(n, rng)[n % hc.N_HARD]]


_REF = {}   # (key) -> what numpy.linalg.eigh gives on that matrix; computed once, shared by every arm


def _reference(key, G):
    if key not in _REF:
        n = G.shape[0]
        w, Z = np.linalg.eigh(G)
        nrm = max(np.abs(w).max(), 1e-300)
        _REF[key] = (np.linalg.eigvalsh(G)[::-1], nrm, np.abs(Z.T @ Z - np.eye(n)).max(),
                     np.abs((G / nrm) @ Z - Z * (w / nrm)[None, :]).max())
    return _REF[key]


def _check_ref(eng, key, G, bad):
    """The three quantities of _check, bounded RELATIVE TO LAPACK: with e_ref the same quantity of numpy.linalg.eigh's own
    output on the same matrix (0 for the eigenvalues), bound = 8 max(e_ref, n eps), never above _check's caps (5e-13 up to
    n = 256, 2e-12 above).  The factor: the NumPy prototype of this algorithm stays within 4 x LAPACK on every hard case
    (and below 0.1 n eps in absolute terms); the device differs from it by reduction order, FMA contraction and
    Newton-refined reciprocals.  Failures are collected in `bad` so that one run reports every offender."""
    n = G.shape[0]
    lam, V, used = eng.sym_eig(G, 2)
    ref, nrm, o_ref, r_ref = _reference(key, G)
    cap = 5e-13 if n <= 256 else 2e-12
    floor = n * hc.EPS
    b_val, b_orth, b_res = min(8 * floor, cap), min(8 * max(o_ref, floor), cap), min(8 * max(r_ref, floor), cap)
    e_val = np.abs(lam - ref).max() / nrm
    e_orth = np.abs(V @ V.T - np.eye(n)).max()
    e_res = np.abs(V @ (G / nrm) - (lam / nrm)[:, None] * V).max()
    print("eig %-44s val %.2e/%.2e orth %.2e/%.2e res %.2e/%.2e" % (key, e_val, b_val, e_orth, b_orth, e_res, b_res))
    if used != 2 or not np.all(np.diff(lam) <= 0) or not (e_val <= b_val and e_orth <= b_orth and e_res <= b_res):
        bad.append((key, used, e_val, b_val, e_orth, b_orth, e_res, b_res))


def _chunks(arm):
    lo, hi = _RANGES[arm]
    return [(arm, a, min(a + 63, hi)) for a in range(lo, hi + 1, 64)]


@pytest.mark.parametrize("arm,lo,hi", [c for arm in _ARMS for c in _chunks(arm)])
def test_every_size_of_every_tridiagonalisation_arm(arm, lo, hi, monkeypatch):
    """Every n of the arm's range (in chunks of 64 sizes per test id), two matrices each: every register layout of the
    four tridiagonalisation kernels (tridiag_full <3..13>, tridiag_reg16 <1..14>, tridiag_reg <1..8>, tridiag_rows <7>,
    <8>, <16> with every n mod 8, its rows being dealt to ceil(n / 8) workgroups) and of the two back-transformations
    (householder_row1 / householder_rows <1, 2, 4, 8>, with all eight tails (n - 2) mod 8 of the compact-WY blocks)."""
    for k, v in _ARMS[arm].items():
        monkeypatch.setenv(k, v)
    from plda_amd import MPlda
    eng = MPlda(0)
    bad, seen, expected = [], set(), set()
    for n in range(lo, hi + 1):
        want = _expected_kernels(n, arm)
        expected |= set(want)
        for name, G in _sweep_matrices(n):
            _check_ref(eng, "sweep n=%d %s" % (n, name), G, bad)
            ran = eng.linalg_last_kernels()
            assert set(want) <= set(ran), (arm, n, want, ran)
            seen |= {k for k in ran if k.startswith(("tridiag_", "householder_"))}
    _assert_union(seen, expected, "%s n=%d..%d" % (arm, lo, hi))
    full = set()
    for n in range(_RANGES[arm][0], _RANGES[arm][1] + 1):
        full |= set(_expected_kernels(n, arm))
    _assert_union(full, _FULL[arm], "the chunks of arm %s together" % arm)
    assert not bad, bad


@pytest.mark.parametrize("n", [21, 101, 105, 210, 255])
@pytest.mark.parametrize("arm", ["default", "eig3"])
def test_hard_cases_of_divide_and_conquer(arm, n, monkeypatch):
    """The whole list of tests/eig_hard_cases.py: merges with one and two surviving poles (k == 1 has a branch of its own
    in dc_merge_roots_kernel), runs of type-2 deflation, negative off-diagonals, glued Wilkinson matrices
    (tests/test_proto_dc_eig.py asserts on the prototype's merge statistics that the cases produce exactly those)."""
    for k, v in _ARMS[arm].items():
        monkeypatch.setenv(k, v)
    from plda_amd import MPlda
    eng = MPlda(0)
    bad = []
    for name, G in hc.hard_cases(n, np.random.default_rng(n)):
        _check_ref(eng, "hard n=%d %s" % (n, name), G, bad)
        assert set(_expected_kernels(n, arm)) <= set(eng.linalg_last_kernels()), (arm, n, name, eng.linalg_last_kernels())
    assert not bad, bad


def _jacobi_sizes():
    return [(1, 48), (49, 96), (97, 136), (160, 160), (200, 200), (255, 255), (256, 256), (257, 257), (512, 512)]


@pytest.mark.parametrize("variant", [None, "1"])
@pytest.mark.parametrize("lo,hi", _jacobi_sizes())
def test_jacobi_every_size(lo, hi, variant, monkeypatch):
    """Block Jacobi (method 1) at every n up to 136 (rows in blocks of four: every remainder, odd and even block counts,
    one to three 64-lane strides per row) and at the sizes around the larger strides, in the Gram form (default) and
    rotation by rotation (PLDA_JACOBI_VARIANT=1); the cases and the bound of test_jacobi_against_numpy.

    Regression test of the second, shifted stage of sym_eig_f64 (csrc/linalg.hip): orthogonal rows of A = V G diagonalise
    G^2, so eigenvalues +l and -l' of nearly equal magnitude stayed mixed -- the Gaussian matrices of n = 87, 113, 160, 512
    left residuals of 3.9e-11, 2.2e-11, 5.0e-11 and 3.1e-11 |G| (1024: 3.6e-10) with eigenvalues and orthogonality at
    1e-13, against the 2e-11 asserted here."""
    if variant is None:
        monkeypatch.delenv("PLDA_JACOBI_VARIANT", raising=False)
    else:
        monkeypatch.setenv("PLDA_JACOBI_VARIANT", variant)
    from plda_amd import MPlda
    eng = MPlda(0)
    for n in range(lo, hi + 1):
        rng = np.random.default_rng(100 + n)
        e = _ceil_div(n, 64)
        want = "jacobi_gram_kernel" if variant is None else "jacobi_block_kernel<%d>" % (1 if e <= 1 else 2 if e <= 2 else 4 if e <= 4 else 8)
        for name, G in _cases(n, rng):
            if name.startswith("scaled") or (name == "graded" and n > 64):
                continue      # (as in test_jacobi_against_numpy)
            _check(eng, name, G, method=1, expect_method=1, tol=2e-11)
            if n > 1:
                assert eng.linalg_last_kernels() == [want], (n, name, eng.linalg_last_kernels())


@pytest.mark.parametrize("variant", [None, "1"])
def test_jacobi_at_its_limit(variant, monkeypatch):
    """n = 1024, the largest size the block Jacobi solver takes (16 rows of A and V in LDS), one Gaussian matrix."""
    if variant is None:
        monkeypatch.delenv("PLDA_JACOBI_VARIANT", raising=False)
    else:
        monkeypatch.setenv("PLDA_JACOBI_VARIANT", variant)
    from plda_amd import MPlda
    eng = MPlda(0)
    A = np.random.default_rng(1124).standard_normal((1024, 1024))
    _check(eng, "gaussian", A + A.T, method=1, expect_method=1, tol=2e-11)
    assert eng.linalg_last_kernels() == ["jacobi_gram_kernel" if variant is None else "jacobi_block_kernel<16>"]
