"""CPU: the host model of the cosine back-end's operands (tests/cosine_model.py) -- that it is a cosine, that the fp32 chain
stays within its budget, that the kernel's summation order does not leave the project's bit-identity cap, and that the
mutants the GPU test must be able to see do leave it.  Also the WCCN / LDA identity behind fit_embedding(kind="wccn") and the
ABI surface of the feature."""
import ctypes as C

import numpy as np
import pytest

import cosine_model as cm
import fp32_chain as fc

LIMIT = 20000
# D = 1: a unit vector of length one is exactly +-1 whatever the arithmetic, and row M / 2 = 0 is the zero row -- no mutant of
# the operands can show there, so the mutants run from D = 7 on
MUTANT_SHAPES = [s for s in cm.SHAPES if s[2] > 1]


def _id(s):
    return "%dx%dx%d" % s


@pytest.fixture(scope="module")
def cases():
    """(operands, pairs, chain) of every shape, with and without statistics: computed once, never written to."""
    out = {}
    for shape in cm.SHAPES:
        for stats in (False, True):
            U, V, zm, zs = cm.case(*shape, stats=stats)
            op = cm.operands(U, V, zm, zs)
            pairs = fc.sample_pairs(shape[0], shape[1], LIMIT)
            out[shape, stats] = (U, V, zm, zs, op, pairs, fc.chain(op.A32, op.B32, pairs))
    return out


@pytest.mark.parametrize("stats", [False, True], ids=["raw", "znorm"])
@pytest.mark.parametrize("shape", cm.SHAPES, ids=_id)
def test_exact_is_the_numpy_cosine_and_the_chain_is_within_budget(cases, shape, stats):
    U, V, zm, zs, op, pairs, got = cases[shape, stats]
    ii, jj = pairs
    M, Nt, D = shape
    assert op.depth == D and op.Kg == max(-(-D // 8) * 8, 16) and op.A32.shape == (M, 2 + op.Kg) and op.B32.shape == (Nt, 2 + op.Kg)
    assert (op.B32[:, 0] == 1).all() and (op.B32[:, 1] == 0).all() and (op.A32[:, 2 + D:] == 0).all() and (op.B32[:, 2 + D:] == 0).all()
    cos = cm.cosine_matrix(U, V)[ii, jj]
    want = zn = cos
    if stats:
        # the model's "exact" carries s_i = fp32(1 / zstd_i) on the cosine, as the operands do (fp32_chain's convention): equal to
        # cos s_i - zmean_i / zstd_i to fp64 roundings, and to the z-norm proper within the 2^-24 of that one rounding
        has = zs != 0.0
        sc = np.where(has, 1.0 / np.where(has, zs, 1.0), 1.0)
        want = np.where(has[ii], cos * sc.astype(np.float32).astype(np.float64)[ii] - zm[ii] * sc[ii], cos)
        zn = np.where(has[ii], (cos - zm[ii]) * sc[ii], cos)
    ex = fc.exact(op, pairs)
    scale = 1.0 + np.abs(want) + (np.abs(zm[ii]) / np.where(zs == 0, 1.0, zs)[ii] if stats else 0.0)
    assert np.all(np.abs(ex - want) <= 64 * D * 2.0 ** -53 * scale), np.abs(ex - want).max()
    assert np.all(np.abs(ex - zn) <= 2.0 ** -23 * scale)
    if not stats:
        assert (ex[ii == M // 2] == 0).all()             # the zero row scores 0
    assert np.all(np.abs(got.astype(np.float64) - ex) <= fc.budget(op, pairs))


@pytest.mark.parametrize("stats", [False, True], ids=["raw", "znorm"])
@pytest.mark.parametrize("shape", cm.SHAPES, ids=_id)
def test_kernel_summation_order_stays_within_the_cap(cases, shape, stats):
    U, V, zm, zs, op, pairs, want = cases[shape, stats]
    lanes = cm.operands(U, V, zm, zs, order="lanes")
    ok, frac, ulp = fc.check(fc.chain(lanes.A32, lanes.B32, pairs), want, fc.allowance(op, pairs))
    print("%s %s: lane order %.4f %% identical, %d ulp" % (_id(shape), stats, 100 * frac, ulp))
    assert ok, (frac, ulp)


def test_lane_order_sum_is_a_sum_of_squares():
    rng = np.random.default_rng(3)
    for D in (1, 7, 63, 64, 65, 200, 513, 2048):
        X = rng.standard_normal((9, D)) * 7
        ss = cm.sumsq_lanes(X)
        assert np.all(np.abs(ss - np.sum(X * X, axis=1)) <= D * 2.0 ** -52 * ss)
    assert cm.sumsq_lanes(np.zeros((2, 70))).tolist() == [0.0, 0.0]


MUTANTS = {
    "round_toward_zero": dict(rnd=fc.round_trunc),
    "norm_in_fp32": dict(norm_fp32=True),
    "scale_after_rounding": dict(scale_after=True),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
@pytest.mark.parametrize("shape", MUTANT_SHAPES, ids=_id)
def test_mutants_fail_the_check(cases, shape, mutant):
    """With statistics (the scale mutant is the identity without them)."""
    U, V, zm, zs, op, pairs, want = cases[shape, True]
    mut = cm.operands(U, V, zm, zs, **MUTANTS[mutant])
    ok, frac, ulp = fc.check(fc.chain(mut.A32, mut.B32, pairs), want, fc.allowance(op, pairs))
    print("%s %s: %.1f %% identical, %d ulp" % (_id(shape), mutant, 100 * frac, ulp))
    assert not ok, (frac, ulp)


def test_pairs_model_is_the_cosine_and_its_map():
    U, V, zm, zs = cm.case(40, 30, 65, stats=True)
    rng = np.random.default_rng(5)
    e, t = rng.integers(0, 40, 500), rng.integers(0, 30, 500)
    mapped, c = cm.pairs(U, V, e, t, zm, zs)
    cos = cm.cosine_matrix(U, V)[e, t]
    assert np.all(np.abs(c.astype(np.float64) - cos) <= 2.0 ** -45)
    has = zs[e] != 0
    assert (mapped[~has] == c[~has]).all() and (c[e == 20] == 0).all()
    assert np.all(np.abs(mapped[has].astype(np.float64) - (cos[has] - zm[e][has]) / zs[e][has]) <= 2.0 ** -40)


def test_wccn_and_full_rank_lda_give_the_same_cosines():
    """WCCN (A W A^T = I by a Cholesky factor) and full-rank LDA (A W A^T = I and A B A^T diagonal) differ by a rotation."""
    rng = np.random.default_rng(11)
    D, K, per = 24, 30, 12
    spk = rng.standard_normal((K, D)) @ rng.standard_normal((D, D))
    X = np.repeat(spk, per, axis=0) + rng.standard_normal((K * per, D)) @ (rng.standard_normal((D, D)) * 0.7)
    y = np.repeat(np.arange(K), per)
    means = np.stack([X[y == k].mean(0) for k in range(K)])
    Xc = X - means[y]
    W = Xc.T @ Xc / len(X)
    Bc = means - X.mean(0)
    B = Bc.T @ Bc / K
    L = np.linalg.cholesky(W)
    A_wccn = np.linalg.inv(L)                                   # A W A^T = I
    lam, Q = np.linalg.eigh(A_wccn @ B @ A_wccn.T)
    A_lda = Q.T[::-1] @ A_wccn                                  # A W A^T = I, A B A^T = diag(lam), descending
    assert np.allclose(A_lda @ W @ A_lda.T, np.eye(D), atol=1e-9)
    G = A_lda @ B @ A_lda.T
    assert np.allclose(G - np.diag(np.diag(G)), 0, atol=1e-9 * np.abs(G).max())
    T = rng.standard_normal((50, D))
    c1 = cm.cosine_matrix(X[:40] @ A_wccn.T, T @ A_wccn.T)
    c2 = cm.cosine_matrix(X[:40] @ A_lda.T, T @ A_lda.T)
    assert np.abs(c1 - c2).max() <= 1e-10


def test_backend_exports_are_in_the_ctypes_table():
    from plda_amd import _native
    i32 = C.c_int32
    assert _native.SIGNATURES["plda_backend_set"] == (C.c_int, [C.c_void_p, i32, i32])
    assert _native.SIGNATURES["plda_backend_get"] == (C.c_int, [C.c_void_p, C.POINTER(i32), C.POINTER(i32)])
