"""Host model of the cosine back-end's operands (plda_amd/csrc/cosine.hip), to the operation.

The trials GEMM contracts S_ij = A_i . B_j + r'_i 1 + s_i q_j (tests/fp32_chain.py models the chain bit for bit).  On a cosine
handle the prep kernel fills those operands from the raw rows, all in fp64 up to the one rounding:

    ss(x) = sum_d x_d^2        inv(x) = 1 / sqrt(ss(x)), 0 when ss(x) == 0
    B_jd = fp32(v_jd inv(v_j))                      q_j = 0, cpair_j = (1, 0)
    sc_i = 1 / zstd_i where statistics are given and zstd_i != 0, else 1;   s_i = fp32(sc_i)
    A_id = fp32((u_id inv(u_i)) * fp64(s_i))        (the scale BEFORE the rounding, as the PLDA prep applies it)
    r'_i = fp32((0 - zmean_i) sc_i) where the row is normalised, else 0;    rpair_i = (r'_i, s_i)

A square is a product, rounded, and a sum (the file is built without contraction), so NumPy's x * x is the kernel's.  What
NumPy does not share is the ORDER of the sum: np.sum adds pairwise, the kernel lane-strided (lane l takes d = l, l + 64, ... in
increasing d) and then through the xor butterfly 32 ... 1.  `order="lanes"` is that order; the default is np.sum, and
tests/test_cosine_model.py shows that the two agree within fp32_chain.check (an fp64 ulp of ss moves an fp32 rounding of an
operand about once in 2^29 elements).
"""
import numpy as np

import fp32_chain as fc


def sumsq_lanes(X):
    """sum_d x_d^2 per row in the kernel's order: 64 lane partials over d = l, l + 64, ..., then the butterfly 32 ... 1."""
    X = np.asarray(X, np.float64)
    R, D = X.shape
    nch = -(-D // 64)
    P = np.zeros((R, nch * 64))
    P[:, :D] = X
    P = P.reshape(R, nch, 64)
    acc = np.zeros((R, 64))
    for c in range(nch):
        acc = acc + P[:, c, :] * P[:, c, :]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return acc[:, 0]


def inv_norm(ss):
    ss = np.asarray(ss, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ss == 0.0, 0.0, 1.0 / np.sqrt(ss))


def _sumsq(X, order, norm_fp32):
    if norm_fp32:       # mutant: the norm summed in fp32
        x = X.astype(np.float32)
        return np.sum(x * x, axis=1, dtype=np.float32).astype(np.float64)
    return sumsq_lanes(X) if order == "lanes" else np.sum(X * X, axis=1)


def operands(U, V, zmean=None, zstd=None, order="sum", rnd=fc.round_rn, norm_fp32=False, scale_after=False):
    """fc.Operands of a cosine call: columns 0 and 1 the bias pair, then Kg = max(round_up(D, 8), 16) planes, depth D.
    Mutants: rnd (the fp64 -> fp32 conversion), norm_fp32 (ss summed in fp32), scale_after (s_i applied to the ROUNDED unit
    vector, in fp32)."""
    U = np.asarray(U, np.float64)
    V = np.asarray(V, np.float64)
    M, D = U.shape
    N = V.shape[0]
    Kg = max(-(-D // 8) * 8, 16)
    zn = zmean is not None and zstd is not None
    sc64, r = np.ones(M), np.zeros(M)
    if zn:
        zstd = np.asarray(zstd, np.float64)
        zmean = np.asarray(zmean, np.float64)
        has = zstd != 0.0
        sc64 = np.where(has, 1.0 / np.where(has, zstd, 1.0), 1.0)
        r = np.where(has, (0.0 - zmean) * sc64, 0.0)
    s32 = sc64.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        un = U * inv_norm(_sumsq(U, order, norm_fp32))[:, None]
        vn = V * inv_norm(_sumsq(V, order, norm_fp32))[:, None]
        a = un * s32.astype(np.float64)[:, None]
    Amain, Bmain = np.zeros((M, Kg)), np.zeros((N, Kg))
    Amain[:, :D], Bmain[:, :D] = a, vn
    A64 = np.concatenate([np.stack([r, sc64], 1), Amain], 1)
    B64 = np.concatenate([np.stack([np.ones(N), np.zeros(N)], 1), Bmain], 1)
    with np.errstate(invalid="ignore", over="ignore"):
        A32, B32 = rnd(A64), rnd(B64)
        if scale_after:
            A32[:, 2:2 + D] = (rnd(un) * s32[:, None]).astype(np.float32)
    return fc.Operands(A64, B64, A32, B32, "cosine", D)


def pairs(U, V, e, t, zmean=None, zstd=None):
    """The trial-list score in np.longdouble: c = (u . v) inv(u) inv(v), then (c - zmean_e) / zstd_e where zstd_e != 0.
    Returns (mapped, c)."""
    U = np.asarray(U, np.longdouble)
    V = np.asarray(V, np.longdouble)
    e = np.asarray(e, np.int64)
    t = np.asarray(t, np.int64)
    u, v = U[e], V[t]
    su, sv = np.sum(u * u, axis=1), np.sum(v * v, axis=1)
    one = np.longdouble(1)
    iu = np.where(su == 0, 0, one / np.sqrt(np.where(su == 0, one, su)))
    iv = np.where(sv == 0, 0, one / np.sqrt(np.where(sv == 0, one, sv)))
    c = np.sum(u * v, axis=1) * iu * iv
    out = c
    if zmean is not None and zstd is not None:
        zm, zs = np.asarray(zmean, np.longdouble)[e], np.asarray(zstd, np.longdouble)[e]
        ok = zs != 0
        out = np.where(ok, (c - zm) / np.where(ok, zs, one), c)
    return out, c


def cosine_matrix(U, V):
    """The NumPy cosine, fp64 [M, N] (zero rows score 0)."""
    U = np.asarray(U, np.float64)
    V = np.asarray(V, np.float64)
    return (U * inv_norm(np.sum(U * U, axis=1))[:, None]) @ (V * inv_norm(np.sum(V * V, axis=1))[:, None]).T


SHAPES = [(1, 1, 1), (17, 33, 7), (65, 130, 64), (130, 257, 65), (300, 260, 200), (33, 515, 513), (40, 24, 2048)]


def case(M, Nt, D, seed=0, stats=False):
    """The rows of one test case: row M // 2 of U all zeros; with stats, zmean / zstd with zstd = 0 on every 7th row."""
    rng = np.random.default_rng(1000 * D + 10 * M + seed)
    U = rng.standard_normal((M, D)) * rng.uniform(0.1, 30.0, (M, 1))
    V = rng.standard_normal((Nt, D)) * rng.uniform(0.1, 30.0, (Nt, 1))
    U[M // 2] = 0.0
    zm = zs = None
    if stats:
        zm = rng.normal(0.02, 0.05, M)
        zs = rng.uniform(0.03, 0.3, M)
        zs[::7] = 0.0
    return U, V, zm, zs
