"""Host model of the fp32 trials GEMM, bit for bit (plda_amd/csrc/score.hip, score_bt4.inc).

Every fp32 trials score is a k-ordered chain of correctly rounded fp32 fused multiply-adds
(v_mfma_f32_32x32x2_f32: D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)), one rounding per product, subnormals
kept) over operands that the prep kernels compute in fp64 and round once to fp32.  This module rebuilds
those operands and that chain on the host, so a test can predict the kernel's bits:

  columns 0, 1   the rank-2 bias pair (r'_i, s_i) x (1, q_j), srcC = 0: acc = fma(s_i, q_j, fma(r'_i, 1, 0))
                 (the 128 x 128 kernel forms the same value as fmaf(s_i, q_j, r'_i))
  columns 2 ..   the packed k-planes in memory order, Kg of them (a multiple of 8):
                   uniform n   A1 = c u / var (* s_i)                       against  v
                   bucketed    A1, then s_i x onehot(b_i - 1)               against  v, then dq_1 .. dq_(G-1)
                               (G - 1 columns padded with zeros to a multiple of 8)
                   depth-2D    A1 (Dp columns), A2 = -1/2 (1/var - 1/(1+psi)) (* s_i) against v, v*v (Dp columns)
                 zero columns pad D up to Dp = round_up(D, 8) and the depth up to 16.

K order (trials_gemm_kernel, header of score.hip "step = 8 k"): per 8-k step p, lane half h reads k-quad
2p + h and component t of the float4 feeds MFMA t, so the chain runs
    8p, 8p+4, 8p+1, 8p+5, 8p+2, 8p+6, 8p+3, 8p+7
after the bias pair.  The 256 x 256 kernels (bt2, bt4) use the same fragment scheme and order.

z-norm (enrol_bias_kernel, prep_side_body, prep_enrol_buckets_body): s_i = fp32(1 / zstd_i) scales the
fp64 A operand before its rounding; r'_i = (r_i - zmean_i) / zstd_i in fp64 (the fp64 reciprocal, not the
rounded s_i); zstd_i == 0 leaves the row as it is (s_i = 1).

The bf16x3 arm (score_bf16x3.inc, scripts/proto_bf16_split.py) contracts the same fp32 operands as three
bf16 terms each, six products kept.  The order of the bf16 MFMA's internal additions is not documented,
so for that arm this module models the error SIZE (`bf16x3_bound`, `bf16x3_emulate`), not the bits.
"""
import numpy as np

U32 = 2.0 ** -24          # unit roundoff of fp32
CS_MAX, CS_NMAX = 64, 4095  # plda_amd/csrc/common.hpp: the bucketed form's limits


# ------------------------------------------------------------------------------------------ fp32 fma
def fma32(a, b, c):
    """Correctly rounded fp32 fma(a, b, c) (round to nearest even) on arrays of fp32 values.

    a*b of two fp32 values is exact in fp64.  p + c is then rounded once to fp64 (s) and once more to
    fp32: that double rounding is wrong only when s lands exactly on an fp32 midpoint, where the TwoSum
    error term e (s + e == p + c exactly) says on which side the exact value lies."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    with np.errstate(over="ignore", invalid="ignore"):
        r = s.astype(np.float32)
        d = s - r.astype(np.float64)                          # exact (Sterbenz)
        toward = np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
        nb = np.nextafter(r, toward)                          # the fp32 neighbour on s's side
        mid = (d != 0) & ((r.astype(np.float64) + nb.astype(np.float64)) * 0.5 == s)
        fix = mid & (e != 0) & ((e > 0) == (d > 0))           # exact value beyond the midpoint, away from r
    return np.where(fix, nb, r).astype(np.float32)


# ------------------------------------------------------------------------------------------ k order
def kernel_order(Kg):
    """Column order of the chain: the bias pair, then the packed k-planes in the MFMA order."""
    assert Kg % 8 == 0, Kg
    main = [8 * p + 4 * h + t for p in range(Kg // 8) for t in range(4) for h in range(2)]
    return np.array([0, 1] + [2 + k for k in main], np.int64)


def chain(A32, B32, pairs=None, order=None):
    """acc = fma32(A[i, k], B[j, k], acc) over the columns in `order` (default: the kernel's), from acc = 0.

    A32 [M, K], B32 [N, K] (fp32, bias pair in columns 0, 1).  pairs = (i_idx, j_idx) evaluates only
    those elements (1-D result); None evaluates all of them ([M, N] result)."""
    A32 = np.asarray(A32, np.float32)
    B32 = np.asarray(B32, np.float32)
    if pairs is None:
        M, N = A32.shape[0], B32.shape[0]
        ii, jj = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
        return chain(A32, B32, (ii.ravel(), jj.ravel()), order).reshape(M, N)
    ii, jj = (np.asarray(x, np.int64) for x in pairs)
    if order is None:
        order = kernel_order(A32.shape[1] - 2)
    At, Bt = np.ascontiguousarray(A32.T), np.ascontiguousarray(B32.T)
    acc = np.zeros(ii.shape[0], np.float32)
    for k in order:
        acc = fma32(At[k][ii], Bt[k][jj], acc)
    return acc


# ------------------------------------------------------------------------------------------ operands
def round_rn(x):
    return np.asarray(x, np.float64).astype(np.float32)


def round_trunc(x):
    """fp64 -> fp32 rounded toward zero (a mutant: what a truncating conversion would pack)."""
    x = np.asarray(x, np.float64)
    r = x.astype(np.float32)
    over = np.abs(r.astype(np.float64)) > np.abs(x)
    return np.where(over, np.nextafter(r, np.float32(0)), r).astype(np.float32)


def _coef(n, psi):
    """llr_coef: c = n psi / (n psi + 1), var = 1 + psi / (n psi + 1) (fp64, the kernels' expression order)."""
    den = n * psi + 1.0
    return n * psi / den, 1.0 + psi / den


def _count_table(psi, n):
    """count_coef: w = c^2 / var, g = 1 / var - 1 / (1 + psi), L = sum_d (log var - log(1 + psi))."""
    c, var = _coef(float(n), psi)
    return c * c / var, 1.0 / var - 1.0 / (1.0 + psi), float(np.sum(np.log(var) - np.log(1.0 + psi)))


def buckets_usable(D, G):
    Dp = -(-D // 8) * 8
    return 2 <= G <= CS_MAX and G - 1 <= max(Dp // 2, 8)


def count_set(counts):
    """The distinct counts as the library finds them, or None when they take the depth-2D form."""
    counts = np.asarray(counts)
    if counts.min() < 1 or counts.max() > CS_NMAX:
        return None
    vals = np.unique(counts)
    return vals if len(vals) <= CS_MAX else None


def pick_form(D, n, mixed_variant=0, cs=None):
    """Which operand form the library takes: 'uniform', 'buckets' or 'depth2d' (score.hip: prepare_operands)."""
    if np.ndim(n) == 0:
        return "uniform"
    cs = count_set(n) if cs is None else cs
    if cs is not None and len(cs) == 1:
        return "uniform"
    if mixed_variant == 1 or cs is None or not buckets_usable(D, len(cs)):
        return "depth2d"
    return "buckets"


class Operands:
    """fp32 operands A32 [M, 2 + Kg], B32 [N, 2 + Kg] and their fp64 values before rounding (A64, B64)."""

    def __init__(self, A64, B64, A32, B32, form, depth):
        self.A64, self.B64, self.A32, self.B32 = A64, B64, A32, B32
        self.form, self.depth = form, depth      # depth: the library's algorithmic depth (score_last_shape()[2])

    @property
    def Kg(self):
        return self.A32.shape[1] - 2


def operands(psi, U, V, n, zmean=None, zstd=None, form=None, cs=None, rnd=round_rn, r_fp32=False, swap_bucket=None):
    """Operands of the trials GEMM for enrol rows U [M, D] with counts n (an int, or an int array) and test
    rows V [N, D], as the prep kernels pack them.

    form: 'uniform' / 'buckets' / 'depth2d' (None: as the library picks it); cs: the count set of the call
    (None: the distinct values of n; a prepared test side brings its own, wider set).
    Mutants: rnd (fp64 -> fp32 conversion), r_fp32 (r_i summed in fp32), swap_bucket = g (rows of bucket g
    get the one-hot column of bucket g + 1 and vice versa)."""
    psi = np.asarray(psi, np.float64)
    U = np.asarray(U, np.float64)
    V = np.asarray(V, np.float64)
    M, D = U.shape
    N = V.shape[0]
    Dp = -(-D // 8) * 8
    if form is None:
        form = pick_form(D, n, cs=cs)
    if form == "uniform" and np.ndim(n) != 0:
        n = int(np.asarray(n).ravel()[0])
    nrow = np.broadcast_to(np.asarray(n, np.float64), (M,)).astype(np.float64)

    # z-norm: s = fp32(1 / zstd) scales A (as a double), r' = (r - zmean) / zstd in fp64; zstd == 0: untouched
    zn = zmean is not None and zstd is not None
    sc64 = np.ones(M)
    if zn:
        zstd = np.asarray(zstd, np.float64)
        zmean = np.asarray(zmean, np.float64)
        has = zstd != 0.0
        sc64 = np.where(has, 1.0 / np.where(has, zstd, 1.0), 1.0)
    s32 = sc64.astype(np.float32)
    rs = s32.astype(np.float64)[:, None]

    def rsum(x):  # the row sums of r_i (fp64; the mutant sums in fp32)
        return np.sum(x.astype(np.float32), axis=1, dtype=np.float32).astype(np.float64) if r_fp32 else np.sum(x, axis=1)

    cols_a, cols_b = [], []
    if form == "uniform":
        w, g, L = _count_table(psi, n)
        c, var = _coef(float(n), psi)
        r = -0.5 * (rsum(w * U * U) + L)
        q = -0.5 * np.sum(g * V * V, axis=1)
        A1 = c * U / var * rs
        Kg = max(Dp, 16)
        Amain, Bmain = np.zeros((M, Kg)), np.zeros((N, Kg))
        Amain[:, :D], Bmain[:, :D] = A1, V
        depth = D
    elif form == "buckets":
        vals = np.unique(np.asarray(n)) if cs is None else np.asarray(cs)
        G = len(vals)
        b = np.searchsorted(vals, np.asarray(n))
        assert (vals[b] == np.asarray(n)).all(), "a count outside the call's count set"
        tabs = [_count_table(psi, v) for v in vals]
        c, var = _coef(nrow[:, None], psi[None, :])
        Lr = np.array([tabs[k][2] for k in b])
        r = -0.5 * (rsum((c * c / var) * U * U) + Lr)
        q = -0.5 * np.sum(tabs[0][1] * V * V, axis=1)
        A1 = c * U / var * rs
        Gx = -(-(G - 1) // 8) * 8
        Kg = Dp + Gx
        Amain, Bmain = np.zeros((M, Kg)), np.zeros((N, Kg))
        Amain[:, :D], Bmain[:, :D] = A1, V
        bb = b.copy()
        if swap_bucket is not None:
            g0 = swap_bucket
            bb[b == g0], bb[b == g0 + 1] = g0 + 1, g0
        rows = np.nonzero(bb > 0)[0]
        Amain[rows, Dp + bb[rows] - 1] = s32[rows]
        for k in range(1, G):
            Bmain[:, Dp + k - 1] = -0.5 * np.sum((tabs[k][1] - tabs[0][1]) * (V * V), axis=1)
        depth = D + G - 1
    elif form == "depth2d":
        c, var = _coef(nrow[:, None], psi[None, :])
        cu = c * U
        r = -0.5 * rsum(np.log(var) - np.log(1.0 + psi) + cu * cu / var)
        q = np.zeros(N)
        Kg = max(2 * Dp, 16)
        Amain, Bmain = np.zeros((M, Kg)), np.zeros((N, Kg))
        Amain[:, :D] = c * U / var * rs
        Amain[:, Dp:Dp + D] = -0.5 * (1.0 / var - 1.0 / (1.0 + psi)) * rs
        Bmain[:, :D], Bmain[:, Dp:Dp + D] = V, V * V
        depth = 2 * D
    else:
        raise ValueError(form)
    if zn:
        r = np.where(has, (r - zmean) * sc64, r)
    A64 = np.concatenate([np.stack([r, sc64], 1), Amain], 1)
    B64 = np.concatenate([np.stack([np.ones(N), q], 1), Bmain], 1)
    A32, B32 = rnd(A64), rnd(B64)
    return Operands(A64, B64, A32, B32, form, depth)


# ------------------------------------------------------------------------------------------ error budgets
def exact(op, pairs):
    """The fp64 value of the contraction on the unrounded fp64 operands (the fp64 oracle's GEMM form)."""
    ii, jj = pairs
    return np.einsum("pk,pk->p", op.A64[ii], op.B64[jj])


def budget(op, pairs):
    """Rigorous bound of |chain(A32, B32) - exact(A64, B64)|:

        gamma_K sum_k |a_k b_k|                     the K fp32 roundings of the chain (K = Kg + 2,
                                                    gamma_K = K u / (1 - K u), u = 2^-24)
      + sum_k |a_k b_k - a64_k b64_k|               the rounding of every operand from fp64 to fp32
      + 2^-50 sum_k |a64_k b64_k|                   slack for the fp64 evaluation of the two sums above"""
    ii, jj = pairs
    K = op.A32.shape[1]
    gam = K * U32 / (1.0 - K * U32)
    a32, b32 = op.A32[ii].astype(np.float64), op.B32[jj].astype(np.float64)
    a64, b64 = op.A64[ii], op.B64[jj]
    p32 = np.abs(a32 * b32).sum(1)
    return gam * p32 + np.abs(a32 * b32 - a64 * b64).sum(1) + 2.0 ** -50 * np.abs(a64 * b64).sum(1)


def magnitude(op, pairs):
    """sum_k |a_k b_k| of the fp32 operands: the natural scale of an element's partial sums."""
    ii, jj = pairs
    return np.abs(op.A32[ii].astype(np.float64) * op.B32[jj].astype(np.float64)).sum(1)


# The allowance for elements that are not bit-identical: 2 ulp (2^-22) of sum_k |a_k b_k|.  One operand whose
# fp32 rounding the prep kernel's fp64 evaluation order (lane-strided sums, the xor butterfly, fma contraction)
# flips moves its product by at most 2^-24 |a_k b_k| (relative to the product) and nudges the later partial sums
# across at most a rounding boundary or two; 2^-22 sum|ab| covers that with room while staying 1/K of `budget`.
ALLOW_ULPS = 2.0


def allowance(op, pairs):
    return ALLOW_ULPS * 2.0 ** -23 * magnitude(op, pairs)


def compare(got, model, allow):
    """(fraction bit-identical, max deviation in fp32 ulps, all non-identical elements within `allow`)."""
    got = np.asarray(got, np.float32)
    model = np.asarray(model, np.float32)
    same = (got == model) | (np.isnan(got) & np.isnan(model))
    gi = got.view(np.int32).astype(np.int64)
    mi = model.view(np.int32).astype(np.int64)
    gi = np.where(gi < 0, -(gi & 0x7fffffff), gi)       # sign-magnitude -> monotone integers
    mi = np.where(mi < 0, -(mi & 0x7fffffff), mi)
    ulps = np.where(same, 0, np.abs(gi - mi))
    dev = np.abs(got.astype(np.float64) - model.astype(np.float64))
    ok = bool(np.all(same | (dev <= allow)))
    return float(same.mean()), int(ulps.max()) if ulps.size else 0, ok


def check(got, model, allow, min_identical=0.999):
    frac, ulp, ok = compare(got, model, allow)
    return ok and frac >= min_identical, frac, ulp


# ------------------------------------------------------------------------------------------ bf16x3 arm
def bf16_rn(x):
    """fp32 -> bf16 (round to nearest even, as bf16_rn_bits), returned as fp32 values."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    h = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return (h.astype(np.uint32) << 16).view(np.float32)


def split3(x):
    """x = x0 + x1 + x2 (split_bf16x3_kernel: each remainder exact in fp32)."""
    x = np.asarray(x, np.float32)
    x0 = bf16_rn(x)
    r1 = (x - x0).astype(np.float32)
    x1 = bf16_rn(r1)
    x2 = bf16_rn((r1 - x1).astype(np.float32))
    return x0, x1, x2


KEPT3 = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))      # products of the arm (score_bf16x3.inc header)
KEPT2 = ((0, 0), (0, 1), (1, 0))                               # a bf16x2-grade contraction (a mutant)
DROPPED3 = ((1, 2), (2, 1), (2, 2))


def bf16x3_emulate(op, pairs, kept=KEPT3):
    """The arm's arithmetic in one admissible order: acc = fp32(r' + s q), then per k the kept bf16 products
    (exact in fp32) added in fp32.  An error-size model: the MFMA's own addition order is not documented."""
    ii, jj = pairs
    At, Bt = np.ascontiguousarray(op.A32.T), np.ascontiguousarray(op.B32.T)
    acc = fma32(At[1][ii], Bt[1][jj], At[0][ii])
    for k in kernel_order(op.Kg)[2:]:
        sa, sb = split3(At[k][ii]), split3(Bt[k][jj])
        for x, y in kept:
            acc = fma32(sa[x], sb[y], acc)
    return acc


def bf16x3_bound(op, pairs):
    """Bound of |bf16x3 score - exact|: the three dropped products, fp32 accumulation of the 6 K kept products
    in any order (gamma with u = 2^-23, so that a truncating accumulator is covered too) and the operand
    rounding from fp64 to fp32."""
    ii, jj = pairs
    K = op.Kg
    At, Bt = op.A32[ii], op.B32[jj]
    sa = [s.astype(np.float64) for s in split3(At)]
    sb = [s.astype(np.float64) for s in split3(Bt)]
    drop = sum(np.abs(sa[x] * sb[y])[:, 2:].sum(1) for x, y in DROPPED3)
    kept = sum(np.abs(sa[x] * sb[y])[:, 2:].sum(1) for x, y in KEPT3)
    n = 6 * K + 2
    gam = n * 2.0 ** -23 / (1.0 - n * 2.0 ** -23)
    a32, b32 = At.astype(np.float64), Bt.astype(np.float64)
    bias = np.abs(a32[:, :2] * b32[:, :2]).sum(1)
    oprnd = np.abs(a32 * b32 - op.A64[ii] * op.B64[jj]).sum(1) + 2.0 ** -50 * np.abs(op.A64[ii] * op.B64[jj]).sum(1)
    return drop + gam * (kept + bias) + oprnd


def rms(x):
    x = np.asarray(x, np.float64)
    return float(np.sqrt(np.mean(x * x)))


# ------------------------------------------------------------------------------------------ sampling
def sample_pairs(M, N, limit, seed=0, tiles=(128, 256)):
    """All M x N elements when that is at most `limit`; otherwise `limit` random ones plus, for every tile
    edge of the kernels' tilings, the last row and the last column (with a random partner index)."""
    if M * N <= limit:
        ii, jj = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
        return ii.ravel(), jj.ravel()
    rng = np.random.default_rng(seed)
    ii = [rng.integers(0, M, limit)]
    jj = [rng.integers(0, N, limit)]
    for t in tiles:
        er = np.unique(np.minimum(np.arange(t - 1, M + t - 1, t), M - 1))
        ec = np.unique(np.minimum(np.arange(t - 1, N + t - 1, t), N - 1))
        ii += [er, rng.integers(0, M, len(ec)), er[: len(ec)] if len(er) >= len(ec) else np.resize(er, len(ec))]
        jj += [rng.integers(0, N, len(er)), ec, ec]
    return np.concatenate(ii), np.concatenate(jj)
