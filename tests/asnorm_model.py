"""Host model of the AS-norm kernels (plda_amd/csrc/snorm.hip), for the tests: the definitions of include/plda_hip.h
restated in NumPy, independent of the product's arithmetic.

  topk_stats(S32, K)     per row of an fp32 score matrix: mean and POPULATION std of the K largest values (ties at the
                         boundary are equal values, so the multiset is well defined; -0.0 == +0.0).  Selection by
                         np.partition on the fp32 values; moments in np.longdouble, two-pass, around the boundary value tau
                         (s - tau is exact), rounded once to float64.  All-equal top-K sets give std exactly 0 and mean
                         exactly that value.
  compaction_attempts(row32, K)   the structure of the selection kernel restated: per attempt to compact the candidates into
                         LDS, (level, candidates, the largest count in one of the 16 wave shares) -- the tests use it to know
                         which path a row takes (candidates <= GATE and a share above WCAP: the cap overflow)
  snorm_sides / snorm_apply   the two-sided map on finished fp32 scores in fp64 (NOT rounded to fp32: the caller rounds).
"""
import numpy as np


def topk_values(row32, K):
    """The K largest values of one fp32 row (any order)."""
    row32 = np.asarray(row32, np.float32)
    n = row32.shape[0]
    assert 1 <= K <= n
    return np.partition(row32, n - K)[n - K:]


def topk_stats(S32, K):
    S32 = np.atleast_2d(np.asarray(S32, np.float32))
    mean = np.empty(S32.shape[0])
    std = np.empty(S32.shape[0])
    for r in range(S32.shape[0]):
        T = topk_values(S32[r], K)
        tau = T.min()
        d = T.astype(np.longdouble) - np.longdouble(tau)
        m1 = d.sum() / np.longdouble(K)
        var = ((d - m1) ** 2).sum() / np.longdouble(K)
        mean[r] = float(np.longdouble(tau) + m1)
        std[r] = float(np.sqrt(var))
    return mean, std


def topk_width(S32, K):
    """max T(r) - min T(r) per row, in fp64 (the `w` of the derived tolerances)."""
    S32 = np.atleast_2d(np.asarray(S32, np.float32))
    return np.array([np.float64(T.max()) - np.float64(T.min()) for T in (topk_values(row, K) for row in S32)])


WAVES, WCAP, GATE = 16, 1024, 8192         # SN_WAVES, SN_WCAP, SN_GATE of csrc/snorm.hip
LEVELS = ((21, 11), (10, 11), (0, 10))     # (shift, bits) of the three radix levels


def _keys(row32):
    u = np.ascontiguousarray(row32, np.float32).view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)
    return np.where(u & 0x80000000, u ^ 0xffffffff, u | 0x80000000).astype(np.uint64)


def compaction_attempts(row32, K):
    """[(level, candidates, max per wave share)] of one row: after a level the keys at or above the boundary bin's lower edge
    are compacted, each of the 16 waves its contiguous share of quads, when they number at most GATE; a share above WCAP
    overflows and the next level tries again."""
    key = _keys(row32)
    nc = key.shape[0]
    seg = -(-((nc + 3) // 4) // WAVES)
    wave = (np.arange(nc) // 4) // seg
    prefix, above_all, out = 0, 0, []
    for level, (shift, bits) in enumerate(LEVELS):
        live = key if level == 0 else key[(key >> np.uint64(shift + bits)) == prefix]
        hist = np.bincount(((live >> np.uint64(shift)) & np.uint64((1 << bits) - 1)).astype(np.int64), minlength=1 << bits)[::-1]
        cum = np.cumsum(hist)
        i = int(np.searchsorted(cum, K - above_all))
        above_all += int(cum[i] - hist[i])
        prefix = (prefix << bits) | ((1 << bits) - 1 - i)
        if level < 2 and above_all + int(hist[i]) <= GATE:
            cand = key >= np.uint64(prefix << shift)
            per = np.bincount(wave[cand], minlength=WAVES)
            out.append((level, int(cand.sum()), int(per.max())))
            if per.max() <= WCAP:
                break
    return out


def snorm_sides(raw32, emean=None, estd=None, tmean=None, tstd=None):
    """(side_e, side_t) in fp64, each [M, Nt] or None: side(raw, m, s) = (raw - m) / s if s != 0 else raw."""
    raw = np.asarray(raw32, np.float32).astype(np.float64)

    def side(m, s, axis):
        if m is None:
            return None
        m = np.asarray(m, np.float64)
        s = np.asarray(s, np.float64)
        m, s = (m[:, None], s[:, None]) if axis == 0 else (m[None, :], s[None, :])
        ok = s != 0.0
        return np.where(ok, (raw - m) / np.where(ok, s, 1.0), raw)
    return side(emean, estd, 0), side(tmean, tstd, 1)


def snorm_apply(raw32, emean=None, estd=None, tmean=None, tstd=None):
    se, st = snorm_sides(raw32, emean, estd, tmean, tstd)
    assert se is not None or st is not None
    if se is None:
        return st
    if st is None:
        return se
    return 0.5 * (se + st)


def ulp32(x):
    """Spacing of fp32 at |x| (of the smallest subnormal below the normal range)."""
    x = np.abs(np.asarray(x, np.float64))
    big = np.minimum(x, np.float64(np.finfo(np.float32).max)).astype(np.float32)
    return np.spacing(big).astype(np.float64)


def stats_tolerance(S32, K, mean, std):
    """The derived bounds of the GPU statistics against topk_stats (fp64 sums of K fp32 values, a handful of roundings each):
    w = max T - min T, delta = 8 K 2^-53 w^2;  |dmean| <= 8 K 2^-53 w + 2^-52 |mean|,  |dstd| <= min(delta / std, sqrt(delta)) +
    2^-52 std."""
    w = topk_width(S32, K)
    u = 2.0 ** -53
    delta = 8.0 * K * u * w * w
    tol_mean = 8.0 * K * u * w + 2.0 ** -52 * np.abs(mean)
    with np.errstate(divide="ignore", invalid="ignore"):
        by_std = np.where(std > 0, delta / np.where(std > 0, std, 1.0), np.inf)
    tol_std = np.minimum(by_std, np.sqrt(delta)) + 2.0 ** -52 * std
    return tol_mean, tol_std
