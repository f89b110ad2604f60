// plda_amd/csrc/snorm.hip -- adaptive symmetric score normalisation (AS-norm / S-norm).
//
// The reference normalises on the enrol side only ("z-norm (other norms are not implemented yet)", its README;
// pldamodule.cpp:196-277).  Here a trial is normalised on BOTH sides, each side against the K LARGEST of its scores
// against a cohort:
//   cohort_topk_stats_kernel   per row of a slab of fp32 cohort scores: the K-th largest value tau by radix refinement on
//                              score_key (11 + 11 + 10 bits, per-row LDS histograms, the crossing found on the device),
//                              then mean and population std of the K largest values from fp64 sums of (s - tau);
//   snorm_apply_kernel         out = 0.5 ((raw - em_i) / es_i + (raw - tm_j) / ts_j) on a slab of finished fp32 scores,
//                              evaluated in fp64 and rounded once.
// The scores themselves are the trials GEMM's (score.hip), one row slab at a time: produced, consumed, dropped.
#include "common.hpp"

#include <algorithm>

namespace plda {

namespace {

// the order-preserving key of eer.hip: a < b <=> key(a) < key(b), -0.0 == +0.0
__device__ __forceinline__ unsigned sn_key(float f) {
  unsigned u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sn_key_value(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

constexpr int SN_THREADS = 1024;
constexpr int SN_WAVES = SN_THREADS / 64;
constexpr int SN_BINS = 2048;
constexpr int SN_COPIES = 8;      // histogram copies, interleaved [bin][lane & 7]: equal bins of one wave spread over 8 banks
constexpr int SN_WCAP = 1024;     // candidate keys per wave (64 KiB for the workgroup)
constexpr int SN_GATE = 8192;     // compaction is tried when the candidates number at most this (half the list: waves differ)

struct SnShared {
  unsigned hist[SN_BINS * SN_COPIES];       // 64 KiB
  unsigned list[SN_WAVES][SN_WCAP];         // 64 KiB: the keys >= the boundary bin's lower edge, per wave in a fixed order
  unsigned wcnt[SN_WAVES], wtot[SN_WAVES];
  unsigned res_bin, res_above, res_cnt;
  int overflow;
  double red[2][SN_WAVES];
};

__device__ __forceinline__ int sn_level_shift(int level) { return level == 0 ? 21 : level == 1 ? 10 : 0; }
__device__ __forceinline__ int sn_level_bits(int level) { return level == 2 ? 10 : 11; }

// every element of the wave's share of the row, four 16-byte loads in flight per lane; f(key, valid) is called by ALL lanes
// of the wave the same number of times (f may ballot)
template <typename F>
__device__ __forceinline__ void sn_scan_row(const float *__restrict__ row, int Nc, int q0, int q1, int lane, F &&f) {
  for (int qb = q0; qb < q1; qb += 256) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = qb + u * 64 + lane;
      v[u] = q < q1 ? *reinterpret_cast<const float4 *>(row + 4 * (int64_t)q) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = qb + u * 64 + lane;
      const int e = 4 * q;
      const bool ok = q < q1;
      f(sn_key(v[u].x), ok && e < Nc);
      f(sn_key(v[u].y), ok && e + 1 < Nc);
      f(sn_key(v[u].z), ok && e + 2 < Nc);
      f(sn_key(v[u].w), ok && e + 3 < Nc);
    }
  }
}
template <typename F>
__device__ __forceinline__ void sn_scan_list(const SnShared &sm, int wave, int lane, F &&f) {
  const unsigned n = sm.wcnt[wave];
  for (unsigned i = lane; i < n; i += 64) f(sm.list[wave][i], true);
}

__device__ __forceinline__ void sn_zero_hist(SnShared &sm, int tid) {
  for (int i = tid; i < SN_BINS * SN_COPIES; i += SN_THREADS) sm.hist[i] = 0u;
}

// The bin in which the krem-th largest of the histogrammed keys lies, the number of keys in higher bins and in it.  Called by
// all threads after the histogram's atomics; leaves the histogram zeroed and the workgroup synchronised.
__device__ __forceinline__ void sn_find_bin(SnShared &sm, int tid, unsigned krem, unsigned &bin, unsigned &above, unsigned &cnt) {
  const int lane = tid & 63, wave = tid >> 6;
  __syncthreads();
  // thread t owns bins 2047 - 2t and 2046 - 2t: a prefix sum over the threads runs from the highest bin downwards
  const int hi = SN_BINS - 1 - 2 * tid, lo = hi - 1;
  unsigned c_hi = 0, c_lo = 0;
#pragma unroll
  for (int c = 0; c < SN_COPIES; ++c) { c_hi += sm.hist[hi * SN_COPIES + c]; c_lo += sm.hist[lo * SN_COPIES + c]; }
  const unsigned local = c_hi + c_lo;
  unsigned incl = local;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned x = __shfl_up(incl, o);
    if (lane >= o) incl += x;
  }
  if (lane == 63) sm.wtot[wave] = incl;
  __syncthreads();
  unsigned excl = incl - local;
  for (int w = 0; w < wave; ++w) excl += sm.wtot[w];
  if (excl < krem && krem <= excl + c_hi) { sm.res_bin = (unsigned)hi; sm.res_above = excl; sm.res_cnt = c_hi; }
  else if (excl + c_hi < krem && krem <= excl + local) { sm.res_bin = (unsigned)lo; sm.res_above = excl + c_hi; sm.res_cnt = c_lo; }
  sn_zero_hist(sm, tid);
  __syncthreads();
  bin = sm.res_bin; above = sm.res_above; cnt = sm.res_cnt;
}

// One workgroup per row.  S: a slab the trials GEMM has just written, 16-byte aligned, ld % 4 == 0 (columns [Nc, ld) are
// never used).  Exact selection without a sort and without a cap on K:
//   level 0..2: histogram of the next 11 / 11 / 10 key bits of the elements that share the prefix found so far, and the bin
//   where the count from the top crosses K.  As soon as the elements at or above the boundary bin number <= SN_GATE, ONE more
//   read compacts their keys into LDS, where the remaining levels and the sums finish (two reads of the row: the usual case,
//   K of a few hundred).  Otherwise (a large K, a boundary bin full of ties) the levels go on over the row and a last read
//   sums with tau known (up to four reads).
// Deterministic: integer histograms; every wave owns a contiguous share of the row and compacts it in a fixed order (ballots,
// no atomics); the fp64 sums are reduced in a fixed order.  Nothing depends on the slab height or the grid.
__global__ __launch_bounds__(SN_THREADS) void cohort_topk_stats_kernel(const float *__restrict__ S, int64_t ld, int Nc, int K,
                                                                       double *__restrict__ mean, double *__restrict__ stdv) {
  __shared__ SnShared sm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float *__restrict__ row = S + (int64_t)blockIdx.x * ld;
  const int Q = (Nc + 3) >> 2;
  const int segQ = (Q + SN_WAVES - 1) / SN_WAVES;
  const int q0 = min(wave * segQ, Q), q1 = min(q0 + segQ, Q);

  sn_zero_hist(sm, tid);
  if (tid == 0) sm.overflow = 0;
  __syncthreads();

  unsigned prefix = 0u, A = 0u;      // the key bits fixed so far; the number of elements whose key lies above that prefix
  bool in_lds = false;
  int level = 0;
  for (; level < 3; ++level) {
    const int shift = sn_level_shift(level), bits = sn_level_bits(level);
    const unsigned mask = (1u << bits) - 1u;
    const int hi_shift = shift + bits;             // (32 at level 0: no prefix yet)
    auto account = [&](unsigned k, bool valid) {
      if (valid && (level == 0 || (k >> hi_shift) == prefix)) atomicAdd(&sm.hist[((k >> shift) & mask) * SN_COPIES + (lane & (SN_COPIES - 1))], 1u);
    };
    if (in_lds) sn_scan_list(sm, wave, lane, account);
    else sn_scan_row(row, Nc, q0, q1, lane, account);
    unsigned bin, above, cnt;
    sn_find_bin(sm, tid, (unsigned)K - A, bin, above, cnt);
    A += above;
    prefix = (prefix << bits) | bin;
    if (!in_lds && level < 2 && A + cnt <= (unsigned)SN_GATE) {
      // the candidates: every key at or above the boundary bin's lower edge
      const unsigned lowkey = prefix << shift;
      unsigned n = 0;
      sn_scan_row(row, Nc, q0, q1, lane, [&](unsigned k, bool valid) {
        const bool cand = valid && k >= lowkey;
        const unsigned long long m = __ballot(cand);
        if (m) {
          const unsigned pos = n + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
          if (cand && pos < (unsigned)SN_WCAP) sm.list[wave][pos] = k;
          n += (unsigned)__popcll(m);
        }
      });
      if (lane == 0) {
        sm.wcnt[wave] = n < (unsigned)SN_WCAP ? n : (unsigned)SN_WCAP;
        if (n > (unsigned)SN_WCAP) sm.overflow = 1;
      }
      __syncthreads();
      const bool ovf = sm.overflow != 0;
      __syncthreads();
      if (tid == 0) sm.overflow = 0;       // (a later attempt at the next level starts clean; ordered by sn_find_bin's barriers)
      in_lds = !ovf;
    }
  }
  // prefix is now the key of tau, the K-th largest value; A elements lie strictly above it
  const unsigned tkey = prefix;
  const double tau = (double)sn_key_value(tkey);
  double s1 = 0.0, s2 = 0.0;
  auto add = [&](unsigned k, bool valid) {
    if (valid && k > tkey) {
      const double d = (double)sn_key_value(k) - tau;      // exact in fp64
      s1 += d;
      s2 = fma(d, d, s2);
    }
  };
  if (in_lds) sn_scan_list(sm, wave, lane, add);
  else sn_scan_row(row, Nc, q0, q1, lane, add);
  s1 = wave_sum_f64(s1);
  s2 = wave_sum_f64(s2);
  if (lane == 0) { sm.red[0][wave] = s1; sm.red[1][wave] = s2; }
  __syncthreads();
  if (tid == 0) {
    double t1 = 0.0, t2 = 0.0;
    for (int w = 0; w < SN_WAVES; ++w) { t1 += sm.red[0][w]; t2 += sm.red[1][w]; }
    const double m1 = t1 / (double)K;
    const double var = t2 / (double)K - m1 * m1;
    mean[blockIdx.x] = tau + m1;
    stdv[blockIdx.x] = sqrt(var > 0.0 ? var : 0.0);
  }
}

// The two-sided map on finished fp32 scores, in place: S[i, j] <- float(0.5 (side(raw, em_i, es_i) + side(raw, tm_j, ts_j))),
// side(raw, m, s) = (raw - m) / s where s != 0, else raw (the reference's guard, pldamodule.cpp:269-273); with one pair
// absent, float(side) of the other.  fp64 throughout, one rounding to fp32; a zero std is carried as (m, 1 / s) = (0, 1),
// which leaves raw exactly.  A thread keeps the statistics of its four columns in registers and walks AP_ROWS rows; the
// columns [Nt, ld) are not touched.
constexpr int AP_ROWS = 32;
__global__ __launch_bounds__(256) void snorm_apply_kernel(float *__restrict__ S, int64_t ld, int64_t M, int64_t Nt,
                                                          const double *__restrict__ em, const double *__restrict__ es,
                                                          const double *__restrict__ tm, const double *__restrict__ ts, int vec) {
  const int64_t j0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (j0 >= Nt) return;
  const int nc = (int)(Nt - j0 < 4 ? Nt - j0 : 4);
  double cm[4] = {0.0, 0.0, 0.0, 0.0}, ci[4] = {1.0, 1.0, 1.0, 1.0};
  if (tm) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < nc) {
        const double s = ts[j0 + c];
        if (s != 0.0) { cm[c] = tm[j0 + c]; ci[c] = 1.0 / s; }
      }
    }
  }
  const double half = (em && tm) ? 0.5 : 1.0;
  const int64_t r0 = (int64_t)blockIdx.y * AP_ROWS, r1 = r0 + AP_ROWS < M ? r0 + AP_ROWS : M;
  for (int64_t r = r0; r < r1; ++r) {
    double rm = 0.0, ri = 1.0;
    if (em) {
      const double s = es[r];
      if (s != 0.0) { rm = em[r]; ri = 1.0 / s; }
    }
    float *p = S + r * ld + j0;
    float x[4];
    if (vec && nc == 4) {
      const float4 v = *reinterpret_cast<const float4 *>(p);
      x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) x[c] = c < nc ? p[c] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double raw = (double)x[c];
      double o;
      if (em && tm) o = half * ((raw - rm) * ri + (raw - cm[c]) * ci[c]);
      else if (em) o = (raw - rm) * ri;
      else o = (raw - cm[c]) * ci[c];
      x[c] = (float)o;
    }
    if (vec && nc == 4) *reinterpret_cast<float4 *>(p) = make_float4(x[0], x[1], x[2], x[3]);
    else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < nc) p[c] = x[c];
    }
  }
}

// rows of one slab of fp32 scores, ld floats per row: <= 2 GiB in whole 256-row tiles, never more than 4 GiB.  Measured at
// 50 000 x 200 000: slabs small enough to stay in the 256 MiB Infinity Cache between the GEMM and its consumer
// (256 rows) cost 58 ms against 44 ms at 2 560 rows -- a tile grid one tile high leaves the GEMM's per-XCD queues short and
// pays the per-launch preparation 196 times, which outweighs the consumer's cache hits.
}  // namespace

int64_t sn_slab_rows(const plda_handle *h, int64_t total_rows, int64_t ld) {
  int64_t rows = std::max<int64_t>(256, (((int64_t)2 << 30) / 4 / ld) / 256 * 256);
  if (h->sn_slab_rows > 0) rows = round_up(h->sn_slab_rows, 128);       // PLDA_SNORM_SLAB_ROWS: small slabs for the tests
  rows = std::min(rows, ((int64_t)4 << 30) / 4 / ld);
  return std::min(rows, total_rows);
}

int cohort_stats_device(plda_handle *h, const double *dX, const int32_t *dn, int n_uniform, int64_t R, const double *dC,
                        int64_t Nc, int64_t top_k, double *dmean, double *dstd, const CountSet *cs_in) {
  if (!can_score(h)) return fail(h, PLDA_E_NOT_FITTED, "cohort_stats: model not fitted");
  if (R < 1) return fail(h, PLDA_E_INVAL, "cohort_stats: R = %lld (must be >= 1)", (long long)R);
  if (Nc < 1) return fail(h, PLDA_E_INVAL, "cohort_stats: Nc = %lld (must be >= 1)", (long long)Nc);
  if (Nc > ((int64_t)1 << 30)) return fail(h, PLDA_E_INVAL, "cohort_stats: Nc = %lld (at most 2^30: one row of scores must fit a slab)", (long long)Nc);
  if (top_k < 1 || top_k > Nc) return fail(h, PLDA_E_INVAL, "cohort_stats: top_k = %lld (must be in 1 ... Nc = %lld)", (long long)top_k, (long long)Nc);
  if (!dX) return fail(h, PLDA_E_INVAL, "cohort_stats: X is NULL");
  if (!dC) return fail(h, PLDA_E_INVAL, "cohort_stats: cohort is NULL");
  if (!dmean) return fail(h, PLDA_E_INVAL, "cohort_stats: mean is NULL");
  if (!dstd) return fail(h, PLDA_E_INVAL, "cohort_stats: std is NULL");
  if (!dn && n_uniform <= 0) return fail(h, PLDA_E_INVAL, "cohort_stats: n_uniform must be > 0 when n is NULL");
  const int D = h->Dout;
  CountSet cs_local;
  const CountSet *cs = nullptr;
  if (dn) {
    if (cs_in) cs = cs_in;
    else { PLDA_TRY(score_count_set_device(h, dn, R, &cs_local)); cs = &cs_local; }
  }
  const int64_t ld = round_up(Nc, 4);
  const int64_t rows = sn_slab_rows(h, R, ld);
  PLDA_HIP(h, h->sn_slab.reserve((size_t)rows * ld * 4));
  float *slab = h->sn_slab.as<float>();
  h->prep_valid = false;           // (the slabs pack the cohort side themselves, once)
  for (int64_t r0 = 0; r0 < R; r0 += rows) {
    const int64_t m = std::min(rows, R - r0);
    {
      TraceScope ts(h, "snorm.cohort_gemm", 0.0, 1);
      PLDA_TRY(score_matrix_device(h, dX + r0 * D, dn ? dn + r0 : nullptr, n_uniform, m, dC, Nc, nullptr, nullptr, slab, ld,
                                   /*reuse_packed_B=*/r0 > 0, cs));
      if (ts.idx >= 0) h->trace_spans[ts.idx].work = 2.0 * (double)h->last_k * (double)m * (double)Nc;
    }
    TraceScope ts(h, "snorm.cohort_select", (double)m * (double)Nc * 4.0, 2);
    cohort_topk_stats_kernel<<<(unsigned)m, SN_THREADS, 0, h->stream>>>(slab, ld, (int)Nc, (int)top_k, dmean + r0, dstd + r0);
    PLDA_LAUNCH_CHECK(h);
  }
  h->last_M = R; h->last_Nt = Nc;
  return PLDA_OK;
}

int score_matrix_snorm_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV,
                              int64_t Nt, const double *demean, const double *destd, const double *dtmean, const double *dtstd,
                              float *dout, int64_t ld, const CountSet *cs_in, bool reuse_packed_B) {
  if (!can_score(h)) return fail(h, PLDA_E_NOT_FITTED, "score_matrix_snorm: model not fitted");
  if ((demean == nullptr) != (destd == nullptr)) return fail(h, PLDA_E_INVAL, "score_matrix_snorm: %s is NULL but its partner is not", demean ? "estd" : "emean");
  if ((dtmean == nullptr) != (dtstd == nullptr)) return fail(h, PLDA_E_INVAL, "score_matrix_snorm: %s is NULL but its partner is not", dtmean ? "tstd" : "tmean");
  if (!demean && !dtmean) return fail(h, PLDA_E_INVAL, "score_matrix_snorm: both statistic pairs are NULL (emean/estd or tmean/tstd must be given)");
  if (M < 1) return fail(h, PLDA_E_INVAL, "score_matrix_snorm: M = %lld (must be >= 1)", (long long)M);
  if (Nt < 1) return fail(h, PLDA_E_INVAL, "score_matrix_snorm: Nt = %lld (must be >= 1)", (long long)Nt);
  if (!dU) return fail(h, PLDA_E_INVAL, "score_matrix_snorm: U is NULL");
  if (!dV) return fail(h, PLDA_E_INVAL, "score_matrix_snorm: V is NULL");
  if (!dout) return fail(h, PLDA_E_INVAL, "score_matrix_snorm: out is NULL");
  if (ld < Nt) return fail(h, PLDA_E_INVAL, "score_matrix_snorm: ld_out = %lld < Nt = %lld", (long long)ld, (long long)Nt);
  if (!dn && n_uniform <= 0) return fail(h, PLDA_E_INVAL, "score_matrix_snorm: n_uniform must be > 0 when n_enrol is NULL");
  const int D = h->Dout;
  CountSet cs_local;
  const CountSet *cs = nullptr;
  if (dn) {
    if (cs_in) cs = cs_in;
    else { PLDA_TRY(score_count_set_device(h, dn, M, &cs_local)); cs = &cs_local; }
  }
  const int64_t rows = sn_slab_rows(h, M, ld);
  const int vec = ((ld & 3) == 0 && (reinterpret_cast<uintptr_t>(dout) & 15) == 0) ? 1 : 0;
  for (int64_t r0 = 0; r0 < M; r0 += rows) {
    const int64_t m = std::min(rows, M - r0);
    float *o = dout + r0 * ld;
    PLDA_TRY(score_matrix_device(h, dU + r0 * D, dn ? dn + r0 : nullptr, n_uniform, m, dV, Nt, nullptr, nullptr, o, ld,
                                 reuse_packed_B || r0 > 0, cs));
    TraceScope ts(h, "snorm.apply", (double)m * (double)Nt * 8.0, 2);
    const dim3 grid((unsigned)ceil_div(Nt, 1024), (unsigned)ceil_div(m, AP_ROWS));
    snorm_apply_kernel<<<grid, 256, 0, h->stream>>>(o, ld, m, Nt, demean ? demean + r0 : nullptr, destd ? destd + r0 : nullptr, dtmean, dtstd, vec);
    PLDA_LAUNCH_CHECK(h);
  }
  h->last_M = M; h->last_Nt = Nt;
  return PLDA_OK;
}

}  // namespace plda
