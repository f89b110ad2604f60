// plda_amd/csrc/eer.hip -- equal error rate of a trials matrix on the GPU (SURVEY.md section 8f
// rank 4).  Replaces /root/reference/scoring/eer.py:68-73, which calls
// bob.measure.eer_threshold(negatives, positives) and bob.measure.farfrr(...): `bob` is an
// absent, un-pinned third-party dependency, so (as for Kaldi) its published definition is
// restated -- oracle/plda_oracle_np.py:eer -- and parity for this row is UNPINNED:
//   farfrr(neg, pos, t):  FAR = #{neg >= t} / Nn,  FRR = #{pos < t} / Np
//   eer_threshold:        candidate thresholds are the minimum score and the midpoints
//                         between consecutive distinct scores of the union; the one with
//                         minimal |FAR - FRR| wins, the later one on ties.
// Sort-free: g(k) = FRR - FAR "after score k" is non-decreasing in k, so the minimum of |g|
// is at the smallest key k1 with g(k1) >= 0 or at its predecessor.  k1 is found EXACTLY by
// three HBM-bound passes over the fp32 scores that histogram an order-preserving uint32 key
// 11 + 11 + 10 bits at a time (per-block LDS histograms, float4 loads, column strips), with the crossing
// located in integer arithmetic on the host between passes.  Algorithmic bytes: 3 x 4 B per trial read, nothing written.
//
// Round 5, large matrices (one process): ONE pass over the matrix instead of three.  A pilot -- the same exact
// refinement on every 32nd row (3 % of the bytes) -- brackets the crossing: the key range [klo, khi) in which the
// SAMPLE's FRR - FAR passes from -delta to +delta, delta = five standard errors of the sample's rates.  The one full pass
// then counts, per class, the trials below klo and appends the scores inside the window to two compact lists (a few per
// mille of the trials; wave-aggregated appends), and the exact refinement finishes on the lists with the counts below
// as its starting offsets.  The answer is the three-pass one bit for bit whenever the window holds the crossing key and
// both of its neighbours -- checked with the exact counts (g(klo) < 0 <= g(khi), neighbours found inside); otherwise, and
// for small or sharded inputs, the three passes run.  PLDA_EER_VARIANT=1 forces them (A/B arm, and what the test compares with).
//
// Non-finite scores (NaN of either sign, +-Inf) among the trials are REFUSED with PLDA_E_INVAL and their exact count, as
// calibration, fusion and minDCF refuse them (the key order would place a NaN at either end of the scores according to its sign
// bit, and an Inf makes midpoints and DET steps NaN).  Three passes: bins 0..3 and 2044..2047 of the pass-0 histogram hold
// exactly the keys whose exponent is all ones -- free, and already global in the sharded forms.  Single pass: a counter of the
// window pass (the pilot sees every 32nd row only; +-Inf pass the window's compares).  DET: a counter of the min/max pass.
// The padding columns [Nt, ld) are never read as data.  On finite scores the restatement is the specification, including
// its last candidate `s_max + 1e-8`, which from |s_max| >= 2^27 on is s_max itself (eer_device's end).
//
// Where things live: the source of the trials (TrialSource: matrix, lists or slabs), the walk over its pieces
// (for_each_piece), the score key and the prototypes of every entry point here are in trial_source.hpp, shared with calib.hip
// and dcf.hip; the slab producer of the operand form (plda_score_eer_dev) is operand_slabs.hip.  This file: the kernels, the
// histogram pass (eer_pass), the poisoned reduction of the sharded forms (reduce_block_or_poison), the refinement, DET.
#include "trial_source.hpp"

#include <algorithm>
#include <cstring>

namespace plda {

// (score_key / key_score / EER_BINS / EER_STRIP: trial_source.hpp, shared with dcf.hip)

// one pass: class c (0 = impostor, 1 = target) histogram of bits [shift, shift + nbits) of the
// keys whose higher bits equal `prefix` (pass 0: every key).  below/above track the largest
// key below and the smallest key above the prefix range (needed for neighbours in pass 2).
typedef float f32x4e __attribute__((ext_vector_type(4)));

// Flat list of scores of one class (the two-list form of scoring/eer.py).
__global__ __launch_bounds__(256) void eer_hist_kernel(const float *__restrict__ scores, int64_t Nt, int fixed_class,
                                                       int shift, int nbits, unsigned prefix, int has_prefix,
                                                       unsigned long long *__restrict__ hist /*[2][EER_BINS]*/,
                                                       unsigned *__restrict__ below, unsigned *__restrict__ above) {
  __shared__ unsigned lh[2][EER_BINS];
  for (int i = threadIdx.x; i < 2 * EER_BINS; i += 256) (&lh[0][0])[i] = 0;
  __syncthreads();
  const unsigned mask = (1u << nbits) - 1u;
  const int hi_shift = shift + nbits;
  unsigned lo_max = 0u, hi_min = 0xffffffffu;

  auto account = [&](bool ok, float sc, int cls) {
    unsigned bin = 0xffffffffu;   // inactive
    if (ok) {
      const unsigned k = score_key(sc);
      if (has_prefix && (k >> hi_shift) != prefix) {
        if ((k >> hi_shift) < prefix) lo_max = k > lo_max ? k : lo_max; else hi_min = k < hi_min ? k : hi_min;
      } else {
        bin = ((k >> shift) & mask) | ((unsigned)cls << 11);
      }
    }
    // plain non-returning LDS atomics: aggregating lanes with equal bins first (12 ballots per element) was slower
    if (bin != 0xffffffffu) atomicAdd(&lh[bin >> 11][bin & 2047u], 1u);
  };

  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx - threadIdx.x < Nt; idx += (int64_t)gridDim.x * 256)
    account(idx < Nt, idx < Nt ? scores[idx] : 0.f, fixed_class);
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * EER_BINS; i += 256) {
    const unsigned v = (&lh[0][0])[i];
    if (v) atomicAdd(hist + i, (unsigned long long)v);
  }
  if (has_prefix) {
    if (lo_max) atomicMax(below, lo_max);
    if (hi_min != 0xffffffffu) atomicMin(above, hi_min);
  }
}

// Matrix pass, strip layout: a workgroup owns EER_STRIP columns -- 4 per thread, whose speaker ids stay in
// registers -- and walks down a slice of the rows, so that the only per-trial memory traffic is the 4-byte score.
// (Workgroups walking along rows re-read the 8-byte speaker id of every column for every row: 12 B of cache
// traffic per trial, 39.4 ms for the three passes over 1e10 trials against 20.4 ms here, identical results:
// profiles/r02_eer_probe.json.)  Four rows are loaded before they are accounted for.
__global__ __launch_bounds__(256) void eer_hist_strip_kernel(const float *__restrict__ scores, int64_t ld, int64_t M,
                                                             int64_t Nt, const int64_t *__restrict__ espk,
                                                             const int64_t *__restrict__ tspk, int64_t rows_per_wg,
                                                             int shift, int nbits, unsigned prefix, int has_prefix,
                                                             unsigned long long *__restrict__ hist,
                                                             unsigned *__restrict__ below, unsigned *__restrict__ above, int64_t row_step) {
  // (row_step > 1: the pilot's sample -- "row" r stands for matrix row r * row_step; M counts sample rows)
  __shared__ unsigned lh[2][EER_BINS];
  for (int i = threadIdx.x; i < 2 * EER_BINS; i += 256) (&lh[0][0])[i] = 0;
  __syncthreads();
  const unsigned mask = (1u << nbits) - 1u;
  const int hi_shift = shift + nbits;
  unsigned lo_max = 0u, hi_min = 0xffffffffu;
  const int64_t strips = (Nt + EER_STRIP - 1) / EER_STRIP;
  const int64_t strip = blockIdx.x % strips, slice = blockIdx.x / strips;
  const int64_t col = strip * EER_STRIP + (int64_t)threadIdx.x * 4;
  const int64_t r0 = slice * rows_per_wg, r1 = (r0 + rows_per_wg < M) ? r0 + rows_per_wg : M;
  int64_t ts[4];
  bool ok[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    ok[e] = col + e < Nt;
    ts[e] = ok[e] ? tspk[col + e] : 0;
  }
  const bool vec = ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(scores) & 15) == 0) && ok[3];

  auto account = [&](float sc, int cls) {
    const unsigned k = score_key(sc);
    if (has_prefix && (k >> hi_shift) != prefix) {
      if ((k >> hi_shift) < prefix) lo_max = k > lo_max ? k : lo_max; else hi_min = k < hi_min ? k : hi_min;
    } else {
      atomicAdd(&lh[cls][(k >> shift) & mask], 1u);
    }
  };

  for (int64_t row = r0; row < r1; row += 4) {
    float v[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (row + u >= r1) break;
      const float *src = scores + (row + u) * row_step * ld + col;
      if (vec) {
        const f32x4e x = __builtin_nontemporal_load(reinterpret_cast<const f32x4e *>(src));
        v[u][0] = x.x; v[u][1] = x.y; v[u][2] = x.z; v[u][3] = x.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[u][e] = ok[e] ? src[e] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (row + u >= r1) break;
      const int64_t spk = espk[(row + u) * row_step];
#pragma unroll
      for (int e = 0; e < 4; ++e) if (ok[e]) account(v[u][e], ts[e] == spk ? 1 : 0);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * EER_BINS; i += 256) {
    const unsigned c = (&lh[0][0])[i];
    if (c) atomicAdd(hist + i, (unsigned long long)c);
  }
  if (has_prefix) {
    if (lo_max) atomicMax(below, lo_max);
    if (hi_min != 0xffffffffu) atomicMin(above, hi_min);
  }
}

// The one full pass of the windowed form (same strip layout).  Per trial: two float compares against the window's
// ends (the key order is the float order, and -0 == +0 in both), one against infinity, the class, four predicated counters
// -- below the window per class, targets, non-finite scores -- and, for the few per mille inside it, a slot in the wave's LDS stage
// (an LDS atomic taken by those lanes only), which leaves for the class's list 512+ scores at a time behind ONE global
// atomic (one global atomic per wave and element serialises on the cursor's line: 0.8 s for a window of a tenth of 1e10
// trials, measured).  The non-finite scores (NaN of either sign, +-Inf) of the columns inside the matrix are counted here
// because the pilot sees every 32nd row only and +-Inf pass the window's compares; the caller refuses the call.  What lies at or
// above the window is not counted: it is the rest.  (It used to be, and the sum of all counters told a NaN; a fifth counter
// beside it cost the call 4 % -- 11.0 -> 11.5 ms on 1e10 trials -- so the new one took its place: same work per trial.)
// A list that fills up keeps counting (the cursor says by how much it overflowed).
struct EerWindowOut {
  unsigned long long below[2], targets, nonfinite, cursor[2];
};
constexpr int EER_WBUF = 1536;       // staged scores per wave and class (48 KB per workgroup); flushed when a batch (<= 1024 more) might not fit
__global__ __launch_bounds__(256) void eer_window_strip_kernel(const float *__restrict__ scores, int64_t ld, int64_t M, int64_t Nt,
                                                               const int64_t *__restrict__ espk, const int64_t *__restrict__ tspk,
                                                               int64_t rows_per_wg, float flo, float fhi, EerWindowOut *__restrict__ wo,
                                                               float *__restrict__ list0, float *__restrict__ list1, unsigned long long cap) {
  __shared__ unsigned long long red[4][4];
  __shared__ float stage[4][2][EER_WBUF];
  __shared__ int fillc[4][2];
  const int64_t strips = (Nt + EER_STRIP - 1) / EER_STRIP;
  const int64_t strip = blockIdx.x % strips, slice = blockIdx.x / strips;
  const int64_t col = strip * EER_STRIP + (int64_t)threadIdx.x * 4;
  const int64_t r0 = slice * rows_per_wg, r1 = (r0 + rows_per_wg < M) ? r0 + rows_per_wg : M;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t ts[4];
  bool ok[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    ok[e] = col + e < Nt;
    ts[e] = ok[e] ? tspk[col + e] : 0;
  }
  const bool vec = ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(scores) & 15) == 0) && ok[3];
  const float qnan = __uint_as_float(0x7fc00000u);
  unsigned b0 = 0, b1 = 0, t1 = 0, nf = 0;      // (a thread sees <= 4 * rows_per_wg trials: 32 bits)
  int *const fc = fillc[wave];
  if (lane < 2) fc[lane] = 0;
  auto flush = [&](int c) {
    const int n = __builtin_amdgcn_readfirstlane(fc[c]);
    if (n == 0) return;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&wo->cursor[c], (unsigned long long)n);
    base = __shfl(base, 0);
    float *dst = c ? list1 : list0;
    const float *src = stage[wave][c];
    for (int i = lane; i < n; i += 64)
      if (base + i < cap) dst[base + i] = src[i];
    if (lane == 0) fc[c] = 0;
  };
  for (int64_t row = r0; row < r1; row += 4) {
    float v[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (row + u >= r1) break;
      const float *src = scores + (row + u) * ld + col;
      if (vec) {
        const f32x4e x = __builtin_nontemporal_load(reinterpret_cast<const f32x4e *>(src));
        v[u][0] = x.x; v[u][1] = x.y; v[u][2] = x.z; v[u][3] = x.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[u][e] = ok[e] ? src[e] : qnan;     // (columns beyond the matrix: counted nowhere)
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (row + u >= r1) break;
      const int64_t spk = espk[row + u];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x = v[u][e];
        const bool tgt = ok[e] && ts[e] == spk;
        const bool lt_lo = x < flo, lt_hi = x < fhi;
        t1 += tgt ? 1u : 0u;
        b1 += (lt_lo && tgt) ? 1u : 0u;
        b0 += (lt_lo && !tgt) ? 1u : 0u;
        nf += !(__builtin_fabsf(x) < __builtin_inff()) ? 1u : 0u;     // NaN or Inf -- and the NaN put in for a column beyond the matrix
        if (lt_hi && !lt_lo) {
          const int c = tgt ? 1 : 0;
          const int slot = atomicAdd(&fc[c], 1);
          stage[wave][c][slot] = x;
        }
      }
    }
    if (__builtin_amdgcn_readfirstlane(fc[0]) > EER_WBUF - 1024) flush(0);
    if (__builtin_amdgcn_readfirstlane(fc[1]) > EER_WBUF - 1024) flush(1);
  }
  flush(0);
  flush(1);
  if (!vec && r1 > r0) {                        // take the NaNs of this thread's own making out again: one per row and missing column
    unsigned missing = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) missing += ok[e] ? 0u : 1u;
    nf -= missing * (unsigned)(r1 - r0);
  }
  unsigned long long c[4] = {b0, b1, t1, nf};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    for (int o = 32; o > 0; o >>= 1) c[q] += __shfl_xor(c[q], o);
    if (lane == 0) red[wave][q] = c[q];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const unsigned long long sum = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    unsigned long long *dst = threadIdx.x == 0 ? &wo->below[0] : threadIdx.x == 1 ? &wo->below[1] : threadIdx.x == 2 ? &wo->targets : &wo->nonfinite;
    if (sum) atomicAdd(dst, sum);
  }
}

// (TrialSource, the data a reduction over labelled trials consumes, and the walk over its pieces: trial_source.hpp)

// One histogram pass over the local data -> hh (host).  No reduction here: see eer_device.  (Declared in trial_source.hpp:
// dcf.hip's level 0 is this pass.)
int eer_pass(plda_handle *h, const TrialSource &src, int shift, int nbits, unsigned prefix, int has_prefix,
             unsigned long long *dhist, unsigned *dbelow, unsigned *dabove, std::vector<unsigned long long> &hh) {
  PLDA_HIP(h, hipMemsetAsync(dhist, 0, 2 * EER_BINS * 8, h->stream));
  PLDA_TRY(for_each_piece(src, [&](const TrialPiece &pc) -> int {
    if (pc.cls < 0) {
      const int64_t strips = ceil_div(pc.Nt, (int64_t)EER_STRIP);
      const int64_t slices = std::max<int64_t>(1, std::min<int64_t>(pc.rows, (256 * 16) / strips));
      const int64_t rows_per_wg = ceil_div(pc.rows, slices);
      eer_hist_strip_kernel<<<(unsigned)(strips * ceil_div(pc.rows, rows_per_wg)), 256, 0, h->stream>>>(
          pc.scores, pc.ld, pc.rows, pc.Nt, pc.espk, src.tspk, rows_per_wg, shift, nbits, prefix, has_prefix, dhist, dbelow, dabove,
          pc.row_step);
    } else {
      const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(pc.Nt, 256), 256 * 16);
      eer_hist_kernel<<<grid, 256, 0, h->stream>>>(pc.scores, pc.Nt, pc.cls, shift, nbits, prefix, has_prefix, dhist, dbelow, dabove);
    }
    return PLDA_OK;
  }));
  PLDA_LAUNCH_CHECK(h);
  hh.resize(2 * EER_BINS);
  PLDA_HIP(h, hipMemcpyAsync(hh.data(), dhist, 2 * EER_BINS * 8, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  return PLDA_OK;
}

bool reduce_block_or_poison(plda_handle *h, const TrialSource &src, const char *who, unsigned long long *H, int *rc) {
  constexpr unsigned long long POISON = 1ull << 48;
  if (src.reduce) {
    if (*rc != PLDA_OK) { std::fill(H, H + 2 * EER_BINS, 0ull); H[0] = POISON; }
    if (src.reduce(src.ctx, H, nullptr, nullptr) != 0 && *rc == PLDA_OK) *rc = fail(h, PLDA_E_INVAL, "%s: the caller's reduction failed", who);
    if (*rc == PLDA_OK && H[0] >= POISON) *rc = fail(h, PLDA_E_NUMERIC, "%s: another rank of the sharded call failed", who);
  }
  return *rc == PLDA_OK;
}

// The definition's last candidate threshold is `s_max + 1e-8`, formed in float64: from |s_max| >= 2^27 on the sum IS s_max, and
// farfrr there counts the trials at s_max as at or above the threshold.
static inline bool last_candidate_collapses(double s) { return s + 1e-8 == s; }

// out: [0] threshold, [1] FAR, [2] FRR, [3] EER = (FAR + FRR) / 2, [4] #targets, [5] #impostors
//
// Non-finite scores (NaN of either sign, +-Inf) are refused with their exact count, before anything else is said about the
// trials; nothing is written to `out`.
//
// Sharded calls (src.reduce): every rank makes the SAME four reduction calls whatever happens locally; a rank that fails
// (HIP error, inconsistent counts) keeps taking part (reduce_block_or_poison).
// window_missed (windowed lists only): set when the crossing key or one of its neighbours is not inside the lists --
// the caller then runs the three passes over the matrix; nothing is written to `out`.
static int eer_device(plda_handle *h, const TrialSource &src, double *out, bool *window_missed = nullptr) {
  typedef unsigned __int128 u128;
  if (window_missed) *window_missed = false;
  unsigned long long *dhist;
  unsigned *dbelow;      // the nearest keys below / above the range: [2]
  PLDA_TRY(carve(h, h->trial_hist, [&](Layout &c) { c.take(dhist, 2 * EER_BINS).take(dbelow, 2).slack(56); }));
  unsigned *dabove = dbelow + 1;
  std::vector<unsigned long long> H;
  // g(k) >= 0  <=>  P(k) * Nn >= (Nn - N(k)) * Np  with P, N = #targets / #impostors with key <= k
  unsigned long long Np = 0, Nn = 0, Pb = 0, Nb = 0;   // totals; counts strictly below the current range
  unsigned prefix = 0;
  const int shifts[3] = {21, 10, 0}, bits[3] = {11, 11, 10};
  unsigned long long cP = 0, cN = 0;   // counts at k1
  long long kmax = -1;                 // the largest key of the data, where pass 0 says it may matter (else unknown)
  std::vector<unsigned long long> last;
  static const unsigned init[2] = {0u, 0xffffffffu};   // (static: the async copy below may read it after this frame)
  int rc = PLDA_OK;                                    // first failure seen by this rank
  for (int pass = 0; pass < 3; ++pass) {
    if (rc == PLDA_OK && pass == 2) {
      const hipError_t e = hipMemcpyAsync(dbelow, init, 8, hipMemcpyHostToDevice, h->stream);
      if (e != hipSuccess) rc = hip_fail(h, e, "hipMemcpyAsync(dbelow)", __FILE__, __LINE__);
    }
    if (rc == PLDA_OK) rc = eer_pass(h, src, shifts[pass], bits[pass], prefix, pass > 0, dhist, dbelow, dabove, H);
    H.resize(2 * EER_BINS);                                  // (a failed pass may not have sized it)
    if (!reduce_block_or_poison(h, src, "eer", H.data(), &rc)) continue;
    const int nb = 1 << bits[pass];
    if (pass == 0) {
      // bins 0..3 and 2044..2047 of the top 11 key bits hold exactly the keys whose exponent is all ones (dcf.hip's level 0
      // counts them the same way); sharded: H is global here, every rank refuses together and keeps making the same calls
      unsigned long long bad = 0;
      for (int b = 0; b < 4; ++b) bad += H[b] + H[EER_BINS + b] + H[2044 + b] + H[EER_BINS + 2044 + b];
      if (bad) { rc = fail(h, PLDA_E_INVAL, "eer: %llu non-finite score(s) among the trials", bad); continue; }
      for (int b = 0; b < nb; ++b) { Nn += H[b]; Np += H[EER_BINS + b]; }
      if (src.windowed) { Np = src.tot_p; Nn = src.tot_n; Pb = src.base_p; Nb = src.base_n; }   // the lists are a window of the data
      if (Np == 0 || Nn == 0) { rc = fail(h, PLDA_E_INVAL, "eer: need at least one target and one impostor trial"); continue; }
      // The largest key, exactly -- wanted only where the last candidate `s_max + 1e-8` can collapse onto s_max (|s_max| >= 2^27,
      // see the end): two more passes down the top bin.  The decision is taken on the global H, so sharded ranks agree on it.
      int top = nb - 1;
      while (top > 0 && !(H[top] | H[EER_BINS + top])) --top;
      if (!src.windowed && (last_candidate_collapses(key_score((unsigned)top << 21)) ||
                            last_candidate_collapses(key_score((((unsigned)top + 1u) << 21) - 1u)))) {
        unsigned kt = (unsigned)top;
        std::vector<unsigned long long> Ht;
        for (int lvl = 1; lvl < 3; ++lvl) {                 // (a failure does not end the loop: the same calls on every rank)
          if (rc == PLDA_OK) rc = eer_pass(h, src, shifts[lvl], bits[lvl], kt, 1, dhist, dbelow, dabove, Ht);
          Ht.resize(2 * EER_BINS);
          if (!reduce_block_or_poison(h, src, "eer", Ht.data(), &rc)) continue;
          int t = (1 << bits[lvl]) - 1;
          while (t > 0 && !(Ht[t] | Ht[EER_BINS + t])) --t;
          kt = (kt << bits[lvl]) | (unsigned)t;
        }
        if (rc != PLDA_OK) continue;
        kmax = (long long)kt;
      }
    }
    int sel = -1;
    unsigned long long P = Pb, N = Nb;
    for (int b = 0; b < nb; ++b) {
      const unsigned long long p2 = P + H[EER_BINS + b], n2 = N + H[b];
      if ((H[b] | H[EER_BINS + b]) && (u128)p2 * Nn >= (u128)(Nn - n2) * Np) { sel = b; cP = H[EER_BINS + b]; cN = H[b]; break; }
      P = p2; N = n2;
    }
    if (sel < 0 && src.windowed && window_missed) { *window_missed = true; return PLDA_OK; }   // the crossing lies above the window
    if (sel < 0) { rc = fail(h, PLDA_E_NUMERIC, "eer: crossing not found (inconsistent counts)"); continue; }
    Pb = P; Nb = N;
    prefix = (prefix << bits[pass]) | (unsigned)sel;
    if (pass == 2) last = H;
  }
  unsigned hb[2] = {0u, 0xffffffffu};
  if (rc == PLDA_OK) {
    hipError_t e = hipMemcpyAsync(hb, dbelow, 8, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) rc = hip_fail(h, e, "copy of the neighbour keys", __FILE__, __LINE__);
  }
  if (src.reduce && src.reduce(src.ctx, nullptr, &hb[0], &hb[1]) != 0 && rc == PLDA_OK)
    rc = fail(h, PLDA_E_INVAL, "eer: the caller's reduction failed");
  if (rc != PLDA_OK) return rc;
  const unsigned k1 = prefix;                       // smallest key with g >= 0; Pb/Nb = counts below k1
  // neighbours of k1 among the data keys
  const int b2 = (int)(k1 & 1023u);
  long long k0 = -1, k2 = -1;
  for (int b = b2 - 1; b >= 0; --b) if (last[b] | last[EER_BINS + b]) { k0 = (long long)((k1 & ~1023u) | (unsigned)b); break; }
  if (k0 < 0 && (Pb + Nb) > 0) k0 = hb[0];
  for (int b = b2 + 1; b < 1024; ++b) if (last[b] | last[EER_BINS + b]) { k2 = (long long)((k1 & ~1023u) | (unsigned)b); break; }
  if (k2 < 0 && (Pb + cP + Nb + cN) < (Np + Nn)) k2 = hb[1];
  if (src.windowed) {
    // the neighbours must have been SEEN in the lists: a predecessor / successor that exists in the data (counts say so)
    // but lies outside the window leaves hb at its initial value
    const bool need0 = (Pb + Nb) > 0, need2 = (Pb + cP + Nb + cN) < (Np + Nn);
    if ((need0 && k0 == 0) || (need2 && k2 == 0xffffffffll)) { if (window_missed) *window_missed = true; return PLDA_OK; }
  }
  // g(k1) = (Pb + cP)/Np - (Nn - Nb - cN)/Nn >= 0 ; g(prev) = Pb/Np - (Nn - Nb)/Nn < 0 (prev = k0, or the start).
  // The choice between the two candidates is made on |FAR - FRR| formed in float64 from the float64 rates,
  // exactly as the definition evaluates it (an exact tie such as 393/400 vs 394/400 around 787/800 must
  // stay a tie and go to the later candidate; extended precision breaks it the other way).
  const double far1 = (double)(Nn - Nb - cN) / (double)Nn, frr1 = (double)(Pb + cP) / (double)Np;
  const double far0 = (double)(Nn - Nb) / (double)Nn, frr0 = (double)Pb / (double)Np;
  // Where the last candidate collapses onto s_max it IS farfrr at s_max: the rates of the candidate before it, which it ties
  // with and, being later, replaces.  That matters in two places: k1 is the largest key (either branch below would answer
  // with a candidate next to it), or k1's successor is and the candidate between them wins.
  double thr, far, frr;
  const double s1 = key_score(k1);
  if (k2 < 0 && last_candidate_collapses(s1)) {
    thr = s1; far = far0; frr = frr0;
  } else if (fabs(far1 - frr1) <= fabs(far0 - frr0)) {     // later candidate wins ties
    const double s = s1;
    thr = k2 >= 0 ? s + ((double)key_score((unsigned)k2) - s) / 2.0 : s + 1e-8;
    far = (double)(Nn - Nb - cN) / (double)Nn; frr = (double)(Pb + cP) / (double)Np;
    if (k2 >= 0 && last_candidate_collapses((double)key_score((unsigned)k2))) {
      // (a window that reaches the top of the data does not know which of its keys is the largest: the three passes do)
      if (src.windowed && src.none_above) { if (window_missed) *window_missed = true; return PLDA_OK; }
      if (!src.windowed && k2 == kmax) thr = (double)key_score((unsigned)k2);
    }
  } else {
    thr = k0 >= 0 ? (double)key_score((unsigned)k0) + (s1 - (double)key_score((unsigned)k0)) / 2.0 : s1;
    far = (double)(Nn - Nb) / (double)Nn; frr = (double)Pb / (double)Np;
  }
  out[0] = thr; out[1] = far; out[2] = frr; out[3] = 0.5 * (far + frr); out[4] = (double)Np; out[5] = (double)Nn;
  return PLDA_OK;
}

// ---- the single-pass form (see the header) ----
constexpr int64_t EER_PILOT_STEP = 32;
// Returns PLDA_OK with *done = true when `out` holds the result; *done = false: run the three passes.
// (full: the whole matrix -- in memory, or as slabs)
static int eer_matrix_windowed(plda_handle *h, const TrialSource &full, double *out, bool *done) {
  typedef unsigned __int128 u128;
  *done = false;
  const int64_t M = full.M, Nt = full.Nt;
  TraceScope ts(h, "eer.pilot");
  unsigned long long *dhist;
  unsigned *dbelow;      // the nearest keys below / above the range: [2]
  EerWindowOut *dwo;     // (a 64-byte line of its own)
  PLDA_TRY(carve(h, h->trial_hist, [&](Layout &c) { c.take(dhist, 2 * EER_BINS).take(dbelow, 2).take(dwo, 1, 64); }));
  unsigned *dabove = dbelow + 1;
  TrialSource smp = TrialSource::matrix(full.scores, full.ld, M, Nt, full.espk, full.tspk).every(EER_PILOT_STEP);
  int64_t pilot_step = EER_PILOT_STEP;
  if (full.kind == TrialSource::SLABS) {
    // the sample is produced (a small GEMM of its own) and must fit the slab buffer
    pilot_step = std::max<int64_t>(EER_PILOT_STEP, ceil_div(M, full.sl->slab_rows));
    const float *sc = nullptr; const int64_t *se = nullptr; int64_t sld = 0, srows = 0;
    PLDA_TRY(full.sl->sample(full.sl->ctx, pilot_step, &sc, &sld, &se, &srows));
    smp = TrialSource::matrix(sc, sld, srows, Nt, se, full.tspk);
  }
  // pilot, pass 0 on the sample: per coarse bin (top 11 key bits) the sample's g = FRR - FAR; the band |g| < delta of five
  // standard errors around the sample's crossing starts in coarse bin ca and ends in cb (often the same); one pass over
  // the sample per end then places the window's ends on sub-bins (22 key bits)
  std::vector<unsigned long long> H0, H1;
  PLDA_TRY(eer_pass(h, smp, 21, 11, 0, 0, dhist, dbelow, dabove, H0));
  unsigned long long Np = 0, Nn = 0;
  for (int b = 0; b < EER_BINS; ++b) { Nn += H0[b]; Np += H0[EER_BINS + b]; }
  if (Np < 2000 || Nn < 2000) return PLDA_OK;                       // too few targets in the sample to bracket anything
  auto g_after = [&](unsigned long long p, unsigned long long n) { return (double)p / (double)Np - (double)(Nn - n) / (double)Nn; };
  double delta = 0.0;
  {
    unsigned long long P = 0, N = 0;
    int c0 = -1;
    for (int b = 0; b < EER_BINS; ++b) {
      const unsigned long long p2 = P + H0[EER_BINS + b], n2 = N + H0[b];
      if ((H0[b] | H0[EER_BINS + b]) && (u128)p2 * Nn >= (u128)(Nn - n2) * Np) { c0 = b; break; }
      P = p2; N = n2;
    }
    if (c0 < 0) return PLDA_OK;
    const double pe = std::min(0.5, std::max((double)P / (double)Np, 10.0 / (double)Np));     // ~ the sample's FRR at the crossing
    delta = 5.0 * (std::sqrt(pe * (1.0 - pe) / (double)Np) + std::sqrt(pe * (1.0 - pe) / (double)Nn)) + 2.0 / (double)Np;
  }
  int ca = -1, cb = -1;
  unsigned long long Pa = 0, Na = 0, Pc = 0, Nc = 0;                 // sample counts below coarse bins ca, cb
  {
    unsigned long long P = 0, N = 0;
    for (int b = 0; b < EER_BINS; ++b) {
      const unsigned long long p2 = P + H0[EER_BINS + b], n2 = N + H0[b];
      const double g = g_after(p2, n2);
      if (ca < 0 && g > -delta) { ca = b; Pa = P; Na = N; }
      if (g >= delta) { cb = b; Pc = P; Nc = N; break; }
      P = p2; N = n2;
    }
  }
  if (ca < 0 || cb < 0) return PLDA_OK;
  int blo = 0, bhi = EER_BINS - 1;
  unsigned long long win_lo = Pa + Na, win_hi = 0;                   // sample trials below the window's ends
  PLDA_TRY(eer_pass(h, smp, 10, 11, (unsigned)ca, 1, dhist, dbelow, dabove, H1));
  {
    unsigned long long p = Pa, n = Na;
    for (int b = 0; b < EER_BINS; ++b) {
      const unsigned long long p2 = p + H1[EER_BINS + b], n2 = n + H1[b];
      if (g_after(p2, n2) > -delta) { blo = b; break; }
      p = p2; n = n2;
    }
    blo = std::max(blo - 1, 0);                                      // one sub-bin of margin
    for (int b = 0; b < blo; ++b) win_lo += H1[b] + H1[EER_BINS + b];
  }
  if (cb != ca) PLDA_TRY(eer_pass(h, smp, 10, 11, (unsigned)cb, 1, dhist, dbelow, dabove, H1));
  {
    unsigned long long p = Pc, n = Nc;
    for (int b = 0; b < EER_BINS; ++b) {
      p += H1[EER_BINS + b]; n += H1[b];
      if (g_after(p, n) >= delta) { bhi = b; break; }
    }
    bhi = std::min(bhi + 1, EER_BINS - 1);
    win_hi = Pc + Nc;
    for (int b = 0; b <= bhi; ++b) win_hi += H1[b] + H1[EER_BINS + b];
  }
  const unsigned klo = ((unsigned)ca << 21) | ((unsigned)blo << 10);
  const unsigned long long khi64 = ((unsigned long long)cb << 21) | ((unsigned long long)(bhi + 1) << 10);
  if (khi64 > 0xffffffffull || khi64 <= klo) return PLDA_OK;
  const unsigned khi = (unsigned)khi64;
  const unsigned long long win = win_hi > win_lo ? win_hi - win_lo : 0;
  // the lists: the sample's in-window count scaled up, with room to spare; too wide a window is not worth a list
  const unsigned long long cap = (unsigned long long)((double)win * (double)pilot_step * 2.0) + (1ull << 20);
  if (cap > (unsigned long long)M * (unsigned long long)Nt / 8) return PLDA_OK;
  PLDA_HIP(h, h->eer_list[0].reserve((size_t)cap * 4));
  PLDA_HIP(h, h->eer_list[1].reserve((size_t)cap * 4));
  ts.next("eer.window_pass", (double)M * (double)Nt * 4.0, 2);
  PLDA_HIP(h, hipMemsetAsync(dwo, 0, sizeof(EerWindowOut), h->stream));
  PLDA_TRY(for_each_piece(full, [&](const TrialPiece &pc) -> int {
    const int64_t strips = ceil_div(Nt, (int64_t)EER_STRIP);
    const int64_t slices = std::max<int64_t>(1, std::min<int64_t>(pc.rows, (256 * 16) / strips));
    const int64_t rows_per_wg = ceil_div(pc.rows, slices);
    eer_window_strip_kernel<<<(unsigned)(strips * ceil_div(pc.rows, rows_per_wg)), 256, 0, h->stream>>>(
        pc.scores, pc.ld, pc.rows, Nt, pc.espk, full.tspk, rows_per_wg, key_score(klo), key_score(khi), dwo, h->eer_list[0].as<float>(), h->eer_list[1].as<float>(), cap);
    PLDA_LAUNCH_CHECK(h);
    return PLDA_OK;
  }));
  EerWindowOut wo;
  PLDA_HIP(h, hipMemcpyAsync(&wo, dwo, sizeof(wo), hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  ts.next("eer.finish_on_window");
  if (wo.nonfinite) return fail(h, PLDA_E_INVAL, "eer: %llu non-finite score(s) among the trials", wo.nonfinite);
  if (wo.cursor[0] > cap || wo.cursor[1] > cap) return PLDA_OK;     // a list overflowed
  // every finite trial is below, inside or above the window
  const unsigned long long seen = wo.below[0] + wo.below[1] + wo.cursor[0] + wo.cursor[1], total = (unsigned long long)M * (unsigned long long)Nt;
  if (seen > total) return PLDA_OK;
  const unsigned long long TP = wo.targets, TN = (unsigned long long)M * (unsigned long long)Nt - wo.targets;
  if (TP == 0 || TN == 0) return fail(h, PLDA_E_INVAL, "eer: need at least one target and one impostor trial");
  // exact g at the window's ends: below it FRR - FAR must still be negative, at its end non-negative
  if ((u128)wo.below[1] * TN >= (u128)(TN - wo.below[0]) * TP) return PLDA_OK;
  if ((u128)(wo.below[1] + wo.cursor[1]) * TN < (u128)(TN - wo.below[0] - wo.cursor[0]) * TP) return PLDA_OK;
  if (wo.cursor[0] + wo.cursor[1] == 0) return PLDA_OK;
  const TrialSource lst = TrialSource::lists(h->eer_list[1].as<float>(), (int64_t)wo.cursor[1], h->eer_list[0].as<float>(), (int64_t)wo.cursor[0])
                              .window_of(wo.below[1], wo.below[0], TP, TN, seen == total);
  bool missed = false;
  PLDA_TRY(eer_device(h, lst, out, &missed));
  *done = !missed;
  return PLDA_OK;
}

// the single-pass form where it applies (one process, large enough), else -- or should its window miss -- the three passes
static int eer_source_device(plda_handle *h, const TrialSource &src, double *out, const char *three_passes_scope) {
  const int64_t M = src.M, Nt = src.Nt;
  h->eer_last_passes = 3;
  if (!src.reduce && h->eer_variant != 1 && (h->eer_variant == 2 || (double)M * (double)Nt >= 2.5e8) && M >= 4 * EER_PILOT_STEP) {
    bool done = false;
    PLDA_TRY(eer_matrix_windowed(h, src, out, &done));
    if (done) { h->eer_last_passes = 1; return PLDA_OK; }
  }
  TraceScope ts(h, three_passes_scope, 3.0 * (double)M * (double)Nt * 4.0, 2);
  return eer_device(h, src, out);
}

int eer_matrix_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *despk,
                      const int64_t *dtspk, double *out, TrialReduce reduce, void *ctx) {
  // a rank of a sharded call may own no row at all (M == 0): it still takes part in the reductions
  if (!out || Nt <= 0 || ld < Nt || M < 0 || (M == 0 && !reduce) || (M > 0 && (!dscores || !despk || !dtspk)))
    return fail(h, PLDA_E_INVAL, "eer: bad argument");
  return eer_source_device(h, TrialSource::matrix(dscores, ld, M, Nt, despk, dtspk).reduced_by(reduce, ctx), out, "eer.three_passes");
}

// EER of a trials matrix that is never held (plda_score_eer_dev; operand_slabs.hip): the pilot's sample is a GEMM of every
// step-th enrol row, every slab is scored and consumed by the window pass; the three-pass form, should the window miss,
// re-scores the slabs per pass.
int score_eer_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV, int64_t Nt,
                     const double *dzmean, const double *dzstd, const int64_t *despk, const int64_t *dtspk, double *out) {
  OperandSlabs os;
  TrialSource src;
  PLDA_TRY(operand_source(h, "score_eer", dU, dn, n_uniform, M, dV, Nt, dzmean, dzstd, despk, dtspk, out, &os, &src));
  return eer_source_device(h, src, out, "eer.three_passes (slabs re-scored per pass)");
}

// ------------------------------------------------------------------------------------
// DET points (round 5): the numbers behind scoring/eer.py:34-62's plot -- bob.measure.plot.det(negatives, positives, 100)
// evaluates farfrr at n thresholds spread evenly from the smallest to the largest score (bob absent: definition
// restated in oracle/plda_oracle_np.py:det, PARITY UNPINNED; the plotting itself stays out of scope).  Two passes over
// the scores: the extreme keys, then per class a histogram of k(s) = #{i : t_i <= s} -- a guess from the division,
// corrected against the fp64 threshold table the host accumulated exactly as the definition does -- from which
// FAR_i = #{neg : k >= i + 1} / Nn and FRR_i = #{pos : k <= i} / Np follow as suffix / prefix sums.  n <= 2047.
// ------------------------------------------------------------------------------------
constexpr int DET_MAX = 2047;
__global__ __launch_bounds__(256) void det_minmax_kernel(const float *__restrict__ scores, int64_t ld, int64_t M, int64_t Nt,
                                                         unsigned *__restrict__ mm /*[0] min key, [1] max key, [2..3] a 64-bit count of non-finite scores*/) {
  unsigned lo = 0xffffffffu, hi = 0u;
  unsigned long long nf = 0;
  const int64_t total = M * Nt;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const float sc = scores[(idx / Nt) * ld + idx % Nt];
    const unsigned k = score_key(sc);
    lo = k < lo ? k : lo; hi = k > hi ? k : hi;
    nf += (__float_as_uint(sc) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;      // NaN of either sign, +-Inf
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned a = __shfl_xor(lo, o), b = __shfl_xor(hi, o);
    lo = a < lo ? a : lo; hi = b > hi ? b : hi;
    nf += __shfl_xor(nf, o);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(mm, lo); atomicMax(mm + 1, hi);
    if (nf) atomicAdd(reinterpret_cast<unsigned long long *>(mm + 2), nf);
  }
}
// cls < 0: the class of trial (i, j) is espk[i] == tspk[j]; else every score is of class cls (the two-list form, M = 1)
__global__ __launch_bounds__(256) void det_hist_kernel(const float *__restrict__ scores, int64_t ld, int64_t M, int64_t Nt,
                                                       const int64_t *__restrict__ espk, const int64_t *__restrict__ tspk, int cls,
                                                       const double *__restrict__ thr, int n, double lo, double inv_step,
                                                       unsigned long long *__restrict__ hist /*[2][DET_MAX + 1]*/) {
  __shared__ unsigned lh[2][DET_MAX + 1];
  __shared__ double ts[DET_MAX + 1];
  for (int i = threadIdx.x; i < 2 * (DET_MAX + 1); i += 256) (&lh[0][0])[i] = 0;
  for (int i = threadIdx.x; i < n; i += 256) ts[i] = thr[i];
  __syncthreads();
  const int64_t total = M * Nt;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t r = idx / Nt, c = idx % Nt;
    const double sc = (double)scores[r * ld + c];
    int k = (int)((sc - lo) * inv_step) + 1;            // guess of #{i : t_i <= s}
    k = k < 0 ? 0 : (k > n ? n : k);
    while (k > 0 && ts[k - 1] > sc) --k;                // t_{k-1} <= s must hold
    while (k < n && ts[k] <= sc) ++k;                   // and t_k > s
    const int cl = cls >= 0 ? cls : (espk[r] == tspk[c] ? 1 : 0);
    atomicAdd(&lh[cl][k], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * (DET_MAX + 1); i += 256) {
    const unsigned v = (&lh[0][0])[i];
    if (v) atomicAdd(hist + i, (unsigned long long)v);
  }
}

static int det_device(plda_handle *h, const TrialSource &src, int npoints, double *far, double *frr, double *thresholds) {
  if (npoints < 2 || npoints > DET_MAX) return fail(h, PLDA_E_INVAL, "det: 2 <= n_points <= %d", DET_MAX);
  const size_t hb = (size_t)2 * (DET_MAX + 1) * 8;
  unsigned long long *dhist;
  unsigned *dmm;         // the smallest and the largest key and the count of non-finite scores, in a 64-byte line
  double *dthr;
  PLDA_TRY(carve(h, h->trial_hist, [&](Layout &c) { c.take(dhist, 2 * (DET_MAX + 1)).take(dmm, 16).take(dthr, DET_MAX).slack(64); }));
  static const unsigned init[4] = {0xffffffffu, 0u, 0u, 0u};
  PLDA_HIP(h, hipMemcpyAsync(dmm, init, 16, hipMemcpyHostToDevice, h->stream));
  PLDA_TRY(for_each_piece(src, [&](const TrialPiece &pc) -> int {
    det_minmax_kernel<<<(unsigned)std::min<int64_t>(ceil_div(pc.rows * pc.Nt, 256), 256 * 32), 256, 0, h->stream>>>(pc.scores, pc.ld, pc.rows, pc.Nt, dmm);
    return PLDA_OK;
  }));
  PLDA_LAUNCH_CHECK(h);
  unsigned mm[4];
  PLDA_HIP(h, hipMemcpyAsync(mm, dmm, 16, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  // one Inf or NaN would make the step, and every threshold after the first, Inf or NaN: refused, like the EER's
  const unsigned long long bad = (unsigned long long)mm[2] | ((unsigned long long)mm[3] << 32);
  if (bad) return fail(h, PLDA_E_INVAL, "det: %llu non-finite score(s) among the trials", bad);
  if (mm[0] > mm[1]) return fail(h, PLDA_E_INVAL, "det: no scores");
  // the thresholds exactly as the definition accumulates them (float64 running sum)
  const double lo = (double)key_score(mm[0]), hi = (double)key_score(mm[1]);
  const double step = (hi - lo) / ((double)npoints - 1.0);
  std::vector<double> thr((size_t)npoints);
  double t = lo;
  for (int i = 0; i < npoints; ++i) { thr[(size_t)i] = t; t += step; }
  PLDA_HIP(h, hipMemcpyAsync(dthr, thr.data(), (size_t)npoints * 8, hipMemcpyHostToDevice, h->stream));
  PLDA_HIP(h, hipMemsetAsync(dhist, 0, hb, h->stream));
  PLDA_TRY(for_each_piece(src, [&](const TrialPiece &pc) -> int {
    det_hist_kernel<<<(unsigned)std::min<int64_t>(ceil_div(pc.rows * pc.Nt, 256), 256 * 8), 256, 0, h->stream>>>(
        pc.scores, pc.ld, pc.rows, pc.Nt, pc.espk, src.tspk, pc.cls, dthr, npoints, lo, step > 0.0 ? 1.0 / step : 0.0, dhist);
    return PLDA_OK;
  }));
  PLDA_LAUNCH_CHECK(h);
  std::vector<unsigned long long> H((size_t)2 * (DET_MAX + 1));
  PLDA_HIP(h, hipMemcpyAsync(H.data(), dhist, hb, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  unsigned long long Nn = 0, Np = 0;
  for (int k = 0; k <= npoints; ++k) { Nn += H[(size_t)k]; Np += H[(size_t)(DET_MAX + 1) + k]; }
  if (Nn == 0 || Np == 0) return fail(h, PLDA_E_INVAL, "det: need at least one target and one impostor score");
  // k(s) = #{i : t_i <= s}:  s >= t_i  <=>  k >= i + 1;   s < t_i  <=>  k <= i
  unsigned long long below_p = 0, ge_n = Nn;
  for (int i = 0; i < npoints; ++i) {
    ge_n -= H[(size_t)i];                                   // impostors with k == i are below t_i
    below_p += H[(size_t)(DET_MAX + 1) + i];                // targets with k <= i are below t_i
    far[i] = (double)ge_n / (double)Nn;
    frr[i] = (double)below_p / (double)Np;
    if (thresholds) thresholds[i] = thr[(size_t)i];
  }
  return PLDA_OK;
}

int det_matrix_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *despk, const int64_t *dtspk,
                      int npoints, double *far, double *frr, double *thresholds) {
  if (!dscores || !despk || !dtspk || !far || !frr || M <= 0 || Nt <= 0 || ld < Nt) return fail(h, PLDA_E_INVAL, "det: bad argument");
  return det_device(h, TrialSource::matrix(dscores, ld, M, Nt, despk, dtspk), npoints, far, frr, thresholds);
}
int det_lists_device(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, int npoints, double *far, double *frr,
                     double *thresholds) {
  if (!dpos || !dneg || !far || !frr || np <= 0 || nn <= 0) return fail(h, PLDA_E_INVAL, "det: need at least one target and one impostor score");
  return det_device(h, TrialSource::lists(dpos, np, dneg, nn), npoints, far, frr, thresholds);
}

int eer_lists_device(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, double *out) {
  if (!dpos || !dneg || !out || np <= 0 || nn <= 0) return fail(h, PLDA_E_INVAL, "eer: need at least one target and one impostor score");
  return eer_device(h, TrialSource::lists(dpos, np, dneg, nn), out);
}

}  // namespace plda
