// plda_amd/csrc/fusion.hip -- linear fusion of K systems' scores by prior-weighted logistic regression on the GPU
// (include/plda_hip.h, "multi-system score fusion"; the fusion half of BOSARIS / FoCal next to calib.hip's calibration half;
// the reference stops at per-system score files, so the definition is the project's own and is pinned by tests/fusion_model.py).
//
// One FUSION PASS at (a[K], c, theta) reads the K fp32 scores of every trial once, in lock-step, and returns one
// plda_fusion_record: per class L, G[K+1] and the packed upper triangle H[(K+1)(K+2)/2] of the feature vector
// phi = (1, s_0 .. s_{K-1}) at the chain value y = fma(a_{K-1}, s_{K-1}, ... fma(a_0, s_0, c)), the exact counts, the fp64
// extremes of y per class and the fp32 extremes of every system.  The Newton fit is host arithmetic on records
// (fusion_newton, a pure function), the apply is the same chain rounded once to fp32 (fusion_map_kernel).
//
// QUALITY-AWARE CALIBRATION (K25; include/plda_hip.h, "quality-aware calibration") adds Q SIDES to the K matrices.  A side is
// one fp32 operation on a per-enrol-row and a per-test-column number (duration, embedding norm, cohort mean ...); its [M, Nt]
// values never exist in memory -- fusion_pass_strip_kernel<K, true> and fusion_side_map_kernel<K> form them in registers; the
// pass hands the assembled fp32 feature array (s_0 .. s_{K-1}, q_0 .. q_{Q-1}) to the same account, store, grid and visiting
// order.  A side pass is therefore bit-identical to a matrix pass over K + Q matrices in which the sides have been
// materialised, and the Newton fit, the record and the refusals are used as they are.  Below, K counts every FEATURE where
// sides are present.
//
// Kernels, all instantiated on K = 1 .. 8 so that every accumulator index is a compile-time constant (a runtime-indexed
// per-thread array would live in scratch); with sides, the number of matrices among the K features is wave-uniform at run
// time (one uniform branch per unrolled feature slot: 8 instantiations instead of 36 on (K, Q)):
//   fusion_pass_strip_kernel<K, SIDES>  walks the K matrices as calib_pass_strip_kernel walks one: a workgroup owns 1024 columns, 4
//       per thread with their test speaker ids in registers, and a slice of the rows.  The K base pointers, pitches and
//       weights travel by value in one kernel-argument struct; 16-byte or scalar loads are chosen PER SYSTEM (each has its
//       own base alignment and pitch).  Rows in flight per thread: 4 (K <= 2), 2 (K <= 4), 1 (K > 4) -- 4 K floats each.
//       Per element, all fp64: the chain, exp(-|y|), log1p, one divide, then NE = 1 + (K+1) + (K+1)(K+2)/2 fused
//       multiply-adds into the thread's NON-TARGET accumulators with multipliers that a select has zeroed for a target
//       (no branch).  A second per-thread set for the targets would double the 2 NE registers (110 at K = 8) for a 2e-4
//       share of a large matrix; instead a wave that holds a target (wave-uniform ballot, as K10) accounts its targets
//       COOPERATIVELY: the set bits of the ballot are visited in ascending lane order, that lane's (s_0 .. s_{K-1}, g, w, L)
//       are broadcast by readlane, and lane e < NE adds entry e's term to the ONE target accumulator it owns.  The order
//       is a function of the data layout alone, so the sums stay deterministic.
//   fusion_pass_list_kernel<K>   K parallel flat arrays of one fixed class: everything goes through the per-thread set.
//   fusion_reduce_kernel         one block of 1024 threads adds the per-block partial records in a fixed order.
//   fusion_map_kernel<K>         out = (float)chain with c = b; in place over one of the inputs allowed.
//   fusion_side_map_kernel<K>    the same over matrices and sides, a side's four test values held in registers.
// The operand form (system 0 produced slab by slab, fusion_pass) launches the same pass kernel per slab with the enrol vectors
// offset to the slab's first row.
// A wave reduces its NE sums by DPP (wave_sum_f64), the four waves of a block are added as (w0 + w1) + (w2 + w3), the block
// writes ONE partial record into handle scratch (h->fusion_part).  No floating-point atomics and no integer ones: a call's
// record is bit-identical from run to run.  The grid is a function of the shape alone (the same for every K; not tunable).
//
// Accuracy of the additions (the header states it): a thread adds its 4 * rows_per_wg non-target terms one after the other,
// a wave its targets one after the other; everything above that is a tree.
//
// Resources (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage with this file's flags, plda_amd/build.py):
// the table at fusion_pass_strip_kernel below -- no scratch and no spill in any instantiation, the K = 8 labelled pass in 244
// registers (two waves per SIMD).  Speed: scripts/fusion_bench.py writes profiles/fusion_*.json,
// scripts/fusion_side_bench.py profiles/fusion_side_*.json (K25).
#include "trial_source.hpp"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <type_traits>

namespace plda {

typedef float f32x4f __attribute__((ext_vector_type(4)));
constexpr int FUSION_STRIP = 1024;           // columns per workgroup (4 per thread), as CALIB_STRIP
constexpr int FUSION_MAX_BLOCKS = 256 * 16;
constexpr int FUSION_KMAX = PLDA_FUSION_MAX_SYSTEMS;
constexpr int FUSION_SLOTS = 1 + (FUSION_KMAX + 1) + (FUSION_KMAX + 1) * (FUSION_KMAX + 2) / 2;   // 55 doubles per class
static_assert(sizeof(plda_fusion_sums) == FUSION_SLOTS * sizeof(double), "plda_fusion_sums is [L, G[9], H[45]]");
static_assert(sizeof(plda_fusion_record) == 1024, "plda_fusion_record layout");

// the K systems of a call, by value in the kernel arguments
struct FusionArgs {
  const float *s[FUSION_KMAX];
  int64_t ld[FUSION_KMAX];
  double a[FUSION_KMAX];
  double c, theta;
};

typedef const FusionArgs __attribute__((address_space(4))) *FusionArgsPtr;   // the same struct where the kernel arguments live

__host__ __device__ constexpr int fusion_entries(int K) { return 1 + (K + 1) + (K + 1) * (K + 2) / 2; }
// entry e of the K-compact order [L, G[0 .. K], H[0 .. (K+1)(K+2)/2)] -> its slot in plda_fusion_sums (K-independent)
__host__ __device__ constexpr int fusion_slot(int K, int e) { return e <= K + 1 ? e : (1 + FUSION_KMAX + 1) + (e - (K + 2)); }

template <int K> struct FusionAcc {
  static constexpr int NE = fusion_entries(K);
  double n[NE];                              // the thread's own sums (non-targets of a matrix; the fixed class of a list)
  double t = 0.0;                            // targets of a matrix: lane e of the wave owns entry e
  double ylo_n = INFINITY, yhi_n = -INFINITY, ylo_t = INFINITY, yhi_t = -INFINITY;
  float slo[K], shi[K];
  unsigned np = 0, nn = 0, miss = 0, fa = 0, bad = 0;   // per thread: at most 4 * rows_per_wg trials (checked by the host)
  __device__ __forceinline__ FusionAcc() {
#pragma unroll
    for (int e = 0; e < NE; ++e) n[e] = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) { slo[k] = INFINITY; shi[k] = -INFINITY; }
  }
};

// which term lane `lane` owns in the cooperative target sum: the coefficient (0 = L, 1 = g, 2 = w, 3 = none) and the two phi
// indices.  Recomputed where it is needed (the rare target path) instead of held in three registers through the whole walk.
template <int K> __device__ __forceinline__ void fusion_lane_role(int lane, int &csel, int &pi, int &pj) {
  csel = 3; pi = 0; pj = 0;
  if (lane == 0) csel = 0;
  else if (lane <= K + 1) { csel = 1; pi = lane - 1; }
  else if (lane < fusion_entries(K)) {
    csel = 2;
    const int t = lane - (K + 2);
    int j = 0;
#pragma unroll
    for (int q = 1; q <= K; ++q) j += (q * (q + 1) / 2 <= t) ? 1 : 0;
    pj = j; pi = t - j * (j + 1) / 2;
  }
}

__device__ __forceinline__ float readlane_f32(float x, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)); }

// CLS: -1 = labelled by `tgt` (matrix), 0 / 1 = every trial of that class (lists).  The labelled form must be entered by EVERY
// lane of the wave, the lanes beyond the last column with valid = false (their sf are zeros and count for nothing): the
// cooperative target sum below needs lane e alive to own entry e, whichever lanes hold trials.
template <int K, int CLS>
__device__ __forceinline__ void fusion_account(FusionAcc<K> &A, const float (&sf)[K], bool valid, bool tgt_in, const FusionArgs &P) {
  const bool tgt = CLS < 0 ? (valid && tgt_in) : CLS != 0;
  double s[K];
  double y = P.c;
  bool nonfinite = false;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    s[k] = (double)sf[k];
    y = fma(P.a[k], s[k], y);
    nonfinite |= (__float_as_uint(sf[k]) & 0x7f800000u) == 0x7f800000u;
    A.slo[k] = valid ? fminf(A.slo[k], sf[k]) : A.slo[k];
    A.shi[k] = valid ? fmaxf(A.shi[k], sf[k]) : A.shi[k];
  }
  const double e = exp(-fabs(y));
  const double l = log1p(e);
  const double r = 1.0 / (1.0 + e);
  const double q = e * r;                    // sigmoid(-|y|)
  const double w = q * r;                    // p (1 - p)
  const bool pos = y >= 0.0;
  const double Ln = fmax(y, 0.0) + l, Lt = fmax(-y, 0.0) + l;   // softplus(y), softplus(-y)
  const double gn = pos ? r : q, gt = pos ? q : r;               // p, 1 - p
  {
    // own sums: a target of a matrix contributes zeros
    const bool mine = CLS >= 0 || (valid && !tgt);
    const double cL = mine ? (CLS == 1 ? Lt : Ln) : 0.0, cg = mine ? (CLS == 1 ? gt : gn) : 0.0, cw = mine ? w : 0.0;
    A.n[0] += cL;
    A.n[1] += cg;
#pragma unroll
    for (int k = 0; k < K; ++k) A.n[2 + k] = fma(cg, s[k], A.n[2 + k]);
    A.n[K + 2] += cw;                        // H[t(0, 0)]
#pragma unroll
    for (int i = 0; i <= K; ++i) {           // row i of the triangle: one w phi_i live at a time
      const double wphi = i == 0 ? cw : cw * s[i > 0 ? i - 1 : 0];
#pragma unroll
      for (int j = (i > 1 ? i : 1); j <= K; ++j) A.n[K + 2 + j * (j + 1) / 2 + i] = fma(wphi, s[j - 1], A.n[K + 2 + j * (j + 1) / 2 + i]);
    }
    A.ylo_n = mine ? fmin(A.ylo_n, y) : A.ylo_n;
    A.yhi_n = mine ? fmax(A.yhi_n, y) : A.yhi_n;
  }
  if (CLS < 0) {
    unsigned long long m = __builtin_amdgcn_ballot_w64(tgt);
    if (m) {                                 // wave-uniform: most waves of a large matrix hold no target
      A.ylo_t = tgt ? fmin(A.ylo_t, y) : A.ylo_t;
      A.yhi_t = tgt ? fmax(A.yhi_t, y) : A.yhi_t;
      int csel, pi, pj;
      fusion_lane_role<K>(threadIdx.x & 63, csel, pi, pj);
      do {                                   // ascending lane order: a fixed order of additions
        const int src = __builtin_ctzll(m);
        m &= m - 1;
        const double bL = readlane_f64(Lt, src), bg = readlane_f64(gt, src), bw = readlane_f64(w, src);
        const double coef = csel == 0 ? bL : csel == 1 ? bg : csel == 2 ? bw : 0.0;
        double fi = 1.0, fj = 1.0;           // phi_0
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const double bs = (double)readlane_f32(sf[k], src);
          fi = pi == k + 1 ? bs : fi;
          fj = pj == k + 1 ? bs : fj;
        }
        A.t += (coef * fi) * fj;
      } while (m);
    }
  }
  A.np += tgt ? 1u : 0u;
  A.nn += (valid && !tgt) ? 1u : 0u;
  A.miss += (tgt && y < P.theta) ? 1u : 0u;
  A.fa += (valid && !tgt && y >= P.theta) ? 1u : 0u;
  A.bad += (valid && nonfinite) ? 1u : 0u;
}

// block (256 threads) -> one record, every addition in a fixed order.  cn: the class of the threads' own sums (0 for a
// matrix and a non-target list, 1 for a target list); the cooperative target sums go to the other class.
template <int K>
__device__ __forceinline__ void fusion_block_store(const FusionAcc<K> &A, int cn, plda_fusion_record *__restrict__ dst) {
  constexpr int NE = FusionAcc<K>::NE;
  __shared__ double red[4][2][FUSION_SLOTS];
  __shared__ double red_y[4][4];
  __shared__ unsigned long long red_c[4][5];
  __shared__ float red_f[4][2 * K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < 4 * 2 * FUSION_SLOTS; i += 256) (&red[0][0][0])[i] = 0.0;
  __syncthreads();
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const double v = wave_sum_f64(A.n[e]);
    if (lane == 0) red[wave][cn][fusion_slot(K, e)] = v;
  }
  if (lane < NE) red[wave][1 - cn][fusion_slot(K, lane)] = A.t;
  double ylo_n = A.ylo_n, yhi_n = A.yhi_n, ylo_t = A.ylo_t, yhi_t = A.yhi_t;
  unsigned long long cnt[5] = {A.np, A.nn, A.miss, A.fa, A.bad};
  float slo[K], shi[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { slo[k] = A.slo[k]; shi[k] = A.shi[k]; }
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 5; ++k) cnt[k] += __shfl_xor(cnt[k], o);
    ylo_n = fmin(ylo_n, __shfl_xor(ylo_n, o)); yhi_n = fmax(yhi_n, __shfl_xor(yhi_n, o));
    ylo_t = fmin(ylo_t, __shfl_xor(ylo_t, o)); yhi_t = fmax(yhi_t, __shfl_xor(yhi_t, o));
#pragma unroll
    for (int k = 0; k < K; ++k) { slo[k] = fminf(slo[k], __shfl_xor(slo[k], o)); shi[k] = fmaxf(shi[k], __shfl_xor(shi[k], o)); }
  }
  if (lane == 0) {
    red_y[wave][0] = ylo_n; red_y[wave][1] = yhi_n; red_y[wave][2] = ylo_t; red_y[wave][3] = yhi_t;
#pragma unroll
    for (int k = 0; k < 5; ++k) red_c[wave][k] = cnt[k];
#pragma unroll
    for (int k = 0; k < K; ++k) { red_f[wave][k] = slo[k]; red_f[wave][K + k] = shi[k]; }
  }
  __syncthreads();
  double *out_sums = reinterpret_cast<double *>(&dst->sum[0]);
  for (int i = threadIdx.x; i < 2 * FUSION_SLOTS; i += 256) {
    const int cl = i / FUSION_SLOTS, sl = i % FUSION_SLOTS;
    out_sums[i] = (red[0][cl][sl] + red[1][cl][sl]) + (red[2][cl][sl] + red[3][cl][sl]);
  }
  if (threadIdx.x == 0) {
    dst->ymin[cn] = fmin(fmin(red_y[0][0], red_y[1][0]), fmin(red_y[2][0], red_y[3][0]));
    dst->ymax[cn] = fmax(fmax(red_y[0][1], red_y[1][1]), fmax(red_y[2][1], red_y[3][1]));
    dst->ymin[1 - cn] = fmin(fmin(red_y[0][2], red_y[1][2]), fmin(red_y[2][2], red_y[3][2]));
    dst->ymax[1 - cn] = fmax(fmax(red_y[0][3], red_y[1][3]), fmax(red_y[2][3], red_y[3][3]));
    dst->np = red_c[0][0] + red_c[1][0] + red_c[2][0] + red_c[3][0];
    dst->nn = red_c[0][1] + red_c[1][1] + red_c[2][1] + red_c[3][1];
    dst->miss = red_c[0][2] + red_c[1][2] + red_c[2][2] + red_c[3][2];
    dst->fa = red_c[0][3] + red_c[1][3] + red_c[2][3] + red_c[3][3];
    dst->nonfinite = red_c[0][4] + red_c[1][4] + red_c[2][4] + red_c[3][4];
    for (int k = 0; k < FUSION_KMAX; ++k) {
      dst->smin[k] = k < K ? fminf(fminf(red_f[0][k], red_f[1][k]), fminf(red_f[2][k], red_f[3][k])) : 0.f;
      dst->smax[k] = k < K ? fmaxf(fmaxf(red_f[0][K + k], red_f[1][K + k]), fmaxf(red_f[2][K + k], red_f[3][K + k])) : 0.f;
    }
    dst->n_systems = K;
    dst->reserved = 0;
  }
}

template <int K> constexpr int fusion_rows_in_flight() { return K <= 2 ? 4 : K <= 4 ? 2 : 1; }

// With sides: S.K matrices followed by sides, up to the kernel's K features.  Feature slot k < S.K is a matrix exactly as in
// FusionArgs; slot k >= S.K is a side: P.s[k] is its TEST vector and P.ld[k] = 0 (a "matrix" of pitch 0, so the strip walk's
// address and alignment arithmetic is the matrix's own), enrol[k] its ENROL vector (already offset to the first row of the
// launch), op[k] its PLDA_SIDE_* code.  P stays the FIRST member: the kernels re-read it at offset 0 of the kernel-argument
// segment (see fusion_pass_strip_kernel).
struct FusionSideArgs {
  FusionArgs P;
  const float *enrol[FUSION_KMAX];
  int32_t op[FUSION_KMAX];
  int32_t K, reserved;
};
static_assert(offsetof(FusionSideArgs, P) == 0, "the kernels read the FusionArgs at offset 0 of the kernel-argument segment");

template <bool SIDES> using FusionKernelArgs = std::conditional_t<SIDES, FusionSideArgs, FusionArgs>;
__device__ __forceinline__ const FusionArgs &fusion_systems(const FusionArgs &P) { return P; }
__device__ __forceinline__ const FusionArgs &fusion_systems(const FusionSideArgs &S) { return S.P; }

typedef const FusionSideArgs __attribute__((address_space(4))) *FusionSideArgsPtr;   // the struct where the kernel arguments live
typedef const float __attribute__((address_space(4))) *SideEnrolPtr;                 // read-only for the kernel's life: scalar loads

// the value of a side for (e = enrol[i], t = test[j]): ONE IEEE fp32 operation, ties and signed zeros by the written comparison
__device__ __forceinline__ float fusion_side_value(int op, float e, float t) {
  const float mn = e < t ? e : t, mx = e > t ? e : t, sm = e + t, ad = fabsf(e - t), pr = e * t;
  return op == PLDA_SIDE_MIN ? mn : op == PLDA_SIDE_MAX ? mx : op == PLDA_SIDE_SUM ? sm : op == PLDA_SIDE_ABSDIFF ? ad : pr;
}

// The labelled pass over K matrices, or (SIDES) over S.K matrices and K - S.K sides: block b writes part[b].  Traversal and
// labelling of calib_pass_strip_kernel.
// Resources on gfx950 (kernel-resource-usage; VGPRs per lane, no AGPRs; scratch 0, SGPR and VGPR spills 0 in every row):
//     K                  1     2     3     4     5     6     7     8
//     labelled pass     94   122   130   156   162   188   214   244     waves per SIMD 5 4 3 3 3 2 2 2  (SIDES or not)
//     list pass         60    69    86   103   122   143   166   191
//     map               16    20    24    28    32    36    40    44
//     side map          20    26    34    42    50    58    66    74
// fusion_reduce_kernel: 73.  Three things keep the K = 8 labelled pass inside the 256 registers of two waves per SIMD:
//   * the file is compiled without machine LICM (build.py, which says what the compiler does with it on and how to
//     reproduce this table): hoisted out of the walk, the fp64 constants of exp / log1p sit in some forty registers for the
//     whole kernel;
//   * for K > 2 the 4 U elements of a step go through ONE copy of the account in a rolled loop (selects on the wave-uniform
//     counter pick the element); 4 U inlined copies also hoist their lane masks and constants into scalar registers, which
//     then spill (scalar spills from K = 3 on);
//   * bases and pitches are re-read from the kernel-argument segment per step, and the per-system 16-byte flags live in one
//     per-thread bit mask, instead of 4 K + 2 K scalar registers held across the account.
// amdgpu_waves_per_eu(2) states the budget; nothing is spilled to meet it.
//
// REQUIREMENT of the re-read: the argument record `S` is the FIRST kernel parameter in both instantiations, and the
// FusionArgs the first member of a FusionSideArgs, so that it lies at offset 0 of the kernel-argument segment
// (explicit arguments are laid out in declaration order from offset 0, a by-value aggregate in place; hidden arguments follow
// them).  Whoever reorders the parameters must move the re-read with them: nothing else would notice.  The empty asm beside
// it has no instruction; its "+s" / "+v" operands only make the three values opaque once per step, so that the loads, the
// bit tests of `vec` and the column bounds are recomputed there instead of being held in scalar registers across the account.
//
// THE SIDE BRANCH (SIDES) lives in the load stage, where the account's registers are not yet live: the instantiations with
// it report the figures of those without exactly.  A side being a matrix of pitch 0, the address, the per-slot choice between
// 16-byte and scalar loads and the column bounds are the matrix's own code; the four test values are RE-READ per row from the
// L2-resident vector (a plain load, where a matrix streams with a non-temporal one), enrol[row] is one scalar load
// (wave-uniform address, constant address space), and the op is a wave-uniform select over the five fp32 results: about 12
// fp32 VALU instructions per side per trial (the five results, four selects, the column bound) beside the account's 221+
// fp64 ones -- MEASURED, they are not free: 20 000 x 20 000 at 2.39 GHz, (K, Q) = (1, 3) 5.80 ms against 4.86 ms for the
// matrix pass on materialised sides, (1, 7) 10.35 against 8.27 ms (profiles/fusion_side_*.json), the pass being bound by VALU
// issue.  A wave-uniform BRANCH on the op (one body of 1 - 2 instructions per value) was tried and not kept: at K = 8 it
// spills two scalar registers (245 VGPRs); it is the next step, for K <= 7 or with the scalar pressure of the K = 8 walk
// reduced first.  Holding the 4 Q test values in registers across the walk instead was not built: the walk already sits at
// 244 of 256 VGPRs at K = 8 and 130 .. 214 in between, so the persistent floats fit only the smallest K, and the pass is
// bound by fp64 VALU issue, not by these loads (has the measurement).  One form for every (K, Q).
// Elements beyond the last column get 0.f, as a matrix's loads give them: they count for nothing, but a NaN from enrol[row]
// in such a lane would otherwise reach the accumulators through 0 * NaN.
template <int K, bool SIDES>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void fusion_pass_strip_kernel(const FusionKernelArgs<SIDES> S, int64_t M, int64_t Nt, const int64_t *__restrict__ espk,
                              const int64_t *__restrict__ tspk, int64_t rows_per_wg, plda_fusion_record *__restrict__ part) {
  const FusionArgs &P = fusion_systems(S);
  constexpr int U = fusion_rows_in_flight<K>();
  const int64_t strips = (Nt + FUSION_STRIP - 1) / FUSION_STRIP;
  const int64_t strip = blockIdx.x % strips, slice = blockIdx.x / strips;
  const int64_t col = strip * FUSION_STRIP + (int64_t)threadIdx.x * 4;
  const int64_t r0 = slice * rows_per_wg, r1 = (r0 + rows_per_wg < M) ? r0 + rows_per_wg : M;
  int64_t ts[4];
  bool ok[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    ok[e] = col + e < Nt;
    ts[e] = ok[e] ? tspk[col + e] : 0;
  }
  unsigned vec = 0;                          // bit k: slot k takes 16-byte loads (one register, not K lane masks; a side's pitch 0 passes)
#pragma unroll
  for (int k = 0; k < K; ++k) vec |= (((P.ld[k] & 3) == 0) && ((reinterpret_cast<uintptr_t>(P.s[k]) & 15) == 0) && ok[3]) ? 1u << k : 0u;
  FusionAcc<K> A;
  for (int64_t row = r0; row < r1; row += U) {
    float v[U][K][4];
    // bases and pitches are re-read from the kernel-argument segment (scalar loads) once per step instead of being held in
    // 4 K scalar registers across the account, whose fp64 constants need those registers
    FusionArgsPtr pp = (FusionArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    int64_t colv = col;
    asm volatile("" : "+s"(pp), "+v"(vec), "+v"(colv));   // (nor are the bit tests of `vec` and the column bounds hoisted into lane masks)
    [[maybe_unused]] const FusionSideArgsPtr sp = (FusionSideArgsPtr)pp;   // SIDES: the same record, with what follows the FusionArgs
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (row + u >= r1) break;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float *src = const_cast<const float *>(pp->s[k]) + (row + u) * pp->ld[k] + col;
        bool side = false;                                   // wave-uniform; slot 0 is always a matrix
        if constexpr (SIDES) side = k > 0 && k >= sp->K;
        if (vec >> k & 1u) {
          const f32x4f x = side ? *reinterpret_cast<const f32x4f *>(src) : __builtin_nontemporal_load(reinterpret_cast<const f32x4f *>(src));
          v[u][k][0] = x.x; v[u][k][1] = x.y; v[u][k][2] = x.z; v[u][k][3] = x.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[u][k][e] = colv + e < Nt ? src[e] : 0.f;
        }
        if constexpr (SIDES) {
          if (side) {
            const float ev = ((SideEnrolPtr)sp->enrol[k])[row + u];
            const int op = sp->op[k];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[u][k][e] = colv + e < Nt ? fusion_side_value(op, ev, v[u][k][e]) : 0.f;
          }
        }
      }
    }
    if constexpr (K <= 2) {                 // K10's shape: every element's account inlined, elements interleave freely
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (row + u >= r1) break;
        const int64_t spk = espk[row + u];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (!__builtin_amdgcn_ballot_w64(ok[e])) continue;      // wave-uniform: a wave wholly beyond the last column
          float sf[K];
#pragma unroll
          for (int k = 0; k < K; ++k) sf[k] = v[u][k][e];
          fusion_account<K, -1>(A, sf, ok[e], ts[e] == spk, P);
        }
      }
    } else {
      // ONE copy of the account: the 4 U elements are visited by a rolled loop whose (wave-uniform) counter picks the
      // element through selects -- 4 U inlined copies hoist their constants into more scalar registers than there are
#pragma unroll 1
      for (int q = 0; q < 4 * U; ++q) {
        const int u = q >> 2, e = q & 3;
        if (row + u >= r1) break;
        const bool valid = colv + e < Nt;
        if (!__builtin_amdgcn_ballot_w64(valid)) continue;        // wave-uniform: a wave wholly beyond the last column
        const int64_t spk = espk[row + u];
        int64_t tse = ts[0];
#pragma unroll
        for (int i = 1; i < 4; ++i) tse = e == i ? ts[i] : tse;
        float sf[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          float x = v[0][k][0];
#pragma unroll
          for (int i = 1; i < 4 * U; ++i) x = q == i ? v[i >> 2][k][i & 3] : x;
          sf[k] = x;
        }
        fusion_account<K, -1>(A, sf, valid, tse == spk, P);
      }
    }
  }
  fusion_block_store<K>(A, 0, part + blockIdx.x);
}

// K parallel flat arrays of one fixed class (P.ld is not used)
template <int K, int CLS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void fusion_pass_list_kernel(const FusionArgs P, int64_t n, plda_fusion_record *__restrict__ part) {
  FusionAcc<K> A;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx - threadIdx.x < n; idx += (int64_t)gridDim.x * 256)
    if (idx < n) {
      float sf[K];
#pragma unroll
      for (int k = 0; k < K; ++k) sf[k] = P.s[k][idx];
      fusion_account<K, CLS>(A, sf, true, CLS != 0, P);
    }
  fusion_block_store<K>(A, CLS, part + blockIdx.x);
}

// part[0 .. n) -> *out, one block of 1024 threads.  Sums: thread (g = tid / 128, e = tid % 128 < 110) adds entry e of the
// partials g, g + 8, ... in ascending order, then the eight groups are added as a fixed tree.  Counts and extremes are exact
// in any order.
__global__ __launch_bounds__(1024) void fusion_reduce_kernel(const plda_fusion_record *__restrict__ part, int64_t n, int K,
                                                              plda_fusion_record *__restrict__ out) {
  __shared__ double red[8][128];
  __shared__ double red_y[16][4];
  __shared__ unsigned long long red_c[16][5];
  __shared__ float red_f[16][2 * FUSION_KMAX];
  const int tid = threadIdx.x, e = tid & 127, g = tid >> 7;
  double acc = 0.0;
  if (e < 2 * FUSION_SLOTS)
    for (int64_t i = g; i < n; i += 8) acc += reinterpret_cast<const double *>(&part[i].sum[0])[e];
  red[g][e] = acc;
  double y[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};   // ymin[0], ymax[0], ymin[1], ymax[1]
  unsigned long long cnt[5] = {0, 0, 0, 0, 0};
  float f[2 * FUSION_KMAX];
#pragma unroll
  for (int k = 0; k < FUSION_KMAX; ++k) { f[k] = INFINITY; f[FUSION_KMAX + k] = -INFINITY; }
  for (int64_t i = tid; i < n; i += 1024) {
    const plda_fusion_record &r = part[i];
    y[0] = fmin(y[0], r.ymin[0]); y[1] = fmax(y[1], r.ymax[0]); y[2] = fmin(y[2], r.ymin[1]); y[3] = fmax(y[3], r.ymax[1]);
    cnt[0] += r.np; cnt[1] += r.nn; cnt[2] += r.miss; cnt[3] += r.fa; cnt[4] += r.nonfinite;
#pragma unroll
    for (int k = 0; k < FUSION_KMAX; ++k) { f[k] = fminf(f[k], r.smin[k]); f[FUSION_KMAX + k] = fmaxf(f[FUSION_KMAX + k], r.smax[k]); }
  }
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 5; ++k) cnt[k] += __shfl_xor(cnt[k], o);
    y[0] = fmin(y[0], __shfl_xor(y[0], o)); y[1] = fmax(y[1], __shfl_xor(y[1], o));
    y[2] = fmin(y[2], __shfl_xor(y[2], o)); y[3] = fmax(y[3], __shfl_xor(y[3], o));
#pragma unroll
    for (int k = 0; k < FUSION_KMAX; ++k) {
      f[k] = fminf(f[k], __shfl_xor(f[k], o));
      f[FUSION_KMAX + k] = fmaxf(f[FUSION_KMAX + k], __shfl_xor(f[FUSION_KMAX + k], o));
    }
  }
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red_y[wave][k] = y[k];
#pragma unroll
    for (int k = 0; k < 5; ++k) red_c[wave][k] = cnt[k];
#pragma unroll
    for (int k = 0; k < 2 * FUSION_KMAX; ++k) red_f[wave][k] = f[k];
  }
  __syncthreads();
  if (tid < 2 * FUSION_SLOTS)
    reinterpret_cast<double *>(&out->sum[0])[tid] =
        ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) + ((red[4][tid] + red[5][tid]) + (red[6][tid] + red[7][tid]));
  if (tid == 0) {
    for (int w = 1; w < 16; ++w) {
      red_y[0][0] = fmin(red_y[0][0], red_y[w][0]); red_y[0][1] = fmax(red_y[0][1], red_y[w][1]);
      red_y[0][2] = fmin(red_y[0][2], red_y[w][2]); red_y[0][3] = fmax(red_y[0][3], red_y[w][3]);
      for (int k = 0; k < 5; ++k) red_c[0][k] += red_c[w][k];
      for (int k = 0; k < FUSION_KMAX; ++k) {
        red_f[0][k] = fminf(red_f[0][k], red_f[w][k]);
        red_f[0][FUSION_KMAX + k] = fmaxf(red_f[0][FUSION_KMAX + k], red_f[w][FUSION_KMAX + k]);
      }
    }
    out->ymin[0] = red_y[0][0]; out->ymax[0] = red_y[0][1]; out->ymin[1] = red_y[0][2]; out->ymax[1] = red_y[0][3];
    out->np = red_c[0][0]; out->nn = red_c[0][1]; out->miss = red_c[0][2]; out->fa = red_c[0][3]; out->nonfinite = red_c[0][4];
    for (int k = 0; k < FUSION_KMAX; ++k) {
      out->smin[k] = k < K ? red_f[0][k] : 0.f;
      out->smax[k] = k < K ? red_f[0][FUSION_KMAX + k] : 0.f;
    }
    out->n_systems = K;
    out->reserved = 0;
  }
}

// out[i, j] = (float)chain(b; s_0[i, j] .. s_{K-1}[i, j]): strips of 1024 columns, rows dealt out over gridDim.y.  In place over
// one of the inputs is allowed (an element is read from every system, then written, by the same thread); columns
// [Nt, ld_out) are not touched.  16-byte access per system and for the output where base and pitch allow.
// (Giving this kernel fusion_side_map_kernel's form -- one template on <K, SIDES> -- was built and measured: 20 / 22 / .. / 46
// VGPRs and 30 .. 47 SGPRs, and at 20 000 x 20 000 its medians lay within 0.5 % of this form's, but at K = 1 outside the spread of
// this form's own two medians, which was the bar: profiles/fusion_map_merge.json.  So matrices keep this text.)
template <int K>
__global__ __launch_bounds__(256) void fusion_map_kernel(const FusionArgs P, int64_t M, int64_t Nt, float *out, int64_t ld_out) {
  const int64_t col = (int64_t)blockIdx.x * FUSION_STRIP + (int64_t)threadIdx.x * 4;
  if (col >= Nt) return;
  const bool full = col + 3 < Nt;
  bool vec[K];
#pragma unroll
  for (int k = 0; k < K; ++k) vec[k] = ((P.ld[k] & 3) == 0) && ((reinterpret_cast<uintptr_t>(P.s[k]) & 15) == 0) && full;
  const bool vec_out = ((ld_out & 3) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0) && full;
  for (int64_t row = blockIdx.y; row < M; row += gridDim.y) {
    double y[4] = {P.c, P.c, P.c, P.c};
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float *src = P.s[k] + row * P.ld[k] + col;
      float x[4];
      if (vec[k]) {
        const f32x4f q = *reinterpret_cast<const f32x4f *>(src);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = col + e < Nt ? src[e] : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = fma(P.a[k], (double)x[e], y[e]);
    }
    float *dst = out + row * ld_out + col;
    if (vec_out) {
      f32x4f q;
      q.x = (float)y[0]; q.y = (float)y[1]; q.z = (float)y[2]; q.w = (float)y[3];
      *reinterpret_cast<f32x4f *>(dst) = q;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (col + e < Nt) dst[e] = (float)y[e];
    }
  }
}

// The map over S.K matrices and K - S.K sides: out[i, j] = (float)chain(b; s_0[i, j] .. , q_0(i, j) ..), fusion_map_kernel's
// walk and rules (in place over one of the matrices allowed, columns [Nt, ld_out) not touched).  Here the four test values of
// every side ARE held in registers (tv, 4 K floats; the kernel has room -- the table at fusion_pass_strip_kernel), so a trial
// costs the matrix reads, one scalar load per side per row and the store: 4 S.K + 4 bytes instead of 4 K + 4.
template <int K>
__global__ __launch_bounds__(256) void fusion_side_map_kernel(const FusionSideArgs S, int64_t M, int64_t Nt, float *out, int64_t ld_out) {
  const int64_t col = (int64_t)blockIdx.x * FUSION_STRIP + (int64_t)threadIdx.x * 4;
  if (col >= Nt) return;
  const bool full = col + 3 < Nt;
  unsigned vec = 0;                          // bit k: slot k takes 16-byte loads; bit K: the output takes 16-byte stores
  float tv[K][4];                            // slot k >= S.K: the side's test values of this thread's columns
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const bool wide = ((S.P.ld[k] & 3) == 0) && ((reinterpret_cast<uintptr_t>(S.P.s[k]) & 15) == 0) && full;
    vec |= wide ? 1u << k : 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) tv[k][e] = 0.f;
    if (k > 0 && k >= S.K) {
      const float *src = S.P.s[k] + col;
      if (wide) {
        const f32x4f q = *reinterpret_cast<const f32x4f *>(src);
        tv[k][0] = q.x; tv[k][1] = q.y; tv[k][2] = q.z; tv[k][3] = q.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) tv[k][e] = col + e < Nt ? src[e] : 0.f;
      }
    }
  }
  vec |= (((ld_out & 3) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0) && full) ? 1u << K : 0u;
  for (int64_t row = blockIdx.y; row < M; row += gridDim.y) {
    // bases, pitches, weights, enrol vectors and ops are re-read from the kernel-argument segment per row (scalar loads; S is
    // the FIRST parameter, see fusion_pass_strip_kernel) and the 16-byte flags sit in one per-thread bit mask: held across the
    // loop they are some 90 scalar registers at K = 8, which spilled from K = 6 on (14 / 30 / 46 SGPRs)
    FusionSideArgsPtr pp = (FusionSideArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(pp), "+v"(vec));
    const double c = pp->P.c;
    double y[4] = {c, c, c, c};
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float x[4];
      if (k > 0 && k >= pp->K) {
        const float ev = ((SideEnrolPtr)pp->enrol[k])[row];
        const int op = pp->op[k];
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = fusion_side_value(op, ev, tv[k][e]);
      } else {
        const float *src = const_cast<const float *>(pp->P.s[k]) + row * pp->P.ld[k] + col;
        if (vec >> k & 1u) {
          const f32x4f q = *reinterpret_cast<const f32x4f *>(src);
          x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) x[e] = col + e < Nt ? src[e] : 0.f;
        }
      }
      const double ak = pp->P.a[k];
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = fma(ak, (double)x[e], y[e]);
    }
    float *dst = out + row * ld_out + col;
    if (vec >> K & 1u) {
      f32x4f q;
      q.x = (float)y[0]; q.y = (float)y[1]; q.z = (float)y[2]; q.w = (float)y[3];
      *reinterpret_cast<f32x4f *>(dst) = q;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (col + e < Nt) dst[e] = (float)y[e];
    }
  }
}

// ------------------------------------------------------------------------------------ host drivers
static int64_t fusion_strip_blocks(int64_t rows, int64_t Nt, int64_t *rows_per_wg) {
  const int64_t strips = ceil_div(Nt, (int64_t)FUSION_STRIP);
  const int64_t slices = std::max<int64_t>(1, std::min<int64_t>(rows, FUSION_MAX_BLOCKS / strips));
  *rows_per_wg = ceil_div(rows, slices);
  return strips * ceil_div(rows, *rows_per_wg);
}
static int64_t fusion_list_blocks(int64_t n) { return std::min<int64_t>(ceil_div(n, 256), FUSION_MAX_BLOCKS); }

// the labelled trials of a fusion call: K matrices under one pair of speaker-id arrays, or K target + K non-target lists.
// With sides (K25): K counts every FEATURE, the first `nsys` of them matrices and the rest sides -- slot
// k >= nsys holds the side's test vector in s[k] (pitch 0), its enrol vector in enrol[k] and its op in op[k].  Operand form:
// `slabs` produces system 0 one row slab at a time (s[0] / ld[0] are then filled per slab).
struct FusionSource {
  int K = 0, nsys = 0;
  bool lists = false;
  const float *s[FUSION_KMAX] = {}, *neg[FUSION_KMAX] = {};   // matrices, or the target lists; the non-target lists
  int64_t ld[FUSION_KMAX] = {};
  int64_t M = 0, Nt = 0;                                       // lists: np, nn
  const int64_t *espk = nullptr, *tspk = nullptr;
  const float *enrol[FUSION_KMAX] = {};
  int32_t op[FUSION_KMAX] = {};
  const TrialSource *slabs = nullptr;
};

// the kernel arguments of `src` at weights a[src.K] and offset c, the enrol vectors of its sides offset to row r0 of the call
static FusionSideArgs fusion_kernel_args(const FusionSource &src, const double *a, double c, int64_t r0) {
  FusionSideArgs S = {};
  for (int k = 0; k < src.K; ++k) { S.P.s[k] = src.s[k]; S.P.ld[k] = src.ld[k]; S.P.a[k] = a[k]; }
  S.P.c = c;
  S.K = src.nsys;
  for (int k = src.nsys; k < src.K; ++k) { S.enrol[k] = src.enrol[k] + r0; S.op[k] = src.op[k]; }
  return S;
}

// the launches: instantiation K = the number of feature slots, SIDES where some of them are sides (S.K matrices < K)
#define FUSION_DISPATCH(K, CALL)                                              \
  switch (K) {                                                               \
    case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; \
    case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; default: CALL(8); break; \
  }

static void fusion_dispatch_strip(plda_handle *h, int K, const FusionSideArgs &S, int64_t rows, int64_t Nt, const int64_t *espk,
                                  const int64_t *tspk, int64_t blocks, int64_t rpw, plda_fusion_record *part) {
#define FUSION_CALL(KK)                                                                                                        \
  if (S.K != K) fusion_pass_strip_kernel<KK, true><<<(unsigned)blocks, 256, 0, h->stream>>>(S, rows, Nt, espk, tspk, rpw, part); \
  else fusion_pass_strip_kernel<KK, false><<<(unsigned)blocks, 256, 0, h->stream>>>(S.P, rows, Nt, espk, tspk, rpw, part)
  FUSION_DISPATCH(K, FUSION_CALL)
#undef FUSION_CALL
}
static void fusion_dispatch_list(plda_handle *h, int K, const FusionArgs &P, int64_t n, int cls, int64_t blocks, plda_fusion_record *part) {
#define FUSION_CALL(KK)                                                                            \
  if (cls) fusion_pass_list_kernel<KK, 1><<<(unsigned)blocks, 256, 0, h->stream>>>(P, n, part);    \
  else fusion_pass_list_kernel<KK, 0><<<(unsigned)blocks, 256, 0, h->stream>>>(P, n, part)
  FUSION_DISPATCH(K, FUSION_CALL)
#undef FUSION_CALL
}
static void fusion_dispatch_map(plda_handle *h, int K, const FusionSideArgs &S, int64_t M, int64_t Nt, float *out, int64_t ld_out) {
  const dim3 grid((unsigned)ceil_div(Nt, (int64_t)FUSION_STRIP), (unsigned)std::min<int64_t>(M, 4096));
#define FUSION_CALL(KK)                                                                             \
  if (S.K != K) fusion_side_map_kernel<KK><<<grid, 256, 0, h->stream>>>(S, M, Nt, out, ld_out);     \
  else fusion_map_kernel<KK><<<grid, 256, 0, h->stream>>>(S.P, M, Nt, out, ld_out)
  FUSION_DISPATCH(K, FUSION_CALL)
#undef FUSION_CALL
}
#undef FUSION_DISPATCH

// One pass over `src` at (a, c, theta) -> *rec (host); synchronises the stream.  A non-finite score, or a class without
// trials, is PLDA_E_INVAL (the record is written all the same).  A matrix call is one piece on the grid of its shape; the
// operand form is one piece per slab (trial_source.hpp), the partials of all slabs sized before anything is launched, as
// calib_pass does, and reduced together in slab order.
static int fusion_pass(plda_handle *h, const FusionSource &src, const double *a, double c, double theta, plda_fusion_record *rec) {
  const TrialSource whole = TrialSource::matrix(src.s[0], src.ld[0], src.M, src.Nt, src.espk, src.tspk);
  const TrialSource &ts = src.slabs ? *src.slabs : whole;
  int64_t total = 0;
  if (src.lists) total = fusion_list_blocks(src.M) + fusion_list_blocks(src.Nt);
  else {
    if (ceil_div(src.Nt, (int64_t)FUSION_STRIP) > (int64_t)0x7fffffff) return fail(h, PLDA_E_CAPACITY, "fusion: too many column strips");
    bool fits = true;
    PLDA_TRY(for_each_piece(ts, [&](const TrialPiece &pc) -> int {
      int64_t rpw = 0;
      const int64_t blocks = fusion_strip_blocks(pc.rows, pc.Nt, &rpw);
      fits = fits && blocks <= (int64_t)0x7fffffff && rpw <= (int64_t)0x3fffffff;
      total += blocks;
      return PLDA_OK;
    }, /*produce=*/false));
    if (!fits || total > (int64_t)0x7fffffff) return fail(h, PLDA_E_CAPACITY, "fusion: too many column strips or rows per workgroup");
  }
  PLDA_HIP(h, h->fusion_part.reserve((size_t)(total + 1) * sizeof(plda_fusion_record)));
  plda_fusion_record *part = h->fusion_part.as<plda_fusion_record>();
  if (src.lists) {
    const int64_t bp = fusion_list_blocks(src.M), bn = fusion_list_blocks(src.Nt);
    FusionArgs P = fusion_kernel_args(src, a, c, 0).P;
    P.theta = theta;
    fusion_dispatch_list(h, src.K, P, src.M, 1, bp, part);
    PLDA_LAUNCH_CHECK(h);
    for (int k = 0; k < src.K; ++k) P.s[k] = src.neg[k];
    fusion_dispatch_list(h, src.K, P, src.Nt, 0, bn, part + bp);
    PLDA_LAUNCH_CHECK(h);
  } else {
    int64_t at = 0;
    PLDA_TRY(for_each_piece(ts, [&](const TrialPiece &pc) -> int {
      int64_t rpw = 0;
      const int64_t blocks = fusion_strip_blocks(pc.rows, pc.Nt, &rpw);
      FusionSideArgs S = fusion_kernel_args(src, a, c, pc.espk - src.espk);
      S.P.theta = theta;
      S.P.s[0] = pc.scores; S.P.ld[0] = pc.ld;
      fusion_dispatch_strip(h, src.K, S, pc.rows, pc.Nt, pc.espk, src.tspk, blocks, rpw, part + at);
      PLDA_LAUNCH_CHECK(h);
      at += blocks;
      return PLDA_OK;
    }));
  }
  fusion_reduce_kernel<<<1, 1024, 0, h->stream>>>(part, total, src.K, part + total);
  PLDA_LAUNCH_CHECK(h);
  PLDA_HIP(h, hipMemcpyAsync(rec, part + total, sizeof(*rec), hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  if (rec->nonfinite)
    return fail(h, PLDA_E_INVAL, src.K == src.nsys ? "fusion: %llu trials with a non-finite score" : "fusion: %llu trials with a non-finite score or side value",
                (unsigned long long)rec->nonfinite);
  if (rec->np == 0 || rec->nn == 0) return fail(h, PLDA_E_INVAL, "fusion: need at least one target and one non-target trial");
  return PLDA_OK;
}

// ------------------------------------------------------------------------------------ the Newton step (pure)
// why: 0 fine, 1 bad argument, 2 a diagonal entry <= 0, 3 a Cholesky pivot <= 1e-12; *at: the index in x = (b, a_0 ..)
static int fusion_newton_core(const plda_fusion_record *r, double prior, double *F, double *d, double *lambda2, int *at) {
  if (!r || !F || !d || !lambda2 || !(prior > 0.0 && prior < 1.0) || r->n_systems < 1 || r->n_systems > FUSION_KMAX || r->np == 0 ||
      r->nn == 0)
    return 1;
  const int n = r->n_systems + 1;
  const double wt = prior / (double)r->np, wn = (1.0 - prior) / (double)r->nn;
  double g[FUSION_KMAX + 1], H[FUSION_KMAX + 1][FUSION_KMAX + 1], L[FUSION_KMAX + 1][FUSION_KMAX + 1], sc[FUSION_KMAX + 1],
      z[FUSION_KMAX + 1], x[FUSION_KMAX + 1];
  *F = wt * r->sum[1].L + wn * r->sum[0].L;
  for (int j = 0; j < n; ++j) {
    g[j] = -wt * r->sum[1].G[j] + wn * r->sum[0].G[j];
    for (int i = 0; i <= j; ++i) H[i][j] = H[j][i] = wt * r->sum[1].H[j * (j + 1) / 2 + i] + wn * r->sum[0].H[j * (j + 1) / 2 + i];
  }
  for (int j = 0; j < n; ++j) {
    if (!(H[j][j] > 0.0)) { *at = j; return 2; }
    sc[j] = 1.0 / std::sqrt(H[j][j]);
  }
  // Cholesky of Hs = D^-1/2 H D^-1/2 (unit diagonal), row by row; L z = gs; L' x = z; d = -D^-1/2 x
  for (int j = 0; j < n; ++j) {
    for (int i = 0; i <= j; ++i) {
      double v = (H[j][i] * sc[j]) * sc[i];
      for (int k = 0; k < i; ++k) v -= L[j][k] * L[i][k];
      if (i < j) L[j][i] = v / L[i][i];
      else {
        if (!(v > 1e-12)) { *at = j; return 3; }
        L[j][j] = std::sqrt(v);
      }
    }
  }
  double lam = 0.0;
  for (int j = 0; j < n; ++j) {
    double v = g[j] * sc[j];
    for (int k = 0; k < j; ++k) v -= L[j][k] * z[k];
    z[j] = v / L[j][j];
    lam += z[j] * z[j];
  }
  for (int j = n - 1; j >= 0; --j) {
    double v = z[j];
    for (int k = j + 1; k < n; ++k) v -= L[k][j] * x[k];
    x[j] = v / L[j][j];
  }
  for (int j = 0; j < n; ++j) d[j] = -(x[j] * sc[j]);
  *lambda2 = lam;
  return 0;
}
static int fusion_newton_fail(plda_handle *h, int why, int at, int nsys = FUSION_KMAX) {   // features from nsys on are sides (K25)
  char who[32];
  if (at == 0) std::snprintf(who, sizeof(who), "the offset");
  else if (at - 1 >= nsys) std::snprintf(who, sizeof(who), "side %d", at - 1 - nsys);
  else std::snprintf(who, sizeof(who), "system %d", at - 1);
  if (why == 2) return fail(h, PLDA_E_INVAL, "fusion_newton: the Hessian's diagonal entry of %s is not positive", who);
  if (why == 3)
    return fail(h, PLDA_E_INVAL, "fusion_newton: the Cholesky pivot of %s is <= 1e-12: it is an affine function of the systems before it "
                                 "to within what the sums resolve (a duplicated or constant system?)", who);
  return fail(h, PLDA_E_INVAL, "fusion_newton: bad argument (a record of 1 .. %d systems with both classes, prior inside (0, 1))", FUSION_KMAX);
}
int fusion_newton(const plda_fusion_record *r, double prior, double *F, double *d, double *lambda2) {
  int at = 0;
  const int why = fusion_newton_core(r, prior, F, d, lambda2, &at);
  return why ? fusion_newton_fail(nullptr, why, at) : PLDA_OK;
}

static double fusion_objective(const plda_fusion_record &r, double prior) {
  return prior / (double)r.np * r.sum[1].L + (1.0 - prior) / (double)r.nn * r.sum[0].L;
}

static int fusion_fit(plda_handle *h, const FusionSource &src, double prior, double tol, int max_iter, plda_fusion_fit *out) {
  if (!out || !(prior > 0.0 && prior < 1.0) || !(tol >= 0.0)) return fail(h, PLDA_E_INVAL, "fusion_fit: bad argument (prior must lie inside (0, 1), tol >= 0)");
  if (tol == 0.0) tol = 1e-18;
  if (max_iter <= 0) max_iter = 100;
  const int K = src.K, n = K + 1;
  const double tau = std::log(prior / (1.0 - prior)), ln2 = std::log(2.0);
  plda_fusion_record rec, trial;
  int passes = 0;
  double x[FUSION_KMAX + 1] = {}, nx[FUSION_KMAX + 1] = {};    // (b, a_0 .. a_{K-1})
  auto take = [&](const double *xx, double shift, plda_fusion_record *r) { return fusion_pass(h, src, xx + 1, xx[0] + shift, 0.0, r); };
  PLDA_TRY(take(x, tau, &rec)); ++passes;
  for (int k = 0; k < K; ++k)
    if (rec.smin[k] == rec.smax[k])
      return k < src.nsys ? fail(h, PLDA_E_INVAL, "fusion_fit: system %d is constant (every score equals %g): the Hessian is singular", k, (double)rec.smin[k])
                          : fail(h, PLDA_E_INVAL, "fusion_fit: side %d is constant (every value equals %g): the Hessian is singular", k - src.nsys, (double)rec.smin[k]);
  double lam2 = INFINITY, F = 0.0;
  int it = 0;
  bool converged = false;
  for (;;) {
    double d[FUSION_KMAX + 1];
    int at = 0;
    const int why = fusion_newton_core(&rec, prior, &F, d, &lam2, &at);
    // on separable data the iteration runs away and the weights w die out trial by trial until fewer than K + 1 trials carry
    // the Hessian: that is where the iteration stops (not converged, separable reported), not a refusal of the systems
    if (why >= 2 && it > 0 && rec.ymin[1] > rec.ymax[0]) break;
    if (why) return fusion_newton_fail(h, why, at, src.nsys);
    if (lam2 <= tol) { converged = true; break; }
    if (it >= max_iter) break;
    double t = 1.0;
    bool accepted = false;
    for (int k = 0; k <= 30; ++k, t *= 0.5) {
      for (int j = 0; j < n; ++j) nx[j] = x[j] + t * d[j];
      PLDA_TRY(take(nx, tau, &trial)); ++passes;
      if (fusion_objective(trial, prior) <= F - 1e-4 * t * lam2 + 0x1p-44 * std::fabs(F)) { accepted = true; break; }
    }
    if (!accepted) break;
    for (int j = 0; j < n; ++j) x[j] = nx[j];
    rec = trial; ++it;
  }
  plda_fusion_record after = rec;
  if (prior != 0.5) { PLDA_TRY(take(x, 0.0, &after)); ++passes; }
  *out = plda_fusion_fit();
  for (int k = 0; k < K; ++k) out->a[k] = x[1 + k];
  out->b = x[0];
  out->objective = fusion_objective(rec, prior) / ln2;
  out->cllr_after = fusion_objective(after, 0.5) / ln2;
  out->lambda2 = lam2;
  out->iterations = it; out->passes = passes; out->converged = converged ? 1 : 0;
  out->separable = rec.ymin[1] > rec.ymax[0] ? 1 : 0;
  return PLDA_OK;
}

static int fusion_matrix_source(plda_handle *h, const char *fn, int K, const float *const *dscores, const int64_t *ld, int64_t M,
                                int64_t Nt, const int64_t *despk, const int64_t *dtspk, bool labelled, FusionSource *s) {
  if (K < 1 || K > FUSION_KMAX) return fail(h, PLDA_E_INVAL, "%s: n_systems must be 1 .. %d (got %d)", fn, FUSION_KMAX, K);
  if (!dscores || !ld || M <= 0 || Nt <= 0 || (labelled && (!despk || !dtspk))) return fail(h, PLDA_E_INVAL, "%s: bad argument", fn);
  for (int k = 0; k < K; ++k) {
    if (!dscores[k]) return fail(h, PLDA_E_INVAL, "%s: the matrix of system %d is NULL", fn, k);
    if (ld[k] < Nt) return fail(h, PLDA_E_INVAL, "%s: ld[%d] = %lld < Nt = %lld", fn, k, (long long)ld[k], (long long)Nt);
    s->s[k] = dscores[k]; s->ld[k] = ld[k];
  }
  s->K = K; s->nsys = K; s->lists = false; s->M = M; s->Nt = Nt; s->espk = despk; s->tspk = dtspk;
  return PLDA_OK;
}
int fusion_list_args_check(plda_handle *h, const char *fn, int K, const float *const *pos, int64_t np, const float *const *neg, int64_t nn) {
  if (K < 1 || K > FUSION_KMAX) return fail(h, PLDA_E_INVAL, "%s: n_systems must be 1 .. %d (got %d)", fn, FUSION_KMAX, K);
  if (!pos || !neg) return fail(h, PLDA_E_INVAL, "%s: the array of %s list pointers is NULL", fn, !pos ? "target" : "non-target");
  if (np <= 0 || nn <= 0) return fail(h, PLDA_E_INVAL, "%s: need at least one target and one non-target trial", fn);
  for (int k = 0; k < K; ++k)
    if (!pos[k] || !neg[k]) return fail(h, PLDA_E_INVAL, "%s: the %s list of system %d is NULL", fn, !pos[k] ? "target" : "non-target", k);
  return PLDA_OK;
}
static int fusion_list_source(plda_handle *h, const char *fn, int K, const float *const *dpos, int64_t np, const float *const *dneg,
                              int64_t nn, FusionSource *s) {
  PLDA_TRY(fusion_list_args_check(h, fn, K, dpos, np, dneg, nn));
  for (int k = 0; k < K; ++k) { s->s[k] = dpos[k]; s->neg[k] = dneg[k]; }
  s->K = K; s->nsys = K; s->lists = true; s->M = np; s->Nt = nn;
  return PLDA_OK;
}

int fusion_pass_matrices_device(plda_handle *h, int K, const float *const *dscores, const int64_t *ld, int64_t M, int64_t Nt,
                                const int64_t *despk, const int64_t *dtspk, const double *a, double c, double theta,
                                plda_fusion_record *out) {
  if (!out || !a) return fail(h, PLDA_E_INVAL, "fusion_pass: the output record or the weight array is NULL");
  FusionSource s;
  PLDA_TRY(fusion_matrix_source(h, "fusion_pass", K, dscores, ld, M, Nt, despk, dtspk, true, &s));
  return fusion_pass(h, s, a, c, theta, out);
}
int fusion_fit_matrices_device(plda_handle *h, int K, const float *const *dscores, const int64_t *ld, int64_t M, int64_t Nt,
                               const int64_t *despk, const int64_t *dtspk, double prior, double tol, int max_iter, plda_fusion_fit *out) {
  if (!out) return fail(h, PLDA_E_INVAL, "fusion_fit: the output structure is NULL");
  FusionSource s;
  PLDA_TRY(fusion_matrix_source(h, "fusion_fit", K, dscores, ld, M, Nt, despk, dtspk, true, &s));
  return fusion_fit(h, s, prior, tol, max_iter, out);
}
int fusion_pass_lists_device(plda_handle *h, int K, const float *const *dpos, int64_t np, const float *const *dneg, int64_t nn,
                             const double *a, double c, double theta, plda_fusion_record *out) {
  if (!out || !a) return fail(h, PLDA_E_INVAL, "fusion_pass: the output record or the weight array is NULL");
  FusionSource s;
  PLDA_TRY(fusion_list_source(h, "fusion_pass", K, dpos, np, dneg, nn, &s));
  return fusion_pass(h, s, a, c, theta, out);
}
int fusion_fit_lists_device(plda_handle *h, int K, const float *const *dpos, int64_t np, const float *const *dneg, int64_t nn,
                            double prior, double tol, int max_iter, plda_fusion_fit *out) {
  if (!out) return fail(h, PLDA_E_INVAL, "fusion_fit: the output structure is NULL");
  FusionSource s;
  PLDA_TRY(fusion_list_source(h, "fusion_fit", K, dpos, np, dneg, nn, &s));
  return fusion_fit(h, s, prior, tol, max_iter, out);
}
// out = (float)chain(b; the features of `src`), the one map behind both entry points (a call without sides is fusion_map's)
static int fusion_map(plda_handle *h, const FusionSource &src, const double *a, double b, float *out, int64_t ld_out) {
  if (ceil_div(src.Nt, (int64_t)FUSION_STRIP) > (int64_t)0x7fffffff)
    return fail(h, PLDA_E_CAPACITY, src.K == src.nsys ? "fusion_map: too many column strips" : "fusion_side_map: too many column strips");
  fusion_dispatch_map(h, src.K, fusion_kernel_args(src, a, b, 0), src.M, src.Nt, out, ld_out);
  PLDA_LAUNCH_CHECK(h);
  return PLDA_OK;
}
int fusion_map_device(plda_handle *h, int K, const float *const *dscores, const int64_t *ld, int64_t M, int64_t Nt, const double *a,
                      double b, float *dout, int64_t ld_out) {
  if (!a || !dout || ld_out < Nt) return fail(h, PLDA_E_INVAL, "fusion_map: bad argument");
  FusionSource s;
  PLDA_TRY(fusion_matrix_source(h, "fusion_map", K, dscores, ld, M, Nt, nullptr, nullptr, false, &s));
  return fusion_map(h, s, a, b, dout, ld_out);
}

// ------------------------------------------------------------------------------------ sides (K25)
// appends the Q sides of a call to a source that holds its K systems: feature slot K + q is side q
static int fusion_side_source(plda_handle *h, const char *fn, int K, int Q, const plda_fusion_side *sides, FusionSource *s) {
  if (Q < 0 || K + Q > FUSION_KMAX)
    return fail(h, PLDA_E_INVAL, "%s: n_systems + n_sides must be at most %d with n_sides >= 0 (got %d + %d)", fn, FUSION_KMAX, K, Q);
  if (Q > 0 && !sides) return fail(h, PLDA_E_INVAL, "%s: the array of sides is NULL", fn);
  for (int q = 0; q < Q; ++q) {
    if (sides[q].op < PLDA_SIDE_MIN || sides[q].op > PLDA_SIDE_PROD) return fail(h, PLDA_E_INVAL, "%s: side %d has op %d (must be 0 .. 4)", fn, q, (int)sides[q].op);
    if (!sides[q].enrol || !sides[q].test) return fail(h, PLDA_E_INVAL, "%s: the %s vector of side %d is NULL", fn, !sides[q].enrol ? "enrol" : "test", q);
    s->s[K + q] = sides[q].test; s->ld[K + q] = 0; s->enrol[K + q] = sides[q].enrol; s->op[K + q] = sides[q].op;
  }
  s->nsys = K; s->K = K + Q;
  return PLDA_OK;
}

int fusion_side_pass_device(plda_handle *h, int K, const float *const *dscores, const int64_t *ld, int Q, const plda_fusion_side *sides,
                            int64_t M, int64_t Nt, const int64_t *despk, const int64_t *dtspk, const double *a, double c, double theta,
                            plda_fusion_record *out) {
  if (!out || !a) return fail(h, PLDA_E_INVAL, "fusion_side_pass: the output record or the weight array is NULL");
  FusionSource s;
  PLDA_TRY(fusion_matrix_source(h, "fusion_side_pass", K, dscores, ld, M, Nt, despk, dtspk, true, &s));
  PLDA_TRY(fusion_side_source(h, "fusion_side_pass", K, Q, sides, &s));
  return fusion_pass(h, s, a, c, theta, out);
}
int fusion_side_fit_device(plda_handle *h, int K, const float *const *dscores, const int64_t *ld, int Q, const plda_fusion_side *sides,
                           int64_t M, int64_t Nt, const int64_t *despk, const int64_t *dtspk, double prior, double tol, int max_iter,
                           plda_fusion_fit *out) {
  if (!out) return fail(h, PLDA_E_INVAL, "fusion_side_fit: the output structure is NULL");
  FusionSource s;
  PLDA_TRY(fusion_matrix_source(h, "fusion_side_fit", K, dscores, ld, M, Nt, despk, dtspk, true, &s));
  PLDA_TRY(fusion_side_source(h, "fusion_side_fit", K, Q, sides, &s));
  return fusion_fit(h, s, prior, tol, max_iter, out);
}
int fusion_side_map_device(plda_handle *h, int K, const float *const *dscores, const int64_t *ld, int Q, const plda_fusion_side *sides,
                           int64_t M, int64_t Nt, const double *a, double b, float *dout, int64_t ld_out) {
  if (!a || !dout || ld_out < Nt) return fail(h, PLDA_E_INVAL, "fusion_side_map: bad argument");
  FusionSource s;
  PLDA_TRY(fusion_matrix_source(h, "fusion_side_map", K, dscores, ld, M, Nt, nullptr, nullptr, false, &s));
  PLDA_TRY(fusion_side_source(h, "fusion_side_map", K, Q, sides, &s));
  return fusion_map(h, s, a, b, dout, ld_out);
}

// the operand forms: system 0 is this model's own matrix, re-scored slab by slab once per pass (operand_slabs.hip)
static int score_fusion_side_source(plda_handle *h, const char *fn, const double *dU, const int32_t *dn, int n_uniform, int64_t M,
                                    const double *dV, int64_t Nt, const double *dzmean, const double *dzstd, const int64_t *despk,
                                    const int64_t *dtspk, int Q, const plda_fusion_side *sides, const void *out, OperandSlabs *os,
                                    TrialSource *ts, FusionSource *s) {
  PLDA_TRY(fusion_side_source(h, fn, 1, Q, sides, s));
  PLDA_TRY(operand_source(h, fn, dU, dn, n_uniform, M, dV, Nt, dzmean, dzstd, despk, dtspk, out, os, ts));
  s->lists = false; s->M = M; s->Nt = Nt; s->espk = despk; s->tspk = dtspk; s->ld[0] = Nt; s->slabs = ts;
  return PLDA_OK;
}
int score_fusion_side_pass_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV,
                                  int64_t Nt, const double *dzmean, const double *dzstd, const int64_t *despk, const int64_t *dtspk, int Q,
                                  const plda_fusion_side *sides, const double *a, double c, double theta, plda_fusion_record *out) {
  if (!a) return fail(h, PLDA_E_INVAL, "score_fusion_side_pass: the weight array is NULL");
  OperandSlabs os;
  TrialSource ts;
  FusionSource s;
  PLDA_TRY(score_fusion_side_source(h, "score_fusion_side_pass", dU, dn, n_uniform, M, dV, Nt, dzmean, dzstd, despk, dtspk, Q, sides, out, &os, &ts, &s));
  return fusion_pass(h, s, a, c, theta, out);
}
int score_fusion_side_fit_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV,
                                 int64_t Nt, const double *dzmean, const double *dzstd, const int64_t *despk, const int64_t *dtspk, int Q,
                                 const plda_fusion_side *sides, double prior, double tol, int max_iter, plda_fusion_fit *out) {
  OperandSlabs os;
  TrialSource ts;
  FusionSource s;
  PLDA_TRY(score_fusion_side_source(h, "score_fusion_side_fit", dU, dn, n_uniform, M, dV, Nt, dzmean, dzstd, despk, dtspk, Q, sides, out, &os, &ts, &s));
  return fusion_fit(h, s, prior, tol, max_iter, out);
}

}  // namespace plda
