// plda_amd/csrc/vbx.hip -- VBx resegmentation: a batched variational-Bayes HMM over the segment sequence of every recording,
// with the PLDA model in its diagonalised space as the emission model, initialised from the clustering's labels (DESIGN.md K16;
// Landini et al., "Bayesian HMM clustering of x-vector sequences (VBx)", 2022; the contract is in include/plda_hip.h, the
// host model in tests/vbx_model.py).
//
// A recording is a chain of dependent steps (2 T per iteration, up to max_iters iterations) and many recordings are
// independent: one workgroup of 8 waves per recording, persistent over the iterations -- the stop test is taken inside the
// kernel, uniform over the workgroup, and the host does not synchronise between iterations.
//
//   vbx_check_kernel   the non-finite values of y, the labels outside [0, 64), the bad entries of Phi (three integer counters;
//                      a call that meets one fails and the kernels behind it write nothing) and S = 1 + max label per recording
//                      (plda_vbx_top2: + labels2 and post2, the second speaker of every segment, selected where the arg-max is)
//   vbx_kernel         <HBM = false> the per-recording state (b, a / gamma, beta, c, m, G, alpha, invL, sqrt Phi, Phi) in LDS;
//                      <HBM = true>  the same arrays in handle scratch.  pi, N and the reduction slots are in LDS in both.
//
// One iteration: (1) N[s], the row pass below; (2) sum_t gamma rho, invL, alpha: one thread per (s, d); (3) the two d-sums per
// speaker, one wave per speaker; (4) lp, m and b = exp(lp - m) for ALL t, the row pass; (5) THE CHAIN: wave 0 runs the forward
// recursion while wave 1 runs the backward one, one lane per speaker, the other waves wait at the barrier; (6) gamma, the
// pi update, sum ln c + sum m, the row pass; (7) the ELBO and the stop test.
//
// The chain holds a multiply-add, one wave reduction (DPP and readlane: wave_sum_f64, no LDS) and one division per step; no exp,
// no log, and every row of b is loaded PF steps before its use (PF = 4 from LDS, 8 from HBM: at 12 and 16 the HBM form spills
// 36 and 84 bytes per lane).  So that the two recursions can run at the same time the backward one does not wait for c_{t+1}: it scales by its own sum, bh_t = (P w + (1 - P) sum_j pi_j
// w_j) / sum_j w_j with w = b_{t+1} bh_{t+1}, which is beta_t times a factor that does not depend on s.  As sum_s a_t beta_t = 1,
// gamma_t = a_t bh_t / z_t with z_t = sum_s a_t bh_t, and b_t beta_t / c_t = b_t bh_t / (z_t c_t) in the pi update.
//
// The row pass: a row t takes SP = the power of two >= S lanes, so a wave holds 64 / SP rows; reductions over s are xor
// butterflies inside the SP lanes, sums over t are per-lane partials over the rows a lane meets (t ascending), combined over
// the wave's rows by butterflies, over the waves in wave order.  Every sum so has an order fixed by (T, S, D) alone: nothing
// depends on the grid, on the grouping into launches or on the run, and there are no floating-point atomics.
//
// The two small fp64 GEMMs (sum_t gamma rho and rho alpha^T, 2 T S D flop each) run on the VECTOR ALU, not on the fp64 matrix
// cores: S is the M or N extent and is typically 3 .. 16, so a 16 x 16 x 4 MFMA tile would be mostly padding; the fixed
// summation order falls out of a plain loop; and the chain, not these products, bounds a recording.  UNMEASURED against an
// MFMA form.
//
// Barriers: only __syncthreads() (barrier and fence in one); the file has no raw s_barrier.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): see the table at vbx_kernel.
#include "common.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <limits>
#include <vector>

namespace plda {

namespace {

constexpr int VBX_T = 512, VBX_W = VBX_T / 64;
constexpr int VBX_MAX_SPK = PLDA_VBX_MAX_SPK;
constexpr int VBX_MAX_D = 4096;
constexpr int VBX_LDS_BYTES = 160 * 1024;      // one workgroup may hold all of a CU's LDS
constexpr int VBX_FIXED_BYTES = 8192;          // pi, N, the reduction slots and the scalars (static LDS; asserted in the kernel)
constexpr long long VBX_LDS_DOUBLES = (VBX_LDS_BYTES - VBX_FIXED_BYTES) / 8;
static_assert(VBX_MAX_SPK == 64, "one lane per speaker");

// one recording of a launch (host-built, uploaded once per enqueue)
struct VbxRec {
  long long off;     // first row (y, labels)
  long long scr;     // HBM class: first double of the state in scratch
  long long goff;    // first double of gamma's interval
  long long poff;    // first double of pi's interval
  int T, S, r, pad;
};

struct VbxPar { double Fa, Fb, P, esig, eps; int max_iters, D; };

__host__ __device__ constexpr long long vbx_dp(long long D) { return D | 1; }   // row stride of alpha / invL: odd, for the LDS banks
__host__ __device__ constexpr long long vbx_state_doubles(long long T, long long S, long long D) {
  return 3 * T * S + 3 * T + 2 * S * vbx_dp(D) + 2 * D;
}

__device__ __forceinline__ bool vbx_finite(double x) { return (__double2hiint(x) & 0x7ff00000) != 0x7ff00000; }

// grid (pieces, recordings)
__global__ __launch_bounds__(256) void vbx_check_kernel(const double *__restrict__ Y, int D, const double *__restrict__ Phi,
                                                        const int *__restrict__ lab, const VbxRec *__restrict__ tab,
                                                        unsigned long long *stat, int *Sout) {
  const VbxRec rc = tab[blockIdx.y];
  const long long total = (long long)rc.T * D;
  const double *__restrict__ y = Y + rc.off * D;
  unsigned bad_y = 0, bad_l = 0, bad_p = 0;
  int mx = -1;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256)
    if (!vbx_finite(y[e])) ++bad_y;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < rc.T; t += gridDim.x * 256) {
    const int l = lab[rc.off + t];
    if (l < 0 || l >= VBX_MAX_SPK) ++bad_l; else mx = max(mx, l);
  }
  if (blockIdx.x == 0 && blockIdx.y == 0)
    for (int d = threadIdx.x; d < D; d += 256) {
      const double p = Phi[d];
      if (!vbx_finite(p) || p < 0.0) ++bad_p;
    }
  // rare, integer: one atomic per lane that met one
  if (bad_y) atomicAdd(stat + 0, (unsigned long long)bad_y);
  if (bad_l) atomicAdd(stat + 1, (unsigned long long)bad_l);
  if (bad_p) atomicAdd(stat + 2, (unsigned long long)bad_p);
  if (mx >= 0) atomicMax(Sout + rc.r, mx + 1);
}

// sum / maximum over the SP lanes of a row: every lane of the row ends with the same bits
__device__ __forceinline__ double vbx_row_sum(double x, int SP) {
  for (int o = 1; o < SP; o <<= 1) x += __shfl_xor(x, o);
  return x;
}
__device__ __forceinline__ double vbx_row_max(double x, int SP) {
  for (int o = 1; o < SP; o <<= 1) x = fmax(x, __shfl_xor(x, o));
  return x;
}
// the per-lane partials of a row pass: over the rows of the wave, then over the waves in wave order -> out[s], s < S
// (part: VBX_W x 64 doubles; two barriers inside, so every thread of the workgroup must call it)
__device__ __forceinline__ void vbx_combine(double x, int SP, int S, int lane, int wave, int tid, double *part, double *out) {
  for (int o = SP; o < 64; o <<= 1) x += __shfl_xor(x, o);
  if (lane < SP) part[wave * 64 + lane] = x;
  __syncthreads();
  if (tid < S) {
    double s = part[tid];
#pragma unroll
    for (int w = 1; w < VBX_W; ++w) s += part[w * 64 + tid];
    out[tid] = s;
  }
  __syncthreads();
}

// Resource report of the two instantiations (gfx950, -O3, 512 threads: 256 VGPRs per lane are there).  Neither uses scratch
// memory; the scalar registers the unrolled chain overflows are kept in VGPR lanes, not in memory:
//   vbx_kernel<false>   VGPRs 160   SGPRs 106 (110 spilled to VGPR lanes)   ScratchSize 0   LDS 7760 static + the state
//   vbx_kernel<true>    VGPRs 211   SGPRs 106 (165 spilled to VGPR lanes)   ScratchSize 0   LDS 7760 static
// (with the second-speaker pass of K21; without it the SGPR spills were 107 and 160, the VGPRs the same)
template <bool HBM>
__global__ __launch_bounds__(VBX_T) void vbx_kernel(const double *__restrict__ Y, const double *__restrict__ Phi,
                                                    const int *__restrict__ lab_in, const VbxRec *__restrict__ tab, double *scratch,
                                                    const unsigned long long *__restrict__ stat, const VbxPar par,
                                                    int *__restrict__ labels, int *__restrict__ n_clusters, double *__restrict__ gamma_out,
                                                    double *__restrict__ pi_out, double *__restrict__ elbo_out, int *__restrict__ iters_out,
                                                    int *__restrict__ labels2, double *__restrict__ post2) {
  extern __shared__ double vbx_smem[];
  __shared__ double pi[64], Ns[64], qs[64], es[64], g0[64], acc[64];
  __shared__ double part[VBX_W * 64];
  __shared__ double red[VBX_W];
  __shared__ double sc_elbo[2];
  __shared__ int first[64], rank[64];
  __shared__ int sc_stop, sc_k;
  static_assert(sizeof(double) * (6 * 64 + VBX_W * 64 + VBX_W + 2) + sizeof(int) * (2 * 64 + 2) <= VBX_FIXED_BYTES, "static LDS");
  if (stat[0] | stat[1] | stat[2]) return;
  constexpr int PF = HBM ? 8 : 4;
  const VbxRec rc = tab[blockIdx.x];
  const int T = rc.T, S = rc.S, D = par.D, Dp = (int)vbx_dp(D);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double P = par.P, Fa = par.Fa, FaFb = par.Fa / par.Fb, omP = 1.0 - par.P;

  double *st;
  if constexpr (HBM) st = scratch + rc.scr; else st = vbx_smem;
  double *B = st;                         // [T, S]  b
  double *A = B + (long long)T * S;       // [T, S]  gamma, a during the chain
  double *BE = A + (long long)T * S;      // [T, S]  the backward variable at its own scale
  double *cc = BE + (long long)T * S;     // [T]
  double *mm = cc + T;                    // [T]
  double *GG = mm + T;                    // [T]
  double *alpha = GG + T;                 // [S, Dp]
  double *invL = alpha + (long long)S * Dp;
  double *sq = invL + (long long)S * Dp;  // [D] sqrt(Phi)
  double *ph = sq + D;                    // [D]
  const double *__restrict__ y = Y + rc.off * D;
  const int *__restrict__ l0 = lab_in + rc.off;

  // the row pass's geometry
  int SP = 1, lg = 0;
  while (SP < S) { SP <<= 1; ++lg; }
  const int GR = 64 >> lg, sub = lane >> lg, s = lane & (SP - 1);
  const bool act = s < S;
  const int sc = act ? s : 0;             // an in-range column for the loads of idle lanes

  // ---- constants of the recording, initial gamma and pi
  for (int d = tid; d < D; d += VBX_T) { const double p = Phi[d]; ph[d] = p; sq[d] = sqrt(p); }
  for (int t = wave; t < T; t += VBX_W) {
    double q = 0.0;
    for (int d = lane; d < D; d += 64) { const double v = y[(long long)t * D + d]; q += v * v; }
    q = wave_sum_f64(q);
    if (lane == 0) GG[t] = -0.5 * (q + (double)D * 1.8378770664093454835606594728112);   // ln 2 pi
  }
  {
    const double den = par.esig + (double)(S - 1), hi = par.esig / den, lo = 1.0 / den;
    for (int e = tid; e < T * S; e += VBX_T) { const int t = e / S, c = e - t * S; A[e] = l0[t] == c ? hi : lo; }
  }
  if (tid < 64) { pi[tid] = tid < S ? 1.0 / (double)S : 0.0; first[tid] = INT_MAX; }
  if (tid == 0) { sc_stop = 0; sc_elbo[0] = 0.0; }
  __syncthreads();

  int it = 0;
  for (;; ++it) {
    // (1) N[s]
    {
      double n = 0.0;
      for (int tb = wave * GR; tb < T; tb += VBX_W * GR) {
        const int t = tb + sub;
        if (t < T && act) n += A[t * S + s];
      }
      vbx_combine(n, SP, S, lane, wave, tid, part, Ns);
    }
    // (2) sum_t gamma[t, s] rho[t, d] in four interleaved partials (t mod 4), invL, alpha
    for (int e = tid; e < S * D; e += VBX_T) {
      const int c = e / D, d = e - c * D;
      const double sd = sq[d];
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
      int t = 0;
      for (; t + 3 < T; t += 4) {
        a0 += A[t * S + c] * (y[(long long)t * D + d] * sd);
        a1 += A[(t + 1) * S + c] * (y[(long long)(t + 1) * D + d] * sd);
        a2 += A[(t + 2) * S + c] * (y[(long long)(t + 2) * D + d] * sd);
        a3 += A[(t + 3) * S + c] * (y[(long long)(t + 3) * D + d] * sd);
      }
      for (; t < T; ++t) a0 += A[t * S + c] * (y[(long long)t * D + d] * sd);
      const double sum = (a0 + a1) + (a2 + a3);
      const double il = 1.0 / (1.0 + FaFb * Ns[c] * ph[d]);
      invL[c * Dp + d] = il;
      alpha[c * Dp + d] = FaFb * il * sum;
    }
    __syncthreads();
    // (3) per speaker: q = 1/2 sum_d (invL + alpha^2) Phi, e = sum_d (ln invL - invL - alpha^2 + 1)
    for (int c = wave; c < S; c += VBX_W) {
      double q = 0.0, e = 0.0;
      for (int d = lane; d < D; d += 64) {
        const double il = invL[c * Dp + d], al = alpha[c * Dp + d];
        q += (il + al * al) * ph[d];
        e += log(il) - il - al * al + 1.0;
      }
      q = wave_sum_f64(q);
      e = wave_sum_f64(e);
      if (lane == 0) { qs[c] = 0.5 * q; es[c] = e; }
    }
    __syncthreads();
    // (4) lp, m, b for every t
    for (int tb = wave * GR; tb < T; tb += VBX_W * GR) {
      const int t = tb + sub, tt = t < T ? t : T - 1;
      const double *__restrict__ yr = y + (long long)tt * D;
      const double *al = alpha + sc * Dp;
      double d0 = 0.0, d1 = 0.0;
      int d = 0;
      for (; d + 1 < D; d += 2) {
        d0 += (yr[d] * sq[d]) * al[d];
        d1 += (yr[d + 1] * sq[d + 1]) * al[d + 1];
      }
      if (d < D) d0 += (yr[d] * sq[d]) * al[d];
      const double lp = Fa * ((d0 + d1) - qs[sc] + GG[tt]);
      const double m = vbx_row_max(act ? lp : -INFINITY, SP);
      if (t < T && act) B[t * S + s] = exp(lp - m);
      if (t < T && s == 0) mm[t] = m;
    }
    __syncthreads();
    // (5) the chain: forward on wave 0, backward on wave 1, one lane per speaker
    if (wave == 0) {
      const bool on = lane < S;
      const int ls = on ? lane : 0;
      const double pis = on ? pi[lane] : 0.0, q1 = omP * pis;
      double nb[PF], a = 0.0;
#pragma unroll
      for (int j = 0; j < PF; ++j) nb[j] = (on && j < T) ? B[j * S + ls] : 0.0;
      for (int t0 = 0; t0 < T; t0 += PF) {
        double cur[PF];
#pragma unroll
        for (int j = 0; j < PF; ++j) {
          cur[j] = nb[j];
          const int tn = t0 + PF + j;
          nb[j] = (on && tn < T) ? B[tn * S + ls] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < PF; ++j) {
          const int t = t0 + j;
          if (t < T) {                     // (uniform)
            const double u = cur[j] * (t == 0 ? pis : P * a + q1);
            const double c = wave_sum_f64(u);
            a = u / c;
            if (on) A[t * S + lane] = a;
            if (lane == 0) cc[t] = c;
          }
        }
      }
    } else if (wave == 1) {
      const bool on = lane < S;
      const int ls = on ? lane : 0;
      const double pis = on ? pi[lane] : 0.0;
      double bh = on ? 1.0 : 0.0;
      if (on) BE[(T - 1) * S + lane] = 1.0;
      double nb[PF];
#pragma unroll
      for (int j = 0; j < PF; ++j) { const int tn = T - 1 - j; nb[j] = (on && tn >= 1) ? B[tn * S + ls] : 0.0; }
      for (int t0 = T - 2; t0 >= 0; t0 -= PF) {
        double cur[PF];
#pragma unroll
        for (int j = 0; j < PF; ++j) {
          cur[j] = nb[j];                  // b of row t0 - j + 1
          const int tn = t0 - j + 1 - PF;
          nb[j] = (on && tn >= 1) ? B[tn * S + ls] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < PF; ++j) {
          const int t = t0 - j;
          if (t >= 0) {                    // (uniform)
            const double w = cur[j] * bh;
            const double sw = wave_sum_f64(pis * w), e = wave_sum_f64(w);
            bh = on ? (P * w + omP * sw) / e : 0.0;
            if (on) BE[t * S + lane] = bh;
          }
        }
      }
    }
    __syncthreads();
    // (6) gamma, the pi update's sums, sum_t (ln c + m)
    {
      double ps = 0.0, ls = 0.0;
      for (int tb = wave * GR; tb < T; tb += VBX_W * GR) {
        const int t = tb + sub, tt = t < T ? t : T - 1;
        const bool on = t < T && act;
        const double bh = BE[tt * S + sc];
        const double g = on ? A[tt * S + sc] * bh : 0.0;
        const double z = vbx_row_sum(g, SP);
        const double c = cc[tt];
        if (on) {
          const double gm = g / z;
          A[t * S + s] = gm;
          if (t == 0) g0[s] = gm; else ps += B[t * S + s] * bh / (z * c);
          if (s == 0) ls += log(c) + mm[t];
        }
      }
      vbx_combine(ps, SP, S, lane, wave, tid, part, acc);
      ls = wave_sum_f64(ls);
      if (lane == 0) red[wave] = ls;
      __syncthreads();
    }
    // (7) pi, the ELBO, the stop test (thread 0 decides, everybody reads the decision)
    double pn = 0.0;
    if (tid < 64) {
      double tot = 0.0;
      for (int c = 0; c < S; ++c) tot += g0[c] + omP * pi[c] * acc[c];
      pn = tid < S ? (g0[tid] + omP * pi[tid] * acc[tid]) / tot : 0.0;
    }
    if (tid == 0) {
      double L = red[0];
#pragma unroll
      for (int w = 1; w < VBX_W; ++w) L += red[w];
      double e = 0.0;
      for (int c = 0; c < S; ++c) e += es[c];
      const double elbo = L + 0.5 * par.Fb * e;
      if (elbo_out) elbo_out[(long long)rc.r * par.max_iters + it] = elbo;
      const bool stop = (it >= 1 && elbo - sc_elbo[0] < par.eps) || it + 1 >= par.max_iters;
      sc_elbo[0] = elbo;
      sc_stop = stop ? 1 : 0;
    }
    __syncthreads();
    if (tid < 64) pi[tid] = pn;
    const int stop = sc_stop;
    __syncthreads();
    if (stop) break;
  }
  const int iters = it + 1;

  // ---- outputs: argmax_s gamma (ties: the smallest s), renumbered by ascending smallest member
  int *lab = labels + rc.off;
  for (int tb = wave * GR; tb < T; tb += VBX_W * GR) {
    const int t = tb + sub, tt = t < T ? t : T - 1;
    double v = act ? A[tt * S + sc] : -INFINITY;
    int bi = act ? s : INT_MAX;
    for (int o = 1; o < SP; o <<= 1) {
      const double ov = __shfl_xor(v, o);
      const int oi = __shfl_xor(bi, o);
      if (oi != INT_MAX && (bi == INT_MAX || ov > v || (ov == v && oi < bi))) { v = ov; bi = oi; }
    }
    if (bi == INT_MAX) bi = 0;             // (a row of NaN: speaker 0)
    if (t < T && s == 0) { lab[t] = bi; atomicMin(&first[bi], t); }
  }
  __syncthreads();
  if (tid < 64) {
    const int f = first[tid];
    int r = 0, k = 0;
    for (int c = 0; c < 64; ++c) { const int fc = first[c]; k += fc != INT_MAX; r += fc < f; }
    rank[tid] = r;
    if (tid == 0) sc_k = k;
  }
  __syncthreads();
  // the second speaker (plda_vbx_top2): the same butterfly over the speakers that are somebody's first choice, the row's own
  // first left out; lab still holds the first choice in the initial numbering.  No candidate (k = 1): -1 and posterior 0
  if (labels2 || post2) {
    for (int tb = wave * GR; tb < T; tb += VBX_W * GR) {
      const int t = tb + sub, tt = t < T ? t : T - 1;
      const bool cand = act && s != lab[tt] && first[s] != INT_MAX;
      double v = cand ? A[tt * S + sc] : -INFINITY;
      int bi = cand ? s : INT_MAX;
      for (int o = 1; o < SP; o <<= 1) {
        const double ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(bi, o);
        if (oi != INT_MAX && (bi == INT_MAX || ov > v || (ov == v && oi < bi))) { v = ov; bi = oi; }
      }
      if (t < T && s == 0) {
        if (labels2) labels2[rc.off + t] = bi == INT_MAX ? -1 : rank[bi];
        if (post2) post2[rc.off + t] = bi == INT_MAX ? 0.0 : v;
      }
    }
    __syncthreads();                       // (every row has read its first choice before lab is renumbered)
  }
  for (int t = tid; t < T; t += VBX_T) lab[t] = rank[lab[t]];
  if (tid == 0) { n_clusters[rc.r] = sc_k; if (iters_out) iters_out[rc.r] = iters; }
  if (gamma_out)
    for (int e = tid; e < T * S; e += VBX_T) gamma_out[rc.goff + e] = A[e];
  if (pi_out && tid < S) pi_out[rc.poff + tid] = pi[tid];
  if (elbo_out)
    for (int i = iters + tid; i < par.max_iters; i += VBX_T) elbo_out[(long long)rc.r * par.max_iters + i] = __longlong_as_double(0x7ff8000000000000ll);
}

template <bool HBM> int vbx_attr(plda_handle *h) {
  static DeviceOnce attr;
  if (attr.needed(h->device)) {
    PLDA_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&vbx_kernel<HBM>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    VBX_LDS_BYTES - VBX_FIXED_BYTES));
    attr.done(h->device);
  }
  return PLDA_OK;
}

int64_t vbx_budget(const plda_handle *h) { return h->vbx_scratch_bytes > 0 ? h->vbx_scratch_bytes : (int64_t)1 << 30; }

__global__ void vbx_add_offset_kernel(double *__restrict__ out, long long total, int D, const double *__restrict__ off) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < total) out[e] += off[e % D];
}

}  // namespace

int vbx_plan(plda_handle *h, int64_t T, int64_t S, int64_t D, int32_t *out) {
  if (!out) return fail(h, PLDA_E_INVAL, "vbx_plan: out is NULL");
  if (T < 1 || T > PLDA_AHC_MAX) return fail(h, PLDA_E_INVAL, "vbx_plan: T = %lld (must be 1 ... PLDA_AHC_MAX = %d)", (long long)T, PLDA_AHC_MAX);
  if (S < 1 || S > VBX_MAX_SPK) return fail(h, PLDA_E_INVAL, "vbx_plan: S = %lld (must be 1 ... PLDA_VBX_MAX_SPK = %d)", (long long)S, VBX_MAX_SPK);
  if (D < 1 || D > VBX_MAX_D) return fail(h, PLDA_E_INVAL, "vbx_plan: D = %lld (must be 1 ... %d)", (long long)D, VBX_MAX_D);
  const long long n = vbx_state_doubles(T, S, D);
  const bool hbm = n > VBX_LDS_DOUBLES;
  out[0] = hbm ? 1 : 0;
  out[1] = hbm ? (int32_t)(n * 8) : 0;
  out[2] = (int32_t)VBX_LDS_DOUBLES;
  return PLDA_OK;
}

int vbx_validate(plda_handle *h, const char *fn, int64_t D, const int64_t *offsets, int64_t R, double Fa, double Fb, double loop_prob,
                 int64_t max_iters, const void *labels, const void *n_clusters, const void *gamma, const int64_t *gamma_off,
                 const void *pi, const int64_t *pi_off) {
  if (R < 1 || R > (int64_t)0x7fffffff) return fail(h, PLDA_E_INVAL, "%s: R = %lld (must be 1 ... 2^31 - 1)", fn, (long long)R);
  if (D < 1 || D > VBX_MAX_D) return fail(h, PLDA_E_INVAL, "%s: D = %lld (must be 1 ... %d)", fn, (long long)D, VBX_MAX_D);
  if (!offsets) return fail(h, PLDA_E_INVAL, "%s: offsets is NULL", fn);
  if (!labels) return fail(h, PLDA_E_INVAL, "%s: labels is NULL", fn);
  if (!n_clusters) return fail(h, PLDA_E_INVAL, "%s: n_clusters is NULL", fn);
  if (!(Fa > 0.0) || !std::isfinite(Fa)) return fail(h, PLDA_E_INVAL, "%s: Fa = %g (must be > 0)", fn, Fa);
  if (!(Fb > 0.0) || !std::isfinite(Fb)) return fail(h, PLDA_E_INVAL, "%s: Fb = %g (must be > 0)", fn, Fb);
  if (!(loop_prob >= 0.0 && loop_prob < 1.0)) return fail(h, PLDA_E_INVAL, "%s: loop_prob = %g (must be in [0, 1))", fn, loop_prob);
  if (max_iters < 1 || max_iters > (1 << 20)) return fail(h, PLDA_E_INVAL, "%s: max_iters = %lld (must be >= 1)", fn, (long long)max_iters);
  if ((gamma != nullptr) != (gamma_off != nullptr)) return fail(h, PLDA_E_INVAL, "%s: gamma and gamma_off must be given together", fn);
  if ((pi != nullptr) != (pi_off != nullptr)) return fail(h, PLDA_E_INVAL, "%s: pi and pi_off must be given together", fn);
  PLDA_TRY(check_recordings(h, fn, offsets, R, PLDA_AHC_MAX, "PLDA_AHC_MAX"));
  if (gamma_off && gamma_off[0] < 0) return fail(h, PLDA_E_INVAL, "%s: gamma_off[0] = %lld (must be >= 0)", fn, (long long)gamma_off[0]);
  if (pi_off && pi_off[0] < 0) return fail(h, PLDA_E_INVAL, "%s: pi_off[0] = %lld (must be >= 0)", fn, (long long)pi_off[0]);
  return PLDA_OK;
}

int vbx_device(plda_handle *h, const double *dY, int64_t D64, const double *dPhi, const int32_t *dlabels_in, const int64_t *offsets,
               int64_t R, double Fa, double Fb, double loop_prob, double init_smoothing, int64_t max_iters, double epsilon,
               int32_t *dlabels, int32_t *dn_clusters, double *dgamma, const int64_t *gamma_off, double *dpi, const int64_t *pi_off,
               double *delbo, int32_t *diters, int32_t *dlabels2, double *dpost2) {
  const char *fn = "vbx";
  if (!h->fitted) return fail(h, PLDA_E_NOT_FITTED, "%s: model not fitted", fn);
  if (!dY) return fail(h, PLDA_E_INVAL, "%s: Y is NULL", fn);
  if (!dlabels_in) return fail(h, PLDA_E_INVAL, "%s: labels_in is NULL", fn);
  PLDA_TRY(vbx_validate(h, fn, D64, offsets, R, Fa, Fb, loop_prob, max_iters, dlabels, dn_clusters, dgamma, gamma_off, dpi, pi_off));
  const int D = (int)D64;
  if (!dPhi) {
    if (D != h->Dout) return fail(h, PLDA_E_INVAL, "%s: D = %d, the model's psi has %d entries (Phi is NULL)", fn, D, h->Dout);
    dPhi = h->d_psi.as<double>();
  }
  // pass 1: the device-side checks and S of every recording
  std::vector<VbxRec> tab((size_t)R);
  int tmax = 0;
  for (int64_t r = 0; r < R; ++r) {
    VbxRec &rc = tab[(size_t)r];
    rc.off = offsets[r]; rc.scr = 0; rc.goff = 0; rc.poff = 0; rc.T = (int)(offsets[r + 1] - offsets[r]); rc.S = 0; rc.r = (int)r; rc.pad = 0;
    tmax = std::max(tmax, rc.T);
  }
  const size_t stat_bytes = 32 + (size_t)R * 4;
  PLDA_HIP(h, h->vbx_stat.reserve(stat_bytes));
  PLDA_HIP(h, h->vbx_tab.reserve(tab.size() * sizeof(VbxRec)));
  PLDA_HIP(h, hipMemsetAsync(h->vbx_stat.p, 0, stat_bytes, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(h->vbx_tab.p, tab.data(), tab.size() * sizeof(VbxRec), hipMemcpyHostToDevice, h->stream));
  VbxRec *dtab = h->vbx_tab.as<VbxRec>();
  unsigned long long *dstat = h->vbx_stat.as<unsigned long long>();
  int *dS = reinterpret_cast<int *>(dstat + 4);
  {
    TraceScope ts(h, "vbx.check");
    const int64_t pieces = std::max<int64_t>(1, std::min<int64_t>(ceil_div((int64_t)tmax * D, 256 * 16), 256));
    for (int64_t c0 = 0; c0 < R; c0 += 32768) {
      const int64_t c = std::min<int64_t>(32768, R - c0);
      vbx_check_kernel<<<dim3((unsigned)pieces, (unsigned)c), 256, 0, h->stream>>>(dY, D, dPhi, dlabels_in, dtab + c0, dstat, dS);
      PLDA_LAUNCH_CHECK(h);
    }
  }
  std::vector<unsigned char> hstat(stat_bytes);
  PLDA_HIP(h, hipMemcpyAsync(hstat.data(), h->vbx_stat.p, stat_bytes, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  const unsigned long long *bad = reinterpret_cast<const unsigned long long *>(hstat.data());
  const int *hS = reinterpret_cast<const int *>(hstat.data() + 32);
  if (bad[0]) return fail(h, PLDA_E_INVAL, "%s: %llu non-finite values in y", fn, bad[0]);
  if (bad[1]) return fail(h, PLDA_E_INVAL, "%s: %llu labels outside [0, PLDA_VBX_MAX_SPK = %d)", fn, bad[1], VBX_MAX_SPK);
  if (bad[2]) return fail(h, PLDA_E_INVAL, "%s: %llu entries of Phi negative or non-finite", fn, bad[2]);
  for (int64_t r = 0; r < R; ++r) {
    VbxRec &rc = tab[(size_t)r];
    rc.S = hS[r];
    const int64_t need = (int64_t)rc.T * rc.S;
    if (gamma_off) {
      if (gamma_off[r + 1] - gamma_off[r] < need)
        return fail(h, PLDA_E_INVAL, "%s: gamma interval %lld holds %lld doubles, its recording needs %d x %d", fn, (long long)r,
                    (long long)(gamma_off[r + 1] - gamma_off[r]), rc.T, rc.S);
      rc.goff = gamma_off[r];
    }
    if (pi_off) {
      if (pi_off[r + 1] - pi_off[r] < rc.S)
        return fail(h, PLDA_E_INVAL, "%s: pi interval %lld holds %lld doubles, its recording needs %d", fn, (long long)r,
                    (long long)(pi_off[r + 1] - pi_off[r]), rc.S);
      rc.poff = pi_off[r];
    }
  }
  // pass 2: the launches -- the LDS class by the size of its state, the HBM class under the scratch budget
  struct Launch { int64_t first, count; size_t lds; bool hbm; };
  std::vector<Launch> launches;
  std::vector<VbxRec> lt;
  lt.reserve((size_t)R);
  static const long long bucket_top[] = {2048, 4096, 8192, VBX_LDS_DOUBLES};     // doubles of state
  long long lo = 0;
  for (long long hi : bucket_top) {
    Launch L{(int64_t)lt.size(), 0, 0, false};
    for (const VbxRec &rc : tab) {
      const long long n = vbx_state_doubles(rc.T, rc.S, D);
      if (n > lo && n <= hi) {
        if (L.count >= 32768) { launches.push_back(L); L = Launch{(int64_t)lt.size(), 0, 0, false}; }
        lt.push_back(rc); ++L.count; L.lds = std::max(L.lds, (size_t)n * 8);
      }
    }
    if (L.count) launches.push_back(L);
    lo = hi;
  }
  const int64_t budget = vbx_budget(h);
  int64_t scratch_need = 0;
  {
    Launch L{(int64_t)lt.size(), 0, 0, true};
    int64_t used = 0;
    for (const VbxRec &rc0 : tab) {
      const long long n = vbx_state_doubles(rc0.T, rc0.S, D);
      if (n <= VBX_LDS_DOUBLES) continue;
      const int64_t bytes = round_up(n * 8, 256);
      if (L.count && (used + bytes > budget || L.count >= 32768)) {
        launches.push_back(L);
        L = Launch{(int64_t)lt.size(), 0, 0, true};
        used = 0;
      }
      VbxRec rc = rc0;
      rc.scr = used / 8;
      lt.push_back(rc);
      ++L.count; used += bytes;
      scratch_need = std::max(scratch_need, used);
    }
    if (L.count) launches.push_back(L);
  }
  if (scratch_need) PLDA_HIP(h, h->vbx_scratch.reserve((size_t)scratch_need));
  PLDA_HIP(h, hipMemcpyAsync(h->vbx_tab.p, lt.data(), lt.size() * sizeof(VbxRec), hipMemcpyHostToDevice, h->stream));
  PLDA_TRY(vbx_attr<false>(h));
  PLDA_TRY(vbx_attr<true>(h));
  const VbxPar par{Fa, Fb, loop_prob, std::exp(init_smoothing), epsilon, (int)max_iters, D};
  {
    TraceScope ts(h, "vbx.iterate");
    for (const Launch &L : launches) {
      if (L.hbm)
        vbx_kernel<true><<<(unsigned)L.count, VBX_T, 0, h->stream>>>(dY, dPhi, dlabels_in, dtab + L.first, h->vbx_scratch.as<double>(), dstat, par,
                                                                    dlabels, dn_clusters, dgamma, dpi, delbo, diters, dlabels2, dpost2);
      else
        vbx_kernel<false><<<(unsigned)L.count, VBX_T, L.lds, h->stream>>>(dY, dPhi, dlabels_in, dtab + L.first, nullptr, dstat, par, dlabels,
                                                                         dn_clusters, dgamma, dpi, delbo, diters, dlabels2, dpost2);
      PLDA_LAUNCH_CHECK(h);
    }
  }
  PLDA_HIP(h, hipStreamSynchronize(h->stream));      // (the launch table's host copy lives until here)
  return PLDA_OK;
}

// out [R, Dout] = X [R, Din] transform^T + offset: TransformIvector without its normalisation factor
int project_rows_device(plda_handle *h, const double *dX, int64_t R, int Din, double *dout) {
  if (!h->fitted) return fail(h, PLDA_E_NOT_FITTED, "project_rows: model not fitted");
  if (Din != h->Din) return fail(h, PLDA_E_INVAL, "project_rows: feature dim %d != model dim %d", Din, h->Din);
  if (R < 0) return fail(h, PLDA_E_INVAL, "project_rows: R = %lld", (long long)R);
  if (R == 0) return PLDA_OK;
  if (!dX || !dout) return fail(h, PLDA_E_INVAL, "project_rows: bad argument");
  TraceScope ts(h, "project_rows.gemm", 2.0 * (double)R * h->Dout * Din, 1);
  PLDA_TRY(gemm_f64(h, R, h->Dout, Din, 1.0, dX, Din, 1, h->d_transform.as<double>(), 1, Din, nullptr, 0.0, dout, h->Dout));
  const long long total = (long long)R * h->Dout;
  vbx_add_offset_kernel<<<(unsigned)ceil_div(total, 256), 256, 0, h->stream>>>(dout, total, h->Dout, h->d_offset.as<double>());
  PLDA_LAUNCH_CHECK(h);
  return PLDA_OK;
}

}  // namespace plda
