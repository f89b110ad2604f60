// plda_amd/csrc/cosine.hip -- the cosine back-end (K27): the operands of the trials GEMM from length-normalised rows, and
// trial lists, for a handle switched with plda_backend_set(h, PLDA_BACKEND_COSINE, D).
//
// The trials GEMM contracts two packed fp32 operand images plus a rank-2 bias, S_ij = A_i . B_j + r'_i 1 + s_i q_j
// (score.hip).  A cosine score is the same contraction with
//     B_jd = (float)(v_jd inv(v_j)),  q_j = 0,  cpair_j = (1, 0)
//     A_id = (float)((u_id inv(u_i)) (double)s_i),  s_i = (float)sc_i,  r'_i = (float)((0 - zmean_i) sc_i),  rpair_i = (r'_i, s_i)
//     ss(x) = sum_d x_d^2,  inv(x) = 1 / sqrt(ss(x)), 0 when ss(x) == 0 (a zero row scores 0, as in the embedding chain)
//     sc_i = 1 / zstd_i where statistics are given and zstd_i != 0; otherwise sc_i = 1 and r'_i = 0 (the row stays
//     un-normalised, as the PLDA preparation and the trial-list kernels leave it)
// all in fp64 up to the one rounding, so the matrix score is (cos - zmean) / zstd in the GEMM's own fp32 chain.  The GEMM
// kernels, their consumers and the layout of the buffers (k-quad planes of float4, Rpad rows, zero padding to Kg;
// prep_side_kernel of score.hip) are untouched: this file only fills them.
//
// The norm has to be known before anything is rounded, so a row is walked twice: once for ss (lane l adds the squares of
// d = l, l + 64, ... in increasing d, then the xor butterfly 32 ... 1 -- every lane holds the sum), once for the packed
// values.  The 4-rows-per-wave form keeps a row of up to 256 dimensions in registers between the walks (one memory round
// trip); every other case reads the row again, from L2 (a workgroup's rows are 16 or 64 x D x 8 bytes).  Whichever form
// runs, a row's packed bits are a function of the row and its own zstd alone: the same in the 16-row and the 64-row
// workgroup, alone or in any batch, one side per launch or both in one (tests).
// This file is built with -ffp-contract=off and holds no fused multiply-add: x * x + acc is a product, rounded, then a sum
// (tests/cosine_model.py is that arithmetic in NumPy).
//
// Non-finite input: a NaN makes ss, inv and with them every packed value of ITS row NaN; an infinity makes ss infinite,
// inv 0 and its own element inf * 0 = NaN -- the row's scores are NaN, no other row is touched.  A finite row whose sum of
// squares overflows or underflows fp64 (|x| beyond 1e154 / below 1e-162) scores 0 or NaN: out of the range of embeddings.
// Rows >= R and planes >= D are written as zeros, the bias pairs of rows >= R too.
//
// Launch shapes: those of the PLDA preparation -- 4 rows per wave (16-row workgroups) for sides of up to 32 768 padded rows,
// 16 above; both short sides in one launch; PLDA_PREP_VARIANT=2 / 3 force 16 / 4 (=1, the three-kernel arm of the PLDA
// preparation, has no counterpart here and is ignored).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; no instantiation uses scratch memory):
//   kernel                            VGPRs  SGPRs  scratch  LDS bytes  waves/SIMD
//   cosine_prep_side_kernel<0, 4>       104     48        0       8704           4
//   cosine_prep_side_kernel<1, 4>        82     42        0       8704           5
//   cosine_prep_side_kernel<0, 16>      256     86        0      33280           2
//   cosine_prep_side_kernel<1, 16>      176     68        0      33280           2
//   cosine_prep_both_kernel             104     54        0      17408           4
//   cosine_pairs_kernel                  24     26        0          0           8
#include "common.hpp"

#include <cmath>

namespace plda {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// 1 / sqrt(ss), 0 for a zero row (NaN stays NaN)
__host__ __device__ __forceinline__ double inv_norm(double ss) { return ss == 0.0 ? 0.0 : 1.0 / sqrt(ss); }

// One side of the operands, one workgroup of RPB = 4 RW rows (wave w owns rows w RW ... w RW + RW - 1), walking the row in
// chunks of 64 dimensions as prep_side_body of score.hip does: the fp32 values of a chunk go through a 64 x RPB LDS tile
// and leave as k-quad planes.  SIDE 0: enrol (A, r', s, rpair), SIDE 1: test (B, q = 0, cpair).
template <int SIDE, int RW>
__device__ __forceinline__ void cosine_prep_body(const int block, const double *__restrict__ X, int D, int64_t R, int64_t Rpad, int KQ,
                                                 const double *__restrict__ zmean, const double *__restrict__ zstd, float *__restrict__ P,
                                                 float *__restrict__ bias, float *__restrict__ rscale, float2 *__restrict__ pair) {
  constexpr int RPB = 4 * RW;
  __shared__ float tile[2][64][RPB + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)block * RPB;
  const int64_t wrow0 = row0 + wave * RW;
  const int nchunk = (KQ * 4 + 63) >> 6;
  const bool zn = SIDE == 0 && zmean && zstd;
  constexpr int KEEP = RW == 4 ? 4 : 1;            // chunks the 4-row form holds in registers between the two walks
  const bool keep = RW == 4 && nchunk <= KEEP;    // (uniform over the launch)

  auto fetch = [&](int c, double (&x)[RW]) {
    const int d = c * 64 + lane;
#pragma unroll
    for (int j = 0; j < RW; ++j) {
      const int64_t row = wrow0 + j;
      x[j] = (c < nchunk && d < D && row < R) ? X[row * (int64_t)D + d] : 0.0;
    }
  };
  double xk[KEEP][RW], acc[RW], sc[RW];
#pragma unroll
  for (int j = 0; j < RW; ++j) acc[j] = 0.0;
  // ---- first walk: the sums of squares (an absent element adds + 0 to a sum that is never negative: the identity)
  if (keep) {
#pragma unroll
    for (int c = 0; c < KEEP; ++c) fetch(c, xk[c]);
#pragma unroll
    for (int c = 0; c < KEEP; ++c)
#pragma unroll
      for (int j = 0; j < RW; ++j) acc[j] = acc[j] + xk[c][j] * xk[c][j];
  } else {
    double xc[RW], xn[RW];
    fetch(0, xn);
    for (int c = 0; c < nchunk; ++c) {
#pragma unroll
      for (int j = 0; j < RW; ++j) xc[j] = xn[j];
      if (c + 1 < nchunk) fetch(c + 1, xn);
#pragma unroll
      for (int j = 0; j < RW; ++j) acc[j] = acc[j] + xc[j] * xc[j];
    }
  }
  // ---- per row: inv (every lane), the z-norm scale and its fp32 rounding
  float sf[RW];
#pragma unroll
  for (int j = 0; j < RW; ++j) {
    double a = acc[j];
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    acc[j] = inv_norm(a);
    sc[j] = 1.0;
    if (zn && wrow0 + j < R) { const double sd = zstd[wrow0 + j]; if (sd != 0.0) sc[j] = 1.0 / sd; }
    sf[j] = (float)sc[j];
  }
  // ---- second walk: the packed values
  auto emit = [&](int c, const double (&x)[RW]) {
    const int d = c * 64 + lane;
    const bool dv = d < D;
    float(*const tl)[RPB + 1] = tile[c & 1];
#pragma unroll
    for (int j = 0; j < RW; ++j) {
      float val = 0.f;
      if (dv && wrow0 + j < R) {
        double v = x[j] * acc[j];
        if (SIDE == 0) v = v * (double)sf[j];
        val = (float)v;
      }
      tl[lane][wave * RW + j] = val;
    }
    __syncthreads();
    const int r = threadIdx.x % RPB;
#pragma unroll
    for (int pass = 0; pass < RPB / 16; ++pass) {
      const int q = threadIdx.x / RPB + pass * (256 / RPB);   // k-quad of the chunk, 0..15
      const int kq = c * 16 + q;
      if (kq < KQ) {
        f32x4 v;
        v.x = tl[4 * q + 0][r];
        v.y = tl[4 * q + 1][r];
        v.z = tl[4 * q + 2][r];
        v.w = tl[4 * q + 3][r];
        reinterpret_cast<f32x4 *>(P)[(int64_t)kq * Rpad + row0 + r] = v;
      }
    }
  };
  if (keep) {
#pragma unroll
    for (int c = 0; c < KEEP; ++c)
      if (c < nchunk) emit(c, xk[c]);
  } else {
    double xc[RW], xn[RW];
    fetch(0, xn);
    for (int c = 0; c < nchunk; ++c) {
#pragma unroll
      for (int j = 0; j < RW; ++j) xc[j] = xn[j];
      if (c + 1 < nchunk) fetch(c + 1, xn);
      emit(c, xc);
    }
  }
  // ---- biases and bias pairs (zeros beyond the side's rows)
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < RW; ++j) {
      const int64_t row = wrow0 + j;
      if (row >= Rpad) continue;
      const bool in = row < R;
      if (SIDE == 0) {
        float r = 0.f;
        if (zn && in && zstd[row] != 0.0) r = (float)((0.0 - zmean[row]) * sc[j]);
        bias[row] = r;
        rscale[row] = in ? sf[j] : 0.f;
        pair[row] = make_float2(r, in ? sf[j] : 0.f);
      } else {
        bias[row] = 0.f;
        pair[row] = make_float2(in ? 1.f : 0.f, 0.f);
      }
    }
  }
}

template <int SIDE, int RW>
__global__ __launch_bounds__(256) void cosine_prep_side_kernel(const double *__restrict__ X, int D, int64_t R, int64_t Rpad, int KQ,
                                                               const double *__restrict__ zmean, const double *__restrict__ zstd,
                                                               float *__restrict__ P, float *__restrict__ bias, float *__restrict__ rscale,
                                                               float2 *__restrict__ pair) {
  cosine_prep_body<SIDE, RW>((int)blockIdx.x, X, D, R, Rpad, KQ, zmean, zstd, P, bias, rscale, pair);
}
// both short sides in one launch: blocks [0, blocksA) the enrol side, the rest the test side
struct CosineSideArgs { const double *X; int64_t R, Rpad; float *P; float *bias; float2 *pair; };
__global__ __launch_bounds__(256) void cosine_prep_both_kernel(const CosineSideArgs a, const CosineSideArgs b, int blocksA, int D, int KQ,
                                                               const double *__restrict__ zmean, const double *__restrict__ zstd,
                                                               float *__restrict__ rscale) {
  if ((int)blockIdx.x < blocksA) cosine_prep_body<0, 4>((int)blockIdx.x, a.X, D, a.R, a.Rpad, KQ, zmean, zstd, a.P, a.bias, rscale, a.pair);
  else cosine_prep_body<1, 4>((int)blockIdx.x - blocksA, b.X, D, b.R, b.Rpad, KQ, nullptr, nullptr, b.P, b.bias, nullptr, b.pair);
}

int cosine_prepare_operands(plda_handle *h, const double *dU, int64_t M, const double *dV, int64_t Nt, const double *dzmean,
                            const double *dzstd, const TrialOperands &op, bool doA, bool doB) {
  const int D = h->Dout;
  float *Apk = h->s_Apk.as<float>(), *Bpk = h->s_Bpk.as<float>();
  const bool fewA = prep_few_rows(h, op.Mpad), fewB = prep_few_rows(h, op.Npad);
  if (doA && doB && fewA && fewB) {
    const CosineSideArgs a{dU, M, op.Mpad, Apk, h->s_rbias.as<float>(), h->s_rpair.as<float2>()};
    const CosineSideArgs b{dV, Nt, op.Npad, Bpk, h->s_cbias.as<float>(), h->s_cpair.as<float2>()};
    cosine_prep_both_kernel<<<(unsigned)((op.Mpad + op.Npad) / 16), 256, 0, h->stream>>>(a, b, (int)(op.Mpad / 16), D, op.KQ, dzmean, dzstd,
                                                                                        h->s_rscale.as<float>());
    PLDA_LAUNCH_CHECK(h);
    return PLDA_OK;
  }
  if (doA) {
    if (fewA)
      cosine_prep_side_kernel<0, 4><<<(unsigned)(op.Mpad / 16), 256, 0, h->stream>>>(dU, D, M, op.Mpad, op.KQ, dzmean, dzstd, Apk, h->s_rbias.as<float>(),
                                                                                   h->s_rscale.as<float>(), h->s_rpair.as<float2>());
    else
      cosine_prep_side_kernel<0, 16><<<(unsigned)(op.Mpad / 64), 256, 0, h->stream>>>(dU, D, M, op.Mpad, op.KQ, dzmean, dzstd, Apk, h->s_rbias.as<float>(),
                                                                                    h->s_rscale.as<float>(), h->s_rpair.as<float2>());
  }
  if (doB) {
    if (fewB)
      cosine_prep_side_kernel<1, 4><<<(unsigned)(op.Npad / 16), 256, 0, h->stream>>>(dV, D, Nt, op.Npad, op.KQ, nullptr, nullptr, Bpk, h->s_cbias.as<float>(),
                                                                                   nullptr, h->s_cpair.as<float2>());
    else
      cosine_prep_side_kernel<1, 16><<<(unsigned)(op.Npad / 64), 256, 0, h->stream>>>(dV, D, Nt, op.Npad, op.KQ, nullptr, nullptr, Bpk, h->s_cbias.as<float>(),
                                                                                    nullptr, h->s_cpair.as<float2>());
  }
  PLDA_LAUNCH_CHECK(h);
  return PLDA_OK;
}

// ------------------------------------------------------------------------------------
// trial list in fp64: one wave per (enrol, test) pair.  c = (sum_d u_d v_d) inv(u) inv(v), then the z-norm map where
// zstd_e != 0, as score_pairs_kernel applies it.  The three sums run lane-strided in increasing d, then the butterfly.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cosine_pairs_kernel(const double *__restrict__ U, const double *__restrict__ V,
                                                           const int64_t *__restrict__ e_idx, const int64_t *__restrict__ t_idx, int64_t P, int D,
                                                           const double *__restrict__ zmean, const double *__restrict__ zstd,
                                                           double *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (p >= P) return;
  const int64_t e = e_idx[p], t = t_idx[p];
  const double *u = U + e * (int64_t)D, *v = V + t * (int64_t)D;
  double dot = 0.0, su = 0.0, sv = 0.0;
  for (int d = lane; d < D; d += 64) {
    const double a = u[d], b = v[d];
    dot = dot + a * b;
    su = su + a * a;
    sv = sv + b * b;
  }
  for (int o = 32; o > 0; o >>= 1) {
    dot += __shfl_xor(dot, o);
    su += __shfl_xor(su, o);
    sv += __shfl_xor(sv, o);
  }
  if (lane == 0) {
    double s = (dot * inv_norm(su)) * inv_norm(sv);
    if (zmean && zstd && zstd[e] != 0.0) s = (s - zmean[e]) / zstd[e];
    out[p] = s;
  }
}

int cosine_pairs_device(plda_handle *h, const double *dU, const double *dV, const int64_t *de, const int64_t *dt, int64_t P,
                        const double *dzmean, const double *dzstd, double *dout) {
  const int wpb = 4;
  cosine_pairs_kernel<<<(unsigned)ceil_div(P, wpb), wpb * 64, 0, h->stream>>>(dU, dV, de, dt, P, h->Dout, dzmean, dzstd, dout);
  PLDA_LAUNCH_CHECK(h);
  return PLDA_OK;
}

double cosine_one_host(const double *u, const double *v, int D, bool has_z, double zmean, double zstd) {
  double dot = 0.0, su = 0.0, sv = 0.0;
  for (int d = 0; d < D; ++d) {
    dot = dot + u[d] * v[d];
    su = su + u[d] * u[d];
    sv = sv + v[d] * v[d];
  }
  double s = (dot * inv_norm(su)) * inv_norm(sv);
  if (has_z && zstd != 0.0) s = (s - zmean) / zstd;
  return s;
}

}  // namespace plda
