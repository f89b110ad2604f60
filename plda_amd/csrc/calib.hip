// plda_amd/csrc/calib.hip -- linear score calibration, Cllr and actual DCF of a labelled trials matrix on the GPU
// (include/plda_hip.h, "linear score calibration"; the reference stops at the EER, scoring/eer.py:68-73, so the definition
// is the project's own and is pinned by tests/calibration_model.py).
//
// One CALIBRATION PASS at (a, c, theta) reads every fp32 score once and returns one plda_calib_record: per class the six
// fp64 sums L, G0, G1, H0, H1, H2 of y = a * (double)s + c, the exact counts (targets, non-targets, misses and false alarms
// at the raw-score threshold theta, non-finite scores) and the fp32 extremes.  Objective, gradient and Hessian of the
// prior-weighted logistic regression, Cllr and actDCF are all read off that record on the host, so the damped Newton fit is a
// host loop over "take a pass" and every source -- matrix, two lists, operands scored slab by slab -- shares it.
//
// Sources: a pass consumes a TrialSource through for_each_piece (trial_source.hpp), as the EER and minDCF passes do; the
// operand forms get theirs from operand_source (operand_slabs.hip).  This file is its own translation unit.
//
// Kernels.  calib_pass_strip_kernel walks the matrix exactly as eer_hist_strip_kernel does (eer.hip: a workgroup owns 1024
// columns, 4 per thread with their speaker ids in registers, and a slice of the rows; 16-byte loads where ld and the base
// allow).  Per element, all fp64: one fma, exp(-|y|), log1p, ONE divide r = 1 / (1 + e) (p and 1 - p are r and e r, w = e r r),
// then the six non-target terms go through selects into per-thread accumulators (no branch), and the target side -- a 2e-4
// share of a 100k x 100k matrix at 20 utterances per speaker -- runs only in waves that hold a target (wave-uniform ballot).
// A wave reduces its 12 sums by DPP (wave_sum_f64), the four waves of a block are added in a fixed order, the block writes
// ONE partial record into handle scratch, and calib_reduce_kernel (one block) adds the partials in a fixed order.  No
// floating-point atomics and no integer ones either: the record of a call is bit-identical from run to run and does not
// depend on which CU ran which block.  The grid is a function of the shape alone (not tunable).
//
// Cost (profiles/calibration_*.json, scripts/calibration_bench.py; box at 2.34 GHz): 61.4 ms per pass over 100k x 100k =
// 6.1 ps per trial, 6.3 x plda_eer_matrix_dev on the same matrix (9.7 ms, the labelled read alone) and 28.5 x faster than the
// same record through stock torch fp64 operations over 2-GiB slabs (1752 ms); 4096 x 4096: 0.19 ms.  The pass is bound by
// VALU ISSUE, not by HBM (profiles/calibration_pmc_100000x100000.json, a counter run of its own): FETCH_SIZE, doubled as a
// wide streaming read must be on gfx950, is 40.0 GB = the matrix once; SQ_INSTS_VALU = 3.46e10 per launch = 221 VALU
// instructions per trial (exp and log1p are software routines, the divide a Newton iteration), nearly all fp64 at >= 4 issue
// cycles per wave: 1.38e11 of the 1.47e11 SIMD-cycles of the launch.  Twice the estimate made before the first measurement
// (2 - 3 x the read time); a cheaper per-element form (a mixed-precision arm, a shared exp / log1p argument reduction) is
// the next step, not part of this version.
//
// Newton (calib_fit): start (a, b) = (0, 0); d = -H^-1 g by a 2 x 2 Cholesky, lambda2 = g' H^-1 g; stop at lambda2 <= tol or
// after max_iter iterations; backtracking t = 1, 1/2, ... (30 halvings) until F(x + t d) <= F(x) - 1e-4 t lambda2 + eps |F(x)|,
// eps = 2^-44: the allowance is the rounding of F itself (the sums are held to a per-term error of 8.4e-14, see the header) --
// without it the last step before convergence, whose gain is below F's resolution, is rejected at random and costs 30
// passes.  tol: the host model's lambda2 floor on Gaussian score sets of 3e3 .. 1e6 trials, scaled and shifted, is 1e-26 ..
// 1e-33 (the sequence ends ... 1e-10, 1e-18, 1e-33: quadratic), so the default 1e-18 is above the floor by eight orders and
// was kept.
#include "trial_source.hpp"

#include <algorithm>
#include <cmath>

namespace plda {

typedef float f32x4c __attribute__((ext_vector_type(4)));
constexpr int CALIB_STRIP = 1024;          // columns per workgroup (4 per thread), as EER_STRIP
constexpr int CALIB_MAX_BLOCKS = 256 * 16;

struct CalibAcc {
  double n[6] = {0, 0, 0, 0, 0, 0}, t[6] = {0, 0, 0, 0, 0, 0};
  unsigned long long np = 0, nn = 0, miss = 0, fa = 0, bad = 0;
  float min_t = INFINITY, max_t = -INFINITY, min_n = INFINITY, max_n = -INFINITY;
};

__device__ __forceinline__ void calib_account(CalibAcc &A, float sf, bool tgt, double a, double c, double theta) {
  const double s = (double)sf;
  const double y = fma(a, s, c);
  const double e = exp(-fabs(y));
  const double l = log1p(e);
  const double r = 1.0 / (1.0 + e);
  const double q = e * r;                    // sigmoid(-|y|)
  const double w = q * r;                    // p (1 - p)
  const bool pos = y >= 0.0;
  const double p = pos ? r : q;              // sigmoid(y)
  const double ws = w * s, wss = ws * s;
  {
    const double L = fmax(y, 0.0) + l;       // softplus(y)
    A.n[0] += tgt ? 0.0 : L;
    A.n[1] += tgt ? 0.0 : p;
    A.n[2] += tgt ? 0.0 : p * s;
    A.n[3] += tgt ? 0.0 : w;
    A.n[4] += tgt ? 0.0 : ws;
    A.n[5] += tgt ? 0.0 : wss;
  }
  if (__builtin_amdgcn_ballot_w64(tgt)) {    // wave-uniform: most waves of a large matrix hold no target
    const double L = fmax(-y, 0.0) + l;      // softplus(-y)
    const double m = pos ? q : r;            // 1 - sigmoid(y)
    A.t[0] += tgt ? L : 0.0;
    A.t[1] += tgt ? m : 0.0;
    A.t[2] += tgt ? m * s : 0.0;
    A.t[3] += tgt ? w : 0.0;
    A.t[4] += tgt ? ws : 0.0;
    A.t[5] += tgt ? wss : 0.0;
    A.min_t = tgt ? fminf(A.min_t, sf) : A.min_t;
    A.max_t = tgt ? fmaxf(A.max_t, sf) : A.max_t;
  }
  A.min_n = tgt ? A.min_n : fminf(A.min_n, sf);
  A.max_n = tgt ? A.max_n : fmaxf(A.max_n, sf);
  A.np += tgt ? 1u : 0u;
  A.nn += tgt ? 0u : 1u;
  A.miss += (tgt && s < theta) ? 1u : 0u;
  A.fa += (!tgt && s >= theta) ? 1u : 0u;
  A.bad += ((__float_as_uint(sf) & 0x7f800000u) == 0x7f800000u) ? 1u : 0u;
}

// block (256 threads) -> one record, every addition in a fixed order
__device__ __forceinline__ void calib_block_store(const CalibAcc &A, plda_calib_record *__restrict__ dst) {
  __shared__ plda_calib_record red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double sums[12];
#pragma unroll
  for (int k = 0; k < 6; ++k) { sums[k] = wave_sum_f64(A.n[k]); sums[6 + k] = wave_sum_f64(A.t[k]); }
  unsigned long long cnt[5] = {A.np, A.nn, A.miss, A.fa, A.bad};
  float lo_t = A.min_t, hi_t = A.max_t, lo_n = A.min_n, hi_n = A.max_n;
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 5; ++k) cnt[k] += __shfl_xor(cnt[k], o);
    lo_t = fminf(lo_t, __shfl_xor(lo_t, o)); hi_t = fmaxf(hi_t, __shfl_xor(hi_t, o));
    lo_n = fminf(lo_n, __shfl_xor(lo_n, o)); hi_n = fmaxf(hi_n, __shfl_xor(hi_n, o));
  }
  if (lane == 0) {
    plda_calib_record &r = red[wave];
#pragma unroll
    for (int k = 0; k < 6; ++k) { r.sum[0][k] = sums[k]; r.sum[1][k] = sums[6 + k]; }
    r.np = cnt[0]; r.nn = cnt[1]; r.miss = cnt[2]; r.fa = cnt[3]; r.nonfinite = cnt[4];
    r.min_t = lo_t; r.max_t = hi_t; r.min_n = lo_n; r.max_n = hi_n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    plda_calib_record o;
    for (int cl = 0; cl < 2; ++cl)
      for (int k = 0; k < 6; ++k) o.sum[cl][k] = (red[0].sum[cl][k] + red[1].sum[cl][k]) + (red[2].sum[cl][k] + red[3].sum[cl][k]);
    o.np = red[0].np + red[1].np + red[2].np + red[3].np;
    o.nn = red[0].nn + red[1].nn + red[2].nn + red[3].nn;
    o.miss = red[0].miss + red[1].miss + red[2].miss + red[3].miss;
    o.fa = red[0].fa + red[1].fa + red[2].fa + red[3].fa;
    o.nonfinite = red[0].nonfinite + red[1].nonfinite + red[2].nonfinite + red[3].nonfinite;
    o.min_t = fminf(fminf(red[0].min_t, red[1].min_t), fminf(red[2].min_t, red[3].min_t));
    o.max_t = fmaxf(fmaxf(red[0].max_t, red[1].max_t), fmaxf(red[2].max_t, red[3].max_t));
    o.min_n = fminf(fminf(red[0].min_n, red[1].min_n), fminf(red[2].min_n, red[3].min_n));
    o.max_n = fmaxf(fmaxf(red[0].max_n, red[1].max_n), fmaxf(red[2].max_n, red[3].max_n));
    *dst = o;
  }
}

// The labelled matrix pass: block b writes part[b].  Traversal and labelling of eer_hist_strip_kernel.
__global__ __launch_bounds__(256) void calib_pass_strip_kernel(const float *__restrict__ scores, int64_t ld, int64_t M, int64_t Nt,
                                                               const int64_t *__restrict__ espk, const int64_t *__restrict__ tspk,
                                                               int64_t rows_per_wg, double a, double c, double theta,
                                                               plda_calib_record *__restrict__ part) {
  const int64_t strips = (Nt + CALIB_STRIP - 1) / CALIB_STRIP;
  const int64_t strip = blockIdx.x % strips, slice = blockIdx.x / strips;
  const int64_t col = strip * CALIB_STRIP + (int64_t)threadIdx.x * 4;
  const int64_t r0 = slice * rows_per_wg, r1 = (r0 + rows_per_wg < M) ? r0 + rows_per_wg : M;
  int64_t ts[4];
  bool ok[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    ok[e] = col + e < Nt;
    ts[e] = ok[e] ? tspk[col + e] : 0;
  }
  const bool vec = ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(scores) & 15) == 0) && ok[3];
  CalibAcc A;
  for (int64_t row = r0; row < r1; row += 4) {
    float v[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (row + u >= r1) break;
      const float *src = scores + (row + u) * ld + col;
      if (vec) {
        const f32x4c x = __builtin_nontemporal_load(reinterpret_cast<const f32x4c *>(src));
        v[u][0] = x.x; v[u][1] = x.y; v[u][2] = x.z; v[u][3] = x.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[u][e] = ok[e] ? src[e] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (row + u >= r1) break;
      const int64_t spk = espk[row + u];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (ok[e]) calib_account(A, v[u][e], ts[e] == spk, a, c, theta);
    }
  }
  calib_block_store(A, part + blockIdx.x);
}

// One flat score array of a fixed class (the list form calls it once per class).
__global__ __launch_bounds__(256) void calib_pass_list_kernel(const float *__restrict__ scores, int64_t n, int fixed_class, double a,
                                                              double c, double theta, plda_calib_record *__restrict__ part) {
  CalibAcc A;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx - threadIdx.x < n; idx += (int64_t)gridDim.x * 256)
    if (idx < n) calib_account(A, scores[idx], fixed_class != 0, a, c, theta);
  calib_block_store(A, part + blockIdx.x);
}

// part[0 .. n) -> *out: thread t adds the partials t, t + 256, ... in ascending order, then the block's fixed tree
__global__ __launch_bounds__(256) void calib_reduce_kernel(const plda_calib_record *__restrict__ part, int64_t n,
                                                           plda_calib_record *__restrict__ out) {
  CalibAcc A;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const plda_calib_record &r = part[i];
#pragma unroll
    for (int k = 0; k < 6; ++k) { A.n[k] += r.sum[0][k]; A.t[k] += r.sum[1][k]; }
    A.np += r.np; A.nn += r.nn; A.miss += r.miss; A.fa += r.fa; A.bad += r.nonfinite;
    A.min_t = fminf(A.min_t, r.min_t); A.max_t = fmaxf(A.max_t, r.max_t);
    A.min_n = fminf(A.min_n, r.min_n); A.max_n = fmaxf(A.max_n, r.max_n);
  }
  calib_block_store(A, out);
}

// out[i, j] = (float)fma(a, (double)s[i, j], b): strips of 1024 columns, rows dealt out over gridDim.y; in place allowed (an
// element is read and written by the same thread); columns [Nt, ld_out) are not touched
__global__ __launch_bounds__(256) void affine_map_kernel(const float *scores, int64_t ld, int64_t M, int64_t Nt, double a, double b,
                                                         float *out, int64_t ld_out) {
  const int64_t col = (int64_t)blockIdx.x * CALIB_STRIP + (int64_t)threadIdx.x * 4;
  if (col >= Nt) return;
  const bool vec = ((ld & 3) == 0) && ((ld_out & 3) == 0) && ((reinterpret_cast<uintptr_t>(scores) & 15) == 0) &&
                   ((reinterpret_cast<uintptr_t>(out) & 15) == 0) && col + 3 < Nt;
  for (int64_t row = blockIdx.y; row < M; row += gridDim.y) {
    const float *src = scores + row * ld + col;
    float *dst = out + row * ld_out + col;
    if (vec) {
      const f32x4c x = *reinterpret_cast<const f32x4c *>(src);
      f32x4c y;
      y.x = (float)fma(a, (double)x.x, b); y.y = (float)fma(a, (double)x.y, b);
      y.z = (float)fma(a, (double)x.z, b); y.w = (float)fma(a, (double)x.w, b);
      *reinterpret_cast<f32x4c *>(dst) = y;
    } else {
      for (int e = 0; e < 4 && col + e < Nt; ++e) dst[e] = (float)fma(a, (double)src[e], b);
    }
  }
}

// ------------------------------------------------------------------------------------ host drivers
static int64_t strip_blocks(int64_t rows, int64_t Nt, int64_t *rows_per_wg) {
  const int64_t strips = ceil_div(Nt, (int64_t)CALIB_STRIP);
  const int64_t slices = std::max<int64_t>(1, std::min<int64_t>(rows, CALIB_MAX_BLOCKS / strips));
  *rows_per_wg = ceil_div(rows, slices);
  return strips * ceil_div(rows, *rows_per_wg);
}
static int64_t list_blocks(int64_t n) { return std::min<int64_t>(ceil_div(n, 256), CALIB_MAX_BLOCKS); }

// One pass over `src` -> *rec (host); synchronises the stream.  A non-finite score, or a class without trials, is
// PLDA_E_INVAL (the record is written all the same).
static int calib_pass(plda_handle *h, const TrialSource &src, double a, double c, double theta, plda_calib_record *rec) {
  int64_t rpw = 0;
  auto blocks_of = [&](const TrialPiece &pc) { return pc.cls < 0 ? strip_blocks(pc.rows, pc.Nt, &rpw) : list_blocks(pc.Nt); };
  // the partials of every piece, in the order of the walk: sized from the extents before anything is launched
  int64_t total = 0, at = 0;
  PLDA_TRY(for_each_piece(src, [&](const TrialPiece &pc) -> int { total += blocks_of(pc); return PLDA_OK; }, /*produce=*/false));
  if (total > (int64_t)0x7fffffff) return fail(h, PLDA_E_CAPACITY, "calib: too many column strips");
  PLDA_HIP(h, h->calib_part.reserve((size_t)(total + 1) * sizeof(plda_calib_record)));
  plda_calib_record *part = h->calib_part.as<plda_calib_record>();
  PLDA_TRY(for_each_piece(src, [&](const TrialPiece &pc) -> int {
    const int64_t blocks = blocks_of(pc);
    if (pc.cls < 0)
      calib_pass_strip_kernel<<<(unsigned)blocks, 256, 0, h->stream>>>(pc.scores, pc.ld, pc.rows, pc.Nt, pc.espk, src.tspk, rpw, a, c, theta, part + at);
    else
      calib_pass_list_kernel<<<(unsigned)blocks, 256, 0, h->stream>>>(pc.scores, pc.Nt, pc.cls, a, c, theta, part + at);
    PLDA_LAUNCH_CHECK(h);
    at += blocks;
    return PLDA_OK;
  }));
  calib_reduce_kernel<<<1, 256, 0, h->stream>>>(part, at, part + total);
  PLDA_LAUNCH_CHECK(h);
  PLDA_HIP(h, hipMemcpyAsync(rec, part + total, sizeof(*rec), hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  if (rec->nonfinite) return fail(h, PLDA_E_INVAL, "calib: %llu non-finite scores", (unsigned long long)rec->nonfinite);
  if (rec->np == 0 || rec->nn == 0) return fail(h, PLDA_E_INVAL, "calib: need at least one target and one non-target trial");
  return PLDA_OK;
}

struct CalibModel { double F, g[2], H[3]; };      // H: aa, ab, bb
static CalibModel calib_model(const plda_calib_record &r, double prior) {
  const double wt = prior / (double)r.np, wn = (1.0 - prior) / (double)r.nn;
  CalibModel m;
  m.F = wt * r.sum[1][0] + wn * r.sum[0][0];
  m.g[0] = -wt * r.sum[1][2] + wn * r.sum[0][2];
  m.g[1] = -wt * r.sum[1][1] + wn * r.sum[0][1];
  m.H[0] = wt * r.sum[1][5] + wn * r.sum[0][5];
  m.H[1] = wt * r.sum[1][4] + wn * r.sum[0][4];
  m.H[2] = wt * r.sum[1][3] + wn * r.sum[0][3];
  return m;
}
// H d = -g by Cholesky, lambda2 = g' H^-1 g; false when H is not positive definite in fp64
static bool calib_solve(const CalibModel &m, double d[2], double *lambda2) {
  if (!(m.H[0] > 0.0)) return false;
  const double l00 = std::sqrt(m.H[0]), l10 = m.H[1] / l00, s = m.H[2] - l10 * l10;
  if (!(s > 0.0)) return false;
  const double l11 = std::sqrt(s);
  const double z0 = m.g[0] / l00, z1 = (m.g[1] - l10 * z0) / l11;
  const double x1 = z1 / l11, x0 = (z0 - l10 * x1) / l00;
  d[0] = -x0; d[1] = -x1;
  *lambda2 = z0 * z0 + z1 * z1;
  return true;
}

static int calib_fit(plda_handle *h, const TrialSource &src, double prior, double tol, int max_iter, plda_calib_fit *out) {
  if (!out || !(prior > 0.0 && prior < 1.0) || !(tol >= 0.0)) return fail(h, PLDA_E_INVAL, "calib_fit: bad argument (prior must lie inside (0, 1), tol >= 0)");
  if (tol == 0.0) tol = 1e-18;
  if (max_iter <= 0) max_iter = 100;
  const double tau = std::log(prior / (1.0 - prior)), ln2 = std::log(2.0);
  plda_calib_record before, rec, trial;
  int passes = 0;
  auto take = [&](double a, double c, plda_calib_record *rec) { return calib_pass(h, src, a, c, 0.0, rec); };
  PLDA_TRY(take(1.0, 0.0, &before)); ++passes;
  if (std::min(before.min_t, before.min_n) == std::max(before.max_t, before.max_n))
    return fail(h, PLDA_E_INVAL, "calib_fit: all scores are equal (the Hessian is singular)");
  double a = 0.0, b = 0.0, lam2 = INFINITY;
  PLDA_TRY(take(a, b + tau, &rec)); ++passes;
  int it = 0;
  bool converged = false;
  for (;;) {
    const CalibModel m = calib_model(rec, prior);
    double d[2];
    if (!calib_solve(m, d, &lam2)) return fail(h, PLDA_E_INVAL, "calib_fit: the Hessian is not positive definite");
    if (lam2 <= tol) { converged = true; break; }
    if (it >= max_iter) break;
    double t = 1.0, na = a, nb = b;
    bool accepted = false;
    for (int k = 0; k <= 30; ++k, t *= 0.5) {
      na = a + t * d[0]; nb = b + t * d[1];
      PLDA_TRY(take(na, nb + tau, &trial)); ++passes;
      if (calib_model(trial, prior).F <= m.F - 1e-4 * t * lam2 + 0x1p-44 * std::fabs(m.F)) { accepted = true; break; }
    }
    if (!accepted) break;
    a = na; b = nb; rec = trial; ++it;
  }
  plda_calib_record after = rec;
  if (prior != 0.5) { PLDA_TRY(take(a, b, &after)); ++passes; }
  out->a = a; out->b = b;
  out->objective = calib_model(rec, prior).F / ln2;
  out->cllr_before = calib_model(before, 0.5).F / ln2;
  out->cllr_after = calib_model(after, 0.5).F / ln2;
  out->lambda2 = lam2;
  out->iterations = it; out->passes = passes; out->converged = converged ? 1 : 0;
  out->separable = before.min_t > before.max_n ? 1 : 0;
  return PLDA_OK;
}

static bool matrix_args_ok(const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *despk, const int64_t *dtspk) {
  return dscores && despk && dtspk && M > 0 && Nt > 0 && ld >= Nt;
}

int calib_pass_matrix_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *despk,
                             const int64_t *dtspk, double a, double c, double theta, plda_calib_record *out) {
  if (!out || !matrix_args_ok(dscores, ld, M, Nt, despk, dtspk)) return fail(h, PLDA_E_INVAL, "calib_pass: bad argument");
  return calib_pass(h, TrialSource::matrix(dscores, ld, M, Nt, despk, dtspk), a, c, theta, out);
}
int calib_fit_matrix_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *despk,
                            const int64_t *dtspk, double prior, double tol, int max_iter, plda_calib_fit *out) {
  if (!out || !matrix_args_ok(dscores, ld, M, Nt, despk, dtspk)) return fail(h, PLDA_E_INVAL, "calib_fit: bad argument");
  return calib_fit(h, TrialSource::matrix(dscores, ld, M, Nt, despk, dtspk), prior, tol, max_iter, out);
}
int calib_pass_lists_device(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, double a, double c,
                            double theta, plda_calib_record *out) {
  if (!dpos || !dneg || !out || np <= 0 || nn <= 0) return fail(h, PLDA_E_INVAL, "calib_pass: need at least one target and one non-target score");
  return calib_pass(h, TrialSource::lists(dpos, np, dneg, nn), a, c, theta, out);
}
int calib_fit_lists_device(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, double prior, double tol,
                           int max_iter, plda_calib_fit *out) {
  if (!dpos || !dneg || !out || np <= 0 || nn <= 0) return fail(h, PLDA_E_INVAL, "calib_fit: need at least one target and one non-target score");
  return calib_fit(h, TrialSource::lists(dpos, np, dneg, nn), prior, tol, max_iter, out);
}

// the operand forms: the slabs are re-scored once per pass (operand_slabs.hip), consumed and dropped
int score_calib_pass_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV, int64_t Nt,
                            const double *dzmean, const double *dzstd, const int64_t *despk, const int64_t *dtspk, double a, double c,
                            double theta, plda_calib_record *out) {
  OperandSlabs os;
  TrialSource s;
  PLDA_TRY(operand_source(h, "score_calib", dU, dn, n_uniform, M, dV, Nt, dzmean, dzstd, despk, dtspk, out, &os, &s));
  return calib_pass(h, s, a, c, theta, out);
}
int score_calib_fit_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV, int64_t Nt,
                           const double *dzmean, const double *dzstd, const int64_t *despk, const int64_t *dtspk, double prior,
                           double tol, int max_iter, plda_calib_fit *out) {
  OperandSlabs os;
  TrialSource s;
  PLDA_TRY(operand_source(h, "score_calib", dU, dn, n_uniform, M, dV, Nt, dzmean, dzstd, despk, dtspk, out, &os, &s));
  return calib_fit(h, s, prior, tol, max_iter, out);
}

int affine_map_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, double a, double b, float *dout,
                      int64_t ld_out) {
  if (!dscores || !dout || M <= 0 || Nt <= 0 || ld < Nt || ld_out < Nt) return fail(h, PLDA_E_INVAL, "affine_map: bad argument");
  if (ceil_div(Nt, (int64_t)CALIB_STRIP) > (int64_t)0x7fffffff) return fail(h, PLDA_E_CAPACITY, "affine_map: too many column strips");
  const dim3 grid((unsigned)ceil_div(Nt, (int64_t)CALIB_STRIP), (unsigned)std::min<int64_t>(M, 4096));
  affine_map_kernel<<<grid, 256, 0, h->stream>>>(dscores, ld, M, Nt, a, b, dout, ld_out);
  PLDA_LAUNCH_CHECK(h);
  return PLDA_OK;
}

}  // namespace plda
