// plda_amd/csrc/adapt.hip -- PLDA domain adaptation (K14; include/plda_hip.h, "PLDA domain adaptation"): the one-read
// statistics pass about a pilot, the unsupervised update (Kaldi's PldaUnsupervisedAdaptor restated, parity unpinned) and the
// interpolation of two models.  The reference has no counterpart (pldamodule.cpp:29 is the `Plda` being adapted).
//
// The heavy lifting is the existing fp64 machinery of linalg.hip, called through its entry points only: syrk_f64 (the fit's
// weighted statistics product) on slabs of centred, augmented rows, gemm_f64, spd_inverse_blocked, sym_eig_dc_f64 /
// sym_eig_f64 and simdiag_enqueue.  The kernels here are element-wise or one-workgroup reductions (__syncthreads only), and
// nothing is accumulated with floating-point atomics: a call's record is bit-identical from run to run.
#include "common.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace plda {

namespace {

constexpr int64_t AD_SLAB_BYTES = (int64_t)64 << 20;   // default slab: 64 MiB of centred rows ...
constexpr int64_t AD_SLAB_MAX_ROWS = 65536;            // ... and at most this many rows

// One slab of the statistics pass: rows [r0, r0 + R) of X [., D] -> S [R, ld] = [x - p | 1 | 0 (pad)], one wave per row.
// bad[0] counts the rows with a non-finite element, bad[1] the negative or non-finite weights (integer atomics: exact).
__global__ __launch_bounds__(256) void adapt_centre_kernel(const double *__restrict__ X, const double *__restrict__ w,
                                                           const double *__restrict__ p, int64_t R, int D, int ld,
                                                           double *__restrict__ S, int *__restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;                       // (whole waves leave together: no barrier follows)
  const double *x = X + r * D;
  double *s = S + r * ld;
  int nonfinite = 0;
  for (int c = lane; c < ld; c += 64) {
    double v = 0.0;
    if (c < D) {
      const double xv = x[c];
      nonfinite |= !isfinite(xv);
      v = xv - p[c];
    } else if (c == D) {
      v = 1.0;
    }
    s[c] = v;
  }
  const bool any_bad = __any(nonfinite);
  if (lane == 0) {
    if (any_bad) atomicAdd(&bad[0], 1);
    if (w) {
      const double wv = w[r];
      if (!(wv >= 0.0) || !isfinite(wv)) atomicAdd(&bad[1], 1);
    }
  }
}

// rec += acc, element by element, unless the call rejected a row (then the record stays as it was); out_tw = rec's tw after
__global__ void adapt_fold_kernel(double *__restrict__ rec, const double *__restrict__ acc, int64_t n, const int *__restrict__ bad,
                                  double *__restrict__ out_tw) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool ok = !bad || (bad[0] == 0 && bad[1] == 0);
  const double v = ok ? rec[i] + acc[i] : rec[i];
  rec[i] = v;
  if (i == n - 1 && out_tw) *out_tw = v;
}

// delta = S1 / tw, mean' = p + delta, scal[0] = tw, scal[1] = ||delta||_2 (one workgroup, fixed-order tree)
__global__ __launch_bounds__(256) void adapt_mean_kernel(const double *__restrict__ rec, const double *__restrict__ p, int D,
                                                         double *__restrict__ delta, double *__restrict__ mean_out,
                                                         double *__restrict__ scal) {
  __shared__ double red[256];
  const int Da = D + 1;
  const double tw = rec[(size_t)D * Da + D];
  double acc = 0.0;
  for (int c = threadIdx.x; c < D; c += 256) {
    const double d = rec[(size_t)c * Da + D] / tw;
    delta[c] = d;
    mean_out[c] = p[c] + d;
    acc += d * d;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) { scal[0] = tw; scal[1] = sqrt(red[0]); }
}

// V = S2 / tw - (1 - mds) delta delta^T
__global__ void adapt_var_kernel(const double *__restrict__ rec, const double *__restrict__ delta, int D, double one_minus_mds,
                                 double *__restrict__ V) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)D * D) return;
  const int i = (int)(idx / D), j = (int)(idx % D);
  const int Da = D + 1;
  const double tw = rec[(size_t)D * Da + D];
  V[idx] = rec[(size_t)i * Da + j] / tw - one_minus_mds * (delta[i] * delta[j]);
}

// out[i][j] = in[i][j] * f(v[i]) (ROWS) or * f(v[j]) (columns); mode 0: sqrt(v), 1: sqrt(1 + v), 2: 1 / sqrt(1 + v)
__global__ void adapt_scale_kernel(const double *__restrict__ in, const double *__restrict__ v, int D, int by_row, int mode,
                                   double *__restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)D * D) return;
  const double x = v[by_row ? idx / D : idx % D];
  const double f = mode == 0 ? sqrt(x) : (mode == 1 ? sqrt(1.0 + x) : 1.0 / sqrt(1.0 + x));
  out[idx] = in[idx] * f;
}

// e_i = max(s_i - 1, 0); scal[2] = number of s_i > 1, scal[3] = s_0, scal[4] = s_{D-1} (s is sorted descending)
__global__ __launch_bounds__(256) void adapt_excess_kernel(const double *__restrict__ s, int D, double *__restrict__ e,
                                                           double *__restrict__ scal) {
  __shared__ int red[256];
  int cnt = 0;
  for (int c = threadIdx.x; c < D; c += 256) {
    const double v = s[c];
    e[c] = fmax(v - 1.0, 0.0);
    cnt += v > 1.0 ? 1 : 0;
  }
  red[threadIdx.x] = cnt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) { scal[2] = (double)red[0]; scal[3] = s[0]; scal[4] = s[D - 1]; }
}

// lower triangle <- mean of the two mirror elements, written to both (the matrices handed to the diagonalisation)
__global__ void adapt_symmetrize_kernel(double *__restrict__ G, int D) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)D * D) return;
  const int i = (int)(idx / D), j = (int)(idx % D);
  if (j < i) {
    const double v = 0.5 * (G[(size_t)i * D + j] + G[(size_t)j * D + i]);
    G[(size_t)i * D + j] = v;
    G[(size_t)j * D + i] = v;
  }
}

// out = a x + b y (out may be x)
__global__ void adapt_axpby_kernel(int64_t n, double a, const double *x, double b, const double *__restrict__ y, double *out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a * x[i] + b * y[i];
}

// the status words of the chain next to the staged model: f[0] SPD inverse(s), f[1] the update's eigensolver, f[2] / f[3] the
// diagonalisation's Cholesky flag and eigensolver status.  A nullptr chol / eig reads as `chol_absent` / `eig_absent`: 0 when
// the diagonalisation checked the word on the host already, 8 ("not handled", as sym_eig_dc_status reports it) when the
// deferred direct eigensolver left no flag behind because the device refused its launch
__global__ void adapt_flags_kernel(const int *__restrict__ own, const int *__restrict__ chol, const int *__restrict__ eig,
                                   int chol_absent, int eig_absent, int *__restrict__ f) {
  f[0] = own[0];
  f[1] = own[1];
  f[2] = chol ? *chol : chol_absent;
  f[3] = eig ? *eig : eig_absent;
}

inline unsigned blocks(int64_t n) { return (unsigned)ceil_div(n, 256); }

constexpr int AD_DMAX = 2048;   // the direct eigensolver's limit (block Jacobi, the second attempt, stops at 1024)

int supported_dim(plda_handle *h, const char *what) {
  if (h->Din > AD_DMAX)
    return fail(h, PLDA_E_INVAL, "%s: model dimension %d; update and blend are supported up to D = %d", what, h->Din, AD_DMAX);
  return PLDA_OK;
}

int square_model(plda_handle *h, const char *what) {
  if (!h->fitted) return fail(h, PLDA_E_NOT_FITTED, "%s: model not fitted", what);
  if (h->Dout != h->Din)
    return fail(h, PLDA_E_INVAL, "%s: the model is truncated (transform %d x %d) and has no covariances; adapt before truncating",
                what, h->Dout, h->Din);
  return PLDA_OK;
}

// The matrices of an update / blend inside h->ad_work (DD = D * D doubles each) and the staged result behind them:
// out = [mean' (D) | T' (DD) | psi' (D) | s (D) | scal (8) | flags (4 ints)], copied to the host in one piece.
struct Work {
  size_t DD;
  double *W, *B, *Tinv, *tmp, *G, *P, *F, *Tm, *W2, *B2, *scr, *vec, *out;
  int *own;
  double *o_mean, *o_T, *o_psi, *o_s, *o_scal;
  int *o_flags;
  size_t out_doubles;
};
int work_layout(plda_handle *h, int D, Work *w) {
  const size_t DD = (size_t)D * D, Dz = (size_t)D;
  w->DD = DD;
  w->out_doubles = 3 * Dz + DD + 8 + 2;
  const size_t total = 13 * DD + 8 * Dz + 16 + w->out_doubles;
  PLDA_HIP(h, h->ad_work.reserve(total * 8));
  double *b = h->ad_work.as<double>();
  w->W = b; w->B = b + DD; w->Tinv = b + 2 * DD; w->tmp = b + 3 * DD; w->G = b + 4 * DD; w->P = b + 5 * DD; w->F = b + 6 * DD;
  w->Tm = b + 7 * DD; w->W2 = b + 8 * DD; w->B2 = b + 9 * DD; w->scr = b + 10 * DD;   // scr: 3 DD
  w->vec = b + 13 * DD;                                                              // delta | e | T2-side vectors ... (8 D)
  w->own = reinterpret_cast<int *>(w->vec + 8 * Dz);                                 // 16 doubles of status words
  w->out = w->vec + 8 * Dz + 16;
  w->o_mean = w->out; w->o_T = w->out + Dz; w->o_psi = w->o_T + DD; w->o_s = w->o_psi + Dz; w->o_scal = w->o_s + Dz;
  w->o_flags = reinterpret_cast<int *>(w->o_scal + 8);
  return PLDA_OK;
}

// W, B and Tinv of a model inside a Work (model_covariances_f64 below)
int model_covariances(plda_handle *h, const double *T, const double *psi, int D, const Work &w, double *W, double *B,
                      double *Tinv, int *flag) {
  return model_covariances_f64(h, T, psi, D, W, B, Tinv, w.tmp, w.scr, flag);
}

// (W', B') in w.W / w.B -> the staged model, read back with the status words; installs it on success.  `chain` enqueues
// everything up to (W', B') and the staged mean; it runs again with the block Jacobi solver if the direct one gave up.
template <typename Chain>
int diagonalise_and_install(plda_handle *h, int D, const Work &w, const char *what, Chain &&chain, std::vector<double> &host) {
  const size_t DD = w.DD, Dz = (size_t)D;
  host.resize(w.out_doubles);
  const int saved_variant = h->eig_variant;
  int rc = PLDA_OK;
  for (int attempt = 0; attempt < 2; ++attempt) {
    rc = [&]() -> int {
      PLDA_HIP(h, hipMemsetAsync(w.own, 0, 16 * 8, h->stream));
      PLDA_HIP(h, hipMemsetAsync(w.o_scal, 0, 8 * 8, h->stream));
      PLDA_TRY(chain());
      adapt_symmetrize_kernel<<<blocks((int64_t)DD), 256, 0, h->stream>>>(w.W, D);
      adapt_symmetrize_kernel<<<blocks((int64_t)DD), 256, 0, h->stream>>>(w.B, D);
      PLDA_LAUNCH_CHECK(h);
      bool pending = false;
      PLDA_TRY(simdiag_enqueue(h, w.W, w.B, D, w.o_T, nullptr, w.o_psi, &pending));
      const int *chol_dev = nullptr, *eig_dev = nullptr;
      if (pending) simdiag_flags(h, D, &chol_dev, &eig_dev);
      // pending without a flag: the direct method did not run (its launch was refused), T' was formed from whatever the
      // eigenvector buffer held -- status 8, and the second attempt runs block Jacobi
      adapt_flags_kernel<<<1, 1, 0, h->stream>>>(w.own, chol_dev, eig_dev, 0, pending ? 8 : 0, w.o_flags);
      PLDA_LAUNCH_CHECK(h);
      PLDA_HIP(h, hipMemcpyAsync(host.data(), w.out, w.out_doubles * 8, hipMemcpyDeviceToHost, h->stream));
      PLDA_HIP(h, hipStreamSynchronize(h->stream));
      return PLDA_OK;
    }();
    if (rc != PLDA_OK) break;
    int f[4];
    std::memcpy(f, host.data() + 3 * Dz + DD + 8, sizeof(f));
    if (f[0]) { rc = fail(h, PLDA_E_NUMERIC, "%s: a model's transform is singular (T^T T is not positive definite)", what); break; }
    if (f[2]) { rc = fail(h, PLDA_E_NUMERIC, "%s: the new within-class covariance is not positive definite", what); break; }
    if (f[1] == 0 && f[3] == 0) break;
    if (attempt == 1 || saved_variant == 1) { rc = fail(h, PLDA_E_NUMERIC, "%s: the eigensolver failed (status %d / %d)", what, f[1], f[3]); break; }
    h->eig_variant = 1;      // the direct method gave up: once more on block Jacobi
  }
  h->eig_variant = saved_variant;
  if (rc != PLDA_OK) return rc;
  const double *hm = host.data(), *hT = hm + Dz, *hp = hT + DD;
  for (size_t i = 0; i < Dz + DD + Dz; ++i)
    if (!std::isfinite(hm[i])) return fail(h, PLDA_E_NUMERIC, "%s: the new model is not finite", what);
  // ---- install (as plda_set_model does): device copies, host mirrors, epoch, prepared test side, offset ----
  PLDA_HIP(h, hipMemcpyAsync(h->d_mean.p, w.o_mean, Dz * 8, hipMemcpyDeviceToDevice, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(h->d_transform.p, w.o_T, DD * 8, hipMemcpyDeviceToDevice, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(h->d_psi.p, w.o_psi, Dz * 8, hipMemcpyDeviceToDevice, h->stream));
  h->h_mean.assign(hm, hm + Dz);
  h->h_transform.assign(hT, hT + DD);
  h->h_psi.assign(hp, hp + Dz);
  ++h->model_epoch;
  h->prep_valid = false;
  PLDA_TRY(compute_offset_device(h));
  h->h_offset.resize(Dz);
  PLDA_HIP(h, hipMemcpyAsync(h->h_offset.data(), h->d_offset.p, Dz * 8, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  return PLDA_OK;
}

int64_t slab_rows_for(const plda_handle *h, int ld) {
  int64_t rows = h->ad_slab_rows > 0 ? h->ad_slab_rows
                                     : std::min<int64_t>(AD_SLAB_MAX_ROWS, std::max<int64_t>(256, AD_SLAB_BYTES / ((int64_t)ld * 8)));
  return std::max<int64_t>(1, rows);
}

}  // namespace

// W = (T^T T)^-1, Tinv = T^-1 = W T^T, B = Tinv diag(psi) Tinv^T  (tmp: D^2, scr: 3 D^2 doubles of scratch; *flag: set when
// T^T T is not SPD).  Shared with dense_pca.hip, which projects the same two covariances.
int model_covariances_f64(plda_handle *h, const double *T, const double *psi, int D, double *W, double *B, double *Tinv, double *tmp,
                          double *scr, int *flag) {
  const size_t DD = (size_t)D * D;
  PLDA_TRY(gemm_f64(h, D, D, D, 1.0, T, 1, D, T, D, 1, nullptr, 0.0, tmp, D));
  PLDA_TRY(spd_inverse_blocked(h, tmp, D, D, (int64_t)DD, W, D, (int64_t)DD, scr, (int64_t)(3 * DD), flag, 1));
  adapt_symmetrize_kernel<<<blocks((int64_t)DD), 256, 0, h->stream>>>(W, D);
  PLDA_LAUNCH_CHECK(h);
  PLDA_TRY(gemm_f64(h, D, D, D, 1.0, W, D, 1, T, 1, D, nullptr, 0.0, Tinv, D));
  adapt_scale_kernel<<<blocks((int64_t)DD), 256, 0, h->stream>>>(Tinv, psi, D, 0, 0, tmp);
  PLDA_LAUNCH_CHECK(h);
  return gemm_f64(h, D, D, D, 1.0, tmp, D, 1, tmp, 1, D, nullptr, 0.0, B, D);
}

int adapt_reset(plda_handle *h) {
  h->ad_has = false;
  h->ad_used = false;
  h->ad_rows = 0;
  h->ad_tw = 0.0;
  h->ad_D = 0;
  h->ad_pilot.clear();
  return PLDA_OK;
}

// the record's device buffer for dimension D, zeroed, with the model mean as pilot (the record itself counts only once
// h->ad_has is set)
static int record_begin(plda_handle *h, int D) {
  const size_t Da = (size_t)D + 1;
  PLDA_HIP(h, h->ad_rec.reserve((Da * Da + D) * 8));
  PLDA_HIP(h, hipMemsetAsync(h->ad_rec.p, 0, Da * Da * 8, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(h->ad_rec.as<double>() + Da * Da, h->d_mean.p, (size_t)D * 8, hipMemcpyDeviceToDevice, h->stream));
  return PLDA_OK;
}
static void record_commit(plda_handle *h, int D) {
  if (h->ad_has) return;
  h->ad_has = true;
  h->ad_used = false;
  h->ad_D = D;
  h->ad_epoch = h->model_epoch;
  h->ad_rows = 0;
  h->ad_tw = 0.0;
  h->ad_pilot = h->h_mean;
}
static int record_current(plda_handle *h, const char *what) {
  if (h->ad_has && (h->ad_epoch != h->model_epoch || h->ad_D != h->Din))
    return fail(h, PLDA_E_INVAL, "%s: the record was taken under an earlier model (the model changed since its pilot); reset first", what);
  return PLDA_OK;
}

int adapt_accumulate(plda_handle *h, const double *X, int64_t N, int Din, const double *weights, bool host) {
  PLDA_TRY(square_model(h, "adapt_accumulate"));
  if (N < 0) return fail(h, PLDA_E_INVAL, "adapt_accumulate: N = %lld", (long long)N);
  if (Din != h->Din) return fail(h, PLDA_E_INVAL, "adapt_accumulate: feature dim %d != model dim %d", Din, h->Din);
  PLDA_TRY(record_current(h, "adapt_accumulate"));
  if (N == 0) return PLDA_OK;
  if (!X) return fail(h, PLDA_E_INVAL, "adapt_accumulate: the rows are NULL");
  const int D = Din, Da = D + 1, ld = (Da + 1) & ~1;
  const size_t nrec = (size_t)Da * Da;
  if (!h->ad_has) PLDA_TRY(record_begin(h, D));
  double *rec = h->ad_rec.as<double>();
  const double *pilot = rec + nrec;
  const int64_t slab = std::min(slab_rows_for(h, ld), N);
  // slab | the call's sums [Da, Da] | the record's tw after the call | reject counters
  PLDA_HIP(h, h->ad_slab.reserve(((size_t)slab * ld + nrec + 2) * 8 + 16));
  double *S = h->ad_slab.as<double>(), *acc = S + (size_t)slab * ld, *dtw = acc + nrec;
  int *bad = reinterpret_cast<int *>(dtw + 1);
  double *stage_x = nullptr, *stage_w = nullptr;
  if (host) {
    PLDA_HIP(h, h->ad_stage.reserve((size_t)slab * (D + 1) * 8));
    stage_x = h->ad_stage.as<double>();
    stage_w = stage_x + (size_t)slab * D;
  }
  PLDA_HIP(h, hipMemsetAsync(bad, 0, 2 * sizeof(int), h->stream));
  for (int64_t r0 = 0; r0 < N; r0 += slab) {
    const int64_t R = std::min(slab, N - r0);
    const double *x = X + r0 * D, *wv = weights ? weights + r0 : nullptr;
    if (host) {
      PLDA_HIP(h, hipMemcpyAsync(stage_x, x, (size_t)R * D * 8, hipMemcpyHostToDevice, h->stream));
      if (wv) PLDA_HIP(h, hipMemcpyAsync(stage_w, wv, (size_t)R * 8, hipMemcpyHostToDevice, h->stream));
      x = stage_x;
      wv = wv ? stage_w : nullptr;
    }
    {
      TraceScope ts(h, "adapt.centre (slab of [x - p | 1])", (double)R * (D + ld) * 8.0, 2);
      adapt_centre_kernel<<<(unsigned)ceil_div(R, 4), 256, 0, h->stream>>>(x, wv, pilot, R, D, ld, S, bad);
      PLDA_LAUNCH_CHECK(h);
    }
    TraceScope ts(h, "adapt.syrk (the fit's weighted SYRK on the slab)", (double)R * Da * Da, 1);
    PLDA_TRY(syrk_f64(h, Da, R, 1.0, S, ld, wv, r0 == 0 ? 0.0 : 1.0, acc, Da));   // slabs are added in the order of the rows
  }
  adapt_fold_kernel<<<blocks((int64_t)nrec), 256, 0, h->stream>>>(rec, acc, (int64_t)nrec, bad, dtw);
  PLDA_LAUNCH_CHECK(h);
  int hbad[2] = {0, 0};
  double htw = 0.0;
  PLDA_HIP(h, hipMemcpyAsync(hbad, bad, sizeof(hbad), hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(&htw, dtw, 8, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  if (hbad[0] || hbad[1])
    return fail(h, PLDA_E_INVAL, "adapt_accumulate: %d row(s) with a non-finite element, %d negative or non-finite weight(s); "
                                 "the record is unchanged", hbad[0], hbad[1]);
  record_commit(h, D);
  h->ad_rows += N;
  h->ad_tw = htw;
  return PLDA_OK;
}

int adapt_get_stats(plda_handle *h, double *tw, int64_t *rows, double *pilot, double *s1, double *s2) {
  PLDA_TRY(square_model(h, "adapt_get_stats"));
  // the caller sized its arrays from the model: a record of another dimension (the model was replaced since) would overrun
  // them.  A stale record of the same dimension stays readable.
  if (h->ad_has && h->ad_D != h->Din)
    return fail(h, PLDA_E_INVAL, "adapt_get_stats: the record has dimension %d, the model %d (the model was replaced since "
                                 "the record's pilot); reset first", h->ad_D, h->Din);
  const int D = h->Din, Da = D + 1;
  if (!h->ad_has) {
    if (tw) *tw = 0.0;
    if (rows) *rows = 0;
    if (pilot) std::memcpy(pilot, h->h_mean.data(), (size_t)D * 8);
    if (s1) std::memset(s1, 0, (size_t)D * 8);
    if (s2) std::memset(s2, 0, (size_t)D * D * 8);
    return PLDA_OK;
  }
  if (tw) *tw = h->ad_tw;
  if (rows) *rows = h->ad_rows;
  if (pilot) std::memcpy(pilot, h->ad_pilot.data(), (size_t)D * 8);
  if (s1 || s2) {
    const double *rec = h->ad_rec.as<double>();
    if (s2) PLDA_HIP(h, hipMemcpy2DAsync(s2, (size_t)D * 8, rec, (size_t)Da * 8, (size_t)D * 8, (size_t)D, hipMemcpyDeviceToHost, h->stream));
    if (s1) PLDA_HIP(h, hipMemcpy2DAsync(s1, 8, rec + D, (size_t)Da * 8, 8, (size_t)D, hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
  }
  return PLDA_OK;
}

int adapt_add_stats(plda_handle *h, double tw, int64_t rows, const double *pilot, const double *s1, const double *s2) {
  PLDA_TRY(square_model(h, "adapt_add_stats"));
  if (!pilot || !s1 || !s2) return fail(h, PLDA_E_INVAL, "adapt_add_stats: pilot, s1 or s2 is NULL");
  if (!(tw >= 0.0) || !std::isfinite(tw) || rows < 0) return fail(h, PLDA_E_INVAL, "adapt_add_stats: tw = %g, rows = %lld", tw, (long long)rows);
  PLDA_TRY(record_current(h, "adapt_add_stats"));
  const int D = h->Din, Da = D + 1;
  const size_t nrec = (size_t)Da * Da;
  const std::vector<double> &mine = h->ad_has ? h->ad_pilot : h->h_mean;
  if (std::memcmp(pilot, mine.data(), (size_t)D * 8) != 0)
    return fail(h, PLDA_E_INVAL, h->ad_has ? "adapt_add_stats: the pilot differs from this record's (records add only about one pilot)"
                                           : "adapt_add_stats: the pilot differs from the model mean (an empty record takes the mean as its pilot)");
  std::vector<double> aug(nrec);
  for (int i = 0; i < D; ++i) {
    for (int j = 0; j < D; ++j) {
      const double v = s2[(size_t)i * D + j];
      if (!std::isfinite(v)) return fail(h, PLDA_E_INVAL, "adapt_add_stats: s2 is not finite");
      aug[(size_t)i * Da + j] = v;
    }
    if (!std::isfinite(s1[i])) return fail(h, PLDA_E_INVAL, "adapt_add_stats: s1 is not finite");
    aug[(size_t)i * Da + D] = s1[i];
    aug[(size_t)D * Da + i] = s1[i];
  }
  aug[(size_t)D * Da + D] = tw;
  if (!h->ad_has) PLDA_TRY(record_begin(h, D));
  PLDA_HIP(h, h->ad_slab.reserve((nrec + 2) * 8 + 16));
  double *acc = h->ad_slab.as<double>(), *dtw = acc + nrec;
  PLDA_HIP(h, hipMemcpyAsync(acc, aug.data(), nrec * 8, hipMemcpyHostToDevice, h->stream));
  adapt_fold_kernel<<<blocks((int64_t)nrec), 256, 0, h->stream>>>(h->ad_rec.as<double>(), acc, (int64_t)nrec, nullptr, dtw);
  PLDA_LAUNCH_CHECK(h);
  double htw = 0.0;
  PLDA_HIP(h, hipMemcpyAsync(&htw, dtw, 8, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  record_commit(h, D);
  h->ad_rows += rows;
  h->ad_tw = htw;
  return PLDA_OK;
}

int adapt_update(plda_handle *h, double ws, double bs, double mds, double *eig, plda_adapt_info *info) {
  PLDA_TRY(square_model(h, "adapt_update"));
  PLDA_TRY(supported_dim(h, "adapt_update"));
  if (!(ws >= 0.0) || !(bs >= 0.0) || !(mds >= 0.0) || !std::isfinite(ws) || !std::isfinite(bs) || !std::isfinite(mds))
    return fail(h, PLDA_E_INVAL, "adapt_update: scales must be finite and >= 0 (within %g, between %g, mean_diff %g)", ws, bs, mds);
  if (!h->ad_has || !(h->ad_tw > 0.0)) return fail(h, PLDA_E_INVAL, "adapt_update: no statistics (total weight %g); accumulate first", h->ad_has ? h->ad_tw : 0.0);
  PLDA_TRY(record_current(h, "adapt_update"));
  if (h->ad_used) return fail(h, PLDA_E_INVAL, "adapt_update: this record has already been used for an update; reset first");
  const int D = h->Din, Da = D + 1;
  const size_t DD = (size_t)D * D, Dz = (size_t)D;
  Work w;
  PLDA_TRY(work_layout(h, D, &w));
  const double *rec = h->ad_rec.as<double>(), *pilot = rec + (size_t)Da * Da;
  const double *T = h->d_transform.as<double>(), *psi = h->d_psi.as<double>();
  double *delta = w.vec, *e = w.vec + Dz;
  const unsigned gDD = blocks((int64_t)DD);
  auto chain = [&]() -> int {
    PLDA_TRY(model_covariances(h, T, psi, D, w, w.W, w.B, w.Tinv, &w.own[0]));
    adapt_mean_kernel<<<1, 256, 0, h->stream>>>(rec, pilot, D, delta, w.o_mean, w.o_scal);
    adapt_var_kernel<<<gDD, 256, 0, h->stream>>>(rec, delta, D, 1.0 - mds, w.F);                    // V (in F for now)
    adapt_scale_kernel<<<gDD, 256, 0, h->stream>>>(T, psi, D, 1, 2, w.Tm);                          // Tm = diag(1 / sqrt(1 + psi)) T
    PLDA_LAUNCH_CHECK(h);
    PLDA_TRY(gemm_f64(h, D, D, D, 1.0, w.Tm, D, 1, w.F, D, 1, nullptr, 0.0, w.tmp, D));             // Tm V
    PLDA_TRY(gemm_f64(h, D, D, D, 1.0, w.tmp, D, 1, w.Tm, 1, D, nullptr, 0.0, w.G, D));             // Vp = Tm V Tm^T
    adapt_symmetrize_kernel<<<gDD, 256, 0, h->stream>>>(w.G, D);
    PLDA_LAUNCH_CHECK(h);
    bool direct = h->eig_variant != 1;
    if (direct) {                                   // deferred: its status word is copied next to ours and read at the end
      PLDA_TRY(sym_eig_dc_f64(h, w.G, D, w.o_s, w.P, nullptr));
      if (h->eigdc_flag) PLDA_HIP(h, hipMemcpyAsync(&w.own[1], h->eigdc_flag, sizeof(int), hipMemcpyDeviceToDevice, h->stream));
      else direct = false;                          // the device cannot run it: block Jacobi (which reads its convergence flag)
    }
    if (!direct) PLDA_TRY(sym_eig_f64(h, w.G, D, w.o_s, w.P, nullptr, nullptr));
    adapt_excess_kernel<<<1, 256, 0, h->stream>>>(w.o_s, D, e, w.o_scal);
    adapt_scale_kernel<<<gDD, 256, 0, h->stream>>>(w.Tinv, psi, D, 0, 1, w.tmp);                    // Tm^-1 = T^-1 diag(sqrt(1 + psi))
    PLDA_LAUNCH_CHECK(h);
    PLDA_TRY(gemm_f64(h, D, D, D, 1.0, w.tmp, D, 1, w.P, 1, D, nullptr, 0.0, w.F, D));              // Tm^-1 P (P's columns = rows of w.P)
    adapt_scale_kernel<<<gDD, 256, 0, h->stream>>>(w.F, e, D, 0, 0, w.tmp);                         // ... diag(sqrt(e))
    PLDA_LAUNCH_CHECK(h);
    if (ws != 0.0) PLDA_TRY(gemm_f64(h, D, D, D, ws, w.tmp, D, 1, w.tmp, 1, D, nullptr, 1.0, w.W, D));   // W' = W + ws E
    if (bs != 0.0) PLDA_TRY(gemm_f64(h, D, D, D, bs, w.tmp, D, 1, w.tmp, 1, D, nullptr, 1.0, w.B, D));   // B' = B + bs E
    return PLDA_OK;
  };
  std::vector<double> host;
  PLDA_TRY(diagonalise_and_install(h, D, w, "adapt_update", chain, host));
  h->ad_used = true;
  const double *hs = host.data() + 2 * Dz + DD, *sc = hs + Dz;
  if (eig) std::memcpy(eig, hs, Dz * 8);
  if (info) {
    info->tot_weight = sc[0];
    info->rows = h->ad_rows;
    info->dim = D;
    info->n_excess = (int32_t)sc[2];
    info->eig_max = sc[3];
    info->eig_min = sc[4];
    info->mean_shift = sc[1];
  }
  return PLDA_OK;
}

int blend_model(plda_handle *h, int D, const double *mean2, const double *transform2, const double *psi2, double alpha,
                double alpha_mean) {
  PLDA_TRY(square_model(h, "blend_model"));
  PLDA_TRY(supported_dim(h, "blend_model"));
  if (!mean2 || !transform2 || !psi2) return fail(h, PLDA_E_INVAL, "blend_model: mean, transform or psi of the second model is NULL");
  if (D != h->Din) return fail(h, PLDA_E_INVAL, "blend_model: the second model has dimension %d, this one %d", D, h->Din);
  if (!(alpha >= 0.0 && alpha <= 1.0) || !(alpha_mean >= 0.0 && alpha_mean <= 1.0))
    return fail(h, PLDA_E_INVAL, "blend_model: alpha = %g, alpha_mean = %g (both must be in [0, 1])", alpha, alpha_mean);
  const size_t DD = (size_t)D * D, Dz = (size_t)D;
  Work w;
  PLDA_TRY(work_layout(h, D, &w));
  double *T2 = w.P, *psi2d = w.vec, *mean2d = w.vec + Dz;
  PLDA_HIP(h, hipMemcpyAsync(T2, transform2, DD * 8, hipMemcpyHostToDevice, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(psi2d, psi2, Dz * 8, hipMemcpyHostToDevice, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(mean2d, mean2, Dz * 8, hipMemcpyHostToDevice, h->stream));
  const double *T = h->d_transform.as<double>(), *psi = h->d_psi.as<double>();
  auto chain = [&]() -> int {
    PLDA_TRY(model_covariances(h, T, psi, D, w, w.W, w.B, w.Tinv, &w.own[0]));
    PLDA_TRY(model_covariances(h, T2, psi2d, D, w, w.W2, w.B2, w.Tinv, &w.own[0]));
    adapt_axpby_kernel<<<blocks((int64_t)DD), 256, 0, h->stream>>>((int64_t)DD, 1.0 - alpha, w.W, alpha, w.W2, w.W);
    adapt_axpby_kernel<<<blocks((int64_t)DD), 256, 0, h->stream>>>((int64_t)DD, 1.0 - alpha, w.B, alpha, w.B2, w.B);
    adapt_axpby_kernel<<<blocks((int64_t)D), 256, 0, h->stream>>>((int64_t)D, 1.0 - alpha_mean, h->d_mean.as<double>(), alpha_mean, mean2d, w.o_mean);
    PLDA_LAUNCH_CHECK(h);
    return PLDA_OK;
  };
  std::vector<double> host;
  return diagonalise_and_install(h, D, w, "blend_model", chain, host);
}

}  // namespace plda
