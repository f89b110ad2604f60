// plda_amd/csrc/dense_pca.hip -- recording-dependent PCA before dense PLDA scoring (the contract is in
// include/plda_hip.h, "dense scoring in a recording's PCA subspace"; the NumPy model in tests/dense_pca_model.py).
//
// Kaldi's ivector-plda-scoring-dense --target-energy restated: per recording a PCA of its own segment vectors, the model
// projected into the leading directions (Plda::ApplyTransform), all segment pairs scored there.  Every recording is a chain
// of small dense problems of order m = min(N, D) <= 512: one workgroup per recording, many recordings in flight.
//
//   dpca_count_kernel    the rows of the call with a non-finite element (one integer counter; a call that meets one fails,
//                        and the kernel behind it writes nothing)
//   dpca_kernel<HBM, T>  steps 1 to 7 of one recording.  <false, 256>: the working matrix A and the eigenvectors V in LDS,
//                        m <= DP_LDS_MAX; <true, 1024>: both in handle scratch.  Everything else a recording needs (centred
//                        rows, basis, projected model, vectors) is in handle scratch in both classes.
//
// The eigensolver (dp_jacobi) is a two-sided cyclic Jacobi in round-robin order: a round holds floor((m + 1) / 2) disjoint
// pairs; their angles are computed first, then the rows of A and of V are rotated, then the columns of A, with a workgroup
// barrier between the phases.  The matrix itself is rotated from both sides (never its square), so the small retained
// directions keep the accuracy a backward-stable solver gives them.  The order of the rotations is a function of m alone
// and every sum runs over ascending indices in one thread: a recording's block does not depend on the batch it is in, on the
// grouping into launches or on the run.  Phases communicate through LDS or through scratch behind __syncthreads() only.
#include "common.hpp"
#include "slab_walk.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace plda {

namespace {

constexpr int DP_MAX_DIM = PLDA_DENSE_PCA_MAX_DIM;
constexpr int DP_LDS_BYTES = 160 * 1024;       // one workgroup may hold all of a CU's LDS
constexpr int DP_T_LDS = 256, DP_T_HBM = 1024;
constexpr int DP_MAX_SWEEPS = 40;
constexpr double DP_RANK_TOL = 0x1p-40;        // rank: eigenvalues above this share of the largest
constexpr double DP_CONV = 0x1p-52;            // |a_pq| <= DP_CONV sqrt(a_pp a_qq): the pair is left alone
constexpr double DP_FLOOR = 0x1p-92;           // ... or |a_pq| <= DP_FLOOR max |a_ii| (a_pp <= 0 on a null direction)

// fixed LDS of a recording of order m: (c, s) and (p, q) of every pair of a round, then the step scalars
constexpr long long dp_lds_bytes(long long m, bool hbm) {
  return (hbm ? 0 : 16 * m * m) + ((m + 1) / 2) * (16 + 4) + 64 + 12;   // (+12: the pair words end on any multiple of 4)
}
constexpr int dp_lds_max_calc() {
  int m = 1;
  while (m < DP_MAX_DIM && dp_lds_bytes(m + 1, false) <= DP_LDS_BYTES) ++m;
  return m;
}
constexpr int DP_LDS_MAX = dp_lds_max_calc();
static_assert(dp_lds_bytes(DP_LDS_MAX, false) <= DP_LDS_BYTES, "the LDS class must fit one CU's LDS");
static_assert(dp_lds_bytes(DP_MAX_DIM, true) <= 64 * 1024, "the HBM class's round state must fit");

// one recording of a launch (host-built from the scratch layout list, uploaded once per enqueue)
struct DpRec {
  long long xoff;    // first row of X (and first entry of deig)
  long long boff;    // first float of the block, relative to the scores pointer
  double *Xc, *A, *V, *P, *Q, *M, *Wp, *Bp, *Y, *vec;
  int *perm;
  int n, r, m, gram;
};

// the scratch of one recording: ONE list gives its bytes and its pointers (layout.hpp).  A, V: the working matrix and the
// eigenvectors (HBM class; LDS otherwise); P: the basis; Q: P W, P B, then L^-1 P; M: the projection; Wp: W', then its
// Cholesky factor; Bp: B', then L^-1 B' L^-T; Y: the projected rows, transposed [d][N]; vec: lam, psi, the factor's diagonal,
// three coefficient rows and the mean; perm: the descending order of the last eigenproblem
void dp_layout(Layout &l, DpRec &rc, int64_t n, int64_t D, int64_t m, bool hbm) {
  l.take(rc.Xc, (size_t)(n * D)).take(rc.A, hbm ? (size_t)(m * m) : 0).take(rc.V, hbm ? (size_t)(m * m) : 0)
      .take(rc.P, (size_t)(m * D)).take(rc.Q, (size_t)(m * D)).take(rc.M, (size_t)(m * D)).take(rc.Wp, (size_t)(m * m))
      .take(rc.Bp, (size_t)(m * m)).take(rc.Y, (size_t)(n * m)).take(rc.vec, (size_t)(6 * m + D)).take(rc.perm, (size_t)m)
      .slack(0);
}

__global__ __launch_bounds__(256) void dpca_count_kernel(const double *__restrict__ X, int64_t rows, int D,
                                                         unsigned long long *bad) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;                    // (whole waves leave together: no barrier follows)
  const double *x = X + r * D;
  int nonfinite = 0;
  for (int c = lane; c < D; c += 64) nonfinite |= !isfinite(x[c]);
  if (__any(nonfinite) && lane == 0) atomicAdd(bad, 1ull);   // rare: one integer atomic per bad row
}

// pair k of round `rnd` of the round-robin over np2 = m rounded up to even players (the last one fixed): p < q; q >= m is the bye
__device__ __forceinline__ void dp_pair(int np2, int rnd, int k, int &p, int &q) {
  const int ring = np2 - 1;
  int a, b;
  if (k == 0) { a = ring; b = rnd; }
  else { a = (rnd + k) % ring; b = (rnd - k + ring) % ring; }
  p = a < b ? a : b;
  q = a < b ? b : a;
}

// Two-sided cyclic Jacobi on the symmetric A [m][m] (destroyed: its diagonal ends as the eigenvalues, unsorted); Vt [m][m]
// ends with the eigenvectors in its ROWS.  cs / pq / nrot: LDS.  Returns the sweeps made, or -1 without convergence.
// Every thread of the workgroup must call it (it holds barriers); the result is uniform.
template <int T>
__device__ int dp_jacobi(double *A, double *Vt, int m, double *cs, int *pq, int *nrot, int tid) {
  constexpr int W = T / 64;
  const int lane = tid & 63, wave = tid >> 6;
  const int np2 = m + (m & 1), half = np2 / 2;
  for (int i = wave; i < m; i += W)
    for (int j = lane; j < m; j += 64) Vt[i * m + j] = i == j ? 1.0 : 0.0;
  double amax = 0.0;
  for (int i = 0; i < m; ++i) amax = fmax(amax, fabs(A[i * m + i]));      // (every thread the same m loads: m <= 512)
  const double floor_abs = DP_FLOOR * amax;
  if (tid == 0) *nrot = 0;
  __syncthreads();
  int sweeps = -1;
  for (int sweep = 0; sweep < DP_MAX_SWEEPS; ++sweep) {
    for (int rnd = 0; rnd < np2 - 1; ++rnd) {
      // angles of the round
      for (int k = tid; k < half; k += T) {
        int p, q;
        dp_pair(np2, rnd, k, p, q);
        double c = 1.0, s = 0.0;
        if (q < m) {
          const double app = A[p * m + p], aqq = A[q * m + q], apq = A[p * m + q];
          const double mag = fabs(apq);
          if (!(mag <= DP_CONV * sqrt(fabs(app * aqq)) || mag <= floor_abs)) {
            const double tau = (aqq - app) / (2.0 * apq);
            const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + t * t);
            s = t * c;
            atomicAdd(nrot, 1);                 // (LDS integer: only "any" is read)
          }
        }
        cs[2 * k] = c; cs[2 * k + 1] = s;
        pq[k] = p | (q << 16);
      }
      __syncthreads();
      // rows p, q of A and of Vt
      for (int k = wave; k < half; k += W) {
        const double c = cs[2 * k], s = cs[2 * k + 1];
        if (s == 0.0) continue;
        const int p = pq[k] & 0xffff, q = pq[k] >> 16;
        for (int j = lane; j < m; j += 64) {
          const double ap = A[p * m + j], aq = A[q * m + j];
          A[p * m + j] = c * ap - s * aq;
          A[q * m + j] = s * ap + c * aq;
          const double vp = Vt[p * m + j], vq = Vt[q * m + j];
          Vt[p * m + j] = c * vp - s * vq;
          Vt[q * m + j] = s * vp + c * vq;
        }
      }
      __syncthreads();
      // columns p, q of A; the rotated pair itself is set to zero exactly
      for (int i = wave; i < m; i += W) {
        for (int k = lane; k < half; k += 64) {
          const double c = cs[2 * k], s = cs[2 * k + 1];
          if (s == 0.0) continue;
          const int p = pq[k] & 0xffff, q = pq[k] >> 16;
          const double ap = A[i * m + p], aq = A[i * m + q];
          double np_ = c * ap - s * aq, nq_ = s * ap + c * aq;
          if (i == p) nq_ = 0.0;
          if (i == q) np_ = 0.0;
          A[i * m + p] = np_;
          A[i * m + q] = nq_;
        }
      }
      __syncthreads();
    }
    const int rotated = *nrot;
    __syncthreads();
    if (tid == 0) *nrot = 0;
    // the lower triangle follows the upper one (the two drift apart by rounding; the angles read the upper)
    for (int i = wave; i < m; i += W)
      for (int j = lane; j < i; j += 64) A[i * m + j] = A[j * m + i];
    __syncthreads();
    if (!rotated) { sweeps = sweep + 1; break; }
  }
  return sweeps;
}

// descending order of the diagonal of A [m][m]: out[rank] = max(diag, floor_at), perm[rank] = index (ties: the smaller index first)
template <int T>
__device__ void dp_sort_diag(const double *A, int m, double *out, int *perm, bool floor0, int tid) {
  for (int k = tid; k < m; k += T) {
    const double v = A[k * m + k];
    int rank = 0;
    for (int j = 0; j < m; ++j) {
      const double o = A[j * m + j];
      rank += (o > v || (o == v && j < k)) ? 1 : 0;
    }
    out[rank] = floor0 ? fmax(v, 0.0) : v;
    perm[rank] = k;
  }
  __syncthreads();
}

// C [Mr][Nc] (ldc) = sum_k A(i, k) B(k, j), ascending k in one thread; lanes run over j
template <int T>
__device__ void dp_gemm(double *C, int ldc, int Mr, int Nc, int K, const double *A, int sam, int sak, const double *B, int sbk,
                        int sbn, int tid) {
  constexpr int W = T / 64;
  const int lane = tid & 63, wave = tid >> 6;
  for (int i = wave; i < Mr; i += W)
    for (int j = lane; j < Nc; j += 64) {
      double acc = 0.0;
      for (int k = 0; k < K; ++k) acc = fma(A[(long long)i * sam + (long long)k * sak], B[(long long)k * sbk + (long long)j * sbn], acc);
      C[(long long)i * ldc + j] = acc;
    }
  __syncthreads();
}

// G [d][d] <- (G + G^T) / 2, both triangles written
template <int T> __device__ void dp_symmetrize(double *G, int d, int tid) {
  constexpr int W = T / 64;
  const int lane = tid & 63, wave = tid >> 6;
  for (int i = wave; i < d; i += W)
    for (int j = lane; j < i; j += 64) {
      const double v = 0.5 * (G[i * d + j] + G[j * d + i]);
      G[i * d + j] = v;
      G[j * d + i] = v;
    }
  __syncthreads();
}

// X [d][nc] (ldx) <- L^-1 X for the lower-triangular L = R^T: R's strict upper triangle in Rm [d][d], its diagonal in rd
template <int T> __device__ void dp_trsm(const double *Rm, const double *rd, int d, double *X, int ldx, int nc, int tid) {
  constexpr int W = T / 64;
  const int lane = tid & 63, wave = tid >> 6;
  for (int k = 0; k < d; ++k) {
    const double piv = rd[k];
    for (int c = tid; c < nc; c += T) X[(long long)k * ldx + c] /= piv;
    __syncthreads();
    for (int i = k + 1 + wave; i < d; i += W) {
      const double l = Rm[k * d + i];
      for (int c = lane; c < nc; c += 64) X[(long long)i * ldx + c] -= l * X[(long long)k * ldx + c];
    }
    __syncthreads();
  }
}

template <bool HBM, int T>
__global__ __launch_bounds__(T) void dpca_kernel(const double *__restrict__ dX, int D, const DpRec *__restrict__ tab,
                                                 const double *__restrict__ Wm, const double *__restrict__ Bm,
                                                 const double *__restrict__ mean, double target, unsigned long long *stat,
                                                 float *__restrict__ scores, int *__restrict__ dims, double *__restrict__ eig) {
  extern __shared__ double dp_smem[];
  if (stat[0]) return;
  constexpr int W = T / 64;
  const DpRec rc = tab[blockIdx.x];
  const int n = rc.n, m = rc.m, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double *__restrict__ X = dX + rc.xoff * D;

  // LDS: [A | V (LDS class)] | cs[2 * half] | scal[7] | two ints | pq[half]
  double *p8 = dp_smem;
  double *A = rc.A, *Vt = rc.V;
  if constexpr (!HBM) { A = p8; p8 += m * m; Vt = p8; p8 += m * m; }
  const int half = (m + 1) / 2;
  double *cs = p8; p8 += 2 * half;
  double *scal = p8; p8 += 7;                  // [0]: the scores' constant term
  int *sint = reinterpret_cast<int *>(p8); p8 += 1;   // [0] the rotation count, [1] the retained dimension
  int *pq = reinterpret_cast<int *>(p8);
  double *lam = rc.vec, *psi = lam + m, *rd = psi + m, *ck = rd + m, *ivar = ck + m, *ivar0 = ivar + m, *mu = ivar0 + m;
  double *Xc = rc.Xc;

  // ---- 1. the mean of the rows (x_0 + the mean of x_i - x_0), the centred rows, C or the Gram matrix
  for (int c = tid; c < D; c += T) {          // about the first row: equal rows centre to exact zeros
    const double x0 = X[c];
    double acc = 0.0;
#pragma unroll 8
    for (int i = 0; i < n; ++i) acc += X[(long long)i * D + c] - x0;
    mu[c] = x0 + acc / (double)n;
  }
  __syncthreads();
  for (int i = wave; i < n; i += W)
    for (int c = lane; c < D; c += 64) Xc[(long long)i * D + c] = X[(long long)i * D + c] - mu[c];
  __syncthreads();
  for (int i = wave; i < m; i += W)
    for (int j = lane; j < m; j += 64) {
      double acc = 0.0;
      if (rc.gram) {
        const double *xi = Xc + (long long)i * D, *xj = Xc + (long long)j * D;
        for (int c = 0; c < D; ++c) acc = fma(xi[c], xj[c], acc);
      } else {
#pragma unroll 4
        for (int r = 0; r < n; ++r) acc = fma(Xc[(long long)r * D + i], Xc[(long long)r * D + j], acc);
      }
      A[i * m + j] = acc / (double)n;
    }
  __syncthreads();

  // ---- 2. eigenvalues, descending
  const int sw1 = dp_jacobi<T>(A, Vt, m, cs, pq, &sint[0], tid);
  if (sw1 < 0) {
    if (tid == 0) atomicMin(&stat[2], (unsigned long long)rc.r);
    return;
  }
  dp_sort_diag<T>(A, m, lam, rc.perm, true, tid);
  if (eig)
    for (int k = tid; k < n; k += T) eig[rc.xoff + k] = k < m ? lam[k] : 0.0;

  // ---- 3. the retained dimension, Kaldi's rule
  if (tid == 0) {
    double E = 0.0;
    for (int k = 0; k < m; ++k) E += lam[k];
    int d = 0;
    if (E > 0.0) {
      int dim = 1;
      double energy = 0.0;
      while (energy / E <= target && dim - 1 < m) { energy += lam[dim - 1]; ++dim; }
      int rho = 0;
      const double cutoff = DP_RANK_TOL * lam[0];
      for (int k = 0; k < m; ++k) rho += lam[k] > cutoff ? 1 : 0;
      d = dim < rho ? dim : rho;
    }
    sint[1] = d;
    if (dims) dims[rc.r] = d;
  }
  __syncthreads();
  const int d = sint[1];
  float *__restrict__ S = scores + rc.boff;
  if (d == 0) {
    for (long long e = tid; e < (long long)n * n; e += T) S[e] = 0.0f;
    return;
  }

  // ---- 4. the basis P [d][D]
  double *P = rc.P, *Q = rc.Q, *M = rc.M, *Wp = rc.Wp, *Bp = rc.Bp, *Yt = rc.Y;
  for (int k = wave; k < d; k += W) {
    const double *u = Vt + rc.perm[k] * m;
    if (rc.gram) {
      const double f = sqrt((double)n * lam[k]);
      for (int c = lane; c < D; c += 64) {
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc = fma(u[i], Xc[(long long)i * D + c], acc);
        P[k * D + c] = acc / f;
      }
    } else {
      for (int c = lane; c < D; c += 64) P[k * D + c] = u[c];
    }
  }
  __syncthreads();

  // ---- 5. the model in the subspace: W' = P W P^T = R^T R, Z = L^-1 B' L^-T = U diag(psi') U^T, M = U^T L^-1 P
  dp_gemm<T>(Q, D, d, D, D, P, D, 1, Wm, D, 1, tid);
  dp_gemm<T>(Wp, d, d, d, D, Q, D, 1, P, 1, D, tid);
  dp_gemm<T>(Q, D, d, D, D, P, D, 1, Bm, D, 1, tid);
  dp_gemm<T>(Bp, d, d, d, D, Q, D, 1, P, 1, D, tid);
  dp_symmetrize<T>(Wp, d, tid);
  dp_symmetrize<T>(Bp, d, tid);
  for (int k = 0; k < d; ++k) {               // upper Cholesky in place: row k scaled, then the trailing update
    const double piv = Wp[k * d + k];
    if (!(piv > 0.0)) {                       // (uniform: every thread reads the same word)
      if (tid == 0) atomicMin(&stat[1], (unsigned long long)rc.r);
      return;
    }
    const double rkk = sqrt(piv);
    if (tid == 0) rd[k] = rkk;                // (the diagonal of R lives in rd: nobody writes Wp[k][k] from here on)
    for (int j = k + 1 + tid; j < d; j += T) Wp[k * d + j] /= rkk;
    __syncthreads();
    for (int i = k + 1 + wave; i < d; i += W) {
      const double l = Wp[k * d + i];
      for (int j = i + lane; j < d; j += 64) Wp[i * d + j] -= l * Wp[k * d + j];
    }
    __syncthreads();
  }
  dp_trsm<T>(Wp, rd, d, Bp, d, d, tid);
  for (int i = wave; i < d; i += W)           // transpose in place
    for (int j = lane; j < i; j += 64) {
      const double a = Bp[i * d + j], b = Bp[j * d + i];
      Bp[i * d + j] = b;
      Bp[j * d + i] = a;
    }
  __syncthreads();
  dp_trsm<T>(Wp, rd, d, Bp, d, d, tid);
  dp_symmetrize<T>(Bp, d, tid);
  for (int e = tid; e < d * d; e += T) A[e] = Bp[e];
  __syncthreads();
  const int sw2 = dp_jacobi<T>(A, Vt, d, cs, pq, &sint[0], tid);
  if (sw2 < 0) {
    if (tid == 0) atomicMin(&stat[2], (unsigned long long)rc.r);
    return;
  }
  dp_sort_diag<T>(A, d, psi, rc.perm, false, tid);
  for (int e = tid; e < d * D; e += T) Q[e] = P[e];
  __syncthreads();
  dp_trsm<T>(Wp, rd, d, Q, D, D, tid);
  for (int k = wave; k < d; k += W) {
    const double *u = Vt + rc.perm[k] * d;
    for (int c = lane; c < D; c += 64) {
      double acc = 0.0;
      for (int l = 0; l < d; ++l) acc = fma(u[l], Q[l * D + c], acc);
      M[k * D + c] = acc;
    }
  }
  for (int k = tid; k < d; k += T) {
    const double ps = psi[k], c = ps / (ps + 1.0);
    ck[k] = c;
    ivar[k] = 1.0 / (1.0 + c);
    ivar0[k] = 1.0 / (1.0 + ps);
  }
  if (tid == 0) {
    double acc = 0.0;
    for (int k = 0; k < d; ++k) { const double ps = psi[k]; acc += log(1.0 + ps / (ps + 1.0)) - log(1.0 + ps); }
    scal[0] = -0.5 * acc;
  }
  __syncthreads();

  // ---- 6. the rows: y_i = M (x_i - mean), length-normalised (num_examples = 1); kept transposed, Yt [d][N]
  for (int k = wave; k < d; k += W)
    for (int i = lane; i < n; i += 64) {
      const double *x = X + (long long)i * D, *mk = M + k * D;
      double acc = 0.0;
      for (int c = 0; c < D; ++c) acc = fma(mk[c], x[c] - mean[c], acc);
      Yt[(long long)k * n + i] = acc;
    }
  __syncthreads();
  for (int i = tid; i < n; i += T) {
    double q = 0.0;
    for (int k = 0; k < d; ++k) { const double y = Yt[(long long)k * n + i]; q += y * y / (psi[k] + 1.0); }
    const double f = sqrt((double)d / q);
    for (int k = 0; k < d; ++k) Yt[(long long)k * n + i] *= f;
  }
  __syncthreads();

  // ---- 7. S[i, j] = LLR(enrol y_i with n = 1, test y_j), fp64, rounded once
  const double cst = scal[0];
  for (int i = wave; i < n; i += W)
    for (int j = lane; j < n; j += 64) {
      double acc = 0.0;
      for (int k = 0; k < d; ++k) {
        const double e = Yt[(long long)k * n + i], t = Yt[(long long)k * n + j];
        const double df = t - ck[k] * e;
        acc += df * df * ivar[k] - t * t * ivar0[k];
      }
      S[(long long)i * n + j] = (float)(cst - 0.5 * acc);
    }
}

template <bool HBM, int T> int dp_attr(plda_handle *h, int bytes) {
  static DeviceOnce attr;
  if (attr.needed(h->device)) {
    PLDA_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&dpca_kernel<HBM, T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    bytes));
    attr.done(h->device);
  }
  return PLDA_OK;
}

int64_t dp_rec_bytes(int64_t n, int64_t D, int64_t m, bool hbm) {
  Layout size;
  DpRec rc;
  dp_layout(size, rc, n, D, m, hbm);
  return (int64_t)round_up((int64_t)size.end, 256);
}

// W = T^-1 T^-T and B = T^-1 diag(psi) T^-T of the installed model, cached per model epoch in h->dp_model
int dp_model(plda_handle *h, const char *fn, const double **W, const double **B) {
  const int D = h->Din;
  const size_t DD = (size_t)D * D;
  double *w = nullptr, *b = nullptr, *tinv = nullptr, *tmp = nullptr, *scr = nullptr;
  int *flag = nullptr;
  const bool had = h->dp_model.p != nullptr;
  const void *before = h->dp_model.p;
  PLDA_TRY(carve(h, h->dp_model, [&](Layout &l) { l.take(w, DD).take(b, DD).take(tinv, DD).take(tmp, DD).take(scr, 3 * DD).take(flag, 4); }));
  *W = w; *B = b;
  if (had && before == h->dp_model.p && h->dp_model_epoch == h->model_epoch && h->dp_model_D == D) return PLDA_OK;
  h->dp_model_D = 0;
  PLDA_HIP(h, hipMemsetAsync(flag, 0, 16, h->stream));
  PLDA_TRY(model_covariances_f64(h, h->d_transform.as<double>(), h->d_psi.as<double>(), D, w, b, tinv, tmp, scr, flag));
  int hflag = 0;
  PLDA_HIP(h, hipMemcpyAsync(&hflag, flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  if (hflag) return fail(h, PLDA_E_NUMERIC, "%s: the model's transform is singular (T^T T is not positive definite)", fn);
  h->dp_model_epoch = h->model_epoch;
  h->dp_model_D = D;
  return PLDA_OK;
}

// Enqueues steps 1 to 7 of recordings [r0, r1); block r starts at dscores + boff[r - r0].  `tables` keeps the host copies of
// the launch tables alive until the caller has synchronised.  h->dp_stat must have been initialised by the caller.
int dp_enqueue(plda_handle *h, const double *dX, const int64_t *offsets, int64_t r0, int64_t r1, double target, float *dscores,
               const int64_t *boff, int32_t *ddims, double *deig, const double *W, const double *B,
               std::vector<std::vector<DpRec>> &tables) {
  const int D = h->Din;
  const int64_t budget = cluster_budget(h);
  struct Group { int64_t first, n_lds, n_hbm; int m_lds; };
  std::vector<Group> groups;
  tables.emplace_back();
  std::vector<DpRec> &tab = tables.back();
  tab.resize((size_t)(r1 - r0));
  std::vector<int64_t> scr_off((size_t)(r1 - r0));
  int64_t need = 0;
  for (int64_t g0 = r0; g0 < r1;) {           // groups of consecutive recordings under the scratch budget, never fewer than one
    int64_t g1 = g0, cur = 0;
    while (g1 < r1) {
      const int64_t n = offsets[g1 + 1] - offsets[g1], m = std::min<int64_t>(n, D);
      const int64_t bytes = dp_rec_bytes(n, D, m, m > DP_LDS_MAX);
      if (cur && (cur + bytes > budget || g1 - g0 >= 32768)) break;
      scr_off[(size_t)(g1 - r0)] = cur;
      cur += bytes;
      ++g1;
    }
    need = std::max(need, cur);
    // the table of a group: its LDS-class recordings first, then its HBM-class ones (each in call order)
    Group G{g0 - r0, 0, 0, 0};
    size_t at = (size_t)(g0 - r0);
    for (int pass = 0; pass < 2; ++pass)
      for (int64_t r = g0; r < g1; ++r) {
        const int64_t n = offsets[r + 1] - offsets[r], m = std::min<int64_t>(n, D);
        const bool hbm = m > DP_LDS_MAX;
        if (hbm != (pass == 1)) continue;
        DpRec &rc = tab[at++];
        rc.xoff = offsets[r]; rc.boff = boff[r - r0]; rc.n = (int)n; rc.r = (int)r; rc.m = (int)m; rc.gram = n <= D ? 1 : 0;
        if (hbm) ++G.n_hbm; else { ++G.n_lds; G.m_lds = std::max(G.m_lds, (int)m); }
      }
    groups.push_back(G);
    g0 = g1;
  }
  PLDA_HIP(h, h->dp_scratch.reserve((size_t)need));
  for (DpRec &rc : tab) {                     // the pointers of every recording, from its place in its group's scratch
    Layout at{h->dp_scratch.as<char>() + scr_off[(size_t)(rc.r - r0)]};
    dp_layout(at, rc, rc.n, D, rc.m, rc.m > DP_LDS_MAX);
  }
  PLDA_HIP(h, h->dp_tab.reserve(tab.size() * sizeof(DpRec)));
  PLDA_HIP(h, hipMemcpyAsync(h->dp_tab.p, tab.data(), tab.size() * sizeof(DpRec), hipMemcpyHostToDevice, h->stream));
  const DpRec *dtab = h->dp_tab.as<DpRec>();
  unsigned long long *stat = h->dp_stat.as<unsigned long long>();
  PLDA_TRY((dp_attr<false, DP_T_LDS>(h, DP_LDS_BYTES)));
  const double *mean = h->d_mean.as<double>();
  TraceScope ts(h, "dense_pca.recordings");
  for (const Group &G : groups) {
    if (G.n_lds) {
      dpca_kernel<false, DP_T_LDS><<<(unsigned)G.n_lds, DP_T_LDS, (size_t)dp_lds_bytes(G.m_lds, false), h->stream>>>(
          dX, D, dtab + G.first, W, B, mean, target, stat, dscores, ddims, deig);
      PLDA_LAUNCH_CHECK(h);
    }
    if (G.n_hbm) {
      dpca_kernel<true, DP_T_HBM><<<(unsigned)G.n_hbm, DP_T_HBM, (size_t)dp_lds_bytes(DP_MAX_DIM, true), h->stream>>>(
          dX, D, dtab + G.first + G.n_lds, W, B, mean, target, stat, dscores, ddims, deig);
      PLDA_LAUNCH_CHECK(h);
    }
  }
  return PLDA_OK;
}

// zeroes the reject counter, sets the two "first failing recording" words to all ones, counts the non-finite rows of the call
int dp_begin(plda_handle *h, const double *dX, int64_t rows) {
  PLDA_HIP(h, h->dp_stat.reserve(24));
  PLDA_HIP(h, hipMemsetAsync(h->dp_stat.p, 0, 8, h->stream));
  PLDA_HIP(h, hipMemsetAsync(h->dp_stat.as<char>() + 8, 0xFF, 16, h->stream));
  TraceScope ts(h, "dense_pca.count", (double)rows * h->Din * 8.0, 2);
  dpca_count_kernel<<<(unsigned)ceil_div(rows, 4), 256, 0, h->stream>>>(dX, rows, h->Din, h->dp_stat.as<unsigned long long>());
  PLDA_LAUNCH_CHECK(h);
  return PLDA_OK;
}

// reads the status words behind everything enqueued (one synchronisation)
int dp_finish(plda_handle *h, const char *fn, int rc) {
  unsigned long long st[3] = {0, ~0ull, ~0ull};
  hipError_t e = hipMemcpyAsync(st, h->dp_stat.p, 24, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (rc != PLDA_OK) return rc;
  PLDA_HIP(h, e);
  if (st[0]) return fail(h, PLDA_E_INVAL, "%s: %llu row(s) with a non-finite element", fn, st[0]);
  if (st[1] != ~0ull) return fail(h, PLDA_E_NUMERIC, "%s: recording %llu: the projected within-class covariance is not positive definite", fn, st[1]);
  if (st[2] != ~0ull) return fail(h, PLDA_E_NUMERIC, "%s: recording %llu: the eigensolver did not converge in %d sweeps", fn, st[2], DP_MAX_SWEEPS);
  return PLDA_OK;
}

}  // namespace

int dense_pca_validate(plda_handle *h, const char *fn, const int64_t *offsets, int64_t R, double target, const int64_t *block_off,
                       bool blocks) {
  if (!h->fitted) return fail(h, PLDA_E_NOT_FITTED, "%s: model not fitted", fn);
  if (h->Dout != h->Din)
    return fail(h, PLDA_E_INVAL, "%s: the model is truncated (transform %d x %d) and has no covariances to project", fn, h->Dout, h->Din);
  if (h->Din > DP_MAX_DIM)
    return fail(h, PLDA_E_INVAL, "%s: model dimension %d (at most PLDA_DENSE_PCA_MAX_DIM = %d)", fn, h->Din, DP_MAX_DIM);
  if (!(target > 0.0 && target < 1.0)) return fail(h, PLDA_E_INVAL, "%s: target_energy = %g (must lie in (0, 1))", fn, target);
  if (R < 1 || R > (int64_t)0x7fffffff) return fail(h, PLDA_E_INVAL, "%s: R = %lld (must be 1 ... 2^31 - 1)", fn, (long long)R);
  if (!offsets) return fail(h, PLDA_E_INVAL, "%s: offsets is NULL", fn);
  PLDA_TRY(check_recordings(h, fn, offsets, R, PLDA_AHC_MAX, "PLDA_AHC_MAX"));
  return blocks ? check_block_off(h, fn, block_off, offsets, R) : PLDA_OK;
}

int dense_pca_plan(plda_handle *h, int64_t N, int32_t D, int32_t *out) {
  if (!out) return fail(h, PLDA_E_INVAL, "dense_pca_plan: out is NULL");
  if (N < 1 || N > PLDA_AHC_MAX) return fail(h, PLDA_E_INVAL, "dense_pca_plan: N = %lld (must be 1 ... PLDA_AHC_MAX = %d)", (long long)N, PLDA_AHC_MAX);
  if (D < 1 || D > DP_MAX_DIM) return fail(h, PLDA_E_INVAL, "dense_pca_plan: D = %d (must be 1 ... PLDA_DENSE_PCA_MAX_DIM = %d)", D, DP_MAX_DIM);
  const int64_t m = std::min<int64_t>(N, D);
  const bool hbm = m > DP_LDS_MAX;
  out[0] = hbm ? 1 : 0;
  out[1] = (int32_t)dp_rec_bytes(N, D, m, hbm);
  out[2] = (int32_t)m;
  out[3] = DP_LDS_MAX;
  return PLDA_OK;
}

int score_dense_pca_device(plda_handle *h, const double *dX, const int64_t *offsets, int64_t R, double target, float *dscores,
                           const int64_t *block_off, int32_t *ddims, double *deig) {
  const char *fn = "score_dense_pca";
  PLDA_TRY(dense_pca_validate(h, fn, offsets, R, target, block_off, true));
  if (!dX) return fail(h, PLDA_E_INVAL, "%s: X is NULL", fn);
  if (!dscores) return fail(h, PLDA_E_INVAL, "%s: scores is NULL", fn);
  const double *W = nullptr, *B = nullptr;
  PLDA_TRY(dp_model(h, fn, &W, &B));
  PLDA_TRY(dp_begin(h, dX, offsets[R]));
  std::vector<std::vector<DpRec>> tables;
  const int rc = dp_enqueue(h, dX, offsets, 0, R, target, dscores, block_off, ddims, deig, W, B, tables);
  return dp_finish(h, fn, rc);
}

int score_dense_pca_ahc_device(plda_handle *h, const double *dX, const int64_t *offsets, int64_t R, double target, const AhcArgs &a) {
  const char *fn = "score_dense_pca_ahc";
  PLDA_TRY(dense_pca_validate(h, fn, offsets, R, target, nullptr, false));
  if (!dX) return fail(h, PLDA_E_INVAL, "%s: X is NULL", fn);
  PLDA_TRY(ahc_validate(h, fn, nullptr, false, offsets, R, a));
  const double *W = nullptr, *B = nullptr;
  PLDA_TRY(dp_model(h, fn, &W, &B));
  // every slab of the walk is scored, clustered by the AHC's own matrix form (its blocks at the walk's boff, closing entry
  // included) and dropped
  SlabWalk walk(offsets, R, cluster_budget(h) / 4);
  PLDA_HIP(h, h->sn_slab.reserve((size_t)walk.largest * 4));
  float *slab = h->sn_slab.as<float>();
  PLDA_TRY(dp_begin(h, dX, offsets[R]));
  std::vector<std::vector<DpRec>> tables;
  std::vector<int64_t> rel;
  while (walk.next()) {
    const int64_t r0 = walk.r0, r1 = walk.r1;
    rel.clear();
    for (int64_t r = r0; r <= r1; ++r) rel.push_back(offsets[r] - offsets[r0]);
    const int rc = dp_enqueue(h, dX, offsets, r0, r1, target, slab, walk.boff.data(), nullptr, nullptr, W, B, tables);
    PLDA_TRY(dp_finish(h, fn, rc));           // (a failed recording leaves its block unwritten: nothing is clustered)
    PLDA_TRY(ahc_matrix_device(h, slab, walk.boff.data(), rel.data(), r1 - r0, a.from(r0, offsets[r0])));
  }
  return PLDA_OK;
}

}  // namespace plda
