// plda_amd/csrc/spectral.hip -- speaker clustering without a threshold: spectral clustering on a pruned k-nearest-neighbour
// affinity graph with the pruning value chosen by the normalised-maximum-eigengap rule (NME-SC, Park et al. 2020), batched
// over recordings (the contract is in include/plda_hip.h, the host model in tests/spectral_model.py).
//
//   cluster_count_kernel<SpecRec>  (common.hpp) the non-finite off-diagonal scores of every recording of the call (one integer
//                              counter; a call that meets one fails before anything else is enqueued)
//   spectral_sym_kernel        c(i, j) = ((double)S[i, j] + (double)S[j, i]) / 2 of one recording, once for all its pruning values
//   spectral_select_kernel<E>  one wave per row, the row's order keys in registers (E per lane): the p-th largest key by
//                              bisection over the 64 key bits (topn.hip's idea), then the j-ascending cut among the keys equal
//                              to it.  A row's neighbours are {j : key > cut key, or key == cut key and j <= cut j}.
//   spectral_laplacian_kernel  one workgroup per row: L = diag(deg) - (B + B^T) / 2 from the two cuts of every pair, and 2 deg
//   (sym_eig_auto_f64)         the spectrum and the eigenvectors, one recording and one pruning value at a time
//   spectral_pick_kernel       gaps, k_gap, g and r of this pruning value in plain fp64; if it beats the recording's best so far
//                              (r, then p_eff, then position) its leading columns and degrees replace the kept ones
//   spectral_kmeans_kernel     one workgroup per recording over the recordings of a group: farthest-first centres, Lloyd steps,
//                              labels renumbered by first occurrence; the embedding in LDS where N k doubles fit, else read
//                              from scratch (the arithmetic and its order are the same in both)
//
// Everything up to L is exact; steps 3, 4 and 6 of the contract are single fp64 operations in a fixed order (the file is built
// with -ffp-contract=off; no fast-math), so a recording's outputs depend on its block, its pruning values and N alone.
#include "common.hpp"
#include "slab_walk.hpp"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace plda {

namespace {

constexpr int SPEC_MAX = PLDA_SPECTRAL_MAX;
constexpr int SPEC_MAX_SPK = PLDA_SPECTRAL_MAX_SPK;
constexpr int SPEC_MAX_P = PLDA_SPECTRAL_MAX_P;
constexpr int KM_T = 256;                  // threads of the k-means workgroup
constexpr int KM_ROWS = SPEC_MAX / KM_T;   // rows per thread
constexpr int KM_U_BYTES = 64 * 1024;      // the embedding of a recording lives in LDS up to this size
static_assert(SPEC_MAX_SPK <= 64, "the k-means kernel numbers its centres with one wave");

// one recording of a launch (host-built, uploaded once per enqueue)
struct SpecRec {
  long long boff;    // first float of the block, relative to the scores pointer
  long long off;     // first segment (labels, embed, deg2)
  long long uoff;    // first double of the kept columns [n, max_speakers] in the group's scratch
  int n, r, kforce, doff;   // segments; recording; num_speakers (0: k_gap); first kept degree in the group's scratch
};
// the best pruning value of a recording so far
struct SpecState { double r; int p_eff, k_gap, have, pad; };

// the order key of a similarity: larger c <=> larger key, -0.0 == +0.0; a finite c never has key 0
__device__ __forceinline__ unsigned long long spec_key(double c) {
  unsigned long long b = (unsigned long long)__double_as_longlong(c);
  if ((b << 1) == 0) b = 0;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ __launch_bounds__(256) void spectral_sym_kernel(const float *__restrict__ blk, int n, double *__restrict__ Cm) {
  const long long total = (long long)n * n;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long i = e / n, j = e - i * n;
    Cm[e] = i == j ? 0.0 : ((double)blk[e] + (double)blk[j * n + i]) / 2.0;
  }
}

// four rows per workgroup, one wave each; 1 <= p <= n - 1
template <int E>
__global__ __launch_bounds__(256) void spectral_select_kernel(const double *__restrict__ Cm, int n, int p,
                                                              unsigned long long *__restrict__ cutkey, int *__restrict__ cutj) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const double *__restrict__ row = Cm + (long long)i * n;
  unsigned long long key[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int j = e * 64 + lane;
    key[e] = (j < n && j != i) ? spec_key(row[j]) : 0ull;
  }
  unsigned long long t = 0;       // the largest t with #{key >= t} >= p: the p-th largest key
  for (int bit = 63; bit >= 0; --bit) {
    const unsigned long long cand = t | (1ull << bit);
    int cnt = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) cnt += __popcll(__ballot(key[e] >= cand));
    if (cnt >= p) t = cand;
  }
  int above = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) above += __popcll(__ballot(key[e] > t));
  const int need = p - above;     // >= 1: the keys equal to t that are kept, by ascending j
  int run = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const unsigned long long mask = __ballot(key[e] == t);
    const int c = __popcll(mask);
    if (run < need && run + c >= need) {
      const int below = __popcll(mask & ((1ull << lane) - 1ull));
      if (((mask >> lane) & 1ull) && run + below == need - 1) { cutkey[i] = t; cutj[i] = e * 64 + lane; }
    }
    run += c;
  }
}

// grid n: row i of L and 2 deg_i
__global__ __launch_bounds__(256) void spectral_laplacian_kernel(const double *__restrict__ Cm, int n,
                                                                 const unsigned long long *__restrict__ cutkey,
                                                                 const int *__restrict__ cutj, double *__restrict__ L,
                                                                 int *__restrict__ deg2) {
  __shared__ int part[4];
  const int i = blockIdx.x, tid = threadIdx.x;
  const unsigned long long ti = cutkey[i];
  const int ji = cutj[i];
  int sum = 0;
  for (int j = tid; j < n; j += 256) {
    if (j == i) continue;
    const unsigned long long k = spec_key(Cm[(long long)i * n + j]);
    const unsigned long long tj = cutkey[j];
    const int a2 = ((k > ti || (k == ti && j <= ji)) ? 1 : 0) + ((k > tj || (k == tj && i <= cutj[j])) ? 1 : 0);
    L[(long long)i * n + j] = a2 ? -0.5 * (double)a2 : 0.0;
    sum += a2;
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
  if ((tid & 63) == 0) part[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) {
    const int tot = part[0] + part[1] + part[2] + part[3];
    deg2[i] = tot;
    L[(long long)i * n + i] = 0.5 * (double)tot;
  }
}

// one workgroup: s [n] descending, V eigenvectors in rows (row q belongs to s[q]).  n == 1: only the eig row is written.
__global__ __launch_bounds__(256) void spectral_pick_kernel(const double *__restrict__ s, const double *__restrict__ V, int n,
                                                            int p_eff, int ms, SpecState *__restrict__ state,
                                                            double *__restrict__ U, const int *__restrict__ deg2,
                                                            int *__restrict__ deg2b, double *__restrict__ eigrow) {
  __shared__ int take;
  const int tid = threadIdx.x;
  if (n == 1) {
    if (eigrow)
      for (int c = tid; c < ms + 2; c += 256) eigrow[c] = (c == 0 || c == ms + 1) ? 0.0 : (double)INFINITY;
    return;
  }
  if (tid == 0) {
    const int kp = min(ms, n - 1);
    int kg = 1;
    double eb = s[n - 2] - s[n - 1];
    for (int k = 2; k <= kp; ++k) {
      const double e = s[n - 1 - k] - s[n - k];
      if (e > eb) { eb = e; kg = k; }
    }
    const double lam_n = s[0];
    const double g = eb / (lam_n + 1e-10);
    const double r = g <= 0.0 ? (double)INFINITY : (double)p_eff / g;
    const SpecState st = *state;
    const bool better = !st.have || r < st.r || (r == st.r && p_eff < st.p_eff);
    if (better) { SpecState nw; nw.r = r; nw.p_eff = p_eff; nw.k_gap = kg; nw.have = 1; nw.pad = 0; *state = nw; }
    take = better ? 1 : 0;
  }
  if (eigrow) {
    const int have = min(ms + 1, n);
    for (int c = tid; c < ms + 2; c += 256) eigrow[c] = c == ms + 1 ? s[0] : (c < have ? s[n - 1 - c] : (double)INFINITY);
  }
  __syncthreads();
  if (!take) return;
  const int kk = min(ms, n);
  for (int c = 0; c < kk; ++c)
    for (int i = tid; i < n; i += 256) U[(long long)i * ms + c] = V[(long long)(n - 1 - c) * n + i];
  for (int i = tid; i < n; i += 256) deg2b[i] = deg2[i];
}

constexpr size_t km_lds_bytes(int nmax, int kmax) {
  const size_t u = (size_t)nmax * kmax * 8;
  return 8 * ((size_t)kmax * kmax + 4) + (u <= (size_t)KM_U_BYTES ? u : (size_t)KM_U_BYTES) + 4 * ((size_t)nmax + 64 + 64 + 8);
}
static_assert(km_lds_bytes(SPEC_MAX, SPEC_MAX_SPK) <= 160 * 1024, "the k-means state must fit one CU's LDS");

// one workgroup per recording of a group
__global__ __launch_bounds__(KM_T) void spectral_kmeans_kernel(const SpecRec *__restrict__ tab, const SpecState *__restrict__ state,
                                                               const double *__restrict__ Uall, const int *__restrict__ deg2b,
                                                               int ms, int max_iters, int *__restrict__ labels,
                                                               int *__restrict__ n_clusters, int *__restrict__ p_used,
                                                               int *__restrict__ k_gap, double *__restrict__ embed,
                                                               int *__restrict__ deg2) {
  extern __shared__ double spec_smem[];
  const SpecRec rc = tab[blockIdx.x];
  const int n = rc.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (n == 1) {
    if (tid == 0) {
      labels[rc.off] = 0;
      n_clusters[rc.r] = 1;
      if (p_used) p_used[rc.r] = 0;
      if (k_gap) k_gap[rc.r] = 1;
      if (deg2) deg2[rc.off] = 0;
    }
    if (embed)
      for (int c = tid; c < ms; c += KM_T) embed[rc.off * ms + c] = c == 0 ? 1.0 : 0.0;
    return;
  }
  const SpecState st = state[blockIdx.x];
  const int k = rc.kforce > 0 ? min(rc.kforce, n) : st.k_gap;
  const double *__restrict__ Ug = Uall + rc.uoff;
  const bool in_lds = (long long)n * k * 8 <= KM_U_BYTES;

  // LDS: cen[k k] | rv[4] | U[n k] (LDS class) | lab[n] | cnt[64] | first[64] | ri[4] | flag
  double *cen = spec_smem;
  double *rv = cen + k * k;
  double *Ul = rv + 4;
  int *lab = reinterpret_cast<int *>(Ul + (in_lds ? n * k : 0));
  int *cnt = lab + n;
  int *first = cnt + 64;
  int *ri = first + 64;
  int *flag = ri + 4;
  if (in_lds)
    for (int e = tid; e < n * k; e += KM_T) { const int i = e / k, c = e - i * k; Ul[e] = Ug[(long long)i * ms + c]; }
  const double *Up = in_lds ? Ul : Ug;
  const int us = in_lds ? k : ms;
  auto dist = [&](int i, int m) {
    double d = 0.0;
    for (int c = 0; c < k; ++c) {
      const double t = Up[(long long)i * us + c] - cen[m * k + c];
      d = d + t * t;
    }
    return d;
  };
  for (int i = tid; i < n; i += KM_T) lab[i] = -1;
  __syncthreads();
  for (int c = tid; c < k; c += KM_T) cen[c] = Up[c];      // centre 0 = row 0
  __syncthreads();
  double mind[KM_ROWS];
#pragma unroll
  for (int q = 0; q < KM_ROWS; ++q) {
    const int i = tid + q * KM_T;
    mind[q] = i < n ? dist(i, 0) : 0.0;
  }
  for (int t = 1; t < k; ++t) {     // the row farthest from the centres so far, ties to the lowest row
    double bv = 0.0;
    int bi = -1;
#pragma unroll
    for (int q = 0; q < KM_ROWS; ++q) {
      const int i = tid + q * KM_T;
      if (i < n && (bi < 0 || mind[q] > bv)) { bv = mind[q]; bi = i; }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
      const double ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    if (lane == 0) { rv[wave] = bv; ri[wave] = bi; }
    __syncthreads();
    bv = rv[0]; bi = ri[0];
#pragma unroll
    for (int w = 1; w < KM_T / 64; ++w) {
      const double ov = rv[w];
      const int oi = ri[w];
      if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    for (int c = tid; c < k; c += KM_T) cen[t * k + c] = Up[(long long)bi * us + c];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < KM_ROWS; ++q) {
      const int i = tid + q * KM_T;
      if (i < n) { const double d = dist(i, t); if (d < mind[q]) mind[q] = d; }
    }
  }
  for (int it = 0; it < max_iters; ++it) {
    if (tid == 0) *flag = 0;
    __syncthreads();
    for (int i = tid; i < n; i += KM_T) {      // nearest centre, ties to the lowest centre
      double bd = dist(i, 0);
      int bm = 0;
      for (int m = 1; m < k; ++m) { const double d = dist(i, m); if (d < bd) { bd = d; bm = m; } }
      if (bm != lab[i]) { lab[i] = bm; *flag = 1; }
    }
    __syncthreads();
    if (!*flag) break;                         // (the flag is cleared again behind the barrier that ends this step)
    for (int e = tid; e < k * k; e += KM_T) {  // centre m, coordinate c: the members' sum by ascending row / the count
      const int m = e / k, c = e - m * k;
      double sum = 0.0;
      int members = 0;
      for (int i = 0; i < n; ++i)
        if (lab[i] == m) { sum = sum + Up[(long long)i * us + c]; ++members; }
      if (members > 0) cen[e] = sum / (double)members;
    }
    __syncthreads();
  }
  // renumbering by first occurrence
  if (tid < 64) first[tid] = 0x7fffffff;
  __syncthreads();
  for (int i = tid; i < n; i += KM_T) atomicMin(&first[lab[i]], i);
  __syncthreads();
  if (tid < 64) {
    const int f = first[tid];
    int rank = 0, used = 0;
    for (int m = 0; m < k; ++m) {
      const int fm = first[m];
      if (fm != 0x7fffffff) { ++used; if (fm < f) ++rank; }
    }
    cnt[tid] = rank;
    if (tid == 0) {
      n_clusters[rc.r] = used;
      if (p_used) p_used[rc.r] = st.p_eff;
      if (k_gap) k_gap[rc.r] = st.k_gap;
    }
  }
  __syncthreads();
  for (int i = tid; i < n; i += KM_T) {
    labels[rc.off + i] = cnt[lab[i]];
    if (deg2) deg2[rc.off + i] = deg2b[rc.doff + i];
  }
  if (embed)
    for (long long e = tid; e < (long long)n * ms; e += KM_T) {
      const int i = (int)(e / ms), c = (int)(e - (long long)i * ms);
      embed[rc.off * ms + e] = c < k ? Up[(long long)i * us + c] : 0.0;
    }
}

int spectral_kmeans_attr(plda_handle *h) {
  static DeviceOnce attr;
  if (attr.needed(h->device)) {
    PLDA_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&spectral_kmeans_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)km_lds_bytes(SPEC_MAX, SPEC_MAX_SPK)));
    attr.done(h->device);
  }
  return PLDA_OK;
}

int spec_class(int n) { int e = 1; while (e * 64 < n) e *= 2; return e; }     // keys per lane of the selection kernel

struct SpecGroup { int64_t first, count, segs; int nmax; };   // table entries [first, first + count), their segments, largest N

// the arrays of h->ahc_scratch (the AHC's own scratch: one clustering call runs at a time and each carves it anew): the working set of one eigenproblem, then what a group keeps until its k-means
struct SpecWork {
  double *Cm, *L, *V, *s;
  unsigned long long *cutkey;
  int *cutj, *deg2;
  double *U;
  int *deg2b;
  SpecState *state;
  void lay(Layout &c, size_t nmax, size_t gsegs, size_t grecs, size_t ms) {
    c.take(Cm, nmax * nmax).take(L, nmax * nmax).take(V, nmax * nmax).take(s, nmax).take(cutkey, nmax).take(cutj, nmax).take(deg2, nmax);
    c.take(U, gsegs * ms).take(deg2b, gsegs).take(state, grecs);
  }
};

// the table of recordings [r0, r1) (blocks at boff[r - r0]) in groups whose kept columns fit cluster_budget, uploaded; `tables` keeps the host copy
// alive until the caller has synchronised
int spectral_table(plda_handle *h, const int64_t *boff, const SpectralArgs &a, int64_t r0, int64_t r1,
                   std::vector<std::vector<SpecRec>> &tables, std::vector<SpecGroup> &groups, const SpecRec **dtab,
                   unsigned long long **dbad) {
  tables.emplace_back();
  std::vector<SpecRec> &tab = tables.back();
  tab.reserve((size_t)(r1 - r0));
  groups.clear();
  const int64_t budget = cluster_budget(h);
  SpecGroup g{0, 0, 0, 0};
  int64_t bytes = 0;
  for (int64_t r = r0; r < r1; ++r) {
    const int64_t n = a.offsets[r + 1] - a.offsets[r];
    const int64_t need = n * a.max_spk * 8 + n * 4 + (int64_t)sizeof(SpecState);
    if (g.count && (bytes + need > budget || g.count >= 65535)) {
      groups.push_back(g);
      g = SpecGroup{(int64_t)tab.size(), 0, 0, 0};
      bytes = 0;
    }
    SpecRec rc;
    rc.boff = boff[r - r0]; rc.off = a.offsets[r]; rc.uoff = g.segs * a.max_spk; rc.n = (int)n; rc.r = (int)r;
    rc.kforce = a.num_spk ? a.num_spk[r] : 0; rc.doff = (int)g.segs;
    tab.push_back(rc);
    ++g.count; g.segs += n; g.nmax = std::max(g.nmax, (int)n); bytes += need;
  }
  if (g.count) groups.push_back(g);
  SpecRec *dt = nullptr;
  unsigned long long *db = nullptr;
  const size_t cnt = tab.size();
  PLDA_TRY(carve(h, h->ahc_tab, [&](Layout &c) { c.take(db, 1).take(dt, cnt); }));
  PLDA_HIP(h, hipMemcpyAsync(dt, tab.data(), cnt * sizeof(SpecRec), hipMemcpyHostToDevice, h->stream));
  *dtab = dt;
  *dbad = db;
  return PLDA_OK;
}

int spectral_select(plda_handle *h, const double *Cm, int n, int p, unsigned long long *cutkey, int *cutj) {
  const unsigned grid = (unsigned)ceil_div(n, 4);
  switch (spec_class(n)) {
#define SEL(E) case E: spectral_select_kernel<E><<<grid, 256, 0, h->stream>>>(Cm, n, p, cutkey, cutj); break
    SEL(1); SEL(2); SEL(4); SEL(8); SEL(16);
    default: spectral_select_kernel<32><<<grid, 256, 0, h->stream>>>(Cm, n, p, cutkey, cutj); break;
#undef SEL
  }
  PLDA_LAUNCH_CHECK(h);
  return PLDA_OK;
}

// Enqueues the clustering of the recordings of one table, group by group.  The eigensolver synchronises the stream once per
// problem (it reads its own status word).
int spectral_enqueue(plda_handle *h, const char *fn, const float *dscores, const SpectralArgs &a, const std::vector<SpecRec> &tab,
                     const SpecRec *dtab, const std::vector<SpecGroup> &groups) {
  const int ms = a.max_spk, P = a.P;
  size_t nmax = 0, gsegs = 0, grecs = 0;
  for (const SpecGroup &g : groups) {
    nmax = std::max(nmax, (size_t)g.nmax); gsegs = std::max(gsegs, (size_t)g.segs); grecs = std::max(grecs, (size_t)g.count);
  }
  if (nmax == 1) nmax = 0;      // (no eigenproblem in the call)
  SpecWork w;
  PLDA_TRY(carve(h, h->ahc_scratch, [&](Layout &c) { w.lay(c, nmax, gsegs, grecs, (size_t)ms); }));
  PLDA_TRY(spectral_kmeans_attr(h));
  for (const SpecGroup &g : groups) {
    PLDA_HIP(h, hipMemsetAsync(w.state, 0, (size_t)g.count * sizeof(SpecState), h->stream));
    for (int64_t q = 0; q < g.count; ++q) {
      const SpecRec &rc = tab[(size_t)(g.first + q)];
      const int n = rc.n;
      const int32_t *prow = a.p_table + (int64_t)rc.r * P;
      double *eig_r = a.eig ? a.eig + (int64_t)rc.r * P * (ms + 2) : nullptr;
      if (n == 1) {
        for (int pos = 0; eig_r && pos < P; ++pos) {
          spectral_pick_kernel<<<1, 256, 0, h->stream>>>(nullptr, nullptr, 1, 0, ms, nullptr, nullptr, nullptr, nullptr,
                                                         eig_r + (int64_t)pos * (ms + 2));
          PLDA_LAUNCH_CHECK(h);
        }
        continue;
      }
      TraceScope ts(h, "spectral.graph");
      const unsigned sg = (unsigned)std::min<int64_t>(ceil_div((int64_t)n * n, 1024), 1024);
      spectral_sym_kernel<<<sg, 256, 0, h->stream>>>(dscores + rc.boff, n, w.Cm);
      PLDA_LAUNCH_CHECK(h);
      for (int pos = 0; pos < P; ++pos) {
        const int p_eff = std::min<int>(prow[pos], n - 1);
        int dup = -1;
        for (int e = 0; e < pos && dup < 0; ++e)
          if (std::min<int>(prow[e], n - 1) == p_eff) dup = e;
        double *eigrow = eig_r ? eig_r + (int64_t)pos * (ms + 2) : nullptr;
        if (dup >= 0) {       // the same graph: the same row, and the earlier position keeps the tie
          if (eigrow)
            PLDA_HIP(h, hipMemcpyAsync(eigrow, eig_r + (int64_t)dup * (ms + 2), (size_t)(ms + 2) * 8, hipMemcpyDeviceToDevice, h->stream));
          continue;
        }
        if (pos) ts.next("spectral.graph");
        PLDA_TRY(spectral_select(h, w.Cm, n, p_eff, w.cutkey, w.cutj));
        spectral_laplacian_kernel<<<(unsigned)n, 256, 0, h->stream>>>(w.Cm, n, w.cutkey, w.cutj, w.L, w.deg2);
        PLDA_LAUNCH_CHECK(h);
        ts.next("spectral.eig");
        const int erc = sym_eig_auto_f64(h, w.L, n, w.s, w.V);
        if (erc == PLDA_E_NUMERIC || erc == PLDA_E_INVAL) {
          const std::string why = h->err;
          return fail(h, PLDA_E_NUMERIC, "%s: the eigensolver gave up on recording %d (N = %d, p = %d): %s", fn, rc.r, n, p_eff, why.c_str());
        }
        PLDA_TRY(erc);
        ts.next("spectral.pick");
        spectral_pick_kernel<<<1, 256, 0, h->stream>>>(w.s, w.V, n, p_eff, ms, w.state + q, w.U + rc.uoff, w.deg2, w.deg2b + rc.doff, eigrow);
        PLDA_LAUNCH_CHECK(h);
      }
    }
    TraceScope ts(h, "spectral.kmeans");
    spectral_kmeans_kernel<<<(unsigned)g.count, KM_T, km_lds_bytes(g.nmax, std::min(ms, g.nmax)), h->stream>>>(
        dtab + g.first, w.state, w.U, w.deg2b, ms, a.max_iters, a.labels, a.n_clusters, a.p_used, a.k_gap, a.embed, a.deg2);
    PLDA_LAUNCH_CHECK(h);
  }
  return PLDA_OK;
}

}  // namespace

int spectral_validate(plda_handle *h, const char *fn, const int64_t *block_off, bool blocks, const SpectralArgs &a) {
  const int64_t R = a.R;
  if (R < 1) return fail(h, PLDA_E_INVAL, "%s: R = %lld (must be >= 1)", fn, (long long)R);
  if (R > (int64_t)0x7fffffff) return fail(h, PLDA_E_INVAL, "%s: R = %lld (at most 2^31 - 1)", fn, (long long)R);
  if (!a.offsets) return fail(h, PLDA_E_INVAL, "%s: offsets is NULL", fn);
  if (!a.p_table) return fail(h, PLDA_E_INVAL, "%s: p_table is NULL", fn);
  if (!a.labels) return fail(h, PLDA_E_INVAL, "%s: labels is NULL", fn);
  if (!a.n_clusters) return fail(h, PLDA_E_INVAL, "%s: n_clusters is NULL", fn);
  if (a.P < 1 || a.P > SPEC_MAX_P) return fail(h, PLDA_E_INVAL, "%s: P = %d (must be 1 ... PLDA_SPECTRAL_MAX_P = %d)", fn, a.P, SPEC_MAX_P);
  if (a.max_spk < 1 || a.max_spk > SPEC_MAX_SPK)
    return fail(h, PLDA_E_INVAL, "%s: max_speakers = %d (must be 1 ... PLDA_SPECTRAL_MAX_SPK = %d)", fn, a.max_spk, SPEC_MAX_SPK);
  if (a.max_iters < 1 || a.max_iters > 1000) return fail(h, PLDA_E_INVAL, "%s: max_iters = %d (must be 1 ... 1000)", fn, a.max_iters);
  PLDA_TRY(check_recordings(h, fn, a.offsets, R, SPEC_MAX, "PLDA_SPECTRAL_MAX", [&](int64_t r, int64_t) {
    for (int q = 0; q < a.P; ++q)
      if (a.p_table[r * a.P + q] < 1)
        return fail(h, PLDA_E_INVAL, "%s: p_table[%lld, %d] = %d (must be >= 1)", fn, (long long)r, q, (int)a.p_table[r * a.P + q]);
    if (a.num_spk && (a.num_spk[r] < 0 || a.num_spk[r] > a.max_spk))
      return fail(h, PLDA_E_INVAL, "%s: num_speakers[%lld] = %d (must be 0 ... max_speakers = %d)", fn, (long long)r, (int)a.num_spk[r],
                  a.max_spk);
    return (int)PLDA_OK;
  }));
  return blocks ? check_block_off(h, fn, block_off, a.offsets, R) : PLDA_OK;
}

int spectral_plan(plda_handle *h, int64_t N, int32_t k, int32_t *out) {
  if (!out) return fail(h, PLDA_E_INVAL, "spectral_plan: out is NULL");
  if (N < 1 || N > SPEC_MAX) return fail(h, PLDA_E_INVAL, "spectral_plan: N = %lld (must be 1 ... PLDA_SPECTRAL_MAX = %d)", (long long)N, SPEC_MAX);
  if (k < 1 || k > SPEC_MAX_SPK) return fail(h, PLDA_E_INVAL, "spectral_plan: k = %d (must be 1 ... PLDA_SPECTRAL_MAX_SPK = %d)", (int)k, SPEC_MAX_SPK);
  const int e = spec_class((int)N);
  out[0] = e;
  out[1] = e * 64;
  out[2] = N * k * 8 <= KM_U_BYTES ? 0 : 1;
  out[3] = (int32_t)std::min<int64_t>(KM_U_BYTES / (8 * k), SPEC_MAX);
  Layout size;
  SpecWork w;
  w.lay(size, N > 1 ? (size_t)N : 0, 0, 0, 0);
  out[4] = (int32_t)size.end;
  return PLDA_OK;
}

int spectral_matrix_device(plda_handle *h, const float *dscores, const int64_t *block_off, const SpectralArgs &a) {
  const char *fn = "spectral_matrix";
  if (!dscores) return fail(h, PLDA_E_INVAL, "%s: scores is NULL", fn);
  PLDA_TRY(spectral_validate(h, fn, block_off, true, a));
  std::vector<std::vector<SpecRec>> tables;
  std::vector<SpecGroup> groups;
  const SpecRec *dtab;
  unsigned long long *dbad;
  PLDA_TRY(spectral_table(h, block_off, a, 0, a.R, tables, groups, &dtab, &dbad));
  PLDA_HIP(h, hipMemsetAsync(dbad, 0, 8, h->stream));
  int rc = cluster_count_enqueue(h, dscores, tables.back().data(), a.R, dtab, dbad);
  if (rc == PLDA_OK) rc = cluster_counted(h, fn, dbad);      // (nothing of the clustering is enqueued before it is known to be zero)
  if (rc == PLDA_OK) rc = spectral_enqueue(h, fn, dscores, a, tables.back(), dtab, groups);
  const hipError_t e = hipStreamSynchronize(h->stream);      // (the host tables go with this frame)
  PLDA_TRY(rc);
  PLDA_HIP(h, e);
  return PLDA_OK;
}

int score_spectral_device(plda_handle *h, const double *dX, const SpectralArgs &a) {
  const char *fn = "score_spectral";
  if (!can_score(h)) return fail(h, PLDA_E_NOT_FITTED, "%s: model not fitted", fn);
  if (!dX) return fail(h, PLDA_E_INVAL, "%s: X is NULL", fn);
  PLDA_TRY(spectral_validate(h, fn, nullptr, false, a));
  SlabWalk walk(a.offsets, a.R, cluster_budget(h) / 4);
  PLDA_HIP(h, h->sn_slab.reserve((size_t)walk.largest * 4));
  float *slab = h->sn_slab.as<float>();
  h->prep_valid = false;           // (every block packs its own two sides)
  std::vector<std::vector<SpecRec>> tables;
  std::vector<SpecGroup> groups;
  // pass 0 (only when the call takes several slabs): every block scored and counted, so that a non-finite score anywhere
  // fails the call before the first output is written; pass 1: scored (again), counted if pass 0 did not run, clustered
  int rc = PLDA_OK;
  for (int pass = walk.slabs > 1 ? 0 : 1; pass < 2 && rc == PLDA_OK; ++pass) {
    walk.rewind();
    while (rc == PLDA_OK && walk.next()) {
      rc = score_blocks_device(h, "spectral.block_gemm", dX, a.offsets, walk.r0, walk.r1, walk.boff.data(), slab);
      const SpecRec *dtab = nullptr;
      unsigned long long *dbad = nullptr;
      if (rc == PLDA_OK) rc = spectral_table(h, walk.boff.data(), a, walk.r0, walk.r1, tables, groups, &dtab, &dbad);
      if (rc == PLDA_OK && (pass == 0 || walk.slabs == 1)) {
        const hipError_t e = hipMemsetAsync(dbad, 0, 8, h->stream);
        if (e != hipSuccess) rc = hip_fail(h, e, "hipMemsetAsync", __FILE__, __LINE__);
        if (rc == PLDA_OK) rc = cluster_count_enqueue(h, slab, tables.back().data(), walk.r1 - walk.r0, dtab, dbad);
        if (rc == PLDA_OK) rc = cluster_counted(h, fn, dbad);
      }
      if (rc == PLDA_OK && pass == 1) rc = spectral_enqueue(h, fn, slab, a, tables.back(), dtab, groups);
    }
  }
  const hipError_t e = hipStreamSynchronize(h->stream);
  PLDA_TRY(rc);
  PLDA_HIP(h, e);
  return PLDA_OK;
}

}  // namespace plda
