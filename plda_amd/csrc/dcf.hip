// plda_amd/csrc/dcf.hip -- exact minimum detection cost (minDCF) of labelled trials at several operating points, without
// sorting (include/plda_hip.h, "exact minimum detection cost"; pinned by tests/mindcf_model.py).
//
// The EER follows ONE crossing down the three key levels (eer.hip), because FRR - FAR is monotone.  The cost
// C(k) = a miss(k) / Np + b fa(k) / Nn is not, so the refinement here is a branch and bound: after a level every bin edge is a
// cut with exact counts (-> incumbents), and a bin is refined further only if it holds both classes and the cost at
// (miss at its lower edge, fa at its upper edge) -- a bound with no tolerance, the expression being monotone in both counts
// also after rounding -- does not exceed the incumbent.  The host step is plda_min_dcf_step (pure; below).
//
// Level 0 is the EER's full histogram (eer_pass, has_prefix = 0; trial_source.hpp).  Every pass reaches its kernels through
// for_each_piece over a TrialSource (trial_source.hpp) with this file's own grid arithmetic per piece; the operand form's
// source comes from operand_source (operand_slabs.hip); the sharded form's sums go through reduce_block_or_poison (eer.hip).
// The new kernels:
//  * dcf_multi_strip_kernel / dcf_multi_flat_kernel: ONE read of the scores refines up to DCF_S = 8 nodes.  The sorted node
//    prefixes sit in LDS; a key outside [first, last] prefix is done after two compares, the others find their slot by three
//    LDS compares; per slot and class a 2048-bin histogram in LDS (n slots x 16 KiB of dynamic LDS: 128 KiB at n = 8, and
//    only what the launch needs when there are fewer nodes, so that more workgroups fit a CU).  1024 threads per workgroup
//    (the strip form: 256 threads across 1024 columns, as eer_hist_strip_kernel, times four row groups), because at 128 KiB
//    one workgroup is all a CU holds.  Integer LDS atomics, 64-bit global merge; no floating-point atomics.
//  * dcf_compact_strip_kernel: the append of eer_window_strip_kernel with "inside the window" replaced by "under one of up
//    to 1024 sorted prefixes" (binary search in LDS).  The level histograms give the lists' lengths exactly beforehand.
//  * dcf_neighbour_kernel: per winning cut the largest key <= its edge and the smallest key above it (registers, wave
//    reduction, one atomic pair per wave and cut).
// More than DCF_S survivors: further launches over the same level.  Every path ends with all surviving ranges resolved to
// single keys: level 2's bins are keys.
#include "trial_source.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace plda {

constexpr int DCF_S = 8;                 // nodes per read
constexpr int DCF_T = 1024;              // threads per workgroup of the multi-prefix kernels
constexpr int DCF_CMAX = 1024;           // prefixes of one compaction read (4 KiB of LDS beside the 48 KiB stage: three workgroups per CU)
constexpr unsigned long long DCF_LIST_CAP = 1ull << 26;   // compact when at most this many trials survive
constexpr int64_t DCF_CHUNK = 4096;      // nodes per host step (128 MiB of host counters)
static const int DCF_SHIFT[3] = {21, 10, 0}, DCF_BITS[3] = {11, 11, 10};

typedef float f32x4d __attribute__((ext_vector_type(4)));

struct DcfPrefixes { unsigned p[DCF_S]; int n; };

// LDS: [n][2][EER_BINS] counters, then the n sorted prefixes
__device__ __forceinline__ void dcf_account(unsigned *__restrict__ lh, const unsigned *__restrict__ sp, int n, unsigned pmin,
                                            unsigned pmax, int hi_shift, int shift, unsigned mask, float sc, int cls) {
  const unsigned k = score_key(sc);
  const unsigned q = k >> hi_shift;
  if (q < pmin || q > pmax) return;
  int lo = 0;                                      // the last slot whose prefix is <= q (sp[0] = pmin <= q)
#pragma unroll
  for (int step = DCF_S / 2; step > 0; step >>= 1) {
    const int j = lo + step;
    if (j < n && sp[j] <= q) lo = j;
  }
  if (sp[lo] != q) return;
  atomicAdd(&lh[(lo * 2 + cls) * EER_BINS + (int)((k >> shift) & mask)], 1u);
}

__device__ __forceinline__ void dcf_lds_init(unsigned *lh, unsigned *sp, const DcfPrefixes &pf) {
  for (int i = threadIdx.x; i < pf.n * 2 * EER_BINS; i += DCF_T) lh[i] = 0;
  if (threadIdx.x < DCF_S) sp[threadIdx.x] = threadIdx.x < pf.n ? pf.p[threadIdx.x] : 0xffffffffu;
  __syncthreads();
}
__device__ __forceinline__ void dcf_lds_merge(const unsigned *lh, int n, unsigned long long *__restrict__ hist) {
  __syncthreads();
  for (int i = threadIdx.x; i < n * 2 * EER_BINS; i += DCF_T) {
    const unsigned c = lh[i];
    if (c) atomicAdd(hist + i, (unsigned long long)c);
  }
}

// hist: [n][2][EER_BINS].  Matrix form: a workgroup owns EER_STRIP columns (4 per thread, their speaker ids in registers)
// and a slice of the rows; its four row groups take four rows each in turn.
__global__ __launch_bounds__(DCF_T) void dcf_multi_strip_kernel(const float *__restrict__ scores, int64_t ld, int64_t M, int64_t Nt,
                                                                const int64_t *__restrict__ espk, const int64_t *__restrict__ tspk,
                                                                int64_t rows_per_wg, int shift, int nbits, DcfPrefixes pf,
                                                                unsigned long long *__restrict__ hist) {
  extern __shared__ unsigned dcf_lds[];
  unsigned *lh = dcf_lds, *sp = dcf_lds + pf.n * 2 * EER_BINS;
  dcf_lds_init(lh, sp, pf);
  const unsigned mask = (1u << nbits) - 1u;
  const int hi_shift = shift + nbits;
  const unsigned pmin = pf.p[0], pmax = pf.p[pf.n - 1];
  const int64_t strips = (Nt + EER_STRIP - 1) / EER_STRIP;
  const int64_t strip = blockIdx.x % strips, slice = blockIdx.x / strips;
  const int ct = threadIdx.x & 255, rg = threadIdx.x >> 8;
  const int64_t col = strip * EER_STRIP + (int64_t)ct * 4;
  const int64_t r0 = slice * rows_per_wg, r1 = (r0 + rows_per_wg < M) ? r0 + rows_per_wg : M;
  int64_t ts[4];
  bool ok[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    ok[e] = col + e < Nt;
    ts[e] = ok[e] ? tspk[col + e] : 0;
  }
  const bool vec = ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(scores) & 15) == 0) && ok[3];
  for (int64_t row = r0 + 4 * rg; row < r1; row += 16) {
    float v[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (row + u >= r1) break;
      const float *src = scores + (row + u) * ld + col;
      if (vec) {
        const f32x4d x = __builtin_nontemporal_load(reinterpret_cast<const f32x4d *>(src));
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
        if (ok[e]) dcf_account(lh, sp, pf.n, pmin, pmax, hi_shift, shift, mask, v[u][e], ts[e] == spk ? 1 : 0);
    }
  }
  dcf_lds_merge(lh, pf.n, hist);
}

// Flat list of scores of one class.
__global__ __launch_bounds__(DCF_T) void dcf_multi_flat_kernel(const float *__restrict__ scores, int64_t n, int cls, int shift,
                                                               int nbits, DcfPrefixes pf, unsigned long long *__restrict__ hist) {
  extern __shared__ unsigned dcf_lds[];
  unsigned *lh = dcf_lds, *sp = dcf_lds + pf.n * 2 * EER_BINS;
  dcf_lds_init(lh, sp, pf);
  const unsigned mask = (1u << nbits) - 1u;
  const int hi_shift = shift + nbits;
  const unsigned pmin = pf.p[0], pmax = pf.p[pf.n - 1];
  for (int64_t idx = (int64_t)blockIdx.x * DCF_T + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * DCF_T)
    dcf_account(lh, sp, pf.n, pmin, pmax, hi_shift, shift, mask, scores[idx], cls);
  dcf_lds_merge(lh, pf.n, hist);
}

// One read appends every trial whose key lies under one of the np sorted prefixes (key >> hi_shift) to its class's list.
// Staging as eer_window_strip_kernel: a slot in the wave's LDS stage per hit, 512+ scores leave behind ONE global atomic.
// cursor[2]: scores appended per class; a write beyond cap is dropped (the caller compares the cursors with the exact
// lengths the histograms gave: they must be equal).
constexpr int DCF_WBUF = 1536;
__global__ __launch_bounds__(256) void dcf_compact_strip_kernel(const float *__restrict__ scores, int64_t ld, int64_t M, int64_t Nt,
                                                                const int64_t *__restrict__ espk, const int64_t *__restrict__ tspk,
                                                                int64_t rows_per_wg, int hi_shift, const unsigned *__restrict__ prefixes,
                                                                int np, unsigned long long *__restrict__ cursor,
                                                                float *__restrict__ list0, float *__restrict__ list1,
                                                                unsigned long long cap0, unsigned long long cap1) {
  __shared__ float stage[4][2][DCF_WBUF];
  __shared__ unsigned sp[DCF_CMAX];
  __shared__ int fillc[4][2];
  for (int i = threadIdx.x; i < np; i += 256) sp[i] = prefixes[i];
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
  int *const fc = fillc[wave];
  if (lane < 2) fc[lane] = 0;
  __syncthreads();
  const unsigned pmin = sp[0], pmax = sp[np - 1];
  auto flush = [&](int c) {
    const int n = __builtin_amdgcn_readfirstlane(fc[c]);
    if (n == 0) return;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&cursor[c], (unsigned long long)n);
    base = __shfl(base, 0);
    float *dst = c ? list1 : list0;
    const unsigned long long cap = c ? cap1 : cap0;
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
        const f32x4d x = __builtin_nontemporal_load(reinterpret_cast<const f32x4d *>(src));
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
      for (int e = 0; e < 4; ++e) {
        if (!ok[e]) continue;
        const unsigned q = score_key(v[u][e]) >> hi_shift;
        if (q < pmin || q > pmax) continue;
        int lo = 0, hi = np - 1;                   // the last prefix <= q
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (sp[mid] <= q) lo = mid; else hi = mid - 1;
        }
        if (sp[lo] != q) continue;
        const int c = ts[e] == spk ? 1 : 0;
        const int slot = atomicAdd(&fc[c], 1);
        stage[wave][c][slot] = v[u][e];
      }
    }
    if (__builtin_amdgcn_readfirstlane(fc[0]) > DCF_WBUF - 1024) flush(0);
    if (__builtin_amdgcn_readfirstlane(fc[1]) > DCF_WBUF - 1024) flush(1);
  }
  flush(0);
  flush(1);
}

// Per cut p < P: nb[2 p] = max key <= edge[p], nb[2 p + 1] = min key > edge[p] (a cut without an edge: every key is above).
struct DcfEdges { unsigned e[PLDA_MIN_DCF_MAX_POINTS]; unsigned has; };
__global__ __launch_bounds__(256) void dcf_neighbour_kernel(const float *__restrict__ scores, int64_t ld, int64_t M, int64_t Nt,
                                                            DcfEdges ed, unsigned *__restrict__ nb) {
  constexpr int P = PLDA_MIN_DCF_MAX_POINTS;
  unsigned lo[P], hi[P];
#pragma unroll
  for (int p = 0; p < P; ++p) { lo[p] = 0u; hi[p] = 0xffffffffu; }
  const int64_t total = M * Nt;
  const bool flat = ld == Nt;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const unsigned k = score_key(flat ? scores[idx] : scores[(idx / Nt) * ld + idx % Nt]);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const bool le = ((ed.has >> p) & 1u) && k <= ed.e[p];
      lo[p] = (le && k > lo[p]) ? k : lo[p];
      hi[p] = (!le && k < hi[p]) ? k : hi[p];
    }
  }
#pragma unroll
  for (int p = 0; p < P; ++p) {
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned a = __shfl_xor(lo[p], o), b = __shfl_xor(hi[p], o);
      lo[p] = a > lo[p] ? a : lo[p]; hi[p] = b < hi[p] ? b : hi[p];
    }
    if ((threadIdx.x & 63) == 0) {
      if (lo[p]) atomicMax(nb + 2 * p, lo[p]);
      if (hi[p] != 0xffffffffu) atomicMin(nb + 2 * p + 1, hi[p]);
    }
  }
}

// ------------------------------------------------------------------------------------ the host step (pure)
#pragma clang fp contract(off)
static inline double dcf_value(double a, double b, unsigned long long miss, unsigned long long fa, double Np, double Nn) {
  return (a * (double)miss) / Np + (b * (double)fa) / Nn;
}

static bool dcf_points_ok(int n_points, const plda_dcf_point *pts) {
  if (!pts || n_points < 1 || n_points > PLDA_MIN_DCF_MAX_POINTS) return false;
  for (int p = 0; p < n_points; ++p)
    if (!(pts[p].prior > 0.0 && pts[p].prior < 1.0 && pts[p].c_miss > 0.0 && pts[p].c_fa > 0.0 && std::isfinite(pts[p].c_miss) &&
          std::isfinite(pts[p].c_fa)))
      return false;
  return true;
}

int min_dcf_step(int level, int64_t n_nodes, const plda_min_dcf_node *nodes, const uint64_t *hist, int n_points,
                 const plda_dcf_point *pts, plda_min_dcf_state *st, int64_t cap_next, plda_min_dcf_node *next, int64_t *n_next) {
  if (level < 0 || level > 2 || n_nodes < 1 || !nodes || !hist || !st || !n_next || !dcf_points_ok(n_points, pts)) return PLDA_E_INVAL;
  if (level == 0 && n_nodes != 1) return PLDA_E_INVAL;
  const int nb = 1 << DCF_BITS[level], shift = DCF_SHIFT[level];
  *n_next = 0;
  if (level == 0) {
    uint64_t Np = 0, Nn = 0, bad = 0;
    for (int b = 0; b < nb; ++b) { Nn += hist[b]; Np += hist[EER_BINS + b]; }
    for (int b = 0; b < 4; ++b) bad += hist[b] + hist[EER_BINS + b] + hist[2044 + b] + hist[EER_BINS + 2044 + b];
    st->np = Np; st->nn = Nn; st->nonfinite = bad;
    if (bad || Np == 0 || Nn == 0) return PLDA_E_INVAL;
    for (int p = 0; p < n_points; ++p) {
      const double a = pts[p].c_miss * pts[p].prior, b = pts[p].c_fa * (1.0 - pts[p].prior);
      st->best[p] = plda_min_dcf_cut{dcf_value(a, b, 0, Nn, (double)Np, (double)Nn), 0, Nn, 0u, 0};
    }
  }
  const double Np = (double)st->np, Nn = (double)st->nn;
  double ca[PLDA_MIN_DCF_MAX_POINTS], cb[PLDA_MIN_DCF_MAX_POINTS];
  for (int p = 0; p < n_points; ++p) { ca[p] = pts[p].c_miss * pts[p].prior; cb[p] = pts[p].c_fa * (1.0 - pts[p].prior); }
  // every upper bin edge is a cut with exact counts (a node's lower edge was its parent's business)
  for (int64_t i = 0; i < n_nodes; ++i) {
    const uint64_t *hn = hist + i * 2 * EER_BINS, *hp = hn + EER_BINS;
    uint64_t miss = nodes[i].miss_below, below_n = nodes[i].nn_below;
    for (int b = 0; b < nb; ++b) {
      if (!(hn[b] | hp[b])) continue;             // (an empty bin's edge is the cut before it)
      miss += hp[b]; below_n += hn[b];
      if (below_n > st->nn || miss > st->np) return PLDA_E_INVAL;
      const uint64_t fa = st->nn - below_n;
      for (int p = 0; p < n_points; ++p) {
        const double v = dcf_value(ca[p], cb[p], miss, fa, Np, Nn);
        plda_min_dcf_cut &best = st->best[p];
        // lowest cut on ties: fewer trials rejected
        if (v < best.value || (v == best.value && miss + below_n < best.miss + (st->nn - best.fa))) {
          const uint32_t edge = (uint32_t)(((((uint64_t)nodes[i].prefix << DCF_BITS[level]) | (uint64_t)b) << shift) | ((1ull << shift) - 1ull));
          best = plda_min_dcf_cut{v, miss, fa, edge, 1};
        }
      }
    }
  }
  if (level == 2) return PLDA_OK;
  for (int64_t i = 0; i < n_nodes; ++i) {
    const uint64_t *hn = hist + i * 2 * EER_BINS, *hp = hn + EER_BINS;
    uint64_t miss = nodes[i].miss_below, below_n = nodes[i].nn_below;
    for (int b = 0; b < nb; ++b) {
      if (hn[b] && hp[b]) {
        const uint64_t fa_hi = st->nn - (below_n + hn[b]);
        bool keep = false;
        for (int p = 0; p < n_points && !keep; ++p) keep = dcf_value(ca[p], cb[p], miss, fa_hi, Np, Nn) <= st->best[p].value;
        if (keep) {
          if (*n_next >= cap_next || !next) return PLDA_E_CAPACITY;
          next[(*n_next)++] = plda_min_dcf_node{(nodes[i].prefix << DCF_BITS[level]) | (uint32_t)b, 0u, miss, below_n, hp[b], hn[b]};
        }
      }
      miss += hp[b]; below_n += hn[b];
    }
  }
  return PLDA_OK;
}

int min_dcf_finish(const plda_min_dcf_state *st, int n_points, const plda_dcf_point *pts, const uint32_t *below, const uint32_t *above,
                   plda_min_dcf *out) {
  if (!st || !below || !above || !out || !dcf_points_ok(n_points, pts) || st->np == 0 || st->nn == 0) return PLDA_E_INVAL;
  for (int p = 0; p < n_points; ++p) {
    const plda_min_dcf_cut &c = st->best[p];
    const uint64_t rejected = c.miss + (st->nn - c.fa);
    const double a = pts[p].c_miss * pts[p].prior, b = pts[p].c_fa * (1.0 - pts[p].prior);
    double thr;
    if (rejected == 0) {
      if (above[p] == 0xffffffffu) return PLDA_E_INVAL;
      thr = (double)key_score(above[p]);
    } else if (rejected == st->np + st->nn) {
      thr = INFINITY;
    } else {
      if (below[p] == 0u || above[p] == 0xffffffffu) return PLDA_E_INVAL;
      const double s = (double)key_score(below[p]);
      thr = s + ((double)key_score(above[p]) - s) / 2.0;
    }
    // the exact minimum never exceeds min(a, b), the cost of the better trivial cut: a quotient above 1 is rounding of
    // (b * Nn) / Nn or (a * Np) / Np alone, and is reported as the exact 1
    out[p] = plda_min_dcf{std::min(c.value / std::min(a, b), 1.0), thr, (double)c.fa / (double)st->nn, (double)c.miss / (double)st->np, c.miss, c.fa};
  }
  return PLDA_OK;
}

// ------------------------------------------------------------------------------------ the device driver
namespace {

int dcf_lds_attr(plda_handle *h) {
  static DeviceOnce attr;
  if (attr.needed(h->device)) {
    const int bytes = DCF_S * 2 * EER_BINS * 4 + DCF_S * 4;
    PLDA_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&dcf_multi_strip_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    PLDA_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&dcf_multi_flat_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    attr.done(h->device);
  }
  return PLDA_OK;
}

// one read: the level's bits under pf.n prefixes -> hh[pf.n][2][EER_BINS] (host, local counts)
int dcf_multi_pass(plda_handle *h, const TrialSource &src, int level, const DcfPrefixes &pf, unsigned long long *dhist, unsigned long long *hh) {
  const size_t hb = (size_t)pf.n * 2 * EER_BINS * 8, lds = (size_t)pf.n * 2 * EER_BINS * 4 + DCF_S * 4;
  PLDA_HIP(h, hipMemsetAsync(dhist, 0, hb, h->stream));
  PLDA_TRY(for_each_piece(src, [&](const TrialPiece &pc) -> int {
    if (pc.cls < 0) {
      const int64_t strips = ceil_div(pc.Nt, (int64_t)EER_STRIP);
      const int64_t slices = std::max<int64_t>(1, std::min<int64_t>(ceil_div(pc.rows, 16), 2048 / strips));
      const int64_t rows_per_wg = ceil_div(pc.rows, slices);
      dcf_multi_strip_kernel<<<(unsigned)(strips * ceil_div(pc.rows, rows_per_wg)), DCF_T, lds, h->stream>>>(
          pc.scores, pc.ld, pc.rows, pc.Nt, pc.espk, src.tspk, rows_per_wg, DCF_SHIFT[level], DCF_BITS[level], pf, dhist);
    } else {
      const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(pc.Nt, (int64_t)DCF_T * 4), 1024);
      dcf_multi_flat_kernel<<<grid, DCF_T, lds, h->stream>>>(pc.scores, pc.Nt, pc.cls, DCF_SHIFT[level], DCF_BITS[level], pf, dhist);
    }
    PLDA_LAUNCH_CHECK(h);
    return PLDA_OK;
  }));
  PLDA_HIP(h, hipMemcpyAsync(hh, dhist, hb, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  return PLDA_OK;
}

int dcf_neighbour_pass(plda_handle *h, const TrialSource &src, const DcfEdges &ed, unsigned *dnb, unsigned *nb /*[2 P]*/) {
  unsigned init[2 * PLDA_MIN_DCF_MAX_POINTS];
  for (int p = 0; p < PLDA_MIN_DCF_MAX_POINTS; ++p) { init[2 * p] = 0u; init[2 * p + 1] = 0xffffffffu; }
  PLDA_HIP(h, hipMemcpyAsync(dnb, init, sizeof(init), hipMemcpyHostToDevice, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));          // (init is a stack array)
  PLDA_TRY(for_each_piece(src, [&](const TrialPiece &pc) -> int {
    const int64_t total = pc.rows * pc.Nt;
    dcf_neighbour_kernel<<<(unsigned)std::min<int64_t>(ceil_div(total, 256 * 8), 256 * 16), 256, 0, h->stream>>>(pc.scores, pc.ld, pc.rows, pc.Nt, ed, dnb);
    PLDA_LAUNCH_CHECK(h);
    return PLDA_OK;
  }));
  PLDA_HIP(h, hipMemcpyAsync(nb, dnb, sizeof(init), hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  return PLDA_OK;
}

}  // namespace

// Sharded calls (src.reduce): every histogram is summed over the ranks before the host step sees it, so every rank takes the
// same decisions and makes the same sequence of reductions.  A rank that fails locally keeps taking part with a poisoned
// histogram (2^48 on counter 0, as eer_device); every rank sees the poison after that very sum and returns an error then.
static int min_dcf_device(plda_handle *h, const TrialSource &src, int n_points, const plda_dcf_point *pts, plda_min_dcf *out, plda_min_dcf_info *info_out) {
  constexpr int P = PLDA_MIN_DCF_MAX_POINTS;
  if (!out || !dcf_points_ok(n_points, pts))
    return fail(h, PLDA_E_INVAL, "min_dcf: 1 .. %d operating points with 0 < prior < 1 and finite costs > 0", P);
  const int S = h->mindcf_variant == 2 ? 2 : DCF_S;
  const bool user_lists = src.kind == TrialSource::LISTS;
  plda_min_dcf_info info;
  std::memset(&info, 0, sizeof(info));
  PLDA_TRY(dcf_lds_attr(h));
  unsigned long long *dhist, *dcursor;
  unsigned *dnb;         // [2 P] neighbour words; (+ the EER's below / above at level 0)
  unsigned *dprefix;     // (256 bytes behind the histograms)
  PLDA_TRY(carve(h, h->trial_hist, [&](Layout &c) { c.take(dhist, (size_t)DCF_S * 2 * EER_BINS).take(dcursor, 2).take(dnb, 2 * P).take(dprefix, DCF_CMAX, 256); }));

  int rc = PLDA_OK;
  // sums one [2][EER_BINS] block over the ranks; false: the call ends here, on every rank
  auto reduce_block = [&](unsigned long long *H) -> bool { return reduce_block_or_poison(h, src, "min_dcf", H, &rc); };

  plda_min_dcf_state st;
  std::memset(&st, 0, sizeof(st));
  std::vector<plda_min_dcf_node> nodes(1, plda_min_dcf_node{0u, 0u, 0, 0, 0, 0}), next;
  std::vector<unsigned long long> H, Hloc, H0;
  // the compacted bins: key >> cshift == prefix, with the number of trials below and through each (the neighbour proof)
  struct CBin { unsigned prefix; unsigned long long c_lo, c_hi; };
  std::vector<CBin> cbins;
  int cshift = 0;
  TrialSource cur = src;                 // the data the levels read: the caller's, then the lists
  bool on_lists = false;

  for (int level = 0; level < 3 && !nodes.empty(); ++level) {
    TraceScope ts(h, level == 0 ? "min_dcf.level0" : level == 1 ? "min_dcf.level1" : "min_dcf.level2");
    const int64_t nn = (int64_t)nodes.size();
    info.level_bins[level] = nn;
    for (const auto &nd : nodes) info.level_trials[level] += level == 0 ? 0 : nd.n_pos + nd.n_neg;
    next.clear();
    for (int64_t c0 = 0; c0 < nn; c0 += DCF_CHUNK) {
      const int64_t cn = std::min(DCF_CHUNK, nn - c0);
      H.assign((size_t)cn * 2 * EER_BINS, 0ull);
      if (src.reduce) Hloc.assign(H.size(), 0ull);
      if (level == 0) {
        if (rc == PLDA_OK) rc = eer_pass(h, cur, DCF_SHIFT[0], DCF_BITS[0], 0u, 0, dhist, dnb, dnb + 1, H0);
        if (rc == PLDA_OK) std::copy(H0.begin(), H0.end(), H.begin());
        ++info.reads; ++info.launches; ++info.level_launches[0];
        if (src.reduce) Hloc = H;
        if (!reduce_block(H.data())) return rc;
      } else {
        for (int64_t b0 = 0; b0 < cn; b0 += S) {
          DcfPrefixes pf;
          pf.n = (int)std::min<int64_t>(S, cn - b0);
          for (int s = 0; s < DCF_S; ++s) pf.p[s] = s < pf.n ? nodes[(size_t)(c0 + b0 + s)].prefix : 0xffffffffu;
          unsigned long long *hb = H.data() + (size_t)b0 * 2 * EER_BINS;
          if (rc == PLDA_OK) rc = dcf_multi_pass(h, cur, level, pf, dhist, hb);
          if (!on_lists) ++info.reads;
          ++info.launches; ++info.level_launches[level];
          if (src.reduce) std::copy(hb, hb + (size_t)pf.n * 2 * EER_BINS, Hloc.begin() + (size_t)b0 * 2 * EER_BINS);
          for (int s = 0; s < pf.n; ++s)
            if (!reduce_block(hb + (size_t)s * 2 * EER_BINS)) return rc;
        }
      }
      const size_t base = next.size();
      const int64_t room = level == 2 ? 0 : level == 0 ? EER_BINS
                                          : (int64_t)std::min<unsigned long long>((unsigned long long)cn * EER_BINS, (st.np + st.nn) / 2 + 1);
      next.resize(base + (size_t)room);
      int64_t got = 0;
      const int step_rc = min_dcf_step(level, cn, nodes.data() + c0, reinterpret_cast<const uint64_t *>(H.data()), n_points, pts, &st, room,
                                       next.data() + base, &got);
      if (step_rc != PLDA_OK && level == 0 && st.nonfinite)
        return fail(h, PLDA_E_INVAL, "min_dcf: %llu non-finite score(s) among the trials", (unsigned long long)st.nonfinite);
      if (step_rc != PLDA_OK && level == 0 && (st.np == 0 || st.nn == 0))
        return fail(h, PLDA_E_INVAL, "min_dcf: need at least one target and one non-target trial");
      if (step_rc != PLDA_OK) return fail(h, PLDA_E_NUMERIC, "min_dcf: inconsistent counts at level %d (%d)", level, step_rc);
      next.resize(base + (size_t)got);
    }
    if (level == 0) { info.np = st.np; info.nn = st.nn; info.level_trials[0] = st.np + st.nn; }
    if (level == 2) break;

    // compaction: one read appends the trials inside the survivors to two lists when they are few and the next level
    // would take more than one read of the scores
    unsigned long long inside = 0;
    for (const auto &nd : next) inside += nd.n_pos + nd.n_neg;
    // (sharded: the lists' lengths are local counts, kept for a level of one chunk)
    if (!on_lists && !user_lists && h->mindcf_variant != 1 && !next.empty() && inside <= DCF_LIST_CAP && (int64_t)next.size() > S &&
        (int64_t)next.size() <= DCF_CMAX && nn <= DCF_CHUNK) {
      ts.next("min_dcf.compact");
      // the lists' exact lengths: the LOCAL counts of the surviving bins (sharded: the histograms before the sums)
      unsigned long long len[2] = {0, 0};
      if (src.reduce) {
        for (const auto &nd : next) {
          const unsigned parent = nd.prefix >> DCF_BITS[level], bin = nd.prefix & ((1u << DCF_BITS[level]) - 1u);
          size_t pi = 0;
          while (pi < nodes.size() && nodes[pi].prefix != parent) ++pi;
          if (pi == nodes.size()) return fail(h, PLDA_E_NUMERIC, "min_dcf: survivor without a parent");
          len[0] += Hloc[pi * 2 * EER_BINS + bin];
          len[1] += Hloc[pi * 2 * EER_BINS + EER_BINS + bin];
        }
      } else {
        for (const auto &nd : next) { len[0] += nd.n_neg; len[1] += nd.n_pos; }
      }
      std::vector<unsigned> pre(next.size());
      for (size_t i = 0; i < next.size(); ++i) pre[i] = next[i].prefix;
      unsigned long long cursor[2] = {0, 0};
      if (rc == PLDA_OK) {
        rc = [&]() -> int {
          PLDA_HIP(h, h->eer_list[0].reserve((size_t)std::max<unsigned long long>(len[0], 1) * 4));
          PLDA_HIP(h, h->eer_list[1].reserve((size_t)std::max<unsigned long long>(len[1], 1) * 4));
          PLDA_HIP(h, hipMemsetAsync(dcursor, 0, 16, h->stream));
          PLDA_HIP(h, hipMemcpyAsync(dprefix, pre.data(), pre.size() * 4, hipMemcpyHostToDevice, h->stream));
          const int hi_shift = DCF_SHIFT[level];           // the survivors' prefixes are key >> this level's shift
          PLDA_TRY(for_each_piece(cur, [&](const TrialPiece &pc) -> int {
            const int64_t strips = ceil_div(pc.Nt, (int64_t)EER_STRIP);
            const int64_t slices = std::max<int64_t>(1, std::min<int64_t>(pc.rows, (256 * 16) / strips));
            const int64_t rows_per_wg = ceil_div(pc.rows, slices);
            dcf_compact_strip_kernel<<<(unsigned)(strips * ceil_div(pc.rows, rows_per_wg)), 256, 0, h->stream>>>(
                pc.scores, pc.ld, pc.rows, pc.Nt, pc.espk, src.tspk, rows_per_wg, hi_shift, dprefix, (int)pre.size(), dcursor,
                h->eer_list[0].as<float>(), h->eer_list[1].as<float>(), len[0], len[1]);
            PLDA_LAUNCH_CHECK(h);
            return PLDA_OK;
          }));
          PLDA_HIP(h, hipMemcpyAsync(cursor, dcursor, 16, hipMemcpyDeviceToHost, h->stream));
          PLDA_HIP(h, hipStreamSynchronize(h->stream));
          // overflow is impossible by construction (the lengths are the histograms' own counts): asserted
          if (cursor[0] != len[0] || cursor[1] != len[1])
            return fail(h, PLDA_E_NUMERIC, "min_dcf: the lists hold %llu + %llu scores, the histograms counted %llu + %llu", cursor[0], cursor[1], len[0], len[1]);
          return PLDA_OK;
        }();
      }
      ++info.reads; ++info.launches;
      info.lists_used = 1;
      on_lists = true;
      cshift = DCF_SHIFT[level];
      for (const auto &nd : next) cbins.push_back(CBin{nd.prefix, nd.miss_below + nd.nn_below, nd.miss_below + nd.nn_below + nd.n_pos + nd.n_neg});
      cur = TrialSource::lists(h->eer_list[1].as<float>(), (int64_t)len[1], h->eer_list[0].as<float>(), (int64_t)len[0]);
      // (a failure here is carried to the next reduction, which every rank reaches: the next level has nodes)
    }
    nodes.swap(next);
  }

  // ---- the keys next to the winning cuts
  TraceScope ts(h, "min_dcf.neighbours");
  DcfEdges ed;
  ed.has = 0;
  for (int p = 0; p < P; ++p) {
    ed.e[p] = p < n_points ? st.best[p].edge : 0xffffffffu;
    if (p >= n_points || st.best[p].has_edge) ed.has |= 1u << p;
  }
  unsigned nb[2 * P];
  const unsigned long long total = st.np + st.nn;
  auto reduce_neighbours = [&]() {
    if (!src.reduce) return;
    for (int p = 0; p < n_points; ++p)
      if (src.reduce(src.ctx, nullptr, &nb[2 * p], &nb[2 * p + 1]) != 0 && rc == PLDA_OK) rc = fail(h, PLDA_E_INVAL, "min_dcf: the caller's reduction failed");
  };
  auto status_round = [&]() -> bool {          // every rank learns whether all of them are still well
    if (!src.reduce) return rc == PLDA_OK;
    std::vector<unsigned long long> Z((size_t)2 * EER_BINS, 0ull);
    return reduce_block(Z.data());
  };
  bool proven = false;
  if (on_lists) {
    if (rc == PLDA_OK) rc = dcf_neighbour_pass(h, cur, ed, dnb, nb);
    ++info.launches;
    if (!status_round()) return rc;
    reduce_neighbours();
    if (!status_round()) return rc;
    auto bin_of = [&](unsigned key) -> const CBin * {
      const unsigned q = key >> cshift;
      auto it = std::lower_bound(cbins.begin(), cbins.end(), q, [](const CBin &b, unsigned v) { return b.prefix < v; });
      return (it != cbins.end() && it->prefix == q) ? &*it : nullptr;
    };
    proven = true;
    for (int p = 0; p < n_points && proven; ++p) {
      const plda_min_dcf_cut &c = st.best[p];
      const unsigned long long R = c.miss + (st.nn - c.fa);
      const unsigned lo = nb[2 * p], hi = nb[2 * p + 1];
      if (R > 0 && R < total) {                 // (the largest key <= the edge matters for a proper cut only)
        const CBin *b = lo ? bin_of(lo) : nullptr;
        if (!b || !((c.has_edge && (lo >> cshift) == (c.edge >> cshift)) || R == b->c_hi)) proven = false;
      }
      if (R < total) {
        const CBin *b = hi != 0xffffffffu ? bin_of(hi) : nullptr;
        if (!b || !((c.has_edge && (hi >> cshift) == (c.edge >> cshift)) || R == b->c_lo)) proven = false;
      }
    }
  }
  if (!proven) {
    if (rc == PLDA_OK) rc = dcf_neighbour_pass(h, src, ed, dnb, nb);
    ++info.reads; ++info.launches; ++info.neighbour_reads;
    if (!status_round()) return rc;
    reduce_neighbours();
    if (!status_round()) return rc;
  }
  unsigned below[P], above[P];
  for (int p = 0; p < P; ++p) { below[p] = nb[2 * p]; above[p] = nb[2 * p + 1]; }
  if (min_dcf_finish(&st, n_points, pts, below, above, out) != PLDA_OK)
    return fail(h, PLDA_E_NUMERIC, "min_dcf: the keys next to a winning cut were not found (inconsistent counts)");
  if (info_out) *info_out = info;
  return PLDA_OK;
}

int min_dcf_matrix_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *despk,
                          const int64_t *dtspk, int n_points, const plda_dcf_point *pts, plda_min_dcf *out, plda_min_dcf_info *info,
                          TrialReduce reduce, void *ctx) {
  // a rank of a sharded call may own no row at all (M == 0): it still takes part in the reductions
  if (!out || Nt <= 0 || ld < Nt || M < 0 || (M == 0 && !reduce) || !dtspk || (M > 0 && (!dscores || !despk)))
    return fail(h, PLDA_E_INVAL, "min_dcf: bad argument");
  return min_dcf_device(h, TrialSource::matrix(dscores, ld, M, Nt, despk, dtspk).reduced_by(reduce, ctx), n_points, pts, out, info);
}

int min_dcf_lists_device(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, int n_points,
                         const plda_dcf_point *pts, plda_min_dcf *out, plda_min_dcf_info *info) {
  if (!dpos || !dneg || !out || np <= 0 || nn <= 0) return fail(h, PLDA_E_INVAL, "min_dcf: need at least one target and one non-target score");
  return min_dcf_device(h, TrialSource::lists(dpos, np, dneg, nn), n_points, pts, out, info);
}

int score_min_dcf_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV, int64_t Nt,
                         const double *dzmean, const double *dzstd, const int64_t *despk, const int64_t *dtspk, int n_points,
                         const plda_dcf_point *pts, plda_min_dcf *out, plda_min_dcf_info *info) {
  OperandSlabs os;
  TrialSource src;
  PLDA_TRY(operand_source(h, "score_min_dcf", dU, dn, n_uniform, M, dV, Nt, dzmean, dzstd, despk, dtspk, out, &os, &src));
  return min_dcf_device(h, src, n_points, pts, out, info);
}

}  // namespace plda
