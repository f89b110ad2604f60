// plda_amd/csrc/rocch.hip -- the ROC convex hull of labelled trials, exact and without a global sort: minCllr, the
// ROCCH-EER and the PAV (pool adjacent violators) calibration map (include/plda_hip.h, "ROC convex hull"; pinned by
// tests/rocch_model.py).
//
// A strict vertex of the lower hull is a cut whose own key group holds a non-target and whose next key group holds a
// target, so only the cuts next to the keys of ONE class can be vertices.  The EDGE class is the rarer one (the targets of a
// trials matrix: one trial in n_speakers).  Its T keys are compacted and sorted; the other class is RANKED among them -- a
// histogram whose bin edges are those keys, counter 2 g for a key strictly below sorted[g] (and above sorted[g - 1]),
// counter 2 g + 1 for a key equal to it -- and the monotone chain over the 2 T + 2 points runs on the host
// (plda_rocch_hull, pure).  Level histograms with a bound (dcf.hip) do not prune here: a key range can be dropped only when
// its whole rectangle of counts lies on or above the hull, which a smooth ROC grants to ranges of a few hundred trials only.
//
// Every pass reaches its kernels through for_each_piece over a TrialSource (trial_source.hpp):
//  * rocch_count_kernel: the number of targets of a matrix from the speaker ids alone (no score is read), which names the
//    edge class -- the targets unless Np > Nn -- and the exact length of its key list.
//  * the EDGE pass (read 1): appends the keys of the edge class with the wave-staged append of eer_window_strip_kernel
//    (a slot in the wave's LDS stage per hit, 512+ keys leave behind one global atomic) and counts its non-finite scores.
//  * a keys-only stable LSD radix sort (8-bit digits; K1a's sort in fit.hip carries values and is left alone).  Equal keys
//    stay in the sorted list: the rank of a key is taken at the FIRST of its run, the host forms the distinct keys and their
//    multiplicities in the scan that it makes anyway.
//  * the RANK pass (read 2), the hot kernel: the strip traversal of eer_hist_strip_kernel.  A search table in LDS -- 2048
//    buckets across [smallest, largest] edge key -> offset into the sorted list -- starts the lower bound a few compares
//    from its end; keys outside [smallest, largest] are done after two compares and go to two register counters.  A
//    contiguous WINDOW of W gaps (2 W uint32 counters in LDS, merged once with 64-bit global adds) takes what falls inside
//    it; the rest goes to 64-bit global atomics one by one (no aggregation of equal destinations within a wave: unmeasured).
//    The window is chosen on the host from a COARSE count -- this same kernel over every ceil(T / 2048)-th edge key, all of
//    whose counters fit the window -- in a read of its own (every 16th row of a large matrix; whole lists and slabs).
//  * rocch_neighbour_kernel (read 3): per hull vertex the largest key <= its cut and the smallest key above it, among all
//    trials: the vertex's key and threshold (the EER's midpoint rule) need keys of the other class that the ranks do not
//    give.  Up to 4095 cuts per read (one more slot takes the keys above a chunk's last cut).
//  * pav_map_kernel: out = (float) llr[segment of key(s)], the table of <= 4096 segments in LDS.
// Integer atomics only: a call is bit-reproducible.
#include "trial_source.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace plda {

constexpr int RC_W = 4096;                // gaps of the rank pass's LDS window (32 KiB of counters beside the 8 KiB table)
constexpr int RC_TAB = 2048;              // buckets of the search table
constexpr int RC_VCAP = 4096;             // cuts of one neighbour read; segments of the PAV table
constexpr int RC_WBUF = 1536;             // staged keys per wave of the edge pass
constexpr int RC_SORT_TILE = 4096;        // keys per workgroup of a radix pass (16 rounds of 256)
constexpr int64_t RC_EDGE_CAP = (int64_t)1 << 24;
constexpr int64_t RC_MAX_ROWS_PER_WG = (int64_t)1 << 20;   // x 1024 columns: a workgroup's LDS counter stays below 2^30

typedef float f32x4r __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool rc_nonfinite(float x) { return !(__builtin_fabsf(x) < __builtin_inff()); }

// ------------------------------------------------------------------------------------ the two walks
// Strip walk (a matrix or a slab): a workgroup of 256 threads owns EER_STRIP columns, 4 per thread with their speaker ids
// in registers, and a slice of the rows; four rows are loaded before they are accounted for.  acc(x, is_target) per trial,
// acc.batch() after every four rows (wave-uniform).  Flat walk (one list of one class): grid stride.
template <class Acc>
__device__ __forceinline__ void rc_walk_strip(const float *__restrict__ scores, int64_t ld, int64_t M, int64_t Nt,
                                              const int64_t *__restrict__ espk, const int64_t *__restrict__ tspk, int64_t rows_per_wg,
                                              int64_t row_step, Acc &acc) {
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
  for (int64_t row = r0; row < r1; row += 4) {
    float v[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (row + u >= r1) break;
      const float *src = scores + (row + u) * row_step * ld + col;
      if (vec) {
        const f32x4r x = __builtin_nontemporal_load(reinterpret_cast<const f32x4r *>(src));
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
      for (int e = 0; e < 4; ++e)
        if (ok[e]) acc(v[u][e], ts[e] == spk);
    }
    acc.batch();
  }
}

template <class Acc>
__device__ __forceinline__ void rc_walk_flat(const float *__restrict__ scores, int64_t n, bool is_target, Acc &acc) {
  // (whole rounds of the grid, so that batch() is reached by every lane of a wave together)
  for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
    const int64_t idx = base + threadIdx.x;
    if (idx < n) acc(scores[idx], is_target);
    acc.batch();
  }
}

// wave sum of a per-thread count -> one 64-bit global add per wave
__device__ __forceinline__ void rc_wave_add(unsigned long long v, unsigned long long *dst) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

// ------------------------------------------------------------------------------------ the edge class of a matrix
// out[0] += #{(i, j): espk[i] == tspk[j]}: the strip layout without the scores
__global__ __launch_bounds__(256) void rocch_count_kernel(const int64_t *__restrict__ espk, int64_t M, const int64_t *__restrict__ tspk,
                                                          int64_t Nt, int64_t rows_per_wg, unsigned long long *__restrict__ out) {
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
  unsigned long long n = 0;
  for (int64_t row = r0; row < r1; ++row) {
    const int64_t spk = espk[row];
#pragma unroll
    for (int e = 0; e < 4; ++e) n += (ok[e] && ts[e] == spk) ? 1u : 0u;
  }
  rc_wave_add(n, out);
}

// ------------------------------------------------------------------------------------ the edge pass
// misc[0]: keys appended (the cursor); misc[1]: non-finite scores of the edge class; misc[2]: of the other class (rank pass)
struct EdgeAcc {
  unsigned *stage;            // this wave's [RC_WBUF]
  int *fill;                  // this wave's fill count
  unsigned *keys;
  unsigned long long cap, *misc;
  bool edge_is_target;
  unsigned nf;
  __device__ __forceinline__ void operator()(float x, bool tgt) {
    if (tgt != edge_is_target) return;
    nf += rc_nonfinite(x) ? 1u : 0u;
    const int slot = atomicAdd(fill, 1);
    stage[slot] = score_key(x);
  }
  __device__ __forceinline__ void flush() {
    const int lane = threadIdx.x & 63;
    const int n = __builtin_amdgcn_readfirstlane(*fill);
    if (n == 0) return;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&misc[0], (unsigned long long)n);
    base = __shfl(base, 0);
    for (int i = lane; i < n; i += 64)
      if (base + i < cap) keys[base + i] = stage[i];     // (a write beyond the counted length is dropped; the caller compares)
    if (lane == 0) *fill = 0;
  }
  __device__ __forceinline__ void batch() {
    if (__builtin_amdgcn_readfirstlane(*fill) > RC_WBUF - 1024) flush();
  }
};

__global__ __launch_bounds__(256) void rocch_edge_strip_kernel(const float *__restrict__ scores, int64_t ld, int64_t M, int64_t Nt,
                                                               const int64_t *__restrict__ espk, const int64_t *__restrict__ tspk,
                                                               int64_t rows_per_wg, int edge_is_target, unsigned *__restrict__ keys,
                                                               unsigned long long cap, unsigned long long *__restrict__ misc) {
  __shared__ unsigned stage[4][RC_WBUF];
  __shared__ int fillc[4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) fillc[wave] = 0;
  __syncthreads();
  EdgeAcc acc{stage[wave], &fillc[wave], keys, cap, misc, edge_is_target != 0, 0u};
  rc_walk_strip(scores, ld, M, Nt, espk, tspk, rows_per_wg, 1, acc);
  acc.flush();
  rc_wave_add(acc.nf, &misc[1]);
}

// the edge list of the two-list form: its keys in place order, its non-finite scores counted
__global__ __launch_bounds__(256) void rocch_edge_flat_kernel(const float *__restrict__ scores, int64_t n, unsigned *__restrict__ keys,
                                                              unsigned long long *__restrict__ misc) {
  unsigned long long nf = 0;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
    const float x = scores[idx];
    nf += rc_nonfinite(x) ? 1u : 0u;
    keys[idx] = score_key(x);
  }
  rc_wave_add(nf, &misc[1]);
}

// ------------------------------------------------------------------------------------ keys-only stable LSD radix sort
// One pass on the 8 bits at `shift`: digit counts per tile -> hist[digit][tile]; an exclusive scan over that array in
// digit-major order gives every (digit, tile) its first slot; the scatter walks a tile in place order, 256 keys a round.
__global__ __launch_bounds__(256) void rocch_sort_hist_kernel(const unsigned *__restrict__ keys, int64_t n, int shift, int64_t tiles,
                                                              unsigned *__restrict__ hist) {
  __shared__ unsigned lh[256];
  lh[threadIdx.x] = 0;
  __syncthreads();
  const int64_t t0 = (int64_t)blockIdx.x * RC_SORT_TILE;
  for (int r = 0; r < RC_SORT_TILE / 256; ++r) {
    const int64_t idx = t0 + r * 256 + threadIdx.x;
    if (idx < n) atomicAdd(&lh[(keys[idx] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(int64_t)threadIdx.x * tiles + blockIdx.x] = lh[threadIdx.x];
}

// exclusive scan of hist[0 .. len) in place by one workgroup of 1024 threads (len <= 2^20 at the edge cap's default)
__global__ __launch_bounds__(1024) void rocch_sort_scan_kernel(unsigned *__restrict__ hist, int64_t len) {
  __shared__ unsigned part[1024];
  const int64_t per = (len + 1023) / 1024;
  const int64_t a = (int64_t)threadIdx.x * per, b = a + per < len ? a + per : len;
  unsigned s = 0;
  for (int64_t i = a; i < b; ++i) s += hist[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const unsigned add = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0u;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  unsigned run = part[threadIdx.x] - s;
  for (int64_t i = a; i < b; ++i) {
    const unsigned c = hist[i];
    hist[i] = run;
    run += c;
  }
}

__global__ __launch_bounds__(256) void rocch_sort_scatter_kernel(const unsigned *__restrict__ keys, int64_t n, int shift, int64_t tiles,
                                                                 const unsigned *__restrict__ hist, unsigned *__restrict__ out) {
  __shared__ unsigned base[256];
  __shared__ unsigned cnt[4][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  base[threadIdx.x] = hist[(int64_t)threadIdx.x * tiles + blockIdx.x];
#pragma unroll
  for (int w = 0; w < 4; ++w) cnt[w][threadIdx.x] = 0;
  __syncthreads();
  const int64_t t0 = (int64_t)blockIdx.x * RC_SORT_TILE;
  for (int r = 0; r < RC_SORT_TILE / 256; ++r) {
    const int64_t idx = t0 + r * 256 + threadIdx.x;
    if (t0 + r * 256 >= n) break;                        // (uniform over the workgroup)
    const bool live = idx < n;
    const unsigned k = live ? keys[idx] : 0u;
    const unsigned d = (k >> shift) & 255u;
    // the lanes of this wave that hold the same digit
    unsigned long long same = __ballot(live);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const unsigned long long m = __ballot(live && ((d >> b) & 1u));
      same &= ((d >> b) & 1u) ? m : ~m;
    }
    const unsigned rank = (unsigned)__popcll(same & ((1ull << lane) - 1ull));
    if (live && rank == 0) cnt[wave][d] = (unsigned)__popcll(same);
    __syncthreads();
    if (live) {
      unsigned off = base[d] + rank;
      for (int w = 0; w < wave; ++w) off += cnt[w][d];
      if (off < n) out[off] = k;
    }
    __syncthreads();
    {
      const unsigned add = (cnt[0][threadIdx.x] + cnt[1][threadIdx.x]) + (cnt[2][threadIdx.x] + cnt[3][threadIdx.x]);
      base[threadIdx.x] += add;
#pragma unroll
      for (int w = 0; w < 4; ++w) cnt[w][threadIdx.x] = 0;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------ the rank pass
// The search table over the sorted list u[0 .. T): bucket b of key k is (k - u[0]) >> shift with shift the smallest that
// leaves at most RC_TAB buckets; tab[b] = lower bound of u[0] + (b << shift), tab[nb] = T.
__host__ __device__ inline int rc_table_shift(unsigned umin, unsigned umax) {
  const unsigned range = umax - umin;
  int bits = 0;
  while (bits < 32 && (range >> bits) != 0u) ++bits;
  return bits > 11 ? bits - 11 : 0;
}
__global__ __launch_bounds__(256) void rocch_table_kernel(const unsigned *__restrict__ u, int64_t T, unsigned *__restrict__ tab) {
  const unsigned umin = u[0], umax = u[T - 1];
  const int shift = rc_table_shift(umin, umax);
  const unsigned nb = ((umax - umin) >> shift) + 1u;
  for (unsigned b = threadIdx.x; b <= RC_TAB; b += 256) {
    unsigned v = (unsigned)T;
    const unsigned long long bound = (unsigned long long)umin + ((unsigned long long)b << shift);
    if (b < nb && bound <= 0xffffffffull) {
      int64_t lo = 0, hi = T;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (u[mid] < (unsigned)bound) lo = mid + 1; else hi = mid;
      }
      v = (unsigned)lo;
    }
    tab[b] = v;
  }
}

// cnt[0 .. 2 T]: the counters; cnt[2 T + 1] / cnt[2 T + 2]: the keys below u[0] / above u[T - 1] (the host folds them into
// counters 0 and 2 T).  LDS: the table [RC_TAB + 1], then 2 W window counters for the counters [2 w0, 2 w0 + 2 W).
struct RankAcc {
  const unsigned *u;
  const unsigned *tab;        // LDS
  unsigned *win;              // LDS
  unsigned long long *cnt;
  int64_t T;
  unsigned umin, umax, w2lo, w2n;
  int shift;
  bool edge_is_target;
  unsigned below, above, nf;
  __device__ __forceinline__ void operator()(float x, bool tgt) {
    if (tgt == edge_is_target) return;
    nf += rc_nonfinite(x) ? 1u : 0u;
    const unsigned k = score_key(x);
    if (k < umin) { ++below; return; }
    if (k > umax) { ++above; return; }
    const unsigned b = (k - umin) >> shift;
    unsigned lo = tab[b], hi = tab[b + 1];
    while (lo < hi) {
      const unsigned mid = (lo + hi) >> 1;
      if (u[mid] < k) lo = mid + 1; else hi = mid;
    }
    if ((int64_t)lo >= T) { ++above; return; }            // (cannot happen for k <= umax; never an index past the list)
    const unsigned long long idx = 2ull * lo + (u[lo] == k ? 1u : 0u);
    const unsigned long long rel = idx - w2lo;             // (wraps to a huge value below the window)
    if (rel < w2n) atomicAdd(&win[(unsigned)rel], 1u);
    else atomicAdd(&cnt[idx], 1ull);
  }
  __device__ __forceinline__ void batch() {}
};

__device__ __forceinline__ void rc_rank_setup(RankAcc &acc, unsigned *lds, const unsigned *u, int64_t T, const unsigned *gtab,
                                              int64_t w0, int W, unsigned long long *cnt, int edge_is_target) {
  for (int i = threadIdx.x; i <= RC_TAB; i += 256) lds[i] = gtab[i];
  unsigned *win = lds + RC_TAB + 1;
  for (int i = threadIdx.x; i < 2 * W; i += 256) win[i] = 0;
  __syncthreads();
  acc.u = u; acc.tab = lds; acc.win = win; acc.cnt = cnt; acc.T = T;
  acc.umin = u[0]; acc.umax = u[T - 1];
  acc.shift = rc_table_shift(acc.umin, acc.umax);
  acc.w2lo = (unsigned)(2 * w0); acc.w2n = (unsigned)(2 * W);
  acc.edge_is_target = edge_is_target != 0;
  acc.below = acc.above = acc.nf = 0;
}
__device__ __forceinline__ void rc_rank_finish(RankAcc &acc, int64_t w0, int W, unsigned long long *misc) {
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * W; i += 256) {
    const unsigned c = acc.win[i];
    if (c) atomicAdd(&acc.cnt[2 * w0 + i], (unsigned long long)c);     // (a counter past 2 T is never incremented)
  }
  rc_wave_add(acc.below, &acc.cnt[2 * acc.T + 1]);
  rc_wave_add(acc.above, &acc.cnt[2 * acc.T + 2]);
  rc_wave_add(acc.nf, &misc[2]);
}

__global__ __launch_bounds__(256) void rocch_rank_strip_kernel(const float *__restrict__ scores, int64_t ld, int64_t M, int64_t Nt,
                                                               const int64_t *__restrict__ espk, const int64_t *__restrict__ tspk,
                                                               int64_t rows_per_wg, int64_t row_step, int edge_is_target,
                                                               const unsigned *__restrict__ u, int64_t T, const unsigned *__restrict__ gtab,
                                                               int64_t w0, int W, unsigned long long *__restrict__ cnt,
                                                               unsigned long long *__restrict__ misc) {
  extern __shared__ unsigned rc_lds[];
  RankAcc acc;
  rc_rank_setup(acc, rc_lds, u, T, gtab, w0, W, cnt, edge_is_target);
  rc_walk_strip(scores, ld, M, Nt, espk, tspk, rows_per_wg, row_step, acc);
  rc_rank_finish(acc, w0, W, misc);
}

// a list of the OTHER class (every element is ranked)
__global__ __launch_bounds__(256) void rocch_rank_flat_kernel(const float *__restrict__ scores, int64_t n, int edge_is_target,
                                                              const unsigned *__restrict__ u, int64_t T, const unsigned *__restrict__ gtab,
                                                              int64_t w0, int W, unsigned long long *__restrict__ cnt,
                                                              unsigned long long *__restrict__ misc) {
  extern __shared__ unsigned rc_lds[];
  RankAcc acc;
  rc_rank_setup(acc, rc_lds, u, T, gtab, w0, W, cnt, edge_is_target);
  rc_walk_flat(scores, n, edge_is_target == 0, acc);
  rc_rank_finish(acc, w0, W, misc);
}

// ------------------------------------------------------------------------------------ the keys next to the vertices' cuts
// edges[0 .. n) ascending, edges[n - 1] = 0xffffffff.  Slot i takes the keys k with edges[i - 1] < k <= edges[i]:
// lo[i] = their maximum (the largest key <= edges[i]), hi[i] = their minimum (the smallest key above edges[i - 1]; hi[0]:
// the smallest key of all).  Every trial of either class counts.  An LDS word is read before its atomic: the extremes
// settle after a few trials and the rest pass with two loads.
__global__ __launch_bounds__(256) void rocch_neighbour_kernel(const float *__restrict__ scores, int64_t ld, int64_t M, int64_t Nt,
                                                              const unsigned *__restrict__ edges, int n, unsigned *__restrict__ lo,
                                                              unsigned *__restrict__ hi) {
  __shared__ unsigned se[RC_VCAP], slo[RC_VCAP], shi[RC_VCAP];
  for (int i = threadIdx.x; i < n; i += 256) { se[i] = edges[i]; slo[i] = 0u; shi[i] = 0xffffffffu; }
  __syncthreads();
  const int64_t total = M * Nt;
  const bool flat = ld == Nt;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const unsigned k = score_key(flat ? scores[idx] : scores[(idx / Nt) * ld + idx % Nt]);
    int a = 0, b = n - 1;                          // the first slot whose edge is >= k (the last edge is the largest word)
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (se[mid] < k) a = mid + 1; else b = mid;
    }
    if (k > slo[a]) atomicMax(&slo[a], k);
    if (k < shi[a]) atomicMin(&shi[a], k);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += 256) {
    if (slo[i]) atomicMax(&lo[i], slo[i]);
    if (shi[i] != 0xffffffffu) atomicMin(&hi[i], shi[i]);
  }
}

// ------------------------------------------------------------------------------------ the PAV map
// out[i, j] = tab[#{interior vertex keys < key(s[i, j])}]; a NaN goes through as it is.  Layout and in-place rule of
// affine_map_kernel (calib.hip).  vkeys[0 .. nseg - 1): the keys of the interior vertices, ascending; tab[0 .. nseg).
__global__ __launch_bounds__(256) void pav_map_kernel(const float *scores, int64_t ld, int64_t M, int64_t Nt, const unsigned *__restrict__ vkeys,
                                                      const float *__restrict__ tab, int nseg, float *out, int64_t ld_out) {
  __shared__ unsigned sk[RC_VCAP];
  __shared__ float st[RC_VCAP];
  for (int i = threadIdx.x; i < nseg; i += 256) { st[i] = tab[i]; if (i < nseg - 1) sk[i] = vkeys[i]; }
  __syncthreads();
  const int64_t col = (int64_t)blockIdx.x * EER_STRIP + (int64_t)threadIdx.x * 4;
  if (col >= Nt) return;
  // the four elements of a thread search in lock-step: a fixed number of steps (uniform over the workgroup), no branch, four
  // independent chains of LDS reads in flight.  Invariant: the answer lies in [base, base + len].
  const int nkeys = nseg - 1;
  auto map4 = [&](const float (&x)[4], float (&y)[4]) {
    unsigned k[4];
    int base[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { k[e] = score_key(x[e]); base[e] = 0; }
    for (int len = nkeys; len > 1;) {
      const int half = len >> 1;
#pragma unroll
      for (int e = 0; e < 4; ++e) base[e] += sk[base[e] + half - 1] < k[e] ? half : 0;
      len -= half;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int seg = base[e] + ((nkeys > 0 && sk[base[e]] < k[e]) ? 1 : 0);
      y[e] = x[e] != x[e] ? x[e] : st[seg];
    }
  };
  const bool vec = ((ld & 3) == 0) && ((ld_out & 3) == 0) && ((reinterpret_cast<uintptr_t>(scores) & 15) == 0) &&
                   ((reinterpret_cast<uintptr_t>(out) & 15) == 0) && col + 3 < Nt;
  for (int64_t row = blockIdx.y; row < M; row += gridDim.y) {
    const float *src = scores + row * ld + col;
    float *dst = out + row * ld_out + col;
    if (vec) {
      const f32x4r x = *reinterpret_cast<const f32x4r *>(src);
      const float in[4] = {x.x, x.y, x.z, x.w};
      float o[4];
      map4(in, o);
      f32x4r y;
      y.x = o[0]; y.y = o[1]; y.z = o[2]; y.w = o[3];
      *reinterpret_cast<f32x4r *>(dst) = y;
    } else {
      float in[4], o[4];
      for (int e = 0; e < 4; ++e) in[e] = col + e < Nt ? src[e] : 0.f;
      map4(in, o);
      for (int e = 0; e < 4 && col + e < Nt; ++e) dst[e] = o[e];
    }
  }
}

// ------------------------------------------------------------------------------------ the host step (pure)
#pragma clang fp contract(off)
namespace {

struct HullPt { uint64_t x, y; uint32_t edge; int32_t has_edge; };

// > 0: a -> b -> c turns left (b is a strict vertex of the lower hull)
inline __int128 rc_cross(const HullPt &a, const HullPt &b, const HullPt &c) {
  return ((__int128)b.x - (__int128)a.x) * ((__int128)c.y - (__int128)b.y) - ((__int128)b.y - (__int128)a.y) * ((__int128)c.x - (__int128)b.x);
}

inline void rc_push(std::vector<HullPt> &st, const HullPt &p) {
  if (st.back().x == p.x && st.back().y == p.y) {        // the same point again: the later cut names it (not the origin)
    if (st.size() > 1) st.back() = p;
    return;
  }
  while (st.size() >= 2 && rc_cross(st[st.size() - 2], st.back(), p) <= 0) st.pop_back();
  st.push_back(p);
}

}  // namespace

// the chain and the figures: `st` holds the strict vertices, *out everything but the caller's arrays
static int rocch_hull_core(int64_t T, const uint32_t *edge_key, const uint64_t *other_lt, const uint64_t *other_le, const uint64_t *edge_lt,
                           const uint64_t *edge_le, int edge_class, uint64_t Np, uint64_t Nn, int64_t cap_vertices, plda_rocch *out,
                           const plda_rocch_vertex *vertices, const double *llr, std::vector<HullPt> &st) {
  if (!out) return PLDA_E_INVAL;
  std::memset(out, 0, sizeof(*out));
  out->np = Np; out->nn = Nn;
  if (T < 1 || !edge_key || !other_lt || !other_le || !edge_lt || !edge_le || (edge_class != 0 && edge_class != 1) || Np == 0 || Nn == 0 ||
      cap_vertices < 0 || (cap_vertices > 0 && (!vertices || !llr)))
    return PLDA_E_INVAL;
  const uint64_t Ne = edge_class ? Np : Nn, No = edge_class ? Nn : Np;
  st.clear();
  st.push_back(HullPt{0, 0, 0u, 0});
  uint64_t pe = 0, po = 0;                                // the counts through the previous key: every sequence is monotone
  for (int64_t j = 0; j < T; ++j) {
    if (j > 0 && edge_key[j] <= edge_key[j - 1]) return PLDA_E_INVAL;
    if (edge_lt[j] != pe || edge_le[j] <= edge_lt[j] || edge_le[j] > Ne || other_lt[j] < po || other_le[j] < other_lt[j] || other_le[j] > No)
      return PLDA_E_INVAL;
    pe = edge_le[j]; po = other_le[j];
    const HullPt below = edge_class ? HullPt{other_lt[j], edge_lt[j], edge_key[j] - 1u, 1} : HullPt{edge_lt[j], other_lt[j], edge_key[j] - 1u, 1};
    const HullPt at = edge_class ? HullPt{other_le[j], edge_le[j], edge_key[j], 1} : HullPt{edge_le[j], other_le[j], edge_key[j], 1};
    if (below.x | below.y) rc_push(st, below);            // (nothing below the first key: that cut is the empty one)
    rc_push(st, at);
  }
  if (pe != Ne) return PLDA_E_INVAL;
  rc_push(st, HullPt{Nn, Np, 0xffffffffu, 1});
  const int64_t nv = (int64_t)st.size();
  out->n_vertices = nv;

  // minCllr and the crossing with y / Np = 1 - x / Nn from the integer vertices
  const double dNp = (double)Np, dNn = (double)Nn;
  double sum_t = 0.0, sum_n = 0.0;
  int64_t cross_at = -1;
  for (int64_t i = 1; i < nv; ++i) {
    const uint64_t dn = st[i].x - st[i - 1].x, dt = st[i].y - st[i - 1].y;
    if (dt && dn) {
      sum_t += ((double)dt / dNp) * std::log1p(((double)dn * dNp) / ((double)dt * dNn));
      sum_n += ((double)dn / dNn) * std::log1p(((double)dt * dNn) / ((double)dn * dNp));
    }
    if (cross_at < 0 && (__int128)st[i].y * Nn + (__int128)st[i].x * Np >= (__int128)Np * Nn) cross_at = i;
  }
  out->min_cllr = (sum_t + sum_n) / (2.0 * std::log(2.0));
  {
    const HullPt &a = st[cross_at - 1], &b = st[cross_at];
    const __int128 dx = (__int128)(b.x - a.x), dy = (__int128)(b.y - a.y);
    const __int128 D = dy * Nn + dx * Np;                                  // > 0: the vertices differ
    const __int128 tn = (__int128)Np * Nn - ((__int128)a.y * Nn + (__int128)a.x * Np);   // t = tn / D in (0, 1]
    const __int128 num = (__int128)a.y * D + tn * dy;                     // eer = (a.y + t dy) / Np
    out->eer = (double)num / (dNp * (double)D);
    out->eer_far_lo = (double)(Nn - a.x) / dNn; out->eer_far_hi = (double)(Nn - b.x) / dNn;
    out->eer_frr_lo = (double)a.y / dNp;        out->eer_frr_hi = (double)b.y / dNp;
  }
  return PLDA_OK;
}

// the vertices (their key the EDGE of the cut, their threshold NaN until rocch_finish) and the segment llrs
static void rocch_hull_write(const std::vector<HullPt> &st, uint64_t Np, uint64_t Nn, plda_rocch_vertex *vertices, double *llr) {
  const int64_t nv = (int64_t)st.size();
  const double prior_term = std::log((double)Np / (double)Nn);
  for (int64_t i = 0; i < nv; ++i) {
    vertices[i] = plda_rocch_vertex{st[i].x, st[i].y, Nn - st[i].x, st[i].y, NAN, st[i].edge, st[i].has_edge};
    if (i > 0) {
      const uint64_t dn = st[i].x - st[i - 1].x, dt = st[i].y - st[i - 1].y;
      llr[i - 1] = dt == 0 ? -INFINITY : dn == 0 ? INFINITY : std::log((double)dt / (double)dn) - prior_term;
    }
  }
}

int rocch_hull(int64_t T, const uint32_t *edge_key, const uint64_t *other_lt, const uint64_t *other_le, const uint64_t *edge_lt,
               const uint64_t *edge_le, int edge_class, uint64_t Np, uint64_t Nn, int64_t cap_vertices, plda_rocch *out,
               plda_rocch_vertex *vertices, double *llr) {
  std::vector<HullPt> st;
  PLDA_TRY(rocch_hull_core(T, edge_key, other_lt, other_le, edge_lt, edge_le, edge_class, Np, Nn, cap_vertices, out, vertices, llr, st));
  if ((int64_t)st.size() > cap_vertices) return PLDA_E_CAPACITY;
  rocch_hull_write(st, Np, Nn, vertices, llr);
  return PLDA_OK;
}

int rocch_finish(int64_t nv, plda_rocch_vertex *v, const uint32_t *below, const uint32_t *above) {
  if (nv < 2 || !v || !below || !above) return PLDA_E_INVAL;
  for (int64_t i = 0; i < nv; ++i) {
    if (i == 0) {
      if (above[0] == 0xffffffffu) return PLDA_E_INVAL;
      v[0].threshold = (double)key_score(above[0]);
      continue;
    }
    if (below[i] == 0u) return PLDA_E_INVAL;
    v[i].key = below[i];
    if (i == nv - 1) { v[i].threshold = INFINITY; continue; }
    if (above[i] == 0xffffffffu || above[i] <= below[i]) return PLDA_E_INVAL;
    const double s = (double)key_score(below[i]);
    v[i].threshold = s + ((double)key_score(above[i]) - s) / 2.0;
  }
  return PLDA_OK;
}

// ------------------------------------------------------------------------------------ the device driver
namespace {

struct RankGrid { int64_t rows_per_wg; unsigned grid; };
RankGrid rc_strip_grid(const TrialPiece &pc) {
  const int64_t strips = ceil_div(pc.Nt, (int64_t)EER_STRIP);
  int64_t slices = std::max<int64_t>(1, std::min<int64_t>(pc.rows, (256 * 16) / strips));
  slices = std::max(slices, ceil_div(pc.rows, RC_MAX_ROWS_PER_WG));
  const int64_t rows_per_wg = ceil_div(pc.rows, slices);
  return RankGrid{rows_per_wg, (unsigned)(strips * ceil_div(pc.rows, rows_per_wg))};
}

// ranks the other class of `src` among u[0 .. T) (device, sorted): cnt[0 .. 2 T + 3) on the device, zeroed here
int rc_rank_pass(plda_handle *h, const TrialSource &src, int edge_is_target, const unsigned *u, int64_t T, unsigned *dtab, int64_t w0, int W,
                 unsigned long long *dcnt, unsigned long long *dmisc) {
  PLDA_HIP(h, hipMemsetAsync(dcnt, 0, (size_t)(2 * T + 3) * 8, h->stream));
  rocch_table_kernel<<<1, 256, 0, h->stream>>>(u, T, dtab);
  PLDA_LAUNCH_CHECK(h);
  const size_t lds = (size_t)(RC_TAB + 1 + 2 * W) * 4;
  PLDA_TRY(for_each_piece(src, [&](const TrialPiece &pc) -> int {
    if (pc.cls < 0) {
      const RankGrid g = rc_strip_grid(pc);
      rocch_rank_strip_kernel<<<g.grid, 256, lds, h->stream>>>(pc.scores, pc.ld, pc.rows, pc.Nt, pc.espk, src.tspk, g.rows_per_wg, pc.row_step,
                                                               edge_is_target, u, T, dtab, w0, W, dcnt, dmisc);
    } else if (pc.cls != edge_is_target) {
      const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(pc.Nt, 1024), 4096);
      rocch_rank_flat_kernel<<<grid, 256, lds, h->stream>>>(pc.scores, pc.Nt, edge_is_target, u, T, dtab, w0, W, dcnt, dmisc);
    }
    PLDA_LAUNCH_CHECK(h);
    return PLDA_OK;
  }));
  return PLDA_OK;
}

int rc_sort(plda_handle *h, unsigned *ka, unsigned *kb, unsigned *dhist, int64_t n) {
  const int64_t tiles = ceil_div(n, (int64_t)RC_SORT_TILE);
  unsigned *src = ka, *dst = kb;
  for (int shift = 0; shift < 32; shift += 8) {
    rocch_sort_hist_kernel<<<(unsigned)tiles, 256, 0, h->stream>>>(src, n, shift, tiles, dhist);
    rocch_sort_scan_kernel<<<1, 1024, 0, h->stream>>>(dhist, 256 * tiles);
    rocch_sort_scatter_kernel<<<(unsigned)tiles, 256, 0, h->stream>>>(src, n, shift, tiles, dhist, dst);
    PLDA_LAUNCH_CHECK(h);
    std::swap(src, dst);
  }
  return PLDA_OK;        // (four passes: the sorted keys are in ka again)
}

}  // namespace

static int rocch_device(plda_handle *h, const TrialSource &src, int64_t cap_vertices, plda_rocch *out, plda_rocch_vertex *vertices,
                        double *llr, plda_rocch_points *points, plda_rocch_info *info_out) {
  if (!out || cap_vertices < 0 || (cap_vertices > 0 && (!vertices || !llr)))
    return fail(h, PLDA_E_INVAL, "rocch: the result is NULL, or a vertex capacity without the vertex and llr arrays");
  if (points && (points->cap < 0 || (points->cap > 0 && (!points->edge_key || !points->other_lt || !points->other_le || !points->edge_lt || !points->edge_le))))
    return fail(h, PLDA_E_INVAL, "rocch: the reduced-points record has a capacity without its arrays");
  std::memset(out, 0, sizeof(*out));
  plda_rocch_info info;
  std::memset(&info, 0, sizeof(info));
  const bool lists = src.kind == TrialSource::LISTS;
  const int64_t cap_edge = h->rocch_edge_cap > 0 ? h->rocch_edge_cap : RC_EDGE_CAP;

  // ---- the class totals and the edge class (a matrix: from the speaker ids alone)
  unsigned long long Np, Nn;
  {
    TraceScope ts(h, "rocch.count");
    if (lists) {
      Np = (unsigned long long)src.np; Nn = (unsigned long long)src.nn;
    } else {
      unsigned long long *dn;
      PLDA_TRY(carve(h, h->trial_hist, [&](Layout &c) { c.take(dn, 1); }));
      PLDA_HIP(h, hipMemsetAsync(dn, 0, 8, h->stream));
      const int64_t strips = ceil_div(src.Nt, (int64_t)EER_STRIP);
      const int64_t slices = std::max<int64_t>(1, std::min<int64_t>(src.M, (256 * 16) / strips));
      const int64_t rows_per_wg = ceil_div(src.M, slices);
      rocch_count_kernel<<<(unsigned)(strips * ceil_div(src.M, rows_per_wg)), 256, 0, h->stream>>>(src.espk, src.M, src.tspk, src.Nt, rows_per_wg, dn);
      PLDA_LAUNCH_CHECK(h);
      PLDA_HIP(h, hipMemcpyAsync(&Np, dn, 8, hipMemcpyDeviceToHost, h->stream));
      PLDA_HIP(h, hipStreamSynchronize(h->stream));
      ++info.launches;
      Nn = (unsigned long long)src.M * (unsigned long long)src.Nt - Np;
    }
  }
  out->np = Np; out->nn = Nn;
  info.np = Np; info.nn = Nn;
  if (Np == 0 || Nn == 0) return fail(h, PLDA_E_INVAL, "rocch: need at least one target and one non-target trial");
  const int edge = Np <= Nn ? 1 : 0;                       // 1: the targets are the edge class (also on a tie)
  const unsigned long long Traw = edge ? Np : Nn, Nother = edge ? Nn : Np;
  info.edge_class = edge; info.t_raw = Traw;
  if (Traw > (unsigned long long)cap_edge)
    return fail(h, PLDA_E_CAPACITY, "rocch: the edge class holds %llu trials, PLDA_ROCCH_EDGE_CAP allows %lld", Traw, (long long)cap_edge);
  const int64_t T = (int64_t)Traw;

  const int W = h->rocch_variant == 1 ? 0 : h->rocch_variant == 2 ? 256 : RC_W;
  const int64_t tiles = ceil_div(T, (int64_t)RC_SORT_TILE);
  unsigned *ka, *kb, *dsort, *dtab, *dedges, *dlo, *dhi;
  unsigned long long *dcnt, *dmisc;
  PLDA_TRY(carve(h, h->trial_hist, [&](Layout &c) {
    c.take(dmisc, 4).take(ka, (size_t)T).take(kb, (size_t)T).take(dsort, (size_t)(256 * tiles)).take(dtab, RC_TAB + 1)
     .take(dcnt, (size_t)(2 * T + 3)).take(dedges, RC_VCAP).take(dlo, RC_VCAP).take(dhi, RC_VCAP);
  }));

  // ---- read 1: the keys of the edge class, then their sort
  std::vector<unsigned> hk((size_t)T);
  unsigned long long misc[4] = {0, 0, 0, 0};
  {
    TraceScope ts(h, "rocch.edge");
    PLDA_HIP(h, hipMemsetAsync(dmisc, 0, 32, h->stream));
    PLDA_TRY(for_each_piece(src, [&](const TrialPiece &pc) -> int {
      if (pc.cls < 0) {
        const RankGrid g = rc_strip_grid(pc);
        rocch_edge_strip_kernel<<<g.grid, 256, 0, h->stream>>>(pc.scores, pc.ld, pc.rows, pc.Nt, pc.espk, src.tspk, g.rows_per_wg, edge, ka, Traw, dmisc);
      } else if (pc.cls == edge) {
        rocch_edge_flat_kernel<<<(unsigned)std::min<int64_t>(ceil_div(pc.Nt, 1024), 4096), 256, 0, h->stream>>>(pc.scores, pc.Nt, ka, dmisc);
      }
      PLDA_LAUNCH_CHECK(h);
      return PLDA_OK;
    }));
    ++info.reads; ++info.launches;
    ts.next("rocch.sort");
    PLDA_TRY(rc_sort(h, ka, kb, dsort, T));
    info.launches += 12;
    PLDA_HIP(h, hipMemcpyAsync(hk.data(), ka, (size_t)T * 4, hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipMemcpyAsync(misc, dmisc, 32, hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
    // (the length is the count's own: a matrix whose ids changed in between would show here)
    if (!lists && misc[0] != Traw) return fail(h, PLDA_E_NUMERIC, "rocch: %llu edge keys appended, %llu counted", misc[0], Traw);
    for (int64_t i = 1; i < T; ++i)
      if (hk[(size_t)i] < hk[(size_t)i - 1]) return fail(h, PLDA_E_NUMERIC, "rocch: the edge keys are not sorted at %lld", (long long)i);
  }

  // ---- the window: from a coarse count over every stride-th edge key (a read of its own) when the gaps outnumber it
  int64_t w0 = 0;
  if (W > 0 && T > W) {
    TraceScope ts(h, "rocch.coarse");
    const int64_t stride = ceil_div(T, (int64_t)RC_TAB), nc = ceil_div(T, stride);
    std::vector<unsigned> ck((size_t)nc);
    for (int64_t j = 0; j < nc; ++j) ck[(size_t)j] = hk[(size_t)(j * stride)];
    PLDA_HIP(h, hipMemcpyAsync(kb, ck.data(), (size_t)nc * 4, hipMemcpyHostToDevice, h->stream));
    TrialSource smp = src;
    if (src.kind == TrialSource::MATRIX && src.M >= 4096) smp.every(16);
    PLDA_TRY(rc_rank_pass(h, smp, edge, kb, nc, dtab, 0, (int)nc, dcnt, dmisc));
    std::vector<unsigned long long> cc((size_t)(2 * nc + 3));
    PLDA_HIP(h, hipMemcpyAsync(cc.data(), dcnt, cc.size() * 8, hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipStreamSynchronize(h->stream));           // (ck and cc are this scope's)
    PLDA_HIP(h, hipMemsetAsync(dmisc + 2, 0, 8, h->stream));  // (the other class's non-finite count is the full rank pass's)
    ++info.reads; info.launches += 2; info.coarse_read = 1;
    // coarse interval j = the gaps ((j - 1) stride, j stride] of the full list; the start that covers the most mass
    std::vector<unsigned long long> pre((size_t)nc + 1, 0ull);
    for (int64_t j = 0; j < nc; ++j) pre[(size_t)j + 1] = pre[(size_t)j] + cc[(size_t)(2 * j)] + cc[(size_t)(2 * j + 1)];
    unsigned long long best = 0;
    for (int64_t j = 0; j < nc; ++j) {
      // window starting at gap max(0, (j - 1) stride + 1): the intervals j .. j + span - 1 lie inside it
      const int64_t start = std::min<int64_t>(std::max<int64_t>(0, (j - 1) * stride + 1), T - W);
      const int64_t j_lo = start == 0 ? 0 : ceil_div(start - 1, stride) + 1;        // first interval wholly at or above `start`
      const int64_t j_hi = std::min<int64_t>(nc - 1, (start + W - 1) / stride);     // last interval wholly below start + W
      unsigned long long mass = j_hi >= j_lo ? pre[(size_t)j_hi + 1] - pre[(size_t)j_lo] : cc[(size_t)(2 * j)] + cc[(size_t)(2 * j + 1)];
      if (mass > best) { best = mass; w0 = start; }
    }
  }
  info.window_start = w0; info.window_size = W;

  // ---- read 2: the ranks
  std::vector<unsigned long long> cnt((size_t)(2 * T + 3));
  {
    TraceScope ts(h, "rocch.rank");
    PLDA_TRY(rc_rank_pass(h, src, edge, ka, T, dtab, w0, W, dcnt, dmisc));
    PLDA_HIP(h, hipMemcpyAsync(cnt.data(), dcnt, cnt.size() * 8, hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipMemcpyAsync(misc, dmisc, 32, hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
    ++info.reads; info.launches += 2;
  }
  if (misc[1] + misc[2])
    return fail(h, PLDA_E_INVAL, "rocch: %llu non-finite score(s) among the trials", misc[1] + misc[2]);
  info.n_register = cnt[(size_t)(2 * T + 1)] + cnt[(size_t)(2 * T + 2)];
  for (int64_t i = 0; i <= 2 * T; ++i) {
    const bool in_win = i >= 2 * w0 && i < 2 * (w0 + W);
    (in_win ? info.n_lds : info.n_global_atomic) += cnt[(size_t)i];
  }
  cnt[0] += cnt[(size_t)(2 * T + 1)];
  cnt[(size_t)(2 * T)] += cnt[(size_t)(2 * T + 2)];
  if (info.n_register + info.n_lds + info.n_global_atomic != Nother)
    return fail(h, PLDA_E_NUMERIC, "rocch: %llu trials of the other class ranked, %llu counted", info.n_register + info.n_lds + info.n_global_atomic, Nother);

  // ---- the reduced points: distinct keys, their multiplicities, the other class below and through each
  std::vector<uint32_t> ek;
  std::vector<uint64_t> olt, ole, elt, ele;
  {
    unsigned long long run = 0;                            // the other class below counter i
    int64_t i = 0;
    while (i < T) {
      int64_t e = i + 1;
      while (e < T && hk[(size_t)e] == hk[(size_t)i]) ++e;
      run += cnt[(size_t)(2 * i)];
      ek.push_back(hk[(size_t)i]); olt.push_back(run);
      run += cnt[(size_t)(2 * i + 1)];
      ole.push_back(run); elt.push_back((uint64_t)i); ele.push_back((uint64_t)e);
      for (int64_t q = i + 1; q < e; ++q)
        if (cnt[(size_t)(2 * q)] | cnt[(size_t)(2 * q + 1)]) return fail(h, PLDA_E_NUMERIC, "rocch: a rank landed inside a run of equal edge keys");
      i = e;
    }
  }
  const int64_t Td = (int64_t)ek.size();
  info.t_distinct = (uint64_t)Td;
  if (points) {
    points->T = Td; points->edge_class = edge;
    if (points->cap >= Td) {
      std::memcpy(points->edge_key, ek.data(), (size_t)Td * 4);
      std::memcpy(points->other_lt, olt.data(), (size_t)Td * 8); std::memcpy(points->other_le, ole.data(), (size_t)Td * 8);
      std::memcpy(points->edge_lt, elt.data(), (size_t)Td * 8);  std::memcpy(points->edge_le, ele.data(), (size_t)Td * 8);
    }
  }

  // ---- the hull (host), then read 3: the keys next to its vertices' cuts
  std::vector<HullPt> chain;
  if (rocch_hull_core(Td, ek.data(), olt.data(), ole.data(), elt.data(), ele.data(), edge, Np, Nn, 0, out, nullptr, nullptr, chain) != PLDA_OK)
    return fail(h, PLDA_E_NUMERIC, "rocch: inconsistent counts in the reduced points");
  const int64_t nv = out->n_vertices;
  std::vector<plda_rocch_vertex> hv((size_t)nv);
  std::vector<double> hl((size_t)nv);
  rocch_hull_write(chain, Np, Nn, hv.data(), hl.data());
  std::vector<unsigned> below((size_t)nv, 0u), above((size_t)nv, 0xffffffffu);
  {
    TraceScope ts(h, "rocch.neighbours");
    // chunks of the cuts 1 .. nv - 1.  Slot i of a chunk is cut c0 + i: lo[i] is its largest key; hi[i] is the smallest key
    // above cut c0 + i - 1 (slot 0 of the first chunk: the smallest key of all; of a later chunk: not used).  A chunk that
    // is not the last gets one more slot with the largest word as its edge, so that every key finds a slot and the key above
    // the chunk's last cut is found in the same read.
    for (int64_t c0 = 1; c0 < nv; c0 += RC_VCAP - 1) {
      const int n = (int)std::min<int64_t>(RC_VCAP - 1, nv - c0);
      const bool last = c0 + n == nv;                      // (the last vertex's edge is the largest word already)
      const int ne = last ? n : n + 1;
      std::vector<unsigned> e((size_t)ne, 0xffffffffu), lo((size_t)ne, 0u), hi((size_t)ne, 0xffffffffu);
      for (int i = 0; i < n; ++i) e[(size_t)i] = hv[(size_t)(c0 + i)].key;
      PLDA_HIP(h, hipMemcpyAsync(dedges, e.data(), (size_t)ne * 4, hipMemcpyHostToDevice, h->stream));
      PLDA_HIP(h, hipMemcpyAsync(dlo, lo.data(), (size_t)ne * 4, hipMemcpyHostToDevice, h->stream));
      PLDA_HIP(h, hipMemcpyAsync(dhi, hi.data(), (size_t)ne * 4, hipMemcpyHostToDevice, h->stream));
      PLDA_TRY(for_each_piece(src, [&](const TrialPiece &pc) -> int {
        const int64_t total = pc.rows * pc.Nt;
        rocch_neighbour_kernel<<<(unsigned)std::min<int64_t>(ceil_div(total, 256 * 8), 256 * 16), 256, 0, h->stream>>>(pc.scores, pc.ld, pc.rows, pc.Nt, dedges, ne, dlo, dhi);
        PLDA_LAUNCH_CHECK(h);
        return PLDA_OK;
      }));
      PLDA_HIP(h, hipMemcpyAsync(lo.data(), dlo, (size_t)ne * 4, hipMemcpyDeviceToHost, h->stream));
      PLDA_HIP(h, hipMemcpyAsync(hi.data(), dhi, (size_t)ne * 4, hipMemcpyDeviceToHost, h->stream));
      PLDA_HIP(h, hipStreamSynchronize(h->stream));
      ++info.reads; ++info.launches; ++info.neighbour_reads;
      for (int i = 0; i < n; ++i) below[(size_t)(c0 + i)] = lo[(size_t)i];
      for (int i = c0 == 1 ? 0 : 1; i < ne; ++i) above[(size_t)(c0 + i - 1)] = hi[(size_t)i];
    }
  }
  if (rocch_finish(nv, hv.data(), below.data(), above.data()) != PLDA_OK)
    return fail(h, PLDA_E_NUMERIC, "rocch: the keys next to a vertex were not found (inconsistent counts)");
  if (info_out) *info_out = info;
  if (points && points->cap < Td)
    return fail(h, PLDA_E_CAPACITY, "rocch: %lld reduced points, the caller's arrays hold %lld", (long long)Td, (long long)points->cap);
  if (nv > cap_vertices)
    return fail(h, PLDA_E_CAPACITY, "rocch: the hull has %lld vertices, the caller's array holds %lld", (long long)nv, (long long)cap_vertices);
  std::memcpy(vertices, hv.data(), (size_t)nv * sizeof(plda_rocch_vertex));
  std::memcpy(llr, hl.data(), (size_t)(nv - 1) * sizeof(double));
  return PLDA_OK;
}

int rocch_matrix_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *despk, const int64_t *dtspk,
                        int64_t cap_vertices, plda_rocch *out, plda_rocch_vertex *vertices, double *llr, plda_rocch_points *points,
                        plda_rocch_info *info) {
  if (!out || !dscores || !despk || !dtspk || M <= 0 || Nt <= 0 || ld < Nt) return fail(h, PLDA_E_INVAL, "rocch: bad argument");
  return rocch_device(h, TrialSource::matrix(dscores, ld, M, Nt, despk, dtspk), cap_vertices, out, vertices, llr, points, info);
}

int rocch_lists_device(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, int64_t cap_vertices, plda_rocch *out,
                       plda_rocch_vertex *vertices, double *llr, plda_rocch_points *points, plda_rocch_info *info) {
  if (!dpos || !dneg || !out || np <= 0 || nn <= 0) return fail(h, PLDA_E_INVAL, "rocch: need at least one target and one non-target score");
  return rocch_device(h, TrialSource::lists(dpos, np, dneg, nn), cap_vertices, out, vertices, llr, points, info);
}

int score_rocch_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV, int64_t Nt,
                       const double *dzmean, const double *dzstd, const int64_t *despk, const int64_t *dtspk, int64_t cap_vertices,
                       plda_rocch *out, plda_rocch_vertex *vertices, double *llr, plda_rocch_points *points, plda_rocch_info *info) {
  OperandSlabs os;
  TrialSource src;
  PLDA_TRY(operand_source(h, "score_rocch", dU, dn, n_uniform, M, dV, Nt, dzmean, dzstd, despk, dtspk, out, &os, &src));
  return rocch_device(h, src, cap_vertices, out, vertices, llr, points, info);
}

// The table of the map: the interior vertices' keys and, per segment, (float) clamp(llr, -bound, bound) (bound <= 0: as it
// is).  More than RC_VCAP segments: PLDA_E_CAPACITY (no global-table fall-back: the hull of 2e4 targets against 1e7
// non-targets has 134 vertices).  The table is uploaded into h->trial_hist and the stream synchronised once for it; the map
// kernel itself is enqueued and not waited for.
int pav_map_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, int64_t n_vertices,
                   const plda_rocch_vertex *vertices, const double *llr, double bound, float *dout, int64_t ld_out) {
  if (!dscores || !dout || !vertices || !llr || M <= 0 || Nt <= 0 || ld < Nt || ld_out < Nt || n_vertices < 2 || bound != bound)
    return fail(h, PLDA_E_INVAL, "pav_map: bad argument");
  const int64_t nseg = n_vertices - 1;
  if (nseg > RC_VCAP) return fail(h, PLDA_E_CAPACITY, "pav_map: %lld segments, the table holds %d", (long long)nseg, RC_VCAP);
  if (ceil_div(Nt, (int64_t)EER_STRIP) > (int64_t)0x7fffffff) return fail(h, PLDA_E_CAPACITY, "pav_map: too many column strips");
  std::vector<unsigned> keys((size_t)std::max<int64_t>(nseg - 1, 1), 0u);
  std::vector<float> tab((size_t)nseg);
  for (int64_t i = 0; i < nseg; ++i) {
    double v = llr[i];
    if (v != v) return fail(h, PLDA_E_INVAL, "pav_map: llr[%lld] is NaN", (long long)i);
    if (i > 0 && v < llr[i - 1]) return fail(h, PLDA_E_INVAL, "pav_map: the llrs must not decrease");
    if (bound > 0.0) v = std::min(std::max(v, -bound), bound);
    tab[(size_t)i] = (float)v;
    if (i + 1 < nseg) {
      if (!vertices[i + 1].has_key || (i > 0 && vertices[i + 1].key <= vertices[i].key)) return fail(h, PLDA_E_INVAL, "pav_map: the vertex keys must ascend");
      keys[(size_t)i] = vertices[i + 1].key;
    }
  }
  unsigned *dkeys;
  float *dtab;
  // (the labelled passes' buffer: every call that uses it lays it out anew, and work on the stream is ordered)
  PLDA_TRY(carve(h, h->trial_hist, [&](Layout &c) { c.take(dkeys, RC_VCAP).take(dtab, RC_VCAP); }));
  PLDA_HIP(h, hipMemcpyAsync(dkeys, keys.data(), keys.size() * 4, hipMemcpyHostToDevice, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(dtab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));            // (keys and tab are this call's: the copies must have read them)
  const dim3 grid((unsigned)ceil_div(Nt, (int64_t)EER_STRIP), (unsigned)std::min<int64_t>(M, 4096));
  pav_map_kernel<<<grid, 256, 0, h->stream>>>(dscores, ld, M, Nt, dkeys, dtab, (int)nseg, dout, ld_out);
  PLDA_LAUNCH_CHECK(h);
  return PLDA_OK;
}

}  // namespace plda
