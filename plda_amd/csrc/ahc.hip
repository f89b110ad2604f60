// plda_amd/csrc/ahc.hip -- speaker clustering: batched average-linkage agglomerative clustering (AHC / UPGMA) on PLDA score
// blocks (the contract is in include/plda_hip.h, the bit-exact host model in tests/ahc_model.py).
//
// The reference stops at verification; Kaldi's PLDA is also the back-end of diarisation (ivector-plda-scoring-dense +
// agglomerative-cluster): every segment of a recording is scored against every other one and the segments are merged
// bottom-up.  A recording is a chain of up to N - 1 DEPENDENT merges, each a few microseconds of work: one workgroup per
// recording, many recordings in flight.
//
//   cluster_count_kernel<AhcRec>  (common.hpp) the non-finite off-diagonal scores of every recording of the call (one integer
//                       counter; a call that meets one fails, and the kernels behind it write nothing)
//   ahc_load_kernel     HBM class: the fp32 block symmetrised into an N x N fp64 matrix of sums in handle scratch
//                       (c(i, j) = -((double)S[i, j] + (double)S[j, i]) / 2, both steps exact; the tile body is ahc_load_tile,
//                       which the wide class's ahcw_load_kernel shares); the LDS class symmetrises straight into LDS at the
//                       head of its merge kernel
//   ahc_merge_kernel    <HBM = false> the strict upper triangle of fp64 sums in LDS, N <= ahc_lds_max();
//                       <HBM = true>  the full symmetric matrix in scratch (row a and row b of a merge are then contiguous).
//                       Both keep the per-slot state in LDS: size, best partner b > a and its v, the member list of the slot.
//   ahc_label_kernel    the final slot of every segment -> cluster numbers 0 .. k - 1 by ascending slot
//   ahcw_*_kernel       the WIDE class (K28, at the end of the file): ONE problem of up to PLDA_AHC_WIDE_MAX vectors on the whole
//                       device under the same contract -- the state in handle scratch, a step cut into three launches; its
//                       count and load kernels are one-block wrappers of cluster_count_block and ahc_load_tile
//
// One step: (1) the global minimum (v, a) is a workgroup reduction over the row cache; (2) sum(a, x) += sum(b, x) for every
// live x, and while x is in hand: a row x < a whose cached partner was a or b, or a row a < x < b whose partner was b, is
// queued for a rescan; any other row x < a takes the new v(x, a) if it beats its cache under (v, then partner index);
// (3) sizes and member lists change hands; (4) the queued rows and row a are rescanned, one wave per row.  Rows above b hold
// only partners above b and are untouched.  Every comparison is on the total order (v, a, b) with IEEE ==, so -0.0 == +0.0,
// and every v is one fp64 division of the sum by the integer product of the sizes: the result does not depend on the order
// in which waves take rows, on the grid or on the grouping into launches.  (The file is built with -ffp-contract=off; it has
// no fast-math and no reciprocal.)
#include "common.hpp"
#include "slab_walk.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace plda {

namespace {

constexpr int AHC_MAX = PLDA_AHC_MAX;
constexpr int AHC_LDS_BYTES = 160 * 1024;      // one workgroup may hold all of a CU's LDS
constexpr int AHC_FIXED_BYTES = 512;           // reduction slots and step scalars
constexpr int AHC_SLOT_BYTES = 8 + 5 * 4;      // bv | bp, sz, list, next, tail
constexpr int AHC_T_LDS = 256, AHC_T_HBM = 1024;
constexpr int AHC_MAX_WAVES = AHC_T_HBM / 64;

// one recording of a launch (host-built, uploaded once per enqueue)
struct AhcRec {
  long long boff;    // first float of the block, relative to the scores pointer
  long long off;     // first segment (labels, slots)
  long long scr;     // HBM class: first double of the N x N sums in scratch
  int n, r, minc, pad;
};

constexpr long long ahc_tri(long long n) { return n * (n - 1) / 2; }
constexpr long long ahc_lds_bytes(long long n, bool hbm) {
  return (hbm ? 0 : 8 * ahc_tri(n)) + (long long)AHC_SLOT_BYTES * n + AHC_FIXED_BYTES;
}
constexpr int ahc_lds_max_calc() {
  int n = 1;
  while (n < AHC_MAX && ahc_lds_bytes(n + 1, false) <= AHC_LDS_BYTES) ++n;
  return n;
}
constexpr int AHC_LDS_MAX = ahc_lds_max_calc();
static_assert(ahc_lds_bytes(AHC_LDS_MAX, false) <= AHC_LDS_BYTES, "the LDS class must fit one CU's LDS");
static_assert(ahc_lds_bytes(AHC_MAX, true) <= AHC_LDS_BYTES, "the HBM class's slot state must fit one CU's LDS");

__device__ __forceinline__ double ahc_cost(float sij, float sji) { return -(((double)sij + (double)sji) / 2.0); }

// lexicographic minimum of (v, i) over the wave, i < 0 = nothing; every lane ends with the result
__device__ __forceinline__ void ahc_wave_min(double &v, int &i) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    if (oi >= 0 && (i < 0 || ov < v || (ov == v && oi < i))) { v = ov; i = oi; }
  }
}

// 32 x 32 threads: tile (ti, tj) of M[i, j] = c(i, j) (M dense, n x n) from the block at S with row stride ld, the transposed
// tile through LDS; diagonal 0.  Every thread of the workgroup must arrive.
__device__ __forceinline__ void ahc_load_tile(const float *__restrict__ S, int n, long long ld, int ti, int tj, double *__restrict__ M) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x, ty = threadIdx.y;
  {   // the mirror tile: rows tj * 32 .., columns ti * 32 ..
    const int r = tj * 32 + ty, c = ti * 32 + tx;
    tile[ty][tx] = (r < n && c < n) ? S[(long long)r * ld + c] : 0.f;
  }
  __syncthreads();
  const int i = ti * 32 + ty, j = tj * 32 + tx;
  if (i < n && j < n) M[(long long)i * n + j] = i == j ? 0.0 : ahc_cost(S[(long long)i * ld + j], tile[tx][ty]);
}

// grid (tiles, recordings of the group): the tiles of every recording's block, found through the launch table
__global__ __launch_bounds__(1024) void ahc_load_kernel(const float *__restrict__ S, const AhcRec *__restrict__ tab,
                                                        double *__restrict__ scratch, const unsigned long long *__restrict__ bad) {
  if (*bad) return;
  const AhcRec rc = tab[blockIdx.y];
  const int n = rc.n, nt = (n + 31) / 32;
  if ((int)blockIdx.x >= nt * nt) return;
  const int ti = blockIdx.x / nt;
  ahc_load_tile(S + rc.boff, n, n, ti, blockIdx.x - ti * nt, scratch + rc.scr);
}

// the sums of a recording: the strict upper triangle in LDS, or the full symmetric matrix in HBM
template <bool HBM> struct AhcSums;
template <> struct AhcSums<false> {
  double *t; int n;
  __device__ __forceinline__ int idx(int i, int j) const { return i * (2 * n - i - 1) / 2 + (j - i - 1); }   // i < j
  __device__ __forceinline__ double get(int i, int j) const { return i < j ? t[idx(i, j)] : t[idx(j, i)]; }
  __device__ __forceinline__ void set(int i, int j, double s) const { if (i < j) t[idx(i, j)] = s; else t[idx(j, i)] = s; }
};
template <> struct AhcSums<true> {
  double *m; int n;
  __device__ __forceinline__ double get(int i, int j) const { return m[(long long)i * n + j]; }
  __device__ __forceinline__ void set(int i, int j, double s) const { m[(long long)i * n + j] = s; m[(long long)j * n + i] = s; }
};

// row x's best partner y in [y0, y1), y0 > x, among the live slots, by (v, y); one wave, every lane gets the result
template <bool HBM>
__device__ __forceinline__ void ahc_scan_row(const AhcSums<HBM> &sums, const int *sz, int x, int y0, int y1, int lane, double &bv,
                                             int &bp) {
  const int sx = sz[x];
  double v = 0.0;
  int p = -1;
#pragma unroll 4
  for (int y = y0 + lane; y < y1; y += 64) {
    const int sy = sz[y];
    const double s = sums.get(x, y);             // (a dead slot's entry is stale, in range and unused: the loads of the
    if (sy > 0) {                                //  unrolled iterations are in flight together)
      const double c = s / (double)(sx * sy);
      if (p < 0 || c < v) { v = c; p = y; }      // y ascends within a lane: a tie keeps the smaller y
    }
  }
  ahc_wave_min(v, p);
  bv = v; bp = p;
}

template <bool HBM, int T>
__global__ __launch_bounds__(T) void ahc_merge_kernel(const float *__restrict__ S, const AhcRec *__restrict__ tab, double *scratch,
                                                      const unsigned long long *__restrict__ bad, int has_thr, double thr,
                                                      int *__restrict__ slot, int *__restrict__ n_clusters,
                                                      int *__restrict__ merge_a, int *__restrict__ merge_b,
                                                      double *__restrict__ merge_cost) {
  extern __shared__ double ahc_smem[];
  if (*bad) return;
  constexpr int W = T / 64;
  const AhcRec rc = tab[blockIdx.x];
  const int n = rc.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // LDS: [triangle (LDS class)] | bv[n] | red_v[16] | bp[n] sz[n] list[n] next[n] tail[n] | red_i[16] | cnt
  double *p8 = ahc_smem;
  AhcSums<HBM> sums;
  if constexpr (HBM) { sums.m = scratch + rc.scr; sums.n = n; }
  else { sums.t = p8; sums.n = n; p8 += ahc_tri(n); }
  double *bv = p8; p8 += n;
  double *red_v = p8; p8 += AHC_MAX_WAVES;
  int *p4 = reinterpret_cast<int *>(p8);
  int *bp = p4; p4 += n;
  int *sz = p4; p4 += n;
  int *list = p4; p4 += n;
  int *next = p4; p4 += n;
  int *tail = p4; p4 += n;
  int *red_i = p4; p4 += AHC_MAX_WAVES;
  int *cnt = p4;

  if constexpr (!HBM) {
    const float *__restrict__ blk = S + rc.boff;
    for (int i = 0; i < n - 1; ++i)
      for (int j = i + 1 + tid; j < n; j += T) sums.t[sums.idx(i, j)] = ahc_cost(blk[(long long)i * n + j], blk[(long long)j * n + i]);
  }
  for (int x = tid; x < n; x += T) { sz[x] = 1; next[x] = -1; tail[x] = x; }
  if (tid == 0) *cnt = 0;
  __syncthreads();
  for (int x = wave; x < n; x += W) {
    double v; int p;
    ahc_scan_row<HBM>(sums, sz, x, x + 1, n, lane, v, p);
    if (lane == 0) { bv[x] = v; bp[x] = p; }
  }
  __syncthreads();

  const int stop_k = rc.minc > 1 ? rc.minc : 1;
  const long long mbase = rc.off - rc.r;      // this recording's first entry of the merge record
  const double neg_thr = -thr;
  int k = n, m = 0;
  while (k > stop_k) {
    // (1) the pair to merge: minimum over the row cache by (v, a); b comes with the row
    double v = 0.0;
    int a = -1;
    for (int x = tid; x < n; x += T) {
      if (sz[x] > 0 && bp[x] >= 0) {
        const double c = bv[x];
        if (a < 0 || c < v) { v = c; a = x; }    // x ascends within a thread
      }
    }
    ahc_wave_min(v, a);
    if (lane == 0) { red_v[wave] = v; red_i[wave] = a; }
    __syncthreads();
    v = red_v[0]; a = red_i[0];
#pragma unroll
    for (int w = 1; w < W; ++w) {
      const double ov = red_v[w];
      const int oi = red_i[w];
      if (oi >= 0 && (a < 0 || ov < v || (ov == v && oi < a))) { v = ov; a = oi; }
    }
    if (a < 0) break;                            // (cannot happen while k > 1; keeps every index below in range)
    if (has_thr && !(v <= neg_thr)) break;
    const int b = bp[a];
    if (tid == 0 && merge_a) { merge_a[mbase + m] = a; merge_b[mbase + m] = b; merge_cost[mbase + m] = v; }
    // (2) the sums of a take b's; rows whose cache the merge touches
    const int nsa = sz[a] + sz[b];
    for (int x = tid; x < n; x += T) {
      const int sx = sz[x];
      if (sx <= 0 || x == a || x == b) continue;
      const double s = sums.get(a, x) + sums.get(b, x);
      sums.set(a, x, s);
      if (x < a) {
        const int p = bp[x];
        if (p == a || p == b) list[atomicAdd(cnt, 1)] = x;
        else {
          const double c = s / (double)(nsa * sx);
          if (c < bv[x] || (c == bv[x] && a < p)) { bv[x] = c; bp[x] = a; }
        }
      } else if (x < b) {
        if (bp[x] == b) list[atomicAdd(cnt, 1)] = x;
      }
    }
    __syncthreads();
    // (3) sizes and members
    if (tid == 0) {
      sz[a] = nsa; sz[b] = 0;
      next[tail[a]] = b; tail[a] = tail[b];
      list[atomicAdd(cnt, 1)] = a;
    }
    __syncthreads();
    // (4) rescans: one wave per row, or -- fewer rows than waves, the usual case -- W / nl waves per row, each on a piece of
    // the row, combined in the order of the pieces (the order (v, y) is total: the split does not change the result)
    const int nl = *cnt;
    const int parts = nl >= W ? 1 : W / nl;
    if (parts == 1) {
      for (int q = wave; q < nl; q += W) {
        const int x = list[q];
        double c; int p;
        ahc_scan_row<HBM>(sums, sz, x, x + 1, n, lane, c, p);
        if (lane == 0) { bv[x] = c; bp[x] = p; }
      }
    } else {
      const int q = wave / parts, pi = wave - q * parts;
      if (q < nl) {
        const int x = list[q];
        const int seg = ((n - x - 1 + parts - 1) / parts + 63) & ~63;
        const int y0 = x + 1 + pi * seg, y1 = min(y0 + seg, n);
        double c; int p;
        ahc_scan_row<HBM>(sums, sz, x, y0, y1, lane, c, p);
        if (lane == 0) { red_v[wave] = c; red_i[wave] = p; }
      }
      __syncthreads();
      if (tid < nl) {
        double c = 0.0;
        int p = -1;
        for (int j = 0; j < parts; ++j) {
          const double oc = red_v[tid * parts + j];
          const int op = red_i[tid * parts + j];
          if (op >= 0 && (p < 0 || oc < c)) { c = oc; p = op; }      // the pieces ascend in y: a tie keeps the smaller y
        }
        const int x = list[tid];
        bv[x] = c; bp[x] = p;
      }
    }
    __syncthreads();
    if (tid == 0) *cnt = 0;                      // (the next append is behind the next step's first barrier)
    --k; ++m;
  }

  // the unused tail of the merge record, the count, and every segment's final slot
  if (merge_a)
    for (int q = m + tid; q < n - 1; q += T) { merge_a[mbase + q] = -1; merge_b[mbase + q] = -1; merge_cost[mbase + q] = INFINITY; }
  if (tid == 0) n_clusters[rc.r] = k;
  for (int s = tid; s < n; s += T)
    if (sz[s] > 0)
      for (int i = s; i >= 0; i = next[i]) slot[rc.off + i] = s;
}

// one workgroup per recording: a slot is live iff slot[s] == s; label = the number of live slots below the segment's slot
__global__ __launch_bounds__(256) void ahc_label_kernel(const AhcRec *__restrict__ tab, const int *__restrict__ slot,
                                                        const unsigned long long *__restrict__ bad, int *__restrict__ labels) {
  __shared__ int rank[AHC_MAX];
  __shared__ int part[256];
  if (*bad) return;
  const AhcRec rc = tab[blockIdx.x];
  const int n = rc.n, tid = threadIdx.x;
  const int *__restrict__ sl = slot + rc.off;
  const int per = (n + 255) / 256, s0 = min(tid * per, n), s1 = min(s0 + per, n);
  int c = 0;
  for (int s = s0; s < s1; ++s) c += sl[s] == s ? 1 : 0;
  part[tid] = c;
  __syncthreads();
  int base = 0;
  for (int t = 0; t < tid; ++t) base += part[t];
  for (int s = s0; s < s1; ++s) { rank[s] = base; base += sl[s] == s ? 1 : 0; }
  __syncthreads();
  for (int i = tid; i < n; i += 256) labels[rc.off + i] = rank[sl[i]];
}

template <bool HBM, int T> int ahc_merge_attr(plda_handle *h) {
  static DeviceOnce attr;
  if (attr.needed(h->device)) {
    PLDA_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&ahc_merge_kernel<HBM, T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    AHC_LDS_BYTES));
    attr.done(h->device);
  }
  return PLDA_OK;
}

// Enqueues the clustering of recordings [r0, r1) whose blocks start at dscores + boff[r - r0].  `tables` keeps the host copy
// of the launch table alive until the caller has synchronised.  h->ahc_stat[0] must have been zeroed by the caller.
int ahc_enqueue(plda_handle *h, const float *dscores, const int64_t *boff, const int64_t *offsets, int64_t r0, int64_t r1,
                const AhcArgs &a, std::vector<std::vector<AhcRec>> &tables) {
  const int64_t cnt = r1 - r0;
  if (cnt <= 0) return PLDA_OK;
  static const int bucket_top[] = {64, 96, 128, 160, AHC_LDS_MAX};
  constexpr int NB = sizeof(bucket_top) / sizeof(bucket_top[0]);
  struct Launch { int64_t first, count; int nmax; bool hbm; int64_t scratch; };
  std::vector<Launch> launches;
  tables.emplace_back();
  std::vector<AhcRec> &tab = tables.back();
  tab.reserve((size_t)cnt);
  auto rec_of = [&](int64_t r) {
    AhcRec rc;
    rc.boff = boff[r - r0]; rc.off = offsets[r]; rc.scr = 0; rc.n = (int)(offsets[r + 1] - offsets[r]); rc.r = (int)r;
    rc.minc = a.minc ? a.minc[r] : 1; rc.pad = 0;
    return rc;
  };
  for (int bk = 0; bk < NB; ++bk) {           // LDS class: one launch per size bucket (the LDS of a launch is its largest N's)
    const int lo = bk ? bucket_top[bk - 1] : 0, hi = bucket_top[bk];
    Launch L{(int64_t)tab.size(), 0, 0, false, 0};
    for (int64_t r = r0; r < r1; ++r) {
      const int64_t n = offsets[r + 1] - offsets[r];
      if (n > lo && n <= hi) { tab.push_back(rec_of(r)); ++L.count; L.nmax = std::max(L.nmax, (int)n); }
    }
    if (L.count) launches.push_back(L);
  }
  const int64_t budget = cluster_budget(h);
  int64_t scratch_need = 0;
  {                                           // HBM class: launches under the scratch budget
    Launch L{(int64_t)tab.size(), 0, 0, true, 0};
    for (int64_t r = r0; r < r1; ++r) {
      const int64_t n = offsets[r + 1] - offsets[r];
      if (n <= AHC_LDS_MAX) continue;
      const int64_t bytes = n * n * 8;
      if (L.count && (L.scratch + bytes > budget || L.count >= 32768)) {
        launches.push_back(L);
        L = Launch{(int64_t)tab.size(), 0, 0, true, 0};
      }
      AhcRec rc = rec_of(r);
      rc.scr = L.scratch / 8;
      tab.push_back(rc);
      ++L.count; L.nmax = std::max(L.nmax, (int)n); L.scratch += bytes;
      scratch_need = std::max(scratch_need, L.scratch);
    }
    if (L.count) launches.push_back(L);
  }
  if (scratch_need) PLDA_HIP(h, h->ahc_scratch.reserve((size_t)scratch_need));
  PLDA_HIP(h, h->ahc_tab.reserve(tab.size() * sizeof(AhcRec)));
  PLDA_HIP(h, h->ahc_slot.reserve((size_t)offsets[r1] * 4));       // (indexed by the call's segment numbers)
  PLDA_HIP(h, hipMemcpyAsync(h->ahc_tab.p, tab.data(), tab.size() * sizeof(AhcRec), hipMemcpyHostToDevice, h->stream));
  const AhcRec *dtab = h->ahc_tab.as<AhcRec>();
  unsigned long long *dbad = h->ahc_stat.as<unsigned long long>();
  double *scratch = h->ahc_scratch.as<double>();
  int *dslot = h->ahc_slot.as<int>();
  PLDA_TRY((ahc_merge_attr<false, AHC_T_LDS>(h)));
  PLDA_TRY((ahc_merge_attr<true, AHC_T_HBM>(h)));

  TraceScope ts(h, "ahc.count");
  PLDA_TRY(cluster_count_enqueue(h, dscores, tab.data(), cnt, dtab, dbad));
  ts.next("ahc.merge");
  for (const Launch &L : launches) {
    const size_t lds = (size_t)ahc_lds_bytes(L.nmax, L.hbm);
    if (L.hbm) {
      const int nt = (L.nmax + 31) / 32;
      ahc_load_kernel<<<dim3((unsigned)(nt * nt), (unsigned)L.count), dim3(32, 32), 0, h->stream>>>(dscores, dtab + L.first, scratch, dbad);
      PLDA_LAUNCH_CHECK(h);
      ahc_merge_kernel<true, AHC_T_HBM><<<(unsigned)L.count, AHC_T_HBM, lds, h->stream>>>(
          dscores, dtab + L.first, scratch, dbad, a.has_thr, a.thr, dslot, a.n_clusters, a.merge_a, a.merge_b, a.merge_cost);
    } else {
      ahc_merge_kernel<false, AHC_T_LDS><<<(unsigned)L.count, AHC_T_LDS, lds, h->stream>>>(
          dscores, dtab + L.first, nullptr, dbad, a.has_thr, a.thr, dslot, a.n_clusters, a.merge_a, a.merge_b, a.merge_cost);
    }
    PLDA_LAUNCH_CHECK(h);
  }
  ts.next("ahc.label");
  for (int64_t c0 = 0; c0 < cnt; c0 += 65536) {      // (the table is in launch order; the labels do not care)
    const int64_t c = std::min<int64_t>(65536, cnt - c0);
    ahc_label_kernel<<<(unsigned)c, 256, 0, h->stream>>>(dtab + c0, dslot, dbad, a.labels);
    PLDA_LAUNCH_CHECK(h);
  }
  return PLDA_OK;
}

// the checks the batched and the wide class share, between each one's own first and last ones
int ahc_check_outputs(plda_handle *h, const char *fn, const AhcArgs &a) {
  if (!a.labels) return fail(h, PLDA_E_INVAL, "%s: labels is NULL", fn);
  if (!a.n_clusters) return fail(h, PLDA_E_INVAL, "%s: n_clusters is NULL", fn);
  const int nm = (a.merge_a ? 1 : 0) + (a.merge_b ? 1 : 0) + (a.merge_cost ? 1 : 0);
  if (nm != 0 && nm != 3) return fail(h, PLDA_E_INVAL, "%s: merge_a, merge_b and merge_cost must be given together or not at all", fn);
  if (a.has_thr && std::isnan(a.thr)) return fail(h, PLDA_E_INVAL, "%s: threshold is NaN", fn);
  return PLDA_OK;
}

// ================================================================================================ the wide class (K28)
// ONE problem of N <= PLDA_AHC_WIDE_MAX vectors on the whole device: the same contract, the state in handle scratch, a step
// cut into three launches (select, update, rescan) so that launch boundaries are the only synchronisation between
// workgroups.  No kernel waits on another workgroup; every loop is bounded by N; every kernel returns at once when the
// control block's `done` is set.
constexpr int AHCW_MAX = PLDA_AHC_WIDE_MAX;
constexpr int AHCW_LAUNCHES = 3;               // select, update, rescan
constexpr int AHCW_BATCH = 256;                // steps between two host reads of `done` (a threshold run only)
constexpr int AHCW_T = 256;                    // update: rows per workgroup; rescan: threads of a piece
constexpr int AHCW_T_SELECT = 1024;
constexpr int AHCW_PIECE_ALIGN = 256;          // a piece's length is a multiple of this
constexpr int AHCW_PIECE_COLS = 4096;          // default: one piece per this many columns, at most AHCW_PIECES_MAX
constexpr int AHCW_PIECES_DEFAULT_MAX = 8, AHCW_PIECES_MAX = 64;
constexpr int AHCW_SCAN_ROWS = 128;            // rescan: the rows of the grid (it strides over the list)
constexpr int AHCW_JUMP_ROUNDS = 16;           // pointer jumping: a chain of parents is shorter than 2^15
static_assert(AHCW_MAX <= (1 << 15), "the jump rounds, the 32-bit size product and the label kernel's LDS assume N <= 2^15");

struct AhcwCtl { int done, m, k, a, b, nsa, cnt, pad; };   // merge cursor m, live slots k, the step's pair and new size, list length

// the arrays of the wide class in h->ahc_scratch: one layout list (common.hpp: carve)
struct AhcwState {
  float *block;            // the operand form's fp32 score block [N, N] (the matrix form: empty)
  double *sums;            // [N, N] fp64, full and symmetric
  double *bv;              // [N] row cache: the value of the best partner
  double *part_v;          // [(N + 1) * P] a row scan's partial results, by list position and piece
  int *sz, *bp, *parent;   // [N] sizes (0: dead), row cache: best partner b > a (-1: none), parent[b] = a of the merge that ended b
  int *list;               // [N + 1] the rows a step rescans (list positions 0 .. cnt - 1; row a is position cnt)
  int *part_p;             // [(N + 1) * P]
  unsigned *arrive;        // [N + 1] pieces of a list position that have finished (back to 0 when the last one has combined)
  AhcwCtl *ctl;
  void lay(Layout &c, size_t n, size_t P, bool with_block) {
    c.take(block, with_block ? n * n : 0, 256).take(sums, n * n, 256).take(bv, n).take(part_v, (n + 1) * P).take(sz, n).take(bp, n)
        .take(parent, n).take(list, n + 1).take(part_p, (n + 1) * P).take(arrive, n + 1).take(ctl, 1);
  }
};

int ahcw_batch(const plda_handle *h) { return h->ahc_wide_batch >= 1 && h->ahc_wide_batch <= 65536 ? (int)h->ahc_wide_batch : AHCW_BATCH; }
int ahcw_pieces(const plda_handle *h, int64_t n) {
  if (h->ahc_wide_pieces >= 1 && h->ahc_wide_pieces <= AHCW_PIECES_MAX) return (int)h->ahc_wide_pieces;
  return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, (int64_t)AHCW_PIECE_COLS), AHCW_PIECES_DEFAULT_MAX));
}
int ahcw_piece_len(int64_t n, int P) { return (int)round_up(ceil_div(n, (int64_t)P), (int64_t)AHCW_PIECE_ALIGN); }

// grid (pieces): the off-diagonal scores that are not finite, added to *bad
__global__ __launch_bounds__(256) void ahcw_count_kernel(const float *__restrict__ S, int n, long long ld, unsigned long long *bad) {
  cluster_count_block(S, n, ld, bad);
}

// grid (tiles, tiles), 32 x 32 threads: sums[i, j] = c(i, j)
__global__ __launch_bounds__(1024) void ahcw_load_kernel(const float *__restrict__ S, int n, long long ld, double *__restrict__ sums,
                                                         const unsigned long long *__restrict__ bad) {
  if (*bad) return;
  ahc_load_tile(S, n, ld, blockIdx.y, blockIdx.x, sums);
}

// grid over x: every slot alive and its own parent, every row on the list (the first rescan fills the whole row cache)
__global__ __launch_bounds__(AHCW_T) void ahcw_init_kernel(int n, AhcwState st, const unsigned long long *__restrict__ bad) {
  const int x = blockIdx.x * AHCW_T + threadIdx.x;
  if (x < n) { st.sz[x] = 1; st.parent[x] = x; st.list[x] = x; st.arrive[x] = 0u; }
  if (x == 0) {
    st.arrive[n] = 0u;
    AhcwCtl c;
    c.done = *bad ? 1 : 0; c.m = 0; c.k = n; c.a = -1; c.b = -1; c.nsa = 0; c.cnt = n; c.pad = 0;
    *st.ctl = c;
  }
}

// one workgroup: the pair to merge is the minimum over the row cache by (v, a), b comes with the row; the stop rule; the merge
// entry, the sizes, the parent of b and the step's descriptor
__global__ __launch_bounds__(AHCW_T_SELECT) void ahcw_select_kernel(int n, AhcwState st, int stop_k, int has_thr, double neg_thr,
                                                                    int *__restrict__ merge_a, int *__restrict__ merge_b,
                                                                    double *__restrict__ merge_cost) {
  __shared__ double red_v[AHCW_T_SELECT / 64];
  __shared__ int red_i[AHCW_T_SELECT / 64];
  if (st.ctl->done) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double v = 0.0;
  int a = -1;
  for (int x = tid; x < n; x += AHCW_T_SELECT) {
    if (st.sz[x] > 0 && st.bp[x] >= 0) {
      const double c = st.bv[x];
      if (a < 0 || c < v) { v = c; a = x; }      // x ascends within a thread
    }
  }
  ahc_wave_min(v, a);
  if (lane == 0) { red_v[wave] = v; red_i[wave] = a; }
  __syncthreads();
  if (tid != 0) return;
  v = red_v[0]; a = red_i[0];
  for (int w = 1; w < AHCW_T_SELECT / 64; ++w) {
    const double ov = red_v[w];
    const int oi = red_i[w];
    if (oi >= 0 && (a < 0 || ov < v || (ov == v && oi < a))) { v = ov; a = oi; }
  }
  AhcwCtl c = *st.ctl;
  if (c.k <= stop_k || a < 0 || (has_thr && !(v <= neg_thr))) { st.ctl->done = 1; return; }
  const int b = st.bp[a];
  if (merge_a) { merge_a[c.m] = a; merge_b[c.m] = b; merge_cost[c.m] = v; }
  c.nsa = st.sz[a] + st.sz[b];
  st.sz[a] = c.nsa; st.sz[b] = 0;
  st.parent[b] = a;
  c.a = a; c.b = b; c.m += 1; c.k -= 1; c.cnt = 0;
  *st.ctl = c;
}

// grid over x, one thread per slot: the sums of a take b's (row a and column a), and while x is in hand the cache logic: a row
// x < a whose cached partner was a or b, or a row a < x < b whose partner was b, goes on the rescan list (in any order: every
// row of it is rescanned on its own); any other row x < a takes the new v(x, a) if it beats its cache under (v, partner)
__global__ __launch_bounds__(AHCW_T) void ahcw_update_kernel(int n, AhcwState st) {
  if (st.ctl->done) return;
  const int x = blockIdx.x * AHCW_T + threadIdx.x;
  if (x >= n) return;
  const int a = st.ctl->a, b = st.ctl->b, nsa = st.ctl->nsa;
  const int sx = st.sz[x];
  if (sx <= 0 || x == a || x == b) return;
  const double s = st.sums[(long long)a * n + x] + st.sums[(long long)b * n + x];
  st.sums[(long long)a * n + x] = s;
  st.sums[(long long)x * n + a] = s;
  if (x < a) {
    const int p = st.bp[x];
    if (p == a || p == b) st.list[atomicAdd(&st.ctl->cnt, 1)] = x;      // (at most n - 2 appends: x != a, x != b)
    else {
      const double c = s / (double)(nsa * sx);
      const double o = st.bv[x];
      if (c < o || (c == o && a < p)) { st.bv[x] = c; st.bp[x] = a; }
    }
  } else if (x < b) {
    if (st.bp[x] == b) st.list[atomicAdd(&st.ctl->cnt, 1)] = x;
  }
}

// grid (P pieces, rows): the grid's rows stride over the list positions 0 .. cnt - 1 and, with_a, position cnt = row a.  A
// workgroup scans the live y > x of its piece [piece * L, (piece + 1) * L) of the row by (v, y).  P == 1: that is the row's
// result.  P > 1: it publishes its partial result and counts itself in; the workgroup that counts in last combines the P
// partial results in piece order (the pieces ascend in y: a tie keeps the smaller y) -- whoever that is, the result is the
// same, and nobody waits.
__global__ __launch_bounds__(AHCW_T) void ahcw_rescan_kernel(int n, AhcwState st, int P, int L, int with_a) {
  __shared__ double red_v[AHCW_T / 64];
  __shared__ int red_i[AHCW_T / 64];
  if (st.ctl->done) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, piece = blockIdx.x;
  const int nl = st.ctl->cnt, total = min(nl + (with_a ? 1 : 0), n + 1);
  for (int q = blockIdx.y; q < total; q += gridDim.y) {
    const int x = q < nl ? st.list[q] : st.ctl->a;
    const int sx = st.sz[x];
    const int y0 = max(piece * L, x + 1), y1 = min((piece + 1) * L, n);
    const double *__restrict__ row = st.sums + (long long)x * n;
    double v = 0.0;
    int p = -1;
#pragma unroll 4
    for (int y = y0 + tid; y < y1; y += AHCW_T) {
      const int sy = st.sz[y];
      const double s = row[y];
      if (sy > 0) {
        const double c = s / (double)(sx * sy);
        if (p < 0 || c < v) { v = c; p = y; }      // y ascends within a thread: a tie keeps the smaller y
      }
    }
    ahc_wave_min(v, p);
    if (lane == 0) { red_v[wave] = v; red_i[wave] = p; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < AHCW_T / 64; ++w) {
        const double ov = red_v[w];
        const int oi = red_i[w];
        if (oi >= 0 && (p < 0 || ov < v || (ov == v && oi < p))) { v = ov; p = oi; }
      }
      if (P == 1) { st.bv[x] = v; st.bp[x] = p; }
      else {
        const long long slot = (long long)q * P;
        __hip_atomic_store(&st.part_v[slot + piece], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&st.part_p[slot + piece], p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned before = __hip_atomic_fetch_add(&st.arrive[q], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (before == (unsigned)(P - 1)) {
          double c = 0.0;
          int bp = -1;
          for (int j = 0; j < P; ++j) {
            const double oc = __hip_atomic_load(&st.part_v[slot + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int op = __hip_atomic_load(&st.part_p[slot + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (op >= 0 && (bp < 0 || oc < c)) { c = oc; bp = op; }
          }
          st.bv[x] = c; st.bp[x] = bp;
          __hip_atomic_store(&st.arrive[q], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    __syncthreads();
  }
}

// one workgroup: every vector's final slot from the parents (parent[b] = a < b; a dead slot's chain ends at a live one) by
// pointer jumping in LDS, the live slots ranked in ascending order, the labels, the cluster count and the record's tail
__global__ __launch_bounds__(1024) void ahcw_label_kernel(int n, AhcwState st, const unsigned long long *__restrict__ bad,
                                                          int *__restrict__ labels, int *__restrict__ n_clusters,
                                                          int *__restrict__ merge_a, int *__restrict__ merge_b,
                                                          double *__restrict__ merge_cost) {
  extern __shared__ int ahcw_par[];
  __shared__ int part[1024];
  if (*bad) return;
  volatile int *par = ahcw_par;
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += 1024) par[i] = st.parent[i];
  __syncthreads();
  // in place: whatever a read meets, old or new, is an ancestor at least as far as the old one, so a chain halves per round
  for (int r = 0; r < AHCW_JUMP_ROUNDS; ++r) {
    for (int i = tid; i < n; i += 1024) par[i] = par[par[i]];
    __syncthreads();
  }
  const int per = (n + 1023) / 1024, s0 = min(tid * per, n), s1 = min(s0 + per, n);
  int c = 0;
  for (int s = s0; s < s1; ++s) c += par[s] == s ? 1 : 0;
  part[tid] = c;
  __syncthreads();
  int base = 0;
  for (int t = 0; t < tid; ++t) base += part[t];
  __syncthreads();
  for (int s = s0; s < s1; ++s)
    if (par[s] == s) { par[s] = -1 - base; ++base; }      // a live slot now holds its rank, encoded below zero
  __syncthreads();
  for (int i = tid; i < n; i += 1024) {
    const int p = par[i];
    labels[i] = p < 0 ? -1 - p : -1 - par[p];
  }
  const int m = st.ctl->m;
  if (merge_a)
    for (int q = m + tid; q < n - 1; q += 1024) { merge_a[q] = -1; merge_b[q] = -1; merge_cost[q] = INFINITY; }
  if (tid == 0) n_clusters[0] = st.ctl->k;
}

int ahcw_label_attr(plda_handle *h) {
  static DeviceOnce attr;
  if (attr.needed(h->device)) {
    PLDA_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&ahcw_label_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    AHCW_MAX * 4));
    attr.done(h->device);
  }
  return PLDA_OK;
}

// carves the state (the operand form: with its block array) and zeroes the counter of non-finite scores
int ahcw_prepare(plda_handle *h, int64_t N, bool with_block, AhcwState &st) {
  const int P = ahcw_pieces(h, N);
  PLDA_TRY(carve(h, h->ahc_scratch, [&](Layout &c) { st.lay(c, (size_t)N, (size_t)P, with_block); }));
  PLDA_HIP(h, h->ahc_stat.reserve(8));
  PLDA_HIP(h, hipMemsetAsync(h->ahc_stat.p, 0, 8, h->stream));
  return PLDA_OK;
}

// Enqueues the whole clustering of the block at dscores (row stride ld) on the state st; reads `done` between batches of
// steps when a threshold may stop the run early.  The caller finishes with cluster_counted.
int ahcw_enqueue(plda_handle *h, const float *dscores, int64_t N, int64_t ld, const AhcArgs &a, const AhcwState &st) {
  const int n = (int)N, P = ahcw_pieces(h, N), L = ahcw_piece_len(N, P), batch = ahcw_batch(h);
  const int stop_k = a.minc_wide > 1 ? a.minc_wide : 1;
  unsigned long long *dbad = h->ahc_stat.as<unsigned long long>();
  PLDA_TRY(ahcw_label_attr(h));
  TraceScope ts(h, "ahc.wide_load");
  {
    const int64_t pieces = std::max<int64_t>(1, std::min<int64_t>(ceil_div(N * N, (int64_t)256 * 16), 4096));
    ahcw_count_kernel<<<(unsigned)pieces, 256, 0, h->stream>>>(dscores, n, (long long)ld, dbad);
    PLDA_LAUNCH_CHECK(h);
    const unsigned nt = (unsigned)((n + 31) / 32);
    ahcw_load_kernel<<<dim3(nt, nt), dim3(32, 32), 0, h->stream>>>(dscores, n, (long long)ld, st.sums, dbad);
    PLDA_LAUNCH_CHECK(h);
    const unsigned gx = (unsigned)ceil_div((int64_t)n, (int64_t)AHCW_T);
    ahcw_init_kernel<<<gx, AHCW_T, 0, h->stream>>>(n, st, dbad);
    PLDA_LAUNCH_CHECK(h);
    ahcw_rescan_kernel<<<dim3((unsigned)P, (unsigned)std::min(n, 4096)), AHCW_T, 0, h->stream>>>(n, st, P, L, 0);
    PLDA_LAUNCH_CHECK(h);
  }
  ts.next("ahc.wide_merge");
  const unsigned gx = (unsigned)ceil_div((int64_t)n, (int64_t)AHCW_T);
  const dim3 gscan((unsigned)P, (unsigned)std::min(n, AHCW_SCAN_ROWS));
  int64_t left = N - stop_k;
  while (left > 0) {
    const int64_t c = a.has_thr ? std::min<int64_t>(batch, left) : left;
    for (int64_t s = 0; s < c; ++s) {
      ahcw_select_kernel<<<1, AHCW_T_SELECT, 0, h->stream>>>(n, st, stop_k, a.has_thr, -a.thr, a.merge_a, a.merge_b, a.merge_cost);
      ahcw_update_kernel<<<gx, AHCW_T, 0, h->stream>>>(n, st);
      ahcw_rescan_kernel<<<gscan, AHCW_T, 0, h->stream>>>(n, st, P, L, 1);
      PLDA_LAUNCH_CHECK(h);
    }
    left -= c;
    if (a.has_thr && left > 0) {
      int done = 0;
      PLDA_HIP(h, hipMemcpyAsync(&done, &st.ctl->done, 4, hipMemcpyDeviceToHost, h->stream));
      PLDA_HIP(h, hipStreamSynchronize(h->stream));
      if (done) break;
    }
  }
  ts.next("ahc.wide_label");
  ahcw_label_kernel<<<1, 1024, (size_t)n * 4, h->stream>>>(n, st, dbad, a.labels, a.n_clusters, a.merge_a, a.merge_b, a.merge_cost);
  PLDA_LAUNCH_CHECK(h);
  return PLDA_OK;
}

}  // namespace

int ahc_wide_plan(plda_handle *h, int64_t N, int64_t *out) {
  if (!out) return fail(h, PLDA_E_INVAL, "ahc_wide_plan: out is NULL");
  if (N < 1 || N > AHCW_MAX)
    return fail(h, PLDA_E_INVAL, "ahc_wide_plan: N = %lld (must be 1 ... PLDA_AHC_WIDE_MAX = %d)", (long long)N, AHCW_MAX);
  const int P = ahcw_pieces(h, N);
  AhcwState st;
  Layout size;
  st.lay(size, (size_t)N, (size_t)P, false);
  out[0] = (int64_t)size.end;
  out[1] = AHCW_LAUNCHES;
  out[2] = ahcw_batch(h);
  out[3] = P;
  return PLDA_OK;
}

int ahc_wide_validate(plda_handle *h, const char *fn, int64_t N, int64_t ld, const AhcArgs &a) {
  if (N < 1 || N > AHCW_MAX)
    return fail(h, PLDA_E_INVAL, "%s: N = %lld (must be 1 ... PLDA_AHC_WIDE_MAX = %d)", fn, (long long)N, AHCW_MAX);
  if (ld < N) return fail(h, PLDA_E_INVAL, "%s: ld = %lld (must be >= N = %lld)", fn, (long long)ld, (long long)N);
  PLDA_TRY(ahc_check_outputs(h, fn, a));
  if (a.minc_wide < 1) return fail(h, PLDA_E_INVAL, "%s: min_clusters = %d (must be >= 1)", fn, (int)a.minc_wide);
  return PLDA_OK;
}

int ahc_wide_matrix_device(plda_handle *h, const float *dscores, int64_t N, int64_t ld, const AhcArgs &a) {
  const char *fn = "ahc_wide_matrix";
  if (!dscores) return fail(h, PLDA_E_INVAL, "%s: scores is NULL", fn);
  PLDA_TRY(ahc_wide_validate(h, fn, N, ld, a));
  AhcwState st;
  PLDA_TRY(ahcw_prepare(h, N, false, st));
  return cluster_counted(h, fn, h->ahc_stat.p, ahcw_enqueue(h, dscores, N, ld, a, st));
}

int score_ahc_wide_device(plda_handle *h, const double *dX, int64_t N, const AhcArgs &a) {
  const char *fn = "score_ahc_wide";
  if (!can_score(h)) return fail(h, PLDA_E_NOT_FITTED, "%s: model not fitted", fn);
  if (!dX) return fail(h, PLDA_E_INVAL, "%s: X is NULL", fn);
  PLDA_TRY(ahc_wide_validate(h, fn, N, N, a));
  AhcwState st;
  PLDA_TRY(ahcw_prepare(h, N, true, st));
  h->prep_valid = false;           // (the block packs its own two sides)
  int rc;
  {
    TraceScope ts(h, "ahc.block_gemm", 2.0 * (double)h->Dout * (double)N * (double)N, 1);
    rc = score_matrix_device(h, dX, nullptr, 1, N, dX, N, nullptr, nullptr, st.block, N);
  }
  if (rc == PLDA_OK) rc = ahcw_enqueue(h, st.block, N, N, a, st);
  return cluster_counted(h, fn, h->ahc_stat.p, rc);
}

int ahc_validate(plda_handle *h, const char *fn, const int64_t *block_off, bool blocks, const int64_t *offsets, int64_t R,
                 const AhcArgs &a) {
  if (R < 1) return fail(h, PLDA_E_INVAL, "%s: R = %lld (must be >= 1)", fn, (long long)R);
  if (R > (int64_t)0x7fffffff) return fail(h, PLDA_E_INVAL, "%s: R = %lld (at most 2^31 - 1)", fn, (long long)R);
  if (!offsets) return fail(h, PLDA_E_INVAL, "%s: offsets is NULL", fn);
  PLDA_TRY(ahc_check_outputs(h, fn, a));
  PLDA_TRY(check_recordings(h, fn, offsets, R, AHC_MAX, "PLDA_AHC_MAX", [&](int64_t r, int64_t) {
    if (a.minc && a.minc[r] < 1)
      return fail(h, PLDA_E_INVAL, "%s: min_clusters[%lld] = %d (must be >= 1)", fn, (long long)r, (int)a.minc[r]);
    return (int)PLDA_OK;
  }));
  return blocks ? check_block_off(h, fn, block_off, offsets, R) : PLDA_OK;
}

int cluster_counted(plda_handle *h, const char *fn, const void *dbad, int rc) {
  unsigned long long bad = 0;
  hipError_t e = hipMemcpyAsync(&bad, dbad, 8, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (rc != PLDA_OK) return rc;
  PLDA_HIP(h, e);
  if (bad) return fail(h, PLDA_E_INVAL, "%s: %llu non-finite scores", fn, bad);
  return PLDA_OK;
}

int score_blocks_device(plda_handle *h, const char *span, const double *dX, const int64_t *offsets, int64_t r0, int64_t r1,
                        const int64_t *boff, float *slab) {
  const int D = h->Dout;
  TraceScope ts(h, span, 0.0, 1);
  double flop = 0.0;
  int rc = PLDA_OK;
  for (int64_t r = r0; r < r1 && rc == PLDA_OK; ++r) {
    const int64_t n = offsets[r + 1] - offsets[r];
    const double *x = dX + offsets[r] * D;
    rc = score_matrix_device(h, x, nullptr, 1, n, x, n, nullptr, nullptr, slab + boff[r - r0], n);
    flop += 2.0 * (double)D * (double)n * (double)n;
  }
  if (ts.idx >= 0) h->trace_spans[ts.idx].work = flop;
  return rc;
}

int ahc_plan(plda_handle *h, int64_t N, int32_t *out) {
  if (!out) return fail(h, PLDA_E_INVAL, "ahc_plan: out is NULL");
  if (N < 1 || N > AHC_MAX) return fail(h, PLDA_E_INVAL, "ahc_plan: N = %lld (must be 1 ... PLDA_AHC_MAX = %d)", (long long)N, AHC_MAX);
  const bool hbm = N > AHC_LDS_MAX;
  out[0] = hbm ? 1 : 0;
  out[1] = hbm ? (int32_t)(N * N * 8) : 0;
  out[2] = AHC_LDS_MAX;
  return PLDA_OK;
}

int ahc_matrix_device(plda_handle *h, const float *dscores, const int64_t *block_off, const int64_t *offsets, int64_t R,
                      const AhcArgs &a) {
  const char *fn = "ahc_matrix";
  if (!dscores) return fail(h, PLDA_E_INVAL, "%s: scores is NULL", fn);
  PLDA_TRY(ahc_validate(h, fn, block_off, true, offsets, R, a));
  PLDA_HIP(h, h->ahc_stat.reserve(8));
  PLDA_HIP(h, hipMemsetAsync(h->ahc_stat.p, 0, 8, h->stream));
  std::vector<std::vector<AhcRec>> tables;
  const int rc = ahc_enqueue(h, dscores, block_off, offsets, 0, R, a, tables);
  return cluster_counted(h, fn, h->ahc_stat.p, rc);
}

int score_ahc_device(plda_handle *h, const double *dX, const int64_t *offsets, int64_t R, const AhcArgs &a) {
  const char *fn = "score_ahc";
  if (!can_score(h)) return fail(h, PLDA_E_NOT_FITTED, "%s: model not fitted", fn);
  if (!dX) return fail(h, PLDA_E_INVAL, "%s: X is NULL", fn);
  PLDA_TRY(ahc_validate(h, fn, nullptr, false, offsets, R, a));
  SlabWalk walk(offsets, R, cluster_budget(h) / 4);
  PLDA_HIP(h, h->sn_slab.reserve((size_t)walk.largest * 4));
  float *slab = h->sn_slab.as<float>();
  h->prep_valid = false;           // (every block packs its own two sides)
  PLDA_HIP(h, h->ahc_stat.reserve(8));
  PLDA_HIP(h, hipMemsetAsync(h->ahc_stat.p, 0, 8, h->stream));
  std::vector<std::vector<AhcRec>> tables;
  int rc = PLDA_OK;
  while (rc == PLDA_OK && walk.next()) {      // every slab scored, counted and clustered in one pass
    rc = score_blocks_device(h, "ahc.block_gemm", dX, offsets, walk.r0, walk.r1, walk.boff.data(), slab);
    if (rc == PLDA_OK) rc = ahc_enqueue(h, slab, walk.boff.data(), offsets, walk.r0, walk.r1, a, tables);
  }
  return cluster_counted(h, fn, h->ahc_stat.p, rc);
}

}  // namespace plda
