// plda_amd/csrc/der.hip -- diarisation error rate: per-recording miss / false alarm / speaker confusion under the OPTIMAL
// one-to-one mapping of reference to hypothesis speakers, and the sweep of a full AHC merge record over Q thresholds
// (the contract is in include/plda_hip.h, the host model in tests/der_model.py).
//
// A recording is a small dependent problem: a confusion matrix of at most 64 x 4096 integers and a shortest-augmenting-path
// assignment on it (Hungarian / Jonker-Volgenant with int64 potentials), at most Sr (Sr + 1) / 2 steps, each a scan of the
// hypothesis speakers.  There are thousands of independent recordings and a sweep multiplies them by Q: one workgroup per
// (recording, threshold).  Everything is an integer; the counts are determined by the input alone.
//
//   der_count_kernel    one workgroup per recording: the entries that break the contract (a label below -1 or above its
//                       limit, a negative duration) added to one counter; Sr and Sh, the distinct labels of either side
//   der_prefix_kernel   sweep, grid (recordings, thresholds): the number of merges the stop rule of the AHC lets through
//                       (Sh = N - that); a record that ends first, or an entry that is no merge, is counted as a bad record
//   der_solve_kernel    <HBM, SWEEP, ATOMS, OVL, JER>, the one __global__ around der_solve_body; all 20 instantiations share one
//                       signature (a form reads only its own arguments) and are launched through der_solve_fn's pointer.
//                       <HBM = false> the Sr x W int64 confusion matrix in LDS (W = max(Sr, Sh): zero columns pad a
//                       hypothesis with fewer speakers than the reference);  <HBM = true> the matrix in handle scratch.
//                       Both keep the column state (potential, slack, predecessor, owner, flag, label) in LDS.
//                       <SWEEP> the hypothesis labels are the slots of the replayed merge prefix.
//                       <ATOMS> the reference side is the scored atoms that der_time.hip cuts from reference turns,
//                       hypothesis segments, collar and UEM (K20): an atom of `ticks` ticks adds them to C[i][j] for every
//                       reference speaker i of its 64-bit mask
//                       <OVL> (with ATOMS, without SWEEP) up to two hypothesis labels per segment (K21, plda_der_timed_ovl):
//                       the labels present range over hyp and hyp2, an atom adds its ticks to C[i][j] for both labels of
//                       its segment, and nhyp in the four counters is the number of labels >= 0
//                       <JER> the JER form of all five shapes (K22): the same fill, with the per-speaker tick sums rt and ht
//                       beside it; the same first assignment and outputs; then the Jaccard weights in place above C and a
//                       second assignment on them (the comment at der_solve_body says where w is computed and why); jer,
//                       jmap and spk come from the second
//
// Resources on gfx950 (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage), LDS / scratch class; no kernel
// of this file has scratch memory or spills, and der_solve_kernel has no static LDS:
//   der_count_kernel 12 VGPRs (<false> and <true>);  der_prefix_kernel 14
//   der_solve_kernel <SWEEP, ATOMS, OVL>     plain: VGPRs   SGPRs     waves/SIMD     JER: VGPRs   SGPRs     waves/SIMD
//     segments            <0, 0, 0>                 44 / 40   48 / 54   8 / 8             82 / 82   83 / 91   5 / 5
//     atoms               <0, 1, 0>                 44 / 40   52 / 60   8 / 8             82 / 82   83 / 91   5 / 5
//     atoms, two labels   <0, 1, 1>                 44 / 40   58 / 65   8 / 8             82 / 82   83 / 91   5 / 5
//     sweep of segments   <1, 0, 0>                 44 / 40   52 / 55   8 / 8             76 / 84   82 / 90   6 / 5
//     sweep of atoms      <1, 1, 0>                 44 / 40   59 / 62   8 / 8             76 / 84   82 / 90   6 / 5
// (the figures of the four kernels with four signatures that this one replaced; the plain two-label shape alone moved, by two
// SGPRs, from 56 / 63)
// With JER = false der_solve_body compiles to what it was before the JER form existed: six of the ten plain instantiations are
// the same instructions in the same order, the other four (segment and two-label form, both classes) differ in the order of
// two independent register clears.
//
// One workgroup of der_solve_kernel: (1) the labels present, as bit sets (64 bits of reference, 4096 of hypothesis), give
// the compact numbering by prefix population counts; (2) the matrix is zeroed and filled with integer atomics, the four
// counters are summed in registers; (3) rows are inserted one by one: each step scans the free columns for the reduced
// cost against the row just reached, keeps the per-column minimum and its predecessor, and takes the workgroup minimum by
// (value, column) -- ties to the smaller column, so the path taken, and with it the map, depends on the matrix alone;
// (4) the potentials move by that minimum, the path is flipped when a free column is reached.
#include "common.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace plda {

namespace {

constexpr int DER_MAX_REF = PLDA_DER_MAX_REF;
constexpr int DER_MAX_HYP = PLDA_AHC_MAX;
constexpr int DER_LDS_BYTES = 160 * 1024;     // one workgroup may hold all of a CU's LDS
constexpr int DER_T = 256;
constexpr int DER_W = DER_T / 64;
constexpr int DER_COL_BYTES = 8 + 8 + 4 * 4;   // v, minv | way, own, used, clab
// red_v[4] cnt[4][4] refmask u[65] hbits[64] | hbase[64] reflab[64] red_i[4]
constexpr int DER_FIXED_BYTES = 8 * (DER_W + 4 * DER_W + 1 + (DER_MAX_REF + 1) + 64) + 4 * (64 + DER_MAX_REF + DER_W);
constexpr long long DER_INF = 1ll << 62;

// one (recording, threshold) of a launch (host-built, uploaded once per call)
struct DerRec {
  long long off;     // first segment
  long long scr;     // HBM class: first int64 of the Sr x W matrix in scratch
  long long out;     // row of counts (and of n_clusters / map)
  int n, sr, sh, w;  // segments; distinct reference / hypothesis labels; max(sr, sh)
  int m, r;          // sweep: merges to replay; the recording (its merge entries start at off - r)
};

constexpr long long der_lds_bytes(long long sr, long long w, long long n_replay, bool hbm) {
  return (hbm ? 0 : 8 * sr * w) + (long long)DER_COL_BYTES * (w + 1) + 4 * n_replay + DER_FIXED_BYTES;
}
static_assert(der_lds_bytes(DER_MAX_REF, DER_MAX_HYP, DER_MAX_HYP, true) <= DER_LDS_BYTES,
              "the scratch class's column state and the replay must fit one CU's LDS");

// The JER form (K22) adds rt[64] (int64) and, outside the sweep, ht[w + 1] (int32).  In the sweep ht takes clab's place: a
// sweep writes no map, so the caller's label of a column is never read.  The second assignment reuses the column state.
constexpr int DER_JER_FIXED_BYTES = 8 * DER_MAX_REF;
constexpr long long der_jer_lds_bytes(long long sr, long long w, long long n_replay, bool hbm, bool sweep) {
  return der_lds_bytes(sr, w, n_replay, hbm) + DER_JER_FIXED_BYTES + (sweep ? 0 : 4 * (w + 1));
}
static_assert(der_jer_lds_bytes(DER_MAX_REF, DER_MAX_HYP, 0, true, false) <= DER_LDS_BYTES &&
              der_jer_lds_bytes(DER_MAX_REF, DER_MAX_HYP, DER_MAX_HYP, true, true) <= DER_LDS_BYTES,
              "the JER form's scratch class must fit one CU's LDS");
// a matrix entry of the JER form once the first assignment is done: w << 31 | C (C <= 2^30, w <= 2^32)
constexpr int DER_JER_SHIFT = 31;
constexpr long long DER_JER_MAX_TICKS = 1ll << 30;

__device__ __forceinline__ long long der_wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// lexicographic minimum of (v, j) over the wave, j < 0 = nothing; every lane ends with the result
__device__ __forceinline__ void der_wave_min(long long &v, int &j) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const long long ov = __shfl_xor(v, o);
    const int oj = __shfl_xor(j, o);
    if (oj >= 0 && (j < 0 || ov < v || (ov == v && oj < j))) { v = ov; j = oj; }
  }
}

__device__ __forceinline__ unsigned long long der_below(int bit) { return bit ? ~0ull >> (64 - bit) : 0ull; }

// one workgroup per recording: stat[0] += the invalid entries; sr[r], sh[r] = the distinct labels (hyp nullable: the sweep)
// <JER>: a recording whose durations add up to more than 2^30 ticks counts as one more invalid entry
template <bool JER = false>
__global__ __launch_bounds__(DER_T) void der_count_kernel(const int *__restrict__ ref, const int *__restrict__ hyp,
                                                          const int *__restrict__ dur, const long long *__restrict__ offsets,
                                                          unsigned long long *stat, int *__restrict__ sr, int *__restrict__ sh) {
  __shared__ unsigned long long bits[JER ? 66 : 65];      // <JER>: bits[65] = the sum of the recording's durations
  __shared__ int tot[2];
  const int tid = threadIdx.x, r = blockIdx.x;
  const long long off = offsets[r];
  const int n = (int)(offsets[r + 1] - off);
  if (tid < (JER ? 66 : 65)) bits[tid] = 0;
  if (tid < 2) tot[tid] = 0;
  __syncthreads();
  unsigned bad = 0;
  for (int t = tid; t < n; t += DER_T) {
    const int a = ref[off + t], b = hyp ? hyp[off + t] : -1, d = dur ? dur[off + t] : 1;
    bool ok = d >= 0;
    if (a < -1 || a >= DER_MAX_REF) ok = false;
    else if (a >= 0) atomicOr(&bits[64], 1ull << a);
    if (b < -1 || b >= DER_MAX_HYP) ok = false;
    else if (b >= 0) atomicOr(&bits[b >> 6], 1ull << (b & 63));
    if (!ok) ++bad;
  }
  if (bad) atomicAdd(stat, (unsigned long long)bad);      // rare: one integer atomic per lane that met one
  if constexpr (JER) {
    long long ticks = 0;
    for (int t = tid; t < n; t += DER_T) {
      const int d = dur ? dur[off + t] : 1;
      if (d > 0) ticks += d;
    }
    ticks = der_wave_sum(ticks);
    if ((tid & 63) == 0) atomicAdd(&bits[65], (unsigned long long)ticks);
  }
  __syncthreads();
  if constexpr (JER) {
    if (tid == 0 && bits[65] > (unsigned long long)DER_JER_MAX_TICKS) atomicAdd(stat, 1ull);
  }
  if (tid < 64) { const int c = __popcll(bits[tid]); if (c) atomicAdd(&tot[1], c); }
  if (tid == 64) tot[0] = __popcll(bits[64]);
  __syncthreads();
  if (tid == 0) { sr[r] = tot[0]; if (sh) sh[r] = tot[1]; }
}

// grid (recordings, thresholds): m[q * R + r] = the merges of recording r that the stop rule lets through at threshold q
// (diarize.cut's loop: k > max(1, minc), then a missing entry is an error, then !(cost <= -threshold) stops); stat[1] += 1 for
// a record that ends before the rule fires or whose prefix holds an entry that is no merge (not 0 <= a < b < N)
__global__ __launch_bounds__(DER_T) void der_prefix_kernel(const int *__restrict__ ma, const int *__restrict__ mb,
                                                           const double *__restrict__ mc, const long long *__restrict__ offsets,
                                                           const double *__restrict__ thr, const int *__restrict__ minc, int R,
                                                           unsigned long long *stat, int *__restrict__ mout) {
  __shared__ int first[2];     // the first entry that fails the threshold; the first that is no merge
  const int tid = threadIdx.x, r = blockIdx.x, q = blockIdx.y;
  const long long off = offsets[r], base = off - r;
  const int n = (int)(offsets[r + 1] - off);
  const int stop_k = minc && minc[r] > 1 ? minc[r] : 1;
  const int limit = n > stop_k ? n - stop_k : 0;
  const double neg_thr = -thr[q];
  if (tid < 2) first[tid] = limit;
  __syncthreads();
  int f_thr = limit, f_bad = limit;
  for (int e = tid; e < limit && e < f_thr && e < f_bad; e += DER_T) {
    const int a = ma[base + e], b = mb[base + e];
    if (!(a >= 0 && a < b && b < n)) f_bad = e;
    else if (!(mc[base + e] <= neg_thr)) f_thr = e;
  }
  if (f_thr < limit) atomicMin(&first[0], f_thr);
  if (f_bad < limit) atomicMin(&first[1], f_bad);
  __syncthreads();
  if (tid == 0) {
    const bool bad = first[1] < first[0];
    if (bad) atomicAdd(stat + 1, 1ull);
    mout[(long long)q * R + r] = bad ? 0 : first[0];
  }
}

// the weight the assignment reads from a matrix entry: C, or in the JER form's second pass the w above C
template <bool JER> __device__ __forceinline__ long long der_weight(long long e, int pass) {
  if constexpr (JER) return pass ? (long long)((unsigned long long)e >> DER_JER_SHIFT) : e;
  else return e;
}

// the confusion matrix of a recording: in LDS, or in HBM scratch (filled with atomics that complete in L2: read back with
// device-scope loads, which do not take a line the CU's vector cache may hold from before)
template <bool HBM> struct DerMat;
template <> struct DerMat<false> {
  long long *c; int w;
  __device__ __forceinline__ long long get(int i, int j) const { return c[i * w + j]; }
  __device__ __forceinline__ void put(int i, int j, long long x) const { c[i * w + j] = x; }
};
template <> struct DerMat<true> {
  long long *c; int w;
  __device__ __forceinline__ long long get(int i, int j) const {
    return __hip_atomic_load(c + (long long)i * w + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void put(int i, int j, long long x) const {
    __hip_atomic_store(c + (long long)i * w + j, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// One workgroup's solve.  ATOMS = false: the segment form (ref, hyp, dur per segment).  ATOMS = true: the time-based form
// (der_time.hip): the reference side is the scored atoms of the recording (ticks, 64-bit reference mask, segment index or -1)
// and the union of their masks; the hypothesis label of an atom is that of its segment (SWEEP: the slot of its segment).
// OVL (with ATOMS, without SWEEP; K21): a segment carries the label set {hyp[t]} u {td.hyp2[t]}, -1 = no such label.
//
// JER (K22; include/plda_hip.h, "Jaccard error rate"): the fill also sums rt[i], the scored ticks of reference speaker i, and
// ht[j], those of hypothesis speaker j (integer LDS atomics).  The first assignment and its outputs are those of the plain
// form.  Then every entry C of the matrix becomes w << 31 | C in place, w = floor(C 2^32 / (rt[i] + ht[j] - C)): ONE 64-bit
// division per entry (C 2^32 <= 2^62, so nothing wider), where a weight computed in the scan would cost one per column per
// step (up to Sr (Sr + 1) / 2 steps) and a second matrix beside C would halve the LDS class.  C <= 2^30 and w <= 2^32 share
// the word.  The second assignment runs the same loop on w from fresh potentials and a fresh column state, under the same
// (value, column) tie rule; jer, jmap and spk are read from it.
template <bool HBM, bool SWEEP, bool ATOMS, bool OVL = false, bool JER = false>
__device__ __forceinline__ void der_solve_body(const int *__restrict__ ref, const int *__restrict__ hyp,
                                               const int *__restrict__ dur, const int *__restrict__ ma,
                                               const int *__restrict__ mb, const DerRec *__restrict__ tab,
                                               long long *scratch, long long *__restrict__ counts,
                                               int *__restrict__ n_clusters, int *__restrict__ map, const DerTimedDev &td,
                                               const DerJerOut &jo = DerJerOut{}) {
  extern __shared__ long long der_smem[];
  const DerRec rc = tab[blockIdx.x];
  const int n = rc.n, w = rc.w, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // LDS: [matrix (LDS class)] | v[w+1] minv[w+1] u[65] red_v[4] cnt[16] refmask hbits[64] | way[w+1] own[w+1] used[w+1] clab[w+1]
  //      hbase[64] reflab[64] red_i[4] | parent[n] (sweep)
  // JER: rt[64] behind hbits, ht[w+1] behind red_i (in the sweep ht IS clab: der_jer_lds_bytes)
  long long *p8 = der_smem;
  DerMat<HBM> mat;
  mat.w = w;
  if constexpr (HBM) mat.c = scratch + rc.scr;
  else { mat.c = p8; p8 += (long long)rc.sr * w; }
  long long *v = p8; p8 += w + 1;
  long long *minv = p8; p8 += w + 1;
  long long *u = p8; p8 += DER_MAX_REF + 1;
  long long *red_v = p8; p8 += DER_W;
  long long *cnt = p8; p8 += 4 * DER_W;
  unsigned long long *refmask = reinterpret_cast<unsigned long long *>(p8); p8 += 1;
  unsigned long long *hbits = reinterpret_cast<unsigned long long *>(p8); p8 += 64;
  unsigned long long *rt = reinterpret_cast<unsigned long long *>(p8);      // JER: the scored ticks of compact row i
  if constexpr (JER) p8 += DER_MAX_REF;
  int *p4 = reinterpret_cast<int *>(p8);
  int *way = p4; p4 += w + 1;
  int *own = p4; p4 += w + 1;      // the row (1-based) that holds column j, 0 = free
  int *used = p4; p4 += w + 1;
  int *clab = p4; p4 += w + 1;     // the caller's label of compact column j (0-based)
  int *hbase = p4; p4 += 64;
  int *reflab = p4; p4 += DER_MAX_REF;
  int *red_i = p4; p4 += DER_W;
  int *ht = clab;                  // JER: the scored ticks of compact column j (0-based); the sweep has no use for clab
  if constexpr (JER && !SWEEP) { ht = p4; p4 += w + 1; }
  int *parent = p4;

  const int *__restrict__ rf = ATOMS ? nullptr : ref + rc.off;
  const int *__restrict__ dr = !ATOMS && dur ? dur + rc.off : nullptr;
  const DerTimedRec tr = ATOMS ? td.recs[rc.r] : DerTimedRec{};

  // (1a) sweep: the slots of the replayed prefix.  parent[b] = a < b for every merge; pointer jumping to the roots -- a read
  // that races with a write sees an ancestor either way, and every round at least doubles the distance covered
  if constexpr (SWEEP) {
    const long long mbase = rc.off - rc.r;
    for (int x = tid; x < n; x += DER_T) parent[x] = x;
    __syncthreads();
    for (int e = tid; e < rc.m; e += DER_T) parent[mb[mbase + e]] = ma[mbase + e];
    __syncthreads();
    for (int round = 0; round < 12; ++round) {
      for (int x = tid; x < n; x += DER_T) {
        const int p = parent[x], g = parent[p];
        if (g != p) parent[x] = g;
      }
      __syncthreads();
    }
  }
  auto hyp_of = [&](int t) -> int {
    if constexpr (SWEEP) return parent[t];
    else return hyp[rc.off + t];
  };
  static_assert(!OVL || (ATOMS && !SWEEP), "the second label belongs to the time-based form against hyp");

  // (1b) the labels present
  if (tid < 64) hbits[tid] = 0;
  if (tid == 64) *refmask = 0;
  __syncthreads();
  {
    unsigned long long rm = 0;
    if constexpr (ATOMS) {
      for (int t = tid; t < n; t += DER_T) {
        const int b = hyp_of(t);
        if (b >= 0) atomicOr(&hbits[(b >> 6) & 63], 1ull << (b & 63));
        if constexpr (OVL) {
          const int b2 = td.hyp2[rc.off + t];
          if (b2 >= 0) atomicOr(&hbits[(b2 >> 6) & 63], 1ull << (b2 & 63));
        }
      }
      if (tid == 0) rm = tr.umask;
    } else {
      for (int t = tid; t < n; t += DER_T) {
        const int a = rf[t], b = hyp_of(t);
        if (a >= 0) rm |= 1ull << (a & 63);
        if (b >= 0) atomicOr(&hbits[(b >> 6) & 63], 1ull << (b & 63));
      }
    }
    if (rm) atomicOr(refmask, rm);
  }
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int k = 0; k < 64; ++k) { hbase[k] = s; s += __popcll(hbits[k]); }
    int i = 0;
    for (unsigned long long mk = *refmask; mk; mk &= mk - 1) reflab[i++] = __ffsll((long long)mk) - 1;
  }
  __syncthreads();
  const unsigned long long rmask = *refmask;
  const int sr = __popcll(rmask), sh = hbase[63] + __popcll(hbits[63]);
  // (the table was sized from der_count_kernel's reading of the same arrays; input that changed under the call must not
  // carry an index out of the layout)
  if (sr != rc.sr || sh != rc.sh) return;
  if constexpr (!(JER && SWEEP)) {
    if (tid < 64) {
      int j = hbase[tid];
      for (unsigned long long mk = hbits[tid]; mk; mk &= mk - 1) clab[j++] = tid * 64 + __ffsll((long long)mk) - 1;
    }
  }
  // (2) the matrix and the column state
  for (long long e = tid; e < (long long)sr * w; e += DER_T) mat.c[e] = 0;
  for (int j = tid; j <= w; j += DER_T) { v[j] = 0; own[j] = 0; }
  if (tid <= DER_MAX_REF) u[tid] = 0;
  if constexpr (JER) {
    for (int j = tid; j <= w; j += DER_T) ht[j] = 0;
    if (tid < DER_MAX_REF) rt[tid] = 0;
  }
  __syncthreads();
  long long c_speech = 0, c_miss = 0, c_fa = 0, c_both = 0;
  if constexpr (ATOMS) {
    // an atom of `ticks` ticks with nref = popcount(mask) reference speakers and nhyp = 0 or 1 (OVL: or 2) hypothesis speakers
    auto fill = [&](int b, unsigned long long am, long long d) {
      if (b >= 0 && b < DER_MAX_HYP && d) {
        const int k = b >> 6, j = hbase[k] + __popcll(hbits[k] & der_below(b & 63));
        if constexpr (JER) atomicAdd(&ht[j], (int)d);      // (also where the atom holds no reference speaker)
        for (unsigned long long mk = am; mk; mk &= mk - 1) {
          const int i = __popcll(rmask & der_below(__ffsll((long long)mk) - 1));
          atomicAdd(reinterpret_cast<unsigned long long *>(mat.c) + (long long)i * w + j, (unsigned long long)d);
        }
      }
    };
    for (int e = tid; e < tr.natoms; e += DER_T) {
      const long long d = td.ticks[tr.aoff + e];
      const unsigned long long am = td.mask[tr.aoff + e] & rmask;
      const int sg = td.seg[tr.aoff + e], b = sg >= 0 && sg < n ? hyp_of(sg) : -1;
      int b2 = -1;
      if constexpr (OVL) b2 = sg >= 0 && sg < n ? td.hyp2[rc.off + sg] : -1;
      const int nref = __popcll(am), nhyp = (b >= 0 ? 1 : 0) + (b2 >= 0 ? 1 : 0);
      c_speech += d * nref;
      c_miss += d * (nref > nhyp ? nref - nhyp : 0);
      c_fa += d * (nhyp > nref ? nhyp - nref : 0);
      c_both += d * (nref < nhyp ? nref : nhyp);
      fill(b, am, d);
      if constexpr (OVL) fill(b2, am, d);
      if constexpr (JER) {
        if (d)
          for (unsigned long long mk = am; mk; mk &= mk - 1)
            atomicAdd(&rt[__popcll(rmask & der_below(__ffsll((long long)mk) - 1))], (unsigned long long)d);
      }
    }
  } else
  for (int t = tid; t < n; t += DER_T) {
    const int a = rf[t], b = hyp_of(t);
    const long long d = dr ? dr[t] : 1;
    if constexpr (JER) {
      if (d > 0) {
        if (a >= 0) atomicAdd(&rt[__popcll(rmask & der_below(a & 63))], (unsigned long long)d);
        if (b >= 0 && b < DER_MAX_HYP) atomicAdd(&ht[hbase[b >> 6] + __popcll(hbits[b >> 6] & der_below(b & 63))], (int)d);
      }
    }
    if (a >= 0) {
      c_speech += d;
      if (b < 0) c_miss += d;
      else {
        c_both += d;
        const int i = __popcll(rmask & der_below(a)), k = b >> 6;
        const int j = hbase[k] + __popcll(hbits[k] & der_below(b & 63));
        if (d) atomicAdd(reinterpret_cast<unsigned long long *>(mat.c) + (long long)i * w + j, (unsigned long long)d);
      }
    } else if (b >= 0) c_fa += d;
  }
  c_speech = der_wave_sum(c_speech); c_miss = der_wave_sum(c_miss); c_fa = der_wave_sum(c_fa); c_both = der_wave_sum(c_both);
  if (lane == 0) { cnt[wave * 4 + 0] = c_speech; cnt[wave * 4 + 1] = c_miss; cnt[wave * 4 + 2] = c_fa; cnt[wave * 4 + 3] = c_both; }
  __syncthreads();

  // (3, 4) the assignment: minimise sum of -C over the rows; thread tid owns the columns j = tid (mod DER_T), column 0 is the
  // virtual column the new row hangs from
  // JER: a second pass of the same loop on the weights w, behind the outputs of the first.  (Two jumps, not a loop or a
  // callable around the text below: either changes the code the plain instantiations compile to; like this they keep it.)
  int pass = 0;
der_assign:
  if constexpr (JER) {
    if (pass == 1) {
      __syncthreads();                             // (the first assignment's own[] and red_v[] have been read)
      // (5) every entry becomes w << 31 | C; the padding columns (C = 0, weight 0) stay 0.  U = 0 needs rt[i] = 0, then C = 0
      for (int i = 0; i < sr; ++i) {
        const unsigned long long rti = rt[i];
        for (int j = tid; j < sh; j += DER_T) {
          const unsigned long long c = (unsigned long long)mat.get(i, j), un = rti + (unsigned)ht[j] - c;
          if (c) mat.put(i, j, (long long)((((c << 32) / un) << DER_JER_SHIFT) | c));
        }
      }
      for (int j = tid; j <= w; j += DER_T) { v[j] = 0; own[j] = 0; }
      if (tid <= DER_MAX_REF) u[tid] = 0;
      if constexpr (HBM) __threadfence();
      __syncthreads();
    }
  }
  for (int i = 1; i <= sr; ++i) {
    for (int j = tid; j <= w; j += DER_T) { minv[j] = DER_INF; used[j] = 0; }
    if (tid == 0) own[0] = i;
    __syncthreads();
    int j0 = 0;
    while (true) {
      if ((j0 & (DER_T - 1)) == tid) used[j0] = 1;
      const int i0 = own[j0];
      const long long ui0 = u[i0];
      long long best = 0;
      int bj = -1;
      for (int j = tid ? tid : DER_T; j <= w; j += DER_T) {
        if (used[j]) continue;
        const long long cur = (j <= sh ? -der_weight<JER>(mat.get(i0 - 1, j - 1), pass) : 0) - ui0 - v[j];
        long long mj = minv[j];
        if (cur < mj) { mj = cur; minv[j] = cur; way[j] = j0; }
        if (bj < 0 || mj < best) { best = mj; bj = j; }      // j ascends within a thread: a tie keeps the smaller column
      }
      der_wave_min(best, bj);
      if (lane == 0) { red_v[wave] = best; red_i[wave] = bj; }
      __syncthreads();
      best = red_v[0]; bj = red_i[0];
#pragma unroll
      for (int k = 1; k < DER_W; ++k) {
        const long long ov = red_v[k];
        const int oj = red_i[k];
        if (oj >= 0 && (bj < 0 || ov < best || (ov == best && oj < bj))) { best = ov; bj = oj; }
      }
      if (bj < 0) break;                           // (cannot happen: w >= sr leaves a free column; keeps every index in range)
      const bool reached = own[bj] == 0;           // (read before the barrier below: behind it thread 0 flips the path)
      for (int j = tid; j <= w; j += DER_T) {
        if (used[j]) { u[own[j]] += best; v[j] -= best; }     // (the owners of used columns are distinct rows)
        else minv[j] -= best;
      }
      __syncthreads();
      j0 = bj;
      if (reached) break;
    }
    if (tid == 0)
      while (j0) { const int j1 = way[j0]; own[j0] = own[j1]; j0 = j1; }
    __syncthreads();
  }

  // the weight of the optimum, the counts, the map
  if constexpr (JER) {
    if (pass == 1) goto der_jer_out;
  }
  {
  long long correct = 0;
  for (int j = tid ? tid : DER_T; j <= sh; j += DER_T)
    if (own[j]) correct += mat.get(own[j] - 1, j - 1);
  correct = der_wave_sum(correct);
  if (lane == 0) red_v[wave] = correct;
  if (map)
    for (int k = tid; k < DER_MAX_REF; k += DER_T) map[rc.out * DER_MAX_REF + k] = -1;
  __syncthreads();
  if (tid == 0) {
    long long s[4] = {0, 0, 0, 0}, cor = 0;
    for (int k = 0; k < DER_W; ++k) {
      cor += red_v[k];
      for (int c = 0; c < 4; ++c) s[c] += cnt[k * 4 + c];
    }
    counts[rc.out * 4 + 0] = s[0]; counts[rc.out * 4 + 1] = s[1]; counts[rc.out * 4 + 2] = s[2]; counts[rc.out * 4 + 3] = s[3] - cor;
    if (n_clusters) n_clusters[rc.out] = sh;
  }
  if (map)
    for (int j = tid ? tid : DER_T; j <= sh; j += DER_T)
      if (own[j] && mat.get(own[j] - 1, j - 1) > 0) map[rc.out * DER_MAX_REF + reflab[own[j] - 1]] = clab[j - 1];
  }

  if constexpr (JER) {
    pass = 1;
    goto der_assign;
  }
der_jer_out:
  if constexpr (JER) {
    constexpr long long CMASK = (1ll << DER_JER_SHIFT) - 1;
    // (7) jer = {n_ref, jsum}; jmap and spk by the rules of map
    long long jsum = 0;
    for (int j = tid ? tid : DER_T; j <= sh; j += DER_T)
      if (own[j]) jsum += (long long)((unsigned long long)mat.get(own[j] - 1, j - 1) >> DER_JER_SHIFT);
    jsum = der_wave_sum(jsum);
    if (lane == 0) red_v[wave] = jsum;
    if (jo.jmap)
      for (int k = tid; k < DER_MAX_REF; k += DER_T) jo.jmap[rc.out * DER_MAX_REF + k] = -1;
    if (jo.spk)
      for (int k = tid; k < DER_MAX_REF; k += DER_T) {
        const long long r0 = (rmask >> k) & 1 ? (long long)rt[__popcll(rmask & der_below(k))] : 0;
        long long *sp = jo.spk + (rc.out * DER_MAX_REF + k) * 3;
        sp[0] = r0; sp[1] = 0; sp[2] = r0;
      }
    __syncthreads();
    if (tid == 0) {
      long long js = 0, nref = 0;
      for (int k = 0; k < DER_W; ++k) js += red_v[k];
      for (int i = 0; i < sr; ++i) nref += rt[i] > 0;
      jo.jer[rc.out * 2 + 0] = nref; jo.jer[rc.out * 2 + 1] = js;
    }
    for (int j = tid ? tid : DER_T; j <= sh; j += DER_T) {
      if (!own[j]) continue;
      const int i = own[j] - 1;
      const long long c = mat.get(i, j - 1) & CMASK;
      if (c <= 0) continue;
      if constexpr (!SWEEP) {
        if (jo.jmap) jo.jmap[rc.out * DER_MAX_REF + reflab[i]] = clab[j - 1];
      }
      if (jo.spk) {
        long long *sp = jo.spk + (rc.out * DER_MAX_REF + reflab[i]) * 3;
        sp[1] = c; sp[2] = (long long)rt[i] + ht[j - 1] - c;
      }
    }
  }
}

// Every form is this one kernel, the form in its template arguments (ref and dur are unused with ATOMS, td without it, ma and
// mb without SWEEP, jo without JER: the body reads none of them then).  Resources: the table in the file header.
template <bool HBM, bool SWEEP, bool ATOMS, bool OVL, bool JER>
__global__ __launch_bounds__(DER_T) void der_solve_kernel(const int *__restrict__ ref, const int *__restrict__ hyp,
                                                          const int *__restrict__ dur, const int *__restrict__ ma,
                                                          const int *__restrict__ mb, const DerRec *__restrict__ tab,
                                                          long long *scratch, long long *__restrict__ counts,
                                                          int *__restrict__ n_clusters, int *__restrict__ map,
                                                          const DerTimedDev td, const DerJerOut jo) {
  der_solve_body<HBM, SWEEP, ATOMS, OVL, JER>(ref, hyp, dur, ma, mb, tab, scratch, counts, n_clusters, map, td, jo);
}

// the instantiation of a launch: 2 classes x 2 (plain, JER) x 5 shapes -- segments, atoms, atoms with two labels, and the
// sweeps of segments and of atoms (a sweep has no second label, and a second label belongs to atoms)
using DerSolveFn = void (*)(const int *, const int *, const int *, const int *, const int *, const DerRec *, long long *, long long *, int *,
                            int *, DerTimedDev, DerJerOut);
template <bool HBM, bool JER> DerSolveFn der_solve_shape(bool sweep, bool atoms, bool ovl) {
  if (sweep) return atoms ? &der_solve_kernel<HBM, true, true, false, JER> : &der_solve_kernel<HBM, true, false, false, JER>;
  if (ovl) return &der_solve_kernel<HBM, false, true, true, JER>;
  return atoms ? &der_solve_kernel<HBM, false, true, false, JER> : &der_solve_kernel<HBM, false, false, false, JER>;
}
DerSolveFn der_solve_fn(bool hbm, bool sweep, bool atoms, bool ovl, bool jer) {
  if (hbm) return jer ? der_solve_shape<true, true>(sweep, atoms, ovl) : der_solve_shape<true, false>(sweep, atoms, ovl);
  return jer ? der_solve_shape<false, true>(sweep, atoms, ovl) : der_solve_shape<false, false>(sweep, atoms, ovl);
}

// every instantiation may take a whole CU's LDS: set once per device
int der_solve_attr(plda_handle *h) {
  static DeviceOnce attr;
  if (attr.needed(h->device)) {
    for (int k = 0; k < 32; ++k) {
      const bool hbm = k & 1, jer = k & 2, sweep = k & 4, atoms = k & 8, ovl = k & 16;
      if (ovl && (sweep || !atoms)) continue;
      PLDA_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void *>(der_solve_fn(hbm, sweep, atoms, ovl, jer)),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, DER_LDS_BYTES));
    }
    attr.done(h->device);
  }
  return PLDA_OK;
}

// the scratch of one launch of scratch-class recordings (PLDA_DER_SCRATCH_BYTES at plda_create for the tests), never less
// than one recording
int64_t der_budget(const plda_handle *h) { return h->der_scratch_bytes > 0 ? h->der_scratch_bytes : (int64_t)256 << 20; }

int der_check_offsets(plda_handle *h, const char *fn, const int64_t *offsets, int64_t R) {
  if (R < 1) return fail(h, PLDA_E_INVAL, "%s: R = %lld (must be >= 1)", fn, (long long)R);
  if (R > (int64_t)0x7fffffff) return fail(h, PLDA_E_INVAL, "%s: R = %lld (at most 2^31 - 1)", fn, (long long)R);
  if (!offsets) return fail(h, PLDA_E_INVAL, "%s: offsets is NULL", fn);
  return check_recordings(h, fn, offsets, R, DER_MAX_HYP, "PLDA_AHC_MAX");
}

// Enqueues the solves of `items` (sr, sh, n, m, off, out, r filled in; w, scr and the launch order are this function's);
// `tab` is the host copy of the launch table, alive until the caller has synchronised.
// `td` non-null: the time-based form (dref and ddur unused).  `jo` non-null: the JER form, with its own LDS accounting.
template <bool SWEEP>
int der_solve_enqueue(plda_handle *h, std::vector<DerRec> &items, std::vector<DerRec> &tab, const int *dref, const int *dhyp,
                      const int *ddur, const int *dma, const int *dmb, long long *dcounts, int *dn_clusters, int *dmap,
                      const DerTimedDev *td, const DerJerOut *jo) {
  static const int bucket_top[] = {8 << 10, 20 << 10, 40 << 10, 80 << 10, DER_LDS_BYTES};
  constexpr int NB = sizeof(bucket_top) / sizeof(bucket_top[0]);
  struct Launch { int64_t first, count; int64_t lds; bool hbm; };
  std::vector<Launch> launches;
  tab.reserve(items.size());
  auto lds_of = [jo](const DerRec &rc, bool hbm) {
    return jo ? der_jer_lds_bytes(rc.sr, rc.w, SWEEP ? rc.n : 0, hbm, SWEEP) : der_lds_bytes(rc.sr, rc.w, SWEEP ? rc.n : 0, hbm);
  };
  for (DerRec &rc : items) rc.w = std::max(rc.sr, rc.sh);
  for (int bk = 0; bk < NB; ++bk) {           // LDS class: one launch per bucket of LDS bytes (a launch takes its largest need)
    const int64_t lo = bk ? bucket_top[bk - 1] : 0, hi = bucket_top[bk];
    Launch L{(int64_t)tab.size(), 0, 0, false};
    for (const DerRec &rc : items) {
      const int64_t b = lds_of(rc, false);
      if (b > lo && b <= hi) { tab.push_back(rc); ++L.count; L.lds = std::max(L.lds, b); }
    }
    if (L.count) launches.push_back(L);
  }
  const int64_t budget = der_budget(h);
  int64_t scratch_need = 0;
  {                                           // scratch class: launches under the budget
    Launch L{(int64_t)tab.size(), 0, 0, true};
    int64_t used = 0;
    for (const DerRec &it : items) {
      if (lds_of(it, false) <= DER_LDS_BYTES) continue;
      const int64_t bytes = (int64_t)8 * it.sr * it.w;
      if (L.count && used + bytes > budget) {
        launches.push_back(L);
        L = Launch{(int64_t)tab.size(), 0, 0, true};
        used = 0;
      }
      DerRec rc = it;
      rc.scr = used / 8;
      tab.push_back(rc);
      ++L.count; L.lds = std::max(L.lds, (int64_t)lds_of(rc, true)); used += bytes;
      scratch_need = std::max(scratch_need, used);
    }
    if (L.count) launches.push_back(L);
  }
  if (scratch_need) PLDA_HIP(h, h->der_scratch.reserve((size_t)scratch_need));
  PLDA_HIP(h, h->der_tab.reserve(tab.size() * sizeof(DerRec)));
  PLDA_HIP(h, hipMemcpyAsync(h->der_tab.p, tab.data(), tab.size() * sizeof(DerRec), hipMemcpyHostToDevice, h->stream));
  const DerRec *dtab = h->der_tab.as<DerRec>();
  long long *scratch = h->der_scratch.as<long long>();
  const bool ovl = !SWEEP && td && td->hyp2;
  PLDA_TRY(der_solve_attr(h));
  TraceScope ts(h, jo ? (SWEEP ? "der.jer_sweep_solve" : "der.jer_solve") : (SWEEP ? "der.sweep_solve" : "der.solve"));
  const DerTimedDev tdv = td ? *td : DerTimedDev{};
  const DerJerOut jov = jo ? *jo : DerJerOut{};
  for (const Launch &L : launches) {
    const DerSolveFn fn = der_solve_fn(L.hbm, SWEEP, td != nullptr, ovl, jo != nullptr);
    for (int64_t c0 = 0; c0 < L.count; c0 += 1 << 20) {
      const unsigned c = (unsigned)std::min<int64_t>(1 << 20, L.count - c0);
      fn<<<c, DER_T, (size_t)L.lds, h->stream>>>(dref, dhyp, ddur, dma, dmb, dtab + L.first + c0, L.hbm ? scratch : nullptr, dcounts,
                                                 dn_clusters, dmap, tdv, jov);
      PLDA_LAUNCH_CHECK(h);
    }
  }
  return PLDA_OK;
}

// the solves of a call, and the synchronisation behind them (also where the enqueue failed half-way: the table is in flight)
template <bool SWEEP>
int der_solve_all(plda_handle *h, std::vector<DerRec> &items, const int *dref, const int *dhyp, const int *ddur,
                  const int *dma, const int *dmb, int64_t *dcounts, int *dn_clusters, int *dmap, const DerTimedDev *td,
                  const DerJerOut *jo) {
  std::vector<DerRec> tab;
  const int rc = der_solve_enqueue<SWEEP>(h, items, tab, dref, dhyp, ddur, dma, dmb, reinterpret_cast<long long *>(dcounts), dn_clusters,
                                   dmap, td, jo);
  const hipError_t e = hipStreamSynchronize(h->stream);
  if (rc != PLDA_OK) return rc;
  PLDA_HIP(h, e);
  return PLDA_OK;
}

}  // namespace

int der_validate(plda_handle *h, const char *fn, const int64_t *offsets, int64_t R) { return der_check_offsets(h, fn, offsets, R); }

int der_sweep_validate(plda_handle *h, const char *fn, const int64_t *offsets, int64_t R, const double *thresholds, int64_t Q,
                       const int32_t *minc) {
  PLDA_TRY(der_check_offsets(h, fn, offsets, R));
  if (Q < 1) return fail(h, PLDA_E_INVAL, "%s: Q = %lld (must be >= 1)", fn, (long long)Q);
  if (Q > 65535) return fail(h, PLDA_E_INVAL, "%s: Q = %lld (at most 65535)", fn, (long long)Q);
  if (!thresholds) return fail(h, PLDA_E_INVAL, "%s: thresholds is NULL", fn);
  for (int64_t q = 0; q < Q; ++q)
    if (std::isnan(thresholds[q])) return fail(h, PLDA_E_INVAL, "%s: thresholds[%lld] is NaN", fn, (long long)q);
  for (int64_t r = 0; minc && r < R; ++r)
    if (minc[r] < 1) return fail(h, PLDA_E_INVAL, "%s: min_clusters[%lld] = %d (must be >= 1)", fn, (long long)r, (int)minc[r]);
  return PLDA_OK;
}

namespace {
int der_plan_of(plda_handle *h, const char *fn, bool jer, int64_t Sr, int64_t Sh, int32_t *out) {
  if (!out) return fail(h, PLDA_E_INVAL, "%s: out is NULL", fn);
  if (Sr < 0 || Sr > DER_MAX_REF) return fail(h, PLDA_E_INVAL, "%s: Sr = %lld (must be 0 ... PLDA_DER_MAX_REF = %d)", fn, (long long)Sr, DER_MAX_REF);
  if (Sh < 0 || Sh > DER_MAX_HYP) return fail(h, PLDA_E_INVAL, "%s: Sh = %lld (must be 0 ... PLDA_AHC_MAX = %d)", fn, (long long)Sh, DER_MAX_HYP);
  auto lds = [&](int64_t w) { return jer ? der_jer_lds_bytes(Sr, w, 0, false, false) : der_lds_bytes(Sr, w, 0, false); };
  const int64_t w = std::max(Sr, Sh);
  const bool hbm = lds(w) > DER_LDS_BYTES;
  int64_t wmax = Sr;                          // the widest matrix of Sr rows the LDS class takes
  while (wmax < DER_MAX_HYP && lds(wmax + 1) <= DER_LDS_BYTES) ++wmax;
  out[0] = hbm ? 1 : 0;
  out[1] = hbm ? (int32_t)(8 * Sr * w) : 0;
  out[2] = (int32_t)wmax;
  return PLDA_OK;
}
}  // namespace

int der_plan(plda_handle *h, int64_t Sr, int64_t Sh, int32_t *out) { return der_plan_of(h, "der_plan", false, Sr, Sh, out); }
// the JER form's boundary: its LDS holds rt and ht beside the column state (the sweeps keep ht in clab's place)
int der_jer_plan(plda_handle *h, int64_t Sr, int64_t Sh, int32_t *out) { return der_plan_of(h, "der_jer_plan", true, Sr, Sh, out); }

namespace {
// one (recording, threshold) of a call: w, scr and the launch order are der_solve_enqueue's
DerRec der_rec(const int64_t *offsets, int64_t r, int64_t out, int sr, int sh, int m) {
  DerRec rc;
  rc.off = offsets[r]; rc.scr = 0; rc.out = out; rc.n = (int)(offsets[r + 1] - offsets[r]);
  rc.sr = sr; rc.sh = sh; rc.w = 0; rc.m = m; rc.r = (int)r;
  return rc;
}

// what der_count_kernel refuses
int der_bad_entries(plda_handle *h, const char *fn, unsigned long long bad, bool jer) {
  return fail(h, PLDA_E_INVAL, "%s: %llu invalid entries (a label below -1 or above its limit, or a negative duration%s)", fn, bad,
              jer ? "; a recording whose durations add up to more than 2^30" : "");
}

// The sweep of either form behind its argument check: the prefix pass (der_prefix_kernel; in the segment form, td NULL, behind
// der_count_kernel), then the Q x R solves.  sr_of(r): the distinct reference labels of recording r in the time-based form;
// the segment form reads them from its count.
// stat: two counters | offsets [R + 1] | thresholds [Q] | sr [R] (segment form only) m [Q, R] minc [R]
template <typename SrOf>
int der_sweep_solve(plda_handle *h, const char *fn, const DerArgs &a, const DerTimedDev *td, SrOf sr_of) {
  const int64_t R = a.R, Q = a.Q, nsr = td ? 0 : R;
  const DerJerOut *jo = a.jer_form ? &a.jo : nullptr;
  const size_t o_thr = 16 + 8 * (size_t)(R + 1), o_int = o_thr + 8 * (size_t)Q;
  PLDA_HIP(h, h->der_stat.reserve(o_int + 4 * (size_t)(nsr + Q * R + R)));
  char *ds = h->der_stat.as<char>();
  unsigned long long *dstat = reinterpret_cast<unsigned long long *>(ds);
  long long *doff = reinterpret_cast<long long *>(ds + 16);
  double *dthr = reinterpret_cast<double *>(ds + o_thr);
  int *dsr = reinterpret_cast<int *>(ds + o_int), *dm = dsr + nsr, *dminc = dm + Q * R;
  PLDA_HIP(h, hipMemsetAsync(ds, 0, 16, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(doff, a.offsets, 8 * (size_t)(R + 1), hipMemcpyHostToDevice, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(dthr, a.thresholds, 8 * (size_t)Q, hipMemcpyHostToDevice, h->stream));
  if (a.minc) PLDA_HIP(h, hipMemcpyAsync(dminc, a.minc, 4 * (size_t)R, hipMemcpyHostToDevice, h->stream));
  {
    TraceScope ts(h, "der.sweep_count");
    if (!td) {
      if (jo) der_count_kernel<true><<<(unsigned)R, DER_T, 0, h->stream>>>(a.ref, nullptr, a.dur, doff, dstat, dsr, nullptr);
      else der_count_kernel<false><<<(unsigned)R, DER_T, 0, h->stream>>>(a.ref, nullptr, a.dur, doff, dstat, dsr, nullptr);
      PLDA_LAUNCH_CHECK(h);
    }
    der_prefix_kernel<<<dim3((unsigned)R, (unsigned)Q), DER_T, 0, h->stream>>>(a.ma, a.mb, a.mc, doff, dthr, a.minc ? dminc : nullptr, (int)R,
                                                                               dstat, dm);
    PLDA_LAUNCH_CHECK(h);
  }
  unsigned long long bad[2] = {0, 0};
  std::vector<int> s((size_t)(nsr + Q * R));      // sr (segment form only), then m
  PLDA_HIP(h, hipMemcpyAsync(bad, ds, 16, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(s.data(), dsr, 4 * s.size(), hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  if (bad[0]) return der_bad_entries(h, fn, bad[0], jo != nullptr);      // (the count alone adds to it)
  if (bad[1])
    return fail(h, PLDA_E_INVAL, "%s: %llu (recording, threshold) pairs whose merge record ends, or holds an entry that is no merge, "
                                 "before the stop rule fires: not a full record", fn, bad[1]);
  std::vector<DerRec> items((size_t)(Q * R));
  for (int64_t q = 0; q < Q; ++q)
    for (int64_t r = 0; r < R; ++r) {
      DerRec &rc = items[(size_t)(q * R + r)];
      rc = der_rec(a.offsets, r, q * R + r, td ? sr_of(r) : s[(size_t)r], 0, s[(size_t)(nsr + q * R + r)]);
      rc.sh = rc.n - rc.m;
    }
  return der_solve_all<true>(h, items, a.ref, nullptr, a.dur, a.ma, a.mb, a.counts, a.n_clusters, nullptr, td, jo);
}
}  // namespace

int der_seg_validate(plda_handle *h, const char *fn, const DerArgs &a, bool sweep) {
  if (!a.ref) return fail(h, PLDA_E_INVAL, "%s: ref is NULL", fn);
  if (!sweep && !a.hyp) return fail(h, PLDA_E_INVAL, "%s: hyp is NULL", fn);
  if (!a.counts) return fail(h, PLDA_E_INVAL, "%s: counts is NULL", fn);
  if (sweep && !a.n_clusters) return fail(h, PLDA_E_INVAL, "%s: n_clusters is NULL", fn);
  if (a.jer_form && !a.jo.jer) return fail(h, PLDA_E_INVAL, "%s: jer is NULL", fn);
  if (sweep) PLDA_TRY(der_sweep_validate(h, fn, a.offsets, a.R, a.thresholds, a.Q, a.minc));
  else PLDA_TRY(der_validate(h, fn, a.offsets, a.R));
  if (sweep && a.offsets[a.R] > a.R && !(a.ma && a.mb && a.mc)) return fail(h, PLDA_E_INVAL, "%s: merge_a, merge_b or merge_cost is NULL", fn);
  return PLDA_OK;
}

int der_seg_device(plda_handle *h, const char *fn, const DerArgs &a, bool sweep) {
  PLDA_TRY(der_seg_validate(h, fn, a, sweep));
  if (sweep) return der_sweep_solve(h, fn, a, nullptr, [](int64_t) { return 0; });
  const int64_t R = a.R;
  const DerJerOut *jo = a.jer_form ? &a.jo : nullptr;
  // stat: two counters | offsets [R + 1] | sr [R] sh [R]
  const size_t ints = 16 + 8 * (size_t)(R + 1);
  PLDA_HIP(h, h->der_stat.reserve(ints + 8 * (size_t)R));
  char *ds = h->der_stat.as<char>();
  unsigned long long *dstat = reinterpret_cast<unsigned long long *>(ds);
  long long *doff = reinterpret_cast<long long *>(ds + 16);
  int *dsr = reinterpret_cast<int *>(ds + ints), *dsh = dsr + R;
  PLDA_HIP(h, hipMemsetAsync(ds, 0, 16, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(doff, a.offsets, 8 * (size_t)(R + 1), hipMemcpyHostToDevice, h->stream));
  {
    TraceScope ts(h, "der.count");
    if (jo) der_count_kernel<true><<<(unsigned)R, DER_T, 0, h->stream>>>(a.ref, a.hyp, a.dur, doff, dstat, dsr, dsh);
    else der_count_kernel<false><<<(unsigned)R, DER_T, 0, h->stream>>>(a.ref, a.hyp, a.dur, doff, dstat, dsr, dsh);
    PLDA_LAUNCH_CHECK(h);
  }
  unsigned long long bad = 0;
  std::vector<int> s((size_t)(2 * R));
  PLDA_HIP(h, hipMemcpyAsync(&bad, ds, 8, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(s.data(), dsr, 8 * (size_t)R, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  if (bad) return der_bad_entries(h, fn, bad, jo != nullptr);
  std::vector<DerRec> items((size_t)R);
  for (int64_t r = 0; r < R; ++r) items[(size_t)r] = der_rec(a.offsets, r, r, s[(size_t)r], s[(size_t)(R + r)], 0);
  return der_solve_all<false>(h, items, a.ref, a.hyp, a.dur, nullptr, nullptr, a.counts, nullptr, a.map, nullptr, jo);
}

// The solves of a time-based call (der_time.hip has validated the call and cut the atoms; recs is the host copy of td.recs):
// one solve per recording against a.hyp (recs[r].sh = its distinct hypothesis labels), or the sweep.
int der_timed_solve(plda_handle *h, const char *fn, const DerTimedRec *recs, const DerTimedDev &td, const DerArgs &a, bool sweep) {
  auto sr_of = [recs](int64_t r) { return __builtin_popcountll(recs[r].umask); };
  if (sweep) return der_sweep_solve(h, fn, a, &td, sr_of);
  std::vector<DerRec> items((size_t)a.R);
  for (int64_t r = 0; r < a.R; ++r) items[(size_t)r] = der_rec(a.offsets, r, r, sr_of(r), recs[r].sh, 0);
  return der_solve_all<false>(h, items, nullptr, a.hyp, nullptr, nullptr, nullptr, a.counts, nullptr, a.map, &td, a.jer_form ? &a.jo : nullptr);
}

}  // namespace plda
