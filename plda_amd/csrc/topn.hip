// plda_amd/csrc/topn.hip -- top-N selection with indices: closed-set identification and watch-list retrieval.
//
// The reference's callers rank the scores of their nested loop (scoring/scorePLDA.py:302-318).  Here a LINE of the fp32
// trials matrix S [M, Nt] is a row (axis 0: its candidates are the columns) or a column (axis 1: its candidates are the
// rows), and the result of a line is its first top_n candidates in the order (score_key descending, candidate index
// ascending): out_index [L, top_n] int64, out_scores [L, top_n] the matrix entries at those indices, bit for bit.  The order is
// total, so the result depends on nothing but the matrix: not on the piece height, the grid, the launch order or the run.
//   topn_rows_kernel   one workgroup per row.  The key tau of the top_n-th largest by radix refinement on score_key (11 + 11 +
//                      10 bits, per-row LDS histograms, as cohort_topk_stats_kernel of snorm.hip) over (key, column) PAIRS;
//                      where more elements equal tau than are still needed, the same refinement on the column index picks
//                      the lowest columns; the <= 256 chosen pairs are rank-sorted in LDS.
//   topn_cols_kernel   one workgroup per 64 adjacent columns, lane = column, so every row read of a wave is 256 coalesced
//                      bytes.  The running result lives in the caller's output arrays, sorted, and is the state across row
//                      pieces.  An element is a candidate while its column's state is not full or its key is strictly above
//                      the state's last key (earlier rows win ties).  Candidates go to an LDS buffer; the workgroup merges
//                      them into the state at chunk boundaries, when the buffer could overflow and at the end of the piece.
//                      Exact for any data; the SPEED depends on it: columns that ascend with the row index make every
//                      element a candidate (a merge per 128 rows), columns that descend none after the first top_n.
// The operand form never holds the matrix: it walks snorm.hip's row slabs (scored by the trials GEMM, mapped by
// snorm_apply_kernel where S-norm statistics are given, consumed here, dropped).  Beyond the slab nothing is allocated:
// the state of axis 1 IS the output.
#include "trial_source.hpp"

#include <algorithm>

namespace plda {

namespace {

constexpr int TN_THREADS = 1024;
constexpr int TN_WAVES = TN_THREADS / 64;
constexpr int TN_BINS = 2048;
constexpr int TN_COPIES = 8;      // histogram copies, interleaved [bin][lane & 7]
constexpr int TN_WCAP = 512;      // candidate pairs per wave (64 KiB for the workgroup)
constexpr int TN_GATE = 4096;     // compaction is tried when the candidates number at most this (half the list: waves differ)

struct TnShared {
  unsigned hist[TN_BINS * TN_COPIES];       // 64 KiB
  uint2 list[TN_WAVES][TN_WCAP];            // 64 KiB: (key, column) of the keys >= the boundary bin's lower edge, per wave
  uint2 sel[PLDA_TOPN_MAX];                 // the chosen pairs, in any order
  unsigned wcnt[TN_WAVES], wtot[TN_WAVES];
  unsigned res_bin, res_above, res_cnt, nsel;
  int overflow;
};

__device__ __forceinline__ int tn_level_shift(int level) { return level == 0 ? 21 : level == 1 ? 10 : 0; }
__device__ __forceinline__ int tn_level_bits(int level) { return level == 2 ? 10 : 11; }

// every element of the wave's share [q0, q1) of the row, in units of UNIT floats (4: 16-byte loads, the row 16-byte aligned
// and its pitch a multiple of 4; 1: any row); four loads in flight per lane.  f(key, column, valid) is called by ALL lanes of
// the wave the same number of times (f may ballot)
template <int UNIT, typename F>
__device__ __forceinline__ void tn_scan_row(const float *__restrict__ row, int Nc, int q0, int q1, int lane, F &&f) {
  for (int qb = q0; qb < q1; qb += 256) {
    float v[4][UNIT];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = qb + u * 64 + lane;
      if constexpr (UNIT == 4) {
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < q1) {
          const float *p = row + 4 * (int64_t)q;
          if (4 * q + 3 < Nc) x = *reinterpret_cast<const float4 *>(p);
          else { x.x = p[0]; if (4 * q + 1 < Nc) x.y = p[1]; if (4 * q + 2 < Nc) x.z = p[2]; }     // the row's last quad: nothing past Nc is read
        }
        v[u][0] = x.x; v[u][1] = x.y; v[u][2] = x.z; v[u][3] = x.w;
      } else {
        v[u][0] = q < q1 ? row[q] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = qb + u * 64 + lane;
      const bool ok = q < q1;
#pragma unroll
      for (int c = 0; c < UNIT; ++c) {
        const int e = UNIT * q + c;
        f(score_key(v[u][c]), (unsigned)e, ok && e < Nc);
      }
    }
  }
}
template <typename F>
__device__ __forceinline__ void tn_scan_list(const TnShared &sm, int wave, int lane, F &&f) {
  const unsigned n = sm.wcnt[wave];
  for (unsigned i = lane; i < n; i += 64) f(sm.list[wave][i].x, sm.list[wave][i].y, true);
}

__device__ __forceinline__ void tn_zero_hist(TnShared &sm, int tid) {
  for (int i = tid; i < TN_BINS * TN_COPIES; i += TN_THREADS) sm.hist[i] = 0u;
}

// The bin in which the krem-th largest of the histogrammed values lies, the number of values in higher bins and in it.  Called
// by all threads after the histogram's atomics; leaves the histogram zeroed and the workgroup synchronised.
__device__ __forceinline__ void tn_find_bin(TnShared &sm, int tid, unsigned krem, unsigned &bin, unsigned &above, unsigned &cnt) {
  const int lane = tid & 63, wave = tid >> 6;
  __syncthreads();
  // thread t owns bins 2047 - 2t and 2046 - 2t: a prefix sum over the threads runs from the highest bin downwards
  const int hi = TN_BINS - 1 - 2 * tid, lo = hi - 1;
  unsigned c_hi = 0, c_lo = 0;
#pragma unroll
  for (int c = 0; c < TN_COPIES; ++c) { c_hi += sm.hist[hi * TN_COPIES + c]; c_lo += sm.hist[lo * TN_COPIES + c]; }
  const unsigned local = c_hi + c_lo;
  unsigned incl = local;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned x = __shfl_up(incl, o);
    if (lane >= o) incl += x;
  }
  if (lane == 63) sm.wtot[wave] = incl;
  __syncthreads();
  unsigned excl = incl - local;
  for (int w = 0; w < wave; ++w) excl += sm.wtot[w];
  if (excl < krem && krem <= excl + c_hi) { sm.res_bin = (unsigned)hi; sm.res_above = excl; sm.res_cnt = c_hi; }
  else if (excl + c_hi < krem && krem <= excl + local) { sm.res_bin = (unsigned)lo; sm.res_above = excl + c_hi; sm.res_cnt = c_lo; }
  tn_zero_hist(sm, tid);
  __syncthreads();
  bin = sm.res_bin; above = sm.res_above; cnt = sm.res_cnt;
}

// One workgroup per row of a piece.  S: fp32 scores, ld floats per row (columns [Nc, ld) are never used; vec: rows 16-byte
// aligned and ld % 4 == 0).  os / oi: the outputs of the piece's first row.
//   1. tau: histogram of the next 11 / 11 / 10 key bits of the elements that share the prefix found so far, and the bin where
//      the count from the top crosses top_n.  As soon as the elements at or above the boundary bin number <= TN_GATE, ONE more
//      read compacts their (key, column) pairs into LDS, where everything else finishes; a row with a crowded boundary bin
//      goes on over the row itself.
//   2. A elements lie strictly above tau and E equal it.  If E > top_n - A, the (top_n - A)-th LOWEST column among the equal
//      ones is found by the same three levels on ~column (columns are distinct: no ties).
//   3. The pairs above tau and the equal ones up to that column are gathered (exactly top_n) and rank-sorted by (key
//      descending, column ascending); the scores are read back from the row, so a -0.0 stays -0.0.
// Integer histograms and counters only; the positions of the gathered pairs vary from run to run, their ranks do not.
__global__ __launch_bounds__(TN_THREADS) void topn_rows_kernel(const float *__restrict__ S, int64_t ld, int Nc, int top_n, int vec,
                                                               float *__restrict__ os, int64_t *__restrict__ oi) {
  __shared__ TnShared sm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float *__restrict__ row = S + (int64_t)blockIdx.x * ld;
  const int unit = vec ? 4 : 1;
  const int Q = (Nc + unit - 1) / unit;
  const int segQ = (Q + TN_WAVES - 1) / TN_WAVES;
  const int q0 = min(wave * segQ, Q), q1 = min(q0 + segQ, Q);

  tn_zero_hist(sm, tid);
  if (tid == 0) { sm.overflow = 0; sm.nsel = 0u; }
  __syncthreads();

  bool in_lds = false;
  auto scan = [&](auto &&f) {
    if (in_lds) tn_scan_list(sm, wave, lane, f);
    else if (vec) tn_scan_row<4>(row, Nc, q0, q1, lane, f);
    else tn_scan_row<1>(row, Nc, q0, q1, lane, f);
  };

  // ---- 1. the key of the top_n-th largest
  unsigned prefix = 0u, A = 0u, E = 0u;      // the key bits fixed so far; the elements whose key lies above that prefix; in the last bin
  for (int level = 0; level < 3; ++level) {
    const int shift = tn_level_shift(level), bits = tn_level_bits(level);
    const unsigned mask = (1u << bits) - 1u;
    const int hi_shift = shift + bits;             // (32 at level 0: no prefix yet)
    scan([&](unsigned k, unsigned, bool valid) {
      if (valid && (level == 0 || (k >> hi_shift) == prefix)) atomicAdd(&sm.hist[((k >> shift) & mask) * TN_COPIES + (lane & (TN_COPIES - 1))], 1u);
    });
    unsigned bin, above;
    tn_find_bin(sm, tid, (unsigned)top_n - A, bin, above, E);
    A += above;
    prefix = (prefix << bits) | bin;
    if (!in_lds && level < 2 && A + E <= (unsigned)TN_GATE) {
      const unsigned lowkey = prefix << shift;
      unsigned n = 0;
      scan([&](unsigned k, unsigned col, bool valid) {
        const bool cand = valid && k >= lowkey;
        const unsigned long long m = __ballot(cand);
        if (m) {
          const unsigned pos = n + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
          if (cand && pos < (unsigned)TN_WCAP) sm.list[wave][pos] = make_uint2(k, col);
          n += (unsigned)__popcll(m);
        }
      });
      if (lane == 0) {
        sm.wcnt[wave] = n < (unsigned)TN_WCAP ? n : (unsigned)TN_WCAP;
        if (n > (unsigned)TN_WCAP) sm.overflow = 1;
      }
      __syncthreads();
      const bool ovf = sm.overflow != 0;
      __syncthreads();
      if (tid == 0) sm.overflow = 0;       // (a later attempt at the next level starts clean; ordered by tn_find_bin's barriers)
      in_lds = !ovf;
    }
  }
  const unsigned tkey = prefix;
  const unsigned need = (unsigned)top_n - A;     // 1 <= need <= E of the elements equal to tau are taken

  // ---- 2. the highest column taken among the elements equal to tau
  unsigned cmax = 0xffffffffu;
  if (E > need) {
    unsigned cpre = 0u, B = 0u, cnt;
    for (int level = 0; level < 3; ++level) {
      const int shift = tn_level_shift(level), bits = tn_level_bits(level);
      const unsigned mask = (1u << bits) - 1u;
      const int hi_shift = shift + bits;
      scan([&](unsigned k, unsigned col, bool valid) {
        const unsigned v = ~col;
        if (valid && k == tkey && (level == 0 || (v >> hi_shift) == cpre)) atomicAdd(&sm.hist[((v >> shift) & mask) * TN_COPIES + (lane & (TN_COPIES - 1))], 1u);
      });
      unsigned bin, above;
      tn_find_bin(sm, tid, need - B, bin, above, cnt);
      B += above;
      cpre = (cpre << bits) | bin;
    }
    cmax = ~cpre;
  }

  // ---- 3. gather and rank
  scan([&](unsigned k, unsigned col, bool valid) {
    if (valid && (k > tkey || (k == tkey && col <= cmax))) {
      const unsigned pos = atomicAdd(&sm.nsel, 1u);
      if (pos < (unsigned)PLDA_TOPN_MAX) sm.sel[pos] = make_uint2(k, col);
    }
  });
  __syncthreads();
  if (tid < top_n && (unsigned)tid < sm.nsel && sm.sel[tid].y < (unsigned)Nc) {
    const uint2 my = sm.sel[tid];
    int rank = 0;
    for (int j = 0; j < top_n; ++j) {
      const uint2 o = sm.sel[j];
      rank += (o.x > my.x || (o.x == my.x && o.y < my.y)) ? 1 : 0;
    }
    const int64_t at = (int64_t)blockIdx.x * top_n + rank;
    oi[at] = (int64_t)my.y;
    os[at] = row[my.y];
  }
}

constexpr int TC_WAVES = 8;
constexpr int TC_THREADS = TC_WAVES * 64;
constexpr int TC_COLS = 64;
constexpr int TC_PER_WAVE = 16;                      // rows of a chunk per wave, all in flight
constexpr int TC_CHUNK = TC_WAVES * TC_PER_WAVE;     // rows between two barriers: 128
constexpr int TC_CAP = 2 * TC_CHUNK;                 // candidates per column the buffer holds: 256
constexpr int TC_PITCH = TC_COLS + 1;                // [position][column], padded: appends and a column's reads spread over the banks

struct TcShared {
  uint2 cand[TC_CAP * TC_PITCH];                     // 130 KiB: (score bits, row)
  uint2 stage[TC_WAVES][PLDA_TOPN_MAX];              // 16 KiB: the state of the column a wave is merging
  unsigned cnt[TC_COLS];
};

// a sorts before b: key descending, then row ascending (x: score bits, y: row)
__device__ __forceinline__ bool tc_before(uint2 a, uint2 b) {
  const unsigned ka = score_key(__uint_as_float(a.x)), kb = score_key(__uint_as_float(b.x));
  return ka > kb || (ka == kb && a.y < b.y);
}

// One workgroup per 64 adjacent columns of a piece of `rows` rows whose first row is row r0 of the matrix.  os / oi
// [Nt, top_n]: on entry the sorted result of rows [0, r0) (min(top_n, r0) entries per column; nothing is read when r0 = 0),
// on exit that of rows [0, r0 + rows).  A chunk of TC_CHUNK rows is spread over the waves (wave w: rows w, w + 8, ...), every
// lane testing its column's elements against the column's tau as of the last merge; the state holds rows of EARLIER chunks
// only, so an element equal to tau loses its tie and strictly-greater is the exact filter.  The buffer is merged when a
// column holds more than TC_CAP - TC_CHUNK candidates (it could overflow in the next chunk) and after the last chunk.
// Merge of a column, by one wave: the state is staged in LDS; a state entry's new rank is its old one plus the candidates
// that sort before it, a candidate's rank the state entries and candidates that sort before it; ranks below top_n are
// written.  The ranks of distinct (key, row) pairs are a permutation, so every slot is written once.
__global__ __launch_bounds__(TC_THREADS) void topn_cols_kernel(const float *__restrict__ S, int64_t ld, int rows, int64_t r0, int Nt,
                                                               int top_n, float *os, int64_t *oi) {
  __shared__ TcShared sm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t col = (int64_t)blockIdx.x * TC_COLS + lane;
  const bool colok = col < Nt;
  if (tid < TC_COLS) sm.cnt[tid] = 0u;
  int have = (int)(r0 < top_n ? r0 : top_n);        // entries per column in the state (the same for every column)
  long long tau = -1;                                // below every key while the state is not full
  if (colok && have == top_n) tau = (long long)score_key(os[col * top_n + top_n - 1]);
  __syncthreads();
  for (int c0 = 0; c0 < rows; c0 += TC_CHUNK) {
    float v[TC_PER_WAVE];
#pragma unroll
    for (int i = 0; i < TC_PER_WAVE; ++i) {
      const int r = c0 + wave + TC_WAVES * i;
      v[i] = (colok && r < rows) ? S[(int64_t)r * ld + col] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < TC_PER_WAVE; ++i) {
      const int r = c0 + wave + TC_WAVES * i;
      if (colok && r < rows && (long long)score_key(v[i]) > tau) {
        const unsigned pos = atomicAdd(&sm.cnt[lane], 1u);
        if (pos < (unsigned)TC_CAP) sm.cand[pos * TC_PITCH + lane] = make_uint2(__float_as_uint(v[i]), (unsigned)(r0 + r));
      }
    }
    __syncthreads();
    const bool last = c0 + TC_CHUNK >= rows;
    const bool merge = last || __any(sm.cnt[lane] > (unsigned)(TC_CAP - TC_CHUNK));     // every wave reads the same 64 counters
    __syncthreads();
    if (!merge) continue;
    for (int cl = wave; cl < TC_COLS; cl += TC_WAVES) {
      const int c = (int)min(sm.cnt[cl], (unsigned)TC_CAP);
      if (c == 0) continue;                          // (wave-uniform; a column past Nt never has a candidate)
      float *cs = os + ((int64_t)blockIdx.x * TC_COLS + cl) * top_n;
      int64_t *ci = oi + ((int64_t)blockIdx.x * TC_COLS + cl) * top_n;
      for (int i = lane; i < have; i += 64) sm.stage[wave][i] = make_uint2(__float_as_uint(cs[i]), (unsigned)ci[i]);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int i = lane; i < have; i += 64) {
        const uint2 it = sm.stage[wave][i];
        int rank = i;
        for (int j = 0; j < c; ++j) rank += tc_before(sm.cand[j * TC_PITCH + cl], it) ? 1 : 0;
        if (rank < top_n) { cs[rank] = __uint_as_float(it.x); ci[rank] = (int64_t)it.y; }
      }
      for (int j = lane; j < c; j += 64) {
        const uint2 it = sm.cand[j * TC_PITCH + cl];
        int rank = 0;
        for (int i = 0; i < have; ++i) rank += tc_before(sm.stage[wave][i], it) ? 1 : 0;
        for (int i = 0; i < c; ++i) rank += tc_before(sm.cand[i * TC_PITCH + cl], it) ? 1 : 0;
        if (rank < top_n) { cs[rank] = __uint_as_float(it.x); ci[rank] = (int64_t)it.y; }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();               // (the next column's staging overwrites what lanes of this one still read)
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __syncthreads();                                 // the merged state is visible to the workgroup
    if (tid < TC_COLS) sm.cnt[tid] = 0u;
    const int64_t seen = r0 + (c0 + TC_CHUNK < rows ? c0 + TC_CHUNK : rows);
    have = (int)(seen < top_n ? seen : top_n);
    if (colok && have == top_n) tau = (long long)score_key(os[col * top_n + top_n - 1]);
    __syncthreads();
  }
}

// one row piece [r0, r0 + m) of the matrix, at S
int topn_piece(plda_handle *h, const float *S, int64_t ld, int64_t m, int64_t r0, int64_t Nt, int axis, int top_n, float *dos,
               int64_t *doi) {
  TraceScope ts(h, axis == 0 ? "topn.rows" : "topn.cols", (double)m * (double)Nt * 4.0, 2);
  if (axis == 0) {
    const int vec = ((ld & 3) == 0 && (reinterpret_cast<uintptr_t>(S) & 15) == 0) ? 1 : 0;
    topn_rows_kernel<<<(unsigned)m, TN_THREADS, 0, h->stream>>>(S, ld, (int)Nt, top_n, vec, dos + r0 * top_n, doi + r0 * top_n);
  } else {
    topn_cols_kernel<<<(unsigned)ceil_div(Nt, TC_COLS), TC_THREADS, 0, h->stream>>>(S, ld, (int)m, r0, (int)Nt, top_n, dos, doi);
  }
  PLDA_LAUNCH_CHECK(h);
  return PLDA_OK;
}

// the checks the two forms share
int topn_check(plda_handle *h, const char *who, int64_t M, int64_t Nt, int axis, int64_t top_n, const void *dos, const void *doi) {
  if (M < 1) return fail(h, PLDA_E_INVAL, "%s: M = %lld (must be >= 1)", who, (long long)M);
  if (Nt < 1) return fail(h, PLDA_E_INVAL, "%s: Nt = %lld (must be >= 1)", who, (long long)Nt);
  if (Nt > ((int64_t)1 << 30)) return fail(h, PLDA_E_INVAL, "%s: Nt = %lld (at most 2^30: one row of scores must fit a slab)", who, (long long)Nt);
  if (axis != 0 && axis != 1) return fail(h, PLDA_E_INVAL, "%s: axis = %d (must be 0: per row, or 1: per column)", who, axis);
  if (axis == 1 && M > (int64_t)0x7fffffff) return fail(h, PLDA_E_INVAL, "%s: M = %lld (at most 2^31 - 1 rows with axis = 1)", who, (long long)M);
  const int64_t len = axis == 0 ? Nt : M;
  if (top_n < 1 || top_n > std::min<int64_t>(PLDA_TOPN_MAX, len))
    return fail(h, PLDA_E_INVAL, "%s: top_n = %lld (must be in 1 ... min(%d, %s = %lld))", who, (long long)top_n, PLDA_TOPN_MAX,
                axis == 0 ? "Nt" : "M", (long long)len);
  if (!dos) return fail(h, PLDA_E_INVAL, "%s: out_scores is NULL", who);
  if (!doi) return fail(h, PLDA_E_INVAL, "%s: out_index is NULL", who);
  return PLDA_OK;
}

}  // namespace

int topn_matrix_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, int axis, int64_t top_n,
                       float *dos, int64_t *doi) {
  PLDA_TRY(topn_check(h, "topn_matrix", M, Nt, axis, top_n, dos, doi));
  if (!dscores) return fail(h, PLDA_E_INVAL, "topn_matrix: scores is NULL");
  if (ld < Nt) return fail(h, PLDA_E_INVAL, "topn_matrix: ld = %lld < Nt = %lld", (long long)ld, (long long)Nt);
  const int64_t rows = sn_slab_rows(h, M, round_up(Nt, 4));
  for (int64_t r0 = 0; r0 < M; r0 += rows)
    PLDA_TRY(topn_piece(h, dscores + r0 * ld, ld, std::min(rows, M - r0), r0, Nt, axis, (int)top_n, dos, doi));
  return PLDA_OK;
}

int score_topn_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV, int64_t Nt,
                      const double *dzmean, const double *dzstd, const double *demean, const double *destd, const double *dtmean,
                      const double *dtstd, int axis, int64_t top_n, float *dos, int64_t *doi, const CountSet *cs_in) {
  if (!can_score(h)) return fail(h, PLDA_E_NOT_FITTED, "score_topn: model not fitted");
  PLDA_TRY(topn_check(h, "score_topn", M, Nt, axis, top_n, dos, doi));
  if ((dzmean == nullptr) != (dzstd == nullptr)) return fail(h, PLDA_E_INVAL, "score_topn: %s is NULL but its partner is not", dzmean ? "zstd" : "zmean");
  if ((demean == nullptr) != (destd == nullptr)) return fail(h, PLDA_E_INVAL, "score_topn: %s is NULL but its partner is not", demean ? "estd" : "emean");
  if ((dtmean == nullptr) != (dtstd == nullptr)) return fail(h, PLDA_E_INVAL, "score_topn: %s is NULL but its partner is not", dtmean ? "tstd" : "tmean");
  const bool snorm = demean || dtmean;
  if (dzmean && snorm) return fail(h, PLDA_E_INVAL, "score_topn: z-norm statistics (zmean/zstd) together with S-norm statistics (emean/estd, tmean/tstd)");
  if (!dU) return fail(h, PLDA_E_INVAL, "score_topn: U is NULL");
  if (!dV) return fail(h, PLDA_E_INVAL, "score_topn: V is NULL");
  if (!dn && n_uniform <= 0) return fail(h, PLDA_E_INVAL, "score_topn: n_uniform must be > 0 when n_enrol is NULL");
  const int D = h->Dout;
  CountSet cs_local;
  const CountSet *cs = nullptr;
  if (dn) {
    if (cs_in) cs = cs_in;
    else { PLDA_TRY(score_count_set_device(h, dn, M, &cs_local)); cs = &cs_local; }
  }
  const int64_t ld = round_up(Nt, 4);
  const int64_t rows = sn_slab_rows(h, M, ld);
  PLDA_HIP(h, h->sn_slab.reserve((size_t)rows * ld * 4));
  float *slab = h->sn_slab.as<float>();
  h->prep_valid = false;           // (the slabs pack the test side themselves, once)
  for (int64_t r0 = 0; r0 < M; r0 += rows) {
    const int64_t m = std::min(rows, M - r0);
    const int32_t *n0 = dn ? dn + r0 : nullptr;
    if (snorm)
      PLDA_TRY(score_matrix_snorm_device(h, dU + r0 * D, n0, n_uniform, m, dV, Nt, demean ? demean + r0 : nullptr,
                                         destd ? destd + r0 : nullptr, dtmean, dtstd, slab, ld, cs, /*reuse_packed_B=*/r0 > 0));
    else
      PLDA_TRY(score_matrix_device(h, dU + r0 * D, n0, n_uniform, m, dV, Nt, dzmean ? dzmean + r0 : nullptr,
                                   dzstd ? dzstd + r0 : nullptr, slab, ld, /*reuse_packed_B=*/r0 > 0, cs));
    PLDA_TRY(topn_piece(h, slab, ld, m, r0, Nt, axis, (int)top_n, dos, doi));
  }
  h->last_M = M; h->last_Nt = Nt;
  return PLDA_OK;
}

}  // namespace plda
