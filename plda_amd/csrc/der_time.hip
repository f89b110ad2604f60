// plda_amd/csrc/der_time.hip -- time-based diarisation error rate: overlapped reference speech, a forgiveness collar, UEM
// scoring regions (the contract is in include/plda_hip.h, "time-based diarisation error rate"; the host models
// are tests/der_time_model.py).  This file cuts every recording's time line into ATOMS -- maximal runs of ticks over which
// the set of reference speakers, the hypothesis segment, the collar depth and the UEM depth do not change -- and keeps the
// scored ones; der.hip's solve then reads atoms where the segment form reads segments (der_solve_kernel<.., ATOMS = true>: the same
// assignment, the matrix filled from atoms).  Everything is an integer; the atoms are a function of the recording alone.
//
//   der_atoms_kernel<HBM>   one workgroup of 256 threads per recording.
//     (1) events.  Every boundary is one 64-bit key (time + 2^20) << 32 | kind << 28 | payload, in a slot fixed by its index:
//         2 per reference turn (start, end; payload = speaker), 4 more per turn when collar > 0 (the zones [b - c, b + c) of
//         both boundaries), 2 per hypothesis segment (payload = segment index), 2 per UEM interval.  An empty interval and an
//         entry that breaks the contract (counted; with hyp2, plda_der_timed_ovl, also a second label without a first or
//         equal to it) leave their slots at the all-ones key, which sorts behind every event.
//         The kinds put every end before every start of the same tick.
//     (2) a bitonic sort of the P keys (P = the slot count rounded up to a power of two, at least 256): in LDS up to
//         P = 16384 (128 KiB of the 160); <HBM> above that the keys live in handle scratch (8 P bytes, at most 1 MiB per
//         recording in flight, launches grouped under the budget of K17's scratch) and go through LDS a tile of 16384 at a
//         time: only the steps at a compare distance of a tile or more (1, 3, 6 passes at P = 2, 4, 8 tiles) run on the
//         scratch itself.  Equal keys are equal events, so the order among them does not matter.
//     (3) scans over the sorted events, each thread a contiguous chunk: the chunk's aggregate (XOR of 1 << speaker, the +-1
//         sums of collar, UEM and hypothesis depth, the position of the last hypothesis start), an exclusive scan of the 256
//         aggregates, then a walk from that prefix.  The XOR gives the reference mask because turns of one speaker are
//         disjoint; the same prefix checks it (a start must find its bit clear, an end set).  A hypothesis depth of 2 is two
//         segments sharing a tick.  The atom behind event k runs to event k + 1 and is SCORED when it is not empty, the collar
//         depth is 0, the UEM depth is positive (no UEM: always), it holds at most one reference speaker under SKIP_OVERLAP,
//         and it holds a reference speaker or a hypothesis segment.
//     (4) the scored atoms are counted per chunk, scanned, and written compacted in time order: (ticks int32, mask u64,
//         segment index int32 or -1); with them the atom count, the union of the masks and the number of distinct hypothesis
//         labels of the recording (all segments), and the call's two violation counters.
//
// Resources (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage): see the table at der_atoms_kernel.
#include "common.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace plda {

namespace {

constexpr int DT_T = 256;
constexpr int DT_BIAS = 1 << 20;                 // the largest collar: a zone may start that far below tick 0
constexpr int DT_MAX_TIME = 1 << 30;
constexpr int DT_MIN_P = 256;
constexpr int DT_LDS_EVENTS = 16384;             // the LDS class: 128 KiB of keys
constexpr int DT_LDS_BYTES = 160 * 1024;
// amask[256] hbits[64] (u64) | acol auem ahyp alast acnt [256] nev (int)
constexpr int DT_FIXED_BYTES = 8 * (DT_T + 64) + 4 * (5 * DT_T + 4);
static_assert(8 * DT_LDS_EVENTS + DT_FIXED_BYTES <= DT_LDS_BYTES, "the LDS class must fit one CU's LDS");
constexpr unsigned long long DT_NONE = ~0ull;
enum { DT_TURN_END = 0, DT_COL_END, DT_HYP_END, DT_UEM_END, DT_TURN_START, DT_COL_START, DT_HYP_START, DT_UEM_START };

// one recording of a launch (host-built, uploaded once per call)
struct DtRec {
  long long toff, soff, uoff;   // first turn, segment, UEM interval
  long long ev;                 // HBM class: first key in the event scratch
  long long aoff;               // first atom
  int nt, n, nu, P;             // turns, segments, UEM intervals; keys to sort
  int r, pad;                   // the recording
};

__host__ __device__ constexpr long long dt_events(long long nt, long long n, long long nu, int collar) {
  return (collar > 0 ? 6 : 2) * nt + 2 * n + 2 * nu;
}

__device__ __forceinline__ unsigned long long dt_key(int t, int kind, int payload) {
  return ((unsigned long long)(unsigned)(t + DT_BIAS) << 32) | ((unsigned long long)kind << 28) | (unsigned)payload;
}

struct DtState { unsigned long long mask; int col, uem, hyp, last; };

__device__ __forceinline__ void dt_apply(DtState &s, unsigned long long key, int pos) {
  const int kind = (int)(key >> 28) & 7;
  switch (kind) {
    case DT_TURN_END: case DT_TURN_START: s.mask ^= 1ull << (key & 63); break;
    case DT_COL_END: --s.col; break;
    case DT_COL_START: ++s.col; break;
    case DT_UEM_END: --s.uem; break;
    case DT_UEM_START: ++s.uem; break;
    case DT_HYP_END: --s.hyp; break;
    default: ++s.hyp; s.last = pos; break;
  }
}

// the steps of merge level k at compare distances jmax, jmax / 2, ..., 1 on the len keys of `buf` (LDS), which are the keys
// base .. base + len of the whole array (the direction of a pair is that of its place in the whole); a barrier behind each
__device__ __forceinline__ void dt_bitonic_tile(unsigned long long *buf, int base, int len, int k, int jmax, int tid) {
  for (int j = jmax; j > 0; j >>= 1) {
    for (int x = tid; x < (len >> 1); x += DT_T) {
      const int lo = ((x & ~(j - 1)) << 1) | (x & (j - 1)), hi = lo | j;
      const unsigned long long a = buf[lo], b = buf[hi];
      if ((a > b) == (((base + lo) & k) == 0)) { buf[lo] = b; buf[hi] = a; }
    }
    __syncthreads();
  }
}

// Resources on gfx950 (kernel-resource-usage): <false> 47 VGPRs, <true> 55 VGPRs; no scratch memory, no spills in either.
// (der_solve_kernel on atoms, der.hip: 44 VGPRs in the LDS class, 40 in the scratch class, as the segment form; no scratch, no spills.
// Its two-label form of K21: the same 44 and 40.  hyp2, K21, left this kernel's 47 and 55 as they were.)
template <bool HBM>
__global__ __launch_bounds__(DT_T) void der_atoms_kernel(const int *__restrict__ tstart, const int *__restrict__ tdur,
                                                         const int *__restrict__ tspk, const int *__restrict__ sstart,
                                                         const int *__restrict__ sdur, const int *__restrict__ hyp,
                                                         const int *__restrict__ hyp2, const int *__restrict__ ustart,
                                                         const int *__restrict__ udur, const DtRec *__restrict__ tab,
                                                         int collar, int flags, int has_uem,
                                                         unsigned long long *events, unsigned long long *stat,
                                                         DerTimedRec *__restrict__ recs, int *__restrict__ aticks,
                                                         int *__restrict__ aseg, unsigned long long *__restrict__ amask_out) {
  extern __shared__ unsigned long long dt_smem[];
  const DtRec rc = tab[blockIdx.x];
  const int tid = threadIdx.x, P = rc.P;
  unsigned long long *p8 = dt_smem;
  unsigned long long *tile = p8, *keys;                   // the LDS class: all P keys; <HBM>: one tile of the keys in scratch
  if constexpr (HBM) { keys = events + rc.ev; p8 += DT_LDS_EVENTS; }
  else { keys = tile; p8 += P; }
  unsigned long long *amask = p8; p8 += DT_T;
  unsigned long long *hbits = p8; p8 += 64;
  int *acol = reinterpret_cast<int *>(p8);
  int *auem = acol + DT_T, *ahyp = auem + DT_T, *alast = ahyp + DT_T, *acnt = alast + DT_T, *nev = acnt + DT_T;

  // (1) the events
  for (int e = tid; e < P; e += DT_T) keys[e] = DT_NONE;
  if (tid < 64) hbits[tid] = 0;
  if (tid == 0) *nev = 0;
  __syncthreads();
  unsigned bad = 0;
  int made = 0;
  const int col0 = 2 * rc.nt, hyp0 = (collar > 0 ? 6 : 2) * rc.nt, uem0 = hyp0 + 2 * rc.n;
  for (int i = tid; i < rc.nt; i += DT_T) {
    const int st = tstart[rc.toff + i], du = tdur[rc.toff + i], sp = tspk[rc.toff + i];
    if (st < 0 || du < 0 || (long long)st + du > DT_MAX_TIME || sp < 0 || sp >= PLDA_DER_MAX_REF) { ++bad; continue; }
    if (du == 0) continue;
    keys[2 * i] = dt_key(st, DT_TURN_START, sp);
    keys[2 * i + 1] = dt_key(st + du, DT_TURN_END, sp);
    made += 2;
    if (collar > 0) {
      keys[col0 + 4 * i] = dt_key(st - collar, DT_COL_START, 0);
      keys[col0 + 4 * i + 1] = dt_key(st + collar, DT_COL_END, 0);
      keys[col0 + 4 * i + 2] = dt_key(st + du - collar, DT_COL_START, 0);
      keys[col0 + 4 * i + 3] = dt_key(st + du + collar, DT_COL_END, 0);
      made += 4;
    }
  }
  for (int t = tid; t < rc.n; t += DT_T) {
    const int st = sstart[rc.soff + t], du = sdur[rc.soff + t], b = hyp ? hyp[rc.soff + t] : 0;
    const int b2 = hyp2 ? hyp2[rc.soff + t] : -1;        // (a second label needs a first one, and another one)
    if (st < 0 || du < 0 || (long long)st + du > DT_MAX_TIME || b < -1 || b >= PLDA_AHC_MAX || b2 < -1 || b2 >= PLDA_AHC_MAX ||
        (b2 >= 0 && (b < 0 || b2 == b))) { ++bad; continue; }
    if (hyp && b >= 0) atomicOr(&hbits[b >> 6], 1ull << (b & 63));
    if (b2 >= 0) atomicOr(&hbits[b2 >> 6], 1ull << (b2 & 63));
    if (du == 0) continue;
    keys[hyp0 + 2 * t] = dt_key(st, DT_HYP_START, t);
    keys[hyp0 + 2 * t + 1] = dt_key(st + du, DT_HYP_END, t);
    made += 2;
  }
  for (int i = tid; i < rc.nu; i += DT_T) {
    const int st = ustart[rc.uoff + i], du = udur[rc.uoff + i];
    if (st < 0 || du < 0 || (long long)st + du > DT_MAX_TIME) { ++bad; continue; }
    if (du == 0) continue;
    keys[uem0 + 2 * i] = dt_key(st, DT_UEM_START, 0);
    keys[uem0 + 2 * i + 1] = dt_key(st + du, DT_UEM_END, 0);
    made += 2;
  }
  if (bad) atomicAdd(stat, (unsigned long long)bad);       // rare: one integer atomic per lane that met one
  if (made) atomicAdd(nev, made);
  __syncthreads();

  // (2) the sort: an ascending bitonic network over the P keys.  The steps with a compare distance below a tile run on the
  // tile in LDS; <HBM> only the steps at a distance of a tile or more touch the keys in scratch, and every merge level ends
  // with one pass of each tile through LDS (P = 32768: 1 pass over scratch and 2 x 2 tile loads, where a plain network has 120)
  if constexpr (!HBM) {
    for (int k = 2; k <= P; k <<= 1) dt_bitonic_tile(keys, 0, P, k, k >> 1, tid);
  } else {
    constexpr int TL = DT_LDS_EVENTS;
    for (int base = 0; base < P; base += TL) {
      for (int e = tid; e < TL; e += DT_T) tile[e] = keys[base + e];
      __syncthreads();
      for (int k = 2; k <= TL; k <<= 1) dt_bitonic_tile(tile, base, TL, k, k >> 1, tid);
      for (int e = tid; e < TL; e += DT_T) keys[base + e] = tile[e];
      __syncthreads();
    }
    for (int k = 2 * TL; k <= P; k <<= 1) {
      for (int j = k >> 1; j >= TL; j >>= 1) {
        for (int x = tid; x < (P >> 1); x += DT_T) {
          const int lo = ((x & ~(j - 1)) << 1) | (x & (j - 1)), hi = lo | j;
          const unsigned long long a = keys[lo], b = keys[hi];
          if ((a > b) == ((lo & k) == 0)) { keys[lo] = b; keys[hi] = a; }
        }
        __syncthreads();
      }
      for (int base = 0; base < P; base += TL) {
        for (int e = tid; e < TL; e += DT_T) tile[e] = keys[base + e];
        __syncthreads();
        dt_bitonic_tile(tile, base, TL, k, TL >> 1, tid);
        for (int e = tid; e < TL; e += DT_T) keys[base + e] = tile[e];
        __syncthreads();
      }
    }
  }

  // (3) the chunk aggregates and their exclusive scan
  const int E = *nev, chunk = (E + DT_T - 1) / DT_T;
  const int lo = min(tid * chunk, E), hi = min(lo + chunk, E);
  {
    DtState s{0, 0, 0, 0, -1};
    for (int pos = lo; pos < hi; ++pos) dt_apply(s, keys[pos], pos);
    amask[tid] = s.mask; acol[tid] = s.col; auem[tid] = s.uem; ahyp[tid] = s.hyp; alast[tid] = s.last;
  }
  __syncthreads();
  if (tid == 0) {
    DtState s{0, 0, 0, 0, -1};
    for (int k = 0; k < DT_T; ++k) {
      const DtState d{amask[k], acol[k], auem[k], ahyp[k], alast[k]};
      amask[k] = s.mask; acol[k] = s.col; auem[k] = s.uem; ahyp[k] = s.hyp; alast[k] = s.last;
      s.mask ^= d.mask; s.col += d.col; s.uem += d.uem; s.hyp += d.hyp; s.last = max(s.last, d.last);
    }
  }
  __syncthreads();
  const DtState start{amask[tid], acol[tid], auem[tid], ahyp[tid], alast[tid]};
  const bool skip = flags & 1;
  // the walk of this thread's chunk: base < 0 checks the events and counts the scored atoms, base >= 0 writes them from there
  auto walk = [&](int base, unsigned &viol, unsigned long long &um) -> int {
    DtState s = start;
    int cnt = 0;
    unsigned long long key = lo < hi ? keys[lo] : 0;
    for (int pos = lo; pos < hi; ++pos) {
      const unsigned long long next = pos + 1 < E ? keys[pos + 1] : key;
      if (base < 0) {
        const int kind = (int)(key >> 28) & 7;
        const bool set = (s.mask >> (key & 63)) & 1;
        if ((kind == DT_TURN_START && set) || (kind == DT_TURN_END && !set) || (kind == DT_HYP_START && s.hyp >= 1)) ++viol;
      }
      dt_apply(s, key, pos);
      const int ticks = (int)(next >> 32) - (int)(key >> 32);
      if (ticks > 0 && s.col == 0 && (!has_uem || s.uem > 0) && !(skip && __popcll(s.mask) > 1) && (s.mask || s.hyp == 1)) {
        if (base >= 0) {
          const long long at = rc.aoff + base + cnt;
          aticks[at] = ticks;
          amask_out[at] = s.mask;
          aseg[at] = s.hyp == 1 && s.last >= 0 ? (int)(keys[s.last] & 0xffff) : -1;
        }
        um |= s.mask;
        ++cnt;
      }
      key = next;
    }
    return cnt;
  };
  unsigned viol = 0;
  unsigned long long um = 0;
  acnt[tid] = walk(-1, viol, um);
  if (viol) atomicAdd(stat + 1, (unsigned long long)viol);
  __syncthreads();                      // (every thread has read its prefix: amask is free for the union)
  if (tid == 0) amask[0] = 0;
  __syncthreads();
  if (um) atomicOr(&amask[0], um);
  // (4) the compacted atoms
  if (tid == 0) {
    int s = 0;
    for (int k = 0; k < DT_T; ++k) { const int c = acnt[k]; acnt[k] = s; s += c; }
    *nev = s;
  }
  __syncthreads();
  walk(acnt[tid], viol, um);
  if (tid == 0) {
    int sh = 0;
    for (int k = 0; k < 64; ++k) sh += __popcll(hbits[k]);
    recs[rc.r] = DerTimedRec{rc.aoff, *nev, sh, amask[0]};
  }
}

int64_t dt_budget(const plda_handle *h) { return h->der_scratch_bytes > 0 ? h->der_scratch_bytes : (int64_t)256 << 20; }

int dt_pow2(int64_t e) {
  int p = DT_MIN_P;
  while (p < e) p <<= 1;
  return p;
}

int dt_check_off(plda_handle *h, const char *fn, const char *name, const char *what, const int64_t *off, int64_t R, int64_t limit,
                 const char *limit_name) {
  if (off[0] != 0) return fail(h, PLDA_E_INVAL, "%s: %s[0] = %lld (must be 0)", fn, name, (long long)off[0]);
  for (int64_t r = 0; r < R; ++r) {
    const int64_t n = off[r + 1] - off[r];
    if (n < 0 || n > limit)
      return fail(h, PLDA_E_INVAL, "%s: recording %lld has %lld %s (must be 0 ... %s = %lld; %s must ascend)", fn, (long long)r,
                  (long long)n, what, limit_name, (long long)limit, name);
  }
  if (off[R] > (int64_t)0x7fffffff) return fail(h, PLDA_E_INVAL, "%s: %lld %s (at most 2^31 - 1)", fn, (long long)off[R], what);
  return PLDA_OK;
}

}  // namespace

int der_timed_plan(plda_handle *h, int64_t n_turns, int64_t n_seg, int64_t n_uem, int32_t collar, int32_t *out) {
  const char *fn = "der_timed_plan";
  if (!out) return fail(h, PLDA_E_INVAL, "%s: out is NULL", fn);
  if (n_turns < 0 || n_turns > PLDA_DER_MAX_TURNS)
    return fail(h, PLDA_E_INVAL, "%s: n_turns = %lld (must be 0 ... PLDA_DER_MAX_TURNS = %d)", fn, (long long)n_turns, PLDA_DER_MAX_TURNS);
  if (n_seg < 0 || n_seg > PLDA_AHC_MAX) return fail(h, PLDA_E_INVAL, "%s: n_seg = %lld (must be 0 ... PLDA_AHC_MAX = %d)", fn, (long long)n_seg, PLDA_AHC_MAX);
  if (n_uem < 0 || n_uem > PLDA_DER_MAX_UEM)
    return fail(h, PLDA_E_INVAL, "%s: n_uem = %lld (must be 0 ... PLDA_DER_MAX_UEM = %d)", fn, (long long)n_uem, PLDA_DER_MAX_UEM);
  if (collar < 0 || collar > DT_BIAS) return fail(h, PLDA_E_INVAL, "%s: collar = %d (must be 0 ... 2^20)", fn, (int)collar);
  const int64_t e = dt_events(n_turns, n_seg, n_uem, collar);
  const bool hbm = e > DT_LDS_EVENTS;
  out[0] = hbm ? 1 : 0;
  out[1] = hbm ? 8 * dt_pow2(e) : 0;
  out[2] = DT_LDS_EVENTS;
  return PLDA_OK;
}

int der_timed_validate(plda_handle *h, const char *fn, const DerArgs &a, bool sweep) {
  if (!a.turn_off) return fail(h, PLDA_E_INVAL, "%s: turn_off is NULL", fn);
  if (!a.sstart) return fail(h, PLDA_E_INVAL, "%s: seg_start is NULL", fn);
  if (!a.sdur) return fail(h, PLDA_E_INVAL, "%s: seg_dur is NULL", fn);
  if (!sweep && !a.hyp) return fail(h, PLDA_E_INVAL, "%s: hyp is NULL", fn);
  if (!a.counts) return fail(h, PLDA_E_INVAL, "%s: counts is NULL", fn);
  if (a.jer_form && !a.jo.jer) return fail(h, PLDA_E_INVAL, "%s: jer is NULL", fn);
  if (sweep && !a.n_clusters) return fail(h, PLDA_E_INVAL, "%s: n_clusters is NULL", fn);
  if (sweep) PLDA_TRY(der_sweep_validate(h, fn, a.offsets, a.R, a.thresholds, a.Q, a.minc));
  else PLDA_TRY(der_validate(h, fn, a.offsets, a.R));
  PLDA_TRY(dt_check_off(h, fn, "turn_off", "turns", a.turn_off, a.R, PLDA_DER_MAX_TURNS, "PLDA_DER_MAX_TURNS"));
  if (a.turn_off[a.R] > 0 && !(a.tstart && a.tdur && a.tspk)) return fail(h, PLDA_E_INVAL, "%s: turn_start, turn_dur or turn_spk is NULL", fn);
  if (a.uem_off) {
    PLDA_TRY(dt_check_off(h, fn, "uem_off", "UEM intervals", a.uem_off, a.R, PLDA_DER_MAX_UEM, "PLDA_DER_MAX_UEM"));
    if (a.uem_off[a.R] > 0 && !(a.ustart && a.udur)) return fail(h, PLDA_E_INVAL, "%s: uem_start or uem_dur is NULL", fn);
  } else if (a.ustart || a.udur) {
    return fail(h, PLDA_E_INVAL, "%s: uem_off is NULL", fn);
  }
  if (a.collar < 0 || a.collar > DT_BIAS) return fail(h, PLDA_E_INVAL, "%s: collar = %d (must be 0 ... 2^20)", fn, (int)a.collar);
  if (a.flags & ~PLDA_DER_SKIP_OVERLAP) return fail(h, PLDA_E_INVAL, "%s: flags = %d (bit 0, PLDA_DER_SKIP_OVERLAP, is the only one)", fn, (int)a.flags);
  if (sweep && a.offsets[a.R] > a.R && !(a.ma && a.mb && a.mc)) return fail(h, PLDA_E_INVAL, "%s: merge_a, merge_b or merge_cost is NULL", fn);
  return PLDA_OK;
}

int der_timed_device(plda_handle *h, const char *fn, const DerArgs &a, bool sweep) {
  PLDA_TRY(der_timed_validate(h, fn, a, sweep));
  const int64_t R = a.R;
  // the launch table: the LDS class by ascending P (one launch per P), then the scratch class in launches under the budget
  std::vector<DtRec> tab((size_t)R);
  int64_t natoms = 0;
  for (int64_t r = 0; r < R; ++r) {
    DtRec &rc = tab[(size_t)r];
    rc.toff = a.turn_off[r]; rc.nt = (int)(a.turn_off[r + 1] - a.turn_off[r]);
    rc.soff = a.offsets[r]; rc.n = (int)(a.offsets[r + 1] - a.offsets[r]);
    rc.uoff = a.uem_off ? a.uem_off[r] : 0; rc.nu = a.uem_off ? (int)(a.uem_off[r + 1] - a.uem_off[r]) : 0;
    const int64_t e = dt_events(rc.nt, rc.n, rc.nu, a.collar);
    rc.P = dt_pow2(e); rc.ev = 0; rc.aoff = natoms; rc.r = (int)r; rc.pad = 0;
    natoms += e;                                          // (E events bound at most E - 1 atoms)
  }
  std::stable_sort(tab.begin(), tab.end(), [](const DtRec &x, const DtRec &y) { return x.P < y.P; });
  struct Launch { int64_t first, count; int P; bool hbm; };
  std::vector<Launch> launches;
  const int64_t budget = dt_budget(h);
  int64_t used = 0, ev_need = 0;
  for (int64_t k = 0; k < R; ++k) {
    DtRec &rc = tab[(size_t)k];
    const bool hbm = rc.P > DT_LDS_EVENTS;
    bool fresh = launches.empty() || launches.back().hbm != hbm || (!hbm && launches.back().P != rc.P);
    if (hbm && !fresh && used + 8 * (int64_t)rc.P > budget) fresh = true;
    if (fresh) { launches.push_back(Launch{k, 0, rc.P, hbm}); used = 0; }
    if (hbm) { rc.ev = used / 8; used += 8 * (int64_t)rc.P; ev_need = std::max(ev_need, used); }
    ++launches.back().count;
    launches.back().P = std::max(launches.back().P, rc.P);
  }
  unsigned long long *dstat = nullptr, *dmask = nullptr;
  DerTimedRec *drecs = nullptr;
  DtRec *dtab = nullptr;
  int *dticks = nullptr, *dseg = nullptr;
  PLDA_TRY(carve(h, h->der_atoms, [&](Layout &l) {
    l.take(dstat, 2).take(drecs, (size_t)R).take(dtab, (size_t)R).take(dmask, (size_t)natoms).take(dticks, (size_t)natoms).take(dseg, (size_t)natoms);
  }));
  if (ev_need) PLDA_HIP(h, h->der_events.reserve((size_t)ev_need));
  static DeviceOnce attr;
  if (attr.needed(h->device)) {
    PLDA_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&der_atoms_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    DT_LDS_BYTES));
    PLDA_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&der_atoms_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    DT_LDS_BYTES));
    attr.done(h->device);
  }
  std::vector<DerTimedRec> recs((size_t)R);
  unsigned long long bad[2] = {0, 0};
  auto enqueue = [&]() -> int {
    PLDA_HIP(h, hipMemsetAsync(dstat, 0, 16, h->stream));
    PLDA_HIP(h, hipMemcpyAsync(dtab, tab.data(), tab.size() * sizeof(DtRec), hipMemcpyHostToDevice, h->stream));
    TraceScope ts(h, "der.atoms");
    unsigned long long *dev = h->der_events.as<unsigned long long>();
    const int32_t *hyp = sweep ? nullptr : a.hyp, *hyp2 = sweep ? nullptr : a.hyp2;      // (the sweep's labels are the replayed slots)
    for (const Launch &L : launches)
      for (int64_t c0 = 0; c0 < L.count; c0 += 1 << 20) {
        const unsigned c = (unsigned)std::min<int64_t>(1 << 20, L.count - c0);
        if (L.hbm)
          der_atoms_kernel<true><<<c, DT_T, 8 * DT_LDS_EVENTS + DT_FIXED_BYTES, h->stream>>>(
              a.tstart, a.tdur, a.tspk, a.sstart, a.sdur, hyp, hyp2, a.ustart, a.udur, dtab + L.first + c0, a.collar, a.flags,
              a.uem_off ? 1 : 0, dev, dstat, drecs, dticks, dseg, dmask);
        else
          der_atoms_kernel<false><<<c, DT_T, (size_t)(8 * L.P + DT_FIXED_BYTES), h->stream>>>(
              a.tstart, a.tdur, a.tspk, a.sstart, a.sdur, hyp, hyp2, a.ustart, a.udur, dtab + L.first + c0, a.collar, a.flags,
              a.uem_off ? 1 : 0, nullptr, dstat, drecs, dticks, dseg, dmask);
        PLDA_LAUNCH_CHECK(h);
      }
    ts.close();
    PLDA_HIP(h, hipMemcpyAsync(bad, dstat, 16, hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipMemcpyAsync(recs.data(), drecs, recs.size() * sizeof(DerTimedRec), hipMemcpyDeviceToHost, h->stream));
    return PLDA_OK;
  };
  const int rc = enqueue();
  const hipError_t e = hipStreamSynchronize(h->stream);     // (also where the enqueue failed half-way: the table is in flight)
  if (rc != PLDA_OK) return rc;
  PLDA_HIP(h, e);
  if (bad[0] || bad[1])
    return fail(h, PLDA_E_INVAL, "%s: %llu invalid entries (a label or a time out of range%s) and %llu invalid events (a turn that starts "
                                 "inside another turn of its speaker, or two hypothesis segments that share a tick)", fn, bad[0],
                a.hyp2 ? ", a second label without a first or equal to it" : "", bad[1]);
  const DerTimedDev td{drecs, dticks, dseg, dmask, sweep ? nullptr : a.hyp2};     // (hyp2 given: the solve's two-label form)
  return der_timed_solve(h, fn, recs.data(), td, a, sweep);
}

}  // namespace plda
