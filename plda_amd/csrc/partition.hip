// plda_amd/csrc/partition.hip -- trial keys (K26): the stable multi-way partition of a trials matrix into one score list per
// (condition bucket, class), on the device (include/plda_hip.h, "trial keys").
//
// The contract is an ORDER: within a list, trials lie by (column strip j / 256, row i, column j), whatever the scores, ld,
// alignment, slab height or grid.  So no cursor is ever taken with an atomic; every trial's slot is computed:
//
//   * geometry (eer_hist_strip_kernel's, one level down): a WAVE owns a unit = (256-column strip, slice of rows), four
//     contiguous columns per lane.  Those columns' speaker ids and codes stay in registers for the whole walk (re-reading the
//     ids per row costs 2x, eer.hip's header); the wave walks down its slice with four rows of loads in flight, float4
//     nontemporal where base and ld allow, scalar otherwise.  The key's table sits in LDS (<= 16 KB); a lane reads the
//     bucket of each of its four pairs from the row of the current enrol code.
//   * rank within a row-strip: each lane packs the lists of its four trials into 8-bit fields of one (n_buckets <= 4) or two
//     64-bit words, and an inclusive scan over the wave (6 shuffle steps) minus the lane's own word gives the exclusive count
//     per list over the lower lanes.  The scan is plain 64-bit addition: a field of the INCLUSIVE sum may reach 256 and carry
//     into its neighbour, but the subtraction is exact modulo 2^64 and every field of the exclusive sum is at most 252, so
//     the difference is the true exclusive sum.  The row total per list is formed in 64-bit arithmetic from lane 63's
//     exclusive fields and its own (256 trials of one list in one row-strip is exactly the case that would wrap a field).
//   * cursors: lane q < 16 holds the next slot of list q of this unit in a register; the other lanes fetch it with a
//     shuffle.  No LDS traffic, no workgroup barrier and no atomic in the loop.
//   * start offsets per (unit, list): a first kernel of the same geometry reads ids and codes only and counts each unit's
//     trials per list (fields flushed into 32-bit counters every 32 rows: a lane adds at most 4 per row).  The host scans
//     the counts unit-ascending (unit = strip * slices + slice, i.e. strip-major then slice-ascending) from each list's
//     offset in its class buffer, and checks the grand totals against the host plan (partition_plan: per-code counts and a
//     hash join): a difference is PLDA_E_HIP and nothing is written.  The slice height is the planner's (so that both
//     100k x 256 and 40 x 1M fill the chip) and cannot show in the output: a list's slots are consecutive in unit order.
//   * slabs (the operand form): the offsets are global and the scatter kernel takes a row range; a unit that a slab boundary
//     cuts continues where it stopped, because every launch writes its cursors back (one wave owns a unit in every launch
//     and the launches are ordered by the stream).
//
// Deviation from the issue's sketch: the table row is read from LDS per pair (4 byte reads per lane and row) instead of
// being held per row in registers -- the row changes with every enrol code, the columns' codes differ per lane.
// The kernel does no arithmetic on scores: they are moved as 32-bit words.
#include "trial_source.hpp"

#include <unordered_map>
#include <vector>

namespace plda {

namespace {

constexpr int PS = PLDA_PARTITION_STRIP;
constexpr int NL = 2 * PLDA_KEY_MAX_BUCKETS;              // lists
constexpr int TAB_MAX = PLDA_KEY_MAX_CODES * PLDA_KEY_MAX_CODES;
static_assert(PS == 256, "a wave of 64 lanes x 4 columns");
typedef float f32x4p __attribute__((ext_vector_type(4)));

struct PartGeom {
  int64_t M, Nt, strips, slices, slice_h;
  int ce, ct;
};

// what a lane knows about its four columns
struct LaneCols {
  int64_t col;
  int64_t ts[4];
  int tc[4];
  bool ok[4];
};

__device__ __forceinline__ void load_table(int8_t *tab, const int8_t *__restrict__ dtable, int n) {
  for (int i = threadIdx.x; i < n; i += 256) tab[i] = dtable[i];
  __syncthreads();
}

__device__ __forceinline__ LaneCols lane_cols(const PartGeom &g, int64_t strip, int lane, const int64_t *__restrict__ tspk,
                                              const uint8_t *__restrict__ tcode) {
  LaneCols c;
  c.col = strip * PS + (int64_t)lane * 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    c.ok[e] = c.col + e < g.Nt;
    c.ts[e] = c.ok[e] ? tspk[c.col + e] : 0;
    c.tc[e] = c.ok[e] ? (int)tcode[c.col + e] : 0;
  }
  return c;
}

// the lists of the lane's four pairs of one row (-1: not a trial), packed: field L of (lo | hi << 64) counts the lane's trials
// of list L
__device__ __forceinline__ void lane_lists(const LaneCols &c, const int8_t *trow, int64_t spk, int L[4], unsigned long long &lo,
                                           unsigned long long &hi) {
  lo = 0; hi = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int b = c.ok[e] ? (int)trow[c.tc[e]] : -1;
    L[e] = b < 0 ? -1 : 2 * b + (c.ts[e] == spk ? 1 : 0);
    if (L[e] >= 0) {
      if (L[e] < 8) lo += 1ull << (8 * L[e]);
      else hi += 1ull << (8 * (L[e] - 8));
    }
  }
}

__device__ __forceinline__ unsigned long long shfl_up64(unsigned long long x, int o) {
  const unsigned a = __shfl_up((unsigned)x, o), b = __shfl_up((unsigned)(x >> 32), o);
  return (unsigned long long)a | ((unsigned long long)b << 32);
}
__device__ __forceinline__ unsigned long long shfl64(unsigned long long x, int src) {
  const unsigned a = __shfl((unsigned)x, src), b = __shfl((unsigned)(x >> 32), src);
  return (unsigned long long)a | ((unsigned long long)b << 32);
}
__device__ __forceinline__ unsigned field(unsigned long long w, int f) { return (unsigned)(w >> (8 * f)) & 255u; }

// the unit of this wave; false: none (the grid's last workgroup)
__device__ __forceinline__ bool wave_unit(const PartGeom &g, int64_t *strip, int64_t *r0, int64_t *r1, int64_t *unit) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  *unit = (int64_t)blockIdx.x * 4 + wave;
  if (*unit >= g.strips * g.slices) return false;
  *strip = *unit / g.slices;
  const int64_t slice = *unit % g.slices;
  *r0 = slice * g.slice_h;
  *r1 = *r0 + g.slice_h < g.M ? *r0 + g.slice_h : g.M;
  return true;
}

// counts[unit][NL]: the trials of every list in every unit; reads ids and codes only
__global__ __launch_bounds__(256) void partition_count_kernel(PartGeom g, const int64_t *__restrict__ espk,
                                                              const uint8_t *__restrict__ ecode, const int64_t *__restrict__ tspk,
                                                              const uint8_t *__restrict__ tcode, const int8_t *__restrict__ dtable,
                                                              unsigned *__restrict__ counts) {
  __shared__ int8_t tab[TAB_MAX];
  load_table(tab, dtable, g.ce * g.ct);
  int64_t strip, r0, r1, unit;
  if (!wave_unit(g, &strip, &r0, &r1, &unit)) return;
  const int lane = threadIdx.x & 63;
  const LaneCols c = lane_cols(g, strip, lane, tspk, tcode);
  unsigned cnt[NL];
#pragma unroll
  for (int q = 0; q < NL; ++q) cnt[q] = 0;
  unsigned long long acc_lo = 0, acc_hi = 0;
  int pending = 0;
  auto flush = [&]() {
#pragma unroll
    for (int q = 0; q < 8; ++q) { cnt[q] += field(acc_lo, q); cnt[8 + q] += field(acc_hi, q); }
    acc_lo = 0; acc_hi = 0; pending = 0;
  };
  for (int64_t row = r0; row < r1; ++row) {
    const int64_t spk = espk[row];
    const int8_t *trow = tab + (int)ecode[row] * g.ct;
    int L[4];
    unsigned long long lo, hi;
    lane_lists(c, trow, spk, L, lo, hi);
    acc_lo += lo; acc_hi += hi;               // (<= 4 per field and row: 32 rows stay below 256)
    if (++pending == 32) flush();
  }
  flush();
#pragma unroll
  for (int q = 0; q < NL; ++q) {
    unsigned v = cnt[q];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == q) counts[unit * NL + q] = v;
  }
}

// The scatter: rows [row0, row0 + rows) of the matrix lie at `scores` (row row0 first).  starts[unit][NL]: the next slot of
// every list of every unit within its class buffer; advanced by what this launch wrote.  HI: lists 8 ... 15 exist.
template <bool HI>
__global__ __launch_bounds__(256) void partition_scatter_kernel(PartGeom g, const float *__restrict__ scores, int64_t ld, int64_t row0,
                                                                int64_t rows, const int64_t *__restrict__ espk,
                                                                const uint8_t *__restrict__ ecode, const int64_t *__restrict__ tspk,
                                                                const uint8_t *__restrict__ tcode, const int8_t *__restrict__ dtable,
                                                                unsigned long long *__restrict__ starts, float *__restrict__ dtar,
                                                                unsigned long long cap_tar, float *__restrict__ dnon,
                                                                unsigned long long cap_non) {
  __shared__ int8_t tab[TAB_MAX];
  load_table(tab, dtable, g.ce * g.ct);
  int64_t strip, r0, r1, unit;
  if (!wave_unit(g, &strip, &r0, &r1, &unit)) return;
  if (r0 < row0) r0 = row0;
  if (r1 > row0 + rows) r1 = row0 + rows;
  if (r0 >= r1) return;
  const int lane = threadIdx.x & 63;
  const LaneCols c = lane_cols(g, strip, lane, tspk, tcode);
  const bool vec = ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(scores) & 15) == 0) && c.ok[3];
  unsigned long long cur = lane < NL ? starts[unit * NL + lane] : 0ull;

  auto place = [&](int64_t row, const unsigned (&v)[4]) {
    const int64_t spk = espk[row];
    const int8_t *trow = tab + (int)ecode[row] * g.ct;
    int L[4];
    unsigned long long lo, hi;
    lane_lists(c, trow, spk, L, lo, hi);
    if (__ballot((lo | hi) != 0ull) == 0ull) return;          // no trial in this row-strip (wave-uniform)
    // inclusive scan of the packed words over the wave, then the exclusive one (exact modulo 2^64: the file header)
    unsigned long long xlo = lo, xhi = hi;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long y = shfl_up64(xlo, o);
      if (lane >= o) xlo += y;
      if (HI) {
        const unsigned long long z = shfl_up64(xhi, o);
        if (lane >= o) xhi += z;
      }
    }
    xlo -= lo; xhi -= hi;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int l = L[e] < 0 ? 0 : L[e];
      const unsigned long long base = shfl64(cur, l);         // (every lane takes part)
      unsigned before = field(HI && l >= 8 ? xhi : xlo, l & 7);
#pragma unroll
      for (int d = 0; d < e; ++d) before += L[d] == L[e] ? 1u : 0u;
      const unsigned long long pos = base + before;
      if (L[e] >= 0) {
        if (L[e] & 1) { if (pos < cap_tar) reinterpret_cast<unsigned *>(dtar)[pos] = v[e]; }
        else { if (pos < cap_non) reinterpret_cast<unsigned *>(dnon)[pos] = v[e]; }
      }
    }
    // the row-strip's totals, in 64-bit arithmetic: lane 63's exclusive fields + its own
    const unsigned long long t_xlo = shfl64(xlo, 63), t_lo = shfl64(lo, 63);
    unsigned long long tot = (unsigned long long)field(t_xlo, lane & 7) + field(t_lo, lane & 7);
    if (HI) {
      const unsigned long long t_xhi = shfl64(xhi, 63), t_hi = shfl64(hi, 63);
      if (lane >= 8) tot = (unsigned long long)field(t_xhi, lane & 7) + field(t_hi, lane & 7);
    } else if (lane >= 8) {
      tot = 0;
    }
    if (lane < NL) cur += tot;
  };

  for (int64_t row = r0; row < r1; row += 4) {
    unsigned v[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (row + u >= r1) break;
      const float *src = scores + (row + u - row0) * ld + c.col;
      if (vec) {
        const f32x4p x = __builtin_nontemporal_load(reinterpret_cast<const f32x4p *>(src));
        v[u][0] = __float_as_uint(x.x); v[u][1] = __float_as_uint(x.y); v[u][2] = __float_as_uint(x.z); v[u][3] = __float_as_uint(x.w);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[u][e] = c.ok[e] ? reinterpret_cast<const unsigned *>(src)[e] : 0u;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (row + u >= r1) break;
      place(row + u, v[u]);
    }
  }
  if (lane < NL) starts[unit * NL + lane] = cur;
}

int key_check(plda_handle *h, const char *fn, const plda_trial_key *key) {
  if (!key || !key->enrol_code || !key->test_code || !key->table)
    return fail(h, PLDA_E_INVAL, "%s: the key, its code arrays or its table is NULL", fn);
  if (key->n_enrol_codes < 1 || key->n_enrol_codes > PLDA_KEY_MAX_CODES || key->n_test_codes < 1 || key->n_test_codes > PLDA_KEY_MAX_CODES)
    return fail(h, PLDA_E_INVAL, "%s: %d x %d codes (1 ... %d per side)", fn, key->n_enrol_codes, key->n_test_codes, PLDA_KEY_MAX_CODES);
  if (key->n_buckets < 1 || key->n_buckets > PLDA_KEY_MAX_BUCKETS)
    return fail(h, PLDA_E_INVAL, "%s: %d buckets (1 ... %d)", fn, key->n_buckets, PLDA_KEY_MAX_BUCKETS);
  const int n = key->n_enrol_codes * key->n_test_codes;
  for (int i = 0; i < n; ++i)
    if (key->table[i] < -1 || key->table[i] >= key->n_buckets)
      return fail(h, PLDA_E_INVAL, "%s: table entry (%d, %d) is %d (-1: not a trial, or a bucket 0 ... %d)", fn, i / key->n_test_codes,
                  i % key->n_test_codes, (int)key->table[i], key->n_buckets - 1);
  return PLDA_OK;
}

}  // namespace

// The plan on the host: HOST ids and codes (key->enrol_code / test_code are host arrays here), O(M + Nt + Ce * Ct)
int partition_plan(plda_handle *h, const char *fn, const int64_t *espk, int64_t M, const int64_t *tspk, int64_t Nt,
                   const plda_trial_key *key, plda_partition_record *plan) {
  if (!espk || !tspk || !plan || M <= 0 || Nt <= 0) return fail(h, PLDA_E_INVAL, "%s: bad argument", fn);
  PLDA_TRY(key_check(h, fn, key));
  const int ce = key->n_enrol_codes, ct = key->n_test_codes, nb = key->n_buckets;
  std::vector<int64_t> ne(ce, 0), nt(ct, 0);
  for (int64_t i = 0; i < M; ++i) {
    if (key->enrol_code[i] >= ce) return fail(h, PLDA_E_INVAL, "%s: enrol_code[%lld] = %d, not below %d", fn, (long long)i, (int)key->enrol_code[i], ce);
    ++ne[key->enrol_code[i]];
  }
  for (int64_t j = 0; j < Nt; ++j) {
    if (key->test_code[j] >= ct) return fail(h, PLDA_E_INVAL, "%s: test_code[%lld] = %d, not below %d", fn, (long long)j, (int)key->test_code[j], ct);
    ++nt[key->test_code[j]];
  }
  int64_t trials[PLDA_KEY_MAX_BUCKETS] = {}, tar[PLDA_KEY_MAX_BUCKETS] = {};
  for (int e = 0; e < ce; ++e)
    for (int t = 0; t < ct; ++t) {
      const int b = key->table[e * ct + t];
      if (b >= 0) trials[b] += ne[e] * nt[t];
    }
  // the hash join, split by code: every enrol speaker gets an index; the rows and the columns of the speakers both sides
  // have are counting-sorted by that index, and per speaker the (enrol code, test code) pairs present are crossed once --
  // the work per speaker is (its distinct enrol codes) x (its distinct test codes), not rows x columns
  std::unordered_map<int64_t, int64_t> index;
  index.reserve((size_t)std::min<int64_t>(M, (int64_t)1 << 26));
  std::vector<int64_t> se((size_t)M), st((size_t)Nt);
  for (int64_t i = 0; i < M; ++i) se[i] = index.emplace(espk[i], (int64_t)index.size()).first->second;
  const int64_t S = (int64_t)index.size();
  std::vector<int64_t> eoff((size_t)S + 1, 0), toff((size_t)S + 1, 0);
  for (int64_t i = 0; i < M; ++i) ++eoff[se[i] + 1];
  for (int64_t j = 0; j < Nt; ++j) {
    auto it = index.find(tspk[j]);
    st[j] = it == index.end() ? -1 : it->second;
    if (st[j] >= 0) ++toff[st[j] + 1];
  }
  for (int64_t s = 0; s < S; ++s) { eoff[s + 1] += eoff[s]; toff[s + 1] += toff[s]; }
  std::vector<uint8_t> ecs((size_t)M), tcs((size_t)toff[S]);
  {
    std::vector<int64_t> eat(eoff.begin(), eoff.end() - 1), tat(toff.begin(), toff.end() - 1);
    for (int64_t i = 0; i < M; ++i) ecs[eat[se[i]]++] = key->enrol_code[i];
    for (int64_t j = 0; j < Nt; ++j) if (st[j] >= 0) tcs[tat[st[j]]++] = key->test_code[j];
  }
  int64_t en[PLDA_KEY_MAX_CODES] = {}, tn[PLDA_KEY_MAX_CODES] = {};
  int el[PLDA_KEY_MAX_CODES], tl[PLDA_KEY_MAX_CODES];
  for (int64_t s = 0; s < S; ++s) {
    if (toff[s] == toff[s + 1]) continue;
    int nel = 0, ntl = 0;
    for (int64_t k = eoff[s]; k < eoff[s + 1]; ++k) if (en[ecs[k]]++ == 0) el[nel++] = ecs[k];
    for (int64_t k = toff[s]; k < toff[s + 1]; ++k) if (tn[tcs[k]]++ == 0) tl[ntl++] = tcs[k];
    for (int a = 0; a < nel; ++a)
      for (int c = 0; c < ntl; ++c) {
        const int b = key->table[el[a] * ct + tl[c]];
        if (b >= 0) tar[b] += en[el[a]] * tn[tl[c]];
      }
    for (int a = 0; a < nel; ++a) en[el[a]] = 0;
    for (int c = 0; c < ntl; ++c) tn[tl[c]] = 0;
  }
  *plan = plda_partition_record{};
  for (int b = 0; b < nb; ++b) {
    plan->count[b][1] = tar[b];
    plan->count[b][0] = trials[b] - tar[b];
    for (int c = 0; c < 2; ++c) {
      plan->offset[b][c] = plan->total[c];
      plan->total[c] += plan->count[b][c];
    }
  }
  for (int b = nb; b < PLDA_KEY_MAX_BUCKETS; ++b)
    for (int c = 0; c < 2; ++c) plan->offset[b][c] = plan->total[c];
  return PLDA_OK;
}

// Every form: the source's ids and the key's codes to the host, the plan, the capacities; the counting kernel, the scan and
// its check; one scatter launch per piece.
int partition_source_device(plda_handle *h, const char *fn, const TrialSource &src, const plda_trial_key *key, float *dtar,
                            int64_t cap_tar, float *dnon, int64_t cap_non, plda_partition_record *plan_out) {
  const int64_t M = src.M, Nt = src.Nt;
  if (!plan_out || !src.espk || !src.tspk || M <= 0 || Nt <= 0) return fail(h, PLDA_E_INVAL, "%s: bad argument", fn);
  PLDA_TRY(key_check(h, fn, key));
  std::vector<int64_t> he((size_t)M), ht((size_t)Nt);
  std::vector<uint8_t> hec((size_t)M), htc((size_t)Nt);
  PLDA_HIP(h, hipMemcpyAsync(he.data(), src.espk, (size_t)M * 8, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(ht.data(), src.tspk, (size_t)Nt * 8, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(hec.data(), key->enrol_code, (size_t)M, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(htc.data(), key->test_code, (size_t)Nt, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  plda_trial_key hkey = *key;
  hkey.enrol_code = hec.data(); hkey.test_code = htc.data();
  plda_partition_record plan;
  PLDA_TRY(partition_plan(h, fn, he.data(), M, ht.data(), Nt, &hkey, &plan));
  *plan_out = plan;
  if (cap_tar < plan.total[1] || cap_non < plan.total[0] || (plan.total[1] > 0 && !dtar) || (plan.total[0] > 0 && !dnon))
    return fail(h, PLDA_E_INVAL, "%s: the buffers hold %lld targets and %lld non-targets, the key selects %lld and %lld", fn,
                (long long)(dtar ? cap_tar : 0), (long long)(dnon ? cap_non : 0), (long long)plan.total[1], (long long)plan.total[0]);
  if (plan.total[0] + plan.total[1] == 0) return PLDA_OK;

  // the planner: about 32 waves per CU IN EVERY LAUNCH (the operand form launches once per slab, and only the units a slab
  // meets have work), slices of at least 16 rows (fewer only when there are fewer) and at most 2^20 (a unit's counts are
  // 32-bit: 2^20 rows x 256 columns)
  PartGeom g;
  g.M = M; g.Nt = Nt; g.ce = key->n_enrol_codes; g.ct = key->n_test_codes;
  g.strips = ceil_div(Nt, PS);
  const int64_t launch_rows = src.kind == TrialSource::SLABS ? std::min(M, src.sl->slab_rows) : M;
  int64_t slices = std::max<int64_t>(1, ceil_div((int64_t)h->num_cus * 32, g.strips));
  slices = std::min(slices, ceil_div(launch_rows, 16));
  g.slice_h = std::min<int64_t>(ceil_div(launch_rows, slices), (int64_t)1 << 20);
  if (h->partition_slice_rows > 0) g.slice_h = std::min<int64_t>(h->partition_slice_rows, (int64_t)1 << 20);      // PLDA_PARTITION_SLICE_ROWS (tests)
  g.slices = ceil_div(M, g.slice_h);
  const int64_t units = g.strips * g.slices;
  const int64_t wgs = ceil_div(units, 4);
  if (wgs > 0x7fffffff) return fail(h, PLDA_E_INVAL, "%s: %lld x %lld is more than one grid of units", fn, (long long)M, (long long)Nt);

  int8_t *dtable = nullptr;
  unsigned *dcounts = nullptr;
  unsigned long long *dstarts = nullptr;
  PLDA_TRY(carve(h, h->trial_hist, [&](Layout &l) {
    l.take(dtable, (size_t)g.ce * g.ct).take(dcounts, (size_t)units * NL).take(dstarts, (size_t)units * NL);
  }));
  PLDA_HIP(h, hipMemcpyAsync(dtable, key->table, (size_t)g.ce * g.ct, hipMemcpyHostToDevice, h->stream));
  partition_count_kernel<<<(unsigned)wgs, 256, 0, h->stream>>>(g, src.espk, key->enrol_code, src.tspk, key->test_code, dtable, dcounts);
  PLDA_LAUNCH_CHECK(h);
  std::vector<unsigned> counts((size_t)units * NL);
  PLDA_HIP(h, hipMemcpyAsync(counts.data(), dcounts, counts.size() * 4, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  std::vector<unsigned long long> starts((size_t)units * NL, 0ull);
  for (int L = 0; L < NL; ++L) {
    const int b = L >> 1, c = L & 1;
    unsigned long long run = (unsigned long long)plan.offset[b][c];
    for (int64_t u = 0; u < units; ++u) {
      starts[(size_t)u * NL + L] = run;
      run += counts[(size_t)u * NL + L];
    }
    if (run - (unsigned long long)plan.offset[b][c] != (unsigned long long)plan.count[b][c])
      return fail(h, PLDA_E_HIP, "%s: the device counted %llu trials of bucket %d, class %d; the plan says %lld", fn,
                  run - (unsigned long long)plan.offset[b][c], b, c, (long long)plan.count[b][c]);
  }
  PLDA_HIP(h, hipMemcpyAsync(dstarts, starts.data(), starts.size() * 8, hipMemcpyHostToDevice, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));      // (`starts` goes with this frame)

  int64_t row0 = 0;
  const bool hi = key->n_buckets > 4;
  return for_each_piece(src, [&](const TrialPiece &pc) -> int {
    auto kern = hi ? partition_scatter_kernel<true> : partition_scatter_kernel<false>;
    kern<<<(unsigned)wgs, 256, 0, h->stream>>>(g, pc.scores, pc.ld, row0, pc.rows, src.espk, key->enrol_code, src.tspk, key->test_code,
                                               dtable, dstarts, dtar, (unsigned long long)plan.total[1], dnon,
                                               (unsigned long long)plan.total[0]);
    PLDA_LAUNCH_CHECK(h);
    row0 += pc.rows;
    return PLDA_OK;
  });
}

int partition_matrix_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *despk,
                            const int64_t *dtspk, const plda_trial_key *key, float *dtar, int64_t cap_tar, float *dnon, int64_t cap_non,
                            plda_partition_record *plan_out) {
  if (!dscores || ld < Nt) return fail(h, PLDA_E_INVAL, "partition_matrix: bad argument");
  return partition_source_device(h, "partition_matrix", TrialSource::matrix(dscores, ld, M, Nt, despk, dtspk), key, dtar, cap_tar, dnon,
                                 cap_non, plan_out);
}

int score_partition_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV, int64_t Nt,
                           const double *dzmean, const double *dzstd, const int64_t *despk, const int64_t *dtspk,
                           const plda_trial_key *key, float *dtar, int64_t cap_tar, float *dnon, int64_t cap_non,
                           plda_partition_record *plan_out) {
  OperandSlabs os;
  TrialSource src;
  PLDA_TRY(operand_source(h, "score_partition", dU, dn, n_uniform, M, dV, Nt, dzmean, dzstd, despk, dtspk, plan_out, &os, &src));
  return partition_source_device(h, "score_partition", src, key, dtar, cap_tar, dnon, cap_non, plan_out);
}

}  // namespace plda
