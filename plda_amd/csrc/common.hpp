// plda_amd/csrc/common.hpp -- handle, error plumbing and device buffers shared by
// the translation units of libplda_hip.so (gfx950 only; no CPU fallback).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <atomic>
#include <vector>

#include "../../include/plda_hip.h"
#include "layout.hpp"

// PLDA_DIAG=1 (plda_amd/build.py --diag -> libplda_hip_diag.so): the measurement arms of the trials GEMM -- bounding arms that
// skip the operand DMA or the stores and return GARBAGE scores, per-wave timelines, clock stamps -- are compiled in and
// selectable through PLDA_GEMM_VARIANT.  The product library is built without it: those kernels are not instantiated and
// plda_create refuses their variant numbers (round-5 review: a stray environment variable must not be able to corrupt scores).
#ifndef PLDA_DIAG
#define PLDA_DIAG 0
#endif

namespace plda {

// Device-allocation bookkeeping shared by the library's only two allocation sites, DevBuf::reserve and Tmp::alloc.
//  * g_device_bytes: the bytes every DevBuf / Tmp of the process holds right now (plda_device_bytes_held; the leak tests).
//  * g_device_bytes_peak: the high-water mark of that counter since the last plda_device_bytes_peak(reset) (one atomic max
//    where the counter grows; the slab-cap test of plda_cohort_stats_dev).
//  * g_scratch_poison (PLDA_SCRATCH_POISON=1 at plda_create; tests only): every allocation gets POISON_TAIL more bytes and is
//    filled with 0xFF bytes (NaN as f64 / f32, -1 as an integer) before it is handed out, so that a kernel reading scratch
//    nobody wrote, or reading past the end of a buffer, shows up as NaN or a bad index instead of the zeros of fresh memory.
//  * g_call_stream: the stream of the entry point running on this thread (api.hip: guarded, set_device; nullptr outside a
//    call) -- a fill is refused while it is being captured into a graph.
// (Not counted or poisoned: the peer transport's flag page, comm.hip, an uncached allocation of its own.)
extern std::atomic<int64_t> g_device_bytes;
extern std::atomic<int64_t> g_device_bytes_peak;
extern std::atomic<int> g_scratch_poison;
extern thread_local hipStream_t g_call_stream;
constexpr size_t POISON_TAIL = (size_t)64 << 10;   // > the row-form EM's worst over-read (15 rows of 8 D bytes at D <= 512)

inline size_t alloc_extra() { return g_scratch_poison.load(std::memory_order_relaxed) ? POISON_TAIL : 0; }
// after a successful allocation of `bytes` (extra included): count it, and poison it when the switch is on
inline hipError_t alloc_done(void *p, size_t bytes) {
  const int64_t now = g_device_bytes.fetch_add((int64_t)bytes, std::memory_order_relaxed) + (int64_t)bytes;
  int64_t peak = g_device_bytes_peak.load(std::memory_order_relaxed);
  while (peak < now && !g_device_bytes_peak.compare_exchange_weak(peak, now, std::memory_order_relaxed)) {}
  if (!g_scratch_poison.load(std::memory_order_relaxed)) return hipSuccess;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (g_call_stream && hipStreamIsCapturing(g_call_stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone)
    return hipErrorStreamCaptureUnsupported;
  hipError_t e = hipMemset(p, 0xFF, bytes);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return e;
}
inline void free_counted(void *p, size_t bytes) {
  if (!p) return;
  (void)hipFree(p);
  g_device_bytes.fetch_sub((int64_t)bytes, std::memory_order_relaxed);
}

// a growable device buffer owned by one handle (or one communicator context): freed by its destructor
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  size_t held = 0;   // bytes of the allocation (cap + the poison tail)
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    size_t want = bytes + bytes / 8 + 256, total = want + alloc_extra();
    hipError_t e = hipMalloc(&p, total);
    if (e != hipSuccess) { p = nullptr; return e; }
    cap = want; held = total;
    e = alloc_done(p, total);
    if (e != hipSuccess) release();
    return e;
  }
  void release() { free_counted(p, held); p = nullptr; cap = 0; held = 0; }
  template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// RAII device temporary of the host-pointer entry points
struct Tmp {
  void *p = nullptr;
  size_t held = 0;
  Tmp() = default;
  Tmp(const Tmp &) = delete;
  Tmp &operator=(const Tmp &) = delete;
  ~Tmp() { free_counted(p, held); }
  hipError_t alloc(size_t bytes) {
    free_counted(p, held); p = nullptr; held = 0;
    const size_t total = (bytes ? bytes : 8) + alloc_extra();
    hipError_t e = hipMalloc(&p, total);
    if (e != hipSuccess) { p = nullptr; return e; }
    held = total;
    e = alloc_done(p, total);
    if (e != hipSuccess) { free_counted(p, held); p = nullptr; held = 0; }
    return e;
  }
  template <typename T> T *as() { return reinterpret_cast<T *>(p); }
};

}  // namespace plda

namespace plda { struct HostPipe; }

namespace plda {
// The distinct enrol counts of a mixed-count trials call (score.hip, "bucketed" path): bucket g <-> vals[g], ascending.
// Passed BY VALUE to the kernels that need it (260 bytes of kernel arguments; no device-side table to keep coherent).
constexpr int CS_MAX = 64;        // more distinct counts than this: the depth-2D form
constexpr int CS_NMAX = 4095;     // a count above this: the depth-2D form
struct CountSet { int G = 0; int32_t vals[CS_MAX] = {}; };
// One (btM, btN) tile grid of trials_gemm_bt4_kernel: per-XCD queues over a table of tiles (score.hip: bt4_schedule)
struct Bt4Table { int btM = -1, btN = -1, colwalk = 0; DevBuf tab; int qbase[8] = {}, qlen[8] = {}; uint64_t used = 0; };
// One arm of PLDA_GEMM_VARIANT: a row of score.hip's table GEMM_ARMS, looked up once by plda_create and kept in the handle.
//  * kernel: which trials-GEMM kernel an fp32 call runs.  GK_SHAPE: the one the shape rule names; GK_128 / GK_BT2 / GK_BT4:
//    that one wherever its guards let it run, else the 128 x 128 kernel; GK_B3: a row of the bf16x3 kernel's instrumentation
//    (PLDA_SCORE_DTYPE chooses that kernel, in front of every arm; an fp32 call under such a row runs the 128 x 128 kernel).
//  * mode: the MODE template bits of the instantiation, for the row's own kernel only (every other kernel runs its MODE 0).
//  * walk: the order of the patches of the one-wave-per-SIMD and the bf16x3 kernel.
//  * diag: a measurement arm (garbage scores or clock stamps), in the diagnostic build only.
enum GemmKernel { GK_SHAPE, GK_128, GK_BT2, GK_BT4, GK_B3 };
enum GemmWalk { GW_SIZE, GW_ROWS, GW_COLS };
struct GemmArm { int variant; GemmKernel kernel; int mode; GemmWalk walk; bool diag; };
}  // namespace plda

// a chunk of rows of ONE source and its coefficients in the EM's two rank-k sums (linalg.hip: em_rank_sums_mstep_f64)
struct SyrkChunk { const double *rows; int nrows; int pad; double c1, c2; };

struct plda_handle {
  std::recursive_mutex mu;   // taken by every C-ABI entry point (api.hip)
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;

  // ---- model (Kaldi `Plda`, pldamodule.cpp:29): host mirror + device copies ----
  bool fitted = false;
  int backend = 0;               // PLDA_BACKEND_PLDA / PLDA_BACKEND_COSINE (plda_backend_set): a cosine handle holds no model, Dout = Din = its dimension
  int Dout = 0, Din = 0;
  std::vector<double> h_mean, h_transform, h_psi, h_offset;
  plda::DevBuf d_mean, d_transform, d_psi, d_offset;
  void *pin_model = nullptr;     // pinned landing area of the model copies that end a fit (mean | transform | psi | offset)
  size_t pin_model_cap = 0;

  // ---- fit state kept for plda_fit_get_stats ----
  int64_t fit_K = 0;
  int fit_D = 0;
  plda::DevBuf f_means, f_counts, f_scatter, f_sum, f_W, f_B;
  plda::DevBuf fit_flag;         // the EM's factorisation flag (read by export_model_kernel at the end of a fit)
  // scratch of the statistics pass and the EM (fit.hip); the grouping's buffers also serve transform's and LDA's grouping
  plda::DevBuf fit_sort;         // the grouping's row permutation, or the radix sort's keys a/b and values a/b
  plda::DevBuf fit_offsets;      // class counts -> offsets [K + 1], then the label-check words (plda_fit: read back by the EM's planning copy)
  plda::DevBuf fit_hist;         // per-chunk class counts -> bases, or the radix sort's digit histograms (+ the largest label)
  plda::DevBuf fit_roww;         // one weight per row of the centroid kernels
  plda::DevBuf fit_xc;           // the statistics pass's class-centred rows [N x D], the operand of the scatter product
  plda::DevBuf fit_mu;           // the global mean, then the EM's scalars (alive until the fit's model export)
  plda::DevBuf fit_csum;         // the class sum's partials per split
  plda::DevBuf em_rows;          // the EM's K x D arrays (row form: the tile table first; its fragment loads over-read the last row)
  plda::DevBuf em_mats;          // the EM's D x D matrices per group (or of the simultaneously-diagonalised arm) and the groups' counts
  plda::DevBuf grp_pos, grp_uniq;   // group_by_label_device: boundary flags -> positions [N + 1]; the distinct labels
  double fit_ms[4] = {0, 0, 0, 0};
  hipEvent_t fit_ev[3] = {nullptr, nullptr, nullptr};   // EM start / end, statistics start on the stream (fit.hip)
  int *fit_dbad = nullptr;       // label-check flags of a statistics pass whose read-back fit_em_device takes over (plda_fit)
  double fit_t0 = 0.0;           // host clock at the start of that pass

  // ---- LDA model (lda.hip; /root/reference/python/liblda/lda.py) ----
  bool lda_fitted = false;
  int lda_solver = 0, lda_D = 0, lda_rank = 0;
  int64_t lda_K = 0;
  plda::DevBuf l_means, l_priors, l_xbar, l_scalings, l_coef, l_intercept, l_evr;
  plda::DevBuf lda_work;         // lda_fit_device's whole workspace (N x D and smaller); the offset row of lda_transform_device

  // ---- host-pointer entry points: pinned ring + copy threads (hostio.hip), two alternating score slabs ----
  plda::HostPipe *hostpipe = nullptr;
  plda::DevBuf hio_O[2];
  int host_variant = 0;          // PLDA_HOST_VARIANT=1: the serial pageable-copy arm of rounds 1-2 (A/B)

  // ---- one-trial score() on the host mirror of psi (plda_score_one): per-n coefficient cache ----
  uint64_t model_epoch = 0;      // bumped whenever the model changes (fit, set_model, truncate, smooth)
  struct OneTrial { uint64_t epoch = ~0ull; int n = 0, D = 0; double logterm = 0.0; std::vector<double> c, ivar, ipsi1; } one;

  // ---- one-trial score through the trial-list kernel: host buffer mapped into the device address space ----
  void *one_host = nullptr, *one_dev = nullptr;
  size_t one_cap = 0;

  // ---- scoring workspace ----
  plda::DevBuf s_Apk, s_Bpk, s_rbias, s_rscale, s_cbias, s_rpair, s_cpair;
  plda::DevBuf s_A16, s_B16;   // the packed operands as three bf16 planes per k-oct (score_bf16x3.inc: opt-in arm)
  int score_dtype = 0;         // PLDA_SCORE_DTYPE=bf16x3 -> 1: the trials GEMM's contraction as three bf16 terms (opt-in; default fp32 MFMA)
  plda::DevBuf host_flag;      // the 8 bytes a kernel leaves for the host: pairs_validate_device's first bad pair, test_side_fingerprint
  plda::DevBuf pair_tab;       // score_pairs_device: the per-count tables, the mean's term and every model's bucket
  plda::DevBuf zn_pilot_rows, zn_pilot_sums;   // z-norm by the pilot: the transformed block of test rows; column sums, squares and counts
  plda::DevBuf tf_pad;   // zero-padded copy of the transform for the one-pass K4 kernel, cached per model
  uint64_t tf_pad_epoch = ~0ull;
  int tf_pad_rows = 0, tf_pad_dinp = 0;
  int64_t last_M = 0, last_Nt = 0;
  const char *last_kernel = nullptr;   // the trials-GEMM kernel of the last score_matrix launch (static string)
  int last_k = 0;
  // the fp64 building blocks' dispatch record (plda_linalg_last_kernels): every dispatch site of linalg.hip and eig_dc.hip
  // appends the kernel it chose with its template arguments (note_kernel below), ';' between entries, each entry once;
  // cleared on entry to plda_sym_eig / plda_gemm_f64 / plda_spd_inverse.  A record that ran full ends in "..."
  char linalg_kernels[1024] = {0};
  int linalg_kernels_len = 0;
  // a test side packed ahead of time (plda_score_prepare_dev / _counts_dev): reused while pointer, size, model and count
  // kind match.  prep_kind: 0 uniform count (prep_nuniform), 1 mixed counts in the depth-2D form, 2 mixed counts in the
  // bucketed form for the count set prep_counts
  bool prep_valid = false;
  int prep_kind = 0;
  plda::CountSet prep_counts;
  const double *prep_dV = nullptr;
  int64_t prep_Nt = 0;
  uint64_t prep_epoch = 0;
  unsigned long long prep_fp = 0;   // content fingerprint of the prepared rows (score.hip: fingerprint_kernel)
  int prep_nuniform = 0;

  // ---- Jacobi sweep graph + warm-start state (linalg.hip) ----
  hipGraphExec_t jac_exec = nullptr;
  double *jac_G = nullptr, *jac_V = nullptr;
  int jac_D = 0;
  long jac_total_sweeps = 0;
  plda::DevBuf jac_work;        // sym_eig_f64: V, A, the eigenvalues and the sweep counters (the sweep graph holds pointers into it)
  // PERSISTENT between calls: the last simultaneous diagonalisation's whitening matrix, eigenvectors (the next call's
  // warm start) and Cholesky flag (linalg.hip: SimdiagState; read back by simdiag_whitening / simdiag_flags / simdiag_finish)
  plda::DevBuf simdiag_state;
  int simdiag_D = 0;
  bool simdiag_has_vr = false;
  plda::DevBuf linalg_part;     // split-K and block partials of the fp64 products (linalg.hip, syrk_blk.inc)
  plda::DevBuf syrk_wts;        // syrk_blk.inc: the row weights of both sources, padded
  bool eig_keep_sign = false;   // LDA: keep negative eigenvalues (PLDA floors them, Kaldi ApplyFloor)

  bool panel_attr_set[16] = {};
  int num_cus = 256;           // hipDeviceAttributeMultiprocessorCount (persistent grids)
  int sort_variant = 0;        // PLDA_SORT_VARIANT=1: fit groups the rows by the radix sort always (0: by counting where the tables fit)
  int transform_variant = 0;   // PLDA_TRANSFORM_VARIANT=1: GEMM + separate length-norm pass (the Dout > 512 path, forced)
  plda::GemmArm gemm_arm = {0, plda::GK_SHAPE, 0, plda::GW_SIZE, false};   // PLDA_GEMM_VARIANT, resolved (default: arm 0)
  int mixed_variant = 0;   // PLDA_MIXED_VARIANT=1: mixed enrol counts always in the depth-2D form [A1 | A2] x [V | V*V] (A/B arm of the bucketed form)
  // PERSISTENT between calls: the scoring coefficient tables of the last call, uniform-count or bucketed (one buffer: a
  // call that fills one form invalidates the other).  Valid while ucoef_* / gcoef_* match (score.hip: prepare_operands)
  plda::DevBuf coef_cache;
  const double *gcoef_ptr = nullptr; uint64_t gcoef_epoch = 0; int gcoef_D = 0; plda::CountSet gcoef_set;   // bucket tables in coef_cache, same rule
  const double *ucoef_ptr = nullptr; uint64_t ucoef_epoch = 0; int ucoef_n = 0, ucoef_D = 0;   // uniform-count coefficients in coef_cache
  int prep_variant = 0;    // PLDA_PREP_VARIANT=1: scoring prep as separate bias / pack / pair kernels (A/B arm of prep_side_kernel)
  int gemm64_variant = 0;  // PLDA_GEMM64_VARIANT=1: fp64 GEMM always on 64 x 64 tiles (A/B arm)
  int jacobi_variant = 0;  // 0: Gram-form block Jacobi round; 1: rotation-by-rotation inner tournament
  int sweep_variant = 0;  // PLDA_SWEEP_VARIANT=1: the 16-wave register kernels of round 2 (SPD inverse, tridiagonalisation); 2: the four-wave scalar sweep at every size (no matrix-core block sweep)
  bool sweep_mfma_attr[17] = {};   // dynamic-LDS attribute of spd_inverse_mfma_kernel<NT> set
  int em_variant = 0;     // 0: grouped closed-form EM (moment or row form by shape); 3 / 4: the moment / the row form always; 1: EM in the simultaneously-diagonalised basis
  int em_groups = 0;      // groups (distinct class counts) of the last grouped EM, 0 if the other path ran
  int em_form = 0;        // EM of the last fit: 0 simultaneously-diagonalised basis, 1 grouped moment form, 2 grouped row form
  // tile schedule of the one-wave-per-SIMD trials GEMM (score.hip: bt4_schedule): per XCD a queue of tiles, consumed
  // through one device-scope counter per queue; the table is rebuilt when the tile grid changes
  plda::DevBuf bt4_cnt, bt4_fringe;   // (bt4_fringe: 256 x 256 scratch slots of the tiles that cross the matrix edge)
  plda::Bt4Table bt4_tabs[6];         // the last few tile grids (sharded scoring alternates full blocks and a ragged tail)
  uint64_t bt4_clock = 0;
  // distinct enrol counts of a mixed-count call: presence bytes + result on the device, pinned landing area
  plda::DevBuf cs_work;
  void *cs_pin = nullptr; int cs_seq = 0;   // pinned words of the count-set result + the sequence number its kernel stores last (score.hip)
  bool timeline_valid = false;   // `timeline` holds the stamps of a timeline or clock arm's launch (score.hip: timeline_buffer)
  plda::DevBuf timeline;

  // ---- profiling (plda_profile_*): event pairs around each trials-GEMM launch ----
  bool prof_on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
  size_t prof_used = 0;
  double prof_flop = 0.0;
  // ---- PLDA_HIP_TRACE / plda_trace_*: named spans (HIP event pairs on the stream) around the stages of fit,
  // transform and scoring; unit 1 = flop, 2 = bytes of algorithmic work ----
  struct TraceSpan { const char *name; hipEvent_t e0, e1; double work; int unit; };
  bool trace_on = false, trace_print = false;
  std::vector<TraceSpan> trace_spans;
  size_t trace_used = 0;

  // ---- multi-GPU (comm.hip): the collective table (RCCL, host-staged or caller-supplied), side stream for the
  // gather, ordering events.  comm_kind: 0 none / emulated, 1 RCCL, 2 host-staged, 3 custom ----
  plda_collectives coll = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int comm_kind = 0;
  bool comm = false;             // a communicator is installed (collectives run)
  int comm_nranks = 1, comm_rank = 0;
  hipStream_t comm_stream = nullptr;
  hipEvent_t comm_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  plda::DevBuf comm_mm, comm_mc;   // merged centroids / counts of a sharded fit (persistent: peers map them)
  plda::DevBuf comm_counts;        // the speaker count of every rank of a sharded fit
  plda::DevBuf comm_hist;          // the [2][2048] counters (or the two key bounds) of one all-reduce of a sharded EER / minDCF

  // ---- further scratch ----
  plda::DevBuf em_chunks;                       // the row-form EM's chunk table (device) ...
  std::vector<SyrkChunk> em_chunks_host;        // ... and its host copy, alive while the upload is in flight
  plda::DevBuf eigdc;            // eig_dc.hip workspace
  plda::DevBuf zn_rows, zn_y, zn_small, zn_cpad;   // z-norm statistics by moments (score.hip; zn_cpad: the padded covariance of the model pass, transform.hip)
  int znorm_variant = 0;         // PLDA_ZNORM_VARIANT=1: every LLR on the fused fp32 GEMM (A/B arm); 2: moments in five passes
  plda::DevBuf eer_slab, eer_smp; // plda_score_eer_dev: the row slab of scores in flight; the pilot's gathered enrol rows
  plda::DevBuf trial_hist;       // eer.hip / dcf.hip: the two histograms of a labelled pass, then its window, DET or survivor output (one buffer: one such call runs at a time); rocch.hip: the edge keys (twice: the sort's two sides), digit histograms, search table, rank counters and neighbour words of a hull call (one layout list), or the PAV map's vertex keys and llr table
  plda::DevBuf eer_list[2];      // eer.hip, single-pass form: the impostor / target scores inside the pilot's key window
  int eer_variant = 0;           // PLDA_EER_VARIANT=1: always the three passes; 2: the single-pass form at every size (tests)
  int mindcf_variant = 0;        // PLDA_MINDCF_VARIANT=1: never compact the survivors into lists; 2: two nodes per read (dcf.hip; tests)
  int rocch_variant = 0;         // PLDA_ROCCH_VARIANT=1: no LDS window, every rank through global atomics; 2: a window of 256 gaps (tests)
  int64_t rocch_edge_cap = 0;    // PLDA_ROCCH_EDGE_CAP: the most edge-class trials a ROCCH call accepts (0: 2^24)
  int64_t eer_slab_rows = 0;     // PLDA_EER_SLAB_ROWS: rows per slab of plda_score_eer_dev (0: <= 4 GiB of scores)
  int64_t partition_slice_rows = 0;   // PLDA_PARTITION_SLICE_ROWS: rows per slice of the partition's units (0: by size, partition.hip; tests -- the output does not depend on it); the partition carves trial_hist (table, unit counts, unit cursors: one layout list)
  plda::DevBuf calib_part;       // calib.hip: one partial plda_calib_record per workgroup of a calibration pass + the reduced one
  plda::DevBuf fusion_part;      // fusion.hip: one partial plda_fusion_record per workgroup of a fusion pass + the reduced one
  plda::DevBuf sn_slab;          // plda_cohort_stats_dev (snorm.hip), plda_score_topn_dev (topn.hip): the row slab of scores in flight
  int64_t sn_slab_rows = 0;      // PLDA_SNORM_SLAB_ROWS: rows per slab of plda_cohort_stats_dev / plda_score_matrix_snorm_dev / plda_topn_matrix_dev / plda_score_topn_dev (0: by size)
  int eer_last_passes = 0;       // full passes over the matrix the last plda_eer_matrix_dev made (1 or 3)
  const int *eigdc_flag = nullptr;   // device flag of the last direct decomposition (sym_eig_dc_status)
  int eig_variant = 0;           // PLDA_EIG_VARIANT: 0 = direct method where supported, 1 = block Jacobi always
  int eig_debug = 0;             // PLDA_EIG_DEBUG (timing experiments only: results are wrong when set)
  int eig_last_method = 0;       // 1 = block Jacobi, 2 = tridiagonalisation + divide and conquer

  // ---- domain adaptation (adapt.hip): the statistics record about the pilot, the slab in flight, the update's matrices ----
  plda::DevBuf ad_rec;           // [(D + 1)^2 augmented sums: S2 | S1 | tw] then the pilot [D]
  plda::DevBuf ad_slab;          // one slab of centred rows [x - p | 1] + the call's partial sums + its reject counters
  plda::DevBuf ad_stage;         // rows (and weights) of one slab of a host-pointer call on their way to the device
  plda::DevBuf ad_work;          // the D x D matrices of plda_adapt_update / plda_blend_model and the staged new model
  int64_t ad_slab_rows = 0;      // PLDA_ADAPT_SLAB_ROWS: rows per slab of plda_adapt_accumulate* (0: by size, adapt.hip)
  bool ad_has = false;           // a record exists (the pilot is set)
  bool ad_used = false;          // plda_adapt_update has consumed it
  int ad_D = 0;
  uint64_t ad_epoch = 0;         // model_epoch at the pilot
  int64_t ad_rows = 0;
  double ad_tw = 0.0;            // host mirror of the record's total weight
  std::vector<double> ad_pilot;  // host mirror of the pilot (bitwise comparisons of plda_adapt_add_stats)

  // ---- speaker clustering (ahc.hip, spectral.hip: one call of either runs at a time and carves these anew) ----
  plda::DevBuf ahc_scratch;      // ahc.hip: the N x N fp64 sums of the HBM-class recordings of one launch, or the wide class's whole state (one layout list: block, sums, sizes, row cache, parents, rescan list, scan partials, control words); spectral.hip: one eigenproblem's working set, then the kept columns, degrees and best-so-far records of one group (one layout list)
  plda::DevBuf ahc_tab;          // ahc.hip: the launch table of a call (one entry per recording); spectral.hip: the call's count of non-finite scores, then the launch table of an enqueue (one layout list)
  plda::DevBuf ahc_slot;         // every segment's final slot, between the merge and the label kernel
  plda::DevBuf ahc_stat;         // the call's count of non-finite scores
  int64_t ahc_scratch_bytes = 0; // PLDA_AHC_SCRATCH_BYTES: the scratch one launch (spectral.hip: one group) may take and the score slab of the operand forms (0: 2 GiB)
  int64_t ahc_wide_batch = 0;    // PLDA_AHC_WIDE_BATCH: the wide class's steps per host check (0: AHCW_BATCH, ahc.hip; tests -- the result does not depend on it)
  int64_t ahc_wide_pieces = 0;   // PLDA_AHC_WIDE_PIECES: the column pieces of one row scan of the wide class (0: by N, ahc.hip; tests -- the result does not depend on it)

  // ---- dense scoring in a recording's PCA subspace (dense_pca.hip) ----
  plda::DevBuf dp_scratch;       // the per-recording arrays of the recordings of one launch group (one layout list per recording)
  plda::DevBuf dp_tab;           // the launch table of an enqueue (one entry per recording, with its scratch pointers)
  plda::DevBuf dp_stat;          // the call's count of non-finite rows, then the first recording that failed its Cholesky / eigensolver
  plda::DevBuf dp_model;         // W and B of the installed model (+ the scratch of forming them), valid while dp_model_epoch matches
  uint64_t dp_model_epoch = 0;
  int dp_model_D = 0;

  // ---- VBx resegmentation (vbx.hip) ----
  plda::DevBuf vbx_scratch;      // the per-recording state of the HBM-class recordings of one launch
  plda::DevBuf vbx_tab;          // the launch table of a call (one entry per recording)
  plda::DevBuf vbx_stat;         // the call's three reject counters, then S of every recording
  int64_t vbx_scratch_bytes = 0; // PLDA_VBX_SCRATCH_BYTES: the scratch one launch may take (0: 1 GiB)

  // ---- diarisation error rate (der.hip) ----
  plda::DevBuf der_scratch;      // the Sr x W int64 confusion matrices of the scratch-class recordings of one launch
  plda::DevBuf der_tab;          // the launch table of a call (one entry per recording and threshold)
  plda::DevBuf der_stat;         // the call's two reject counters, its offsets and thresholds, then Sr, Sh / the prefix lengths
  int64_t der_scratch_bytes = 0; // PLDA_DER_SCRATCH_BYTES: the scratch one launch may take (0: 256 MiB)
  plda::DevBuf der_atoms;        // der_time.hip: the call's violation counter, launch table, per-recording records and scored atoms (one layout list)
  plda::DevBuf der_events;       // der_time.hip: the event keys of the scratch-class recordings of one launch (under the same budget)

  // ---- embedding chain (embed.hip): host mirror (plda_embed_get returns it bit for bit) + device copies ----
  bool em_has = false;
  int em_Din = 0, em_Dout = 0, em_dinp = 0, em_class = 0;
  bool em_has_min = false, em_has_A = false, em_has_mout = false;
  double em_len_in = 0.0, em_len_out = 0.0;
  std::vector<double> em_h_min, em_h_A, em_h_mout;
  plda::DevBuf em_min, em_A, em_mout;
  plda::DevBuf em_apad;          // A zero-padded for the fused kernel ([rows of the Dout class][Din rounded up to 16]), rebuilt by every set
  plda::DevBuf em_v, em_g;       // class 2: one chunk of v and of A v
  plda::DevBuf em_fit;           // plda_embed_fit*: all of v [N, Din], then the statistics
  int embed_variant = 0;         // PLDA_EMBED_VARIANT=1: class 2 (row pass + GEMM + row pass) for every chain with A (A/B arm, tests)
  int embed_cus = 0;             // PLDA_EMBED_CUS: the CU count the fused kernel's main / tail split is sized for (0: the device's; tests)
};

namespace plda {

int fail(plda_handle *h, int code, const char *fmt, ...);
// what a scoring entry point needs: a PLDA model, or the cosine back-end (which scores without one)
inline bool can_score(const plda_handle *h) { return h->fitted || h->backend == PLDA_BACKEND_COSINE; }
// the refusal of every entry point that would install a PLDA model on a cosine handle (nullptr handle text: none)
int refuse_on_cosine(plda_handle *h, const char *fn);
int hip_fail(plda_handle *h, hipError_t e, const char *what, const char *file, int line);
// appends "name", "name<a>", "name<a,b>" or "name<a,b,c>" (+ suffix) to h->linalg_kernels: host-side text only, a few
// dozen nanoseconds per dispatch (no printf formatting: the EM issues hundreds of these products per fit)
void note_kernel(plda_handle *h, const char *name, int nargs = 0, int a = 0, int b = 0, int c = 0, const char *suffix = nullptr);
inline void note_kernels_clear(plda_handle *h) { h->linalg_kernels_len = 0; h->linalg_kernels[0] = 0; }

#define PLDA_HIP(h, expr)                                                          \
  do {                                                                             \
    hipError_t _e = (expr);                                                        \
    if (_e != hipSuccess) return plda::hip_fail((h), _e, #expr, __FILE__, __LINE__); \
  } while (0)

#define PLDA_TRY(...)             \
  do {                            \
    int _rc = (__VA_ARGS__);      \
    if (_rc != PLDA_OK) return _rc; \
  } while (0)

#define PLDA_LAUNCH_CHECK(h) PLDA_HIP(h, hipGetLastError())

// Carves `buf` into the arrays of one list (layout.hpp): sizes the list, reserves, then runs it again for the pointers.
// lay(Layout &) assigns the caller's pointers; they are valid until the next reserve of `buf`.
template <typename F> int carve(plda_handle *h, DevBuf &buf, F &&lay) {
  Layout size;
  lay(size);
  if (!size.ok) return fail(h, PLDA_E_INVAL, "scratch layout overflows size_t");
  PLDA_HIP(h, buf.reserve(size.end));
  Layout at{buf.as<char>()};
  lay(at);
  return PLDA_OK;
}

// RAII span of the trace: records an event on h->stream at construction and destruction (nothing when tracing is off;
// never inside a stream capture).  `name` must be a string literal.
struct TraceScope {
  plda_handle *h;
  long idx = -1;
  TraceScope(plda_handle *hh, const char *name, double work = 0.0, int unit = 0) : h(hh) { open(name, work, unit); }
  // closes the running span and opens the next stage's
  void next(const char *name, double work = 0.0, int unit = 0) {
    close();
    open(name, work, unit);
  }
  void close() {
    if (idx >= 0) (void)hipEventRecord(h->trace_spans[idx].e1, h->stream);
    idx = -1;
  }
  void open(const char *name, double work, int unit) {
    if (!h->trace_on) return;
    // bounded: a long-running process that never reads the trace keeps its first 8192 spans (16 384 events), not an
    // ever-growing vector; plda_trace_read(reset) or plda_destroy start over
    if (h->trace_used >= 8192) return;
    if (h->trace_used == h->trace_spans.size()) {
      plda_handle::TraceSpan sp{name, nullptr, nullptr, 0.0, 0};
      if (hipEventCreate(&sp.e0) != hipSuccess || hipEventCreate(&sp.e1) != hipSuccess) return;
      h->trace_spans.push_back(sp);
    }
    idx = (long)h->trace_used++;
    auto &sp = h->trace_spans[idx];
    sp.name = name; sp.work = work; sp.unit = unit;
    (void)hipEventRecord(sp.e0, h->stream);
  }
  ~TraceScope() { close(); }
};

// Function attributes (the dynamic-LDS opt-in) are per DEVICE, and handles on different GPUs or threads share a launch
// template's statics: one bit per device, set only after the attribute call succeeded (two racing threads both set it).
struct DeviceOnce {
  std::atomic<unsigned long long> mask{0};
  bool needed(int device) const { return !(mask.load(std::memory_order_acquire) & (1ull << (device & 63))); }
  void done(int device) { mask.fetch_or(1ull << (device & 63), std::memory_order_release); }
};

constexpr size_t TIMELINE_WORDS = 8 * 16 * 8 * 8;   // [tile < 8][stage < 16][wave < 8][8] shader-clock stamps

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
inline int64_t ceil_div(int64_t x, int64_t m) { return (x + m - 1) / m; }

// upload model arrays held in h->h_* to the device copies
int model_to_device(plda_handle *h);

// ---- linalg.hip (fp64 building blocks; all enqueue on h->stream) ----
// C[M,N] (ldc) = alpha * sum_k A(m,k) * kw[k]? * B(k,n) + beta * C
// A(m,k) = A[m*sam + k*sak], B(k,n) = B[k*sbk + n*sbn]; exactly one of (sam,sak)
// and one of (sbk,sbn) must be 1.  kw nullable.  Uses split-K with a
// deterministic second-stage reduction when K is long and M*N small.
int gemm_f64_batched(plda_handle *h, int64_t M, int64_t N, int64_t K, double alpha, const double *A, int64_t sam,
                     int64_t sak, int64_t strideA, const double *B, int64_t sbk, int64_t sbn, int64_t strideB,
                     const double *kw, double beta, double *C, int64_t ldc, int64_t strideC, int batch);
// C = X^T diag(kw) X + w2 X2^T X2 (one launch for D <= 208)
int syrk_pair_f64(plda_handle *h, int D, int64_t K1, const double *X, int64_t ldx, const double *kw, int64_t K2,
                  const double *X2, int64_t ldx2, double w2, double *C, int64_t ldc);
// the row-form EM's two rank-k sums + M-step in two launches (D <= 208; *used = false otherwise): a table of row chunks with
// their coefficients in the two sums (built once per fit), Bout != Bin
int em_rank_chunk_bound(int G, int D, int64_t K, int cus);
int em_rank_chunks(int G, int D, int64_t K, int cus, const double *X, const double *gn, const double *gk, const double *Z,
                   const double *Wn, SyrkChunk *out);
int em_rank_sums_mstep_f64(plda_handle *h, int D, const SyrkChunk *chunks, int nchunks, const double *S, double sumK, double cw,
                           double cntW, double cntB, double *W, const double *Bin, double *Bout, bool *used);
int syrk_znorm_f64(plda_handle *h, int D0, int64_t K, const double *X, const double *zc, const double *zs, double *C, bool *used);
int gemm_f64(plda_handle *h, int64_t M, int64_t N, int64_t K, double alpha, const double *A,
             int64_t sam, int64_t sak, const double *B, int64_t sbk, int64_t sbn,
             const double *kw, double beta, double *C, int64_t ldc);
// in-place lower Cholesky (upper triangle zeroed); *dflag (device int) set to 1 on failure
// X = L^{-1} for lower-triangular L (row-major); X written fully (upper = 0)
// up to three independent batched products C = A B of one shape in one launch (M, N, K <= 256), else sequentially
struct GemmSet {
  const double *A; int64_t sam, sak, strideA;
  const double *B; int64_t sbk, sbn, strideB;
  double *C; int64_t ldc, strideC;
};
int gemm_f64_multi(plda_handle *h, int64_t M, int64_t N, int64_t K, const GemmSet *sets, int nsets, int batch);
int spd_inverse_f64(plda_handle *h, const double *W, const double *B, const double *gn, int D, double *out,
                    int *dflag, int batch);
// T_g = chol(W + gn[g] B)^-1 (lower triangular) for g < batch; scr: 3 D^2 doubles per group
int whiten_groups_f64(plda_handle *h, const double *W, const double *B, const double *gn, int D, double *T, double *scr,
                      int *dflag, int batch);
// [batch] SPD inverses of any size (A^-1 = T^T T, T = blocked whitening); out may be A itself; scr: 3 n^2 doubles each
int spd_inverse_blocked(plda_handle *h, const double *A, int n, int lda, int64_t sa, double *out, int ldo,
                        int64_t so, double *scr, int64_t sscr, int *dflag, int batch);
// symmetric eigendecomposition of G (row-major, destroyed): eigenvalues sorted
// descending in s[D] (floored at 0), eigenvectors in the ROWS of Vrows.
int sym_eig_f64(plda_handle *h, double *G, int D, double *s, double *Vrows, int *sweeps_out,
                const double *warm);
// direct method (eig_dc.hip): Householder tridiagonalisation + divide and conquer + back-transformation.
// *status != 0: not supported / gave up -> use sym_eig_f64.  G is not modified.
int sym_eig_dc_f64(plda_handle *h, const double *G, int D, double *s, double *Vrows, int *status);   // status == nullptr: deferred
int sym_eig_dc_status(plda_handle *h, int *status);
// eig_sort_kernel of linalg.hip (rank sort descending, optional floor at zero, row permutation)
int eig_sort_rows(plda_handle *h, const double *lam, const double *V, int D, double *s, double *Vsorted);
int sym_eig_auto_f64(plda_handle *h, double *G, int D, double *s, double *Vrows);   // direct, else block Jacobi
int simdiag_enqueue(plda_handle *h, const double *W, const double *B, int D, double *T, double *Tinv, double *psi,
                    bool *pending);
int simdiag_finish(plda_handle *h, const double *W, const double *B, int D, double *T, double *Tinv, double *psi,
                   bool *redo);
void simdiag_flags(plda_handle *h, int D, const int **chol_flag, const int **eig_flag);
int simdiag_finish_with(plda_handle *h, const double *W, const double *B, int D, double *T, double *Tinv, double *psi,
                        int chol_flag, int eig_status, bool *redo);
// simultaneous diagonalisation of (W,B): T W T^T = I, T B T^T = diag(psi);
// T [D,D], Tinv = T^{-1} (nullable), psi[D].  W,B are not modified.
int simdiag_f64(plda_handle *h, const double *W, const double *B, int D, double *T,
                double *Tinv, double *psi, bool warm_start);
const double *simdiag_whitening(plda_handle *h, int D);   // chol(W)^-1 of the last simdiag of size D (device, [D][D])

int syrk_f64(plda_handle *h, int D, int64_t K, double alpha, const double *X, int64_t ldx, const double *kw, double beta,
             double *C, int64_t ldc);   // C = alpha X^T diag(kw) X + beta C, X [K, D] (both triangles written)

// ---- adapt.hip (PLDA domain adaptation: the unsupervised adaptor's statistics and update, interpolation of two models) ----
int adapt_reset(plda_handle *h);
int adapt_accumulate(plda_handle *h, const double *X, int64_t N, int Din, const double *weights, bool host);
int adapt_get_stats(plda_handle *h, double *tw, int64_t *rows, double *pilot, double *s1, double *s2);
int adapt_add_stats(plda_handle *h, double tw, int64_t rows, const double *pilot, const double *s1, const double *s2);
int adapt_update(plda_handle *h, double ws, double bs, double mds, double *eig, plda_adapt_info *info);
int blend_model(plda_handle *h, int D, const double *mean2, const double *transform2, const double *psi2, double alpha,
                double alpha_mean);
// W = (T^T T)^-1, Tinv = T^-1, B = Tinv diag(psi) Tinv^T of a square model (tmp: D^2, scr: 3 D^2 doubles; *flag: T^T T not SPD)
int model_covariances_f64(plda_handle *h, const double *T, const double *psi, int D, double *W, double *B, double *Tinv, double *tmp,
                          double *scr, int *flag);

// ---- embed.hip (the embedding chain in front of the model: centre, length-normalise, project, re-centre, length-normalise) ----
int embed_plan(plda_handle *h, int Din, int Dout, int has_A, int dtype, int32_t *out);
int embed_set(plda_handle *h, int Din, int Dout, const double *m_in, double len_in, const double *A, const double *m_out,
              double len_out);   // HOST arrays
int embed_clear(plda_handle *h);
int embed_apply_device(plda_handle *h, const void *dX, int dtype, int64_t R, int Din, double *dout);
int embed_fit_validate(plda_handle *h, int dtype, int64_t N, int Din, bool has_labels, int64_t K, int kind, int Dout, double len_in,
                       double len_out);
int embed_fit_device(plda_handle *h, const void *dX, int dtype, int64_t N, int Din, const uint64_t *dlabels, int64_t K, int kind,
                     int Dout, double len_in, double len_out, double *eig);   // eig: HOST, nullable

// ---- the clustering family (ahc.hip, spectral.hip, dense_pca.hip, vbx.hip, der.hip): what its files share ----
// The recordings check of every validator, behind the validator's own head (its R, NULL and scalar checks): offsets[0], every
// recording's size in 1 ... max_n (printed as `max_name`), each(r, n) for the checks that belong inside the same walk, the total.
template <typename F>
int check_recordings(plda_handle *h, const char *fn, const int64_t *offsets, int64_t R, int max_n, const char *max_name, F &&each) {
  if (offsets[0] != 0) return fail(h, PLDA_E_INVAL, "%s: offsets[0] = %lld (must be 0)", fn, (long long)offsets[0]);
  for (int64_t r = 0; r < R; ++r) {
    const int64_t n = offsets[r + 1] - offsets[r];
    if (n < 1 || n > max_n)
      return fail(h, PLDA_E_INVAL, "%s: recording %lld has %lld segments (must be 1 ... %s = %d; offsets must ascend)", fn, (long long)r,
                  (long long)n, max_name, max_n);
    PLDA_TRY(each(r, n));
  }
  if (offsets[R] > (int64_t)0x7fffffff) return fail(h, PLDA_E_INVAL, "%s: %lld segments (at most 2^31 - 1)", fn, (long long)offsets[R]);
  return PLDA_OK;
}
inline int check_recordings(plda_handle *h, const char *fn, const int64_t *offsets, int64_t R, int max_n, const char *max_name) {
  return check_recordings(h, fn, offsets, R, max_n, max_name, [](int64_t, int64_t) { return PLDA_OK; });
}
// behind it, in the forms that take score blocks: block r holds at least N_r x N_r floats
inline int check_block_off(plda_handle *h, const char *fn, const int64_t *block_off, const int64_t *offsets, int64_t R) {
  if (!block_off) return fail(h, PLDA_E_INVAL, "%s: block_off is NULL", fn);
  if (block_off[0] < 0) return fail(h, PLDA_E_INVAL, "%s: block_off[0] = %lld (must be >= 0)", fn, (long long)block_off[0]);
  for (int64_t r = 0; r < R; ++r) {
    const int64_t n = offsets[r + 1] - offsets[r];
    if (block_off[r + 1] - block_off[r] < n * n)
      return fail(h, PLDA_E_INVAL, "%s: block %lld holds %lld floats, its recording needs %lld x %lld", fn, (long long)r,
                  (long long)(block_off[r + 1] - block_off[r]), (long long)n, (long long)n);
  }
  return PLDA_OK;
}
// the scratch of one launch or group of the AHC, spectral and dense-PCA back-ends, and four times the floats of one score slab
// of their operand forms (slab_walk.hpp): the S-norm slab's rule (<= 2 GiB; PLDA_AHC_SCRATCH_BYTES at plda_create for the
// tests), never less than one recording
inline int64_t cluster_budget(const plda_handle *h) { return h->ahc_scratch_bytes > 0 ? h->ahc_scratch_bytes : (int64_t)2 << 30; }
// ahc.hip: scores the blocks of recordings [r0, r1) of dX into the slab at boff[r - r0] (a SlabWalk's run), under one trace
// span `span` (a string literal) that carries their flop count
int score_blocks_device(plda_handle *h, const char *span, const double *dX, const int64_t *offsets, int64_t r0, int64_t r1,
                        const int64_t *boff, float *slab);
// ahc.hip: reads the 8-byte counter of non-finite scores behind everything enqueued, and synchronises even when rc has already
// failed (the host tables of the launches must outlive the stream); rc if it failed, else the count's error, else PLDA_OK
int cluster_counted(plda_handle *h, const char *fn, const void *dbad, int rc = PLDA_OK);

// ---- ahc.hip (speaker clustering: batched average-linkage AHC on score blocks; block_off / offsets / minc are HOST arrays) ----
// The arguments every plda_*ahc* call shares.  Outputs: labels and n_clusters are required, the merge record is nullable as a group.
struct AhcArgs {
  int has_thr = 0; double thr = 0.0;
  const int32_t *minc = nullptr;      // the batched classes: min_clusters per recording (HOST, nullable)
  int32_t minc_wide = 1;              // the wide class: its one min_clusters
  int32_t *labels = nullptr, *n_clusters = nullptr, *merge_a = nullptr, *merge_b = nullptr;
  double *merge_cost = nullptr;
  // the record of the recordings from r0 on, whose first segment is seg0, numbered from 0 (their merge record starts at seg0 - r0)
  AhcArgs from(int64_t r0, int64_t seg0) const {
    AhcArgs s = *this;
    const int64_t m0 = seg0 - r0;
    s.minc = minc ? minc + r0 : nullptr; s.labels = labels + seg0; s.n_clusters = n_clusters + r0;
    s.merge_a = merge_a ? merge_a + m0 : nullptr; s.merge_b = merge_b ? merge_b + m0 : nullptr;
    s.merge_cost = merge_cost ? merge_cost + m0 : nullptr;
    return s;
  }
};
int ahc_plan(plda_handle *h, int64_t N, int32_t *out);
// the argument check of every form (blocks: block_off is checked against the recordings' sizes); pointers are only compared with NULL
int ahc_validate(plda_handle *h, const char *fn, const int64_t *block_off, bool blocks, const int64_t *offsets, int64_t R,
                 const AhcArgs &a);
int ahc_matrix_device(plda_handle *h, const float *dscores, const int64_t *block_off, const int64_t *offsets, int64_t R,
                      const AhcArgs &a);
int score_ahc_device(plda_handle *h, const double *dX, const int64_t *offsets, int64_t R, const AhcArgs &a);
// the wide class: one problem of N <= PLDA_AHC_WIDE_MAX vectors on the whole device (K28)
int ahc_wide_plan(plda_handle *h, int64_t N, int64_t *out);
int ahc_wide_validate(plda_handle *h, const char *fn, int64_t N, int64_t ld, const AhcArgs &a);
int ahc_wide_matrix_device(plda_handle *h, const float *dscores, int64_t N, int64_t ld, const AhcArgs &a);
int score_ahc_wide_device(plda_handle *h, const double *dX, int64_t N, const AhcArgs &a);

// ---- spectral.hip (spectral clustering with auto-tuned pruning; offsets / block_off / p_table / num_spk are HOST arrays) ----
// The arguments every plda_spectral* / plda_score_spectral* call shares.  Outputs: labels and n_clusters are required, the rest nullable.
struct SpectralArgs {
  const int64_t *offsets = nullptr; int64_t R = 0;
  const int32_t *p_table = nullptr; int P = 0, max_spk = 0;
  const int32_t *num_spk = nullptr; int max_iters = 0;
  int32_t *labels = nullptr, *n_clusters = nullptr, *p_used = nullptr, *k_gap = nullptr;
  double *eig = nullptr, *embed = nullptr;
  int32_t *deg2 = nullptr;
};
int spectral_plan(plda_handle *h, int64_t N, int32_t k, int32_t *out);
// the argument check of every form (blocks: block_off is checked against the recordings' sizes); pointers are only compared with NULL
int spectral_validate(plda_handle *h, const char *fn, const int64_t *block_off, bool blocks, const SpectralArgs &a);
int spectral_matrix_device(plda_handle *h, const float *dscores, const int64_t *block_off, const SpectralArgs &a);
int score_spectral_device(plda_handle *h, const double *dX, const SpectralArgs &a);

// ---- dense_pca.hip (recording-dependent PCA before dense scoring; offsets / block_off / minc are HOST arrays) ----
int dense_pca_plan(plda_handle *h, int64_t N, int32_t D, int32_t *out);
// the host-side argument check of every form (blocks: block_off is checked against the recordings' sizes)
int dense_pca_validate(plda_handle *h, const char *fn, const int64_t *offsets, int64_t R, double target, const int64_t *block_off,
                       bool blocks);
int score_dense_pca_device(plda_handle *h, const double *dX, const int64_t *offsets, int64_t R, double target, float *dscores,
                           const int64_t *block_off, int32_t *ddims, double *deig);
int score_dense_pca_ahc_device(plda_handle *h, const double *dX, const int64_t *offsets, int64_t R, double target, const AhcArgs &a);

// ---- der.hip (diarisation error rate: optimal speaker mapping, threshold sweep; offsets / thresholds / minc are HOST arrays) ----
int der_plan(plda_handle *h, int64_t Sr, int64_t Sh, int32_t *out);
int der_jer_plan(plda_handle *h, int64_t Sr, int64_t Sh, int32_t *out);
// the outputs the JER entry points add (K22): jer [.., 2] = {n_ref, jsum}; jmap [R, 64] and spk [R, 64, 3] nullable
struct DerJerOut { long long *jer = nullptr; int *jmap = nullptr; long long *spk = nullptr; };
// the checks of offsets / R and of the sweep's thresholds, Q and min_clusters, shared by every form
int der_validate(plda_handle *h, const char *fn, const int64_t *offsets, int64_t R);
int der_sweep_validate(plda_handle *h, const char *fn, const int64_t *offsets, int64_t R, const double *thresholds, int64_t Q,
                       const int32_t *minc);
// The arguments of every plda_der* call; a field the form does not have stays NULL / 0.  Segment forms: ref, dur; time-based
// forms: the turns, segments and UEM.  sweep: ma, mb, mc, thresholds, Q, minc, n_clusters; otherwise hyp (hyp2), map.
struct DerArgs {
  const int32_t *ref = nullptr, *dur = nullptr;
  const int32_t *tstart = nullptr, *tdur = nullptr, *tspk = nullptr; const int64_t *turn_off = nullptr;
  const int32_t *sstart = nullptr, *sdur = nullptr;
  const int32_t *hyp = nullptr, *hyp2 = nullptr;      // hyp2: the second hypothesis label of every segment (plda_der_timed_ovl, nullable)
  const int64_t *offsets = nullptr; int64_t R = 0;
  const int32_t *ustart = nullptr, *udur = nullptr; const int64_t *uem_off = nullptr;
  int32_t collar = 0, flags = 0;
  const int32_t *ma = nullptr, *mb = nullptr; const double *mc = nullptr;
  const double *thresholds = nullptr; int64_t Q = 0; const int32_t *minc = nullptr;
  int64_t *counts = nullptr; int32_t *n_clusters = nullptr, *map = nullptr;
  bool jer_form = false;              // plda_der*_jer*: jo.jer is required, jo.jmap and jo.spk are nullable
  DerJerOut jo;
};
// the host-side argument check of the segment forms (pointers are only compared with NULL; the host forms run it before they
// allocate or upload) and their device form (jer_form: the sum of a recording's durations is at most 2^30)
int der_seg_validate(plda_handle *h, const char *fn, const DerArgs &a, bool sweep);
int der_seg_device(plda_handle *h, const char *fn, const DerArgs &a, bool sweep);

// ---- der_time.hip (time-based DER: overlapped reference speech, collar, UEM; every *_off array is a HOST array) ----
// one recording's scored atoms, as der_atoms_kernel leaves them and der.hip's solve reads them
struct DerTimedRec { long long aoff; int natoms, sh; unsigned long long umask; };   // first atom; atoms; distinct hyp labels; union of masks
struct DerTimedDev {
  const DerTimedRec *recs; const int *ticks; const int *seg; const unsigned long long *mask;
  const int *hyp2;      // plda_der_timed_ovl: the second label of every segment; NULL: one label per segment
};
int der_timed_plan(plda_handle *h, int64_t n_turns, int64_t n_seg, int64_t n_uem, int32_t collar, int32_t *out);
// the host-side argument check (pointers are only compared with NULL; the host forms run it before they allocate or upload)
int der_timed_validate(plda_handle *h, const char *fn, const DerArgs &a, bool sweep);
int der_timed_device(plda_handle *h, const char *fn, const DerArgs &a, bool sweep);
// der.hip: the solves behind the atoms (against a.hyp, or the sweep of the merge record); recs is the host copy of td.recs
int der_timed_solve(plda_handle *h, const char *fn, const DerTimedRec *recs, const DerTimedDev &td, const DerArgs &a, bool sweep);

// ---- vbx.hip (VBx resegmentation: a batched Bayesian HMM on PLDA vectors; offsets / gamma_off / pi_off are HOST arrays) ----
int vbx_plan(plda_handle *h, int64_t T, int64_t S, int64_t D, int32_t *out);
// the argument check of both forms; pointers are only compared with NULL
int vbx_validate(plda_handle *h, const char *fn, int64_t D, const int64_t *offsets, int64_t R, double Fa, double Fb, double loop_prob,
                 int64_t max_iters, const void *labels, const void *n_clusters, const void *gamma, const int64_t *gamma_off,
                 const void *pi, const int64_t *pi_off);
int vbx_device(plda_handle *h, const double *dY, int64_t D, const double *dPhi, const int32_t *dlabels_in, const int64_t *offsets,
               int64_t R, double Fa, double Fb, double loop_prob, double init_smoothing, int64_t max_iters, double epsilon,
               int32_t *dlabels, int32_t *dn_clusters, double *dgamma, const int64_t *gamma_off, double *dpi, const int64_t *pi_off,
               double *delbo, int32_t *diters, int32_t *dlabels2 = nullptr, double *dpost2 = nullptr);
int project_rows_device(plda_handle *h, const double *dX, int64_t R, int Din, double *dout);

// ---- frontend.hip ----
int htk_frames_device(plda_handle *h, const void *dblob, const int64_t *dfile_off, const int64_t *dframe_off,
                      int64_t U, int64_t T, int samplesize, int frm_ext, float *dout);
int dvector_pool_device(plda_handle *h, const void *dframes, int dtype, int64_t T, int D,
                        const int64_t *doffsets, int64_t U, int method, int l2norm, double *dout);

// ---- fit.hip ----
int group_means_device(plda_handle *h, const double *dX, int64_t N, int D, const uint64_t *ddense,
                       int64_t Ku, double *dmeans, int32_t *dcounts32);
int lda_fit_device(plda_handle *h, const double *dX, int64_t N, int D, const uint64_t *dlabels, int64_t K,
                   int solver, const double *priors_host);
int lda_predict_device(plda_handle *h, const double *dX, int64_t N, int mode, double *dout);
int lda_transform_device(plda_handle *h, const double *dX, int64_t N, int ncomp, double *dout);
int fit_stats_device(plda_handle *h, const double *dX, int64_t N, int D, const uint64_t *dlabels, int64_t K, bool defer_check = false);
int fit_em_device(plda_handle *h, int64_t K, int D, int iters);
int fit_device(plda_handle *h, const double *dX, int64_t N, int D, const uint64_t *dlabels,
               int64_t K, int iters);
int compute_offset_device(plda_handle *h);   // offset = -transform . mean (Plda::ComputeDerivedVars)
int group_by_label_device(plda_handle *h, const uint64_t *dlabels, int64_t N, uint32_t **perm_out, int **offsets_out,
                          uint64_t **uniq_out, int64_t *G_out);
int group_centroids_device(plda_handle *h, const double *dX, int64_t N, int D, const uint32_t *perm, const int *offsets,
                           int64_t G, double *dmeans, int32_t *dcounts32);

// ---- score.hip ----
// the packed operands of one trials GEMM (score.hip: prepare_operands fills it)
struct TrialOperands {
  int64_t Mpad, Npad;
  int KQ, Kg;   // padded GEMM depth (multiple of 8) and its k-quad count
  int Kg_alg;   // algorithmic depth: Dout (uniform n, cosine), Dout + G - 1 (mixed n, bucketed) or 2 Dout (mixed n, depth-2D form)
  int kind;     // 0 uniform count, 1 mixed counts in the depth-2D form, 2 mixed counts bucketed by distinct count
  bool mixed;   // kind == 1
};
// Rows per wave of the one-pass prep kernels: 4 while a side has at most 32 768 padded rows, 16 beyond
// (PLDA_PREP_VARIANT=3 / 2: 4 / 16 forced).
inline bool prep_few_rows(const plda_handle *h, int64_t rpad) { return h->prep_variant == 3 || (h->prep_variant != 2 && rpad <= 32768); }
const GemmArm *gemm_arm_lookup(int variant);   // the row of PLDA_GEMM_VARIANT=variant; nullptr: no such arm
// cs: the distinct enrol counts of the caller's whole call (mixed counts; nullptr: found from dn on the device)
int score_matrix_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M,
                        const double *dV, int64_t Nt, const double *dzmean, const double *dzstd,
                        float *dout, int64_t ld, bool reuse_packed_B = false, const CountSet *cs = nullptr);
void score_count_set_host(const int32_t *n, int64_t M, CountSet *cs);
// M, cs: the enrol set's size and its distinct counts (long lists run on per-count tables; M = 0: the list is short)
int score_pairs_device(plda_handle *h, const double *dU, const int32_t *dn, const double *dV,
                       const int64_t *de, const int64_t *dt, int64_t P, const double *dzmean,
                       const double *dzstd, double *dout, int64_t M = 0, const CountSet *cs = nullptr);
int znorm_stats_device(plda_handle *h, const double *dbkg, int64_t Nb, int num_examples, int Din,
                       const double *dmodels, int64_t M, double *dmean, double *dstd);
int pairs_validate_device(plda_handle *h, const int64_t *de, const int64_t *dt, int64_t P, int64_t M, int64_t Nt, long long *bad);
int score_count_set_device(plda_handle *h, const int32_t *dn, int64_t M, CountSet *cs);
int score_prepare_device(plda_handle *h, const double *dV, int64_t Nt, int kind, int n_uniform, const CountSet *cs);
// norm()'s model pass: per row x, out_mean = sum_c x_c (m_c - q_c x_c / 2) + *mD, out_std = sqrt(max(x^T C x + lin . x + *crr, 0)); D <= 208
int quadform_rows_device(plda_handle *h, const double *dX, int64_t R, int D, const double *C, int ldc, const double *lin,
                         const double *m, const double *q, const double *mD, const double *crr, double *out_mean,
                         double *out_std, bool *used);
int transform_rows_device(plda_handle *h, const double *dX, int64_t R, int Din,
                          const int32_t *dn, int n_uniform, double *dout);
// what transform_rows_device runs for R rows on the installed model (plda_transform_plan reports it): arm 0 = the one-pass kernel
// (cls 0 .. 4: Dout <= 128 / 208 / 256 / 384 / 512; rows [0, main_rows) in blocks of main_block rows, then tail_rows rows in
// blocks of tail_block rows, 0 without a tail), arm 1 = GEMM + length-norm pass (cls -1, every row in main_rows)
struct TfPlan { int arm, cls, main_block, tail_block; int64_t main_rows, tail_rows; };
TfPlan transform_plan(const plda_handle *h, int64_t R);

// ---- cosine.hip (the cosine back-end: the operands of the trials GEMM from length-normalised rows, and trial lists) ----
// fills the buffers prepare_operands reserved (s_Apk / s_Bpk, s_rbias, s_rscale, s_rpair, s_cbias, s_cpair) for the sides asked for
int cosine_prepare_operands(plda_handle *h, const double *dU, int64_t M, const double *dV, int64_t Nt, const double *dzmean,
                            const double *dzstd, const TrialOperands &op, bool doA, bool doB);
int cosine_pairs_device(plda_handle *h, const double *dU, const double *dV, const int64_t *de, const int64_t *dt, int64_t P,
                        const double *dzmean, const double *dzstd, double *dout);
// one trial on the host, the expression of cosine_pairs_kernel
double cosine_one_host(const double *u, const double *v, int D, bool has_z, double zmean, double zstd);

// ---- snorm.hip (adaptive symmetric score normalisation: top-K cohort statistics, the two-sided map) ----
// cs: as score_matrix_device (the distinct counts of the caller's whole call; nullptr: found here)
int cohort_stats_device(plda_handle *h, const double *dX, const int32_t *dn, int n_uniform, int64_t R, const double *dC,
                        int64_t Nc, int64_t top_k, double *dmean, double *dstd, const CountSet *cs = nullptr);
int score_matrix_snorm_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV,
                              int64_t Nt, const double *demean, const double *destd, const double *dtmean, const double *dtstd,
                              float *dout, int64_t ld, const CountSet *cs = nullptr, bool reuse_packed_B = false);
// rows of one slab of fp32 scores with ld floats per row (the height rule of every walk over h->sn_slab)
int64_t sn_slab_rows(const plda_handle *h, int64_t total_rows, int64_t ld);

// ---- topn.hip (top-N selection with indices: per row, axis 0, or per column, axis 1, of a trials matrix)
int topn_matrix_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, int axis, int64_t top_n,
                       float *dout_scores, int64_t *dout_index);
int score_topn_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV, int64_t Nt,
                      const double *dzmean, const double *dzstd, const double *demean, const double *destd, const double *dtmean,
                      const double *dtstd, int axis, int64_t top_n, float *dout_scores, int64_t *dout_index,
                      const CountSet *cs = nullptr);

// ---- comm.hip (the communicator of a handle and the row-sharded forms over it)
int comm_init(plda_handle *h, int nranks, int rank, const void *uid);
int comm_init_custom(plda_handle *h, int nranks, int rank, const plda_collectives *t);
int comm_init_host(plda_handle *h, int nranks, int rank, const plda_host_collectives *t);
int comm_init_peer(plda_handle *h, int nranks, int rank, const plda_host_collectives *t);
int comm_destroy(plda_handle *h);
int comm_check(plda_handle *h);
int comm_describe(plda_handle *h, std::string &js);
int score_matrix_sharded_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M,
                                const double *dV, int64_t Nt, const double *dzmean, const double *dzstd, float *dlocal,
                                int64_t ld_local, float *dfull, int64_t ld_full, int64_t block_rows, int gather);
int znorm_stats_sharded_device(plda_handle *h, const double *dbkg, int64_t Nb, int num_examples, int Din,
                               const double *dmodels, int64_t M, double *dmean, double *dstd);
int fit_sharded_device(plda_handle *h, const double *dX, int64_t N, int D, const uint64_t *dlabels, int64_t K, int iters);
int cohort_stats_sharded_device(plda_handle *h, const double *dX, const int32_t *dn, int n_uniform, int64_t Rows, const double *dC,
                                int64_t Nc, int64_t top_k, double *dmean, double *dstd);

// (the labelled-trials source of the EER / DET / calibration / minDCF reductions and their score key: trial_source.hpp)

#ifdef __HIPCC__
// fp64 wave-wide sum through DPP: quad butterflies, then half-row and row mirrors (every
// lane of a 16-lane row then holds the row sum), then four readlanes.  ~6x shorter
// dependency chain than __shfl_xor, which lowers to ds_bpermute for 64-bit values.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x) {
  int lo = __double2loint(x), hi = __double2hiint(x);
  lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double x, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l),
                          __builtin_amdgcn_readlane(__double2loint(x), l));
}
__device__ __forceinline__ double wave_sum_f64(double x) {
  x += dpp_f64<0xB1>(x);    // quad_perm [1,0,3,2]
  x += dpp_f64<0x4E>(x);    // quad_perm [2,3,0,1]
  x += dpp_f64<0x141>(x);   // row_half_mirror
  x += dpp_f64<0x140>(x);   // row_mirror
  return (readlane_f64(x, 0) + readlane_f64(x, 16)) + (readlane_f64(x, 32) + readlane_f64(x, 48));
}

// ---- the clustering family: the count of non-finite scores (ahc.hip, spectral.hip) ----
__device__ __forceinline__ bool cluster_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }
// the off-diagonal elements of the n x n block at blk (row stride ld) that are not finite, added to *bad; the workgroups
// blockIdx.x of 256 threads share the block
__device__ __forceinline__ void cluster_count_block(const float *__restrict__ blk, long long n, long long ld, unsigned long long *bad) {
  const long long total = n * n;
  unsigned cnt = 0;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long i = e / n, j = e - i * n;
    if (i != j && !cluster_finite(blk[i * ld + j])) ++cnt;
  }
  if (cnt) atomicAdd(bad, (unsigned long long)cnt);   // rare: one integer atomic per lane that met one
}
// grid (pieces, recordings): the blocks of a launch table (Rec: boff, n), each dense
template <typename Rec>
__global__ __launch_bounds__(256) void cluster_count_kernel(const float *__restrict__ S, const Rec *__restrict__ tab, unsigned long long *bad) {
  const long long n = tab[blockIdx.y].n;
  cluster_count_block(S + tab[blockIdx.y].boff, n, n, bad);
}
// enqueues the count over the cnt recordings of a table (tab: its host copy, dtab: the uploaded one), 32768 recordings a launch
template <typename Rec>
int cluster_count_enqueue(plda_handle *h, const float *dscores, const Rec *tab, int64_t cnt, const Rec *dtab, unsigned long long *dbad) {
  for (int64_t c0 = 0; c0 < cnt; c0 += 32768) {
    const int64_t c = std::min<int64_t>(32768, cnt - c0);
    int nmax = 0;
    for (int64_t q = c0; q < c0 + c; ++q) nmax = std::max(nmax, tab[q].n);
    const int64_t pieces = std::max<int64_t>(1, std::min<int64_t>(ceil_div((int64_t)nmax * nmax, 256 * 16), 1024));
    cluster_count_kernel<Rec><<<dim3((unsigned)pieces, (unsigned)c), 256, 0, h->stream>>>(dscores, dtab + c0, dbad);
    PLDA_LAUNCH_CHECK(h);
  }
  return PLDA_OK;
}
#endif

}  // namespace plda
