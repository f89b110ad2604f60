/*
 * include/plda_hip.h -- C ABI of libplda_hip.so, the MI355X (gfx950) PLDA engine.
 *
 * This is the drop-in boundary for the reference's native object
 * `libplda.MPlda` (RicherMans/PLDA src/pldamodule.cpp): every entry point names
 * the reference interface it replaces.  Plain pointers and sizes only; no
 * CPython, NumPy or torch types cross this boundary.  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *  - every function returns an int status: PLDA_OK (0) or a negative PLDA_E_*;
 *    the text of the last failure on a handle is plda_last_error(h)
 *    (plda_last_error(NULL) = last failure of plda_create on this thread).
 *    Nothing aborts and nothing throws across the ABI (the reference lets Kaldi
 *    assertions abort the process, pldamodule.cpp has no try/catch).
 *  - matrices are row-major, C-contiguous, fp64 (the reference reads every
 *    array as f64: pldamodule.cpp:72, kaldi-utils.hpp:99-111); labels are
 *    uint64 (npy_long read as 8 bytes, pldamodule.cpp:74).
 *  - "host" entry points borrow caller memory for the duration of the call and
 *    write only caller-allocated outputs (ownership: the reference copies its
 *    inputs immediately, kaldi-utils.hpp:99-122).  "_dev" entry points take
 *    pointers into this GPU's HBM and enqueue on the handle's stream without
 *    synchronising.
 *  - one handle = one GPU + one HIP stream.  Every entry point takes the handle's mutex, so calls on
 *    one handle from several threads are safe and serialised (the reference holds the GIL for the
 *    whole call, pldamodule.cpp has no threads); use one handle per thread for concurrency.
 *    plda_destroy must not race with other calls on the same handle.
 *  - there is NO CPU fallback: without a usable gfx950 device plda_create fails.
 *  - feature dimension: 1 ... 2048 (plda_fit*, plda_lda_fit*, plda_sym_eig return PLDA_E_INVAL above).  The
 *    reference has no cap (its own tests stop at 1024, tests/pldatest.py:55); the engine's is the direct eigensolver's
 *    (one workgroup per 8 rows, all 256 CUs at 2048).  Above 1024 ONLY that solver exists: it needs ceil(D/8) co-resident
 *    workgroups, so on a device that exposes fewer CUs (CU masking, a partitioned GPU) a fit / GetOutput / plda_sym_eig
 *    with D in (1024, 2048] returns PLDA_E_INVAL with a message that says so, and plda_sym_eig(method = 1, the block
 *    Jacobi solver) is rejected above 1024 at the boundary.  INTEGRATION.md, "Limits".
 */
#ifndef PLDA_HIP_H_
#define PLDA_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLDA_OK 0
#define PLDA_E_INVAL (-1)     /* bad argument (NULL, non-positive size, dim mismatch) */
#define PLDA_E_ONE_SPEAKER (-2) /* fit with a single speaker (pldamodule.cpp:83-86) */
#define PLDA_E_NUMERIC (-3)   /* not positive definite / eigensolver did not converge */
#define PLDA_E_NOT_FITTED (-4)
#define PLDA_E_HIP (-5)       /* HIP runtime failure (message has the hipError string) */
#define PLDA_E_LABELS (-6)    /* fit labels not dense 0..K-1 (pldamodule.cpp:88-92 indexes by value) */
#define PLDA_E_CAPACITY (-7)  /* caller output too small */

typedef struct plda_handle plda_handle;

/* ---- lifecycle: replaces Plda_new / MPLDA_dealloc (pldamodule.cpp:297-316) and
 *      the module init initlibplda (pldamodule.cpp:371-384) ---- */
int plda_create(int device, plda_handle **out);
int plda_destroy(plda_handle *h);
/* A long-lived handle.  A handle owns growable device scratch and caches that survive between calls, and the law that
 * governs them is part of its contract: after ANY sequence of earlier successful or refused calls on a handle, a call's
 * outputs equal, bit for bit, the outputs of the same call on a fresh handle that holds the same model (the model a fresh
 * handle gets from plda_get_model's arrays through plda_set_model).  Scratch an earlier, larger call filled is never read
 * before it is written; a cache is keyed on everything it was computed from; a refused call leaves nothing a later call can
 * see.  tests/test_gpu_handle_history.py holds the entry points to it, the bf16x3 contraction and the one-wave-per-SIMD
 * kernel's tile tables included (tests/history_cases.py lists, per device buffer of the handle, what reaches it).
 * What persists BY DESIGN, and is therefore state a caller sets and reads, not history:
 *   - the PLDA model (plda_fit*, plda_set_model, plda_truncate, plda_smooth, plda_adapt_update, plda_blend_model replace it;
 *     each bumps the model's epoch, on which every model-derived cache is keyed) and the statistics of the last fit
 *     (plda_fit_get_stats*, plda_fit_plan, plda_fit_timings);
 *   - the LDA model (plda_lda_*) and the embedding chain (plda_embed_set / _fit / _clear);
 *   - the adaptation record between plda_adapt_reset and plda_adapt_update (refused under another model epoch);
 *   - a prepared test side (plda_score_prepare*_dev) until plda_score_unprepare, a call that repacks the test side, or a new
 *     model; it is reused only while pointer, size, model epoch, count kind and content fingerprint match;
 *   - the stream (plda_set_stream), the communicator (plda_comm_*), the profile and trace switches and their records;
 *   - the dispatch records of the last call: plda_score_last_kernel / _shape, plda_linalg_last_kernels, plda_fit_plan.
 * What persists as an optimisation and never changes a result's bits: the scoring coefficient tables (uniform or bucketed,
 * one buffer), K4's padded transform, the one-trial host coefficients, the dense-PCA covariances of the model, the tile
 * tables of the one-wave-per-SIMD trials GEMM, the captured Jacobi sweep graph, and the eigenvector warm start of the
 * simultaneous diagonalisation (dropped at the start of every fit, so that fits are bit-reproducible).  Scratch grows and
 * is given back by plda_destroy only. */
const char *plda_last_error(const plda_handle *h);
int plda_abi_version(void);
/* bit 0: built with -DPLDA_DIAG=1 (libplda_hip_diag.so: + the measurement arms of the trials GEMM, some of which return
 * garbage scores; selected by PLDA_GEMM_VARIANT).  The product library returns 0 and plda_create refuses those variants; both
 * libraries refuse a PLDA_GEMM_VARIANT that names no arm (profiles/SWITCHES.md lists the arms). */
int plda_build_flags(void);
/* bytes of device memory the library's buffers hold right now, over every handle of the process (the device scratch and
 * model copies of the handles, the temporaries of calls in flight; not the one uncached flag page of the peer transport,
 * plda_comm_init_peer).  With PLDA_SCRATCH_POISON=1 in the environment at
 * plda_create (tests only), every later device allocation of the library is 64 KiB longer than asked for and filled with
 * 0xFF bytes (NaN as a float) before its first use; an allocation that would need the fill while the handle's stream is
 * being captured fails with PLDA_E_HIP. */
int64_t plda_device_bytes_held(void);
/* the high-water mark of that counter since the last call with reset != 0 (process-wide, like the counter; a reset sets the
 * mark to what is held at that moment).  What a call needed at its worst: read, call, read again. */
int64_t plda_device_bytes_peak(int32_t reset);
/* enqueue on exactly this hipStream_t (e.g. torch's current stream; NULL is HIP's default
 * stream, with its implicit-synchronisation rules); plda_reset_stream goes back to the
 * handle's own non-blocking stream */
int plda_set_stream(plda_handle *h, void *hip_stream);
int plda_reset_stream(plda_handle *h);
int plda_synchronize(plda_handle *h);

/* ---- fit: replaces MPlda_fit (pldamodule.cpp:42-109) ----
 * labels must be dense 0..K-1 (the Python shim compacts arbitrary unsigned
 * labels first).  Runs: label counting-sort, per-speaker centroids,
 * AddSamples(1/n_k) scatter (pldamodule.cpp:94-98), `iters` EM iterations
 * (Kaldi PldaEstimator::Estimate, :102-106) and GetOutput, all on the GPU in fp64. */
int plda_fit(plda_handle *h, const double *X, int64_t N, int32_t D /* <= 2048 */,
             const uint64_t *labels, int32_t iters);
int plda_fit_dev(plda_handle *h, const double *dX, int64_t N, int32_t D,
                 const uint64_t *dlabels, int64_t K, int32_t iters);
/* The same fit in its two halves, for fitting on several GPUs: every
 * quantity AddSamples accumulates (pldamodule.cpp:94-98) is a sum over speakers, so each rank
 * runs the statistics pass on the rows of ITS speakers (local dense labels 0..K-1),
 *   plda_fit_stats_dev      -> means[K,D], counts[K], offset scatter[D,D] of those speakers,
 *   plda_fit_get_stats_dev  copies them to caller-owned DEVICE buffers (any may be NULL),
 * the ranks all-reduce the scatter and all-gather means/counts, and every rank then runs
 *   plda_fit_em_dev         EM + GetOutput (pldamodule.cpp:102-106) on the merged statistics.
 * plda_fit_dev == plda_fit_stats_dev followed by plda_fit_em_dev on the handle's own buffers. */
int plda_fit_stats_dev(plda_handle *h, const double *dX, int64_t N, int32_t D,
                       const uint64_t *dlabels, int64_t K);
int plda_fit_get_stats_dev(plda_handle *h, double *dmeans, int64_t *dcounts, double *dscatter);
int plda_fit_em_dev(plda_handle *h, const double *dmeans, const int64_t *dcounts, int64_t K,
                    const double *dscatter, int32_t D, int32_t iters);
/* timings of the last fit, milliseconds: [0] statistics pass (sort+centroid+scatter): host wall clock of
 * plda_fit_stats*, its span on the stream inside plda_fit (which does not synchronise between the two halves);
 * [1] EM loop (all iterations): its span on the stream between two events (planning of the count groups
 * on the host included); [2] GetOutput: the rest of the call's wall clock behind the EM (its kernels, the
 * export of the model and status words to the host mirror, the one synchronisation); [3] = iterations run.
 * [1] + [2] = wall clock of plda_fit_em_dev; [0] + [1] + [2] = wall clock of plda_fit. */
int plda_fit_timings(plda_handle *h, double out_ms[4]);
/* how the EM of the last fit ran (pldamodule.cpp:102-105 is one loop over the classes; here the classes are grouped by
 * their utterance count, the reason the reference sorts them, pldamodule.cpp:94-100): out[0] = number of distinct counts G
 * (0: not grouped), out[1] = 0 EM in the simultaneously-diagonalised basis, 1 grouped on per-group second moments
 * (few groups of many classes), 2 grouped on the class means (many groups). */
int plda_fit_plan(plda_handle *h, int32_t out[2]);
/* staged access to the fit internals (parity tests of SURVEY.md rows a3-a7):
 * any pointer may be NULL.  means[K*D] in label order, counts[K], scatter[D*D],
 * sum[D], W[D*D], B[D*D] (final within/between covariances before GetOutput). */
int plda_fit_get_stats(plda_handle *h, double *means, int64_t *counts, double *scatter,
                       double *sum, double *W, double *B);
int plda_fit_num_classes(plda_handle *h, int64_t *K);

/* ---- model state: the Kaldi `Plda` held at pldamodule.cpp:29 ----
 * transform is [Dout, Din] row-major; after fit Dout == Din == D. */
int plda_get_dims(plda_handle *h, int32_t *Dout, int32_t *Din);
int plda_get_model(plda_handle *h, double *mean /*[Din]*/, double *transform /*[Dout*Din]*/,
                   double *psi /*[Dout]*/, double *offset /*[Dout]*/);
int plda_set_model(plda_handle *h, int32_t Dout, int32_t Din, const double *mean,
                   const double *transform, const double *psi);
/* build extension ("targetdim"): keep the first
 * `targetdim` rows of transform / psi (largest between-class variance). */
int plda_truncate(plda_handle *h, int32_t targetdim);
/* replaces Plda::SmoothWithinClassCovariance reached at pldamodule.cpp:158-160 */
int plda_smooth(plda_handle *h, double factor);

/* ---- transform: replaces Mplda_transform (pldamodule.cpp:111-194) ----
 * groups rows by label (any u64 values), averages, applies
 * Plda::TransformIvector(mean, n) (:171) incl. length normalisation.  Outputs
 * ascending by label (std::map order, :164).  *Ku: in = capacity (rows of the
 * out arrays), out = number of groups. */
int plda_transform_groups(plda_handle *h, const double *X, int64_t N, int32_t Din,
                          const uint64_t *labels, uint64_t *out_labels,
                          int64_t *out_counts, double *out_vecs /*[Ku*Dout]*/,
                          int64_t *Ku);
/* the same on HBM-resident rows and labels; outputs (device): out_labels[Ku] u64, out_counts[Ku] int32,
 * out_vecs[Ku, Dout].  Grouping is a device radix sort over as many 8-bit digits as the largest label has. */
int plda_transform_groups_dev(plda_handle *h, const double *dX, int64_t N, int32_t Din,
                              const uint64_t *dlabels, uint64_t *dout_labels, int32_t *dout_counts,
                              double *dout_vecs, int64_t *Ku);
/* batched Plda::TransformIvector on R already-averaged rows; num_examples[R]
 * (int32) or, if NULL, `n_uniform` for every row.
 * DEFINITION.  t = T (x - mean), w_d = 1 / (psi_d + 1/n), s = sum_d t_d^2 w_d, out = sqrt(Dout / s) t, per row, in fp64.  A row's
 * result depends on that row and its count alone: its bits are the same at every position of a launch and with any neighbours.
 * EDGES, each pinned by tests/test_gpu_transform_edges.py:
 *   - t = 0 exactly (x = mean = 0, for instance): the row has no direction and comes back all NaN.  A row EQUAL to a non-zero
 *     mean gives a t of rounding residue; its result is unspecified (finite or NaN), its neighbours are untouched.
 *   - a row with a NaN or an Inf element comes back all NaN (given that no element of T is exactly zero); every other row is
 *     bit-identical to the call without it.
 *   - counts <= 0 (Kaldi asserts num_examples > 0).  n_uniform <= 0 without an array: PLDA_E_INVAL.  plda_transform_rows, whose
 *     counts are in host memory, counts such rows before any device work: PLDA_E_INVAL with their number and the first such row
 *     in plda_last_error, nothing is written, the handle keeps working.  plda_transform_rows_dev does not read device memory
 *     on the host: a row whose count is <= 0 comes back all NaN, its neighbours are untouched.
 *   - scale: the sum s is formed from t_d^2 in fp64, so rows with |t| between about 1e-150 and 1e+150 are normalised like any
 *     other (1e-100 and 1e+100 are tested beside ordinary rows); beyond that s leaves the fp64 range and the row is unspecified.
 *   - an offset mean.  The product is evaluated in the reference's own form T x + (-T mean), not as T (x - mean): with
 *     u = 2^-53 an element of t carries an absolute error of up to (Din + 2) u sum_k |T_ok| (|x_k| + |mean_k|), i.e. the
 *     RELATIVE error of the output grows linearly with |mean| / |x - mean|: the bound is 6e-10 (Dout = 208) to 2e-9 (512) of
 *     |out| at |mean| = 1e3 spreads and 6e-7 to 2e-6 at 1e6 spreads; the measured deviation is below a hundredth of that
 *     (profiles/transform_parity.json, per case).
 *     Callers whose data sit far from the origin centre them first (plda_embed_set's input mean).
 * plda_transform_plan: what the two entry points run for R rows on the installed model, without touching the device --
 *   out[0] = the arm: 0 the one-pass kernel, 1 a GEMM and a length-norm pass (Dout > 512, or PLDA_TRANSFORM_VARIANT=1);
 *   out[1] = the dimension class of arm 0: 0 .. 4 for Dout <= 128 / 208 / 256 / 384 / 512 (-1 on arm 1);
 *   out[2], out[3] = the rows of the main launch (a whole number of rounds of one block per compute unit; every row on arm 1)
 *   and the rows of one of its blocks (128 for classes 0 .. 2, 64 for classes 3 and 4; on arm 1 the 4 rows of a length-norm block);
 *   out[4], out[5] = the rows of the tail launch and of one of its blocks (16, 32, 64 or the main block's rows; 0, 0 without a tail);
 *   out[6] = the compute units the split was made for; out[7] = 0.  PLDA_E_NOT_FITTED without a model, PLDA_E_INVAL for R < 0. */
int plda_transform_rows(plda_handle *h, const double *Xbar, int64_t R, int32_t Din,
                        const int32_t *num_examples, int32_t n_uniform, double *out);
int plda_transform_rows_dev(plda_handle *h, const double *dXbar, int64_t R, int32_t Din,
                            const int32_t *dnum_examples, int32_t n_uniform, double *dout);
int plda_transform_plan(plda_handle *h, int64_t R, int64_t out[8]);

/* ---- score: replaces MPlda_score (pldamodule.cpp:258-277) ----
 * Trial list: P pairs (enrol row e_idx[p] of U, test row t_idx[p] of V), each
 * Plda::LogLikelihoodRatio(U[e], n[e], V[t]) (:266) in fp64, then the optional
 * z-norm (s - zmean[e]) / zstd[e] (:269-273) where zmean/zstd are non-NULL and
 * zstd[e] != 0.  plda.score() is the P == 1 case.
 * Lists of >= 16 384 trials (a trials file: scoring/scorePLDA.py:299-321) run on per-count tables -- the terms of the LLR that
 * depend on (n[e], dimension) only are tabulated per distinct count -- in fp64, equal to the per-element form to 1e-11; their
 * indices are checked on the device.  An index outside [0, M) x [0, Nt) is PLDA_E_INVAL naming the first such trial. */
int plda_score_pairs(plda_handle *h, const double *U, const int32_t *n_enrol, int64_t M,
                     const double *V, int64_t Nt, const int64_t *e_idx,
                     const int64_t *t_idx, int64_t P, const double *zmean,
                     const double *zstd, double *out);
/* ONE trial, evaluated on the host: plda.score() (pldamodule.cpp:258-277) is one LogLikelihoodRatio (:266) per
 * Python call, i.e. 2 D numbers and ~5 D flop -- a GPU launch + synchronisation costs ten times that, so the scalar
 * call is served from the handle's host mirror of psi (fp64, per-count terms cached; the library's own code, no
 * oracle).  u, v: already-transformed vectors [Dout]; has_z != 0 applies (s - zmean) / zstd where zstd != 0 (:269-273).
 * Batches belong on plda_score_pairs / plda_score_matrix. */
int plda_score_one(plda_handle *h, const double *u, int32_t n_enrol, const double *v, int32_t has_z,
                   double zmean, double zstd, double *out);
/* Dense trials matrix out[i*ld_out + j] = LLR(U[i], n[i], V[j]) for the M x Nt
 * block (the nested Python loop of scoring/scorePLDA.py:302-318 and
 * tests/pldatest.py:29-33 as one launch): fp64 bias terms + fp32 MFMA GEMM,
 * fp32 scores.  n_enrol NULL => every row uses n_uniform (GEMM depth Dout).
 * Otherwise the rows are bucketed by their G DISTINCT counts and the depth is
 * Dout + G - 1 (one column-bias vector per distinct count, carried as extra
 * contraction columns; C4's n in 1..5 at D = 256: 264 instead of 512); counts
 * above 4095, more than 64 distinct ones or G - 1 > Dout / 2 take the depth-2*Dout
 * form [A1 | A2] x [V | V*V].  plda_score_matrix finds the distinct counts on the
 * host; the _dev entry points find them with one small device pass and ONE wait
 * for the handle's stream per call (the host must know G to size the operands);
 * uniform calls and calls that reuse a prepared test side of the depth-2*Dout
 * form enqueue only.  zmean/zstd as above (nullable). */
int plda_score_matrix(plda_handle *h, const double *U, const int32_t *n_enrol,
                      int32_t n_uniform, int64_t M, const double *V, int64_t Nt,
                      const double *zmean, const double *zstd, float *out,
                      int64_t ld_out);
int plda_score_matrix_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol,
                          int32_t n_uniform, int64_t M, const double *dV, int64_t Nt,
                          const double *dzmean, const double *dzstd, float *dout,
                          int64_t ld_out);
/* One test set against many enrol sets (the reference's callers score every enrol model against the same test
 * utterances, scoring/scorePLDA.py:302-318): plda_score_prepare_dev packs the test side once -- fp64 -> k-quad packed
 * fp32 (+ V*V when enrol counts differ: mixed_counts != 0; else the column biases for n_uniform) -- and later
 * plda_score_matrix_dev / _sharded_dev calls with the SAME dV, Nt, model and kind of enrol counts skip that work (C3:
 * 2.1 of 72 ms per call).  The cache is keyed on (dV, Nt, model epoch, kind of counts) AND guarded by a content
 * fingerprint of 64 rows spread over the set (first and last included), taken at prepare time: a reusing call recomputes
 * it (one small kernel + a stream synchronisation, ~30 us; once per call, not per block of a sharded call) and, when the
 * rows behind the pointer have changed -- an in-place update, or an allocator that handed the address to another tensor
 * -- treats the cache as MISSED: the rows are packed again and the call succeeds (round 5; rounds 3-4 returned
 * PLDA_E_INVAL here, which failed legitimate calls whose new tensor sat at a recycled address).  Rows outside the sample
 * are still the caller's promise.  A different test side, a model change (fit, set_model, truncate, smooth) or
 * plda_score_unprepare end the reuse silently.  Test sides whose packed form would reach 4 GiB are refused (such calls
 * are scored in column blocks, each packed per call).
 * mixed_counts != 0 prepares the depth-2*Dout form, which later mixed-count calls then USE (no count pass, no wait);
 * plda_score_prepare_counts_dev prepares the faster bucketed form for the distinct enrol counts the later calls will
 * bring (host array `counts`, any order, duplicates allowed): calls whose counts are a subset reuse it, others repack. */
int plda_score_prepare_dev(plda_handle *h, const double *dV, int64_t Nt, int32_t mixed_counts, int32_t n_uniform);
int plda_score_prepare_counts_dev(plda_handle *h, const double *dV, int64_t Nt, const int32_t *counts, int32_t num_counts);
int plda_score_unprepare(plda_handle *h);
/* Kernel timing for roofline accounting: when enabled, every trials-GEMM launch is
 * bracketed by HIP events recorded on the stream it is launched on; plda_profile_read
 * synchronises and returns the accumulated GEMM milliseconds, launches, and the
 * algorithmic flop (2 * gemm_k per trial) since the last reset. */
int plda_profile_enable(plda_handle *h, int32_t on);
int plda_profile_read(plda_handle *h, double *gemm_ms, int64_t *launches, double *gemm_flop,
                      int32_t reset);
/* Diagnostic (PLDA_HIP tracing knob; diagnostic build only): with a timeline arm in the environment at
 * plda_create (PLDA_GEMM_VARIANT=31: the two-waves 256 x 256 kernel, 41: the one-wave one), the trials GEMM runs an
 * instrumented instantiation whose workgroup 0 stamps the shader clock per wave at every stage barrier (arrive, leave) and around every tile epilogue.
 * out[tile < 8][stage < 16][wave < 8][8] = {barrier arrive, leave, start of steps 1..3 of the stage (0 if
 * absent), -, epilogue start, epilogue end (the last two in stage slot 15)}. */
int plda_profile_timeline(plda_handle *h, uint64_t *out, int64_t cap_words);

/* Per-stage timing (PLDA_HIP_TRACE): named spans bracketed by HIP events on the stream around
 * the stages of fit (label sort, centroids K1, scatter SYRK K2, EM, GetOutput: whitening / tridiagonalisation /
 * divide and conquer / back-transformation), transform and scoring.  plda_trace_read synchronises the stream and
 * writes a JSON array [{"name", "calls", "ms", "work", "unit"}] aggregated by name ("work" = algorithmic flop or
 * bytes of the stage where one is defined) into json[cap]; PLDA_E_CAPACITY if it does not fit.  With the
 * environment variable PLDA_HIP_TRACE=1 tracing is on from plda_create and the summary is printed to stderr by
 * plda_destroy.  The reference has no counterpart (its stages are Kaldi calls inside pldamodule.cpp:76-106). */
int plda_trace_enable(plda_handle *h, int32_t on);
int plda_trace_read(plda_handle *h, char *json, int64_t cap, int32_t reset);

/* The symmetric eigensolver of GetOutput on its own (diagnostics and tests; the reference reaches it only through
 * Plda estimation, pldamodule.cpp:102-106 -> Kaldi SpMatrix::Eig).  G [D,D] row-major symmetric, host pointers.
 * eigenvalues[D] descending (signed), eigenvectors [D,D] with eigenvector i in ROW i.  method: 0 = what fit uses
 * (tridiagonalisation + divide and conquer where supported, else block Jacobi), 1 = block Jacobi, 2 = direct
 * method or PLDA_E_NUMERIC.  *method_used (nullable) reports 1 or 2. */
int plda_sym_eig(plda_handle *h, const double *G, int32_t D, int32_t method, double *eigenvalues,
                 double *eigenvectors, int32_t *method_used);
/* The fp64 GEMM behind fit and GetOutput on its own (diagnostics and tests; the reference reaches its counterpart,
 * ATLAS dgemm, only through Kaldi inside pldamodule.cpp:76-106).  `batch` products C_b = alpha op(A_b) op(B_b) + beta C_b,
 * host pointers, row-major: A_b is [M,K] (transA = 0) or [K,M] (transA = 1), B_b is [K,N] or [N,K], C_b [M,N]; operands
 * are stored back to back.  kw (nullable, batch = 1 only): K weights folded into the contraction, sum_k w_k a_mk b_kn.
 * The dispatch is the product's: one 16 x 16 tile per workgroup for M, N, K <= 256, the panel kernel for deeper
 * small products, 64 x 64 / 128 x 128 tiles with split-K above. */
int plda_gemm_f64(plda_handle *h, int64_t M, int64_t N, int64_t K, double alpha, const double *A, int32_t transA,
                  const double *B, int32_t transB, const double *kw, double beta, double *C, int32_t batch);

/* The SPD inverse of the EM's E-step on its own (diagnostics and tests; the reference reaches it only through
 * PldaEstimator::GetStatsFromClassMeans, Kaldi ivector/plda.cc:436-447 -> SpMatrix::Invert).  A [D,D] row-major
 * symmetric positive definite, host pointers; inverse [D,D].  D <= 64: scalar sweep operator in registers,
 * D <= 256: block sweeps on the fp64 matrix cores, above: blocked whitening.  PLDA_E_NUMERIC when a pivot is not
 * positive. */
int plda_spd_inverse(plda_handle *h, const double *A, int32_t D, double *inverse);
/* algorithmic work of the last score_matrix call: flop of the trials GEMM and
 * its depth, for roofline accounting */
int plda_score_last_shape(plda_handle *h, int64_t *M, int64_t *Nt, int32_t *gemm_k);
/* name of the trials-GEMM kernel the last plda_score_matrix* call launched (roofline accounting: bench.py names the
 * kernel its `roofline` block prices); "" before the first call.  PLDA_E_CAPACITY when it does not fit name[cap]. */
int plda_score_last_kernel(plda_handle *h, char *name, int64_t cap);
/* The kernels that the fp64 building blocks (the eigensolver, the GEMM / SYRK family, the SPD inverse and whitening)
 * dispatched since the last call of plda_sym_eig, plda_gemm_f64 or plda_spd_inverse, which clear the record on entry
 * (tests pin a dispatch class by it; the reference has no counterpart).  Host-side text, template arguments included,
 * entries separated by ';' and each listed once in the order of its first launch, e.g.
 * "tridiag_full_kernel<7>;gemm_f64_panel_kernel<0,0,2>;householder_row1_kernel<2>"; a record that ran full ends in the
 * entry "...".  PLDA_E_CAPACITY when it does not fit out[cap] (1024 bytes always do). */
int plda_linalg_last_kernels(plda_handle *h, char *out, int64_t cap);

/* ---- S-norm / adaptive S-norm (AS-norm): no counterpart in the reference, whose README says of score normalisation
 *      "z-norm (other norms are not implemented yet)" ----
 * A trial is normalised on BOTH sides, the enrol model against a cohort and the test vector against the same cohort, each
 * side with the top_k LARGEST of its cohort scores (the closest impostors); top_k = Nc is plain S-norm.
 *
 * plda_cohort_stats*: X [R, Dout] and the cohort C [Nc, Dout] are already-transformed vectors (the cohort with
 * num_examples = 1); n / n_uniform are the counts of the rows of X as in plda_score_matrix (test utterances: n_uniform = 1,
 * where the LLR is symmetric in its two vectors).  With s[r, c] the fp32 score plda_score_matrix_dev(X, n, C) writes
 * without z-norm statistics, and T(r) the multiset of the top_k largest s[r, .] (-0.0 == +0.0; finite scores only):
 * mean[r] = mean of T(r), std[r] = POPULATION standard deviation of T(r) (as pldamodule.cpp:240-250 for z-norm), both fp64.
 * Selection is exact (radix refinement per row, no sort, no cap on top_k); the sums are taken of (s - tau), tau the
 * top_k-th largest value, so a row whose top_k values are equal has std exactly 0.  The result of a row does not depend on
 * how the call is cut into slabs.  The R x Nc scores exist one row slab at a time (scored by the trials GEMM with the cohort
 * side packed once, consumed, dropped): the call holds one slab of <= 4 GiB (by default <= 2 GiB;
 * PLDA_SNORM_SLAB_ROWS in the environment at plda_create sets the rows per slab) beyond the
 * packed operands, whatever R x Nc is.  A prepared test side (plda_score_prepare_dev) is dropped.  The _dev form enqueues on
 * the handle's stream (mixed counts: one wait, as plda_score_matrix_dev).
 *
 * plda_score_matrix_snorm*: the trials matrix of plda_score_matrix (no z-norm) mapped with per-row statistics (emean, estd)[M]
 * and per-column statistics (tmean, tstd)[Nt], in fp64 on the finished fp32 score `raw`, rounded once to fp32:
 *     side(raw, m, s) = (raw - m) / s  if s != 0  else raw                       (the guard of pldamodule.cpp:269-273)
 *     out[i, j] = 0.5 * (side(raw, emean[i], estd[i]) + side(raw, tmean[j], tstd[j]))
 * One pair may be NULL (both of its pointers): out = side of the other pair, without the 0.5.  Both pairs NULL, or one
 * pointer of a pair alone, is PLDA_E_INVAL.  Columns [Nt, ld_out) are not written. */
int plda_cohort_stats_dev(plda_handle *h, const double *dX, const int32_t *dn, int32_t n_uniform, int64_t R,
                          const double *dC, int64_t Nc, int64_t top_k, double *dmean, double *dstd);
int plda_cohort_stats(plda_handle *h, const double *X, const int32_t *n, int32_t n_uniform, int64_t R,
                      const double *C, int64_t Nc, int64_t top_k, double *mean, double *std);
int plda_score_matrix_snorm_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M,
                                const double *dV, int64_t Nt, const double *demean, const double *destd,
                                const double *dtmean, const double *dtstd, float *dout, int64_t ld_out);
int plda_score_matrix_snorm(plda_handle *h, const double *U, const int32_t *n_enrol, int32_t n_uniform, int64_t M,
                            const double *V, int64_t Nt, const double *emean, const double *estd, const double *tmean,
                            const double *tstd, float *out, int64_t ld_out);

/* ---- top-N retrieval with indices: closed-set identification (for each test utterance the best enrolled models) and
 *      watch-list retrieval (for each enrolled model the best utterances of an archive); what the reference's callers do
 *      with the scores of their nested loop (scoring/scorePLDA.py:302-318) ----
 * S is the fp32 trials matrix [M, Nt].  A LINE is a row (axis = 0: line i is row i, its candidates are the columns j) or a
 * column (axis = 1: line j is column j, its candidates are the rows i).  With key the order-preserving integer key of a score
 * (-0.0 == +0.0; a total order on all bit patterns, so non-finite scores are not an error: they sort where their keys put
 * them), the result of a line is its first top_n candidates in the order (key descending, candidate index ascending):
 *     out_index[line, r]   int64: the candidate's index
 *     out_scores[line, r]  fp32: the matrix entry at that index, bit for bit (a -0.0 stays -0.0)
 * both [L, top_n] row-major, L = M (axis 0) or Nt (axis 1); nothing else is written.  The order is total, so the result does
 * not depend on the slab height, the grid, the launch order or the run.  Exact for any data; the speed of axis 1 depends on
 * the data (columns whose scores ascend with the row index are its worst case, descending ones its best).
 * axis must be 0 or 1, 1 <= top_n <= min(PLDA_TOPN_MAX, length of a line), Nt <= 2^30 (axis 1: M < 2^31); else PLDA_E_INVAL.
 *
 * plda_topn_matrix_dev: on a finished matrix in HBM (row pitch ld >= Nt floats; columns [Nt, ld) are never used), walked in
 * row pieces of the slab height below.  Enqueues on the handle's stream, does not synchronise, allocates nothing.
 * plda_score_topn*: the operand form -- the matrix is never held.  The scores are those of plda_score_matrix_dev with the
 * z-norm pair (zmean, zstd)[M] (both NULL: none) or, with one or both S-norm pairs (emean, estd)[M], (tmean, tstd)[Nt], those
 * of plda_score_matrix_snorm_dev.  The z-norm pair together with an S-norm pair, or one pointer of a pair alone, is
 * PLDA_E_INVAL.  The scores exist one row slab at a time, as in plda_cohort_stats_dev (the same slab buffer, height rule and
 * PLDA_SNORM_SLAB_ROWS; the test side packed once, the distinct counts found once; a prepared test side is dropped); beyond
 * the slab and the packed operands the call allocates nothing: the running result of axis 1 lives in the output arrays. */
#define PLDA_TOPN_MAX 256
int plda_topn_matrix_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, int32_t axis, int64_t top_n,
                         float *dout_scores, int64_t *dout_index);
int plda_score_topn_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M,
                        const double *dV, int64_t Nt, const double *dzmean, const double *dzstd, const double *demean,
                        const double *destd, const double *dtmean, const double *dtstd, int32_t axis, int64_t top_n,
                        float *dout_scores, int64_t *dout_index);
int plda_score_topn(plda_handle *h, const double *U, const int32_t *n_enrol, int32_t n_uniform, int64_t M, const double *V,
                    int64_t Nt, const double *zmean, const double *zstd, const double *emean, const double *estd,
                    const double *tmean, const double *tstd, int32_t axis, int64_t top_n, float *out_scores,
                    int64_t *out_index);

/* ---- z-norm: replaces MPlda_norm (pldamodule.cpp:196-256) ----
 * Every cohort row is transformed with num_examples = Nb (:224) and scored as
 * the TRAIN side with n = 1 against every model vector (:235); per model the
 * mean and population std over the cohort (:240-250).  Fused: the Nb x M score
 * matrix is never materialised.  models are already-transformed vectors. */
/* num_examples: the count the reference hands to TransformIvector at :224, i.e. the
 * row count of the FULL background matrix; differs from Nb only when the caller
 * passes a row subset (numutts > 0, :204-216).  0 means Nb. */
int plda_znorm_stats(plda_handle *h, const double *bkg, int64_t Nb, int32_t num_examples,
                     int32_t Din, const double *models, int64_t M, double *out_mean,
                     double *out_std);
int plda_znorm_stats_dev(plda_handle *h, const double *dbkg, int64_t Nb, int32_t num_examples,
                         int32_t Din, const double *dmodels, int64_t M, double *dout_mean,
                         double *dout_std);

/* ---- d-vector front-end (the step before the path): replaces
 * scoring/extractdvector.py:19-58 -- per-frame L2 normalisation (getnormalizedvector,
 * :19-29; skipped when l2norm == 0, the *_nol2 variants :50-59) and pooling over each
 * utterance's frames: method 0 = mean (:37-39), 1 = max (:32-34), 2 = population
 * variance (:42-47).  frames [T, D] row-major, dtype 0 = float32 / 1 = float64;
 * offsets[U+1] frame boundaries of the U utterances; out [U, D] fp64.  Accumulation is
 * fp64 for either dtype (a float32 frame converts exactly, so both meet the same bounds):
 * mean and max within 1e-12 of np.mean / np.max relative to the largest output; the variance
 * is one pass over sums shifted by the utterance's first (normalised) frame and stays within
 * about n eps (1 + ((y0 - mean) / std)^2) of the two-pass np.var, relative and per column,
 * also where |mean| >> std (tested to 1e-10).  An empty utterance gives a NaN row; NaN and
 * Inf propagate as they do in NumPy (a NaN element: its column, or the whole row under
 * l2norm; an all-zero frame under l2norm: the whole row NaN). ---- */
int plda_dvector_pool(plda_handle *h, const void *frames, int32_t dtype, int64_t T, int32_t D,
                      const int64_t *offsets, int64_t U, int32_t method, int32_t l2norm,
                      double *out);
int plda_dvector_pool_dev(plda_handle *h, const void *dframes, int32_t dtype, int64_t T, int32_t D,
                          const int64_t *doffsets, int64_t U, int32_t method, int32_t l2norm,
                          double *dout);

/* ---- HTK feature files (the data format in front of the path): replaces the reference's reader
 * chtk::htk_load (chtk/chtk.cpp:38-88, called at src/kaldi-utils.hpp:22; header layout
 * chtk/chtk.h:52-57).  A call decodes a BATCH of U files whose DATA sections (everything after
 * the 12-byte header) sit in one blob: file u starts at 32-bit word file_off[u] of the blob and
 * has frame_off[u+1] - frame_off[u] frames of `samplesize` bytes (a multiple of 4); a file
 * shorter than its header claims must be zero-padded to that size, which is what the
 * reference's zero-initialised read buffer yields (chtk.cpp:56-57).  out [T, (2 frm_ext + 1) *
 * samplesize / 4] float32, T = frame_off[U]: every word byte-swapped (big-endian floats), frame
 * i = frames clamp(i - frm_ext .. i + frm_ext, 0, n - 1) of its file concatenated (:71-86).
 * Bit-exact with the reference; the output feeds plda_dvector_pool_dev with the same
 * frame_off. ---- */
int plda_htk_frames(plda_handle *h, const void *blob, int64_t blob_bytes, const int64_t *file_off,
                    const int64_t *frame_off, int64_t U, int32_t samplesize, int32_t frm_ext,
                    float *out);
int plda_htk_frames_dev(plda_handle *h, const void *dblob, const int64_t *dfile_off,
                        const int64_t *dframe_off, int64_t U, int64_t T, int32_t samplesize,
                        int32_t frm_ext, float *dout);

/* ---- equal error rate (the step after the path): replaces scoring/eer.py:68-73
 * (bob.measure.eer_threshold + farfrr; bob is absent and un-pinned, its published
 * definition is restated: FAR = #{impostor >= t}/Nn, FRR = #{target < t}/Np, t = the
 * midpoint after the score where |FAR - FRR| is minimal, later candidate on ties).
 * out[6] = threshold, FAR, FRR, EER = (FAR + FRR)/2, #targets, #impostors.
 * _matrix: trial (i, j) of the fp32 score matrix is a target iff enrol_spk[i] == test_spk[j];
 * _lists: separate target / impostor score arrays (the two files eer.py reads).
 *
 * NON-FINITE SCORES ARE REFUSED.  A trial is a column in [0, Nt) of a row in [0, M), or an element of a list.  A NaN of either
 * sign, +Inf or -Inf among the trials -- an all-NaN row is a regular output of the transform, see there -- makes every EER and
 * DET entry point (plda_eer_lists, plda_eer_matrix_dev, plda_score_eer_dev, plda_eer_matrix_sharded_dev,
 * plda_eer_matrix_comm_dev, plda_det_lists, plda_det_matrix_dev) return PLDA_E_INVAL with plda_last_error
 * "eer: <count> non-finite score(s) among the trials" (resp. "det: ..."), as calibration, fusion and minDCF do.  The count is
 * exact, and global in the sharded forms, where every rank refuses together; it is reported before "need at least one target
 * and one impostor".  Nothing is written to out, far, frr or thresholds, and the handle stays usable.
 * PADDING IS NOT DATA: the columns [Nt, ld) of a matrix may hold anything, NaN and Inf included, and change nothing.
 * FINITE SCORES: oracle/plda_oracle_np.py:eer is the specification, the extremes (+-FLT_MAX, subnormals, +-0 = one score)
 * included, and the rates returned are always farfrr at the threshold returned.  The definition's last candidate is
 * s_max + 1e-8 formed in float64; from |s_max| >= 2^27 on that sum is s_max itself, the candidate then counts the trials AT s_max
 * as accepted -- the rates of the candidate before it -- and, being the later one, wins their tie: all scores equal to
 * s >= 2^27 give (s, FAR 1, FRR 0, EER 0.5), where s < 2^27 gives (s + 1e-8, FAR 0, FRR 1, EER 0.5). ---- */
int plda_eer_matrix_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt,
                        const int64_t *denrol_spk, const int64_t *dtest_spk, double *out);
int plda_eer_lists(plda_handle *h, const float *pos, int64_t np, const float *neg, int64_t nn,
                   double *out);
/* The points of the DET curve scoring/eer.py:34-62 plots (bob.measure.plot.det(negatives, positives, 100); definition
 * restated, bob absent): n_points (2 .. 2047) thresholds spread evenly from the smallest to the largest score, accumulated in
 * float64; far[i] = #{impostor >= t_i} / Nn, frr[i] = #{target < t_i} / Np (HOST arrays; thresholds nullable).  The plot's axes
 * are the normal deviates of the two rates (plda_amd.eer.ppndf); drawing it stays with the caller.  One non-finite score
 * would make the step and every threshold after the first Inf or NaN: refused with its count, as above; padding is not data. */
int plda_det_matrix_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt,
                        const int64_t *denrol_spk, const int64_t *dtest_spk, int32_t n_points, double *far, double *frr,
                        double *thresholds);
int plda_det_lists(plda_handle *h, const float *pos, int64_t np, const float *neg, int64_t nn, int32_t n_points,
                   double *far, double *frr, double *thresholds);
/* The EER of the trials between enrol models and test vectors WITHOUT the matrix (round 5): what the reference's caller
 * wants from its M x Nt calls of MPlda_score (scoring/scorePLDA.py:302-318 -> scoring/eer.py:68-76) is these six numbers,
 * not the scores -- BASELINE C4's matrix is 192 GB.  Arguments as plda_score_matrix_dev (transformed vectors, per-model
 * counts or one count, optional z-norm statistics) plus the speaker ids of plda_eer_matrix_dev; the scores exist one row
 * slab of <= 4 GiB at a time (scored by the trials GEMM, consumed by the one-pass EER, dropped).  The result is identical
 * to plda_score_matrix_dev + plda_eer_matrix_dev.  out is a HOST array; the call synchronises the handle's stream. */
int plda_score_eer_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M,
                       const double *dV, int64_t Nt, const double *dzmean, const double *dzstd,
                       const int64_t *denrol_spk, const int64_t *dtest_spk, double *out);
/* Row-sharded trials matrix (one process per GPU, each holding a slab of enrol rows and ALL test
 * labels): the same three histogram passes over the local slab; after each pass the library calls
 * `reduce(ctx, hist, NULL, NULL)` with hist[2 * 2048] host counters to be SUMMED over the ranks in
 * place, and once at the end `reduce(ctx, NULL, below, above)` with two host words to be replaced
 * by their MAX resp. MIN over the ranks.  The callback returns 0 on success.  Every rank gets the
 * global result; scores never leave their GPU (the exchange is 3 x 32 KiB + 8 bytes; two more passes, each with its
 * reduction, where the largest score may reach 2^27 in magnitude -- decided on the summed counters, so on every rank alike).
 * A rank that refuses (non-finite scores anywhere: the count is the global one) still makes every call its peers wait in.
 * plda_amd/sharding.py:eer_sharded supplies a torch.distributed callback. */
typedef int (*plda_eer_reduce_fn)(void *ctx, unsigned long long *hist, unsigned *below, unsigned *above);
int plda_eer_matrix_sharded_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt,
                                const int64_t *denrol_spk, const int64_t *dtest_spk,
                                plda_eer_reduce_fn reduce, void *ctx, double *out);

/* ---- linear score calibration, Cllr and actual DCF (the step after normalisation; the reference stops at the EER,
 * scoring/eer.py:68-73, so this is the project's own extension: tests/calibration_model.py pins it).
 *
 * A z- or AS-normalised score is not a log-likelihood ratio any more; the affine map llr = a * s + b, trained by
 * prior-weighted logistic regression on labelled trials (the "linear calibration" of BOSARIS / FoCal), makes it one.
 * Trials and their class are those of plda_eer_matrix_dev / plda_eer_lists: an fp32 score s, a target iff
 * enrol_spk[i] == test_spk[j] (matrix and operand forms) or by list.  Np, Nn are the class counts.
 *
 * One CALIBRATION PASS at (a, c, theta), all fp64, computes per trial y = a * (double)s + c, e = exp(-|y|), and in the
 * overflow-free forms softplus(y) = max(y, 0) + log1p(e), p = sigmoid(y) = y >= 0 ? 1/(1+e) : e/(1+e), w = p (1 - p) = e/(1+e)^2:
 *
 *     class        L                   G0           G1             H0       H1         H2
 *     target       sum softplus(-y)    sum (1-p)    sum (1-p) s    sum w    sum w s    sum w s^2
 *     non-target   sum softplus(y)     sum p        sum p s        sum w    sum w s    sum w s^2
 *
 * plus the exact integers Np, Nn, miss = #{target: (double)s < theta}, fa = #{non-target: (double)s >= theta} (the FAR / FRR
 * convention of the EER above; the threshold is compared on the RAW score, so the counts do not depend on how y was
 * rounded), the number of non-finite scores, and per class the fp32 minimum and maximum: one plda_calib_record.  Its sums and
 * counts add across row shards (min / max combine by min / max), so a sharded form is a reduction of records.  The sums are
 * taken without floating-point atomics in a fixed order: the record of a call is bit-identical from run to run.  Accuracy:
 * a non-zero term has |y| < 746 and a relative error of at most (|y| + c0) 2^-53, c0 a handful of ulps for exp, log1p
 * and the divide, i.e. < 8.4e-14; every sum is within 1e-12 * sum |term| of the exact one.
 *
 * From one record, with effective target prior pi, tau = log(pi / (1 - pi)) and the pass taken at c = b + tau:
 *     F(a, b; pi) = pi/Np * L_t + (1-pi)/Nn * L_n   (nats);   dF/da = -pi/Np * G1_t + (1-pi)/Nn * G1_n,  dF/db likewise from
 *     G0;  the 2 x 2 Hessian from (H2, H1, H0) with the same two weights;
 *     Cllr = F(1, 0; 0.5) / ln 2 of the scores as they are, Cllr(a, b) = F(a, b; 0.5) / ln 2 after a map;
 *     actDCF(pi, Cmiss, Cfa) = (Cmiss pi miss/Np + Cfa (1-pi) fa/Nn) / min(Cmiss pi, Cfa (1-pi)) at the Bayes threshold,
 *     which the caller turns into the raw-score threshold theta = (log(Cfa (1-pi) / (Cmiss pi)) - b) / a  (a > 0) before
 *     the pass (plda_amd/calibration.py:act_dcf).
 * A pass that meets a non-finite score returns PLDA_E_INVAL with the count in plda_last_error, Np == 0 or Nn == 0 likewise
 * (the record is written all the same): no score is silently left out.
 *
 * FIT: damped Newton on (a, b) from (0, 0) -- there p = sigmoid(tau) for every trial and the Hessian is the scores'
 * weighted second-moment matrix, well conditioned whatever the scale of the scores (a = 1 saturates on raw LLRs of a few
 * hundred).  Direction d = -H^-1 g, decrement lambda2 = g' H^-1 g; stop when lambda2 <= tol (tol == 0: the default 1e-18 --
 * the host model's floor of lambda2 is 1e-26 .. 1e-33 on sets of 3e3 .. 1e6 trials, so the default stands) or after max_iter
 * (<= 0: 100) iterations; backtracking t = 1, 1/2, ... (at most 30 halvings) until
 * F(x + t d) <= F(x) - 1e-4 t lambda2 + 2^-44 |F(x)| -- the last term is the rounding of F itself, without which the final
 * step, whose gain is below F's resolution, is refused at random.  The accepted point's record is the next iteration's.
 * `passes` counts every pass of the call: one at (1, 0) for cllr_before, one at the start, one per trial point, and one
 * more for cllr_after when prior != 0.5.  All scores equal, or a Hessian that is not positive definite in fp64, is
 * PLDA_E_INVAL; prior outside (0, 1) or tol < 0 likewise.  separable = (min target > max non-target): the optimum is then at
 * infinity and the caller is told (converged is usually 0) instead of being handed a huge `a` silently.
 *
 * APPLY: plda_affine_map_dev writes out[i, j] = (float)fma(a, (double)s[i, j], b) -- one rounding to fp64, one to fp32 --
 * in place if dout == dscores and ld_out == ld; columns [Nt, ld_out) are not written (plda_score_matrix_snorm's contract).
 * It enqueues on the handle's stream and does not synchronise.
 *
 * The _lists forms take HOST arrays of scores; out_record / out_fit are HOST structures and these calls synchronise the
 * handle's stream, as plda_score_eer_dev does.  The operand forms (arguments as plda_score_eer_dev) never hold the matrix:
 * the slabs are RE-SCORED once per pass -- a fit of a dozen passes scores the trials a dozen times -- and give the scores
 * of plda_score_matrix_dev bit for bit. ---- */
typedef struct plda_calib_record {
  double sum[2][6];        /* [0 = non-target, 1 = target][L, G0, G1, H0, H1, H2] */
  uint64_t np, nn, miss, fa, nonfinite;
  float min_t, max_t, min_n, max_n;   /* +inf / -inf for a class without trials */
} plda_calib_record;
typedef struct plda_calib_fit {
  double a, b;
  double objective;        /* F(a, b; prior) / ln 2 */
  double cllr_before, cllr_after;
  double lambda2;          /* the Newton decrement at (a, b) */
  int32_t iterations, passes, converged, separable;
} plda_calib_fit;
int plda_calib_pass_matrix_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt,
                               const int64_t *denrol_spk, const int64_t *dtest_spk, double a, double c, double theta,
                               plda_calib_record *out_record);
int plda_calib_pass_lists(plda_handle *h, const float *pos, int64_t np, const float *neg, int64_t nn, double a, double c,
                          double theta, plda_calib_record *out_record);
int plda_score_calib_pass_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M,
                              const double *dV, int64_t Nt, const double *dzmean, const double *dzstd,
                              const int64_t *denrol_spk, const int64_t *dtest_spk, double a, double c, double theta,
                              plda_calib_record *out_record);
int plda_calib_fit_matrix_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt,
                              const int64_t *denrol_spk, const int64_t *dtest_spk, double prior, double tol,
                              int32_t max_iter, plda_calib_fit *out_fit);
int plda_calib_fit_lists(plda_handle *h, const float *pos, int64_t np, const float *neg, int64_t nn, double prior,
                         double tol, int32_t max_iter, plda_calib_fit *out_fit);
int plda_score_calib_fit_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M,
                             const double *dV, int64_t Nt, const double *dzmean, const double *dzstd,
                             const int64_t *denrol_spk, const int64_t *dtest_spk, double prior, double tol,
                             int32_t max_iter, plda_calib_fit *out_fit);
int plda_affine_map_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, double a, double b,
                        float *dout, int64_t ld_out);

/* ---- multi-system score fusion by prior-weighted logistic regression (csrc/fusion.hip; the "fusion" half of BOSARIS /
 * FoCal next to the calibration above; the reference writes one score file per back-end -- scoring/scorePLDA.py,
 * scoring/scoreLDA.py -- and combines nothing, so this is the project's own extension: tests/fusion_model.py pins it).
 *
 * INPUTS: K systems, 1 <= K <= PLDA_FUSION_MAX_SYSTEMS; system k gives an fp32 score s_k for every trial.  Trials and their
 * class are those of plda_eer_matrix_dev / plda_eer_lists.  Matrix form: K matrices [M, Nt], each with its own base pointer
 * and row pitch ld[k] >= Nt, under ONE pair of speaker-id arrays (trial (i, j) is a target iff enrol_spk[i] == test_spk[j]).
 * Lists form: K parallel target arrays of length np and K parallel non-target arrays of length nn; element t of every
 * array is the same trial.
 *
 * FUSED VALUE: a fixed chain of fused multiply-adds in fp64,
 *     y_0 = c,   y_{k+1} = fma(a_k, (double)s_k, y_k),   y = y_K.
 * The order and the single rounding per step are part of the contract (the apply is pinned bit for bit on it).
 *
 * One FUSION PASS at (a[K], c, theta) uses the feature vector phi = (1, s_0, .., s_{K-1}) (K + 1 entries) and e, softplus, p,
 * w of y exactly as the calibration pass.  Per class (g = 1 - p for a target, p for a non-target):
 *     L = sum softplus(-/+ y),    G[j] = sum g phi_j,    H[t(i, j)] = sum w phi_i phi_j  for i <= j,  t(i, j) = j (j + 1) / 2 + i
 * (the packing does not depend on K; at K = 1 G and H are the calibration's G0, G1 and H0, H1, H2), plus the exact integers
 * np, nn, miss = #{target: y < theta}, fa = #{non-target: y >= theta} (compared on the CHAIN VALUE y, not on a raw score),
 * nonfinite = the number of trials in which any system's score is non-finite, per class the fp64 minimum and maximum of y,
 * and per system the fp32 minimum and maximum of s_k over all trials: one plda_fusion_record, with arrays dimensioned for
 * K = 8, entries beyond K zero and n_systems stored.  A non-finite score, or an empty class, is PLDA_E_INVAL with the count
 * in plda_last_error; the record is written all the same.  The sums are taken without floating-point atomics in a fixed
 * order and the grid is a function of the shape and K alone: a call's record is bit-identical from run to run.  Sums and
 * counts add across row shards (extremes by min / max).
 *
 * ACCURACY (derived, not measured).  The chain has K roundings, each of at most u |partial| <= u Y with u = 2^-53 and
 * Y = |c| + sum_k |a_k s_k| -- Y and not |y|, because the chain can cancel; exp(-|y|) turns the absolute error K u Y of y
 * into a relative one, and the term's own operations (exp, log1p, the divide, the products with phi) add c0, a handful of
 * ulps: a non-zero term has a relative error of at most ((K + 1) Y + c0) 2^-53.  Where (K + 1) Ymax <= 2000 over the call's
 * trials that is at most 2.3e-13 per term.  The additions: a sum is a fixed tree of 34 levels (wave, block, partial records)
 * over RUNS that are added one term after the other, and a run of n terms adds at most (n - 1) u sum |term|.  With R the rows
 * a workgroup walks (R = ceil(M / min(M, floor(4096 / ceil(Nt / 1024)))), a non-target run is one thread's 4 R trials; the
 * target run is the targets of one WAVE (its lanes' targets go into one accumulator per entry), at most 256 R.  So every sum
 * is within (2.3e-13 + (n + 34) u) sum |term| of the exact one, n = 4 R resp. the largest number of targets one wave meets:
 * inside the calibration's band 1e-12 sum |term| as a WORST case while n <= 6900 -- every non-target sum up to R = 1700, every
 * target sum whose waves meet fewer than 6900 targets (at 20 utterances per speaker a wave of a 100k x 100k matrix, R = 2440,
 * meets about 130).  Beyond that (whole waves of targets over thousands of rows) 1e-12 is a typical figure, the error of
 * such a run growing like sqrt(n) u for terms of one sign, not a bound.  A list pass has runs of n / (4096 * 256) terms.
 *
 * FIT: damped Newton on x = (b, a_0 .. a_{K-1}) from 0.  From the record of a pass at c = b + logit(prior):
 *     F = pi/Np L_t + (1-pi)/Nn L_n,   g_j = -pi/Np G_t[j] + (1-pi)/Nn G_n[j],   H assembled with the same two weights.
 * Direction: scale to unit diagonal, Hs = D^-1/2 H D^-1/2 (the outcome is then independent of each system's units: PLDA LLRs
 * of a few hundred and LDA log-posteriors of -20 are handled alike), Cholesky of Hs, d = -H^-1 g, lambda2 = g' H^-1 g.  A
 * diagonal entry <= 0, or a Cholesky pivot <= 1e-12, is PLDA_E_INVAL: the entries are known to 1e-12, so a smaller pivot is
 * indistinguishable from a system that is an affine function of the others; the error names the pivot's system.  A system
 * with smin == smax is refused before any Newton step, by name.  After the first step, a degenerate Hessian at a point
 * where the classes are separable (the run-away of a separable set) ends the iteration, unconverged, instead of failing
 * the call; lambda2 is then the decrement of the last point at which it could be computed, the one before.  Decrement, stopping rule (tol 0 -> 1e-18, max_iter <= 0 ->
 * 100), Armijo backtracking with the 2^-44 |F| allowance are the calibration's, unchanged.  `passes` counts every pass of the
 * call: one at the start, one per trial point, one more for cllr_after = F(x; 0.5) / ln 2 when prior != 0.5 (there is no
 * "before": K systems have no common scale to report one on).  separable = (ymin_t > ymax_n at the returned point).
 * plda_fusion_newton is the step as a pure function (no handle, no GPU; the pattern of plda_min_dcf_step): from a record taken
 * at c = b + logit(prior) it returns F (nats), d[n_systems + 1] in the order of x, and lambda2; the device fit calls it and the
 * CPU tests drive a whole fit through it with the host model's records.  Its refusals leave their text in plda_last_error(NULL).
 *
 * APPLY: plda_fusion_map_dev writes out[i, j] = (float)y, the chain with c = b: one rounding to fp32.  In place if dout is
 * one of the inputs with ld_out == ld[k]; any other overlap is the caller's error.  Columns [Nt, ld_out) are not written.  It
 * enqueues on the handle's stream and does not synchronise.
 *
 * CONVENTIONS: the pointer arrays (const float *const *, const int64_t *ld, const double *a) are HOST arrays of K entries;
 * the matrices they name are in HBM (_dev) or on the host (_lists).  Records and fit results are HOST structures; the pass
 * and fit calls synchronise the handle's stream, as the calibration's do.
 *
 * OUT OF SCOPE, each on purpose: an operand form (the systems are different models; the caller holds their matrices); the
 * row-sharded form (the record adds across shards as the calibration's does -- unbuilt there too); regularisation; minCllr.
 * (Quality measures / side information and this model's own operand form: the next section.) ---- */
#define PLDA_FUSION_MAX_SYSTEMS 8
typedef struct plda_fusion_sums {
  double L;
  double G[PLDA_FUSION_MAX_SYSTEMS + 1];
  double H[(PLDA_FUSION_MAX_SYSTEMS + 1) * (PLDA_FUSION_MAX_SYSTEMS + 2) / 2];   /* t(i, j) = j (j + 1) / 2 + i, i <= j */
} plda_fusion_sums;
typedef struct plda_fusion_record {
  plda_fusion_sums sum[2];           /* [0 = non-target, 1 = target] */
  double ymin[2], ymax[2];           /* of the chain value per class; +inf / -inf for a class without trials */
  uint64_t np, nn, miss, fa, nonfinite;
  float smin[PLDA_FUSION_MAX_SYSTEMS], smax[PLDA_FUSION_MAX_SYSTEMS];   /* per system over all trials */
  int32_t n_systems, reserved;
} plda_fusion_record;
typedef struct plda_fusion_fit {
  double a[PLDA_FUSION_MAX_SYSTEMS];
  double b;
  double objective;                  /* F(x; prior) / ln 2 */
  double cllr_after;
  double lambda2;                    /* the Newton decrement at the returned point */
  int32_t iterations, passes, converged, separable;
} plda_fusion_fit;
int plda_fusion_pass_matrices_dev(plda_handle *h, int32_t n_systems, const float *const *dscores, const int64_t *ld, int64_t M,
                                  int64_t Nt, const int64_t *denrol_spk, const int64_t *dtest_spk, const double *a, double c,
                                  double theta, plda_fusion_record *out_record);
int plda_fusion_pass_lists(plda_handle *h, int32_t n_systems, const float *const *pos, int64_t np, const float *const *neg,
                           int64_t nn, const double *a, double c, double theta, plda_fusion_record *out_record);
int plda_fusion_fit_matrices_dev(plda_handle *h, int32_t n_systems, const float *const *dscores, const int64_t *ld, int64_t M,
                                 int64_t Nt, const int64_t *denrol_spk, const int64_t *dtest_spk, double prior, double tol,
                                 int32_t max_iter, plda_fusion_fit *out_fit);
int plda_fusion_fit_lists(plda_handle *h, int32_t n_systems, const float *const *pos, int64_t np, const float *const *neg,
                          int64_t nn, double prior, double tol, int32_t max_iter, plda_fusion_fit *out_fit);
int plda_fusion_map_dev(plda_handle *h, int32_t n_systems, const float *const *dscores, const int64_t *ld, int64_t M, int64_t Nt,
                        const double *a, double b, float *dout, int64_t ld_out);
int plda_fusion_newton(const plda_fusion_record *record, double prior, double *F, double *d, double *lambda2);

/* ---- quality-aware calibration: side-information terms in the fusion (K25; csrc/fusion.hip; the quality measure
 * functions -- duration, embedding norm, the AS-norm cohort mean -- put in front of reported verification numbers since
 * VoxSRC-20; the project's own extension like the fusion above, pinned by tests/fusion_side_model.py).
 *
 * A call has K >= 1 SYSTEMS (fp32 matrices, exactly as plda_fusion_*_matrices_dev takes them) and Q >= 0 SIDES with
 * K + Q <= PLDA_FUSION_MAX_SYSTEMS.  Side q is {op, enrol[M], test[Nt]}: two fp32 DEVICE vectors and an op code; its value
 * for trial (i, j) is ONE IEEE fp32 operation on e = enrol[i], t = test[j]:
 *     PLDA_SIDE_MIN      e < t ? e : t          PLDA_SIDE_MAX   e > t ? e : t          PLDA_SIDE_SUM   e + t
 *     PLDA_SIDE_ABSDIFF  fabsf(e - t)           PLDA_SIDE_PROD  e * t
 * Ties and signed zeros follow the written comparison (MIN of (+0, -0) is -0, the `t`; with a NaN operand the comparison is false, so MIN
 * and MAX return t, whatever it is; the other three return NaN).  A one-sided quality is SUM with a zero vector on the other side.  The value never exists
 * in memory: the kernels form it in registers, so a side costs M + Nt floats where a materialised "system" costs M * Nt.
 *
 * FEATURE VECTOR phi = (1, s_0 .. s_{K-1}, q_0 .. q_{Q-1}); the CHAIN is the fusion's over these K + Q fp32 values in that
 * order with weights a[K + Q]; the RECORD is an unchanged plda_fusion_record with n_systems = K + Q (smin / smax of a side
 * are the extremes of its values over all trials; a trial whose side value is non-finite counts in `nonfinite` like a
 * non-finite score); the FIT is the fusion's, and plda_fusion_newton takes these records as they are.
 *
 * THE CONTRACT: a side pass, fit or map is BIT-IDENTICAL to plda_fusion_pass_matrices_dev / _fit_matrices_dev / _map_dev
 * over K + Q matrices in which every side has been materialised with the fp32 operation above, at any pitch or alignment
 * of those matrices: same grid, same visiting order, same account (the accuracy statement of the fusion holds unchanged).
 * Q = 0 is accepted and IS the existing path.
 *
 * OPERAND FORM (plda_score_fusion_side_*_dev): system 0 is this model's own score matrix -- the arguments of
 * plda_score_calib_fit_dev -- produced slab by slab and never held; K = 1, a[1 + Q].  Its record sums across slabs (one
 * launch per slab, the partial records of all slabs reduced together in slab order), so it is NOT bit-identical to the
 * matrix form: integers are equal, sums agree within the fusion's band, and it is bit-identical from run to run.
 *
 * REFUSALS, PLDA_E_INVAL with a text naming the argument or side: n_systems < 1 or n_systems + n_sides > 8 (n_sides < 0); a
 * NULL `sides` with n_sides > 0; an op outside 0 .. 4; a NULL vector.  A side with smin == smax is refused before any Newton
 * step, by name ("side q"), like a constant system; linearly dependent sides (the same side twice; MIN, MAX and SUM of one
 * pair of vectors) meet the fusion's Cholesky-pivot refusal, whose text names the side.
 *
 * CONVENTIONS: `sides` is a HOST array of n_sides entries, like the pointer arrays of the fusion; the vectors it names are in
 * HBM.  The map may run in place over one of the K matrices under the fusion's rule; columns [Nt, ld_out) stay untouched.
 *
 * OUT OF SCOPE, each on purpose: regularisation; non-linear quality maps (a side enters the chain linearly; log-duration
 * and the like are the caller's transform of the vectors); a row-sharded form; quality terms in the LIST forms -- there the
 * caller evaluates the side per listed trial and passes it as one more list, which the list forms already take. ---- */
#define PLDA_SIDE_MIN 0
#define PLDA_SIDE_MAX 1
#define PLDA_SIDE_SUM 2
#define PLDA_SIDE_ABSDIFF 3
#define PLDA_SIDE_PROD 4
typedef struct plda_fusion_side {
  const float *enrol, *test;         /* device vectors [M], [Nt] */
  int32_t op, reserved;              /* PLDA_SIDE_*; reserved = 0 */
} plda_fusion_side;
int plda_fusion_side_pass_dev(plda_handle *h, int32_t n_systems, const float *const *dscores, const int64_t *ld, int32_t n_sides,
                              const plda_fusion_side *sides, int64_t M, int64_t Nt, const int64_t *denrol_spk,
                              const int64_t *dtest_spk, const double *a, double c, double theta, plda_fusion_record *out_record);
int plda_fusion_side_fit_dev(plda_handle *h, int32_t n_systems, const float *const *dscores, const int64_t *ld, int32_t n_sides,
                             const plda_fusion_side *sides, int64_t M, int64_t Nt, const int64_t *denrol_spk,
                             const int64_t *dtest_spk, double prior, double tol, int32_t max_iter, plda_fusion_fit *out_fit);
int plda_fusion_side_map_dev(plda_handle *h, int32_t n_systems, const float *const *dscores, const int64_t *ld, int32_t n_sides,
                             const plda_fusion_side *sides, int64_t M, int64_t Nt, const double *a, double b, float *dout,
                             int64_t ld_out);
int plda_score_fusion_side_pass_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M,
                                    const double *dV, int64_t Nt, const double *dzmean, const double *dzstd,
                                    const int64_t *denrol_spk, const int64_t *dtest_spk, int32_t n_sides,
                                    const plda_fusion_side *sides, const double *a, double c, double theta,
                                    plda_fusion_record *out_record);
int plda_score_fusion_side_fit_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M,
                                   const double *dV, int64_t Nt, const double *dzmean, const double *dzstd,
                                   const int64_t *denrol_spk, const int64_t *dtest_spk, int32_t n_sides,
                                   const plda_fusion_side *sides, double prior, double tol, int32_t max_iter,
                                   plda_fusion_fit *out_fit);

/* ---- exact minimum detection cost (minDCF; NIST SRE min_Cprimary, VoxCeleb's minDCF) at up to 8 operating points,
 * without sorting (csrc/dcf.hip; the project's own extension like the calibration above: tests/mindcf_model.py pins it).
 * actDCF - minDCF is the calibration loss of a system.
 *
 * Trials, classes, key order and rate conventions are those of plda_eer_matrix_dev / plda_eer_lists: an fp32 score, a
 * target iff enrol_spk[i] == test_spk[j] (or by list), -0.0 == +0.0, FAR(t) = #{non-target >= t} / Nn,
 * FRR(t) = #{target < t} / Np.  "Key" is the order-preserving 32-bit key of a score (a < b <=> key(a) < key(b)).
 *   * A CUT is "reject every trial whose key is <= k" for a key k present in the data, plus the cut that rejects nothing.
 *     (The cut at the largest key rejects everything.)  A cut has exact integer counts miss = #{target key <= k},
 *     fa = #{non-target key > k}; the empty cut has (0, Nn).
 *   * An OPERATING POINT is (prior, c_miss, c_fa), 0 < prior < 1, costs > 0.  The cost of a cut is evaluated in fp64 exactly
 *     as plda_amd/calibration.py:act_dcf evaluates it:
 *         v = ((c_miss * prior) * miss) / Np + ((c_fa * (1 - prior)) * fa) / Nn,   dcf = v / min(c_miss * prior, c_fa * (1 - prior)).
 *     minDCF is the smallest v over all cuts; among cuts whose fp64 v are equal the LOWEST cut wins.
 *     The reported min_dcf is min(dcf, 1): in exact arithmetic the better trivial cut costs exactly min(c_miss * prior,
 *     c_fa * (1 - prior)), so no minimum exceeds 1, but (b * Nn) / Nn is not b for every Nn in fp64 (Nn = 50, b = 0.95: one ulp
 *     above), and a quotient of 1 + 2^-52 would be rounding alone.  The winning cut is chosen on v, before this.
 *   * Reported per point: min_dcf (normalised), miss, fa, far = fa / Nn, frr = miss / Np, and threshold: the smallest score
 *     for the empty cut, +inf for the cut at the largest key, otherwise s + (s' - s) / 2 in fp64 with s the score of k and
 *     s' the next larger score present (the EER's midpoint rule).
 *   * A non-finite score fails the call with PLDA_E_INVAL and the count in plda_last_error, as a calibration pass does;
 *     Np == 0 or Nn == 0 likewise.
 * Two properties follow from evaluating v by ONE fixed expression on integers: (1) it is monotone in miss and in fa also
 * after rounding, so the same expression at (miss at the lower end, fa at the upper end) of a key range is a lower bound on
 * every cut inside the range with no tolerance; (2) min_dcf <= act_dcf holds bit-wise for any threshold, because a
 * calibration pass at that threshold returns the counts of some cut.
 *
 * METHOD: branch and bound over the three key levels of the EER (bits 11 + 11 + 10).  A NODE is a key prefix whose next
 * bits are histogrammed per class; level 0 has one node (every key).  After a level the host step (plda_min_dcf_step, a
 * pure function) forms integer prefix sums: every bin edge is a cut with exact counts and updates each point's incumbent
 * (value, then lowest cut); a bin SURVIVES for a point iff it holds both classes and v(miss at its lower edge, fa at its
 * upper edge) <= incumbent; the survivors of a level, the union over the points, are the next level's nodes.  One read of
 * the scores refines up to 8 nodes at once.  When the trials inside the survivors are few and the next level would need
 * more than one read, one read appends them to two lists and the remaining levels run on the lists.  The keys next to the
 * winning cuts come from a last pass over the lists when the counts prove that they lie inside them, otherwise over the
 * scores.  Integer atomics only: a call is bit-reproducible.
 *
 * out[n_points] / info (nullable) are HOST structures; the calls synchronise the handle's stream.  Arguments otherwise as
 * the EER / calibration siblings; the operand form re-scores the slabs once per read; the _comm form is the row-sharded
 * matrix of plda_eer_matrix_comm_dev (every histogram summed over the ranks, survivors decided identically everywhere,
 * lists local).  PLDA_MINDCF_VARIANT (read by plda_create): 1 = never use the lists, 2 = two nodes per read. ---- */
#define PLDA_MIN_DCF_MAX_POINTS 8
typedef struct plda_dcf_point { double prior, c_miss, c_fa; } plda_dcf_point;
typedef struct plda_min_dcf { double min_dcf, threshold, far, frr; uint64_t miss, fa; } plda_min_dcf;
typedef struct plda_min_dcf_info {
  uint64_t np, nn;
  int32_t reads;              /* passes over the scores themselves (matrix, slabs or the caller's lists) */
  int32_t launches;           /* histogram / append / neighbour passes in all, those over the compact lists included */
  int32_t lists_used;         /* 1: surviving trials were appended to lists and the remaining levels ran there */
  int32_t neighbour_reads;    /* of `reads`: passes that only looked for the keys next to the winning cuts */
  int32_t level_launches[3];  /* histogram passes per level */
  int32_t reserved;
  int64_t level_bins[3];      /* nodes refined at each level (1 at level 0) */
  uint64_t level_trials[3];   /* trials inside them */
} plda_min_dcf_info;
int plda_min_dcf_matrix_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt,
                            const int64_t *denrol_spk, const int64_t *dtest_spk, int32_t n_points,
                            const plda_dcf_point *points, plda_min_dcf *out, plda_min_dcf_info *info);
int plda_min_dcf_lists(plda_handle *h, const float *pos, int64_t np, const float *neg, int64_t nn, int32_t n_points,
                       const plda_dcf_point *points, plda_min_dcf *out, plda_min_dcf_info *info);
int plda_score_min_dcf_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M,
                           const double *dV, int64_t Nt, const double *dzmean, const double *dzstd,
                           const int64_t *denrol_spk, const int64_t *dtest_spk, int32_t n_points,
                           const plda_dcf_point *points, plda_min_dcf *out, plda_min_dcf_info *info);
/* The host step as pure functions (no handle, no GPU; the CPU tests drive the whole refinement through them with NumPy
 * histograms).  plda_min_dcf_step: `hist` holds, per node, [2][2048] counters (class 0 = non-target) of the level's bits
 * (level 0, 1: 11 bits; level 2: 10 bits) of the keys under the node's prefix; nodes ascend by prefix.  Level 0 takes one
 * node (prefix 0), sets state->np / nn / nonfinite from the histogram and starts every incumbent at the empty cut; a
 * non-finite score, an empty class or a bad point is PLDA_E_INVAL.  The survivors are written to next[0 .. *n_next)
 * (ascending; PLDA_E_CAPACITY when more than cap_next; none after level 2).  Any subset of a level's nodes may be given per
 * call: the bound holds against whatever incumbent has been reached.  edge: the cut rejects the keys <= edge.
 * plda_min_dcf_finish: below[p] / above[p] = the largest key <= best[p].edge and the smallest key above it among the keys
 * present (0 / 0xffffffff: none; a cut without an edge rejects nothing, above = the smallest key). */
typedef struct plda_min_dcf_node { uint32_t prefix, reserved; uint64_t miss_below, nn_below, n_pos, n_neg; } plda_min_dcf_node;
typedef struct plda_min_dcf_cut { double value; uint64_t miss, fa; uint32_t edge; int32_t has_edge; } plda_min_dcf_cut;
typedef struct plda_min_dcf_state { uint64_t np, nn, nonfinite; plda_min_dcf_cut best[PLDA_MIN_DCF_MAX_POINTS]; } plda_min_dcf_state;
int plda_min_dcf_step(int32_t level, int64_t n_nodes, const plda_min_dcf_node *nodes, const uint64_t *hist, int32_t n_points,
                      const plda_dcf_point *points, plda_min_dcf_state *state, int64_t cap_next, plda_min_dcf_node *next,
                      int64_t *n_next);
int plda_min_dcf_finish(const plda_min_dcf_state *state, int32_t n_points, const plda_dcf_point *points, const uint32_t *below,
                        const uint32_t *above, plda_min_dcf *out);

/* ---- ROC convex hull (ROCCH), minCllr, the ROCCH-EER and PAV calibration, exact on integers and without a global sort
 * (csrc/rocch.hip; the remaining corner of the BOSARIS evaluation set next to the EER, Cllr / actDCF and minDCF above; the
 * project's own extension: tests/rocch_model.py pins it).  Cllr = minCllr + calibration loss.
 *
 * Trials, classes, keys and cuts are those of plda_min_dcf_*: an fp32 score, -0.0 == +0.0, `key` the order-preserving 32-bit
 * key, a CUT "reject every key <= k" for a key k present in the data, plus the empty cut.  A non-finite score fails the call
 * with PLDA_E_INVAL and the count in plda_last_error; Np == 0 or Nn == 0 likewise.
 *   * ROC POINT of a cut: x = #{non-target key <= k}, y = #{target key <= k}, both integers.  The empty cut is (0, 0), the cut
 *     at the largest key (Nn, Np).  Tied keys of both classes move together: one key is one point.
 *   * ROCCH: the lower convex hull of those points from (0, 0) to (Nn, Np).  Only strict vertices are kept: a middle point is
 *     dropped when the cross product (128-bit integers on the host: it reaches 1e20 at 1e10 trials) is <= 0.  A vertex
 *     record carries x, y, fa = Nn - x, miss = y, the key of its cut (has_key = 0 for the empty cut) and a threshold by the
 *     EER's midpoint rule exactly as plda_min_dcf reports it: the smallest score for the empty cut, +inf for the last
 *     vertex, otherwise s + (s' - s) / 2 in fp64 with s the score of the key and s' the next larger score present.
 *   * PAV: segment i between the vertices i and i + 1 has dn_i = delta x, dt_i = delta y and covers the keys in
 *     (key(V_i), key(V_i+1)]; the first segment also takes everything below, the last everything above.
 *     llr_i = log(dt_i / dn_i) - log(Np / Nn), -inf when dt_i == 0, +inf when dn_i == 0.  The slopes rise strictly, so the
 *     map is non-decreasing.  NO Laplace dummy trials are added: BOSARIS's optloglr adds them (its end segments are finite);
 *     parity with BOSARIS is unpinned (it is not on the build machine).
 *   * minCllr = [ sum_i (dt_i / Np) log1p((dn_i Np) / (dt_i Nn)) + sum_i (dn_i / Nn) log1p((dt_i Nn) / (dn_i Np)) ] / (2 ln 2),
 *     a segment with dt_i == 0 or dn_i == 0 contributing 0; fp64, two sums over the segments in ascending order.  It is the
 *     optimum of the calibration's Cllr over all non-decreasing maps of the score: 0 for separated lists, exactly 1 for a
 *     single key or for targets entirely below the non-targets.
 *   * ROCCH-EER: the point where the hull meets y / Np = 1 - x / Nn, in fp64 from the integer vertices a, b of the segment
 *     that crosses (b the first vertex with y Nn + x Np >= Np Nn): with D = dy Nn + dx Np and tn = Np Nn - (a.y Nn + a.x Np),
 *     eer = (a.y D + tn dy) / (Np D), the numerator an exact 128-bit integer.  eer_far_lo / eer_frr_lo are the rates of a,
 *     eer_far_hi / eer_frr_hi those of b.
 *
 * METHOD: a strict vertex is a cut whose own key group holds a non-target and whose next key group holds a target, so only
 * the cuts next to the keys of ONE class can be vertices.  The EDGE class is the one with fewer trials (the targets on a
 * tie; a matrix: counted from the speaker ids alone).  With u_1 < ... < u_T its distinct keys, the hull of the 2 T points
 * (#other < u_j, #edge < u_j), (#other <= u_j, #edge <= u_j), oriented to (x, y), plus the two end points is the hull of all
 * points.  Read 1 appends the edge keys (at most PLDA_ROCCH_EDGE_CAP of them, default 2^24: PLDA_E_CAPACITY above, the
 * message naming both numbers), which are sorted on the device; read 2 ranks the other class among them (counter 2 g for a
 * key strictly inside gap g, 2 g + 1 for a key equal to the g-th sorted edge key; a window of 4096 gaps in LDS chosen from a
 * coarse count at every ceil(T / 2048)-th edge key -- a read of its own, every 16th row of a matrix of >= 4096 rows -- the
 * rest by 64-bit global atomics); the host forms the distinct keys, the integer prefix sums and the monotone chain
 * (plda_rocch_hull); read 3 finds the keys next to each vertex's cut (plda_rocch_finish), 4095 cuts per read.  Integer
 * atomics only: a call is bit-reproducible.  The operand form re-scores its slabs once per read.  There is no row-sharded
 * (_comm) form: it would need the edge keys gathered.
 * PLDA_ROCCH_VARIANT (read by plda_create): 1 = no LDS window, every rank through global atomics; 2 = a window of 256 gaps.
 *
 * out / vertices[cap_vertices] / llr[cap_vertices - 1] / points / info are HOST memory; the calls synchronise the handle's
 * stream.  out is written (np, nn, n_vertices, min_cllr, eer, ...) also when the hull has more than cap_vertices vertices:
 * that is PLDA_E_CAPACITY with the needed count in out->n_vertices and the arrays untouched (cap_vertices == 0 asks for the
 * figures alone and fails the same way).  points (nullable): the caller sets cap and the five arrays; the call writes T and
 * edge_class (1: the targets are the edge class) and, when cap >= T, per distinct edge key j: edge_key, other_lt / other_le =
 * #{other-class key < / <= u_j}, edge_lt / edge_le likewise for the edge class; cap < T is PLDA_E_CAPACITY.
 *
 * plda_pav_map_dev: out[i, j] = (float) llr[segment of key(s[i, j])] from a vertex array and its llrs (HOST arrays, as the
 * calls above return them; at most 4097 vertices, PLDA_E_CAPACITY above: there is no global-table fall-back).  NaN in gives
 * that NaN out; +-inf fall into the end segments by their keys; bound > 0 clamps the table to [-bound, bound] before the
 * cast.  Layout, columns [Nt, ld_out) and the in-place rule (dout == dscores, ld_out == ld) as plda_affine_map_dev.  The
 * table is uploaded first and the stream synchronised once for it; the map itself is enqueued and not waited for. ---- */
typedef struct plda_rocch_vertex { uint64_t x, y, fa, miss; double threshold; uint32_t key; int32_t has_key; } plda_rocch_vertex;
typedef struct plda_rocch {
  uint64_t np, nn;
  int64_t n_vertices;
  double min_cllr, eer, eer_far_lo, eer_far_hi, eer_frr_lo, eer_frr_hi;
} plda_rocch;
typedef struct plda_rocch_points {
  int64_t cap, T;
  int32_t edge_class, reserved;
  uint32_t *edge_key;
  uint64_t *other_lt, *other_le, *edge_lt, *edge_le;
} plda_rocch_points;
typedef struct plda_rocch_info {
  uint64_t np, nn;
  uint64_t t_raw, t_distinct;      /* trials of the edge class; its distinct keys */
  uint64_t n_lds, n_global_atomic, n_register;   /* ranks counted in the LDS window / by global atomics / outside [u_1, u_T] */
  int64_t window_start, window_size;   /* the window's first gap and its gaps (0: none) */
  int32_t reads;                   /* passes over the scores (the coarse and the neighbour reads included) */
  int32_t launches;
  int32_t edge_class;              /* 1: targets */
  int32_t coarse_read;             /* 1: the window was chosen from a coarse count, taken in a read of its own */
  int32_t neighbour_reads;
  int32_t reserved;
} plda_rocch_info;
int plda_rocch_matrix_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *denrol_spk,
                          const int64_t *dtest_spk, int64_t cap_vertices, plda_rocch *out, plda_rocch_vertex *vertices,
                          double *llr, plda_rocch_points *points, plda_rocch_info *info);
int plda_rocch_lists(plda_handle *h, const float *pos, int64_t np, const float *neg, int64_t nn, int64_t cap_vertices,
                     plda_rocch *out, plda_rocch_vertex *vertices, double *llr, plda_rocch_points *points, plda_rocch_info *info);
int plda_score_rocch_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M,
                         const double *dV, int64_t Nt, const double *dzmean, const double *dzstd, const int64_t *denrol_spk,
                         const int64_t *dtest_spk, int64_t cap_vertices, plda_rocch *out, plda_rocch_vertex *vertices,
                         double *llr, plda_rocch_points *points, plda_rocch_info *info);
int plda_pav_map_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, int64_t n_vertices,
                     const plda_rocch_vertex *vertices, const double *llr, double bound, float *dout, int64_t ld_out);
/* The host steps as pure functions (no handle, no GPU; the pattern of plda_min_dcf_step).  plda_rocch_hull: the reduced
 * points of T >= 1 distinct ascending edge keys (edge_lt[0] == 0, edge_lt[j] == edge_le[j - 1], the last edge_le the class
 * total; anything inconsistent is PLDA_E_INVAL) -> out, the vertices and llr[n_vertices - 1].  A vertex's `key` is here the
 * EDGE of its cut -- "reject every key <= key": u_j, or u_j - 1 for the cut just below u_j, the largest word for the last
 * vertex -- and its threshold NaN.  plda_rocch_finish: below[v] = the largest key present <= that edge, above[v] = the
 * smallest key present above it (above[0]: the smallest key of all; below[0] and above[n - 1] are not read) -> key = below[v]
 * and the threshold. */
int plda_rocch_hull(int64_t T, const uint32_t *edge_key, const uint64_t *other_lt, const uint64_t *other_le,
                    const uint64_t *edge_lt, const uint64_t *edge_le, int32_t edge_class, uint64_t np, uint64_t nn,
                    int64_t cap_vertices, plda_rocch *out, plda_rocch_vertex *vertices, double *llr);
int plda_rocch_finish(int64_t n_vertices, plda_rocch_vertex *vertices, const uint32_t *below, const uint32_t *above);

/* ---- trial keys: masked trials and per-condition lists (K26; csrc/partition.hip; what BOSARIS calls a Key).  For the matrix
 * and operand forms above every one of the M x Nt pairs is a trial.  A key says which pairs are trials and which condition
 * bucket each trial belongs to, and a stable multi-way partition turns a trials matrix -- resident, or produced slab by slab
 * from the operands -- into score lists on the device, one per (bucket, class), for the device-list forms of the consumers.
 *
 * The key.  enrol_code[M] and test_code[Nt] are uint8 with values < n_enrol_codes / < n_test_codes, both
 * 1 ... PLDA_KEY_MAX_CODES.  table[n_enrol_codes * n_test_codes] is a HOST int8 array, row-major by enrol code: entry
 * (e, t) is the bucket 0 ... n_buckets - 1 of a pair with those codes, or -1: the pair is not a trial;
 * 1 <= n_buckets <= PLDA_KEY_MAX_BUCKETS.  Class as everywhere: pair (i, j) is a target (class 1) iff
 * enrol_spk[i] == test_spk[j], a non-target (class 0) otherwise.  A trial's list is L = 2 * bucket + class.  A code out of
 * range, a table entry outside [-1, n_buckets), a limit exceeded or a NULL array: PLDA_E_INVAL with a message, nothing is
 * written.
 *
 * The output.  Two device buffers of floats: dtar (class 1) and dnon (class 0).  In each, bucket 0's list comes first, then
 * bucket 1's, ..., contiguously: list (b, c) is count[b][c] scores from offset[b][c] of its class buffer, and the first
 * total[c] floats of a buffer are the POOLED list of that class, with no copy.  Nothing is written beyond total[c].
 *
 * The order (PLDA_PARTITION_STRIP = 256).  Within a list, trials are ordered by (column strip j / 256, row i, column j); for
 * Nt <= 256 that is row-major order.  The order is a function of the key, the speaker ids and the shape alone: not of the
 * scores, ld, the base pointer's alignment, the slab height of the operand form or anything the library chooses (slice
 * height, grid).  K matrices partitioned with one key therefore give aligned lists (element k of list L is the same trial
 * in each: the list forms of the fusion apply per bucket), and the fp64 sums the consumers form are reproducible to the bit.
 * Scores are copied verbatim: the bits of -0.0, of every NaN and of +-Inf arrive unchanged (refusing non-finite scores
 * stays the consumers' job); the padding columns [Nt, ld) are never read as data.
 *
 * plda_partition_plan: a pure host function (no handle, no GPU; the pattern of plda_rocch_hull; its message goes to
 * plda_last_error(NULL)).  From HOST speaker ids and a key whose code arrays are HOST arrays it fills the record in
 * O(M + Nt + n_enrol_codes * n_test_codes): the per-code counts and the table give every bucket's trials, a hash join of the
 * speaker ids gives its targets.  Callers size the buffers from total[].
 * plda_partition_matrix_dev: the key carries DEVICE code arrays (and the HOST table).  The ids and codes are brought to the
 * host, checked and planned as above; cap_tar < total[1] or cap_non < total[0] (capacities in floats; a buffer may be NULL
 * when its total is 0) is PLDA_E_INVAL before anything is written, with *plan_out filled so that the caller can size.  A
 * counting kernel then reads ids and codes only -- its grand totals must equal the plan's, anything else is PLDA_E_HIP --
 * and one kernel reads every score once and writes the selected ones.  The call synchronises for the counts; the partition
 * kernel itself is enqueued on the handle's stream and not waited for.
 * plda_score_partition_dev: the operand form (arguments as plda_score_eer_dev): the matrix is never held, only the selected
 * trials are written; its lists are bit-identical to plda_score_matrix_dev + plda_partition_matrix_dev.
 *
 * The device-list forms of the consumers (plda_*_lists_dev): each is its _lists sibling on lists that are already on the
 * device (two device pointers; the fusion's pos / neg stay HOST arrays of n_systems DEVICE pointers) -- no upload, the same
 * argument checks and messages, results bit-identical to the host form on the same values in the same order.  Outputs are
 * HOST structures and arrays as in the host forms. ---- */
#define PLDA_KEY_MAX_CODES 128
#define PLDA_KEY_MAX_BUCKETS 8
#define PLDA_PARTITION_STRIP 256
typedef struct plda_trial_key {
  const uint8_t *enrol_code, *test_code;   /* [M], [Nt]: HOST for plda_partition_plan, DEVICE for the _dev forms */
  const int8_t *table;                     /* HOST [n_enrol_codes * n_test_codes] */
  int32_t n_enrol_codes, n_test_codes, n_buckets, reserved;
} plda_trial_key;
typedef struct plda_partition_record {     /* the plan of a partition; [bucket][class], class 1 = targets */
  int64_t count[PLDA_KEY_MAX_BUCKETS][2];
  int64_t offset[PLDA_KEY_MAX_BUCKETS][2]; /* a list's start within its class buffer, in floats */
  int64_t total[2];
} plda_partition_record;
int plda_partition_plan(const int64_t *enrol_spk, int64_t M, const int64_t *test_spk, int64_t Nt, const plda_trial_key *key,
                        plda_partition_record *plan);
int plda_partition_matrix_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *denrol_spk,
                              const int64_t *dtest_spk, const plda_trial_key *key, float *dtar, int64_t cap_tar, float *dnon,
                              int64_t cap_non, plda_partition_record *plan_out);
int plda_score_partition_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M,
                             const double *dV, int64_t Nt, const double *dzmean, const double *dzstd, const int64_t *denrol_spk,
                             const int64_t *dtest_spk, const plda_trial_key *key, float *dtar, int64_t cap_tar, float *dnon,
                             int64_t cap_non, plda_partition_record *plan_out);
int plda_eer_lists_dev(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, double *out);
int plda_det_lists_dev(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, int32_t n_points, double *far,
                       double *frr, double *thresholds);
int plda_min_dcf_lists_dev(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, int32_t n_points,
                           const plda_dcf_point *points, plda_min_dcf *out, plda_min_dcf_info *info);
int plda_calib_pass_lists_dev(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, double a, double c,
                              double theta, plda_calib_record *out_record);
int plda_calib_fit_lists_dev(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, double prior, double tol,
                             int32_t max_iter, plda_calib_fit *out_fit);
int plda_rocch_lists_dev(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, int64_t cap_vertices,
                         plda_rocch *out, plda_rocch_vertex *vertices, double *llr, plda_rocch_points *points,
                         plda_rocch_info *info);
int plda_fusion_pass_lists_dev(plda_handle *h, int32_t n_systems, const float *const *dpos, int64_t np, const float *const *dneg,
                               int64_t nn, const double *a, double c, double theta, plda_fusion_record *out_record);
int plda_fusion_fit_lists_dev(plda_handle *h, int32_t n_systems, const float *const *dpos, int64_t np, const float *const *dneg,
                              int64_t nn, double prior, double tol, int32_t max_iter, plda_fusion_fit *out_fit);

/* ---- several GPUs of one node: one process per GPU, one handle per process.  The reference
 * has no counterpart (one process, one thread; its native object libplda.MPlda, pldamodule.cpp:280-295, is the only
 * thing callers bind, so the sharded path lives behind the same object).
 *
 * Every collective the library issues goes through ONE table of three operations on DEVICE pointers
 * (plda_collectives); three providers fill it:
 *   plda_comm_init         RCCL over xGMI (the default and the production transport).  librccl is opened lazily by
 *                          this call -- a single-GPU user never needs it.  Rank 0 calls plda_comm_unique_id and
 *                          distributes the 128 bytes by any means (MPI, a file, torch.distributed's store); every rank
 *                          then calls plda_comm_init (collective).
 *   plda_comm_init_host    any HOST transport (MPI, gloo, shared memory): the caller supplies the two operations on
 *                          host buffers, the library stages device data through a pinned bounce buffer in bounded
 *                          chunks.  This is also how the sharded entry points are tested with several processes on
 *                          ONE GPU (RCCL refuses two ranks on one device): tests/test_gpu_comm_procs.py.
 *   plda_comm_init_peer    direct writes over xGMI (round 4): every rank opens the others' buffers through HIP IPC and
 *                          PUSHES its piece into them with device-to-device copies, one copy stream per peer -- all 7
 *                          links of a GPU busy at once (~1.07 TB/s) where a ring moves one link's ~153 GB/s (SURVEY.md
 *                          section 5).  `bootstrap` = the host operations of plda_comm_init_host; only its
 *                          all_gather_v is used: it carries the IPC handles (72 bytes per rank and call) and is the
 *                          rendezvous the inter-process events need -- no device data crosses the host.  Works between
 *                          processes on one device too.  "transport": "peer" in plda_comm_describe.
 *   plda_comm_init_custom  the device-level table itself.
 * All callbacks return 0 on success.  Buffers are byte-addressed; `hip_stream` is the hipStream_t the operation must
 * be ordered on (enqueue, or synchronise it and work on the host).
 *
 *   plda_shard_plan                 the row partition of the trials matrix, as a pure function (no handle, no GPU):
 *       block b of `block_rows` rows (rounded up to a multiple of 256; <= 0: 4096) belongs to rank b mod R; the rows
 *       left over after the last full round of R blocks are dealt out once more in R equal smaller blocks, so the
 *       tail does not land on rank 0.  Writes this rank's blocks (first row, row count) in ascending order; a rank's
 *       COMPACT slab holds them back to back, *local_rows rows in all.
 *   plda_score_matrix_sharded_dev   every rank passes the SAME replicated inputs (all M enrol rows, all Nt tests,
 *       a replicated model) and scores the blocks plda_shard_plan gives it, straight into their final rows of the
 *       full matrix dout[M, ld_out] (which must hold M * ld_out floats).  gather == 0: that is all (scores stay
 *       sharded: what thresholding, counting, EER want; no collective).  gather != 0: every R consecutive blocks are
 *       assembled on every rank by one IN-PLACE all-gather on a side stream while the next blocks are being
 *       scored (no staging copy; ragged tail: all_gather_v); whole ld_out-wide rows travel, so the padding columns
 *       [Nt, ld_out) of dout are overwritten with unspecified values; the handle's stream is ordered behind the
 *       last one.
 *   plda_score_matrix_sharded_local_dev   the same partition with COMPACT output: this rank's blocks back to back in
 *       dlocal[local_rows, ld_local] -- a rank holds M/R rows of scores, not M (C4 on 8 GPUs: 24 GB instead of
 *       192 GB).  dfull == NULL: scores stay sharded.  dfull != NULL (needs ld_full == ld_local): the full
 *       [M, ld_full] matrix is assembled there on every rank as well, super-block by super-block, overlapped as above.
 *   plda_znorm_stats_sharded_dev    MPlda_norm (pldamodule.cpp:196-256) with the M models split contiguously
 *       over the ranks (every rank scans the whole cohort); full mean / std arrays on every rank.
 *   plda_fit_sharded_dev            MPlda_fit with the statistics pass (pldamodule.cpp:76-100) over THIS rank's
 *       speakers (local dense labels 0..K-1; a speaker's rows must all be on one rank); the D x D offset
 *       scatter is all-reduced, centroids and counts are all-gathered in rank order, and EM + GetOutput
 *       (:102-106) run as replicas on every rank from identical inputs.
 *   plda_eer_matrix_comm_dev        plda_eer_matrix_sharded_dev with the handle's collectives; the compact slab of
 *       plda_score_matrix_sharded_local_dev (with the speaker ids of ITS rows) is what it takes.
 *   plda_min_dcf_matrix_comm_dev    the same for the minimum detection cost (plda_min_dcf_matrix_dev).
 * Without a communicator all of them run as a single rank. ---- */
#define PLDA_DT_F64 0
#define PLDA_DT_U64 1
#define PLDA_DT_U32 2
#define PLDA_OP_SUM 0
#define PLDA_OP_MAX 1
#define PLDA_OP_MIN 2
typedef struct plda_collectives {
  void *ctx;
  /* every rank contributes `bytes` at dsend; drecv receives nranks * bytes in rank order.  dsend may be
   * drecv + rank * bytes (in place). */
  int (*all_gather)(void *ctx, const void *dsend, void *drecv, int64_t bytes, void *hip_stream);
  /* ragged, in place: rank q owns bytes [offs[q], offs[q] + counts[q]) of the same dbuf on every rank (counts may be
   * 0); afterwards every rank holds every piece.  offs / counts: nranks host int64 each, identical on all ranks. */
  int (*all_gather_v)(void *ctx, void *dbuf, const int64_t *offs, const int64_t *counts, void *hip_stream);
  /* element-wise, in place: dtype PLDA_DT_*, op PLDA_OP_* */
  int (*all_reduce)(void *ctx, void *dbuf, int64_t count, int32_t dtype, int32_t op, void *hip_stream);
  /* called once by plda_comm_destroy / plda_destroy; may be NULL */
  void (*destroy)(void *ctx);
} plda_collectives;
typedef struct plda_host_collectives {
  void *ctx;
  /* the same two operations on HOST memory (the library's pinned bounce buffer), blocking */
  int (*all_gather_v)(void *ctx, void *hbuf, const int64_t *offs, const int64_t *counts);
  int (*all_reduce)(void *ctx, void *hbuf, int64_t count, int32_t dtype, int32_t op);
  void (*destroy)(void *ctx);
} plda_host_collectives;
int plda_comm_unique_id(void *out, int64_t cap_bytes /* >= 128 */);
int plda_comm_init(plda_handle *h, int32_t nranks, int32_t rank, const void *unique_id);
int plda_comm_init_custom(plda_handle *h, int32_t nranks, int32_t rank, const plda_collectives *table);
int plda_comm_init_host(plda_handle *h, int32_t nranks, int32_t rank, const plda_host_collectives *table);
int plda_comm_init_peer(plda_handle *h, int32_t nranks, int32_t rank, const plda_host_collectives *bootstrap);
int plda_comm_destroy(plda_handle *h);
int plda_comm_info(plda_handle *h, int32_t *nranks, int32_t *rank);
/* who takes part, as the TRANSPORT reports it, written as a JSON object into json[cap]: {"transport": "rccl" | "host"
 * | "peer" | "custom" | "none" | "emulated", "nranks", "rank", "device", "pci_bus_id"}; for RCCL nranks / rank / device come
 * from ncclCommCount / ncclCommUserRank / ncclCommCuDevice (plus "rccl_version"), not from what the caller passed in */
int plda_comm_describe(plda_handle *h, char *json, int64_t cap);
/* test hook: act as rank `rank` of `nranks` WITHOUT a communicator (no collective runs, gather is ignored):
 * lets one GPU play every rank in turn and check that the shards tile the whole problem */
int plda_comm_emulate(plda_handle *h, int32_t nranks, int32_t rank);
int plda_shard_plan(int64_t M, int32_t nranks, int32_t rank, int64_t block_rows, int64_t *row_start,
                    int64_t *row_count, int64_t cap, int64_t *nblocks, int64_t *local_rows);
int plda_score_matrix_sharded_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform,
                                  int64_t M, const double *dV, int64_t Nt, const double *dzmean,
                                  const double *dzstd, float *dout, int64_t ld_out, int64_t block_rows,
                                  int32_t gather);
int plda_score_matrix_sharded_local_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform,
                                        int64_t M, const double *dV, int64_t Nt, const double *dzmean,
                                        const double *dzstd, float *dlocal, int64_t ld_local, int64_t block_rows,
                                        float *dfull, int64_t ld_full);
int plda_znorm_stats_sharded_dev(plda_handle *h, const double *dbkg, int64_t Nb, int32_t num_examples,
                                 int32_t Din, const double *dmodels, int64_t M, double *dout_mean,
                                 double *dout_std);
/* plda_cohort_stats_dev with the R rows split contiguously over the ranks exactly like plda_znorm_stats_sharded_dev (every rank
 * passes ALL rows and the whole cohort); one all-gather of the two fp64 result vectors: every rank ends with all R results,
 * bit-identical to the single-rank call. */
int plda_cohort_stats_sharded_dev(plda_handle *h, const double *dX, const int32_t *dn, int32_t n_uniform, int64_t R,
                                  const double *dC, int64_t Nc, int64_t top_k, double *dmean, double *dstd);
int plda_fit_sharded_dev(plda_handle *h, const double *dX, int64_t N, int32_t D, const uint64_t *dlabels,
                         int64_t K, int32_t iters);
int plda_eer_matrix_comm_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt,
                             const int64_t *denrol_spk, const int64_t *dtest_spk, double *out);
/* plda_min_dcf_matrix_dev of a row-sharded matrix (arguments as above; M == 0 is allowed: a rank that owns no row still takes
 * part).  Every rank gets the global result.  A rank that fails keeps its peers out of a blocked collective by the
 * poisoned-histogram protocol of the sharded EER. */
int plda_min_dcf_matrix_comm_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt,
                                 const int64_t *denrol_spk, const int64_t *dtest_spk, int32_t n_points,
                                 const plda_dcf_point *points, plda_min_dcf *out, plda_min_dcf_info *info);

/* ---- PLDA domain adaptation (K14): moving the model on the handle -- the Kaldi `Plda` held at pldamodule.cpp:29 -- onto
 * another domain, without labels (unsupervised adaptation) or by interpolation with a second model (supervised).  The
 * reference has NO counterpart: it can only refit.  The unsupervised update restates Kaldi's PldaUnsupervisedAdaptor
 * (ivector/plda.h, the class behind ivector-adapt-plda) and its defaults from the published algorithm; PARITY UNPINNED, like
 * the rest of the PLDA path (no Kaldi build to compare with).  All fp64.
 *
 * The model is (mean m [D], transform T [D, D], psi [D]); its covariances are within-class W = (T^T T)^-1, between-class
 * B = T^-1 diag(psi) T^-T, total W + B.  Adaptation needs the SQUARE model: on a handle truncated with plda_truncate
 * (Dout < Din) every entry point below returns PLDA_E_INVAL ("adapt before truncating").
 *
 * Statistics.  The pilot p is the model mean at the first accumulation after a reset.  Over the rows x_i [Din] with weights
 * w_i >= 0 (NULL: 1) the record is  tw = sum w_i,  rows = the number of rows,  S1 = sum w_i (x_i - p),
 * S2 = sum w_i (x_i - p)(x_i - p)^T  (symmetric, both triangles stored)  and p itself.  The sums are taken about p, not about
 * 0 as Kaldi's AddStats takes them: the variance then does not come out of the cancellation sum x x^T / tw - mean mean^T
 * (at D = 24, 4000 rows of unit spread offset by 1e5 that form loses 7e-5 of the variance, this one 4e-16).  The record adds
 * over calls, and with an equal pilot over handles and ranks (plda_adapt_get_stats / plda_adapt_add_stats; no collective
 * is built in).  The rows are read once, slab by slab: each slab is written as centred rows [x - p | 1] into a bounded
 * buffer and multiplied by the weighted fp64 SYRK of the fit's statistics pass, the augmented column giving S2, S1 and tw in
 * one product; the slabs' results are added in the order of the rows.  Rows per slab: 64 MiB of centred rows, at most 65 536
 * rows; PLDA_ADAPT_SLAB_ROWS in the environment at plda_create overrides it.  The record of a call is bit-identical from
 * run to run (no floating-point atomics); the device scratch of a call does not grow with N.
 *
 * Update with (within_scale ws, between_scale bs, mean_diff_scale mds; Kaldi's defaults 0.3 / 0.7 / 1.0):
 *   1. delta = S1 / tw, mean' = p + delta
 *   2. V = S2 / tw - (1 - mds) delta delta^T      (Kaldi's centred variance + mds delta delta^T; mds = 1: S2 / tw exactly)
 *   3. Tm = diag(1 / sqrt(1 + psi)) T             (the basis in which the model's total covariance is the identity)
 *   4. Vp = Tm V Tm^T, symmetrised, = P diag(s) P^T, s descending
 *   5. e_i = max(s_i - 1, 0)                      (the variance the data shows beyond the model's)
 *   6. E = Tm^-1 P diag(e) P^T Tm^-T,  Tm^-1 = W T^T diag(sqrt(1 + psi))
 *   7. W' = W + ws E,  B' = B + bs E
 * and the new model is mean', (transform, psi) = the simultaneous diagonalisation of (W', B') exactly as the fit's GetOutput
 * makes it (Cholesky whitening of W', eigenvalues descending, floored at 0), offset refreshed.  (Kaldi adds ws e and bs e to
 * the diagonals of P^T diag(1 / (1 + psi)) P and P^T diag(psi / (1 + psi)) P and maps back with (P^T Tm)^-1: the same thing;
 * the form above leaves the unchanged part alone and needs only the SPD inverse.)
 * Blend with a second model (mean2, T2, psi2) of the same D and alpha, alpha_mean in [0, 1]:  W' = (1 - alpha) W + alpha W2,
 * B' likewise, mean' = (1 - alpha_mean) m + alpha_mean mean2, the new model their simultaneous diagonalisation.
 *
 * Both enqueue their whole chain of D x D products, the SPD inverse, the eigensolver and the diagonalisation without a host
 * round trip and synchronise once to read the status words, the eigenvalues and the new model (then once more for the
 * refreshed offset, as plda_smooth does).  On any failure (a factorisation flag, the eigensolver) the OLD model stays
 * installed, untouched, and PLDA_E_NUMERIC is returned.  On success the handle behaves as after plda_set_model: a test side
 * prepared with plda_score_prepare_dev is dropped, plda_score_one sees the new model.  Update and blend are supported up to
 * D = 2048, the limit of the direct eigensolver (its fallback, block Jacobi, stops at 1024); a larger model is PLDA_E_INVAL,
 * checked before any work.  The statistics entry points have no such limit.
 *
 *   plda_adapt_reset            forgets the record (the next accumulation takes the pilot anew)
 *   plda_adapt_accumulate_dev   dX [N, Din] and dweights [N] (nullable) in HBM; plda_adapt_accumulate: the same from host
 *                               memory.  Both synchronise (they report rejected rows).  N == 0: nothing happens.  N < 0, a Din
 *                               that is not the model's, a model that is not fitted (PLDA_E_NOT_FITTED) or truncated: an
 *                               error.  A non-finite row or a negative / non-finite weight: PLDA_E_INVAL with the counts in
 *                               plda_last_error, the record left as it was before the call.  A record taken under an
 *                               earlier model (the model changed since the pilot): PLDA_E_INVAL ("reset first").
 *   plda_adapt_get_stats        host outputs, any NULL: tw, rows, pilot [D], s1 [D], s2 [D, D] (an empty record: zeros, the
 *                               pilot that would be taken).  D is the MODEL's dimension, which is what the caller can size
 *                               its arrays from: a record whose dimension differs from the model's (the model was replaced by
 *                               one of another D since the pilot) is PLDA_E_INVAL ("reset first") and nothing is written.  A
 *                               record of an earlier model of the same D stays readable.
 *   plda_adapt_add_stats        adds the record of another handle or rank.  Its pilot must equal this record's bit for bit
 *                               (PLDA_E_INVAL otherwise); an empty record adopts it only if it equals the model mean.
 *   plda_adapt_update           eig [D] (host, nullable) receives s; info (nullable) the summary below.  tw <= 0, a negative
 *                               or non-finite scale, or a second update on the same record: PLDA_E_INVAL.
 *   plda_blend_model            host arrays, as plda_set_model takes them ---- */
typedef struct {
  double tot_weight;    /* tw */
  int64_t rows;
  int32_t dim;          /* D */
  int32_t n_excess;     /* number of s_i > 1 */
  double eig_max;       /* s_0 */
  double eig_min;       /* s_{D-1} */
  double mean_shift;    /* ||delta||_2 */
} plda_adapt_info;
int plda_adapt_reset(plda_handle *h);
int plda_adapt_accumulate_dev(plda_handle *h, const double *dX, int64_t N, int32_t Din, const double *dweights);
int plda_adapt_accumulate(plda_handle *h, const double *X, int64_t N, int32_t Din, const double *weights);
int plda_adapt_get_stats(plda_handle *h, double *tw, int64_t *rows, double *pilot, double *s1, double *s2);
int plda_adapt_add_stats(plda_handle *h, double tw, int64_t rows, const double *pilot, const double *s1,
                         const double *s2);
int plda_adapt_update(plda_handle *h, double within_scale, double between_scale, double mean_diff_scale,
                      double *eig, plda_adapt_info *info);
int plda_blend_model(plda_handle *h, int32_t D, const double *mean2, const double *transform2, const double *psi2,
                     double alpha, double alpha_mean);

/* ---- speaker clustering (K15; csrc/ahc.hip): batched average-linkage agglomerative clustering (AHC / UPGMA) on PLDA score
 * blocks -- the diarisation use of a PLDA back-end (Kaldi: ivector-plda-scoring-dense + agglomerative-cluster).  The reference
 * has NO counterpart (it verifies, it does not cluster), so this is the project's own extension: tests/ahc_model.py pins it to
 * the bit.
 *
 * A RECORDING r is a run of N = offsets[r+1] - offsets[r] consecutive segments, 1 <= N <= PLDA_AHC_MAX.  Its input is an fp32
 * score block S [N, N], row-major.  The diagonal is never read.
 *
 * COST.  c(i, j) = -((double)S[i, j] + (double)S[j, i]) / 2 for i != j; both steps are exact in fp64.  (The two fp32
 * triangles of a PLDA block differ in their last bits, so the block is symmetrised, not half-read.)  A non-finite
 * off-diagonal score fails the call with PLDA_E_INVAL and the count in plda_last_error, as a calibration pass does; the
 * outputs of such a call are unspecified.
 *
 * STATE.  Clusters live in slots; a cluster's slot is its smallest member index.  Every pair of live slots a < b holds
 * sum(a, b), the fp64 sum of c over the size(a) * size(b) cross pairs.  At the start sum(i, j) = c(i, j), every size is 1 and
 * k = N slots are live.
 *
 * ONE STEP.  The candidate value of a pair is v(a, b) = sum(a, b) / (double)(size(a) * size(b)): the integer product, one
 * conversion, one IEEE fp64 division (no fast-math, no reciprocal).  The pair to merge is the minimum under the total order
 * v ascending, then a ascending, then b ascending; -0.0 == +0.0.  The step STOPS the recording if k <= max(1, min_clusters[r]),
 * or if has_threshold != 0 and !(v <= -(double)threshold) (a score threshold: pairs whose average score is at least the
 * threshold merge).  Otherwise, for every other live slot x, sum(a, x) <- sum(a, x) + sum(b, x) -- one fp64 addition with the
 * operands in that order -- then size(a) += size(b), slot b dies and k drops by one.  This is average linkage on sums, as
 * Kaldi keeps them.  The result is fully determined by the input bits: it does not depend on the grid, on how recordings are
 * grouped into launches, or on the run.
 *
 * OUTPUTS.  labels int32 [T], T = offsets[R]: within a recording the clusters are numbered 0 .. k-1 by ascending slot.
 * n_clusters int32 [R].  The merge record is nullable -- pass all three of its pointers or none (one alone: PLDA_E_INVAL):
 * merge_a, merge_b int32 and merge_cost fp64, each [T - R]; recording r owns entries [offsets[r] - r, offsets[r+1] - r - 1):
 * the merges made come first, in order, with cost = v; the unused tail holds -1, -1, +inf.  Nothing else is written.
 *
 * METHOD.  One workgroup per recording, in two dispatch classes: the LDS class holds the strict upper triangle of the sums in
 * LDS, the HBM class an N x N fp64 matrix in handle scratch (N * N * 8 bytes per recording in flight); both keep a per-slot
 * cache (best partner b > a and its v) in LDS, so a step is a workgroup reduction over the cache, an update of row and column
 * a, and a rescan of only the rows whose cached partner was a or b.  The LDS class takes the largest N whose triangle and
 * cache fit the 160 KiB of one compute unit.  The recordings of a call are grouped into launches so that the HBM-class scratch
 * of a launch stays within 2 GiB (never fewer than one recording; PLDA_AHC_SCRATCH_BYTES in the environment at plda_create
 * sets another budget: tests); the scratch belongs to the handle and is freed by plda_destroy.
 *
 *   plda_ahc_plan         out[0] = the class of a recording of N segments (0 LDS, 1 HBM), out[1] = the scratch bytes one
 *                         such recording takes (0 in the LDS class), out[2] = the largest N of the LDS class.
 *   plda_ahc_matrix_dev   packed blocks in HBM: block r starts at dscores + block_off[r], row-major N_r x N_r.  block_off
 *                         [R + 1] (in floats), offsets [R + 1] and min_clusters [R] (nullable: 1 everywhere) are HOST arrays
 *                         (the host sizes the launches from them; the convention of the fusion's pointer arrays); scores and
 *                         outputs are in HBM.  PLDA_E_INVAL: offsets that do not ascend from 0, a recording that is empty or
 *                         above PLDA_AHC_MAX, block_off[r+1] - block_off[r] < N_r * N_r, min_clusters[r] < 1.  Enqueues on the
 *                         handle's stream and synchronises it once, to read the count of non-finite scores (as the
 *                         calibration's _dev forms do).
 *   plda_ahc_matrix       the same with scores and outputs in host memory.
 *   plda_score_ahc*       the operand form: X [T, Dout] holds already-transformed segment vectors (num_examples = 1).  The
 *                         block of recording r is what plda_score_matrix_dev(X_r, NULL, 1, N_r, X_r, N_r, NULL, NULL, ..,
 *                         ld_out = N_r) writes, bit for bit: it comes from that same enqueue path, one call per recording,
 *                         into the S-norm slab buffer, as many consecutive recordings at a time as the budget above holds
 *                         (each block at a 256-byte boundary), clustered, dropped.  A prepared test side is dropped, as in
 *                         plda_cohort_stats_dev.
 * OUT OF SCOPE, each on purpose: Kaldi's per-recording mean subtraction; its two-pass clustering of very long recordings;
 * one problem above PLDA_AHC_WIDE_MAX = 32768 vectors; one problem on more than one GPU.  (Several workgroups on one problem,
 * for N above PLDA_AHC_MAX, are the section "corpus-scale clustering" below.)  (The per-recording PCA before scoring is the
 * section after it.)  (DER is the section "diarisation error rate" below; RTTM files are
 * read and written by plda_amd/rttm.py, on the host.) ---- */
#define PLDA_AHC_MAX 4096
int plda_ahc_plan(plda_handle *h, int64_t N, int32_t out[3]);
int plda_ahc_matrix_dev(plda_handle *h, const float *dscores, const int64_t *block_off, const int64_t *offsets, int64_t R,
                        int32_t has_threshold, double threshold, const int32_t *min_clusters, int32_t *dlabels,
                        int32_t *dn_clusters, int32_t *dmerge_a, int32_t *dmerge_b, double *dmerge_cost);
int plda_ahc_matrix(plda_handle *h, const float *scores, const int64_t *block_off, const int64_t *offsets, int64_t R,
                    int32_t has_threshold, double threshold, const int32_t *min_clusters, int32_t *labels, int32_t *n_clusters,
                    int32_t *merge_a, int32_t *merge_b, double *merge_cost);
int plda_score_ahc_dev(plda_handle *h, const double *dX, const int64_t *offsets, int64_t R, int32_t has_threshold,
                       double threshold, const int32_t *min_clusters, int32_t *dlabels, int32_t *dn_clusters,
                       int32_t *dmerge_a, int32_t *dmerge_b, double *dmerge_cost);
int plda_score_ahc(plda_handle *h, const double *X, const int64_t *offsets, int64_t R, int32_t has_threshold, double threshold,
                   const int32_t *min_clusters, int32_t *labels, int32_t *n_clusters, int32_t *merge_a, int32_t *merge_b,
                   double *merge_cost);

/* ---- corpus-scale clustering (K28; csrc/ahc.hip, the "wide" class): ONE clustering problem of N vectors, 1 <= N <=
 * PLDA_AHC_WIDE_MAX, spread over the whole device -- the first step of clustering-based domain adaptation (Garcia-Romero et
 * al. 2014: cluster the unlabelled in-domain corpus with the out-of-domain model, fit a model on the pseudo-labels,
 * interpolate), and recordings longer than PLDA_AHC_MAX segments.
 *
 * The CONTRACT is that of "speaker clustering" above with R = 1, word for word: the cost c(i, j), sums updated by one fp64
 * addition with the operands in that order, v = one IEEE division by the integer product of the sizes (below 2^28 at this N),
 * the order (v, a, b) with -0.0 == +0.0, the stop rule, labels by ascending slot, the merge record [N - 1] with its -1 / -1 /
 * +inf tail, and the failure on a non-finite off-diagonal score with the count.  tests/ahc_model.py is the model of both; at
 * N <= PLDA_AHC_MAX the wide class and the one-workgroup classes give the same bits.
 *
 * METHOD.  The state lives in handle scratch (one layout list in the clustering scratch buffer: the operand form's fp32 block,
 * 4 N^2 bytes; the N x N fp64 sums, 8 N^2 bytes -- 8 GiB at the maximum; sizes; the row cache, best partner b > a and its v;
 * parents; the rescan list; the row scans' partial results; the control words with the merge cursor), freed by plda_destroy.
 * A STEP is three launches, and launch boundaries are the only synchronisation between workgroups: SELECT (one workgroup: the
 * minimum of the row cache under (v, a), the stop rule -- a stop sets a device-side `done` word --, the merge entry, sizes,
 * parent[b] = a), UPDATE (a grid over x: sum(a, x) += sum(b, x) into row a and column a; a row whose cached partner was a or b
 * is appended to the rescan list, any other row x < a takes v(x, a) if it wins), RESCAN (a grid striding over the list and
 * row a; a row is scanned in a fixed number of column pieces, each by one workgroup, and the workgroup that finishes a row's
 * last piece combines them in piece order -- nobody waits).  Every kernel returns at once when `done` is set.  No workgroup
 * waits on another inside a launch; every loop is bounded by N.  With a threshold the host enqueues a batch of steps and then
 * reads `done`; when only a cluster count stops the run the number of steps is known and nothing is read until the end.  The
 * final slot of every vector comes from the parents (parent[b] = a < b) by pointer jumping, then the label rule.
 *
 *   plda_ahc_wide_plan        out[0] = the scratch bytes of the matrix form at N (the operand form adds 4 N^2), out[1] = the
 *                             launches per step, out[2] = the steps per host check, out[3] = the pieces a row scan is split
 *                             into.  PLDA_AHC_WIDE_BATCH and PLDA_AHC_WIDE_PIECES in the environment at plda_create set the
 *                             last two (tests; 1 ... 65536 and 1 ... 64, anything else: the default); the result depends on
 *                             neither.
 *   plda_ahc_wide_matrix_dev  the fp32 block in HBM, row-major N x N with row stride ld >= N (in floats); min_clusters is ONE
 *                             value >= 1; outputs in HBM: labels [N], n_clusters [1], the nullable merge record [N - 1].
 *                             Takes EVERY N from 1 up and always runs the wide class.  PLDA_E_INVAL: N < 1 or N >
 *                             PLDA_AHC_WIDE_MAX, ld < N, a NaN threshold, min_clusters < 1, one or two of the three merge
 *                             pointers.  Synchronises the stream at every host check and once at the end.
 *   plda_ahc_wide_matrix      the same with scores and outputs in host memory.
 *   plda_score_ahc_wide*      the operand form: X [N, Dout] already-transformed vectors (num_examples = 1).  The block is what
 *                             plda_score_matrix_dev(X, NULL, 1, N, X, N, NULL, NULL, .., ld_out = N) writes, bit for bit,
 *                             scored into the class's own block array (not the S-norm slab: its 2 GiB rule does not fit),
 *                             clustered, dropped.  A cosine handle takes the same path.  A prepared test side is dropped.
 * OUT OF SCOPE: see "speaker clustering". ---- */
#define PLDA_AHC_WIDE_MAX 32768
int plda_ahc_wide_plan(plda_handle *h, int64_t N, int64_t out[4]);
int plda_ahc_wide_matrix_dev(plda_handle *h, const float *dscores, int64_t N, int64_t ld, int32_t has_threshold, double threshold,
                             int32_t min_clusters, int32_t *dlabels, int32_t *dn_clusters, int32_t *dmerge_a, int32_t *dmerge_b,
                             double *dmerge_cost);
int plda_ahc_wide_matrix(plda_handle *h, const float *scores, int64_t N, int64_t ld, int32_t has_threshold, double threshold,
                         int32_t min_clusters, int32_t *labels, int32_t *n_clusters, int32_t *merge_a, int32_t *merge_b,
                         double *merge_cost);
int plda_score_ahc_wide_dev(plda_handle *h, const double *dX, int64_t N, int32_t has_threshold, double threshold,
                            int32_t min_clusters, int32_t *dlabels, int32_t *dn_clusters, int32_t *dmerge_a, int32_t *dmerge_b,
                            double *dmerge_cost);
int plda_score_ahc_wide(plda_handle *h, const double *X, int64_t N, int32_t has_threshold, double threshold, int32_t min_clusters,
                        int32_t *labels, int32_t *n_clusters, int32_t *merge_a, int32_t *merge_b, double *merge_cost);

/* ---- spectral clustering with auto-tuned pruning (K24; csrc/spectral.hip): the clusterer that needs no threshold and no
 * development set -- a pruned k-nearest-neighbour affinity graph, the speaker count from the largest eigengap of its
 * Laplacian, the pruning value by the normalised-maximum-eigengap rule (NME-SC; Park et al. 2020), k-means on the spectral
 * embedding.  Only the ORDER of the scores within a row matters, so PLDA LLRs, the PCA blocks of the next section and cosine
 * similarities are treated alike.  The reference has NO counterpart; tests/spectral_model.py is the NumPy model.
 *
 * A RECORDING r is a run of N = offsets[r+1] - offsets[r] consecutive segments, 1 <= N <= PLDA_SPECTRAL_MAX (the direct
 * eigensolver's limit).  Its input is an fp32 score block S [N, N], row-major, in the format of "speaker clustering" above.
 *
 * 1 SIMILARITY.  c(i, j) = ((double)S[i, j] + (double)S[j, i]) / 2 for i != j, exact.  The diagonal is never read.  A
 *   non-finite off-diagonal score fails the call with PLDA_E_INVAL and the count in plda_last_error; nothing is written (the
 *   count is read before anything else is enqueued; the operand form scores a call of several slabs twice for that).
 * 2 GRAPH at pruning value p.  p_eff = min(p, N - 1).  Row i keeps its p_eff best partners j != i under the total order
 *   (c descending, j ascending), -0.0 == +0.0: B[i, j] = 1 for those, else 0.  A = (B + B^T) / 2 (entries 0, 1/2, 1; diagonal
 *   0), deg_i = sum_j A[i, j], L = diag(deg) - A.  Exact, a function of the input bits alone.
 * 3 SPECTRUM.  The eigenvalues of L ascending, l_1 <= ... <= l_N, as the library's fp64 eigensolver returns them (floored at
 *   0: L is positive semi-definite).  K' = min(max_speakers, N - 1), 1 <= max_speakers <= PLDA_SPECTRAL_MAX_SPK (the VBx's
 *   label limit).  e_k = l_{k+1} - l_k for k = 1 .. K'; k_gap = the smallest k whose gap is maximal; g = e_{k_gap} /
 *   (l_N + 1e-10); r = (double)p_eff / g, +inf if g <= 0.  Plain fp64, one operation each, IEEE < and ==.
 * 4 SWEEP.  Row r of p_table [R, P] holds the recording's P pruning values (1 <= P <= PLDA_SPECTRAL_MAX_P, every value >= 1,
 *   duplicates allowed; equal p_eff are solved once).  The value used is the one of the smallest r, ties to the smaller p_eff,
 *   then to the earlier position.  k = min(num_speakers[r], N) when num_speakers is given and > 0 (it may not exceed
 *   max_speakers), else k_gap at the value used.
 * 5 EMBEDDING.  U [N, k]: the eigenvectors of the k smallest eigenvalues at the value used (kept from the sweep: nothing is
 *   solved twice), no row normalisation.
 * 6 K-MEANS, to the operation.  d(i, m) = sum_c (u_ic - m_c)^2, c ascending, fp64, the product and the sum unfused.  Centre 0 =
 *   row 0; every further centre is the row with the largest minimum d to the centres so far, ties to the lowest row.  A Lloyd
 *   step sends every row to its nearest centre (ties to the lowest centre); if no row moved (every row moves in the first
 *   step) the iteration stops, else every centre with members becomes (sum_i u_ic, i ascending from 0.0) / (double)count -- an
 *   empty centre keeps its place -- and the next step follows, max_iters steps at most (1 ... 1000).  Labels are renumbered
 *   0 .. by first occurrence; n_clusters = the number of distinct labels.
 *   N = 1: one cluster, no eigenproblem: label 0, p_used 0, k_gap 1, eigenvalue 0, embedding 1.0, deg2 0.
 *
 * A recording's outputs are bit-identical alone, in any batch, under any grouping into launches and from run to run: every
 * dispatch depends on N (and, in the k-means, on k) only, and the two k-means classes run the same operations in the same order.
 *
 * OUTPUTS.  labels int32 [T], n_clusters int32 [R].  Nullable: p_used int32 [R] (the p_eff used), k_gap int32 [R]; eig fp64
 * [R, P, max_speakers + 2]: per pruning value the min(max_speakers + 1, N) smallest eigenvalues ascending, +inf behind them,
 * l_N in the last slot; embed fp64 [T, max_speakers]: a row's first k entries are its embedding, the rest +0.0; deg2 int32 [T]
 * = 2 deg at the value used.  Nothing else is written.
 *
 * METHOD.  Per recording: the symmetrised block once; per distinct p_eff a selection kernel (one wave per row, the row's
 * order keys in registers, the p-th largest key by bisection over the key bits, then the j-ascending cut among its equals),
 * the Laplacian from the two cuts of every pair, the library's fp64 eigensolver (direct up to PLDA_SPECTRAL_MAX, one problem
 * at a time; it synchronises the stream once per problem), and a kernel that forms r and keeps the columns if it is the best
 * so far.  Per group of recordings one k-means launch, one workgroup per recording, the embedding in LDS where N k doubles
 * fit 64 KiB and read from scratch above.  The scratch belongs to the handle (freed by plda_destroy); the kept columns of a
 * group and the operand form's score slab stay within the AHC's budget (2 GiB; PLDA_AHC_SCRATCH_BYTES), never fewer than one
 * recording.
 *
 *   plda_spectral_plan        out[0] = keys per lane of the selection kernel for N (1, 2, 4 ... 32), out[1] = the largest N of
 *                             that class, out[2] = the k-means class of (N, k) (0 LDS, 1 scratch), out[3] = the largest N of
 *                             class 0 at this k, out[4] = the scratch bytes of one eigenproblem of order N.
 *   plda_spectral_matrix_dev  packed blocks in HBM as plda_ahc_matrix_dev takes them.  block_off [R + 1], offsets [R + 1],
 *                             p_table [R, P] and num_speakers [R] (nullable: k_gap everywhere) are HOST arrays.
 *   plda_spectral_matrix      the same with scores and outputs in host memory.
 *   plda_score_spectral*      the operand form: X [T, Dout] transformed segment vectors; the blocks come from the enqueue path
 *                             and the slab walk of plda_score_ahc*, bit for bit what plda_score_matrix_dev writes.
 * ERRORS.  PLDA_E_INVAL: the argument errors of plda_ahc_matrix_dev; a recording above PLDA_SPECTRAL_MAX; P, max_speakers or
 * max_iters out of range; a p < 1; num_speakers[r] < 0 or > max_speakers -- all before any device work.  PLDA_E_NUMERIC: the
 * eigensolver gave up; the message names the recording (outputs of earlier groups may have been written).
 * OUT OF SCOPE, each on purpose: a batched eigensolver for many small recordings and an eigenvalues-only sweep (what they
 * would be worth: scripts/spectral_bench.py's eigensolver share); recordings above 2048 (only the block Jacobi is left there);
 * a normalised Laplacian; a device-resident chain from the per-recording PCA. ---- */
#define PLDA_SPECTRAL_MAX 2048
#define PLDA_SPECTRAL_MAX_SPK 64
#define PLDA_SPECTRAL_MAX_P 16
int plda_spectral_plan(plda_handle *h, int64_t N, int32_t k, int32_t out[5]);
int plda_spectral_matrix_dev(plda_handle *h, const float *dscores, const int64_t *block_off, const int64_t *offsets, int64_t R,
                             const int32_t *p_table, int32_t P, int32_t max_speakers, const int32_t *num_speakers, int32_t max_iters,
                             int32_t *dlabels, int32_t *dn_clusters, int32_t *dp_used, int32_t *dk_gap, double *deig, double *dembed,
                             int32_t *ddeg2);
int plda_spectral_matrix(plda_handle *h, const float *scores, const int64_t *block_off, const int64_t *offsets, int64_t R,
                         const int32_t *p_table, int32_t P, int32_t max_speakers, const int32_t *num_speakers, int32_t max_iters,
                         int32_t *labels, int32_t *n_clusters, int32_t *p_used, int32_t *k_gap, double *eig, double *embed,
                         int32_t *deg2);
int plda_score_spectral_dev(plda_handle *h, const double *dX, const int64_t *offsets, int64_t R, const int32_t *p_table, int32_t P,
                            int32_t max_speakers, const int32_t *num_speakers, int32_t max_iters, int32_t *dlabels,
                            int32_t *dn_clusters, int32_t *dp_used, int32_t *dk_gap, double *deig, double *dembed, int32_t *ddeg2);
int plda_score_spectral(plda_handle *h, const double *X, const int64_t *offsets, int64_t R, const int32_t *p_table, int32_t P,
                        int32_t max_speakers, const int32_t *num_speakers, int32_t max_iters, int32_t *labels, int32_t *n_clusters,
                        int32_t *p_used, int32_t *k_gap, double *eig, double *embed, int32_t *deg2);

/* ---- dense scoring in a recording's PCA subspace (K19; csrc/dense_pca.hip): Kaldi's ivector-plda-scoring-dense
 * --target-energy=t restated (EstPca, Plda::ApplyTransform, TransformIvector, LogLikelihoodRatio; parity unpinned like the rest
 * of PLDA).  The reference has NO counterpart; tests/dense_pca_model.py is the NumPy model.  Everything is fp64; a score is
 * rounded to fp32 once.
 *
 * The model (mean, transform T [D, D], psi) must be untruncated, Dout = Din = D <= PLDA_DENSE_PCA_MAX_DIM.  Once per model:
 * W = T^-1 T^-T and B = T^-1 diag(psi) T^-T (the domain adaptation's routine, kept on the handle until the model changes).
 *
 * A RECORDING r owns rows offsets[r] .. offsets[r+1] of X [T, D], in the model's INPUT space, 1 <= N <= PLDA_AHC_MAX.
 *   1. mu = the mean of its rows, formed as x_0 + mean(x_i - x_0) so that equal rows centre to exact zeros;
 *      C = (1 / N) sum (x_i - mu)(x_i - mu)^T from the centred rows.  m = min(N, D).  For N <= D the solver works on the Gram
 *      matrix G = (1 / N) Xc Xc^T [N, N], which has the same non-zero eigenvalues; the eigenvectors of C are then
 *      p_k = Xc^T u_k / sqrt(N lam_k).
 *   2. lam_1 >= ... >= lam_m (floored at 0), E = their sum in that order; the rank is rho = #{k : lam_k > 2^-40 lam_1}.
 *   3. Kaldi's rule to the letter: dim = 1, energy = 0; while energy / E <= target_energy: energy += lam[dim - 1], dim++ (one
 *      more than the smallest count whose energy share exceeds the target).  d = min(dim, rho): where Kaldi would keep a
 *      direction of zero variance that its SVD picks arbitrarily, it is DROPPED here.  E = 0 (N = 1, or all rows equal):
 *      d = 0 and the whole block is +0.0f.
 *   4. P [d, D]: the d leading eigenvectors as rows.
 *   5. W' = P W P^T, B' = P B P^T (each symmetrised); Cholesky W' = L L^T; L^-1 B' L^-T = U diag(psi') U^T, psi' descending;
 *      M = U^T L^-1 P [d, D].  W' not positive definite: PLDA_E_NUMERIC naming the (first such) recording.
 *   6. y_i = M (x_i - mean), scaled by sqrt(d / sum_k y_ik^2 / (psi'_k + 1)): plda_transform_rows with num_examples = 1.
 *   7. S[i, j] = LogLikelihoodRatio(enrol y_i with n = 1, test y_j), the diagonal like any other entry; no z-norm, no
 *      calibration.  The block is stored row-major N x N at dscores + block_off[r], the format plda_ahc_matrix_dev reads.
 * The scores depend on the retained subspace only, not on the basis inside it; with d = D they are the full model's.
 *
 * METHOD.  One workgroup per recording runs steps 1 to 7 in one kernel.  Both eigenproblems (order m, then order d) go through
 * one routine, a two-sided cyclic Jacobi in round-robin order (floor((m + 1) / 2) disjoint rotations per round, odd m with a
 * bye): the angles of a round, then its row phase (A and the eigenvectors), then its column phase, workgroup barriers between.
 * A pair is left alone when |a_pq| <= 2^-52 sqrt(|a_pp a_qq|) or |a_pq| <= 2^-92 max_i |a_ii| at entry (on a null direction
 * a_pp is a rounding residue of either sign and the first test cannot be met; such an entry is 2^52 times below what the rank
 * rule can see); a sweep without a rotation ends the solve; 40 sweeps without one: PLDA_E_NUMERIC naming the recording.  The
 * matrix itself is rotated from both sides, never its square.  The rotation order depends on m alone and every sum has a fixed
 * order: a recording's block is bit-identical alone, in any batch, under any launch grouping, and from run to run.  Two
 * dispatch classes: the LDS class (m up to out[3] of the plan) keeps the working matrix and the eigenvectors in the 160 KiB of
 * LDS of one compute unit, the HBM class in handle scratch; centred rows, basis, projected model and projected rows are in
 * handle scratch in both, carved per recording from one layout list.  Consecutive recordings are grouped into launches under
 * the AHC's 2 GiB scratch budget (PLDA_AHC_SCRATCH_BYTES sets another: tests), at most two launches per group: the number of
 * launches of a call does not depend on R.  The scratch belongs to the handle and is freed by plda_destroy.
 *
 *   plda_dense_pca_plan        out[0] = the class of a recording of N segments at dimension D (0 LDS, 1 HBM), out[1] = the
 *                              scratch bytes one such recording takes, out[2] = m, out[3] = the largest m of the LDS class.
 *   plda_score_dense_pca_dev   X, scores and the nullable ddims int32 [R] (d of every recording) and deig fp64 [T] (recording r
 *                              owns entries offsets[r] .. offsets[r+1]: its m eigenvalues, descending, then zeros) in HBM;
 *                              offsets [R + 1] and block_off [R + 1] (floats) are HOST arrays, the convention of
 *                              plda_ahc_matrix_dev.  Synchronises the handle's stream once (twice on the first call after a
 *                              model change, which forms W and B).
 *   plda_score_dense_pca       the same with everything in host memory.
 *   plda_score_dense_pca_ahc*  the blocks go into the S-norm slab buffer, as many consecutive recordings at a time as the
 *                              budget holds, are clustered by plda_ahc_matrix_dev's own path and dropped: labels, n_clusters
 *                              and the nullable merge record as in "speaker clustering" above, equal to plda_ahc_matrix on the
 *                              blocks of plda_score_dense_pca.
 * ERRORS.  PLDA_E_NOT_FITTED without a model.  PLDA_E_INVAL: target_energy outside (0, 1), offsets that do not ascend from 0,
 * an empty recording or one above PLDA_AHC_MAX, block_off[r+1] - block_off[r] < N_r^2, D > PLDA_DENSE_PCA_MAX_DIM, a truncated
 * model, the clustering's own argument errors; a row with a non-finite element fails the call with the count of such rows in
 * plda_last_error, and nothing is written.  PLDA_E_NUMERIC as above; the outputs of such a call are unspecified.
 * OUT OF SCOPE, each on purpose: Kaldi's per-recording mean subtraction of the vectors before the PCA estimate is applied to
 * them; several workgroups on one recording; an fp64 matrix-core tile for the covariance. ---- */
#define PLDA_DENSE_PCA_MAX_DIM 512
int plda_dense_pca_plan(plda_handle *h, int64_t N, int32_t D, int32_t out[4]);
int plda_score_dense_pca_dev(plda_handle *h, const double *dX, const int64_t *offsets, int64_t R, double target_energy,
                             float *dscores, const int64_t *block_off, int32_t *ddims, double *deig);
int plda_score_dense_pca(plda_handle *h, const double *X, const int64_t *offsets, int64_t R, double target_energy, float *scores,
                         const int64_t *block_off, int32_t *dims, double *eig);
int plda_score_dense_pca_ahc_dev(plda_handle *h, const double *dX, const int64_t *offsets, int64_t R, double target_energy,
                                 int32_t has_threshold, double threshold, const int32_t *min_clusters, int32_t *dlabels,
                                 int32_t *dn_clusters, int32_t *dmerge_a, int32_t *dmerge_b, double *dmerge_cost);
int plda_score_dense_pca_ahc(plda_handle *h, const double *X, const int64_t *offsets, int64_t R, double target_energy,
                             int32_t has_threshold, double threshold, const int32_t *min_clusters, int32_t *labels,
                             int32_t *n_clusters, int32_t *merge_a, int32_t *merge_b, double *merge_cost);

/* ---- VBx resegmentation (K16; csrc/vbx.hip): a batched variational-Bayes HMM over the segment sequence of every recording,
 * the step every x-vector diarisation recipe runs behind the AHC (Landini et al., "Bayesian HMM clustering of x-vector
 * sequences (VBx)", 2022).  The emission model is the PLDA model in its diagonalised space (within-class covariance I,
 * between-class covariance diag(Phi)); the initialisation is the AHC's labels.  The reference has NO counterpart; this is the
 * project's own extension, pinned by the NumPy model tests/vbx_model.py.  Everything is fp64.
 *
 * A RECORDING r is a run of T = offsets[r+1] - offsets[r] consecutive rows, 1 <= T <= PLDA_AHC_MAX.  Row t holds y_t [D], the
 * segment vector in the model's diagonalised space WITHOUT the length normalisation of TransformIvector (y = transform x +
 * offset: plda_project_rows), and an initial label l_t in [0, S), S = 1 + max_t l_t over the recording, 1 <= S <=
 * PLDA_VBX_MAX_SPK.  A label value with no segment is allowed.  Phi [D] is the between-class variance (NULL: the model's psi;
 * D must then be Dout).
 *
 * PARAMETERS.  Fa > 0 (0.3), Fb > 0 (17), loop_prob P in [0, 1) (0.99), init_smoothing sigma (5.0), max_iters >= 1 (40),
 * epsilon (1e-4).
 *
 * CONSTANTS.  rho[t,d] = y[t,d] sqrt(Phi[d]);  G[t] = -1/2 (sum_d y[t,d]^2 + D ln 2 pi).
 * START.  gamma[t,s] = e^sigma / (e^sigma + S - 1) for s = l_t and 1 / (e^sigma + S - 1) otherwise;  pi[s] = 1 / S.
 * ONE ITERATION i = 0, 1, ...
 *    1.  N[s] = sum_t gamma[t,s]
 *    2.  invL[s,d] = 1 / (1 + (Fa/Fb) N[s] Phi[d])
 *    3.  alpha[s,d] = (Fa/Fb) invL[s,d] sum_t gamma[t,s] rho[t,d]
 *    4.  lp[t,s] = Fa (sum_d rho[t,d] alpha[s,d] - 1/2 sum_d (invL[s,d] + alpha[s,d]^2) Phi[d] + G[t])
 *    5.  m[t] = max_s lp[t,s],  b[t,s] = exp(lp[t,s] - m[t])
 *    6.  forward:  u_0 = b_0 o pi,  u_t = b_t o (P a_{t-1} + (1 - P) pi),  c_t = sum_s u_t[s],  a_t = u_t / c_t
 *    7.  backward: beta_{T-1} = 1,  w = b_{t+1} o beta_{t+1},  beta_t[s] = (P w[s] + (1 - P) sum_j pi[j] w[j]) / c_{t+1}
 *    8.  gamma = a o beta
 *    9.  L = sum_t ln c_t + sum_t m[t]
 *   10.  pi'[s] = gamma[0,s] + (1 - P) pi[s] sum_{t>=1} b[t,s] beta[t,s] / c_t,  then pi = pi' / sum pi'
 *   11.  ELBO_i = L + (Fb/2) sum_{s,d} (ln invL - invL - alpha^2 + 1)
 *   12.  stop after iteration i >= 1 when ELBO_i - ELBO_{i-1} < epsilon (a comparison with a NaN is false), and after
 *        max_iters iterations in any case.
 * Steps 6 - 10 are the scaled form of the usual log-domain forward-backward for the transition matrix P I + (1 - P) 1 pi^T
 * (sum a_{t-1} = 1).  It is the DEFINITION: it puts no transcendental on the dependent chain, and a speaker whose pi underflows
 * to 0 simply dies where the log form gives -inf - -inf.  (The device runs 6 and 7 at the same time: its backward variable is
 * scaled by its own row sum, which gamma = a o beta / sum_s (a o beta) removes again; csrc/vbx.hip.)
 *
 * OUTPUTS.  labels int32 [T_total]: argmax_s gamma[t,s] of the last iteration run, ties to the smallest s, renumbered 0 .. k-1
 * per recording by ascending smallest member (the AHC's rule).  n_clusters int32 [R]: k.  Nullable: gamma fp64, packed,
 * recording r at gamma_off[r], row-major T_r x S_r, columns in the INITIAL numbering (gamma and gamma_off together or neither);
 * pi fp64 packed at pi_off[r], S_r entries (likewise); elbo fp64 [R, max_iters], entries at and beyond iters[r] quiet NaN;
 * iters int32 [R].  Nothing else is written.
 *
 * SECOND SPEAKER (K21; plda_vbx_top2[_dev], the recipe's --output-2nd).  Two more outputs, each nullable on its own, taken from
 * the same last-iteration gamma.  Let first(t) = argmax_s gamma[t,s], ties to the smallest s (labels before renumbering), and A
 * the set of speakers that are first(t) for at least one t of the recording, |A| = k = n_clusters[r].  Then
 *   second(t) = argmax over s in A \ {first(t)} of gamma[t,s], ties to the smallest s;
 *   post2   fp64  [T_total]: gamma[t, second(t)], the very bits the gamma output holds there;
 *   labels2 int32 [T_total]: second(t) in the renumbering of labels (0 .. k-1 by ascending smallest first-member).
 * k = 1: labels2[t] = -1 and post2[t] = 0.  A speaker that is nobody's first choice is dead in the VB sense and gets no number,
 * however high its posterior in a row: n_clusters and labels stay exactly plda_vbx's.  Where to USE the second speaker is the
 * caller's decision (an external overlap detector, or a floor on post2: plda_amd/diarize.py, apply_overlap).  The other six
 * outputs are bit-identical to plda_vbx's on the same input.
 *
 * ERRORS, all PLDA_E_INVAL: offsets that do not ascend from 0, an empty recording or one above PLDA_AHC_MAX, a parameter outside
 * its range, D outside 1 ... 4096 -- before any device work; a non-finite y, a label outside [0, 64), Phi[d] < 0 or non-finite
 * -- found on the device, with their count in plda_last_error; gamma_off[r+1] - gamma_off[r] < T_r S_r or pi_off[r+1] -
 * pi_off[r] < S_r -- known once S is.  None of them writes an output.  A model that is not fitted: PLDA_E_NOT_FITTED.
 *
 * DETERMINISM.  Every sum (N, sum_t gamma rho, the d-dots, c_t, sum ln c_t, pi') is taken in an order fixed by (T, S, D) alone
 * and there are no floating-point atomics: a recording's outputs are bit-identical from run to run, alone or inside any batch,
 * and under any grouping into launches.  labels2 and post2 are a selection from that gamma by comparisons alone (a butterfly
 * over the speaker lanes whose result does not depend on the order of its steps): the same holds for them.
 *
 * METHOD.  One workgroup per recording, persistent over the iterations (no host synchronisation between them), one lane per
 * speaker on the chain.  Two dispatch classes: the LDS class keeps the state (b, a, beta, c, m, G, alpha, invL, sqrt Phi, Phi:
 * 3 T S + 3 T + 2 S (D | 1) + 2 D doubles) in the LDS of one compute unit, the HBM class in handle scratch, grouped into
 * launches under 1 GiB (never fewer than one recording; PLDA_VBX_SCRATCH_BYTES in the environment at plda_create sets another
 * budget: tests); the scratch belongs to the handle and is freed by plda_destroy.
 *
 *   plda_vbx_plan            out[0] = the class of a recording of (T, S, D) (0 LDS, 1 HBM), out[1] = the scratch bytes one such
 *                            recording takes (0 in the LDS class), out[2] = the LDS class's limit in doubles of state.
 *   plda_vbx_dev             Y, Phi, labels_in and the outputs in HBM; offsets [R + 1], gamma_off [R + 1], pi_off [R + 1] are
 *                            HOST arrays (the AHC's and the fusion's convention).  Synchronises the handle's stream twice: to
 *                            read the reject counters and S, and at its end.
 *   plda_vbx                 the same with everything in host memory.
 *   plda_vbx_top2[_dev]      plda_vbx[_dev] with labels2 and post2 behind its arguments: the same kernels, one more pass over the
 *                            speaker lanes of every row where the arg-max is taken, in both classes; gamma is not read again
 *                            from HBM by a second kernel.
 *   plda_project_rows[_dev]  out [R, Dout] = X [R, Din] transform^T + offset: TransformIvector without its normalisation
 *                            factor, through the library's fp64 GEMM.
 * (Length normalisation and the LDA fit before the model: the section "embedding chain" below, K18.)
 * OUT OF SCOPE, each on purpose: more than 64 initial speakers; several workgroups on one recording; an overlap detector; a third
 * speaker.  (DER: the section "diarisation error rate" below; RTTM: plda_amd/rttm.py.) ---- */
#define PLDA_VBX_MAX_SPK 64
int plda_vbx_plan(plda_handle *h, int64_t T, int64_t S, int64_t D, int32_t out[3]);
int plda_vbx_dev(plda_handle *h, const double *dY, int64_t D, const double *dPhi, const int32_t *dlabels_in, const int64_t *offsets,
                 int64_t R, double Fa, double Fb, double loop_prob, double init_smoothing, int64_t max_iters, double epsilon,
                 int32_t *dlabels, int32_t *dn_clusters, double *dgamma, const int64_t *gamma_off, double *dpi, const int64_t *pi_off,
                 double *delbo, int32_t *diters);
int plda_vbx(plda_handle *h, const double *Y, int64_t D, const double *Phi, const int32_t *labels_in, const int64_t *offsets, int64_t R,
             double Fa, double Fb, double loop_prob, double init_smoothing, int64_t max_iters, double epsilon, int32_t *labels,
             int32_t *n_clusters, double *gamma, const int64_t *gamma_off, double *pi, const int64_t *pi_off, double *elbo,
             int32_t *iters);
int plda_vbx_top2_dev(plda_handle *h, const double *dY, int64_t D, const double *dPhi, const int32_t *dlabels_in, const int64_t *offsets,
                      int64_t R, double Fa, double Fb, double loop_prob, double init_smoothing, int64_t max_iters, double epsilon,
                      int32_t *dlabels, int32_t *dn_clusters, double *dgamma, const int64_t *gamma_off, double *dpi, const int64_t *pi_off,
                      double *delbo, int32_t *diters, int32_t *dlabels2, double *dpost2);
int plda_vbx_top2(plda_handle *h, const double *Y, int64_t D, const double *Phi, const int32_t *labels_in, const int64_t *offsets,
                  int64_t R, double Fa, double Fb, double loop_prob, double init_smoothing, int64_t max_iters, double epsilon,
                  int32_t *labels, int32_t *n_clusters, double *gamma, const int64_t *gamma_off, double *pi, const int64_t *pi_off,
                  double *elbo, int32_t *iters, int32_t *labels2, double *post2);
int plda_project_rows_dev(plda_handle *h, const double *dX, int64_t R, int32_t Din, double *dout);
int plda_project_rows(plda_handle *h, const double *X, int64_t R, int32_t Din, double *out);

/* ---- diarisation error rate (K17; csrc/der.hip): segment-level miss, false alarm and speaker confusion of R recordings under
 * the OPTIMAL one-to-one mapping of reference to hypothesis speakers, and the sweep of a full AHC merge record over Q
 * thresholds -- the metric of the diarisation path, on the device like EER, minDCF and Cllr.  The reference has NO counterpart;
 * tests/der_model.py is the host model.  Everything is an integer: nothing on the device is floating-point but the
 * comparison of a merge cost with a threshold.
 *
 * A RECORDING r owns segments offsets[r] .. offsets[r+1], 1 <= N <= PLDA_AHC_MAX.  Per segment t:
 *   ref[t]  int32: -1 = reference non-speech, otherwise 0 <= ref < PLDA_DER_MAX_REF;
 *   hyp[t]  int32: -1 = hypothesis non-speech, otherwise 0 <= hyp < PLDA_AHC_MAX;
 *   dur[t]  int32 >= 0, in ticks of the caller's choosing; dur is nullable: NULL = 1 everywhere.
 * A label value with no segment is allowed: the labels of either side are compacted per recording before anything else
 * (Sr distinct reference labels, Sh distinct hypothesis labels).
 *
 * COUNTS, all int64.  With C[i][j] = the sum of dur over the segments with ref = i and hyp = j:
 *   speech    = sum of dur over ref >= 0
 *   miss      = sum of dur over ref >= 0 and hyp < 0
 *   fa        = sum of dur over ref < 0 and hyp >= 0
 *   correct   = the maximum of sum_i C[i][m(i)] over all one-to-one partial maps m of reference to hypothesis speakers
 *   confusion = (sum of dur over ref >= 0 and hyp >= 0) - correct
 * The output is counts int64 [R, 4] = {speech, miss, fa, confusion}.  DER = (miss + fa + confusion) / speech is the CALLER's
 * division.  The optimum VALUE is unique, so the counts are fully determined by the input: they do not depend on the grid, on
 * the batch, on the grouping into launches or on the run.
 *
 * MAP (nullable), int32 [R, PLDA_DER_MAX_REF]: entry [r, i] = the hypothesis label mapped to reference label i, both in the
 * caller's own label values; -1 for a reference label that is absent, unmapped, or mapped to a speaker it shares no tick with
 * (a pair with C = 0 is reported as -1).  The map is one-to-one and attains `correct`.  Among optima of equal weight it is not
 * canonical, but it is a function of the recording's own matrix: the same alone or in any batch.
 *
 * SWEEP.  merge_a, merge_b, merge_cost are a FULL merge record in the layout of plda_ahc_matrix (one taken with has_threshold
 * = 0 and min_clusters = 1).  For every threshold q and recording r the prefix of the record is replayed under exactly the
 * stop rule of the AHC: stop when k <= max(1, min_clusters[r]) or !(cost <= -(double)thresholds[q]).  The slots are the
 * hypothesis labels (no hypothesis non-speech), scored as above: counts int64 [Q, R, 4], n_clusters int32 [Q, R].  A record
 * that ends (entry -1), or holds an entry that is not 0 <= a < b < N, before the stop rule fires is not a full record:
 * PLDA_E_INVAL.  So counts[q], n_clusters[q] are what plda_ahc_matrix at thresholds[q] followed by plda_der return, from one
 * device run of the clustering.
 *
 * ERRORS, all PLDA_E_INVAL: offsets that do not ascend from 0, an empty recording or one above PLDA_AHC_MAX, Q < 1 (or above
 * 65535), a NaN threshold, min_clusters[r] < 1 -- before any device work; a label below -1 or at or above its limit, a negative
 * dur -- found on the device, with their count in plda_last_error; a record that is not full.  None of them writes an output.
 *
 * METHOD.  One pass validates the call and counts Sr and Sh (the sweep: the length of every prefix) per recording; the host
 * reads that with one synchronisation of the handle's stream and sizes the launches.  Then one workgroup per (recording,
 * threshold): the labels present as bit sets, the compact Sr x W matrix (W = max(Sr, Sh): zero columns pad a hypothesis
 * with fewer speakers) filled by integer atomics, and a shortest-augmenting-path assignment (Hungarian / Jonker-Volgenant)
 * with int64 potentials, rows = reference speakers: at most Sr (Sr + 1) / 2 steps, each an update of the column slack and a
 * workgroup (value, column) minimum.  Two dispatch classes: the matrix in LDS while matrix and column state (32 bytes a
 * column) fit the 160 KiB of one compute unit, otherwise in handle scratch (8 Sr W bytes, at most 2 MiB, per recording in
 * flight), grouped into launches under 256 MiB (never fewer than one recording; PLDA_DER_SCRATCH_BYTES in the environment at
 * plda_create sets another budget: tests).  The column state is in LDS in both.  The sweep's replay takes 4 N more bytes of
 * LDS, so near the boundary a sweep entry may take the scratch class where plda_der_plan names the LDS class; no output
 * shows the class.  Every threshold is solved on its own.  The scratch belongs to the handle and is freed by plda_destroy.
 *
 *   plda_der_plan        out[0] = the class of a recording of Sr (0 ... 64) reference and Sh (0 ... PLDA_AHC_MAX) hypothesis
 *                        speakers (0 LDS, 1 scratch), out[1] = the scratch bytes one such recording takes (0 in the LDS
 *                        class), out[2] = the largest W = max(Sr, Sh) the LDS class takes at this Sr.
 *   plda_der_dev         ref, hyp, dur (nullable) and the outputs in HBM; offsets [R + 1] is a HOST array (the convention of
 *                        plda_ahc_matrix_dev).  Synchronises the handle's stream twice: to read the counters, and at its end.
 *   plda_der             the same with everything in host memory.
 *   plda_der_sweep_dev   the merge record, ref, dur (nullable) and the outputs in HBM; offsets [R + 1], thresholds [Q] and
 *                        min_clusters [R] (nullable: 1 everywhere) are HOST arrays.
 *   plda_der_sweep       the same with everything in host memory.
 * (Overlapped reference speech, a forgiveness collar and time-based scoring are the next section; here a segment has one
 * reference and one hypothesis label.  The Jaccard error rate and the per-speaker figures are the section after that.) ---- */
#define PLDA_DER_MAX_REF 64
int plda_der_plan(plda_handle *h, int64_t Sr, int64_t Sh, int32_t out[3]);
int plda_der_dev(plda_handle *h, const int32_t *dref, const int32_t *dhyp, const int32_t *ddur, const int64_t *offsets, int64_t R,
                 int64_t *dcounts, int32_t *dmap);
int plda_der(plda_handle *h, const int32_t *ref, const int32_t *hyp, const int32_t *dur, const int64_t *offsets, int64_t R,
             int64_t *counts, int32_t *map);
int plda_der_sweep_dev(plda_handle *h, const int32_t *dmerge_a, const int32_t *dmerge_b, const double *dmerge_cost,
                       const int64_t *offsets, int64_t R, const int32_t *dref, const int32_t *ddur, const double *thresholds, int64_t Q,
                       const int32_t *min_clusters, int64_t *dcounts, int32_t *dn_clusters);
int plda_der_sweep(plda_handle *h, const int32_t *merge_a, const int32_t *merge_b, const double *merge_cost, const int64_t *offsets,
                   int64_t R, const int32_t *ref, const int32_t *dur, const double *thresholds, int64_t Q, const int32_t *min_clusters,
                   int64_t *counts, int32_t *n_clusters);

/* ---- time-based diarisation error rate (K20; csrc/der_time.hip, the solve of csrc/der.hip): DER over TIME, with overlapped
 * reference speech, a forgiveness collar and UEM scoring regions.  This is md-eval's definition restated on integer ticks,
 * with the speaker mapping optimal over the scored region.  Parity with md-eval is UNPINNED: neither md-eval, dscore nor
 * pyannote.metrics is on the build machine; tests/der_time_model.py holds the two host models (tick by tick, and by intervals).
 *
 * All times are integer TICKS (the tick is the caller's; plda_amd/rttm.py uses 0.01 s).  Every interval is half-open,
 * [start, start + dur).  Per recording r:
 *   REFERENCE TURNS (turn_start, turn_dur, turn_spk), int32: turns turn_off[r] .. turn_off[r+1], in any order, 0 <= turn_spk <
 *     PLDA_DER_MAX_REF.  Two or more reference speakers may talk at once.  Turns of the SAME speaker must be disjoint
 *     (abutting is allowed).  A turn with dur = 0 is ignored.  A recording may have no turn.
 *   HYPOTHESIS SEGMENTS (seg_start, seg_dur, hyp), int32: segments offsets[r] .. offsets[r+1] (1 <= N <= PLDA_AHC_MAX: the rows
 *     the clustering labels), in any order, pairwise disjoint in time: at most one hypothesis speaker talks at any tick.
 *     hyp = -1 is non-speech, otherwise 0 <= hyp < PLDA_AHC_MAX; dur = 0 is ignored.
 *   UEM (nullable): scored intervals (uem_start, uem_dur), intervals uem_off[r] .. uem_off[r+1]; they may overlap each other,
 *     a tick is inside if any interval covers it.  uem_off NULL (then uem_start and uem_dur must be NULL): every tick is scored.
 *   collar c >= 0 ticks: every turn boundary b (start and end of every reference turn AS GIVEN, abutting turns included)
 *     removes [b - c, b + c) from scoring.  Zones may overlap each other and may reach below tick 0.
 *   flags: bit 0, PLDA_DER_SKIP_OVERLAP (md-eval's -1), additionally removes every tick with more than one reference speaker.
 * For a scored tick t: Rset(t) = the reference speakers talking at t, nref = |Rset|; nhyp = 0 or 1, j(t) the hypothesis label
 * when nhyp = 1.  COUNTS, all int64, in the layout of plda_der:
 *   speech    = sum of nref
 *   miss      = sum of max(0, nref - nhyp)
 *   fa        = sum of max(0, nhyp - nref)
 *   C[i][j]   = #{scored t : i in Rset(t), j = j(t)}
 *   correct   = the maximum of sum_i C[i][m(i)] over all one-to-one partial maps m
 *   confusion = sum of min(nref, nhyp) - correct
 * counts int64 [R, 4] = {speech, miss, fa, confusion}; DER is the caller's division.  map (nullable) int32 [R, 64] follows the
 * rules of plda_der's.  EXAMPLE: ref A [0, 10), B [5, 15); hyp X [0, 15).  Collar 0: {20, 5, 0, 5}.  Collar 1 removes [-1, 1),
 * [4, 6), [9, 11), [14, 16): {12, 3, 0, 3}.
 *
 * TWO HYPOTHESIS LABELS PER SEGMENT (K21; plda_der_timed_ovl[_dev]).  hyp2 int32 [T_total], nullable, is the second speaker of
 * every segment: -1 = none; hyp2[t] >= 0 requires 0 <= hyp2[t] < PLDA_AHC_MAX, hyp[t] >= 0 and hyp2[t] != hyp[t] (anything else
 * is an ENTRY violation, below).  The segments stay pairwise disjoint in time; a segment carries the label set J = {hyp[t]} u
 * {hyp2[t]} without the -1s, so at most two hypothesis speakers talk at any tick, and the labels of a recording are compacted
 * over both arrays.  With J(t) the label set of the segment over a scored tick (empty outside every segment) and nhyp = |J(t)|
 * in {0, 1, 2}:
 *   speech   += nref
 *   miss     += max(0, nref - nhyp)
 *   fa       += max(0, nhyp - nref)
 *   C[i][j]  += 1 for every i in Rset(t) and every j in J(t)
 *   correct   = the maximum of sum_i C[i][m(i)] over all one-to-one partial maps m
 *   confusion = sum of min(nref, nhyp) - correct
 * A one-to-one map matches at most min(nref, nhyp) pairs on any tick, so confusion >= 0.  EXAMPLES, ref A [0, 10), B [5, 15),
 * collar 0:   hyp [0, 5) X, [5, 10) X + Y, [10, 15) Y: {20, 0, 0, 0};   hyp [0, 15) X + Y: {20, 0, 10, 0};   hyp [0, 15) X,
 * hyp2 = -1: {20, 5, 0, 5} (plda_der_timed's figure).  With hyp2 = NULL, counts and map equal plda_der_timed's.  The atoms do
 * not change (ticks, reference mask, segment index); the solve looks both labels of an atom's segment up.
 *
 * SWEEP: as plda_der_sweep, the hypothesis label of segment t being the slot of the replayed merge prefix (no hypothesis
 * non-speech); counts [Q, R, 4], n_clusters [Q, R] (= N - merges, every segment counted, scored or not).  The time line is cut
 * once per recording; all Q thresholds read the same atoms.
 *
 * LIMITS: N <= PLDA_AHC_MAX, PLDA_DER_MAX_TURNS turns and PLDA_DER_MAX_UEM UEM intervals per recording; 0 <= start, start +
 * dur <= 2^30; 0 <= collar <= 2^20.
 * ERRORS, all PLDA_E_INVAL, none writes an output.  On the host, before any device work: an offset array (offsets, turn_off,
 * uem_off) that does not ascend from 0 or exceeds its limit, collar or flags out of range, the sweep's Q, thresholds,
 * min_clusters as in plda_der_sweep, a NULL array.  On the device, counted, the two counts in plda_last_error: ENTRIES with a
 * label or a time out of range (plda_der_timed_ovl: also a second label without a first, or equal to it); EVENTS that meet a
 * state the contract excludes -- a turn that starts inside another turn of its speaker (its start finds the speaker talking,
 * and a later end finds them silent: one violation may be counted at more than one event), a hypothesis segment that starts
 * while another is open.  A record that is not full: as plda_der_sweep.
 *
 * METHOD.  der_atoms_kernel, one workgroup per recording: one 64-bit key per boundary -- 2 per turn, 4 more per turn when collar
 * > 0, 2 per segment, 2 per UEM interval, ends before starts on the same tick -- sorted by a bitonic network, in LDS up to
 * 16384 key slots, above that in handle scratch (8 bytes a slot, slots rounded up to a power of two, at most 1 MiB per
 * recording, launches grouped under the budget of plda_der's scratch, PLDA_DER_SCRATCH_BYTES).  Scans over the sorted events
 * give every atom (a maximal run of ticks without an event) its 64-bit reference mask (an XOR scan: same-speaker turns are
 * disjoint, and the same prefix checks that), collar, UEM and hypothesis depth (+-1 scans) and hypothesis segment (a max
 * scan).  The scored atoms are compacted in time order into handle scratch (ticks, mask, segment index: 16 bytes each, at
 * most one per event); plda_der's solve then fills C from atoms (an atom adds its ticks to C[i][j] for every speaker i of
 * its mask) and runs the same assignment, in the same two classes.  Every sum is an integer: the counts do not depend on the
 * grid, the batch, the launch grouping or the run.  All scratch belongs to the handle and is freed by plda_destroy.
 *
 *   plda_der_timed_plan        out[0] = the event-sort class of a recording of n_turns, n_seg, n_uem at this collar (0 LDS,
 *                              1 scratch), out[1] = its scratch bytes (0 in the LDS class), out[2] = the largest event-slot
 *                              count of the LDS class.
 *   plda_der_timed_dev         the turn, segment and UEM arrays and the outputs in HBM; turn_off, offsets, uem_off [R + 1] are
 *                              HOST arrays.  Synchronises the handle's stream twice.
 *   plda_der_timed             the same with everything in host memory.
 *   plda_der_timed_ovl[_dev]   plda_der_timed[_dev] with hyp2 behind hyp (nullable: then it IS plda_der_timed[_dev]).
 *   plda_der_timed_sweep_dev   the merge record, the arrays and the outputs in HBM; the three offset arrays, thresholds [Q] and
 *                              min_clusters [R] (nullable) are HOST arrays.
 *   plda_der_timed_sweep       the same with everything in host memory.
 * OUT OF SCOPE, each on purpose: more than two simultaneous hypothesis speakers; second labels in the threshold sweeps (the AHC
 * has none); word-level or SAD-only scoring; several workgroups on one recording.  (JER and the per-speaker figures: the next
 * section.) ---- */
#define PLDA_DER_MAX_TURNS 16384
#define PLDA_DER_MAX_UEM 1024
#define PLDA_DER_SKIP_OVERLAP 1
int plda_der_timed_plan(plda_handle *h, int64_t n_turns, int64_t n_seg, int64_t n_uem, int32_t collar, int32_t out[3]);
int plda_der_timed_dev(plda_handle *h, const int32_t *dturn_start, const int32_t *dturn_dur, const int32_t *dturn_spk,
                       const int64_t *turn_off, const int32_t *dseg_start, const int32_t *dseg_dur, const int32_t *dhyp,
                       const int64_t *offsets, int64_t R, const int32_t *duem_start, const int32_t *duem_dur, const int64_t *uem_off,
                       int32_t collar, int32_t flags, int64_t *dcounts, int32_t *dmap);
int plda_der_timed(plda_handle *h, const int32_t *turn_start, const int32_t *turn_dur, const int32_t *turn_spk, const int64_t *turn_off,
                   const int32_t *seg_start, const int32_t *seg_dur, const int32_t *hyp, const int64_t *offsets, int64_t R,
                   const int32_t *uem_start, const int32_t *uem_dur, const int64_t *uem_off, int32_t collar, int32_t flags,
                   int64_t *counts, int32_t *map);
int plda_der_timed_ovl_dev(plda_handle *h, const int32_t *dturn_start, const int32_t *dturn_dur, const int32_t *dturn_spk,
                           const int64_t *turn_off, const int32_t *dseg_start, const int32_t *dseg_dur, const int32_t *dhyp,
                           const int32_t *dhyp2, const int64_t *offsets, int64_t R, const int32_t *duem_start, const int32_t *duem_dur,
                           const int64_t *uem_off, int32_t collar, int32_t flags, int64_t *dcounts, int32_t *dmap);
int plda_der_timed_ovl(plda_handle *h, const int32_t *turn_start, const int32_t *turn_dur, const int32_t *turn_spk, const int64_t *turn_off,
                       const int32_t *seg_start, const int32_t *seg_dur, const int32_t *hyp, const int32_t *hyp2, const int64_t *offsets,
                       int64_t R, const int32_t *uem_start, const int32_t *uem_dur, const int64_t *uem_off, int32_t collar, int32_t flags,
                       int64_t *counts, int32_t *map);
int plda_der_timed_sweep_dev(plda_handle *h, const int32_t *dmerge_a, const int32_t *dmerge_b, const double *dmerge_cost,
                             const int32_t *dturn_start, const int32_t *dturn_dur, const int32_t *dturn_spk, const int64_t *turn_off,
                             const int32_t *dseg_start, const int32_t *dseg_dur, const int64_t *offsets, int64_t R,
                             const int32_t *duem_start, const int32_t *duem_dur, const int64_t *uem_off, int32_t collar, int32_t flags,
                             const double *thresholds, int64_t Q, const int32_t *min_clusters, int64_t *dcounts, int32_t *dn_clusters);
int plda_der_timed_sweep(plda_handle *h, const int32_t *merge_a, const int32_t *merge_b, const double *merge_cost,
                         const int32_t *turn_start, const int32_t *turn_dur, const int32_t *turn_spk, const int64_t *turn_off,
                         const int32_t *seg_start, const int32_t *seg_dur, const int64_t *offsets, int64_t R, const int32_t *uem_start,
                         const int32_t *uem_dur, const int64_t *uem_off, int32_t collar, int32_t flags, const double *thresholds,
                         int64_t Q, const int32_t *min_clusters, int64_t *counts, int32_t *n_clusters);

/* ---- Jaccard error rate and per-speaker figures (K22; the JER form of csrc/der.hip's solve): the second metric of every
 * diarisation evaluation (DIHARD, VoxConverse, dscore), beside DER, from the same call.  Everything is an integer, as in the
 * three sections above: the device result is a function of the input alone.  tests/jer_model.py is the host model.
 *
 * PER RECORDING.  The scored ticks, Rset(t) and J(t) are exactly those of plda_der_timed_ovl (in the segment form: the
 * segments, each weighted by dur; ref = -1 is "no reference speaker", hyp = -1 "no hypothesis speaker").  With C[i][j] as
 * defined there:
 *   rt[i]   = #{scored t : i in Rset(t)}
 *   ht[j]   = #{scored t : j in J(t)}          (ticks without reference speech count; segment form: segments with ref = -1)
 *   a reference speaker COUNTS if rt[i] >= 1; n_ref = the number of such speakers.  In the timed form this is the set of map
 *   (the union of the scored masks); in the segment form a label all of whose segments have dur = 0 does not count
 *   U[i][j] = rt[i] + ht[j] - C[i][j]           (>= 1 whenever rt[i] >= 1)
 *   w[i][j] = floor(C[i][j] 2^32 / U[i][j])     an integer in [0, 2^32]: the Jaccard index quantised DOWNWARDS to 2^-32
 *   jsum    = the maximum of sum_i w[i][m(i)] over all one-to-one partial maps m of reference to hypothesis speakers
 * OUTPUTS.
 *   jer  int64 [R, 2] = {n_ref, jsum} (sweeps: [Q, R, 2]).  JER = 1 - jsum / (n_ref 2^32) is the CALLER's division, as DER is;
 *        n_ref = 0 gives {0, 0}.  Pooled over recordings: 1 - sum jsum / (2^32 sum n_ref), dscore's mean over all reference
 *        speakers of all files.  jsum is unique: jer does not depend on the grid, the batch, the launch grouping, the dispatch
 *        class or the run.  BOUND: every w is below the exact index times 2^32 by less than 1, so jsum differs from the
 *        optimum over exact rationals by less than n_ref, i.e. by less than n_ref 2^-32 in units of the index, and JER
 *        differs from the exact-rational figure by less than 2^-32.
 *   jmap int32 [R, 64] (nullable) follows the rules of map: caller's label values; -1 for a speaker that is absent, unmapped
 *        or mapped to a speaker it shares no tick with; one-to-one; it attains jsum; among equal optima it is not canonical
 *        but a function of the recording's own matrices alone.  jmap may differ from map (example 3).
 *   spk  int64 [R, 64, 3] (nullable) = {rt[i], I_i, U_i} per reference label value: under jmap I_i = C[i][jmap(i)] and
 *        U_i = rt[i] + ht[jmap(i)] - I_i; an unmapped speaker has I_i = 0, U_i = rt[i]; a label that is absent (or does not
 *        count) has {0, 0, 0}.  LAW: sum_i floor(I_i 2^32 / U_i) == jsum.  The speaker's own error rate is 1 - I_i / U_i.
 *   counts, map (and n_clusters in the sweeps): the values of plda_der / plda_der_timed_ovl / the sweeps on the same input.
 * EXAMPLES, collar 0.  (1) ref A [0, 10), B [5, 15); hyp X [0, 15): rt = 10, 10; ht = 15; C = 10, 10; w = 2863311530 for
 * both pairs, one is mapped: jer = {2, 2863311530}, JER = 2/3.  (2) the same reference; hyp [0, 5) X, [5, 10) X + Y, [10, 15)
 * Y: jer = {2, 8589934592}, JER = 0.  (3) ref A [0, 100); hyp X [0, 40), Y [40, 70), X [200, 1200): counts = {100, 30, 1000,
 * 30} with map A -> X; w[A][X] = floor(40 2^32 / 1100) = 156180628, w[A][Y] = floor(30 2^32 / 100) = 1288490188: jmap A -> Y,
 * jer = {1, 1288490188}, JER = 0.7.
 *
 * LIMITS.  The timed forms keep theirs (times <= 2^30, so C 2^32 <= 2^62).  The segment forms ADDITIONALLY require the sum of
 * dur over a recording's segments to be at most 2^30: a violation is found on the device, counted with the other entry
 * violations, answered with PLDA_E_INVAL, and nothing is written (plda_der itself keeps accepting larger sums).
 * ERRORS: those of the entry point each one extends (host checks before any device work, device violations counted, no output
 * written), and jer = NULL is PLDA_E_INVAL.
 *
 * PARITY WITH dscore IS UNPINNED: dscore is not on the build machine.  Known differences: dscore scores JER on 10 ms frames
 * WITHOUT a collar -- here collar, UEM and PLDA_DER_SKIP_OVERLAP apply as given, so pass collar = 0 for dscore's figure;
 * dscore's map is optimal on exact Jaccard indices, ours on the indices quantised to 2^-32 (the bound above); dscore reports
 * 100 % for a file with hypothesis speech and no reference speaker, here that file has n_ref = 0 and no rate.
 *
 * METHOD.  The solve of plda_der with two additions in the same workgroup: while C is filled, rt and ht are summed with
 * integer LDS atomics; after the first assignment (counts, map) every entry of the matrix becomes w << 31 | C in place -- ONE
 * 64-bit division per entry, no second matrix, nothing wider than 64 bits -- and the assignment runs again on w from fresh
 * potentials and a fresh column state, under the same (value, column) tie rule.  LDS: 512 bytes of rt and 4 (W + 1) bytes of
 * ht beyond plda_der's (the sweeps keep ht where the map's column labels would be), so the LDS / scratch boundary is the JER
 * form's own; the scratch class uses plda_der's scratch under the same budget.
 *
 *   plda_der_jer_plan              plda_der_plan under the JER form's LDS accounting (the non-sweep form's).
 *   plda_der_jer[_dev]             plda_der[_dev], then jer, jmap (nullable), spk (nullable).
 *   plda_der_timed_jer[_dev]       plda_der_timed_ovl[_dev] (hyp2 nullable), then the same three.
 *   plda_der_jer_sweep[_dev]       plda_der_sweep[_dev], then jer [Q, R, 2].
 *   plda_der_timed_jer_sweep[_dev] plda_der_timed_sweep[_dev], then jer [Q, R, 2]. ---- */
int plda_der_jer_plan(plda_handle *h, int64_t Sr, int64_t Sh, int32_t out[3]);
int plda_der_jer_dev(plda_handle *h, const int32_t *dref, const int32_t *dhyp, const int32_t *ddur, const int64_t *offsets, int64_t R,
                     int64_t *dcounts, int32_t *dmap, int64_t *djer, int32_t *djmap, int64_t *dspk);
int plda_der_jer(plda_handle *h, const int32_t *ref, const int32_t *hyp, const int32_t *dur, const int64_t *offsets, int64_t R,
                 int64_t *counts, int32_t *map, int64_t *jer, int32_t *jmap, int64_t *spk);
int plda_der_jer_sweep_dev(plda_handle *h, const int32_t *dmerge_a, const int32_t *dmerge_b, const double *dmerge_cost,
                           const int64_t *offsets, int64_t R, const int32_t *dref, const int32_t *ddur, const double *thresholds,
                           int64_t Q, const int32_t *min_clusters, int64_t *dcounts, int32_t *dn_clusters, int64_t *djer);
int plda_der_jer_sweep(plda_handle *h, const int32_t *merge_a, const int32_t *merge_b, const double *merge_cost, const int64_t *offsets,
                       int64_t R, const int32_t *ref, const int32_t *dur, const double *thresholds, int64_t Q,
                       const int32_t *min_clusters, int64_t *counts, int32_t *n_clusters, int64_t *jer);
int plda_der_timed_jer_dev(plda_handle *h, const int32_t *dturn_start, const int32_t *dturn_dur, const int32_t *dturn_spk,
                           const int64_t *turn_off, const int32_t *dseg_start, const int32_t *dseg_dur, const int32_t *dhyp,
                           const int32_t *dhyp2, const int64_t *offsets, int64_t R, const int32_t *duem_start, const int32_t *duem_dur,
                           const int64_t *uem_off, int32_t collar, int32_t flags, int64_t *dcounts, int32_t *dmap, int64_t *djer,
                           int32_t *djmap, int64_t *dspk);
int plda_der_timed_jer(plda_handle *h, const int32_t *turn_start, const int32_t *turn_dur, const int32_t *turn_spk, const int64_t *turn_off,
                       const int32_t *seg_start, const int32_t *seg_dur, const int32_t *hyp, const int32_t *hyp2, const int64_t *offsets,
                       int64_t R, const int32_t *uem_start, const int32_t *uem_dur, const int64_t *uem_off, int32_t collar, int32_t flags,
                       int64_t *counts, int32_t *map, int64_t *jer, int32_t *jmap, int64_t *spk);
int plda_der_timed_jer_sweep_dev(plda_handle *h, const int32_t *dmerge_a, const int32_t *dmerge_b, const double *dmerge_cost,
                                 const int32_t *dturn_start, const int32_t *dturn_dur, const int32_t *dturn_spk, const int64_t *turn_off,
                                 const int32_t *dseg_start, const int32_t *dseg_dur, const int64_t *offsets, int64_t R,
                                 const int32_t *duem_start, const int32_t *duem_dur, const int64_t *uem_off, int32_t collar,
                                 int32_t flags, const double *thresholds, int64_t Q, const int32_t *min_clusters, int64_t *dcounts,
                                 int32_t *dn_clusters, int64_t *djer);
int plda_der_timed_jer_sweep(plda_handle *h, const int32_t *merge_a, const int32_t *merge_b, const double *merge_cost,
                             const int32_t *turn_start, const int32_t *turn_dur, const int32_t *turn_spk, const int64_t *turn_off,
                             const int32_t *seg_start, const int32_t *seg_dur, const int64_t *offsets, int64_t R,
                             const int32_t *uem_start, const int32_t *uem_dur, const int64_t *uem_off, int32_t collar, int32_t flags,
                             const double *thresholds, int64_t Q, const int32_t *min_clusters, int64_t *counts, int32_t *n_clusters,
                             int64_t *jer);

/* ---- embedding chain (K18; csrc/embed.hip): what every x-vector / i-vector recipe runs between the extractor and a Gaussian
 * PLDA -- Kaldi's ivector-subtract-global-mean | transform-vec | ivector-normalize-length, the VBx recipe's
 * l2(LDA l2(x - m1) - m2).  All arithmetic fp64.  A chain is (Din, Dout, m_in, len_in, A, m_out, len_out); for a row x [Din]:
 *   1. v = x - m_in                        m_in [Din], NULL = 0
 *   2. if len_in > 0: v <- v len_in / |v|  (a row with |v| = 0 stays 0)
 *   3. u = A v                             A [Dout, Din] row-major, NULL = identity (Dout == Din required)
 *   4. u <- u - m_out                      m_out [Dout], NULL = 0
 *   5. if len_out > 0: u <- u len_out / |u| (a zero row stays 0)
 * and the output is u, fp64 [R, Dout].  Kaldi's recipes are (m_in, 0, A, -, sqrt(Dout)), VBx is (m1, 1, LDA, m2, 1), centre
 * and normalise only is (m, 0, -, -, sqrt(D)).  The input is fp64 (dtype 0) or fp32 (dtype 1); fp32 is widened exactly at the
 * load, so an fp32 array and its host-widened fp64 copy give the same output bits.  A non-finite input element makes its own
 * output row non-finite and touches no other row; nothing is rejected on the device.  `out` must not overlap X.
 * DETERMINISM: a row's output is a function of the row, the chain and the value of the input alone: the same bits from run to
 * run, alone (R = 1) or at any position of any batch -- an enrolment vector embedded alone scores bit-identically to one
 * embedded in a batch.  (How each class keeps the order of the k-sum and of both norm sums fixed: csrc/embed.hip.)  The rule
 * holds per handle configuration: PLDA_EMBED_VARIANT selects another class, which rounds differently.
 * Limits: 1 <= Din <= PLDA_EMBED_MAX_DIN, 1 <= Dout <= PLDA_EMBED_MAX_DOUT (the PLDA fit's own limit).
 * Dispatch classes (plda_embed_plan): 0 = no A, one wave per row, one read and one write; 1 = A and Dout <= 512, one pass on
 * v_mfma_f64_16x16x4_f64, a workgroup owns whole rows and all columns (K4's shape), A zero-padded once per chain; 2 = A and
 * Dout > 512: row pass into handle scratch, the library's fp64 GEMM, row pass, in chunks of exactly 16 384 rows (at most
 * 512 MiB + 256 MiB of scratch; the last chunk is padded with zero rows so that the GEMM's dispatch never depends on R).
 * PLDA_EMBED_VARIANT=1 in the environment at plda_create forces class 2 for every chain with A (tests, the bench's A/B arm;
 * any value but 0 / 1: PLDA_E_INVAL).  PLDA_EMBED_CUS=n (tests only; a whole number 1 ... 4096, anything else: PLDA_E_INVAL)
 * sizes class 1's main / tail split for n compute units instead of the device's, so that a few hundred rows reach every block
 * shape; by the determinism rule it changes no output bit.
 * The C entry points of the model (plda_fit, plda_transform_rows, ...) never apply a chain implicitly.
 *   plda_embed_set       installs a chain from HOST arrays (copied).  PLDA_E_INVAL before any device work, the installed chain
 *                        untouched: a dimension outside its limit, A NULL with Dout != Din, a negative or non-finite len_*, a
 *                        non-finite element of m_in, A or m_out.
 *   plda_embed_clear     removes it.
 *   plda_embed_dims      Din, Dout, flags (bit 0 m_in, 1 A, 2 m_out present); no chain: PLDA_E_NOT_FITTED.
 *   plda_embed_get       the chain as it was set, bit for bit (host arrays; any NULL; absent parts are not written).
 *   plda_embed_plan      out[0] = class, out[1] = rows per workgroup of the main launch (class 1: 128, 64 or 32; the tail launch
 *                        halves that down to 16 until every compute unit has at most one block), out[2] = its LDS bytes.
 *   plda_embed_apply_dev X [R, Din] of dtype and out [R, Dout] in HBM; enqueues on the handle's stream.  No chain:
 *                        PLDA_E_NOT_FITTED; Din != the chain's, dtype not 0 / 1: PLDA_E_INVAL; R <= 0: nothing, PLDA_OK.
 *   plda_embed_apply     the same with host arrays (one upload, one download).
 *   plda_embed_fit_dev   estimates a chain from rows X [N, Din] and installs it.  m_in = the column mean of X (fp64, about a
 *                        pilot row, fixed order); v_i = steps 1-2; mu = the mean of the v_i.  kind 0 "centre": A NULL, Dout =
 *                        Din, m_out = mu.  kind 1 "whiten": C = (1/N) sum (v_i - mu)(v_i - mu)^T = Q L Q^T, L descending, row i
 *                        of A = l_i^-1/2 q_i^T for i < Dout, m_out = A mu; l_{Dout-1} <= N Din 2^-53 l_0: PLDA_E_NUMERIC.  kind 2
 *                        "lda" (labels dense 0 .. K-1): W = (1/N) sum_k sum_{i in k} (v_i - mu_k)(v_i - mu_k)^T, B = (1/N)
 *                        sum_k n_k (mu_k - mu)(mu_k - mu)^T, A W A^T = I, A B A^T = diag(e), e the Dout largest generalised
 *                        eigenvalues, descending, m_out = A mu; a singular W: PLDA_E_NUMERIC; K < 2: PLDA_E_INVAL.  Plain Fisher
 *                        LDA: restated, parity unpinned against Kaldi's ivector-compute-lda.  eig (HOST, nullable) receives the
 *                        Dout eigenvalues (l for kind 1, e for kind 2).  PLDA_E_INVAL before any device work: kind outside
 *                        0 .. 2, Dout > Din for kinds 1 / 2 (kind 0: Dout != Din), Din > 2048 for kinds 1 / 2 (the eigensolver's
 *                        limit; kind 0 takes every Din up to PLDA_EMBED_MAX_DIN), kind 2 without labels, N < 2, the errors
 *                        of plda_embed_set.  An error leaves the installed chain bit-identical.  Scratch: all of v, N Din 8 bytes,
 *                        plus O(Din^2 + K Din).
 *   plda_embed_fit       the same with host arrays; K is found from the labels (max + 1).
 * OUT OF SCOPE, each on purpose: fp32 or bf16 output; more than one
 * matrix per chain.  (The cosine back-end is the section "cosine back-end" below, K27.  Within-class covariance normalisation
 * needs no kernel of its own under it: WCCN is A with A W A^T = I, full-rank LDA (kind 2, Dout = Din) differs from it by a
 * rotation, and a cosine is invariant to rotations -- MPlda.fit_embedding(kind="wccn") fits kind 2 at Dout = Din.) ---- */
#define PLDA_EMBED_MAX_DIN 4096
#define PLDA_EMBED_MAX_DOUT 2048
int plda_embed_set(plda_handle *h, int32_t Din, int32_t Dout, const double *m_in, double len_in, const double *A,
                   const double *m_out, double len_out);
int plda_embed_clear(plda_handle *h);
int plda_embed_dims(plda_handle *h, int32_t *Din, int32_t *Dout, int32_t *flags);
int plda_embed_get(plda_handle *h, double *m_in, double *len_in, double *A, double *m_out, double *len_out);
int plda_embed_plan(plda_handle *h, int32_t Din, int32_t Dout, int32_t has_A, int32_t dtype, int32_t out[3]);
int plda_embed_apply_dev(plda_handle *h, const void *dX, int32_t dtype, int64_t R, int32_t Din, double *dout);
int plda_embed_apply(plda_handle *h, const void *X, int32_t dtype, int64_t R, int32_t Din, double *out);
int plda_embed_fit_dev(plda_handle *h, const void *dX, int32_t dtype, int64_t N, int32_t Din, const uint64_t *dlabels, int64_t K,
                       int32_t kind, int32_t Dout, double len_in, double len_out, double *eig);
int plda_embed_fit(plda_handle *h, const void *X, int32_t dtype, int64_t N, int32_t Din, const uint64_t *labels, int32_t kind,
                   int32_t Dout, double len_in, double len_out, double *eig);

/* ---- cosine back-end (K27; csrc/cosine.hip): a second back-end behind every scoring entry point.  A handle is a PLDA handle
 * (the default) or a cosine handle, never both.  On a cosine handle a score is the cosine of the two rows,
 *     c(u, v) = (sum_d u_d v_d) inv(u) inv(v),   inv(x) = 1 / sqrt(sum_d x_d^2), 0 for a zero row (which scores 0),
 * and with z-norm statistics (c - zmean_i) / zstd_i where zstd_i != 0 (such a row is left un-normalised, as on a PLDA handle).
 * The operand forms reach the trials GEMM through the same seam as PLDA scores: the packed operands are the unit rows
 * (the enrol side times 1 / zstd_i), rounded once from fp64 to fp32, q_j = 0 and r'_i = -zmean_i / zstd_i; the GEMM kernels
 * and every consumer are the PLDA ones -- plda_score_matrix[_dev] and its sharded pair, plda_score_matrix_snorm*,
 * plda_cohort_stats*, plda_score_topn*, plda_score_eer_dev, plda_score_min_dcf_dev, plda_score_rocch_dev, plda_score_calib_*_dev,
 * plda_score_fusion_side_*_dev, plda_score_partition_dev, plda_score_ahc*, plda_score_spectral*, plda_score_prepare*_dev.
 * plda_score_pairs and plda_score_one evaluate c in fp64.  Rows are [.., D] fp64 of ANY length: they are length-normalised
 * here.  n_enrol / n_uniform are checked as on a PLDA handle and then ignored (a model vector is a model vector: GEMM depth D,
 * the uniform path); plda_score_prepare[_counts]_dev prepares the one form a cosine test side has.
 * A row's packed bits depend on the row and its own zstd alone (not on the batch, the launch shape or PLDA_PREP_VARIANT 2 / 3;
 * PLDA_PREP_VARIANT=1 is ignored).  A non-finite element makes its own row's (column's) scores NaN and touches no other.
 *   plda_backend_set(h, PLDA_BACKEND_COSINE, D)   1 <= D <= 2048, and the handle holds no PLDA model (PLDA_E_INVAL otherwise:
 *                        create another handle).  Dout = Din = D (plda_get_dims answers (D, D)); a test side prepared before is
 *                        dropped, the coefficient caches too.
 *   plda_backend_set(h, PLDA_BACKEND_PLDA, 0)     a cosine handle returns to the empty PLDA state (no model); a PLDA handle is
 *                        left as it is, model included.  D != 0 here, or any other kind: PLDA_E_INVAL.
 *   plda_backend_get     kind, and D of a cosine handle (0 on a PLDA handle); either pointer may be NULL.
 * ON A COSINE HANDLE every entry point that installs a PLDA model (plda_fit*, plda_fit_em_dev, plda_fit_sharded*,
 * plda_set_model) returns PLDA_E_INVAL and says why; every entry point that needs the model proper (plda_transform*,
 * plda_adapt_*, plda_blend_model, plda_truncate, plda_smooth, plda_znorm_stats*, plda_vbx*, plda_project_rows*, the dense-PCA
 * forms, plda_get_model, the sharded cohort statistics) returns PLDA_E_NOT_FITTED, and plda_last_error ends in
 * "(cosine back-end selected: this entry point needs a PLDA model)".  The embedding chain, the LDA model, the matrix forms and
 * everything that takes scores are independent of the back-end.
 * OUT OF SCOPE, each on purpose: fp32 or bf16 row input to the operand forms; a closed form of plda_znorm_stats for cosines
 * (z-norm statistics of a cosine handle come from plda_cohort_stats with top_k = Nc); score averaging instead of model
 * averaging for multi-session enrolment.  The sharded forms and the opt-in bf16x3 arm consume the same operands and work by
 * construction; they are not tested on a cosine handle. ---- */
#define PLDA_BACKEND_PLDA 0
#define PLDA_BACKEND_COSINE 1
int plda_backend_set(plda_handle *h, int32_t kind, int32_t D);
int plda_backend_get(plda_handle *h, int32_t *kind, int32_t *D);

/* ---- LDA: replaces the reference's second model, the pure-Python
 * class LDA of python/liblda/lda.py (used by scoring/scoreLDA.py:175,224,241), on the same
 * handle.  All fp64.  solver: 0 = 'svd' (lda.py:171-209), 1 = 'eigen' (:134-169),
 * 2 = 'lsqr' (:211-240).  labels dense 0..K-1 (the shim compacts np.unique order, :112-116);
 * priors: K host doubles or NULL = class frequencies (:113-119), renormalised when their sum
 * is not exactly 1 (:121-122).  A singular within-class covariance with the eigen solver
 * returns PLDA_E_NUMERIC (the reference raises LinAlgError from scipy.linalg.eigh, :157).
 *   plda_lda_dims        K, D, rank (columns of scalings: svd = retained rank, eigen = D,
 *                        lsqr = 0), solver
 *   plda_lda_get_model   priors[K], means[K,D], xbar[D] (svd), scalings[D,rank] (svd, eigen),
 *                        coef[K,D], intercept[K], explained_variance_ratio[D] (eigen); any NULL
 *   plda_lda_set_model   restores a saved model (the reference cannot persist one)
 *   plda_lda_predict     out[N,K]; mode 0 decision_function (:242-270), 1 predict_log_proba
 *                        (:296-314), 2 the logistic of the decision values (first half of
 *                        predict_proba, :283-287), 3 the same one-vs-rest normalised (:292)
 *   plda_lda_transform   out[N,ncomp] = X scalings[:, :ncomp] (eigen, :333-334) or
 *                        (X - xbar) scalings[:, :ncomp] (svd, :331-332); lsqr -> PLDA_E_INVAL ---- */
int plda_lda_fit(plda_handle *h, const double *X, int64_t N, int32_t D, const uint64_t *labels,
                 int32_t solver, const double *priors);
int plda_lda_fit_dev(plda_handle *h, const double *dX, int64_t N, int32_t D, const uint64_t *dlabels,
                     int64_t K, int32_t solver, const double *priors);
int plda_lda_dims(plda_handle *h, int64_t *K, int32_t *D, int32_t *rank, int32_t *solver);
int plda_lda_get_model(plda_handle *h, double *priors, double *means, double *xbar, double *scalings,
                       double *coef, double *intercept, double *evr);
int plda_lda_set_model(plda_handle *h, int32_t solver, int64_t K, int32_t D, int32_t rank,
                       const double *priors, const double *means, const double *xbar,
                       const double *scalings, const double *coef, const double *intercept);
int plda_lda_predict(plda_handle *h, const double *X, int64_t N, int32_t D, int32_t mode, double *out);
int plda_lda_predict_dev(plda_handle *h, const double *dX, int64_t N, int32_t mode, double *dout);
int plda_lda_transform(plda_handle *h, const double *X, int64_t N, int32_t D, int32_t ncomp, double *out);
int plda_lda_transform_dev(plda_handle *h, const double *dX, int64_t N, int32_t ncomp, double *dout);

#ifdef __cplusplus
}
#endif
#endif
