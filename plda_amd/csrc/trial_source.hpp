// plda_amd/csrc/trial_source.hpp -- what a reduction over labelled trials consumes, and the one walk over it.
//
// The EER and DET points (eer.hip), the calibration pass (calib.hip), the minDCF levels (dcf.hip) and the ROC convex hull
// (rocch.hip) all read labelled trials
// that arrive in one of three kinds: a trials matrix in HBM with the speaker ids of its rows and columns (possibly the local
// rows of a row-sharded matrix), two flat lists of target / non-target scores, or a matrix that exists one row slab at a time
// (the operand forms: operand_slabs.hip scores a slab, the consumer reads it, the next slab overwrites it).  A TrialSource
// names its kind; for_each_piece is the only place that turns a source into the pieces a kernel is launched on.  The
// device-side entry points of the four consumers are declared here, once, for api.hip and comm.hip.
#pragma once

#include "common.hpp"

#include <algorithm>

namespace plda {

// ---- the order-preserving key of a score, its inverse, the histogram width and the strip width of the passes
constexpr int EER_BINS = 2048;
constexpr int EER_STRIP = 1024;
inline float key_score(unsigned k) {
  const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}
#ifdef __HIPCC__
__device__ __forceinline__ unsigned score_key(float f) {
  unsigned u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;      // -0.0 == +0.0 as scores: one candidate threshold, not two
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // monotone: a < b  <=>  key(a) < key(b)
}
#endif

// row-sharded matrix: after every local pass the caller's reduction makes the counts global
// (hist: sum over ranks; below: max; above: min)
typedef int (*TrialReduce)(void *ctx, unsigned long long *hist, unsigned *below, unsigned *above);

// produce: enqueue the scores of rows [r0, r0 + rows) (rows <= slab_rows) on the handle's stream, say where they are;
// sample: the same for every step-th row of the matrix (<= slab_rows of them) together with THOSE rows' speaker ids
struct TrialSlabs {
  int64_t slab_rows;
  int (*produce)(void *ctx, int64_t r0, int64_t rows, const float **scores, int64_t *ld);
  int (*sample)(void *ctx, int64_t step, const float **scores, int64_t *ld, const int64_t **espk, int64_t *rows);
  void *ctx;
};

struct TrialSource {
  enum Kind { MATRIX, LISTS, SLABS };
  Kind kind = MATRIX;
  const float *scores = nullptr; int64_t ld = 0, M = 0, Nt = 0; const int64_t *espk = nullptr, *tspk = nullptr;   // MATRIX; SLABS: the whole matrix, scores unset
  const float *pos = nullptr; int64_t np = 0; const float *neg = nullptr; int64_t nn = 0;                         // LISTS
  const TrialSlabs *sl = nullptr;                                                                                  // SLABS
  TrialReduce reduce = nullptr;                // nullptr = single process
  void *ctx = nullptr;
  int64_t row_step = 1;                        // MATRIX: every row_step-th row only (the pilot's sample)
  // windowed lists (the EER's single-pass form): the lists hold the scores of a key window only; the counts below it and
  // the class totals come from the full pass
  bool windowed = false, none_above = false;   // none_above: no trial lies above the window (its top is the data's top)
  unsigned long long base_p = 0, base_n = 0, tot_p = 0, tot_n = 0;

  // (M == 0: a rank of a sharded call that owns no row -- no piece, but it takes part in the reductions)
  static TrialSource matrix(const float *scores, int64_t ld, int64_t M, int64_t Nt, const int64_t *espk, const int64_t *tspk) {
    TrialSource s;
    s.kind = MATRIX; s.scores = scores; s.ld = ld; s.M = M; s.Nt = Nt; s.espk = espk; s.tspk = tspk;
    return s;
  }
  static TrialSource lists(const float *pos, int64_t np, const float *neg, int64_t nn) {
    TrialSource s;
    s.kind = LISTS; s.pos = pos; s.np = np; s.neg = neg; s.nn = nn;
    return s;
  }
  static TrialSource slabs(const TrialSlabs *sl, int64_t M, int64_t Nt, const int64_t *espk, const int64_t *tspk) {
    TrialSource s;
    s.kind = SLABS; s.sl = sl; s.ld = Nt; s.M = M; s.Nt = Nt; s.espk = espk; s.tspk = tspk;
    return s;
  }
  TrialSource &reduced_by(TrialReduce r, void *c) { reduce = r; ctx = c; return *this; }
  TrialSource &every(int64_t step) { row_step = step; return *this; }
  TrialSource &window_of(unsigned long long bp, unsigned long long bn, unsigned long long tp, unsigned long long tn, bool no_above) {
    windowed = true; none_above = no_above; base_p = bp; base_n = bn; tot_p = tp; tot_n = tn;
    return *this;
  }
};

// One launch's worth of a source: `rows` rows of Nt scores.  cls < 0: labelled rows -- "row" r is scores + r * row_step * ld
// with speaker espk[r * row_step]; cls = 0 / 1: one flat list of that class (rows = 1, ld = Nt, no espk).
struct TrialPiece { const float *scores; int64_t ld, rows, Nt; const int64_t *espk; int64_t row_step; int cls; };

// Every piece of the local data in turn: the slabs in ascending r0, each produced just before f sees it; else the matrix if
// it has rows; else the non-target list and then the target list, each if non-empty.  f returns a status; the first failure
// ends the walk.  produce = false: the same extents (rows, Nt, cls) with no slab produced and the GPU untouched -- a slab's
// piece then carries no scores (calib_pass sizes its partials this way before it launches anything).
template <class F>
int for_each_piece(const TrialSource &src, F &&f, bool produce = true) {
  switch (src.kind) {
    case TrialSource::SLABS:
      for (int64_t r0 = 0; r0 < src.M; r0 += src.sl->slab_rows) {
        const int64_t rows = std::min(src.sl->slab_rows, src.M - r0);
        const float *sc = nullptr;
        int64_t ld = src.Nt;
        if (produce) PLDA_TRY(src.sl->produce(src.sl->ctx, r0, rows, &sc, &ld));
        PLDA_TRY(f(TrialPiece{sc, ld, rows, src.Nt, src.espk + r0, 1, -1}));
      }
      break;
    case TrialSource::MATRIX: {
      const int64_t rows = ceil_div(src.M, src.row_step);
      if (rows > 0) PLDA_TRY(f(TrialPiece{src.scores, src.ld, rows, src.Nt, src.espk, src.row_step, -1}));
      break;
    }
    case TrialSource::LISTS:
      if (src.nn > 0) PLDA_TRY(f(TrialPiece{src.neg, src.nn, 1, src.nn, nullptr, 1, 0}));
      if (src.np > 0) PLDA_TRY(f(TrialPiece{src.pos, src.np, 1, src.np, nullptr, 1, 1}));
      break;
  }
  return PLDA_OK;
}

// ---- operand_slabs.hip: the slabs of the operand forms (plda_score_eer_dev, plda_score_min_dcf_dev, plda_score_calib_*_dev)
// are produced by the trials GEMM.  The distinct enrol counts are found once, the test side is packed by the first slab.
struct OperandSlabs {
  plda_handle *h;
  const double *dU; const int32_t *dn; int n_uniform; int64_t M; const double *dV; int64_t Nt;
  const double *dzm, *dzs; const int64_t *despk;
  CountSet cs; bool has_cs; bool packedB;
  float *slab; int64_t slab_rows;
  TrialSlabs sl;                               // what the returned source points to: *this must outlive it, where it is
};
// The prologue of an operand form: the fitted / null / n_uniform checks (messages prefixed with `who`), the slab set-up, the
// ready source.
int operand_source(plda_handle *h, const char *who, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV,
                   int64_t Nt, const double *dzmean, const double *dzstd, const int64_t *despk, const int64_t *dtspk, const void *out,
                   OperandSlabs *os, TrialSource *src);

// ---- eer.hip
// one histogram pass of the EER over the local data: bits [shift, shift + nbits) of the keys whose higher bits equal
// `prefix` (has_prefix = 0: every key) -> hh[2][EER_BINS] on the host, class 0 = non-target; dhist: 2 * EER_BINS * 8 device bytes
int eer_pass(plda_handle *h, const TrialSource &src, int shift, int nbits, unsigned prefix, int has_prefix,
             unsigned long long *dhist, unsigned *dbelow, unsigned *dabove, std::vector<unsigned long long> &hh);
// Sharded calls (src.reduce; nothing otherwise): sums one [2][EER_BINS] block over the ranks.  Every rank makes the same
// reduction calls whatever happens locally: a rank that has failed (*rc) keeps taking part with a poisoned block -- 2^48
// added to counter 0, far above any real count -- so that all ranks see the failure after this very sum and return an error
// together instead of leaving their peers blocked in a collective.  Returns *rc == PLDA_OK.
bool reduce_block_or_poison(plda_handle *h, const TrialSource &src, const char *who, unsigned long long *H, int *rc);
int eer_matrix_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *despk,
                      const int64_t *dtspk, double *out, TrialReduce reduce = nullptr, void *ctx = nullptr);
int eer_lists_device(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, double *out);
int score_eer_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV, int64_t Nt,
                     const double *dzmean, const double *dzstd, const int64_t *despk, const int64_t *dtspk, double *out);
int det_matrix_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *despk, const int64_t *dtspk,
                      int npoints, double *far, double *frr, double *thresholds);
int det_lists_device(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, int npoints, double *far, double *frr,
                     double *thresholds);
// ---- dcf.hip
int min_dcf_step(int level, int64_t n_nodes, const plda_min_dcf_node *nodes, const uint64_t *hist, int n_points,
                 const plda_dcf_point *pts, plda_min_dcf_state *st, int64_t cap_next, plda_min_dcf_node *next, int64_t *n_next);
int min_dcf_finish(const plda_min_dcf_state *st, int n_points, const plda_dcf_point *pts, const uint32_t *below, const uint32_t *above,
                   plda_min_dcf *out);
int min_dcf_matrix_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *despk,
                          const int64_t *dtspk, int n_points, const plda_dcf_point *pts, plda_min_dcf *out, plda_min_dcf_info *info,
                          TrialReduce reduce, void *ctx);
int min_dcf_lists_device(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, int n_points,
                         const plda_dcf_point *pts, plda_min_dcf *out, plda_min_dcf_info *info);
int score_min_dcf_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV, int64_t Nt,
                         const double *dzmean, const double *dzstd, const int64_t *despk, const int64_t *dtspk, int n_points,
                         const plda_dcf_point *pts, plda_min_dcf *out, plda_min_dcf_info *info);
// ---- rocch.hip
int rocch_hull(int64_t T, const uint32_t *edge_key, const uint64_t *other_lt, const uint64_t *other_le, const uint64_t *edge_lt,
               const uint64_t *edge_le, int edge_class, uint64_t Np, uint64_t Nn, int64_t cap_vertices, plda_rocch *out,
               plda_rocch_vertex *vertices, double *llr);
int rocch_finish(int64_t n_vertices, plda_rocch_vertex *vertices, const uint32_t *below, const uint32_t *above);
int rocch_matrix_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *despk, const int64_t *dtspk,
                        int64_t cap_vertices, plda_rocch *out, plda_rocch_vertex *vertices, double *llr, plda_rocch_points *points,
                        plda_rocch_info *info);
int rocch_lists_device(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, int64_t cap_vertices, plda_rocch *out,
                       plda_rocch_vertex *vertices, double *llr, plda_rocch_points *points, plda_rocch_info *info);
int score_rocch_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV, int64_t Nt,
                       const double *dzmean, const double *dzstd, const int64_t *despk, const int64_t *dtspk, int64_t cap_vertices,
                       plda_rocch *out, plda_rocch_vertex *vertices, double *llr, plda_rocch_points *points, plda_rocch_info *info);
int pav_map_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, int64_t n_vertices,
                   const plda_rocch_vertex *vertices, const double *llr, double bound, float *dout, int64_t ld_out);
// ---- calib.hip
int calib_pass_matrix_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *despk,
                             const int64_t *dtspk, double a, double c, double theta, plda_calib_record *out);
int calib_fit_matrix_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *despk,
                            const int64_t *dtspk, double prior, double tol, int max_iter, plda_calib_fit *out);
int calib_pass_lists_device(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, double a, double c,
                            double theta, plda_calib_record *out);
int calib_fit_lists_device(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, double prior, double tol,
                           int max_iter, plda_calib_fit *out);
int score_calib_pass_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV, int64_t Nt,
                            const double *dzmean, const double *dzstd, const int64_t *despk, const int64_t *dtspk, double a, double c,
                            double theta, plda_calib_record *out);
int score_calib_fit_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV, int64_t Nt,
                           const double *dzmean, const double *dzstd, const int64_t *despk, const int64_t *dtspk, double prior,
                           double tol, int max_iter, plda_calib_fit *out);
int affine_map_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, double a, double b, float *dout,
                      int64_t ld_out);
// ---- fusion.hip (K systems in lock-step; pointer arrays are HOST arrays of K device pointers)
int fusion_pass_matrices_device(plda_handle *h, int K, const float *const *dscores, const int64_t *ld, int64_t M, int64_t Nt,
                                const int64_t *despk, const int64_t *dtspk, const double *a, double c, double theta,
                                plda_fusion_record *out);
int fusion_fit_matrices_device(plda_handle *h, int K, const float *const *dscores, const int64_t *ld, int64_t M, int64_t Nt,
                               const int64_t *despk, const int64_t *dtspk, double prior, double tol, int max_iter, plda_fusion_fit *out);
int fusion_pass_lists_device(plda_handle *h, int K, const float *const *dpos, int64_t np, const float *const *dneg, int64_t nn,
                             const double *a, double c, double theta, plda_fusion_record *out);
int fusion_fit_lists_device(plda_handle *h, int K, const float *const *dpos, int64_t np, const float *const *dneg, int64_t nn,
                            double prior, double tol, int max_iter, plda_fusion_fit *out);
int fusion_map_device(plda_handle *h, int K, const float *const *dscores, const int64_t *ld, int64_t M, int64_t Nt, const double *a,
                      double b, float *dout, int64_t ld_out);
// K matrices + Q sides formed in registers (K25; kernels in fusion.hip); `sides` is a HOST array of Q entries
int fusion_side_pass_device(plda_handle *h, int K, const float *const *dscores, const int64_t *ld, int Q, const plda_fusion_side *sides,
                            int64_t M, int64_t Nt, const int64_t *despk, const int64_t *dtspk, const double *a, double c, double theta,
                            plda_fusion_record *out);
int fusion_side_fit_device(plda_handle *h, int K, const float *const *dscores, const int64_t *ld, int Q, const plda_fusion_side *sides,
                           int64_t M, int64_t Nt, const int64_t *despk, const int64_t *dtspk, double prior, double tol, int max_iter,
                           plda_fusion_fit *out);
int fusion_side_map_device(plda_handle *h, int K, const float *const *dscores, const int64_t *ld, int Q, const plda_fusion_side *sides,
                           int64_t M, int64_t Nt, const double *a, double b, float *dout, int64_t ld_out);
int score_fusion_side_pass_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV,
                                  int64_t Nt, const double *dzmean, const double *dzstd, const int64_t *despk, const int64_t *dtspk, int Q,
                                  const plda_fusion_side *sides, const double *a, double c, double theta, plda_fusion_record *out);
int score_fusion_side_fit_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV,
                                 int64_t Nt, const double *dzmean, const double *dzstd, const int64_t *despk, const int64_t *dtspk, int Q,
                                 const plda_fusion_side *sides, double prior, double tol, int max_iter, plda_fusion_fit *out);
// the argument check of the list forms (K, the two pointer arrays, their K entries, the lengths): used by the host-list entry
// points before they upload, and by the device-list drivers
int fusion_list_args_check(plda_handle *h, const char *fn, int K, const float *const *pos, int64_t np, const float *const *neg, int64_t nn);
int fusion_newton(const plda_fusion_record *r, double prior, double *F, double *d, double *lambda2);
// ---- partition.hip (trial keys, K26): the plan on the host (h: where a message goes, may be nullptr), the two device forms
int partition_plan(plda_handle *h, const char *fn, const int64_t *espk, int64_t M, const int64_t *tspk, int64_t Nt,
                   const plda_trial_key *key, plda_partition_record *plan);
int partition_matrix_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *despk,
                            const int64_t *dtspk, const plda_trial_key *key, float *dtar, int64_t cap_tar, float *dnon, int64_t cap_non,
                            plda_partition_record *plan_out);
int score_partition_device(plda_handle *h, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV, int64_t Nt,
                           const double *dzmean, const double *dzstd, const int64_t *despk, const int64_t *dtspk,
                           const plda_trial_key *key, float *dtar, int64_t cap_tar, float *dnon, int64_t cap_non,
                           plda_partition_record *plan_out);
// ---- comm.hip: the row-sharded forms over the installed communicator
int eer_matrix_comm_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *despk,
                           const int64_t *dtspk, double *out);
int min_dcf_matrix_comm_device(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *despk,
                               const int64_t *dtspk, int n_points, const plda_dcf_point *pts, plda_min_dcf *out, plda_min_dcf_info *info);

}  // namespace plda
