// plda_amd/csrc/operand_slabs.hip -- the labelled trials of the operand forms (plda_score_eer_dev, plda_score_min_dcf_dev,
// plda_score_calib_pass_dev, plda_score_calib_fit_dev): a trials matrix that is never held.
//
// The reference's caller scores every trial and hands the scores to eer.py (scoring/scorePLDA.py:302-318 ->
// scoring/eer.py:68-76): what it wants is a few numbers, not M x Nt floats -- C4's matrix is 192 GB.  Here the scores exist one
// row slab at a time (<= 4 GiB): every slab is scored by the trials GEMM (the test side packed once, the distinct enrol counts
// found once), consumed by the reduction's kernel and overwritten by the next; a reduction that takes several passes
// re-scores the slabs per pass.  The EER's pilot samples every step-th enrol row through a small GEMM of its own.  Identical
// to the matrix forms on the materialised matrix (the kernels give a trial the same bits wherever its tile lies).
// Not yet inside the GEMM's epilogue: the slab is written and read back once, through HBM.
// (snorm.hip's cohort slabs use another buffer and another height rule; they are not these.)
#include "trial_source.hpp"

namespace plda {

__global__ void eer_gather_rows_kernel(const double *__restrict__ X, int D, int64_t step, int64_t rows, double *__restrict__ out) {
  const int64_t r = blockIdx.x;
  if (r >= rows) return;
  for (int d = threadIdx.x; d < D; d += blockDim.x) out[r * D + d] = X[r * step * D + d];
}
__global__ void eer_gather_meta_kernel(const int32_t *__restrict__ n, const double *__restrict__ zm, const double *__restrict__ zs,
                                       const int64_t *__restrict__ spk, int64_t step, int64_t rows, int32_t *__restrict__ on,
                                       double *__restrict__ ozm, double *__restrict__ ozs, int64_t *__restrict__ ospk) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  if (n) on[r] = n[r * step];
  if (zm) { ozm[r] = zm[r * step]; ozs[r] = zs[r * step]; }
  ospk[r] = spk[r * step];
}

static int operand_produce(void *vc, int64_t r0, int64_t rows, const float **scores, int64_t *ld) {
  auto *c = static_cast<OperandSlabs *>(vc);
  const int D = c->h->Dout;
  PLDA_TRY(score_matrix_device(c->h, c->dU + r0 * D, c->dn ? c->dn + r0 : nullptr, c->n_uniform, rows, c->dV, c->Nt,
                               c->dzm ? c->dzm + r0 : nullptr, c->dzs ? c->dzs + r0 : nullptr, c->slab, c->Nt, c->packedB,
                               c->has_cs ? &c->cs : nullptr));
  c->packedB = true;
  *scores = c->slab; *ld = c->Nt;
  return PLDA_OK;
}
static int operand_sample(void *vc, int64_t step, const float **scores, int64_t *ld, const int64_t **espk, int64_t *rows) {
  auto *c = static_cast<OperandSlabs *>(vc);
  plda_handle *h = c->h;
  const int D = h->Dout;
  const int64_t Ms = ceil_div(c->M, step);
  const size_t oU = 0, oZ = round_up((size_t)Ms * D * 8, 256), oS = oZ + round_up((size_t)Ms * 16, 256), oN = oS + round_up((size_t)Ms * 8, 256);
  PLDA_HIP(h, h->eer_smp.reserve(oN + (size_t)Ms * 4 + 256));
  char *b = h->eer_smp.as<char>();
  double *sU = reinterpret_cast<double *>(b + oU), *szm = reinterpret_cast<double *>(b + oZ), *szs = szm + Ms;
  int64_t *sspk = reinterpret_cast<int64_t *>(b + oS);
  int32_t *sn = reinterpret_cast<int32_t *>(b + oN);
  eer_gather_rows_kernel<<<(unsigned)Ms, 256, 0, h->stream>>>(c->dU, D, step, Ms, sU);
  eer_gather_meta_kernel<<<(unsigned)ceil_div(Ms, 256), 256, 0, h->stream>>>(c->dn, c->dzm, c->dzs, c->despk, step, Ms, sn, szm, szs, sspk);
  PLDA_LAUNCH_CHECK(h);
  PLDA_TRY(score_matrix_device(h, sU, c->dn ? sn : nullptr, c->n_uniform, Ms, c->dV, c->Nt, c->dzm ? szm : nullptr, c->dzm ? szs : nullptr,
                               c->slab, c->Nt, c->packedB, c->has_cs ? &c->cs : nullptr));
  c->packedB = true;
  *scores = c->slab; *ld = c->Nt; *espk = sspk; *rows = Ms;
  return PLDA_OK;
}

int operand_source(plda_handle *h, const char *who, const double *dU, const int32_t *dn, int n_uniform, int64_t M, const double *dV,
                   int64_t Nt, const double *dzmean, const double *dzstd, const int64_t *despk, const int64_t *dtspk, const void *out,
                   OperandSlabs *c, TrialSource *src) {
  if (!can_score(h)) return fail(h, PLDA_E_NOT_FITTED, "%s: model not fitted", who);
  if (!dU || !dV || !despk || !dtspk || !out || M <= 0 || Nt <= 0) return fail(h, PLDA_E_INVAL, "%s: bad argument", who);
  if (!dn && n_uniform <= 0) return fail(h, PLDA_E_INVAL, "%s: n_uniform must be > 0 when n_enrol is NULL", who);
  // the set-up: the distinct enrol counts found once, the slab height, the slab buffer
  *c = OperandSlabs{h, dU, dn, n_uniform, M, dV, Nt, (dzmean && dzstd) ? dzmean : nullptr, (dzmean && dzstd) ? dzstd : nullptr, despk};
  c->has_cs = false; c->packedB = false;
  if (dn) { PLDA_TRY(score_count_set_device(h, dn, M, &c->cs)); c->has_cs = true; }
  // slabs of <= 4 GiB of scores, whole 256-row tiles, at least one tile row
  int64_t rows = std::max<int64_t>(256, (((int64_t)4 << 30) / 4 / Nt) / 256 * 256);
  if (h->eer_slab_rows > 0) rows = round_up(h->eer_slab_rows, 256);      // PLDA_EER_SLAB_ROWS: small slabs for the tests
  rows = std::min(rows, round_up(M, 256));
  c->slab_rows = rows;
  PLDA_HIP(h, h->eer_slab.reserve((size_t)rows * Nt * 4));
  c->slab = h->eer_slab.as<float>();
  c->sl = TrialSlabs{rows, operand_produce, operand_sample, c};
  h->prep_valid = false;           // (the slabs pack the test side themselves)
  *src = TrialSource::slabs(&c->sl, M, Nt, despk, dtspk);
  return PLDA_OK;
}

}  // namespace plda
