// plda_amd/csrc/embed.hip -- K18: the embedding chain in front of the PLDA model (include/plda_hip.h, "embedding chain"):
//     v = x - m_in;  v <- v len_in / |v|;  u = A v;  u <- u - m_out;  u <- u len_out / |u|        (each part optional)
// fp64 throughout, fp32 or fp64 rows in, fp64 rows out.  Kaldi's ivector-subtract-global-mean | transform-vec |
// ivector-normalize-length and the VBx recipe's l2(LDA l2(x - m1) - m2) are both instances.
//
// Three dispatch classes (plda_embed_plan):
//   0  A null: embed_rows_kernel, one wave per row, the row in registers (element d = 64 e + lane), both norms by the fixed
//      DPP tree of wave_sum_f64, one read and one write.
//   1  A present, Dout <= 512: embed_fused_kernel, K4's shape (csrc/transform.hip): a workgroup of 8 waves owns 16 * 8 / CH rows
//      and ALL columns, wave (rg, ch) accumulates 16 rows x NT 16-column tiles in v_mfma_f64_16x16x4_f64 accumulators.  Operand
//      stages of 16 k: A's rows (zero-padded once per chain, h->em_apad) + the block's rows of x - m_in (widened from fp32 at
//      the load), double-buffered in LDS, fetched global -> registers before the MFMAs of the previous stage and written behind
//      them; one __syncthreads() per stage.  |v|^2 is accumulated by the staging threads; s1 = len_in / |v| scales the
//      accumulators in the epilogue (it commutes with A), then m_out, |u|^2 across the tiles through LDS, one write.
//   2  A present, Dout > 512 (or PLDA_EMBED_VARIANT=1, any Dout): per chunk of EMBED_CHUNK rows, embed_rows_kernel writes v to
//      handle scratch, gemm_f64 forms A v, embed_rows_kernel reads that and writes the finished rows.
//
// The bits of a row do not depend on where it stands (the determinism rule of the header):
//   * class 0: a row is one wave's work, whatever the grid.
//   * class 1: every output element is ONE accumulator's chain over the k-steps in ascending order, whichever wave and block
//     shape holds it; |v|^2 is summed by the 16 threads (lk = t & 15, a DPP row) that stage the row, thread lk over k = lk,
//     lk + 16, ... in order and then the four DPP steps -- the same in every block shape; |u|^2 is summed per 16-column tile
//     by the four DPP steps and then over the tiles 0 .. ceil(Dout / 16) - 1 in ascending order by every lane, independent of
//     how the tiles are dealt to the column slices.  The file is built with -ffp-contract=off (build.py): every fused
//     multiply-add is written as fma(), so no instantiation contracts differently from another.
//   * class 2: gemm_f64 chooses its kernel and its split of k by the shape of the product, so every chunk is a product of
//     EXACTLY EMBED_CHUNK rows (the rows past the end are zeros and go to scratch): the dispatch is a function of (Din, Dout)
//     alone.  A call of one row costs a chunk's product; that is the price of the rule in the class nobody should be in.
//
// Block shapes of class 1 (main launch over a whole number of rounds of the grid, then one tail launch with the smallest
// blocks that still give every CU at most one -- K4's rule): Dout <= 128: <8,1> 128 rows, tails <4,2> 64, <2,4> 32, <1,8> 16;
// <= 208: <13,1>, <7,2>, <4,4>, <2,8>; <= 256: <16,1>, <8,2>, <4,4>, <2,8>; <= 384: <12,2> 64 rows, <6,4>, <3,8>; <= 512:
// <8,4> 32 rows, <4,8> (K4's <16,2> of 64 rows spills here -- 52 bytes of scratch per lane beside the staging registers of
// this kernel, also with A fetched in quarters -- and is not built; what the 32-row blocks cost at Dout > 384 is unmeasured).
// K4's recorded negative results were taken as given and not re-measured here: LDS-DMA staging, 4-wave workgroups,
// register-resident A.  Not carried over from K4 (unmeasured here): the early / late wave split of the
// staging work, the split fetch and the next block's prefetch under the epilogue.
//
// Measured (scripts/embed_bench.py, profiles/embed_*.json; whole plda_embed_apply_dev calls between HIP events, a warm-up, 5
// repetitions, medians, one box in one session, clock read after each shape 2.1 - 2.4 GHz), class 1 against the forced class-2
// arm on the same shape: 100 000 x 512 -> 200 fp32 0.515 against 0.955 ms (1.85 x; 0.51 of the fp64 MFMA peak against 0.27);
// 1 200 000 x 256 -> 128 fp32 2.04 against 3.91 ms (1.92 x; 0.49); 100 000 x 200 -> 200 fp64 0.252 against 0.488 ms (1.93 x;
// 0.40).  Class 1 wins on all three and stays.  It is behind transform_fused_kernel at the same sizes (0.54 / 0.76 / 0.54): what
// of K4's round-3 work it lacks is listed above.  Class 0, 1 000 000 x 512 fp32: 1.67 ms = 0.46 of 8 TB/s.
//
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage with the flags of build.py, gfx950): no instantiation spills a
// VGPR or uses scratch memory.  SGPR spills (to VGPR lanes, not to memory): embed_rows_kernel<*, 64> 46, embed_fused_kernel<*, 16, 1>
// 4, none elsewhere.  VGPRs:
//   embed_fused_kernel<fp32 | fp64, NT, CH>: <8,1> 164 | 164; <4,2> 116 | 116; <2,4> 90 | 90; <1,8> 74 | 74; <13,1> 232 | 232;
//    <7,2> 166 | 166; <4,4> 128 | 128; <2,8> 98 | 98; <16,1> 251 | 251; <8,2> 180 | 180; <12,2> 250 | 250; <6,4> 188 | 188;
//    <3,8> 130 | 130; <8,4> 224 | 224; <4,8> 174 | 174;
//   embed_rows_kernel<fp32 | fp64, EPL>: <2> 18 | 18; <8> 30 | 30; <32> 102 | 126; <64> 199 | 255;
//   the fit's and the padding kernels: embed_pad_kernel 13; embed_center_kernel 13; embed_symmetrize_kernel 8;
//    embed_pivot_check_kernel 14; embed_colsum_kernel<fp32> 14; embed_colmean_kernel<fp32> 15; embed_colsum_kernel<fp64> 14;
//    embed_colmean_kernel<fp64> 16;
#include "common.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace plda {

constexpr int64_t EMBED_CHUNK = 16384;   // rows of one class-2 product (16384 x 4096 doubles of v = 512 MiB at the largest Din)

typedef double f64x4e __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double em_dpp16_sum(double x) {   // sum over a DPP row of 16 lanes, every lane gets it
  x += dpp_f64<0xB1>(x);     // quad_perm [1,0,3,2]
  x += dpp_f64<0x4E>(x);     // quad_perm [2,3,0,1]
  x += dpp_f64<0x141>(x);    // row_half_mirror
  x += dpp_f64<0x140>(x);    // row_mirror
  return x;
}
// len / sqrt(ss): 0 for a zero row (it stays 0), NaN for a NaN sum; division and square root are IEEE
__device__ __forceinline__ double em_scale(double len, double ss) { return ss == 0.0 ? 0.0 : len / sqrt(ss); }

// ------------------------------------------------------------------------------------
// class 0 (and both row passes of class 2): one wave per row, the row in registers.
//   v = x - c1; if (l1 > 0) v *= l1 / |v|; v -= c2; if (l2 > 0) v *= l2 / |v|     (c1, c2 nullable)
// Rows R .. Rpad - 1 of `out` are written as zeros (class 2 pads its chunk).  X and out may be the same rows only if TIN
// is double (a lane reads exactly the elements it writes); neither is __restrict__.
// ------------------------------------------------------------------------------------
template <typename TIN, int EPL>
__global__ __launch_bounds__(256) void embed_rows_kernel(const TIN *X, int64_t R, int64_t Rpad, int D, const double *c1, double l1,
                                                         const double *c2, double l2, double *out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= Rpad) return;
  double *o = out + row * (int64_t)D;
  if (row >= R) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int d = e * 64 + lane;
      if (d < D) o[d] = 0.0;
    }
    return;
  }
  const TIN *x = X + row * (int64_t)D;
  double v[EPL];
  double ss = 0.0;
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int d = e * 64 + lane;
    double xv = 0.0;
    if (d < D) {
      xv = (double)x[d];
      if (c1) xv -= c1[d];
    }
    v[e] = xv;
    ss = fma(xv, xv, ss);
  }
  if (l1 > 0.0) {
    const double f = em_scale(l1, wave_sum_f64(ss));
#pragma unroll
    for (int e = 0; e < EPL; ++e) v[e] *= f;
  }
  if (c2) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int d = e * 64 + lane;
      if (d < D) v[e] -= c2[d];
    }
  }
  if (l2 > 0.0) {
    double s2 = 0.0;
#pragma unroll
    for (int e = 0; e < EPL; ++e) s2 = fma(v[e], v[e], s2);
    const double f = em_scale(l2, wave_sum_f64(s2));
#pragma unroll
    for (int e = 0; e < EPL; ++e) v[e] *= f;
  }
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int d = e * 64 + lane;
    if (d < D) o[d] = v[e];
  }
}

template <typename TIN>
static int launch_rows(plda_handle *h, const TIN *X, int64_t R, int64_t Rpad, int D, const double *c1, double l1, const double *c2,
                       double l2, double *out) {
  const int64_t SLAB = (int64_t)1 << 30;   // rows per launch (a grid of 2^28 workgroups)
  for (int64_t r0 = 0; r0 < Rpad; r0 += SLAB) {
    const int64_t rp = std::min(SLAB, Rpad - r0), rr = std::max<int64_t>(0, std::min(rp, R - r0));
    const unsigned grid = (unsigned)ceil_div(rp, 4);
    const TIN *x = X + r0 * D;
    double *o = out + r0 * D;
    if (D <= 128) embed_rows_kernel<TIN, 2><<<grid, 256, 0, h->stream>>>(x, rr, rp, D, c1, l1, c2, l2, o);
    else if (D <= 512) embed_rows_kernel<TIN, 8><<<grid, 256, 0, h->stream>>>(x, rr, rp, D, c1, l1, c2, l2, o);
    else if (D <= 2048) embed_rows_kernel<TIN, 32><<<grid, 256, 0, h->stream>>>(x, rr, rp, D, c1, l1, c2, l2, o);
    else embed_rows_kernel<TIN, 64><<<grid, 256, 0, h->stream>>>(x, rr, rp, D, c1, l1, c2, l2, o);
    PLDA_LAUNCH_CHECK(h);
  }
  return PLDA_OK;
}

// ------------------------------------------------------------------------------------
// class 1: the fused kernel
// ------------------------------------------------------------------------------------
template <int NT, int CH>
struct EmGeom {
  static constexpr int KS = 16;                        // depth of a stage: four MFMA k-steps
  static constexpr int RG = 8 / CH;                    // row groups of 16 rows
  static constexpr int ROWS = 16 * RG;
  static constexpr int COLS = 16 * NT * CH;
  static constexpr int RPP = 32;                       // rows one fetch pass of the 512 threads covers (16 k each)
  static constexpr int TP = (COLS + RPP - 1) / RPP;    // fetch passes over A's rows
  static constexpr int TR = TP * RPP;                  // rows of A's LDS stage (the padded A has at least as many)
  static constexpr int XP = (ROWS + RPP - 1) / RPP;
  // row pitch in doubles: KS + 2 is conflict-free for the fragment reads (TfGeom::LD, transform.hip); KS + 1 where that
  // does not fit the LDS
  static constexpr int LD = ((size_t)(TR + ROWS) * (KS + 2) * 16 <= 160 * 1024) ? KS + 2 : KS + 1;
  static constexpr int STAGE = (TR + ROWS) * LD;
  static constexpr size_t LDS_BYTES = (size_t)2 * STAGE * 8;
  static constexpr int SCRATCH = COLS + ROWS + (COLS / 16) * ROWS;   // the epilogue's doubles: m_out | |v|^2 | tile sums
};

// Apad: [>= TR rows][Dinp = Din rounded up to 16], zeros outside A.  X's row pointers are clamped to the last row, its k to
// the last column (the value is replaced by 0 at the LDS write); nothing is read or written out of bounds.
template <typename TIN, int NT, int CH>
__global__ __launch_bounds__(512) void embed_fused_kernel(const TIN *__restrict__ X, int64_t R, int Din,
                                                          const double *__restrict__ Apad, int Dinp, int Dout,
                                                          const double *__restrict__ m_in, double len_in,
                                                          const double *__restrict__ m_out, double len_out,
                                                          double *__restrict__ out) {
  using G = EmGeom<NT, CH>;
  constexpr int KS = G::KS, RG = G::RG, ROWS = G::ROWS, COLS = G::COLS, RPP = G::RPP, TP = G::TP, TR = G::TR, XP = G::XP;
  constexpr int LD = G::LD, STAGE = G::STAGE, KSTEPS = KS / 4;
  constexpr int NQ = NT >= 12 ? 2 : 1;
  extern __shared__ __attribute__((aligned(16))) double em_lds[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int rg = wave % RG, ch = wave / RG;
  const int fi = lane & 15, fk = lane >> 4;
  const int lk = t & 15, lr = t >> 4;       // this thread's k and first row inside a fetch pass (lr < 32)
  // 32-bit element offsets from uniform bases (the padded A has at most 512 x 4096 elements, a block of X 128 x 4096): one
  // register per thread instead of a 64-bit pointer per fetch pass
  const unsigned aoff = (unsigned)(lr * Dinp + lk), astep = (unsigned)(RPP * Dinp);
  const int afrag = (ch * NT * 16 + fi) * LD + fk, xfrag = (TR + rg * 16 + fi) * LD + fk;
  const int64_t nblocks = (R + ROWS - 1) / ROWS;
  const int ntiles = (Dout + 15) >> 4;

  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int64_t r0 = blk * ROWS;
    const TIN *xb = X + r0 * (int64_t)Din;
    const int rmax = (int)min((int64_t)ROWS - 1, R - 1 - r0);
    unsigned xo[XP];
    double ra[(TP + NQ - 1) / NQ], rx[XP], sq[XP];
#pragma unroll
    for (int p = 0; p < XP; ++p) {
      xo[p] = (unsigned)(min(lr + RPP * p, rmax) * Din);
      sq[p] = 0.0;
    }
    // A's rows of a stage come in NQ phases (pass p belongs to phase p % NQ): in one go where the registers allow, in halves
    // beside 12 or more accumulator tiles -- phase 0 is requested at the top of a stage, phase j + 1 when phase j is
    // written to the other buffer, behind every KSTEPS / NQ k-steps; the last phase is written at the stage's end
    auto fetch_a = [&](int k0, int q) {
#pragma unroll
      for (int p = 0; p < TP; ++p)
        if (p % NQ == q) ra[p / NQ] = Apad[aoff + (unsigned)p * astep + (unsigned)k0];
    };
    auto stage_a = [&](double *buf, int q) {
#pragma unroll
      for (int p = 0; p < TP; ++p)
        if (p % NQ == q) buf[(lr + RPP * p) * LD + lk] = ra[p / NQ];
    };
    auto fetch_x = [&](int k0) {
      const int k = k0 + lk;
      const bool kok = k < Din;
      const int kc = kok ? k : Din - 1;
      const double mi = m_in ? m_in[kc] : 0.0;
#pragma unroll
      for (int p = 0; p < XP; ++p) {
        const double xv = (double)xb[xo[p] + (unsigned)kc] - mi;
        rx[p] = kok ? xv : 0.0;
      }
    };
    auto stage_x = [&](double *buf) {
#pragma unroll
      for (int p = 0; p < XP; ++p)
        if (lr + RPP * p < ROWS) {
          buf[(TR + lr + RPP * p) * LD + lk] = rx[p];
          sq[p] = fma(rx[p], rx[p], sq[p]);
        }
    };

    int cur = 0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      fetch_a(0, q);
      stage_a(em_lds, q);
    }
    fetch_x(0);
    stage_x(em_lds);
    __syncthreads();
    f64x4e acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = f64x4e{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < Din; k0 += KS) {
      const bool more = k0 + KS < Din;
      double *nxt = em_lds + (cur ^ 1) * STAGE;
      if (more) {
        fetch_a(k0 + KS, 0);
        fetch_x(k0 + KS);
      }
      const int ksteps = min(KSTEPS, (Din - k0 + 3) >> 2);   // the last stage of a ragged Din: only the k-steps that hold data
      const double *As = em_lds + cur * STAGE + afrag, *Xs = em_lds + cur * STAGE + xfrag;
#pragma unroll
      for (int kk = 0; kk < KSTEPS; ++kk) {
        if (kk < ksteps) {
          const double a = Xs[kk * 4];
#pragma unroll
          for (int tn = 0; tn < NT; ++tn) {
            const double b = As[tn * 16 * LD + kk * 4];
            acc[tn] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[tn], 0, 0, 0);
          }
        }
        asm volatile("" ::: "memory");     // fragment reads stay inside their k-step (transform.hip)
        if ((kk + 1) % (KSTEPS / NQ) == 0 && (kk + 1) / (KSTEPS / NQ) < NQ && more) {
          stage_a(nxt, (kk + 1) / (KSTEPS / NQ) - 1);
          fetch_a(k0 + KS, (kk + 1) / (KSTEPS / NQ));
        }
      }
      if (more) {
        stage_a(nxt, NQ - 1);
        stage_x(nxt);
      }
      __syncthreads();
      cur ^= 1;
    }

    // both stage buffers are dead behind the loop's last barrier: the epilogue's scratch takes their place
    double *mo = em_lds, *vn = mo + COLS, *red = vn + ROWS;
#pragma unroll
    for (int p = 0; p < XP; ++p) {
      const double s = em_dpp16_sum(sq[p]);
      if (lk == 0 && lr + RPP * p < ROWS) vn[lr + RPP * p] = s;
    }
    for (int c = t; c < COLS; c += 512) mo[c] = (m_out && c < Dout) ? m_out[c] : 0.0;
    __syncthreads();
    // accumulator layout: column = lane & 15 of the tile, row = (lane >> 4) + 4 * reg
    const int rloc = rg * 16 + fk;
    double s1[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) s1[r] = len_in > 0.0 ? em_scale(len_in, vn[rloc + 4 * r]) : 1.0;
#pragma unroll
    for (int tn = 0; tn < NT; ++tn) {
      const int col = (ch * NT + tn) * 16 + fi;
      const bool cok = col < Dout;
      const double off = mo[col];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double u = cok ? acc[tn][r] * s1[r] - off : 0.0;
        acc[tn][r] = u;
        if (len_out > 0.0) {
          const double ps = em_dpp16_sum(u * u);
          if (fi == 0) red[(ch * NT + tn) * ROWS + rloc + 4 * r] = ps;
        }
      }
      asm volatile("" ::: "memory");       // one tile at a time: interleaved, the 4 NT DPP chains spill
    }
    double s2[4] = {1.0, 1.0, 1.0, 1.0};
    if (len_out > 0.0) {
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double tot = 0.0;
        for (int tl = 0; tl < ntiles; ++tl) tot += red[tl * ROWS + rloc + 4 * r];   // ascending tiles: the same sum in every shape
        s2[r] = em_scale(len_out, tot);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t grow = r0 + rloc + 4 * r;
      if (grow < R) {
        double *o = out + grow * (int64_t)Dout;
#pragma unroll
        for (int tn = 0; tn < NT; ++tn) {
          const int col = (ch * NT + tn) * 16 + fi;
          if (col < Dout) o[col] = acc[tn][r] * s2[r];
        }
      }
    }
    __syncthreads();   // the scratch is the next block's first stage
  }
}

__global__ void embed_pad_kernel(const double *__restrict__ A, int Dout, int Din, double *__restrict__ P, int rows, int Dinp) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)rows * Dinp) return;
  const int r = (int)(idx / Dinp), c = (int)(idx % Dinp);
  P[idx] = (r < Dout && c < Din) ? A[(int64_t)r * Din + c] : 0.0;
}

template <typename TIN, int NT, int CH>
static int launch_fused(plda_handle *h, const TIN *dX, int64_t R, double *dout, int cus) {
  using G = EmGeom<NT, CH>;
  static_assert(G::LDS_BYTES <= 160 * 1024, "stage buffers exceed the LDS of a CU");
  static_assert((size_t)G::SCRATCH <= (size_t)2 * G::STAGE, "the epilogue's scratch must fit the stage buffers");
  static DeviceOnce attr;          // (per instantiation and device; setting it twice is harmless)
  if (attr.needed(h->device)) {
    PLDA_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&embed_fused_kernel<TIN, NT, CH>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_BYTES));
    attr.done(h->device);
  }
  embed_fused_kernel<TIN, NT, CH><<<(unsigned)std::min<int64_t>(ceil_div(R, (int64_t)G::ROWS), cus), 512, G::LDS_BYTES, h->stream>>>(
      dX, R, h->em_Din, h->em_apad.as<double>(), h->em_dinp, h->em_Dout, h->em_has_min ? h->em_min.as<double>() : nullptr,
      h->em_len_in, h->em_has_mout ? h->em_mout.as<double>() : nullptr, h->em_len_out, dout);
  PLDA_LAUNCH_CHECK(h);
  return PLDA_OK;
}

// the block shapes of one Dout class: main <NT0, CH0>, tails <NT1, 2> (CH0 = 1 only), <NT2, 4>, <NT3, 8>
template <typename TIN, int NT0, int CH0, int NT1, int NT2, int NT3>
static int fused_class(plda_handle *h, const TIN *dX, int64_t R, double *dout) {
  constexpr int ROWS0 = EmGeom<NT0, CH0>::ROWS;
  const int64_t G = h->embed_cus > 0 ? h->embed_cus : h->num_cus;
  const int Din = h->em_Din, Dout = h->em_Dout;
  const int64_t nb = ceil_div(R, (int64_t)ROWS0);
  const int64_t rows_main = std::min(R, nb / G * G * ROWS0);   // a whole number of rounds of the persistent grid
  if (rows_main > 0) PLDA_TRY((launch_fused<TIN, NT0, CH0>(h, dX, rows_main, dout, (int)G)));
  const int64_t Rt = R - rows_main;
  if (Rt <= 0) return PLDA_OK;
  const TIN *tX = dX + rows_main * Din;
  double *to = dout + rows_main * (int64_t)Dout;
  const int64_t per_cu = ceil_div(Rt, G);
  if (per_cu <= 16) return launch_fused<TIN, NT3, 8>(h, tX, Rt, to, (int)G);
  if (per_cu <= 32) return launch_fused<TIN, NT2, 4>(h, tX, Rt, to, (int)G);
  if constexpr (CH0 == 1) {
    if (per_cu <= 64) return launch_fused<TIN, NT1, 2>(h, tX, Rt, to, (int)G);
  }
  return launch_fused<TIN, NT0, CH0>(h, tX, Rt, to, (int)G);
}

template <typename TIN>
static int fused_dispatch(plda_handle *h, const TIN *dX, int64_t R, double *dout) {
  const int D = h->em_Dout;
  if (D <= 128) return fused_class<TIN, 8, 1, 4, 2, 1>(h, dX, R, dout);
  if (D <= 208) return fused_class<TIN, 13, 1, 7, 4, 2>(h, dX, R, dout);
  if (D <= 256) return fused_class<TIN, 16, 1, 8, 4, 2>(h, dX, R, dout);
  if (D <= 384) return fused_class<TIN, 12, 2, 12, 6, 3>(h, dX, R, dout);
  return fused_class<TIN, 8, 4, 8, 8, 4>(h, dX, R, dout);
}

// main block shape of a class-1 chain: rows per workgroup, LDS bytes, rows of the padded A
static void fused_shape(int Dout, int *rows, int *lds, int *padrows) {
  if (Dout <= 128) { *rows = 128; *lds = (int)EmGeom<8, 1>::LDS_BYTES; *padrows = 128; }
  else if (Dout <= 208) { *rows = 128; *lds = (int)EmGeom<13, 1>::LDS_BYTES; *padrows = 256; }
  else if (Dout <= 256) { *rows = 128; *lds = (int)EmGeom<16, 1>::LDS_BYTES; *padrows = 256; }
  else if (Dout <= 384) { *rows = 64; *lds = (int)EmGeom<12, 2>::LDS_BYTES; *padrows = 384; }
  else { *rows = 32; *lds = (int)EmGeom<8, 4>::LDS_BYTES; *padrows = 512; }
}
static_assert(EmGeom<8, 1>::TR <= 128 && EmGeom<4, 2>::TR <= 128 && EmGeom<2, 4>::TR <= 128 && EmGeom<1, 8>::TR <= 128, "padded A");
static_assert(EmGeom<13, 1>::TR <= 256 && EmGeom<7, 2>::TR <= 256 && EmGeom<4, 4>::TR <= 256 && EmGeom<2, 8>::TR <= 256, "padded A");
static_assert(EmGeom<16, 1>::TR <= 256 && EmGeom<8, 2>::TR <= 256, "padded A");
static_assert(EmGeom<12, 2>::TR <= 384 && EmGeom<6, 4>::TR <= 384 && EmGeom<3, 8>::TR <= 384, "padded A");
static_assert(EmGeom<8, 4>::TR <= 512 && EmGeom<4, 8>::TR <= 512, "padded A");

static int embed_class_of(const plda_handle *h, int Dout, bool has_A) {
  if (!has_A) return 0;
  return (Dout <= 512 && h->embed_variant != 1) ? 1 : 2;
}

int embed_plan(plda_handle *h, int Din, int Dout, int has_A, int dtype, int32_t *out) {
  if (!out) return fail(h, PLDA_E_INVAL, "embed_plan: out is NULL");
  if (Din < 1 || Din > PLDA_EMBED_MAX_DIN || Dout < 1 || Dout > PLDA_EMBED_MAX_DOUT || (dtype != 0 && dtype != 1) ||
      (!has_A && Dout != Din))
    return fail(h, PLDA_E_INVAL, "embed_plan: Din %d (1 ... %d), Dout %d (1 ... %d; = Din without A), dtype %d (0 fp64, 1 fp32)", Din,
                PLDA_EMBED_MAX_DIN, Dout, PLDA_EMBED_MAX_DOUT, dtype);
  const int cls = embed_class_of(h, Dout, has_A != 0);
  out[0] = cls;
  if (cls == 1) {
    int rows, lds, pad;
    fused_shape(Dout, &rows, &lds, &pad);
    out[1] = rows; out[2] = lds;
  } else {
    out[1] = 4; out[2] = 0;      // one wave per row, four rows per workgroup, no LDS
  }
  return PLDA_OK;
}

static bool all_finite(const double *p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

// everything is checked before anything of the handle is touched: a refused chain leaves the installed one as it was
int embed_set(plda_handle *h, int Din, int Dout, const double *m_in, double len_in, const double *A, const double *m_out,
              double len_out) {
  if (Din < 1 || Din > PLDA_EMBED_MAX_DIN || Dout < 1 || Dout > PLDA_EMBED_MAX_DOUT)
    return fail(h, PLDA_E_INVAL, "embed_set: Din %d (1 ... %d), Dout %d (1 ... %d)", Din, PLDA_EMBED_MAX_DIN, Dout, PLDA_EMBED_MAX_DOUT);
  if (!A && Dout != Din) return fail(h, PLDA_E_INVAL, "embed_set: without A, Dout %d must equal Din %d", Dout, Din);
  if (!(len_in >= 0.0) || !std::isfinite(len_in) || !(len_out >= 0.0) || !std::isfinite(len_out))
    return fail(h, PLDA_E_INVAL, "embed_set: len_in and len_out must be finite and >= 0");
  if ((m_in && !all_finite(m_in, (size_t)Din)) || (A && !all_finite(A, (size_t)Dout * Din)) || (m_out && !all_finite(m_out, (size_t)Dout)))
    return fail(h, PLDA_E_INVAL, "embed_set: m_in, A and m_out must be finite");
  // host mirrors first (they may throw std::bad_alloc: built aside and swapped in)
  std::vector<double> hm, ha, ho;
  if (m_in) hm.assign(m_in, m_in + Din);
  if (A) ha.assign(A, A + (size_t)Dout * Din);
  if (m_out) ho.assign(m_out, m_out + Dout);
  const int cls = embed_class_of(h, Dout, A != nullptr);
  int rows = 0, lds = 0, padrows = 0;
  const int dinp = (int)round_up(Din, 16);
  if (cls == 1) fused_shape(Dout, &rows, &lds, &padrows);
  h->em_has = false;               // (a HIP error below leaves no chain rather than half of one)
  PLDA_HIP(h, h->em_min.reserve((size_t)Din * 8));
  PLDA_HIP(h, h->em_mout.reserve((size_t)Dout * 8));
  if (A) PLDA_HIP(h, h->em_A.reserve((size_t)Dout * Din * 8));
  if (cls == 1) PLDA_HIP(h, h->em_apad.reserve((size_t)padrows * dinp * 8));
  if (m_in) PLDA_HIP(h, hipMemcpyAsync(h->em_min.p, hm.data(), (size_t)Din * 8, hipMemcpyHostToDevice, h->stream));
  if (m_out) PLDA_HIP(h, hipMemcpyAsync(h->em_mout.p, ho.data(), (size_t)Dout * 8, hipMemcpyHostToDevice, h->stream));
  if (A) PLDA_HIP(h, hipMemcpyAsync(h->em_A.p, ha.data(), (size_t)Dout * Din * 8, hipMemcpyHostToDevice, h->stream));
  if (cls == 1) {
    embed_pad_kernel<<<(unsigned)ceil_div((int64_t)padrows * dinp, 256), 256, 0, h->stream>>>(h->em_A.as<double>(), Dout, Din,
                                                                                             h->em_apad.as<double>(), padrows, dinp);
    PLDA_LAUNCH_CHECK(h);
  }
  PLDA_HIP(h, hipStreamSynchronize(h->stream));   // the copies read hm / ha / ho
  h->em_h_min.swap(hm); h->em_h_A.swap(ha); h->em_h_mout.swap(ho);
  h->em_Din = Din; h->em_Dout = Dout; h->em_len_in = len_in; h->em_len_out = len_out;
  h->em_has_min = m_in != nullptr; h->em_has_A = A != nullptr; h->em_has_mout = m_out != nullptr;
  h->em_dinp = dinp; h->em_class = cls;
  h->em_has = true;
  return PLDA_OK;
}

int embed_clear(plda_handle *h) {
  h->em_has = false;
  h->em_h_min.clear(); h->em_h_A.clear(); h->em_h_mout.clear();
  return PLDA_OK;
}

template <typename TIN>
static int embed_apply_t(plda_handle *h, const TIN *dX, int64_t R, double *dout) {
  const int Din = h->em_Din, Dout = h->em_Dout;
  const double *mi = h->em_has_min ? h->em_min.as<double>() : nullptr, *mo = h->em_has_mout ? h->em_mout.as<double>() : nullptr;
  if (h->em_class == 0) {
    TraceScope ts(h, "embed.rows (K18 class 0)", (double)R * Din * (sizeof(TIN) + 8.0), 2);
    return launch_rows<TIN>(h, dX, R, R, Din, mi, h->em_len_in, mo, h->em_len_out, dout);
  }
  if (h->em_class == 1) {
    TraceScope ts(h, "embed.fused (K18 class 1)", 2.0 * (double)R * Dout * Din, 1);
    return fused_dispatch<TIN>(h, dX, R, dout);
  }
  TraceScope ts(h, "embed.rows + gemm + rows (K18 class 2)", 2.0 * (double)R * Dout * Din, 1);
  PLDA_HIP(h, h->em_v.reserve((size_t)EMBED_CHUNK * Din * 8));
  PLDA_HIP(h, h->em_g.reserve((size_t)EMBED_CHUNK * Dout * 8));
  double *V = h->em_v.as<double>(), *Gm = h->em_g.as<double>();
  for (int64_t r0 = 0; r0 < R; r0 += EMBED_CHUNK) {
    const int64_t rc = std::min(EMBED_CHUNK, R - r0);
    PLDA_TRY(launch_rows<TIN>(h, dX + r0 * Din, rc, EMBED_CHUNK, Din, mi, h->em_len_in, nullptr, 0.0, V));
    PLDA_TRY(gemm_f64(h, EMBED_CHUNK, Dout, Din, 1.0, V, Din, 1, h->em_A.as<double>(), 1, Din, nullptr, 0.0, Gm, Dout));
    PLDA_TRY(launch_rows<double>(h, Gm, rc, rc, Dout, mo, h->em_len_out, nullptr, 0.0, dout + r0 * (int64_t)Dout));
  }
  return PLDA_OK;
}

int embed_apply_device(plda_handle *h, const void *dX, int dtype, int64_t R, int Din, double *dout) {
  if (!h->em_has) return fail(h, PLDA_E_NOT_FITTED, "embed_apply: no embedding chain is set");
  if (dtype != 0 && dtype != 1) return fail(h, PLDA_E_INVAL, "embed_apply: dtype %d (0 fp64, 1 fp32)", dtype);
  if (Din != h->em_Din) return fail(h, PLDA_E_INVAL, "embed_apply: feature dim %d != the chain's input dim %d", Din, h->em_Din);
  if (R <= 0) return PLDA_OK;
  if (!dX || !dout) return fail(h, PLDA_E_INVAL, "embed_apply: bad argument");
  return dtype == 1 ? embed_apply_t<float>(h, static_cast<const float *>(dX), R, dout)
                    : embed_apply_t<double>(h, static_cast<const double *>(dX), R, dout);
}

// ------------------------------------------------------------------------------------
// the fit (plda_embed_fit*): m_in, v, mu and the statistics on the device with the library's own building blocks (the
// centroid kernels of fit.hip, the fp64 GEMM / SYRK, sym_eig, the simultaneous diagonalisation of linalg.hip); the last
// step -- scaling Dout rows of a D x D matrix and m_out = A mu -- on the host, which receives the chain anyway.
// Scratch (h->em_fit): all of v [N, Din] (not in slabs: the centroid pass and the SYRK of the centred rows both want every
// row), D x D matrices, the class means.
// ------------------------------------------------------------------------------------
constexpr int CS_ROWS = 256;   // rows of one partial column sum

// part[b][d] = sum over the rows i of chunk b, in order, of X[i][d] - X[0][d] (the pilot row: a data offset costs nothing)
template <typename TIN>
__global__ __launch_bounds__(256) void embed_colsum_kernel(const TIN *__restrict__ X, int64_t N, int D, double *__restrict__ part) {
  const int64_t i0 = (int64_t)blockIdx.x * CS_ROWS, i1 = min(N, i0 + CS_ROWS);
  for (int d = threadIdx.x; d < D; d += 256) {
    const double p = (double)X[d];
    double sacc = 0.0;
    for (int64_t i = i0; i < i1; ++i) sacc += (double)X[i * D + d] - p;
    part[(int64_t)blockIdx.x * D + d] = sacc;
  }
}
// mean[d] = X[0][d] + (sum of the partials, in order) / N
template <typename TIN>
__global__ void embed_colmean_kernel(const TIN *__restrict__ X, int64_t N, int D, const double *__restrict__ part, int64_t nparts,
                                     double *__restrict__ mean) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  double sacc = 0.0;
  for (int64_t b = 0; b < nparts; ++b) sacc += part[b * D + d];
  mean[d] = (double)X[d] + sacc / (double)N;
}
// V[i][d] -= (labels ? means[labels[i]][d] : means[d])
__global__ void embed_center_kernel(double *__restrict__ V, const uint64_t *__restrict__ labels, const double *__restrict__ means,
                                    int64_t N, int D) {
  const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (idx >= N * D) return;
  const int64_t i = idx / D;
  const int d = (int)(idx - i * D);
  V[idx] -= means[(labels ? (int64_t)labels[i] * D : 0) + d];
}
// Mc[k][d] = means[k][d] - mu[d];  wk[k] = counts[k] / N
__global__ void embed_between_rows_kernel(const double *__restrict__ means, const double *__restrict__ mu, const int32_t *__restrict__ counts,
                                          int64_t K, int D, double inv_n, double *__restrict__ Mc, double *__restrict__ wk) {
  const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (idx >= K * D) return;
  const int64_t k = idx / D;
  const int d = (int)(idx - k * D);
  Mc[idx] = means[idx] - mu[d];
  if (d == 0) wk[k] = (double)counts[k] * inv_n;
}
__global__ void embed_symmetrize_kernel(double *__restrict__ S, int D) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= D * D) return;
  const int i = idx / D, j = idx % D;
  if (j >= i) return;
  const double a = 0.5 * (S[(size_t)i * D + j] + S[(size_t)j * D + i]);
  S[(size_t)i * D + j] = a;
  S[(size_t)j * D + i] = a;
}
// *flag = 1 where a Cholesky pivot of W, 1 / T1[k][k]^2 with T1 = chol(W)^-1, is not above the rounding error of its own
// computation (the rule of lda_pivot_check_kernel, lda.hip): W is singular to working precision
__global__ void embed_pivot_check_kernel(const double *__restrict__ T1, const double *__restrict__ W, int D, int *__restrict__ flag) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= D) return;
  const double tt = T1[(size_t)k * D + k];
  if (!(1.0 / (tt * tt) > (double)D * 2.220446049250313e-16 * W[(size_t)k * D + k])) *flag = 1;
}

template <typename TIN>
static int column_mean(plda_handle *h, const TIN *X, int64_t N, int D, double *part, double *mean) {
  const int64_t nparts = ceil_div(N, (int64_t)CS_ROWS);
  embed_colsum_kernel<TIN><<<(unsigned)nparts, 256, 0, h->stream>>>(X, N, D, part);
  PLDA_LAUNCH_CHECK(h);
  embed_colmean_kernel<TIN><<<(unsigned)ceil_div(D, 256), 256, 0, h->stream>>>(X, N, D, part, nparts, mean);
  PLDA_LAUNCH_CHECK(h);
  return PLDA_OK;
}

int embed_fit_validate(plda_handle *h, int dtype, int64_t N, int Din, bool has_labels, int64_t K, int kind, int Dout, double len_in,
                       double len_out) {
  if (dtype != 0 && dtype != 1) return fail(h, PLDA_E_INVAL, "embed_fit: dtype %d (0 fp64, 1 fp32)", dtype);
  if (kind < 0 || kind > 2) return fail(h, PLDA_E_INVAL, "embed_fit: kind %d (0 centre, 1 whiten, 2 lda)", kind);
  if (Din < 1 || Din > PLDA_EMBED_MAX_DIN || Dout < 1 || Dout > PLDA_EMBED_MAX_DOUT)
    return fail(h, PLDA_E_INVAL, "embed_fit: Din %d (1 ... %d), Dout %d (1 ... %d)", Din, PLDA_EMBED_MAX_DIN, Dout, PLDA_EMBED_MAX_DOUT);
  if (kind == 0 ? Dout != Din : Dout > Din)
    return fail(h, PLDA_E_INVAL, "embed_fit: Dout %d with Din %d (kind 0: equal; kinds 1, 2: Dout <= Din)", Dout, Din);
  if (kind != 0 && Din > 2048) return fail(h, PLDA_E_INVAL, "embed_fit: kinds 1 and 2 take Din <= 2048 (the eigensolver's limit), got %d", Din);
  if (N < 2 || N >= ((int64_t)1 << 31)) return fail(h, PLDA_E_INVAL, "embed_fit: N = %lld (2 ... 2^31 - 1)", (long long)N);
  if (!(len_in >= 0.0) || !std::isfinite(len_in) || !(len_out >= 0.0) || !std::isfinite(len_out))
    return fail(h, PLDA_E_INVAL, "embed_fit: len_in and len_out must be finite and >= 0");
  if (kind == 2) {
    if (!has_labels) return fail(h, PLDA_E_INVAL, "embed_fit: kind 2 (lda) needs labels");
    if (K < 2 || K > N) return fail(h, PLDA_E_INVAL, "embed_fit: K = %lld classes (2 ... N)", (long long)K);
  }
  return PLDA_OK;
}

template <typename TIN>
static int embed_fit_t(plda_handle *h, const TIN *dX, int64_t N, int D, const uint64_t *dlabels, int64_t K, int kind, int Dout,
                       double len_in, double len_out, double *eig) {
  const size_t DD = (size_t)D * D, KD = kind == 2 ? (size_t)K * D : 0;
  const int64_t nparts = ceil_div(N, (int64_t)CS_ROWS);
  // [V N*D][part nparts*D][m_in D][mu D][lam D][S DD][S2 DD][T DD][means KD][Mc KD][wk K][counts K][flag]
  const size_t doubles = (size_t)N * D + (size_t)nparts * D + 3 * (size_t)D + (kind ? 3 * DD : 0) + 2 * KD + (kind == 2 ? (size_t)K : 0);
  PLDA_HIP(h, h->em_fit.reserve(doubles * 8 + (kind == 2 ? (size_t)K * 4 : 0) + 64));
  double *V = h->em_fit.as<double>(), *part = V + (size_t)N * D, *dmin = part + (size_t)nparts * D, *dmu = dmin + D, *lam = dmu + D,
         *S = lam + D, *S2 = S + (kind ? DD : 0), *T = S2 + (kind ? DD : 0), *means = T + (kind ? DD : 0), *Mc = means + KD, *wk = Mc + KD;
  int32_t *counts = reinterpret_cast<int32_t *>(wk + (kind == 2 ? K : 0));
  int *dflag = reinterpret_cast<int *>(counts + (kind == 2 ? K : 0)) + 1;

  TraceScope ts(h, "embed.fit (K18)");
  PLDA_TRY(column_mean<TIN>(h, dX, N, D, part, dmin));
  PLDA_TRY(launch_rows<TIN>(h, dX, N, N, D, dmin, len_in, nullptr, 0.0, V));
  PLDA_TRY(column_mean<double>(h, V, N, D, part, dmu));
  std::vector<double> hmin((size_t)D), hmu((size_t)D);
  PLDA_HIP(h, hipMemcpyAsync(hmin.data(), dmin, (size_t)D * 8, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(hmu.data(), dmu, (size_t)D * 8, hipMemcpyDeviceToHost, h->stream));
  if (kind == 0) {
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
    return embed_set(h, D, D, hmin.data(), len_in, nullptr, hmu.data(), len_out);
  }
  const unsigned nd_blocks = (unsigned)ceil_div(N * (int64_t)D, 256), dd_blocks = (unsigned)ceil_div((int64_t)DD, 256);
  std::vector<double> hl((size_t)D), hT((size_t)Dout * D);
  if (kind == 1) {
    embed_center_kernel<<<nd_blocks, 256, 0, h->stream>>>(V, nullptr, dmu, N, D);
    PLDA_LAUNCH_CHECK(h);
    PLDA_TRY(gemm_f64(h, D, D, N, 1.0 / (double)N, V, 1, D, V, D, 1, nullptr, 0.0, S, D));
    embed_symmetrize_kernel<<<dd_blocks, 256, 0, h->stream>>>(S, D);
    PLDA_LAUNCH_CHECK(h);
    PLDA_TRY(sym_eig_auto_f64(h, S, D, lam, T));            // eigenvalues descending, eigenvectors in the rows of T
    PLDA_HIP(h, hipMemcpyAsync(hl.data(), lam, (size_t)D * 8, hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipMemcpyAsync(hT.data(), T, (size_t)Dout * D * 8, hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
    if (!(hl[Dout - 1] > (double)N * (double)D * 1.1102230246251565e-16 * hl[0]))
      return fail(h, PLDA_E_NUMERIC, "embed_fit: eigenvalue %d of the covariance (%g) is not above N Din 2^-53 times the largest (%g)",
                  Dout - 1, hl[Dout - 1], hl[0]);
    for (int i = 0; i < Dout; ++i) {
      const double sc = 1.0 / std::sqrt(hl[i]);
      for (int d = 0; d < D; ++d) hT[(size_t)i * D + d] *= sc;
    }
  } else {
    PLDA_TRY(group_means_device(h, V, N, D, dlabels, K, means, counts));
    std::vector<int32_t> hc((size_t)K);
    PLDA_HIP(h, hipMemcpyAsync(hc.data(), counts, (size_t)K * 4, hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
    for (int64_t k = 0; k < K; ++k)
      if (hc[k] <= 0) return fail(h, PLDA_E_LABELS, "embed_fit: labels must be dense 0..K-1 (label %lld unused)", (long long)k);
    embed_between_rows_kernel<<<(unsigned)ceil_div(K * (int64_t)D, 256), 256, 0, h->stream>>>(means, dmu, counts, K, D, 1.0 / (double)N, Mc, wk);
    embed_center_kernel<<<nd_blocks, 256, 0, h->stream>>>(V, dlabels, means, N, D);
    PLDA_LAUNCH_CHECK(h);
    double *W = S, *B = S2;
    PLDA_TRY(gemm_f64(h, D, D, N, 1.0 / (double)N, V, 1, D, V, D, 1, nullptr, 0.0, W, D));
    PLDA_TRY(gemm_f64(h, D, D, K, 1.0, Mc, 1, D, Mc, D, 1, wk, 0.0, B, D));
    embed_symmetrize_kernel<<<dd_blocks, 256, 0, h->stream>>>(W, D);
    embed_symmetrize_kernel<<<dd_blocks, 256, 0, h->stream>>>(B, D);
    PLDA_LAUNCH_CHECK(h);
    h->simdiag_has_vr = false;
    PLDA_TRY(simdiag_f64(h, W, B, D, T, nullptr, lam, false));   // T W T^T = I, T B T^T = diag(lam), descending
    int hsing = 0;
    PLDA_HIP(h, hipMemsetAsync(dflag, 0, sizeof(int), h->stream));
    embed_pivot_check_kernel<<<(unsigned)ceil_div(D, 256), 256, 0, h->stream>>>(simdiag_whitening(h, D), W, D, dflag);
    PLDA_LAUNCH_CHECK(h);
    PLDA_HIP(h, hipMemcpyAsync(&hsing, dflag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipMemcpyAsync(hl.data(), lam, (size_t)D * 8, hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipMemcpyAsync(hT.data(), T, (size_t)Dout * D * 8, hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
    if (hsing) return fail(h, PLDA_E_NUMERIC, "embed_fit: the within-class covariance is not positive definite");
  }
  std::vector<double> hmo((size_t)Dout);
  for (int i = 0; i < Dout; ++i) {
    double sacc = 0.0;
    for (int d = 0; d < D; ++d) sacc = std::fma(hT[(size_t)i * D + d], hmu[d], sacc);
    hmo[i] = sacc;
  }
  PLDA_TRY(embed_set(h, D, Dout, hmin.data(), len_in, hT.data(), hmo.data(), len_out));
  if (eig) std::memcpy(eig, hl.data(), (size_t)Dout * 8);
  return PLDA_OK;
}

int embed_fit_device(plda_handle *h, const void *dX, int dtype, int64_t N, int Din, const uint64_t *dlabels, int64_t K, int kind,
                     int Dout, double len_in, double len_out, double *eig) {
  PLDA_TRY(embed_fit_validate(h, dtype, N, Din, dlabels != nullptr, K, kind, Dout, len_in, len_out));
  if (!dX) return fail(h, PLDA_E_INVAL, "embed_fit: X is NULL");
  return dtype == 1 ? embed_fit_t<float>(h, static_cast<const float *>(dX), N, Din, dlabels, K, kind, Dout, len_in, len_out, eig)
                    : embed_fit_t<double>(h, static_cast<const double *>(dX), N, Din, dlabels, K, kind, Dout, len_in, len_out, eig);
}

}  // namespace plda
