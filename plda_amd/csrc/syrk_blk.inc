// plda_amd/csrc/syrk_blk.inc -- K2 for 208 < D <= 512 (round 4): C = X^T diag(w) X + w2 X2^T X2, lower triangle, from ONE
// read of full rows.  Included by linalg.hip inside namespace plda.
//
// Replaces the scatter of PldaStats::AddSamples (offset_scatter.AddMat2 / AddVec2, reached from
// /root/reference/src/pldamodule.cpp:94-98) for the BASELINE shapes C3 (D = 512) and C4 (D = 256).
//
// What it replaces here: syrk_lower_kernel launches the lower-triangular 128 x 128 super-tiles, each re-reading two
// 128-column slabs of X per row chunk -- 16 GB moved for the 4 GB of rows at C3, MFMA pipe 40 % busy by the executed
// (triangle) count, 8.3 ms (round-3 review, weak 3 / 4).  The triangle of a 512-wide product is 1 MB of fp64 accumulators,
// twice a CU's register file, so the unit of work is a GROUP of up to four workgroups on one XCD that share a row chunk:
//   * the D x D output is cut into 64 x 64 blocks of 4 x 4 MFMA tiles (v_mfma_f64_16x16x4_f64); a wave owns either one block
//     below the diagonal (16 tiles) or two blocks on it (10 tiles each: the tiles with column <= row).  D = 512: 28 + 8
//     blocks = 32 waves = 4 workgroups; D = 256: 6 + 4 blocks = 8 waves = 1 workgroup.  A and B operands of a tile are the
//     same kind of fragment (4 rows x 16 columns of X, row-major in LDS), so a full block reads 8 fragments per 16 MFMAs
//     and a diagonal block 4 per 10;
//   * every workgroup stages the FULL rows of its group's chunk, 16 rows per stage, two stages in LDS (128 KiB at D = 512),
//     by LDS DMA (buffer_load ... lds, 1 KiB = 128 columns of one row per instruction); the workgroups of a group sit on
//     one XCD (block b -> XCD b % 8) and walk the chunk together, so the rows come from HBM once and from that L2 after;
//   * the pipeline is the trials GEMM's: the stage barrier sits in front of a stage's LAST k-step, whose fragments are in
//     registers by then; behind it the next stage's first fragments are fetched and the DMA of the stage after next goes
//     into the buffer just freed;
//   * row weights (1 / n_label, the wrapper's class weight pldamodule.cpp:97; -1 for the centroid rows of the pair form)
//     ride through LDS beside the rows and multiply the B-side fragments after their LDS read;
//   * partial sums of the computed tiles only, one slab per group, summed in fixed order and mirrored by
//     syrk_tri_reduce_kernel (deterministic, exactly symmetric).
// Needs D and the row strides even (16-byte DMA granules).
constexpr int SB_ROWS = 16;                      // rows per stage
constexpr int SB_MAXWAVES = 32;                  // waves of a group

struct SyrkBlkPlan {
  // per wave of the group: unit 0 and unit 1 as (row block) | (column block << 8) | (kind << 16); kind 0 none, 1 full, 2 diagonal
  int unit[SB_MAXWAVES][2];
  int nwg;                                       // workgroups per group
};

#define SBK_SB __builtin_amdgcn_sched_barrier(0)
// vmcnt(0) lgkmcnt(0) + s_barrier, with COMPILER barriers on both sides.  llvm.amdgcn.s.barrier is IntrNoMem: without the memory
// clobbers the optimiser is free to move plain LDS loads across it, and it did -- the fragment reads of a stage's LAST k-step were
// sunk below the stage barrier (they are first used behind it), where another wave's DMA of the stage after next may already be
// overwriting the buffer: one k-step of one wave multiplied rows of two different stages, a rank-2..6 error in ONE 64 x 64 block
// about once in a thousand launches (round 6: tests/test_gpu_fit.py::test_statistics_pass_block_scatter_kernel[512-6000-100]
// failed in 2 of 10 runs of the whole suite; scripts/stress_scatter.py reproduces it).
#define SBK_BARRIER()                          \
  do {                                         \
    asm volatile("" ::: "memory");             \
    __builtin_amdgcn_s_waitcnt(0x0070);        \
    __builtin_amdgcn_s_barrier();              \
    asm volatile("" ::: "memory");             \
  } while (0)

struct SyrkBlkArgs {
  int D;
  int64_t K[2], rows[2], ld[2];                  // per phase (matrix): rows in all, rows per group, row stride in doubles
  const double *M[2], *W[2];                     // per phase: the matrix and its row weights
  double *part;
};

// One wave's share of a group's chunk.  KIND 1: one full block (row block rb0, column block cb0); KIND 2: two diagonal
// blocks rb0, rb1; KIND 0: no tiles (it still moves its share of the rows and meets the barriers).  The three instantiations
// run side by side in one workgroup: s_barrier counts waves, not program counters.
template <int KIND>
__device__ __forceinline__ void syrk_blk_wave(const SyrkBlkArgs &g, int group, int wave, int lane, int rb0, int cb0, int rb1, bool has1,
                                              double *sb_smem) {
  constexpr int NACC = KIND == 1 ? 16 : KIND == 2 ? 20 : 1;
  constexpr int NA = KIND == 2 ? 8 : 4;          // row-side fragments per k-step (KIND 2: both blocks')
  constexpr int NB = KIND == 1 ? 4 : 0;          // column-side fragments (full blocks)
  const int D = g.D;
  const int fi = lane & 15, fk = lane >> 4;
  const int ncp = (D + 127) / 128;               // 1 KiB pieces per row
  const int pitch = ncp * 128;                   // doubles per staged row: whole pieces (a piece always writes 1 KiB of LDS)
  const int stage_doubles = SB_ROWS * pitch;
  typedef __attribute__((address_space(3))) char lds_char;
  lds_char *const lds = (lds_char *)sb_smem;
  const double *const Ws = sb_smem + 2 * stage_doubles;   // 2 x 32 doubles of row weights
  const int npieces = SB_ROWS * ncp;             // pieces of a stage; wave w moves pieces w, w + 8, ...

  f64x4 acc[NACC];
#pragma unroll
  for (int c = 0; c < NACC; ++c) acc[c] = f64x4{0.0, 0.0, 0.0, 0.0};
  // per-lane column offset inside a piece: 2 doubles per lane; a piece's first column rides on the scalar offset, the last
  // piece of a row whose width is not a multiple of 128 re-reads the row's last two columns in its surplus lanes
  const int lastw = D - (ncp - 1) * 128;         // columns of the last piece
  const unsigned vo_full = (unsigned)(2 * lane) * 8u;
  const unsigned vo_last = (unsigned)(2 * lane > lastw - 2 ? lastw - 2 : 2 * lane) * 8u;

  for (int ph = 0; ph < 2; ++ph) {
    const int64_t g0 = (int64_t)group * g.rows[ph];
    const int64_t g1 = g0 + g.rows[ph] < g.K[ph] ? g0 + g.rows[ph] : g.K[ph];
    if (g0 >= g1) continue;                       // (uniform over the workgroup)
    const int64_t nrows = g1 - g0;
    const int nstages = (int)((nrows + SB_ROWS - 1) / SB_ROWS);
    const __amdgpu_buffer_rsrc_t rsM = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(g.M[ph] + g0 * g.ld[ph]), 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(g.W[ph] + g0), 0, -1, 0x00020000);
    const unsigned rowbytes = (unsigned)g.ld[ph] * 8u;
    int d_stage = 0;                              // the stage the DMA cursor fills next
    auto dma_stage = [&]() {
      const int buf = d_stage & 1;
      const int r0 = d_stage * SB_ROWS;
      int r = 0, c = wave;                        // piece p = wave, wave + 8, ...: row p / ncp, piece-in-row p % ncp
      while (c >= ncp) { c -= ncp; ++r; }
      for (int p = wave; p < npieces; p += 8) {
        int row = r0 + r;
        row = row > (int)nrows - 1 ? (int)nrows - 1 : row;   // past the end: a valid row again, its weight is zeroed below
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsM, (lds_char *)(lds + ((size_t)buf * stage_doubles + (size_t)r * pitch) * 8 + c * 1024), 16,
                                                 (int)(c == ncp - 1 ? vo_last : vo_full), (int)((unsigned)row * rowbytes + (unsigned)c * 1024u), 0, 0);
        c += 8;
        while (c >= ncp) { c -= ncp; ++r; }
      }
      if (wave == 0) {
        // 16 weights = 128 B: lanes 0 .. 31 carry them (4 B per lane), the others re-read the last one
        int wrow = r0 * 2 + (lane < 32 ? lane : 31);          // in dwords
        const int wmax = (int)nrows * 2 - 1;
        wrow = wrow > wmax ? wmax : wrow;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (lds_char *)(lds + ((size_t)2 * stage_doubles + (size_t)buf * 32) * 8), 4,
                                                 (int)((unsigned)wrow * 4u), 0, 0, 0);
      }
      ++d_stage;
    };
    dma_stage();
    SBK_BARRIER();
    if (nstages > 1) dma_stage();

    // fragments of one k-step (4 rows) of buffer `buf`; w = the k-step's row weight of this lane (0 past the end)
    auto load_frags = [&](int buf, int kk, int r0, double (&a)[NA > 0 ? NA : 1], double (&b)[NB > 0 ? NB : 1], double &w) {
      const double *Xr = sb_smem + (size_t)buf * stage_doubles + (size_t)(kk * 4 + fk) * pitch + fi;
      if (KIND != 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = Xr[rb0 * 64 + i * 16];
      }
      if (KIND == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = Xr[cb0 * 64 + i * 16];
      }
      if (KIND == 2) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[4 + i] = Xr[rb1 * 64 + i * 16];
      }
      const double wl = Ws[buf * 32 + kk * 4 + fk];
      w = (r0 + kk * 4 + fk < (int)nrows) ? wl : 0.0;
    };
    auto mfma_step = [&](const double (&a)[NA > 0 ? NA : 1], const double (&b)[NB > 0 ? NB : 1], double w) {
      if (KIND == 1) {
        double bw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bw[j] = b[j] * w;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i * 4 + j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], bw[j], acc[i * 4 + j], 0, 0, 0);
      } else if (KIND == 2) {
        double aw[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) aw[j] = a[j] * w;
        // the two blocks' chains interleaved
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j <= i; ++j) {
            acc[i * (i + 1) / 2 + j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], aw[j], acc[i * (i + 1) / 2 + j], 0, 0, 0);
            acc[10 + i * (i + 1) / 2 + j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[4 + i], aw[4 + j], acc[10 + i * (i + 1) / 2 + j], 0, 0, 0);
          }
      }
    };

    double xa[NA > 0 ? NA : 1], xb[NB > 0 ? NB : 1], ya[NA > 0 ? NA : 1], yb[NB > 0 ? NB : 1], xw = 0.0, yw = 0.0;
    load_frags(0, 0, 0, xa, xb, xw);
#pragma unroll 1
    for (int s = 0; s < nstages; ++s) {
      const int buf = s & 1;
      const int r0 = s * SB_ROWS;
      // k-steps 0, 1, 2 (fragments alternate between the x and the y set), then the early barrier, then k-step 3
      load_frags(buf, 1, r0, ya, yb, yw); SBK_SB;
      mfma_step(xa, xb, xw); SBK_SB;
      load_frags(buf, 2, r0, xa, xb, xw); SBK_SB;
      mfma_step(ya, yb, yw); SBK_SB;
      load_frags(buf, 3, r0, ya, yb, yw); SBK_SB;
      mfma_step(xa, xb, xw); SBK_SB;
      // every wave has its last fragments of this stage in registers and its DMAs of the next stage have landed
      SBK_BARRIER();
      SBK_SB;
      if (s + 1 < nstages) load_frags(buf ^ 1, 0, r0 + SB_ROWS, xa, xb, xw);
      SBK_SB;
      if (d_stage < nstages) dma_stage();                          // stage s + 2 into the buffer just freed
      SBK_SB;
      mfma_step(ya, yb, yw); SBK_SB;
    }
    SBK_BARRIER();                                  // the next phase's first DMA overwrites buffer 0
  }

  // partial: tile (r, c) at slot r (r + 1) / 2 + c, 256 doubles in the MFMA C layout (what syrk_tri_reduce_kernel sums)
  const int nt = (D + 15) / 16, ntri = nt * (nt + 1) / 2;
  double *slab = g.part + (int64_t)group * ntri * 256;
  auto put = [&](int tr, int tc, const f64x4 &v) {
    if (tr < nt && tc <= tr) {
      double *d = slab + ((int64_t)tr * (tr + 1) / 2 + tc) * 256 + lane;
#pragma unroll
      for (int r = 0; r < 4; ++r) d[r * 64] = v[r];
    }
  };
  if (KIND == 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) put(rb0 * 4 + i, cb0 * 4 + j, acc[i * 4 + j]);
  } else if (KIND == 2) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        put(rb0 * 4 + i, rb0 * 4 + j, acc[i * (i + 1) / 2 + j]);
        if (has1) put(rb1 * 4 + i, rb1 * 4 + j, acc[10 + i * (i + 1) / 2 + j]);
      }
  }
}

__global__ __launch_bounds__(512, 1) void syrk_blk_kernel(const SyrkBlkArgs g, const SyrkBlkPlan plan, int groups) {
  extern __shared__ __attribute__((aligned(16))) double sb_smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // block b -> XCD b % 8; the nwg workgroups of a group are consecutive on one XCD
  const int x = blockIdx.x & 7, seq = blockIdx.x >> 3;
  const int role = seq % plan.nwg, group = (seq / plan.nwg) * 8 + x;
  if (group >= groups) return;
  const int gw = role * 8 + wave;                                 // this wave's index in the group
  const int u0 = plan.unit[gw][0], u1 = plan.unit[gw][1];
  const int kind0 = u0 >> 16;
  const int rb0 = u0 & 255, cb0 = (u0 >> 8) & 255;
  const bool has1 = (u1 >> 16) == 2;
  const int rb1 = has1 ? (u1 & 255) : rb0;                        // (a lone diagonal block: its twin is computed, not written)
  if (kind0 == 1) syrk_blk_wave<1>(g, group, wave, lane, rb0, cb0, rb1, has1, sb_smem);
  else if (kind0 == 2) syrk_blk_wave<2>(g, group, wave, lane, rb0, cb0, rb1, has1, sb_smem);
  else syrk_blk_wave<0>(g, group, wave, lane, rb0, cb0, rb1, has1, sb_smem);
}
#undef SBK_SB
#undef SBK_BARRIER

__global__ void fill_f64_kernel(double *__restrict__ p, int64_t n, double v) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// host side: the group's wave plan, the row chunks, the launch.  Returns PLDA_OK and *used = true when the kernel applies.
static int syrk_blk_pair(plda_handle *h, int D, int64_t K1, const double *X, int64_t ldx, const double *kw, int64_t K2,
                         const double *X2, int64_t ldx2, double w2, double alpha, double beta, double *C, int64_t ldc, bool *used) {
  *used = false;
  if (D <= TRI_NT * 16 || D > 512 || (D & 1) || (ldx & 1) || (K2 > 0 && (ldx2 & 1)) || K1 <= 0) return PLDA_OK;
  if ((reinterpret_cast<uintptr_t>(X) & 15) || (K2 > 0 && (reinterpret_cast<uintptr_t>(X2) & 15))) return PLDA_OK;
  const int nb = (D + 63) / 64;
  SyrkBlkPlan plan;
  for (auto &u : plan.unit) u[0] = u[1] = 0;
  // full blocks first (one per wave), then the diagonal blocks in pairs; a group's diagonal waves are spread over its
  // workgroups (wave 7 of workgroup 0, 1, ...: they carry 20 tiles against 16)
  std::vector<int> full, diag;
  for (int r = 0; r < nb; ++r)
    for (int c = 0; c < r; ++c) full.push_back(r | (c << 8) | (1 << 16));
  for (int r = 0; r < nb; ++r) diag.push_back(r | (r << 8) | (2 << 16));
  const int ndw = (int)(diag.size() + 1) / 2, nwaves = (int)full.size() + ndw;
  if (nwaves > SB_MAXWAVES) return PLDA_OK;
  plan.nwg = (nwaves + 7) / 8;
  {
    std::vector<int> slots(plan.nwg * 8, -1);   // -1 free
    // diagonal-pair waves: the last wave slots of successive workgroups
    size_t di = 0;
    for (int k = 0; k < ndw; ++k) {
      const int wg = k % plan.nwg, w = 7 - k / plan.nwg;
      const int g = wg * 8 + w;
      plan.unit[g][0] = diag[di++];
      if (di < diag.size()) plan.unit[g][1] = diag[di++];
      slots[g] = 1;
    }
    size_t fi = 0;
    for (int g = 0; g < plan.nwg * 8 && fi < full.size(); ++g)
      if (slots[g] < 0) { plan.unit[g][0] = full[fi++]; slots[g] = 1; }
  }
  const int cus = h->num_cus > 0 ? h->num_cus : 256;
  int groups = std::max(8, (cus / plan.nwg) / 8 * 8);
  // chunks of whole stages; no more groups than there are stages
  const int64_t st1 = ceil_div(K1, SB_ROWS);
  groups = (int)std::min<int64_t>(groups, std::max<int64_t>(8, round_up(st1, 8)));
  const int64_t rows1 = round_up(ceil_div(K1, groups), SB_ROWS);
  const int64_t rows2 = K2 > 0 ? round_up(ceil_div(K2, groups), SB_ROWS) : 0;
  if (rows1 * ldx * 8 >= (1ll << 32) || rows2 * ldx2 * 8 >= (1ll << 32)) return PLDA_OK;   // 32-bit DMA offsets inside a chunk
  const int nt = (int)ceil_div(D, 16), ntri = nt * (nt + 1) / 2;
  PLDA_HIP(h, h->linalg_part.reserve((size_t)groups * ntri * 256 * 8));
  double *part = h->linalg_part.as<double>();
  // weights as arrays for both phases (ones when the rows are unweighted, w2 for the second matrix), each with room behind
  // its last row for the block kernel's over-read
  double *wts, *W2;
  PLDA_TRY(carve(h, h->syrk_wts, [&](Layout &c) { c.take(wts, K1 + 16).take(W2, K2 + 48); }));
  const double *W1 = kw;
  if (!kw) {
    fill_f64_kernel<<<(unsigned)ceil_div(K1, 256), 256, 0, h->stream>>>(wts, K1, 1.0);
    W1 = wts;
  }
  if (K2 > 0) fill_f64_kernel<<<(unsigned)ceil_div(K2, 256), 256, 0, h->stream>>>(W2, K2, w2);
  const size_t ldsb = ((size_t)2 * SB_ROWS * ceil_div(D, 128) * 128 + 64) * 8;
  static DeviceOnce attr;
  if (attr.needed(h->device)) {
    PLDA_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&syrk_blk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr.done(h->device);
  }
  const unsigned grid = (unsigned)(groups * plan.nwg);
  SyrkBlkArgs ga;
  ga.D = D;
  ga.K[0] = K1; ga.rows[0] = rows1; ga.ld[0] = ldx; ga.M[0] = X; ga.W[0] = W1;
  ga.K[1] = K2; ga.rows[1] = rows2; ga.ld[1] = K2 > 0 ? ldx2 : ldx; ga.M[1] = K2 > 0 ? X2 : X; ga.W[1] = K2 > 0 ? W2 : W1;
  ga.part = part;
  note_kernel(h, "syrk_blk_kernel");
  syrk_blk_kernel<<<grid, 512, ldsb, h->stream>>>(ga, plan, groups);
  syrk_tri_reduce_kernel<<<(unsigned)ntri, 1024, 0, h->stream>>>(part, groups, D, alpha, beta, C, ldc);
  PLDA_LAUNCH_CHECK(h);
  *used = true;
  return PLDA_OK;
}
