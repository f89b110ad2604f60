// plda_amd/csrc/score_bf16x3.inc -- OPT-IN arm of K5 (PLDA_SCORE_DTYPE=bf16x3): the fp32 contraction of the trials GEMM
// as three bf16 terms per operand and six bf16 MFMAs per 16 k.  Included by score.hip inside namespace plda.
//
// Replaces, like the fp32 kernels, MPlda_score -> Plda::LogLikelihoodRatio (/root/reference/src/pldamodule.cpp:258-277)
// driven M x Nt times by scoring/scorePLDA.py:302-318.  NOT the product default and never the headline number:
// north_star prescribes fp32 MFMA for the trials GEMM; this arm exists because that kernel sits at its ceiling (0.90-0.92
// of 157 TFLOP/s) and the only lever left on the BASELINE shapes is another roofline (round-4 review, next 9).
//
// Arithmetic.  Every packed fp32 operand value x (the SAME values the fp32 kernels contract: biases, z-norm map and
// count buckets are upstream of this file) is split as x = x0 + x1 + x2, x0 = bf16(x), x1 = bf16(x - x0),
// x2 = bf16(x - x0 - x1): 3 x 8 significand bits.  a b = a0 b0 + (a0 b1 + a1 b0) + (a1 b1 + a0 b2 + a2 b0) + O(2^-24 |a b|);
// the three dropped products are below one fp32 ulp of the term.  Products of bf16 pairs are exact in fp32 and
// v_mfma_f32_32x32x16_bf16 accumulates in fp32, so what is lost against the fp32 kernels is the ORDER of the additions
// and those three products.  Measured on MI355X against the exact fp64 contraction (tests/test_gpu_score_model.py, D = 200,
// 255 x 257, scores up to |100 - 190|): max |delta| 2.3e-5 .. 9.8e-5 (the fp32 kernel's: 2.6e-5 .. 1.0e-4), RMS error
// 0.85 - 0.87 x the fp32 kernel's -- the arm is no less accurate than fp32, and stays within its split-model bound
// (three dropped products + fp32 accumulation) by a factor of 300 or more.  tests/test_gpu_bf16x3.py holds it to the same
// 1e-4 tolerance against the fp64 oracle as the fp32 kernels.
//
// Cost.  Per 16 k and 32 x 32 block: 6 MFMAs x 32 cycles = 192 cycles against 8 x 64 = 512 of v_mfma_f32_32x32x2_f32:
// C2's 1e10 trials are 9.8 ms of matrix pipe at 100 %, beside 40 GB of scores = 5 ms of HBM at 8 TB/s -- the arm's
// roofline is the HBM WRITE of the scores, which is what bench.py prices it against (extra key, never `roofline`).
//
// Shape.  Persistent, one workgroup of 8 waves per CU = two GROUPS of four (one wave per SIMD each), each group with its own
// stream of 256 x 128 tiles (wave tile 128 x 64 = 4 x 2 blocks, 128 accumulators) and its own two stage buffers, run in
// PING-PONG: see the kernel.  Built and measured before it (C2, 100k x 100k, D = 200): one 8-wave workgroup on a 256 x 256
// tile, all waves in step, two stage buffers 24.3 ms, three 23.3, with scalar addressing 21.0; two independent 4-wave
// workgroups per CU 22.0 -- they start together, do identical work and stay in phase; bounding arms of both forms: 13.2-13.4
// ms without DMA and stores, +3.6 with the DMA, +3.5-4.4 with the stores, nothing overlapping.  Also measured on the ping-pong
// form and dropped: the stage requests moved into the C phase, two steps ahead (22.3 ms, MFMA-busy 0.56: a wave's DMA issue
// -- M0 set-up, address arithmetic -- stalls its own MFMA stream; in the M phase it is the other group's MFMAs that run);
// the same requests spread one per five MFMAs over the C phase (23.2 ms, 0.515: the no-DMA arm of that form 18.1 -- a
// `buffer_load ... lds` between bf16 MFMAs costs far more than the one 32-cycle slot it costs beside a multiplying partner).
// Operand layout "k-oct packed x 3": plane (ko, s) = P[(3 ko + s)][row][8 bf16] -- 16-byte items like the fp32 k-quad planes,
// so a wave's DMA piece is again 64 rows = 1 KiB contiguous, landing lane-linear, and lane (i, h) reads the item of row i in
// k-oct 2 p + h as one ds_read_b128 = its A / B fragment of MFMA step p.  A stage is ONE 16-k step of both sides (6 planes x
// (256 + 128) rows x 16 B = 36 KiB); the DMA cursor runs one step ahead and crosses tile boundaries.  Plain dword stores from
// the accumulator layout (two 128-byte row pieces per instruction), the matrix edge by the descriptor's size: no fringe scratch.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
constexpr unsigned B3_STAGE_BYTES = 36864;           // one 16-k step: 6 planes x (256 A rows + 128 B rows) x 16 B
constexpr int B3_LDS = 4 * B3_STAGE_BYTES;           // 147 456 B: two groups x two stages
constexpr int B3_PR = 4, B3_PC = 16;                 // patch of 256 x 128 tiles an XCD's 64 workgroups share (1024 x 2048 trials)

__device__ __forceinline__ unsigned bf16_rn_bits(float x) {      // round to nearest even (finite inputs)
  const unsigned u = __float_as_uint(x);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// fp32 k-quad planes [KQ][Rpad] -> bf16 x 3 k-oct planes [3 KO][Rpad]  (KO even; k-octs beyond KQ / 2 are zero)
__global__ __launch_bounds__(256) void split_bf16x3_kernel(const f32x4 *__restrict__ P32, int64_t Rpad, int KQ, f32x4 *__restrict__ P16) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int ko = blockIdx.y;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  const f32x4 lo = 2 * ko < KQ ? P32[(int64_t)(2 * ko) * Rpad + row] : z;
  const f32x4 hi = 2 * ko + 1 < KQ ? P32[(int64_t)(2 * ko + 1) * Rpad + row] : z;
  const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  unsigned w[3][4];
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    unsigned h[3][2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const float v = x[j + e];
      const unsigned u0 = bf16_rn_bits(v);
      const float r1 = v - __uint_as_float(u0 << 16);
      const unsigned u1 = bf16_rn_bits(r1);
      const float r2 = r1 - __uint_as_float(u1 << 16);
      h[0][e] = u0; h[1][e] = u1; h[2][e] = bf16_rn_bits(r2);
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) w[s][j >> 1] = h[s][0] | (h[s][1] << 16);
  }
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    f32x4 o;
    o.x = __uint_as_float(w[s][0]); o.y = __uint_as_float(w[s][1]); o.z = __uint_as_float(w[s][2]); o.w = __uint_as_float(w[s][3]);
    P16[(int64_t)(3 * ko + s) * Rpad + row] = o;
  }
}

// (Addressing: operands and scores go through buffer descriptors with the tile / plane / row parts on the SCALAR offset --
//  the first version computed 64-bit addresses per DMA piece and per store, with a bounds branch around every store: 2 000
//  instructions of epilogue per tile and wave.  Needs packed operands < 4 GiB and ld < 2^22, like the fp32 256 x 256
//  kernels: the host splits larger problems.)
// MODE bits 2 / 3: bounding arms (timing only, garbage scores): no operand DMA / no output stores (PLDA_GEMM_VARIANT=54 / 58 / 62)
template <int MODE>
__global__ __launch_bounds__(512, 1) void trials_gemm_bf16x3_kernel(
    const f32x4 *__restrict__ A16, const f32x4 *__restrict__ B16, unsigned Mpad, unsigned Npad, int nsteps,
    const float *__restrict__ rbias, const float *__restrict__ rscale, const float *__restrict__ cbias,
    float *__restrict__ out, int64_t ld, int64_t M, int64_t Nt, int btM, int btN, int pM, int pN, int colwalk,
    unsigned long long *__restrict__ dbg) {
  extern __shared__ __attribute__((aligned(16))) f32x4 smem3[];
  // MODE bit 4: the product kernel + workgroup 0's shader-clock / 100 MHz stamps (PLDA_GEMM_VARIANT=63: which clock the part holds under this load)
  unsigned long long clk_c0 = 0, clk_r0 = 0;
  if ((MODE & 16) && threadIdx.x == 0) { clk_c0 = __builtin_amdgcn_s_memtime(); clk_r0 = __builtin_amdgcn_s_memrealtime(); }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int grp = wave >> 2, gw = wave & 3;                 // group (its own tile stream, its own stage buffers), wave of the group
  const int wm = gw >> 1, wn = gw & 1;                      // 2 x 2 waves, 128 x 64 each: tile 256 x 128
  const int i = lane & 31, hh = lane >> 5;
  const int xcd = blockIdx.x & 7, lb = (blockIdx.x >> 3) * 2 + grp;   // this group takes tile `lb` (of B3_PR x B3_PC) of every patch its XCD walks
  const int lbm = lb / B3_PC, lbn = lb % B3_PC;
  const int lane16 = lane * 16;
  LDS_AS char *const lds = (LDS_AS char *)smem3 + (unsigned)grp * (2u * B3_STAGE_BYTES);
  const f32x4 *const ldsf = smem3 + grp * (2 * B3_STAGE_BYTES / 16);
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<f32x4 *>(A16), 0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<f32x4 *>(B16), 0, -1, 0x00020000);
  const unsigned strideA = Mpad * 16u, strideB = Npad * 16u;     // bytes per plane
  // DMA pieces of a stage (1 KiB = 64 rows of a plane): A 6 planes x 4 chunks -- wave w of the group moves chunk w of every
  // plane -- B 6 planes x 2 chunks -- wave w moves pieces 3 w .. 3 w + 2 (plane = piece >> 1, chunk = piece & 1)
  const unsigned bq0 = 3u * (unsigned)gw;

  const int npatch = bt4_queue_patches<int>(xcd, pM, pN, colwalk);   // patches this XCD walks (score.hip: row or column order)
  // the next iteration >= it whose tile exists; false: none left
  auto find_tile = [&](int &it, int &r0, int &c0) -> bool {
    for (;; ++it) {
      if (it >= npatch) return false;
      int pm, pn;
      bt4_patch<int>(xcd, it, pM, pN, colwalk, pm, pn);
      const int tm = pm * B3_PR + lbm, tn = pn * B3_PC + lbn;
      if (tm < btM && tn < btN) { r0 = tm * 256; c0 = tn * 128; return true; }
    }
  };
  auto issue = [&](int r0, int c0, int st, int b) {
    if (MODE & 4) return;
    const unsigned l0 = (unsigned)b * B3_STAGE_BYTES;
    const unsigned offA = ((unsigned)r0 + (unsigned)gw * 64u) * 16u + (unsigned)(6 * st) * strideA;
#pragma unroll
    for (int j = 0; j < 6; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (LDS_AS void *)(lds + l0 + j * 4096u + (unsigned)gw * 1024u), 16, lane16, (int)(offA + (unsigned)j * strideA), 0, 0);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const unsigned q = bq0 + j, plane = q >> 1, chunk = q & 1u;
      const unsigned offB = ((unsigned)c0 + chunk * 64u) * 16u + ((unsigned)(6 * st) + plane) * strideB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (LDS_AS void *)(lds + l0 + 24576u + plane * 2048u + chunk * 1024u), 16, lane16, (int)offB, 0, 0);
    }
  };
  auto make_rs = [&](const void *p, unsigned nr) {
    const unsigned long long a = reinterpret_cast<unsigned long long>(p);
    const unsigned long long u = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)a);
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<float *>(u), 0, (int)__builtin_amdgcn_readfirstlane((int)nr), 0x00020000);
  };
  auto sync = [&]() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0x0070);      // vmcnt(0) lgkmcnt(0): this wave's DMA pieces, stores and fragment reads are done
    __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory");
  };

  // ---- PING-PONG.  Every step of a group is two phases separated by workgroup barriers: an M phase (DMA issue of the next
  //      step, at a tile's first step the previous tile's stores and the new bias, then this step's 18 fragment reads) and a
  //      C phase (the step's 48 MFMAs).  Group 1 runs one barrier behind group 0, so on every SIMD exactly one of its two waves
  //      is in its C phase: the matrix pipe sees one uninterrupted MFMA stream, the memory work of the other wave costs
  //      it nothing.  Both groups make the same number of barrier pairs (a group with fewer tiles idles through the rest).
  int ntiles = 0;
  { int t = 0, a, b; while (find_tile(t, a, b)) { ++ntiles; ++t; } }
  int other = 0;
  {
    const int lbo = (blockIdx.x >> 3) * 2 + (grp ^ 1), om = lbo / B3_PC, on = lbo % B3_PC;
    for (int t = 0; t < npatch; ++t) {
      int pm, pn;
      bt4_patch<int>(xcd, t, pM, pN, colwalk, pm, pn);
      if (pm * B3_PR + om < btM && pn * B3_PC + on < btN) ++other;
    }
  }
  const int pairs = max(ntiles, other) * nsteps;            // barrier pairs every wave of the workgroup makes
  int it = 0, r0 = 0, c0 = 0;
  bool have = find_tile(it, r0, c0);
  if (have) issue(r0, c0, 0, 0);
  if (grp == 1) sync();
  int cur = 0, st = 0;
  unsigned p_ldb = 0, p_vo[2] = {0x80000000u, 0x80000000u}, p_nr = 0;
  const float *p_base = out;
  f32x16 acc[4][2];
  bf16x8 a[3][4], b[3][2];
  auto store_tile = [&]() {
    if (MODE & 8) {
#pragma unroll
      for (int tm = 0; tm < 4; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
          for (int r = 0; r < 16; ++r) asm volatile("" ::"v"(acc[tm][tn][r]));
      return;
    }
    const __amdgpu_buffer_rsrc_t rs = make_rs(p_base, p_nr);
    const unsigned ldb = (unsigned)__builtin_amdgcn_readfirstlane((int)p_ldb);
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const unsigned so = (unsigned)(wm * 128 + tm * 32 + (r & 3) + 8 * (r >> 2)) * ldb;
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
          const float v = acc[tm][tn][r];
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs, (int)p_vo[tn], (int)so, 2 /* nt */);
        }
      }
  };
  bool drained = false;                                     // this wave waited for its DMA before its last stores (no wait at the next (A))
  for (int pr = 0; pr < pairs; ++pr) {
    // (A) my M phase begins, the other group's C phase.  This step's stage has landed: vmcnt(0) -- except right behind a
    // tile's stores, which were issued BEHIND a wait for the DMA (below): waiting here would wait for their write
    // acknowledgements, 5-10 k cycles under this kernel's HBM load, with the other group's MFMAs held at its barrier
    if (!drained) __builtin_amdgcn_s_waitcnt(0x0070);
    drained = false;
    asm volatile("" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory");
    if (have) {
      // the stage after this one: the tile's next step, or the next tile's first
      int nit = it, nr0 = r0, nc0 = c0;
      bool nhave = true;
      if (st + 1 == nsteps) { nit = it + 1; nhave = find_tile(nit, nr0, nc0); }
      if (nhave) issue(nr0, nc0, st + 1 == nsteps ? 0 : st + 1, cur ^ 1);
      if (st == 0) {
        // a tile begins: the accumulators start from the bias fma(s_i, q_j, r'_i) -- the same starting value as the fp32 kernels
        const int64_t wrow0 = (int64_t)r0 + wm * 128, wcol0 = (int64_t)c0 + wn * 64;
        float cb[2];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) cb[tn] = cbias[wcol0 + tn * 32 + i];
#pragma unroll
        for (int tm = 0; tm < 4; ++tm)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 rb = *reinterpret_cast<const f32x4 *>(rbias + wrow0 + tm * 32 + 8 * q + 4 * hh);
            const f32x4 rs = *reinterpret_cast<const f32x4 *>(rscale + wrow0 + tm * 32 + 8 * q + 4 * hh);
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
              for (int e = 0; e < 4; ++e) acc[tm][tn][4 * q + e] = __builtin_fmaf(rs[e], cb[tn], rb[e]);
          }
        // where this tile's scores will go: one descriptor per tile whose size ends behind the last valid element (rows >= M
        // fall outside it); lanes of columns >= Nt get an offset outside it; row and block parts ride on the scalar offset
        const int rows_ok = (int)min((int64_t)256, M - r0), cols_ok = (int)min((int64_t)128, Nt - c0);
        p_ldb = 4u * (unsigned)ld;
        p_base = out + ((int64_t)r0 * ld + c0);
        p_nr = (unsigned)(rows_ok - 1) * p_ldb + (unsigned)cols_ok * 4u;
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
          const int col = wn * 64 + tn * 32 + i;
          p_vo[tn] = col < cols_ok ? (unsigned)hh * 4u * p_ldb + (unsigned)col * 4u : 0x80000000u;
        }
      }
      const f32x4 *As = ldsf + cur * (B3_STAGE_BYTES / 16) + (hh * 3) * 256 + wm * 128 + i;
      const f32x4 *Bs = ldsf + cur * (B3_STAGE_BYTES / 16) + 1536 + (hh * 3) * 128 + wn * 64 + i;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
#pragma unroll
        for (int tm = 0; tm < 4; ++tm) a[s][tm] = __builtin_bit_cast(bf16x8, As[s * 256 + tm * 32]);
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) b[s][tn] = __builtin_bit_cast(bf16x8, Bs[s * 128 + tn * 32]);
      }
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_waitcnt(0xc07f);                   // lgkmcnt(0) only: the fragments are in registers -- their LDS latency belongs to this
      __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory");                         // M phase, the DMA just issued stays in flight.  (B) my C phase begins, the other group's M phase
      // smallest terms first; eight independent chains per term keep the pipe full
#define B3_TERM(SA, SB)                                                                                              \
  _Pragma("unroll") for (int tm = 0; tm < 4; ++tm) _Pragma("unroll") for (int tn = 0; tn < 2; ++tn)                  \
      acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[SA][tm], b[SB][tn], acc[tm][tn], 0, 0, 0);
      B3_TERM(0, 2) B3_TERM(2, 0) B3_TERM(1, 1) B3_TERM(0, 1) B3_TERM(1, 0) B3_TERM(0, 0)
#undef B3_TERM
      cur ^= 1;
      if (++st == nsteps) {
        // the tile is done: its scores leave at the end of this C phase, behind a wait for the DMA in flight (the next step's
        // stage), so that the next (A) need not wait for anything
        __builtin_amdgcn_s_waitcnt(0x0070);
        store_tile();
        drained = true;
        st = 0; it = nit; r0 = nr0; c0 = nc0; have = nhave;
      }
    } else {
      asm volatile("" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory");
    }
  }
  if (grp == 0) sync();
  __builtin_amdgcn_s_waitcnt(0x0070);
  if ((MODE & 16) && threadIdx.x == 0 && blockIdx.x == 0) {
    dbg[0] = __builtin_amdgcn_s_memtime() - clk_c0; dbg[1] = __builtin_amdgcn_s_memrealtime() - clk_r0; dbg[2] = (unsigned long long)ntiles;
  }
}
