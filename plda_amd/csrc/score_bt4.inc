// plda_amd/csrc/score_bt4.inc -- K5, the 256 x 256 trials GEMM with ONE wave per SIMD (round 4).
// Included by score.hip inside namespace plda (same operand layout, fragment scheme, bias pairs and
// k order as trials_gemm_bt2_kernel: the scores are bit-identical).
//
// Replaces, like the kernels above, MPlda_score -> Plda::LogLikelihoodRatio
// (/root/reference/src/pldamodule.cpp:258-277) driven M x Nt times by scoring/scorePLDA.py:302-318.
//
// Why another shape.  trials_gemm_bt2_kernel keeps two 128 x 64 waves per SIMD; its timeline shows the
// loss at the tile boundary: both waves of a SIMD enter their 128-store epilogues one step apart, a
// store instruction waits 31-47 cycles for a gap in the partner's operand reads, and for ~3 900 cycles
// per tile neither wave feeds the matrix pipe (DESIGN.md section 3, findings 8 and 9).  Here a
// workgroup is 4 waves (2 x 2), one per SIMD, each owning 128 x 128 = 4 x 4 MFMA tiles: 256
// accumulator registers in the AGPR half of the 512-register file a lone wave has, fragments and
// addresses in the VGPR half.  A lone wave has ~15 free issue slots per 64-cycle MFMA, so the
// epilogue is spread over MFMA work of the SAME wave instead of competing with a partner:
//   * stages 0 .. nst-2 of a tile run k-major exactly like bt2 (step pairs on two fragment sets, the
//     early barrier in front of a stage's last step, that step carrying the DMA pieces of the stage
//     after next);
//   * the LAST stage runs its first step k-major while the fragments of its remaining FS-1 steps
//     are fetched into registers (96 VGPRs at FS = 4); then comes the stage barrier (nobody reads
//     the stage buffer any more) and the rest of the stage runs BLOCK-major: pairs of 32 x 32
//     accumulator blocks are finished one after the other (two interleaved chains of 4 (FS-1) MFMAs),
//     and the 32 dword stores of a finished pair go out between the MFMAs of the next pair --
//     straight from the accumulator registers (MUBUF stores read AGPRs), 2-3 per two MFMAs;
//   * the last pair's stores ride under the bias MFMAs of the next tile (which overwrite the other 14
//     blocks first);
//   * the matrix edge costs this kernel nothing: a tile that crosses it is written whole into a scratch slot (256 x 256) and
//     fringe_copy_kernel moves its inside part to the matrix behind the launch (C2: 781 of 152 881 tiles, 50 us).  Built
//     first and dropped: a bounds-checked store pass before the accumulators are reused, two instantiations of the
//     block-major part, per-slot branches between two store forms (each made the compiler copy accumulator blocks into
//     VGPRs or spill them on the main path); the row offset on the vector offset with the edge in num_records (one v_add
//     per store: 116 000 against 108 500 cycles per tile); the fringe on the 128 x 128 kernel (0.33 of 28.7 ms at C2).
// The tile boundary (what lies between the last MFMA of one tile and the first k-step MFMA of the next; figures for <4, 0>,
// D = 200, profiles/bt4_tile_boundary.txt): 109 245 -> 108 090 cycles per tile, 94.7 -> 95.7 % of them MFMA work.
//   * the next tile is the tile the DMA cursor stands in during this tile's last stage, so its place, existence and bias
//     slot are the cursor's own d_r0 / d_c0 / d_ok / d_slot: no three-slot queue beside it, no selects at the back edge;
//   * its output base, row stride, lane offset (tile_out) are computed between the first MFMA pairs of the block-major part
//     and its bias fragments are read three MFMA pairs before that part ends: the back edge carries finished values, the
//     first bias MFMA waits for no LDS round trip, and between the bias MFMAs and the first step only the stage loop's own set-up is left;
//   * ONE place stores the carried block pair (a workgroup without a further tile passes the bias block once more and
//     leaves behind it): with a second copy of the 32 stores on the exit path the compiler hoisted their operands to the
//     loop head, 32 v_accvgpr_read_b32 per tile that waited for the previous tile's last MFMAs.  One is left (a31 -> a VGPR
//     behind an s_nop 6; it stays whatever the order of the 32 stores and with the carried blocks defined before the loop);
//   * the cursor's advance at the end of the block-major part is straight-line (dma_advance_mid: d_st == 1 there);
//   * SGPRs: the queue table lives in front of the tile table (BT4_QHDR) instead of 16 argument SGPRs indexed by compare /
//     branch cascades, one bias descriptor chosen per wave instead of two, the table entry comes by a global load on the
//     table's pointer instead of a third descriptor, loop-carried flags are ints (a bool is a lane mask: two SGPRs, and
//     `pending ? -1 : 0` on one became a VGPR descriptor word, i.e. a waterfall loop around every carried store):
//     31 SGPRs spilled to VGPR lanes (45 v_readlane / 31 v_writelane, most inside the tile loop) -> none.
//   ISA of <4, 0>, parent -> now: 2 647 -> 2 084 instructions; v_accvgpr_read_b32 32 -> 1; v_readlane / v_writelane 45 / 31 ->
//   0 / 0; loop head up to the first bias MFMA 43 + 22 -> 16 instructions; ds_read + lgkmcnt(0) wait in front of the first bias
//   MFMA: the 4 + 1 are now in the block-major part / satisfied; last bias MFMA -> first k-step MFMA ~55 -> ~25; last
//   block-major MFMA -> loop head ~45 (3 taken branches) -> ~22 (2); v_mfma 608, ds_read_b128 80 as before; buffer_store_dword
//   288 -> 256 (the exit path's copy), LDS-DMA 70 -> 66 (one bias piece per site, the advance without one).
//   Measured and dropped (part B of the same work): skewing the four waves behind a regular stage's early barrier (wave w
//   waits w passes of an `s_nop 15` loop, ~30 cycles each) so that their 16 DMA pieces do not reach the address unit in
//   lockstep: 109 085 against 108 085 cycles per tile, 28.49 against 28.32 ms -- every regular stage longer by more than
//   the skew.  Not built: the stage's pieces spread over its last TWO steps (+32 VGPRs), odd stages without the x/y copy.
// Stage sizes: nst = ceil(nsteps / 4) balanced stages, the LARGER ones last, so that the block-major
// part is as long as possible (D = 200: 3,3,3,4,4,4,4 -> FS = 4: 12 288 cycles for the 1024 stores of a CU).
// Needs nst >= 3 (K >= 72); smaller depths stay on bt2.
// LDS: 2 x 64 KiB stage buffers + 3 x 4 KiB bias slots + a 64-byte mailbox = 140 KiB.
constexpr int BT4_BIAS = 2 * 65536;
constexpr int BT4_MBOX = BT4_BIAS + 3 * 4096;      // 4 ints: the tile the DMA cursor enters next (wave 0 -> all waves)
constexpr int BT4_LDS = BT4_MBOX + 64;             // 143424 B
struct Bt4Queues { int qbase[8]; int qlen[8]; };   // per XCD: first entry and length of its tile queue (score.hip: bt4_schedule)
// The kernel does not take Bt4Queues as an argument (16 argument SGPRs indexed through compare / branch cascades: 31 SGPRs
// spilled to VGPR lanes): the first BT4_QHDR entries of the tile table are the queue table, entry x = (first entry of
// queue x, already counted from the start of the table; its length), read with one scalar load where a queue is entered.
constexpr int BT4_QHDR = 8;
// The queue counters (cnt[0 .. 7], device scope).  The first BT4_OWN entries of a queue are the first tiles of its XCD's 32
// workgroups (taken by position, no round trip); counter value v therefore means entry BT4_OWN + v, and a launch starts from
// ZERO whatever the tile grid.  The launch leaves them at zero itself: every workgroup counts out on cnt[BT4_DONE] after its
// last atomic has returned, and the last one to leave clears the nine words -- rounds 4-5a reset them with a one-wave kernel in
// front of every launch (4.4 us of a 250 us call at 8192 x 8192 x 200).
constexpr unsigned BT4_OWN = 32;
constexpr int BT4_DONE = 16;
__device__ __forceinline__ void bt4_leave(unsigned *__restrict__ cnt) {
  if (threadIdx.x == 0) {       // (wave 0's lane 0 issued every atomic of this workgroup and has seen their results)
    const unsigned left = __hip_atomic_fetch_add(cnt + BT4_DONE, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (left == gridDim.x - 1) {
#pragma unroll
      for (int x = 0; x < 8; ++x) __hip_atomic_store(cnt + x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(cnt + BT4_DONE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

#define BT4_SB __builtin_amdgcn_sched_barrier(0)
#define BT4_MFMA(AF, BF, TM, TN) acc[TM][TN] = __builtin_amdgcn_mfma_f32_32x32x2f32(AF, BF, acc[TM][TN], 0, 0, 0);
#define BT4_MFMA2(T, S, TM, TN)                                                                     \
  BT4_MFMA(S##a[TM][T], S##b[TN][T], TM, TN) BT4_MFMA(S##a[TM][T], S##b[TN + 1][T], TM, TN + 1)
#define BT4_MFMA4(T, S, TM) BT4_MFMA2(T, S, TM, 0) BT4_MFMA2(T, S, TM, 2)
#define BT4_MFMA16(T, S) BT4_MFMA4(T, S, 0) BT4_MFMA4(T, S, 1) BT4_MFMA4(T, S, 2) BT4_MFMA4(T, S, 3)
#define BT4_LOAD(S, AP, BP)                                                                         \
  S##a[0] = (AP)[0]; S##a[1] = (AP)[32]; S##a[2] = (AP)[64]; S##a[3] = (AP)[96];                    \
  S##b[0] = (BP)[0]; S##b[1] = (BP)[32]; S##b[2] = (BP)[64]; S##b[3] = (BP)[96];
#define BT4_XYC(T)                                                                                  \
  xa[0][T] = ya[0][T]; xa[1][T] = ya[1][T]; xa[2][T] = ya[2][T]; xa[3][T] = ya[3][T];               \
  xb[0][T] = yb[0][T]; xb[1][T] = yb[1][T]; xb[2][T] = yb[2][T]; xb[3][T] = yb[3][T];
// a stage's first step when its step count is odd: computes on x, fetches into y, copies y -> x (a lone
// wave has the issue slots for the 32 moves)
#define BT4_STEP_ODD(AP, BP)                                                                        \
  BT4_MFMA16(0, x) BT4_SB; BT4_LOAD(y, AP, BP) BT4_SB;                                              \
  BT4_MFMA16(1, x) BT4_SB; BT4_XYC(0) BT4_SB; BT4_MFMA16(2, x) BT4_SB; BT4_XYC(1) BT4_SB;           \
  BT4_MFMA16(3, x) BT4_SB; BT4_XYC(2) BT4_XYC(3) BT4_SB;
#define BT4_STEP_FIRST(AP, BP)                                                                      \
  BT4_MFMA16(0, x) BT4_SB; BT4_LOAD(y, AP, BP) BT4_SB;                                              \
  BT4_MFMA16(1, x) BT4_MFMA16(2, x) BT4_MFMA16(3, x) BT4_SB;
#define BT4_STEP_SECOND(AP, BP)                                                                     \
  BT4_MFMA16(0, y) BT4_SB; BT4_LOAD(x, AP, BP) BT4_SB;                                              \
  BT4_MFMA16(1, y) BT4_MFMA16(2, y) BT4_MFMA16(3, y) BT4_SB;
// a (non-final) stage's last step: early barrier, the next stage's first fragments, the 16 DMA pieces of the stage after
// that, one per two MFMAs.  (Measured and dropped: staggering the four waves' pieces -- wave w behind MFMA 4 j + w -- through a
// uniform branch around each DMA instruction: 64 branches per step cost more than the queueing at the address unit they
// avoid, 114 600 against 108 500 cycles per tile at D = 200.  Branches around MFMAs, or any branch inside the block-major
// part below, make the compiler shuffle accumulator blocks through VGPRs: 300 to 1600 copy instructions, scratch spills.)
#define BT4_DSLOT(T, TM, TN, J) BT4_MFMA2(T, y, TM, TN) BT4_SB; dma_piece(J); BT4_SB;
#define BT4_STEP_LAST()                                                                             \
  stage_barrier();                                                                                  \
  BT4_SB; BT4_MFMA16(0, y) BT4_SB; BT4_LOAD(x, An, Bn) BT4_SB;                                      \
  BT4_DSLOT(1, 0, 0, 0) BT4_DSLOT(1, 0, 2, 1) BT4_DSLOT(1, 1, 0, 2) BT4_DSLOT(1, 1, 2, 3)           \
  BT4_DSLOT(1, 2, 0, 4) BT4_DSLOT(1, 2, 2, 5) BT4_DSLOT(1, 3, 0, 6) BT4_DSLOT(1, 3, 2, 7)           \
  BT4_DSLOT(2, 0, 0, 8) BT4_DSLOT(2, 0, 2, 9) BT4_DSLOT(2, 1, 0, 10) BT4_DSLOT(2, 1, 2, 11)         \
  BT4_DSLOT(2, 2, 0, 12) BT4_DSLOT(2, 2, 2, 13) BT4_DSLOT(2, 3, 0, 14) BT4_DSLOT(2, 3, 2, 15)       \
  BT4_MFMA4(3, y, 0) BT4_SB; dma_advance(); BT4_SB;                                                 \
  BT4_MFMA4(3, y, 1) BT4_MFMA4(3, y, 2) BT4_MFMA4(3, y, 3) BT4_SB;

// MODE bit 0: timeline instrumentation (diagnostic); bits 2 / 3: bounding arms (timing only, garbage scores):
// no operand DMA / no output stores.
template <int FS, int MODE>
__global__ __launch_bounds__(256, 1) void trials_gemm_bt4_kernel(
    const f32x4 *__restrict__ Apk, const f32x4 *__restrict__ Bpk, unsigned Mpad, unsigned Npad, int KQ,
    const float2 *__restrict__ rpair, const float2 *__restrict__ cpair, float *__restrict__ out, int64_t ld, int Mrows, int Ncols, float *__restrict__ fringe, const int2 *__restrict__ tab, unsigned *__restrict__ cnt,
    unsigned long long *__restrict__ dbg) {
  extern __shared__ __attribute__((aligned(16))) f32x4 smem[];
  static_assert(FS == 3 || FS == 4, "the last stage has 3 or 4 steps");
  constexpr bool TL = (MODE & 1) != 0;
  constexpr bool NODMA = (MODE & 4) != 0, NOSTORE = (MODE & 8) != 0;
  constexpr bool CLK = (MODE & 16) != 0;                          // the product kernel + clock stamps of workgroup 0 (see bt2)
  unsigned long long clk_c0 = 0, clk_r0 = 0;
  if (CLK && threadIdx.x == 0) { clk_c0 = __builtin_amdgcn_s_memtime(); clk_r0 = __builtin_amdgcn_s_memrealtime(); }
  constexpr int NSLOT = 4 * (FS - 1);                             // MFMA pairs of one block pair in the block-major part
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;                        // 2 x 2 waves, 128 x 128 each
  const int i = lane & 31, hh = lane >> 5;
  const int xcd = blockIdx.x & 7, lb = blockIdx.x >> 3;
  const int nsteps = KQ >> 1;                                     // 8-k steps per tile (>= 9 here)
  const int nst = (nsteps + 3) >> 2;                              // stages per tile (>= 3)
  const int sbase = nsteps / nst, srem = nsteps - sbase * nst;    // stage j has sbase + (j >= nst - srem) steps
  const int big0 = nst - srem;
  const int lane16 = lane * 16;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<f32x4 *>(Apk), 0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<f32x4 *>(Bpk), 0, -1, 0x00020000);
  LDS_AS char *const lds = (LDS_AS char *)smem;

  // ---- tile queue (score.hip: bt4_schedule).  A workgroup's first tile is entry `lb` of its XCD's queue; every further
  //      one is "the next entry": an atomic on the queue's counter, then the entry's load -- both asynchronous, driven by
  //      WAVE 0 from inside the stage barriers (never from the MFMA-interleaved code) and handed to the other waves through
  //      a 16-byte mailbox in LDS in front of the barrier of the stage in which the DMA cursor changes tiles.  A queue
  //      that has run dry sends the workgroup on to the next XCD's.
  volatile LDS_AS int *const mbox = (volatile LDS_AS int *)(lds + BT4_MBOX);
  int myq = xcd, q_tries = 0;                 // (wave 0) the queue being consumed and how many have been found dry
  int q_len_cur, q_base_cur;                  // the queue table's entry of myq (a uniform address: one scalar load)
  auto q_enter = [&](int q) { const int2 e = tab[q]; q_base_cur = __builtin_amdgcn_readfirstlane(e.x); q_len_cur = __builtin_amdgcn_readfirstlane(e.y); };
  q_enter(xcd);
  auto q_next = [&]() { myq = (myq + 1) & 7; ++q_tries; q_enter(myq); };
  auto take = [&]() -> int {                  // next slot of queue myq (uniform over the wave)
    unsigned sl = 0;
    if (lane == 0) sl = BT4_OWN + __hip_atomic_fetch_add(cnt + myq, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __builtin_amdgcn_readfirstlane((int)sl);
  };
  // synchronous form (prologue, and when a queue runs dry): the next tile of myq or of the queues after it; r0 = -1: none left
  auto fetch_sync = [&](int &fr0, int &fc0) {
    fr0 = fc0 = -1;
    while (q_tries < 8) {
      const int sl = take();
      if (sl < q_len_cur) {
        const int2 e = tab[q_base_cur + sl];
        fr0 = __builtin_amdgcn_readfirstlane(e.x); fc0 = __builtin_amdgcn_readfirstlane(e.y);
        return;
      }
      q_next();
    }
  };
  int nx_r0 = -1, nx_c0 = -1;                 // (all waves) the tile the DMA cursor enters at its next tile change
  // (wave 0) whether the queues may still hold tiles: the last tile published was a real one
  int more_tiles = 1;
  {
    if (wave == 0) {
      int a0 = -1, a1 = -1, b0 = -1, b1 = -1;
      if (lb < q_len_cur) { const int2 e = tab[q_base_cur + lb]; a0 = __builtin_amdgcn_readfirstlane(e.x); a1 = __builtin_amdgcn_readfirstlane(e.y); }
      else fetch_sync(a0, a1);
      if (a0 >= 0) fetch_sync(b0, b1);     // the second tile, in the mailbox from the start
      mbox[0] = a0; mbox[1] = a1; mbox[2] = b0; mbox[3] = b1;
      more_tiles = b0 >= 0 ? 1 : 0;
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0x0070);
    __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory");
  }
  const int t0_r0 = __builtin_amdgcn_readfirstlane(mbox[0]), t0_c0 = __builtin_amdgcn_readfirstlane(mbox[1]);
  if (t0_r0 < 0) { bt4_leave(cnt); return; }
  int d_ok = 1;                               // the cursor stands in a real tile (an int: a loop-carried bool lives in a lane mask)

  // ---- DMA cursor.  This wave moves rows [wave*64, +64) of the 8 k-quad planes of a stage, A side then B side:
  //      16 pieces of 1 KiB per stage ----
  const unsigned strideA1 = Mpad * 16u, strideB1 = Npad * 16u;    // bytes per k-quad plane
  const unsigned ldsw = (unsigned)wave * 1024u;
  int d_st = 0, d_slot = 0;
  int d_r0 = t0_r0, d_c0 = t0_c0;
  unsigned d_offA = ((unsigned)d_r0 + (unsigned)wave * 64u) * 16u;
  unsigned d_offB = ((unsigned)d_c0 + (unsigned)wave * 64u) * 16u;
  unsigned d_lds = 0;
  float *const bias_lds = reinterpret_cast<float *>(reinterpret_cast<char *>(smem) + BT4_BIAS);
  // a tile's bias pairs: 2 KiB per side, one piece from each wave (waves 0, 1 the row side, 2, 3 the column side): ONE
  // descriptor and one instruction per wave, chosen here
  const unsigned long long bias_src = reinterpret_cast<unsigned long long>(wave < 2 ? (const void *)rpair : (const void *)cpair);
  const __amdgpu_buffer_rsrc_t rsBias = __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<void *>(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(bias_src >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)bias_src)), 0, -1, 0x00020000);
  const int bias_w = (wave & 1) * 1024;

  auto dma_piece = [&](int jj) {
    if (NODMA) return;
    if (jj < 8)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (LDS_AS void *)(lds + d_lds + ldsw + jj * 4096u), 16, lane16,
                                               (int)(d_offA + (unsigned)jj * strideA1), 0, 0);
    else
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (LDS_AS void *)(lds + d_lds + 32768u + ldsw + (jj - 8) * 4096u), 16,
                                               lane16, (int)(d_offB + (unsigned)(jj - 8) * strideB1), 0, 0);
  };
  auto dma_advance = [&]() {
    if (d_st == 0 && d_ok && !NODMA) {
      // the tile's bias pairs: 2 KiB per side, one piece from each wave (MUBUF DMA, see bt2)
      float *dst = bias_lds + d_slot * 1024 + wave * 256;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsBias, (LDS_AS void *)dst, 16, lane16, (wave < 2 ? d_r0 : d_c0) * 8 + bias_w, 0, 0);
    }
    const unsigned npd = (unsigned)(sbase + (d_st >= big0 ? 1 : 0));
    d_offA += npd * 2u * strideA1;
    d_offB += npd * 2u * strideB1;
    d_lds ^= 65536u;
    if (++d_st == nst) {
      d_st = 0;
      d_slot = d_slot == 2 ? 0 : d_slot + 1;
      if (d_ok) d_ok = nx_r0 >= 0 ? 1 : 0;
      if (d_ok) { d_r0 = nx_r0; d_c0 = nx_c0; }
      d_offA = ((unsigned)d_r0 + (unsigned)wave * 64u) * 16u;
      d_offB = ((unsigned)d_c0 + (unsigned)wave * 64u) * 16u;
    }
  };

  // The advance at the end of the block-major part, straight-line.  Precondition: d_st == 1.  The cursor entered
  // (t + 1, stage 0) in the last step of stage nst - 2 of tile t (that step's dma_advance() took the tile change or came from
  // it with d_st == 0 and left d_st == 1; the prologue leaves the same state for the first tile), the block-major part has
  // just issued the pieces of (t + 1, stage 1), and nst >= 3 (the host requires it where use_bt4 is decided) keeps
  // stage 2 inside the same tile: no tile change, no bias DMA, nothing to decide.
  const unsigned np1 = (unsigned)(sbase + (1 >= big0 ? 1 : 0));   // steps of stage 1
  auto dma_advance_mid = [&]() {
    d_offA += np1 * 2u * strideA1;
    d_offB += np1 * 2u * strideB1;
    d_lds ^= 65536u;
    ++d_st;
  };

  int tseq = 0, st = 0;
  unsigned long long t_arr = 0;
  // timeline words of workgroup 0: [tile < 8][stage < 16][wave < 4][8]: 0 barrier arrival, 1 barrier leave,
  // 2..5 step starts; stage slot 15 words 6, 7: start and end of the block-major part
  // (the asm memory clobbers around every raw s_barrier of this file: llvm.amdgcn.s.barrier is IntrNoMem, so the optimiser may move
  //  plain LDS loads across it -- it did in syrk_blk.inc, a one-in-a-thousand wrong block, round 6.  Here the compiler had kept the
  //  last step's fragment reads in front of the barrier; with the clobbers it has to, and the code is the same but for three
  //  scalar instructions.)
  auto stage_barrier = [&]() {
    if (TL) t_arr = __builtin_amdgcn_s_memtime();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0x0070);   // vmcnt(0) lgkmcnt(0): this wave's DMAs of the next stage have landed
    __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory");
    // the DMA cursor changes tiles in the step behind this barrier when it stands in a tile's last stage: every wave takes
    // the tile to enter from the mailbox (wave 0 put it there at the end of the previous tile, see the tile loop)
    if (d_ok && d_st == nst - 1) { nx_r0 = __builtin_amdgcn_readfirstlane(mbox[2]); nx_c0 = __builtin_amdgcn_readfirstlane(mbox[3]); }
    if (TL) {
      const unsigned long long t_lv = __builtin_amdgcn_s_memtime();
      if (blockIdx.x == 0 && lane == 0 && tseq < 8 && st < 16) {
        unsigned long long *p = dbg + (((size_t)tseq * 16 + st) * 4 + wave) * 8;
        p[0] = t_arr; p[1] = t_lv;
      }
    }
  };
  auto step_stamp = [&](int sn) {
    if (TL) {
      const unsigned long long ts = __builtin_amdgcn_s_memtime();
      if (blockIdx.x == 0 && lane == 0 && tseq < 8 && st < 16) dbg[(((size_t)tseq * 16 + st) * 4 + wave) * 8 + 1 + sn] = ts;
    }
  };

  // ---- prologue: stage 0 of the first tile, barrier, then stage 1 in a burst ----
#pragma unroll
  for (int jj = 0; jj < 16; ++jj) dma_piece(jj);
  dma_advance();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0x0070);
  __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory");
#pragma unroll
  for (int jj = 0; jj < 16; ++jj) dma_piece(jj);
  dma_advance();

  int cur = 0;
  int have = 1;                             // (an int, like pending: a loop-carried bool lives in a lane mask)
  const f32x4 *const Abase = smem + hh * 256 + wm * 128 + i;
  const f32x4 *const Bbase = smem + 8 * 256 + hh * 256 + wn * 128 + i;
  f32x4 xa[4], xb[4], ya[4], yb[4];
  f32x4 fa[FS - 1][4], fb[FS - 1][4];
  f32x16 acc[4][4];
  BT4_LOAD(x, Abase, Bbase)
  // the bias fragments of a tile are read one tile ahead (in the block-major part of the tile before; the first tile's here,
  // behind the prologue's barrier, which covered the DMA of bias slot 0), so that the first bias MFMA of a tile waits for no
  // LDS round trip
  float ap[4], bp[4];
  auto bias_read = [&](int slot) {
    const float *const bl = bias_lds + slot * 1024;
#pragma unroll
    for (int tm = 0; tm < 4; ++tm) ap[tm] = bl[(wm * 128 + tm * 32 + i) * 2 + hh];
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) bp[tn] = bl[512 + (wn * 128 + tn * 32 + i) * 2 + hh];
  };
  bias_read(0);

  // ---- output addressing.  A register r = 4 q + e of a 32 x 32 accumulator block holds rows 8 q + e and 8 q + e + 4
  //      (lane >> 5) of 32 consecutive columns: one dword store = two full 128-byte row pieces.  The lane part of the
  //      address is constant over a tile, row and block column ride on the SCALAR offset (a vector add per store costs the
  //      lone wave ~8 cycles of MFMA issue each, 7 % of a tile at D = 200: measured), the base is per tile.
  //      The matrix edge: a tile that crosses it is written WHOLE into its slot of the `fringe` scratch (256 x 256, row
  //      stride 256) and copied out by fringe_copy_kernel behind this launch -- no bounds in this kernel's store path.
  const int tilesM = (Mrows + 255) >> 8, tilesN = (Ncols + 255) >> 8;
  const int edge_tm = (Mrows & 255) != 0 ? tilesM - 1 : -1, edge_tn = (Ncols & 255) != 0 ? tilesN - 1 : -1;   // the tile row / column that crosses the edge (-1: none)
  int pending = 0, p_lo = 0, p_hi = 0;      // (ints, not bools: they stay on the scalar unit)
  unsigned p_ldb = 0, p_voff = 0;
  auto make_rs = [&](int lo, int hi, int nr) {
    const unsigned long long a = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(hi) << 32) | (unsigned)__builtin_amdgcn_readfirstlane(lo);
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<float *>(a), 0, __builtin_amdgcn_readfirstlane(nr), 0x00020000);
  };
  int nostore_gate = 1;                     // (bounding arm: opaque, so that the accumulators stay live and the MFMAs are not dead code)
  if (NOSTORE) asm volatile("" : "+s"(nostore_gate));
  auto store_reg = [&](const __amdgpu_buffer_rsrc_t rs, unsigned vo, unsigned rowb, int tm, int tn, int r) {
    if (NOSTORE && nostore_gate) return;
    // (the block column rides on the instruction's immediate offset -- a constant added to the vector offset folds into
    //  it -- so that the two stores of a register pair share ONE scalar offset: every instruction of this wave costs an
    //  issue slot the matrix pipe waits for, and the second multiply-add per pair was 128 of them per tile)
    const unsigned so = (unsigned)(tm * 32 + 8 * (r >> 2) + (r & 3)) * rowb;
    const float v = acc[tm][tn][r];          // (a bit_cast of the element expression itself reads element 0)
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs, (int)(vo + (unsigned)tn * 128u), (int)so, 2 /* nt */);
  };
  // the k-th of the 32 stores of block pair p (blocks (p >> 1, 2 (p & 1)) and (p >> 1, 2 (p & 1) + 1))
  auto store_pair = [&](const __amdgpu_buffer_rsrc_t rs, unsigned vo, unsigned rowb, int p, int k) {
    store_reg(rs, vo, rowb, p >> 1, 2 * (p & 1) + (k & 1), k >> 1);
  };
  // a tile's output: its place in the matrix, or -- a tile that crosses the matrix edge -- slot `tile row` (last tile
  // column) / `tilesM + tile column` (last tile row) of the fringe scratch.  Scalar selects only: it runs for the NEXT tile
  // between the MFMAs of the block-major part (everything it reads exists since the cursor's tile change in stage nst - 3),
  // so that the back edge carries finished values and nothing stands between a tile's bias MFMAs and its first step.
  auto tile_out = [&](int tr0, int tc0, int &t_lo, int &t_hi, unsigned &t_ldb, unsigned &t_voff) {
    const int tmi = tr0 >> 8, tni = tc0 >> 8;
    const int e_col = tni == edge_tn ? 1 : 0, e_row = tmi == edge_tm ? 1 : 0;
    const int edge = e_col | e_row;
    const int fslot = e_col ? tmi : tilesM + tni;
    const unsigned long long a_f = reinterpret_cast<unsigned long long>(fringe) + 4ull * (unsigned long long)((int64_t)fslot * 65536 + (wm * 128) * 256 + wn * 128);
    const unsigned long long a_m = reinterpret_cast<unsigned long long>(out) + 4ull * (unsigned long long)(((int64_t)tr0 + wm * 128) * ld + tc0 + wn * 128);
    const unsigned long long o_addr = edge ? a_f : a_m;
    t_ldb = (unsigned)__builtin_amdgcn_readfirstlane((int)(edge ? 1024u : 4u * (unsigned)ld));   // bytes per output row (ld < 2^22)
    t_voff = (unsigned)hh * (4u * t_ldb) + (unsigned)i * 4u;
    t_lo = __builtin_amdgcn_readfirstlane((int)(unsigned)o_addr); t_hi = __builtin_amdgcn_readfirstlane((int)(unsigned)(o_addr >> 32));
  };
  int o_lo, o_hi;                           // this tile's output base, row stride in bytes and lane offset
  unsigned ldb, voff;
  tile_out(d_r0, d_c0, o_lo, o_hi, ldb, voff);
  for (;;) {
    // (opaque per tile: the row offsets are then one scalar multiply beside each store; left loop-invariant, the
    //  compiler hoists all 128 of them out of the tile loop and spills them to VGPR lanes)
    p_ldb = (unsigned)__builtin_amdgcn_readfirstlane((int)p_ldb);
    asm volatile("" : "+s"(p_ldb));
    ldb = (unsigned)__builtin_amdgcn_readfirstlane((int)ldb);
    asm volatile("" : "+s"(ldb));
    // (rebuilt per tile from scalars that went through readfirstlane: a loop-carried descriptor -- or one the compiler can
    //  prove equal to the previous tile's -- ends up in vector registers and every store in a waterfall loop)
    const __amdgpu_buffer_rsrc_t p_rs = make_rs(p_lo, p_hi, -pending);   // (num_records 0 on the first tile: nothing carried)
    const __amdgpu_buffer_rsrc_t rs = make_rs(o_lo, o_hi, -1);
    // ---- the tile queue, one fetch per tile, at three fixed places of the tile's code (all wave 0, none inside the
    //      MFMA-interleaved parts): here the atomic on the queue's counter; behind the last stage's barrier -- whose vmcnt(0)
    //      has seen the slot number arrive -- the load of that slot's table entry; at the end of the tile the entry goes into
    //      the mailbox, from where every wave takes it at the DMA cursor's tile change in the NEXT tile.  The two values live
    //      inside one loop iteration with a single definition each, so the compiler has no reason to copy them -- as loop-
    //      carried registers written under a state machine in the stage barriers they were copied right behind the issue, an
    //      s_waitcnt vmcnt(0) for a memory round trip in the middle of wave 0's MFMA stream (~1 500 cycles per tile).
    unsigned long long t_top0 = 0;
    if (TL) t_top0 = __builtin_amdgcn_s_memtime();
    const bool fetching = wave == 0 && more_tiles != 0;   // (more_tiles == 0 where !have: the tile published last was none)
    // (f_raw, f_ent: defined ONLY on the fetching path -- initialised on the other, the merge would be a copy of the
    //  value right behind its issue, i.e. a wait for the memory round trip.  score.hip is compiled with the atomic
    //  optimizer off: it rewrites this one-lane atomic into a wave reduction that reads the result back at once.)
    unsigned f_raw;
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    u32x2 f_ent;
    int f_sl = 0;
    if (fetching && lane == 0) f_raw = __hip_atomic_fetch_add(cnt + myq, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // accumulators start from the bias r'_i + s_i q_j: one rank-2 MFMA per block on the tile's bias pairs (srcC = 0).
    // The previous tile's last block pair (blocks 14, 15) is stored under the bias MFMAs of blocks 0 .. 13.
    // A workgroup that has no further tile (!have) takes this block once more for the carried stores and leaves behind it:
    // ONE place stores block pair 7.  (With a second copy of the 32 stores on the exit path the compiler hoisted their
    // common operands to the loop head: 32 v_accvgpr_read_b32 in front of every tile, waiting for the last MFMAs of the
    // tile before with nothing behind them in the pipe.)
    {
      const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (pending) {
#pragma unroll
        for (int b = 0; b < 14; ++b) {
          acc[b >> 2][b & 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[b >> 2], bp[b & 3], zero16, 0, 0, 0);
          BT4_SB;
          store_pair(p_rs, p_voff, p_ldb, 7, 2 * b);
          store_pair(p_rs, p_voff, p_ldb, 7, 2 * b + 1);
          BT4_SB;
        }
#pragma unroll
        for (int k = 28; k < 32; ++k) store_pair(p_rs, p_voff, p_ldb, 7, k);
        BT4_SB;
        acc[3][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[3], bp[2], zero16, 0, 0, 0);
        acc[3][3] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[3], bp[3], zero16, 0, 0, 0);
      } else {
#pragma unroll
        for (int b = 0; b < 16; ++b)
          acc[b >> 2][b & 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[b >> 2], bp[b & 3], zero16, 0, 0, 0);
      }
      BT4_SB;
    }
    if (!have) break;
    if (TL) {
      const unsigned long long t_top1 = __builtin_amdgcn_s_memtime();
      if (blockIdx.x == 0 && lane == 0 && tseq < 8) {
        unsigned long long *p = dbg + (((size_t)tseq * 16 + 15) * 4 + wave) * 8;
        p[2] = t_top0; p[3] = t_top1;      // the tile's top: entry, and behind the bias MFMAs with the carried stores
      }
    }
    // The next tile is the one the DMA cursor stands in during this tile's last stage: it entered it in stage nst - 3 of
    // this tile and leaves it in stage nst - 3 of the next (nst >= 3), so d_r0 / d_c0 / d_ok / d_slot ARE the next tile's
    // place, existence and bias slot there -- no queue of tile slots beside the cursor.
    int n_have = 0, n_lo = 0, n_hi = 0;
    unsigned n_ldb = 0, n_voff = 0;

    for (st = 0; st < nst - 1; ++st) {
      const int np = sbase + (st >= big0 ? 1 : 0);
      const f32x4 *Ac = Abase + cur * 4096, *Bc = Bbase + cur * 4096;
      const f32x4 *An = Abase + (cur ^ 1) * 4096, *Bn = Bbase + (cur ^ 1) * 4096;
      int sn = 0;                // step whose fragments are in x
      if (np & 1) {
        step_stamp(1);
        BT4_STEP_ODD(Ac + 512, Bc + 512)
        sn = 1;
      }
#pragma unroll 1
      for (; sn + 2 < np; sn += 2) {
        step_stamp(sn + 1);
        BT4_STEP_FIRST(Ac + (sn + 1) * 512, Bc + (sn + 1) * 512)
        BT4_STEP_SECOND(Ac + (sn + 2) * 512, Bc + (sn + 2) * 512)
      }
      step_stamp(sn + 1);
      BT4_STEP_FIRST(Ac + (sn + 1) * 512, Bc + (sn + 1) * 512)
      BT4_STEP_LAST()
      cur ^= 1;
    }

    // ---- last stage (FS steps; st == nst - 1).  Step 0 k-major on x while the fragments of steps 1 .. FS-1 are fetched ----
    {
      const f32x4 *Ac = Abase + cur * 4096, *Bc = Bbase + cur * 4096;
      const f32x4 *An = Abase + (cur ^ 1) * 4096, *Bn = Bbase + (cur ^ 1) * 4096;
      step_stamp(1);
      BT4_MFMA16(0, x) BT4_SB;
#pragma unroll
      for (int s = 0; s < FS - 1; ++s) {
        const f32x4 *const ap = Ac + (s + 1) * 512, *const bp = Bc + (s + 1) * 512;
        fa[s][0] = ap[0]; fa[s][1] = ap[32]; fa[s][2] = ap[64]; fa[s][3] = ap[96];
        fb[s][0] = bp[0]; fb[s][1] = bp[32]; fb[s][2] = bp[64]; fb[s][3] = bp[96];
      }
      BT4_SB;
      BT4_MFMA16(1, x) BT4_MFMA16(2, x) BT4_MFMA16(3, x) BT4_SB;
      // every wave holds the rest of the stage in registers: the stage buffer is free, the next tile's first stage has landed
      stage_barrier();
      if (fetching) {
        f_sl = __builtin_amdgcn_readfirstlane((int)(BT4_OWN + f_raw));
        // (a vector-memory load although the address is uniform: a scalar load's result would sit in lgkmcnt, where the next
        //  fragment wait of this wave -- lgkmcnt(0), scalar loads return out of order -- waits for the table's memory
        //  latency; a dry queue: entry 0 is read and dropped.  The index goes through a VGPR on purpose: a global load on the
        //  table's pointer, which the scalar unit holds anyway, instead of four more SGPRs for a buffer descriptor.)
        int f_idx = q_base_cur + (f_sl < q_len_cur ? f_sl : 0);
        asm volatile("" : "+v"(f_idx));
        f_ent = *reinterpret_cast<const u32x2 *>(tab + f_idx);
      }
      BT4_SB;
      BT4_LOAD(x, An, Bn)
      BT4_SB;
      unsigned long long t_b0 = 0;
      if (TL) t_b0 = __builtin_amdgcn_s_memtime();
      // block-major: block pair p = (tm, 2 tnp), (tm, 2 tnp + 1): two interleaved chains; the 32 stores of pair p - 1 and
      // two DMA pieces of the stage after next go out between its MFMAs (no branch in here: see BT4_STEP_LAST)
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        const int tm = p >> 1, tn0 = 2 * (p & 1);
#pragma unroll
        for (int s = 0; s < FS - 1; ++s)
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            acc[tm][tn0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s][tm][t], fb[s][tn0][t], acc[tm][tn0], 0, 0, 0);
            acc[tm][tn0 + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s][tm][t], fb[s][tn0 + 1][t], acc[tm][tn0 + 1], 0, 0, 0);
            BT4_SB;
            const int slot = s * 4 + t;
            if (p > 0) {
#pragma unroll
              for (int k = 32 * slot / NSLOT; k < 32 * (slot + 1) / NSLOT; ++k) store_pair(rs, voff, ldb, p - 1, k);
            }
            if (p == 0 && slot == 0) {          // (pair 0 carries no stores: its issue slots are free)
              // (the empty asm statements keep the arithmetic HERE: without them the optimiser moves its scalar part in
              //  front of the part's first MFMA pair and sinks the lane offset to the back edge)
              int n_r0 = d_r0, n_c0 = d_c0;
              asm volatile("" : "+s"(n_r0), "+s"(n_c0));
              n_have = d_ok;
              tile_out(n_r0, n_c0, n_lo, n_hi, n_ldb, n_voff);
              asm volatile("" : "+s"(n_lo), "+s"(n_hi), "+s"(n_ldb), "+v"(n_voff));
            }
            // the next tile's bias fragments: its slot is in LDS since this stage's barrier (the bias DMA went out with the
            // cursor's advance in the last step of stage nst - 2 and that barrier's vmcnt(0) covered it); it is written
            // again two tiles from here
            if (p == 7 && slot == NSLOT - 3) bias_read(d_slot);
            if (slot == 1) dma_piece(2 * p);
            if (slot == NSLOT / 2 + 1) dma_piece(2 * p + 1);
            if (p == 7 && slot == NSLOT - 1) { dma_advance_mid(); asm volatile("" : "+s"(d_offA), "+s"(d_offB), "+s"(d_lds), "+s"(d_st)); }
            BT4_SB;
          }
      }
      if (TL) {
        const unsigned long long t_b1 = __builtin_amdgcn_s_memtime();
        if (blockIdx.x == 0 && lane == 0 && tseq < 8) {
          unsigned long long *p = dbg + (((size_t)tseq * 16 + 15) * 4 + wave) * 8;
          p[6] = t_b0; p[7] = t_b1;
        }
      }
      cur ^= 1;
    }
    if (fetching) {
      int e0 = __builtin_amdgcn_readfirstlane((int)f_ent.x), e1 = __builtin_amdgcn_readfirstlane((int)f_ent.y);
      if (f_sl >= q_len_cur) { q_next(); fetch_sync(e0, e1); }             // queue dry: rare, synchronous
      mbox[2] = e0; mbox[3] = e1;
      more_tiles = e0 >= 0 ? 1 : 0;
    }
    pending = 1; p_lo = o_lo; p_hi = o_hi; p_ldb = ldb; p_voff = voff;
    o_lo = n_lo; o_hi = n_hi; ldb = n_ldb; voff = n_voff;
    ++tseq;
    have = n_have;
  }
  __builtin_amdgcn_s_waitcnt(0x0070);   // no DMA may land in LDS after the workgroup has gone (nor an atomic of the queue be in flight)
  bt4_leave(cnt);
  if (CLK && threadIdx.x == 0) {     // every workgroup: dbg[8 + 4 b ..] = start / end in shader cycles and in 100 MHz ticks
    const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    unsigned long long *p = dbg + 8 + 4 * (size_t)blockIdx.x;
    p[0] = c1 - clk_c0; p[1] = clk_r0; p[2] = r1; p[3] = (unsigned long long)tseq;
    if (blockIdx.x == 0) { dbg[0] = c1 - clk_c0; dbg[1] = r1 - clk_r0; dbg[2] = (unsigned long long)tseq; }
  }
}
#undef BT4_STEP_LAST
#undef BT4_DSLOT
#undef BT4_STEP_SECOND
#undef BT4_STEP_FIRST
#undef BT4_STEP_ODD
#undef BT4_XYC
#undef BT4_LOAD
#undef BT4_MFMA16
#undef BT4_MFMA4
#undef BT4_MFMA2
#undef BT4_MFMA
#undef BT4_SB

// The inside part of the tiles that cross the matrix edge, from their scratch slots to the matrix (see the kernel above):
// slot s < tilesM is tile (s, tilesN - 1), slot tilesM + t is tile (tilesM - 1, t).  One workgroup per 32 rows of a slot.
__global__ __launch_bounds__(256) void fringe_copy_kernel(const float *__restrict__ fringe, float *__restrict__ out, int64_t ld, int Mrows,
                                                          int Ncols, int tilesM, int tilesN, int rag_m, int rag_n) {
  const int slot = blockIdx.x >> 3, part = blockIdx.x & 7;
  int tm, tn;
  if (slot < tilesM) { tm = slot; tn = tilesN - 1; if (!rag_n) return; }
  else { tm = tilesM - 1; tn = slot - tilesM; if (!rag_m || (rag_n && tn == tilesN - 1)) return; }   // (the corner tile lives in the column's slot)
  if (tn >= tilesN) return;
  const float *src = fringe + (int64_t)slot * 65536;
  const int rows = min(256, Mrows - tm * 256), cols = min(256, Ncols - tn * 256);
  const int c = threadIdx.x;
  if (c >= cols) return;
  for (int r = part * 32; r < min(rows, part * 32 + 32); ++r)
    __builtin_nontemporal_store(src[r * 256 + c], out + ((int64_t)tm * 256 + r) * ld + (int64_t)tn * 256 + c);
}
