// Wave-lockstep emulation of the labelled fusion pass (plda_amd/csrc/fusion.hip) on the CPU, for tests/test_fusion_emulation.py:
// the kernel text itself (kernels.inc, cut out of fusion.hip by the test) compiled for the host, 256 host threads per block, every
// cross-lane operation (ballot, readlane, shuffles, the wave sum, the block barrier) through barriers.  It checks the LOGIC of the
// walk -- steps of U rows, partial steps, edges, the cooperative target sum, the block and grid reductions -- not the GPU's
// arithmetic: exp / log1p are the host's, the wave sum adds in lane order.  With Q sides it runs the SIDES = true instantiation
// on K + Q feature slots, the kernel-argument segment then being the whole FusionSideArgs.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <pthread.h>
#include <type_traits>
#include <vector>
#include "plda_hip.h"
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __shared__ static
#define __launch_bounds__(...)
struct Dim3 { unsigned x = 0, y = 0, z = 0; };
static thread_local Dim3 threadIdx, blockIdx;
static Dim3 gridDim;
static pthread_barrier_t g_block_bar, g_wave_bar[16];
static uint64_t g_slot[16][64];
static void *g_kernarg;
static inline int my_lane() { return threadIdx.x & 63; }
static inline int my_wave() { return threadIdx.x >> 6; }
static inline void __syncthreads() { pthread_barrier_wait(&g_block_bar); }
static inline uint64_t xchg(uint64_t v, int from) {          // every lane publishes v, then reads lane `from`
  const int w = my_wave();
  g_slot[w][my_lane()] = v;
  pthread_barrier_wait(&g_wave_bar[w]);
  const uint64_t r = g_slot[w][from];
  pthread_barrier_wait(&g_wave_bar[w]);
  return r;
}
static inline unsigned long long __builtin_amdgcn_ballot_w64(bool p) {
  const int w = my_wave();
  g_slot[w][my_lane()] = p ? 1 : 0;
  pthread_barrier_wait(&g_wave_bar[w]);
  unsigned long long m = 0;
  for (int l = 0; l < 64; ++l) m |= (unsigned long long)(g_slot[w][l] & 1) << l;
  pthread_barrier_wait(&g_wave_bar[w]);
  return m;
}
static inline int __builtin_amdgcn_readlane(int v, int l) { return (int)(uint32_t)xchg((uint32_t)v, l); }
static inline double readlane_f64(double x, int l) { uint64_t b; memcpy(&b, &x, 8); b = xchg(b, l); memcpy(&x, &b, 8); return x; }
template <typename T> static inline T __shfl_xor(T v, int o) { uint64_t b = 0; memcpy(&b, &v, sizeof(T)); b = xchg(b, my_lane() ^ o); memcpy(&v, &b, sizeof(T)); return v; }
static inline double wave_sum_f64(double x) {                // lane order; one exchange
  const int w = my_wave();
  memcpy(&g_slot[w][my_lane()], &x, 8);
  pthread_barrier_wait(&g_wave_bar[w]);
  double s = 0;
  for (int l = 0; l < 64; ++l) { double v; memcpy(&v, &g_slot[w][l], 8); s += v; }
  pthread_barrier_wait(&g_wave_bar[w]);
  return s;
}
static inline unsigned __float_as_uint(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static inline int __float_as_int(float f) { int u; memcpy(&u, &f, 4); return u; }
static inline float __int_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }
#define __builtin_amdgcn_kernarg_segment_ptr() g_kernarg
template <typename T> static inline T ceil_div(T a, T b) { return (a + b - 1) / b; }
namespace plda {
#include "kernels.inc"
}
using namespace plda;

struct Launch { void (*fn)(void *); void *ctx; unsigned tid, bid; };
static void *thread_main(void *p) { Launch *L = (Launch *)p; threadIdx.x = L->tid; blockIdx.x = L->bid; L->fn(L->ctx); return nullptr; }
static void run_grid(unsigned blocks, unsigned threads, void (*fn)(void *), void *ctx) {
  gridDim.x = blocks;
  pthread_barrier_init(&g_block_bar, nullptr, threads);
  for (unsigned w = 0; w < threads / 64; ++w) pthread_barrier_init(&g_wave_bar[w], nullptr, 64);
  std::vector<pthread_t> th(threads);
  std::vector<Launch> L(threads);
  for (unsigned b = 0; b < blocks; ++b) {
    for (unsigned t = 0; t < threads; ++t) { L[t] = {fn, ctx, t, b}; pthread_create(&th[t], nullptr, thread_main, &L[t]); }
    for (unsigned t = 0; t < threads; ++t) pthread_join(th[t], nullptr);
  }
}
struct Ctx { FusionSideArgs S; int64_t M, Nt; const int64_t *es, *ts; int64_t rpw; plda_fusion_record *part; int64_t nparts; int K; };
template <int K, bool SIDES> static void strip_fn(void *c) {
  Ctx *x = (Ctx *)c;
  if constexpr (SIDES) fusion_pass_strip_kernel<K, true>(x->S, x->M, x->Nt, x->es, x->ts, x->rpw, x->part);
  else fusion_pass_strip_kernel<K, false>(x->S.P, x->M, x->Nt, x->es, x->ts, x->rpw, x->part);
}
template <int K> static void (*strip_of(bool sides))(void *) { return sides ? strip_fn<K, true> : strip_fn<K, false>; }
static void reduce_fn(void *c) { Ctx *x = (Ctx *)c; fusion_reduce_kernel(x->part, x->nparts, x->K, x->part + x->nparts); }

// usage: emu K M Nt in.bin out.bin [Q] ; in.bin: K x (ld int64, off int64), Q x (op int64, off int64, test floats int64), a[K + Q],
// c, theta, es[M], ts[Nt], then per system (off + M * ld) floats, then per side M enrol floats and its test floats (the vector
// starts `off` floats into them; what follows its Nt values is padding that the kernel must not use)
int main(int argc, char **argv) {
  const int K = atoi(argv[1]), Q = argc > 6 ? atoi(argv[6]) : 0, T = K + Q;
  const int64_t M = atoll(argv[2]), Nt = atoll(argv[3]);
  if (K < 1 || Q < 0 || T > FUSION_KMAX) return 2;
  FILE *f = fopen(argv[4], "rb");
  Ctx x;
  memset(&x.S, 0, sizeof(x.S));
  FusionArgs &P = x.S.P;
  int64_t ld[8], off[8], op[8], toff[8], tlen[8];
  for (int k = 0; k < K; ++k) { fread(&ld[k], 8, 1, f); fread(&off[k], 8, 1, f); }
  for (int k = K; k < T; ++k) { fread(&op[k], 8, 1, f); fread(&toff[k], 8, 1, f); fread(&tlen[k], 8, 1, f); }
  fread(P.a, 8, T, f); fread(&P.c, 8, 1, f); fread(&P.theta, 8, 1, f);
  std::vector<int64_t> es(M), ts(Nt);
  fread(es.data(), 8, M, f); fread(ts.data(), 8, Nt, f);
  auto floats = [&](int64_t n) {
    float *b = (float *)aligned_alloc(64, (n * 4 + 63) / 64 * 64);
    fread(b, 4, n, f);
    return b;
  };
  for (int k = 0; k < K; ++k) { P.s[k] = floats(off[k] + M * ld[k]) + off[k]; P.ld[k] = ld[k]; }
  for (int k = K; k < T; ++k) {
    if (toff[k] + Nt > tlen[k]) return 2;
    x.S.enrol[k] = floats(M);
    P.s[k] = floats(tlen[k]) + toff[k]; P.ld[k] = 0;
    x.S.op[k] = (int32_t)op[k];
  }
  x.S.K = K;
  fclose(f);
  g_kernarg = &x.S;                          // the FusionArgs at offset 0, as in the kernel-argument segment
  const int64_t strips = ceil_div(Nt, (int64_t)FUSION_STRIP);
  const int64_t slices = std::max<int64_t>(1, std::min<int64_t>(M, FUSION_MAX_BLOCKS / strips));
  // the emulation creates 256 threads per block: keep the grid small (the library's rule with a cap of 8 slices)
  const int64_t sl = std::min<int64_t>(slices, 8);
  x.rpw = ceil_div(M, sl);
  const int64_t total = strips * ceil_div(M, x.rpw);
  std::vector<plda_fusion_record> part(total + 1);
  memset(part.data(), 0xff, part.size() * sizeof(plda_fusion_record));
  x.M = M; x.Nt = Nt; x.es = es.data(); x.ts = ts.data(); x.part = part.data(); x.nparts = total; x.K = T;
  void (*fn)(void *) = T == 1 ? strip_of<1>(Q) : T == 2 ? strip_of<2>(Q) : T == 3 ? strip_of<3>(Q) : T == 4 ? strip_of<4>(Q) : T == 5 ? strip_of<5>(Q) : T == 6 ? strip_of<6>(Q) : T == 7 ? strip_of<7>(Q) : strip_of<8>(Q);
  run_grid((unsigned)total, 256, fn, &x);
  run_grid(1, 1024, reduce_fn, &x);
  f = fopen(argv[5], "wb");
  fwrite(&part[total], sizeof(plda_fusion_record), 1, f);
  fclose(f);
  printf("blocks %lld\n", (long long)total);
  return 0;
}
