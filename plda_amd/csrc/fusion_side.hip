// plda_amd/csrc/fusion_side.hip -- quality-aware calibration (K25): the fusion pass and map over K score matrices and Q SIDES
// (include/plda_hip.h, "quality-aware calibration").  A side is one fp32 operation on a per-enrol-row and a per-test-column
// number (duration, embedding norm, cohort mean ...); its [M, Nt] values never exist in memory -- the kernels here form them
// in registers and hand the assembled fp32 feature array (s_0 .. s_{K-1}, q_0 .. q_{Q-1}) to the SAME fusion_account and
// fusion_block_store as fusion.hip's matrix kernel (the shared part of fusion.hip, included below), on the same grid and in
// the same visiting order.  A side pass is therefore bit-identical to a matrix pass over K + Q matrices in which the sides
// have been materialised, and the Newton fit, the record and the refusals of fusion.hip are used as they are (its host
// drivers launch these kernels).
//
// Kernels, instantiated on T = K + Q = 1 .. 8 with K wave-uniform at run time (one uniform branch per unrolled feature slot,
// so every accumulator and value index stays a compile-time constant; 8 instantiations instead of 36 on (K, Q)):
//   fusion_side_pass_strip_kernel<T>  fusion_pass_strip_kernel's walk, line for line.  A side is A MATRIX OF PITCH 0: slot
//       k >= K carries the side's test vector in P.s[k] with P.ld[k] = 0, so the address, the per-slot choice between 16-byte
//       and scalar loads and the column bounds are the matrix kernel's own code; the four test values are RE-READ per row
//       from the L2-resident vector (a plain load, where a matrix streams with a non-temporal one), enrol[row] is one scalar
//       load (wave-uniform address, constant address space), and the op is a wave-uniform select over the five fp32
//       results: about 12 fp32 VALU instructions per side per trial (the five results, four selects, the column bound) beside
//       the account's 221+ fp64 ones -- MEASURED, they are not free: 20 000 x 20 000 at 2.39 GHz, (K, Q) = (1, 3) 5.80 ms
//       against 4.86 ms for the matrix pass on materialised sides, (1, 7) 10.35 against 8.27 ms (profiles/fusion_side_*.json),
//       the pass being bound by VALU issue.  A wave-uniform BRANCH on the op (one body of 1 - 2 instructions per value)
//       was tried and not kept: at T = 8 it spills two scalar registers (245 VGPRs); it is the next step, for T <= 7 or with
//       the scalar pressure of the T = 8 walk reduced first.  Holding the 4 Q test values
//       in registers across the walk instead was not built: the matrix kernel already sits at 244 of 256 VGPRs at T = 8 and
//       130 .. 214 in between, so the persistent floats fit only the smallest T, and the pass is bound by fp64 VALU issue,
//       not by these loads (has the measurement).  One form for every (K, Q), no spill anywhere.
//       Elements beyond the last column get 0.f, as the matrix kernel's loads give them: they count for nothing, but a NaN
//       from enrol[row] in such a lane would otherwise reach the accumulators through 0 * NaN.
//   fusion_side_map_kernel<T>         fusion_map_kernel's walk; here the 4 test values of every side ARE held in registers
//       (4 T floats; the kernel has room), so a trial costs the K matrix reads, one scalar load per side per row and the
//       store: 4 K + 4 bytes instead of 4 (K + Q) + 4.
// The operand form (system 0 produced slab by slab, fusion.hip's fusion_pass) launches the same pass kernel per slab with the
// enrol vectors offset to the slab's first row.
//
// Resources on gfx950 (hipcc -Rpass-analysis=kernel-resource-usage with this file's flags, plda_amd/build.py -- the flags of
// fusion.hip, without machine LICM for the reason told there; VGPRs per lane, no AGPRs; scratch 0, SGPR and VGPR spills 0 in
// every instantiation):
//     T                  1     2     3     4     5     6     7     8
//     side pass         94   122   130   156   162   188   214   244     waves per SIMD 5 4 3 3 3 2 2 2
//     side map          20    26    34    42    50    58    66    74
// The side pass reports the matrix pass's figures exactly (fusion.hip's table): the side branch lives in the load stage, where
// the account's registers are not yet live.  The map (fusion.hip's: 16 .. 44) pays 4 T registers for the held test values;
// it re-reads bases, pitches, weights and ops from the kernel-argument segment per row -- held in scalar registers they
// spilled from T = 6 on (14 / 30 / 46 SGPRs).
#define PLDA_FUSION_SHARED_ONLY 1   // the shared device code of fusion.hip, without its kernels and host drivers
#include "fusion.hip"

namespace plda {

typedef const FusionSideArgs __attribute__((address_space(4))) *FusionSideArgsPtr;   // the struct where the kernel arguments live
typedef const float __attribute__((address_space(4))) *SideEnrolPtr;                 // read-only for the kernel's life: scalar loads

// the value of a side for (e = enrol[i], t = test[j]): ONE IEEE fp32 operation, ties and signed zeros by the written comparison
__device__ __forceinline__ float fusion_side_value(int op, float e, float t) {
  const float mn = e < t ? e : t, mx = e > t ? e : t, sm = e + t, ad = fabsf(e - t), pr = e * t;
  return op == PLDA_SIDE_MIN ? mn : op == PLDA_SIDE_MAX ? mx : op == PLDA_SIDE_SUM ? sm : op == PLDA_SIDE_ABSDIFF ? ad : pr;
}

// The labelled pass over K matrices and T - K sides: block b writes part[b].  fusion_pass_strip_kernel with the side branch
// in its load stage and nothing else changed; S (whose first member is the FusionArgs) is the FIRST kernel parameter, for the
// re-read at offset 0 of the kernel-argument segment that the matrix kernel explains.
template <int T>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void fusion_side_pass_strip_kernel(const FusionSideArgs S, int64_t M, int64_t Nt, const int64_t *__restrict__ espk,
                                   const int64_t *__restrict__ tspk, int64_t rows_per_wg, plda_fusion_record *__restrict__ part) {
  constexpr int U = fusion_rows_in_flight<T>();
  const int64_t strips = (Nt + FUSION_STRIP - 1) / FUSION_STRIP;
  const int64_t strip = blockIdx.x % strips, slice = blockIdx.x / strips;
  const int64_t col = strip * FUSION_STRIP + (int64_t)threadIdx.x * 4;
  const int64_t r0 = slice * rows_per_wg, r1 = (r0 + rows_per_wg < M) ? r0 + rows_per_wg : M;
  int64_t ts[4];
  bool ok[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    ok[e] = col + e < Nt;
    ts[e] = ok[e] ? tspk[col + e] : 0;
  }
  unsigned vec = 0;                          // bit k: slot k takes 16-byte loads (a side's pitch 0 passes the pitch test)
#pragma unroll
  for (int k = 0; k < T; ++k) vec |= (((S.P.ld[k] & 3) == 0) && ((reinterpret_cast<uintptr_t>(S.P.s[k]) & 15) == 0) && ok[3]) ? 1u << k : 0u;
  FusionAcc<T> A;
  for (int64_t row = r0; row < r1; row += U) {
    float v[U][T][4];
    FusionSideArgsPtr pp = (FusionSideArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    int64_t colv = col;
    asm volatile("" : "+s"(pp), "+v"(vec), "+v"(colv));
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (row + u >= r1) break;
#pragma unroll
      for (int k = 0; k < T; ++k) {
        const float *src = const_cast<const float *>(pp->P.s[k]) + (row + u) * pp->P.ld[k] + col;
        const bool side = k > 0 && k >= pp->K;               // wave-uniform; slot 0 is always a matrix
        if (vec >> k & 1u) {
          const f32x4f x = side ? *reinterpret_cast<const f32x4f *>(src) : __builtin_nontemporal_load(reinterpret_cast<const f32x4f *>(src));
          v[u][k][0] = x.x; v[u][k][1] = x.y; v[u][k][2] = x.z; v[u][k][3] = x.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[u][k][e] = colv + e < Nt ? src[e] : 0.f;
        }
        if (side) {
          const float ev = ((SideEnrolPtr)pp->enrol[k])[row + u];
          const int op = pp->op[k];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[u][k][e] = colv + e < Nt ? fusion_side_value(op, ev, v[u][k][e]) : 0.f;
        }
      }
    }
    if constexpr (T <= 2) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (row + u >= r1) break;
        const int64_t spk = espk[row + u];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (!__builtin_amdgcn_ballot_w64(ok[e])) continue;      // wave-uniform: a wave wholly beyond the last column
          float sf[T];
#pragma unroll
          for (int k = 0; k < T; ++k) sf[k] = v[u][k][e];
          fusion_account<T, -1>(A, sf, ok[e], ts[e] == spk, S.P);
        }
      }
    } else {
      // ONE copy of the account behind a rolled loop, as in the matrix kernel and for its reason
#pragma unroll 1
      for (int q = 0; q < 4 * U; ++q) {
        const int u = q >> 2, e = q & 3;
        if (row + u >= r1) break;
        const bool valid = colv + e < Nt;
        if (!__builtin_amdgcn_ballot_w64(valid)) continue;        // wave-uniform: a wave wholly beyond the last column
        const int64_t spk = espk[row + u];
        int64_t tse = ts[0];
#pragma unroll
        for (int i = 1; i < 4; ++i) tse = e == i ? ts[i] : tse;
        float sf[T];
#pragma unroll
        for (int k = 0; k < T; ++k) {
          float x = v[0][k][0];
#pragma unroll
          for (int i = 1; i < 4 * U; ++i) x = q == i ? v[i >> 2][k][i & 3] : x;
          sf[k] = x;
        }
        fusion_account<T, -1>(A, sf, valid, tse == spk, S.P);
      }
    }
  }
  fusion_block_store<T>(A, 0, part + blockIdx.x);
}

// out[i, j] = (float)chain(b; s_0[i, j] .. s_{K-1}[i, j], q_0(i, j) .. q_{Q-1}(i, j)): fusion_map_kernel's walk and rules (in
// place over one of the K matrices allowed, columns [Nt, ld_out) not touched); a side's four test values stay in registers.
template <int T>
__global__ __launch_bounds__(256) void fusion_side_map_kernel(const FusionSideArgs S, int64_t M, int64_t Nt, float *out, int64_t ld_out) {
  const int64_t col = (int64_t)blockIdx.x * FUSION_STRIP + (int64_t)threadIdx.x * 4;
  if (col >= Nt) return;
  const bool full = col + 3 < Nt;
  unsigned vec = 0;                          // bit k: slot k takes 16-byte loads; bit T: the output takes 16-byte stores
  float tv[T][4];                            // slot k >= K: the side's test values of this thread's columns
#pragma unroll
  for (int k = 0; k < T; ++k) {
    const bool wide = ((S.P.ld[k] & 3) == 0) && ((reinterpret_cast<uintptr_t>(S.P.s[k]) & 15) == 0) && full;
    vec |= wide ? 1u << k : 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) tv[k][e] = 0.f;
    if (k > 0 && k >= S.K) {
      const float *src = S.P.s[k] + col;
      if (wide) {
        const f32x4f q = *reinterpret_cast<const f32x4f *>(src);
        tv[k][0] = q.x; tv[k][1] = q.y; tv[k][2] = q.z; tv[k][3] = q.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) tv[k][e] = col + e < Nt ? src[e] : 0.f;
      }
    }
  }
  vec |= (((ld_out & 3) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0) && full) ? 1u << T : 0u;
  for (int64_t row = blockIdx.y; row < M; row += gridDim.y) {
    // bases, pitches, weights, enrol vectors and ops are re-read from the kernel-argument segment per row (scalar loads) and
    // the 16-byte flags sit in one per-thread bit mask: held across the loop they are some 90 scalar registers at T = 8, which
    // spill (the pass kernel's device, for the same reason)
    FusionSideArgsPtr pp = (FusionSideArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(pp), "+v"(vec));
    const double c = pp->P.c;
    double y[4] = {c, c, c, c};
#pragma unroll
    for (int k = 0; k < T; ++k) {
      float x[4];
      if (k > 0 && k >= pp->K) {
        const float ev = ((SideEnrolPtr)pp->enrol[k])[row];
        const int op = pp->op[k];
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = fusion_side_value(op, ev, tv[k][e]);
      } else {
        const float *src = const_cast<const float *>(pp->P.s[k]) + row * pp->P.ld[k] + col;
        if (vec >> k & 1u) {
          const f32x4f q = *reinterpret_cast<const f32x4f *>(src);
          x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) x[e] = col + e < Nt ? src[e] : 0.f;
        }
      }
      const double ak = pp->P.a[k];
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = fma(ak, (double)x[e], y[e]);
    }
    float *dst = out + row * ld_out + col;
    if (vec >> T & 1u) {
      f32x4f q;
      q.x = (float)y[0]; q.y = (float)y[1]; q.z = (float)y[2]; q.w = (float)y[3];
      *reinterpret_cast<f32x4f *>(dst) = q;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (col + e < Nt) dst[e] = (float)y[e];
    }
  }
}

// ------------------------------------------------------------------------------------ launchers (called by fusion.hip)
#define FUSION_SIDE_DISPATCH(T, CALL)                                          \
  switch (T) {                                                                \
    case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; \
    case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; default: CALL(8); break; \
  }

void fusion_side_launch_strip(plda_handle *h, const FusionSideArgs &S, int T, int64_t rows, int64_t Nt, const int64_t *espk,
                              const int64_t *tspk, int64_t blocks, int64_t rows_per_wg, plda_fusion_record *part) {
#define FUSION_SIDE_CALL(TT) fusion_side_pass_strip_kernel<TT><<<(unsigned)blocks, 256, 0, h->stream>>>(S, rows, Nt, espk, tspk, rows_per_wg, part)
  FUSION_SIDE_DISPATCH(T, FUSION_SIDE_CALL)
#undef FUSION_SIDE_CALL
}

void fusion_side_launch_map(plda_handle *h, const FusionSideArgs &S, int T, int64_t M, int64_t Nt, float *out, int64_t ld_out) {
  const dim3 grid((unsigned)ceil_div(Nt, (int64_t)FUSION_STRIP), (unsigned)std::min<int64_t>(M, 4096));
#define FUSION_SIDE_CALL(TT) fusion_side_map_kernel<TT><<<grid, 256, 0, h->stream>>>(S, M, Nt, out, ld_out)
  FUSION_SIDE_DISPATCH(T, FUSION_SIDE_CALL)
#undef FUSION_SIDE_CALL
}

}  // namespace plda
