// gemm_core_widen.hip.h — bf16-storage operands for the float32 tile core of gemm_core.hip.h.
//
// A bf16 -> float32 widening is exact, so a product that reads an operand as bf16 and widens
// it on the way into LDS returns the bits of the float32 kernel on the promoted copy -- as long
// as the LDS image and the k order are the float32 kernel's.  TileLoaderH fetches the elements of
// TileLoader's f32x4 slots (same thread -> element map: 4 bf16 = one 8-byte load per slot), keeps
// the RAW halves in the prefetch registers (half the registers of a float32 set) and widens when
// it writes the same [128][BK+4] / [BK][128+4] image.  The K loops below are gemm_tile_accum's
// (plain double buffer and the two-register-set DEEP loop, without the PIPE / segmented forms,
// which no bf16 caller uses) with the loader of each operand as a template parameter, so that a
// product may mix one bf16 and one float32 operand.  compute_ktile is shared: same MFMA order.
//
// The float32 loader and loops of gemm_core.hip.h are untouched: this file only adds.
#pragma once
#include "gemm_core.hip.h"

namespace psk {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// bf16 bits -> float32: the value's upper 16 bits
__device__ __forceinline__ float widen_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float widen_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
__device__ __forceinline__ float gload1h(const uint16_t* p) {
  return __uint_as_float((uint32_t)(*(const uint16_t PS_GLOBAL*)(p)) << 16);
}
// 4 consecutive bf16 (8-byte aligned) -> f32x4
__device__ __forceinline__ f32x4 widen4(u32x2 r) {
  f32x4 v = {widen_lo(r[0]), widen_hi(r[0]), widen_lo(r[1]), widen_hi(r[1])};
  return v;
}
__device__ __forceinline__ u32x2 gload4h_raw(const uint16_t* p) { return *(const u32x2 PS_GLOBAL*)(p); }

struct OperandH {
  const uint16_t* p;  // bf16 elements
  int ld;             // in elements
  int mn0;
  int MN;
  int K;
  bool vec;  // 8-byte vector loads are legal (base 8-byte aligned, ld % 4 == 0)
};

// float32 loader under the interface the loops below expect
template <int LAYOUT, int BK, bool GUARD>
struct LdF32 : TileLoader<LAYOUT, BK, GUARD> {
  using Reg = f32x4;
  using Op = Operand;
};

template <int LAYOUT, int BK, bool GUARD>
struct TileLoaderH {
  using Reg = u32x2;
  using Op = OperandH;
  using F = TileLoader<LAYOUT, BK, GUARD>;   // thread -> element map of the float32 loader
  static constexpr int NV = F::NV;
  static constexpr int ROWS_PER_V = F::ROWS_PER_V;

  __device__ static inline void load(const OperandH& op, int k0, int tid, u32x2 (&r)[NV]) {
    if (!GUARD) {
      // wave-uniform base + one 32-bit byte offset per lane, as TileLoader::load (2-byte elements)
      uint32_t off = F::lane_byte_offset(op.ld, tid) >> 1;
      asm volatile("" : "+v"(off));
      const uint16_t* base = LAYOUT == KC ? op.p + (int64_t)op.mn0 * op.ld + k0
                                          : op.p + (int64_t)k0 * op.ld + op.mn0;
#pragma unroll
      for (int v = 0; v < NV; ++v)
        r[v] = *(const u32x2 PS_GLOBAL*)((const char PS_GLOBAL*)(base + (int64_t)(v * ROWS_PER_V) * op.ld) +
                                         (uint64_t)off);
      return;
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      int mn, k;
      F::coords(v, tid, mn, k);
      const int gmn = op.mn0 + mn;
      const int gk = k0 + k;
      // run of 4 elements along the contiguous direction: k (KC) or mn (MC)
      const uint16_t* src = LAYOUT == KC ? op.p + (int64_t)gmn * op.ld + gk
                                         : op.p + (int64_t)gk * op.ld + gmn;
      const bool row_ok = LAYOUT == KC ? gmn < op.MN : gk < op.K;
      const int first = LAYOUT == KC ? gk : gmn;
      const int extent = LAYOUT == KC ? op.K : op.MN;
      u32x2 t = {0u, 0u};
      if (row_ok) {
        if (op.vec && first + 3 < extent) {
          t = gload4h_raw(src);
        } else {
          uint32_t h[4] = {0u, 0u, 0u, 0u};
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (first + e < extent) h[e] = *(const uint16_t PS_GLOBAL*)(src + e);
          t[0] = h[0] | (h[1] << 16);
          t[1] = h[2] | (h[3] << 16);
        }
      }
      r[v] = t;
    }
  }

  // registers -> LDS image (widened: the float32 loader's image)
  __device__ static inline void store(float* s, int tid, const u32x2 (&r)[NV]) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      int mn, k;
      F::coords(v, tid, mn, k);
      float* dst = (LAYOUT == KC) ? s + mn * SmemCfg<BK>::KC_LD + k
                                  : s + k * SmemCfg<BK>::MC_LD + mn;
      *reinterpret_cast<f32x4*>(dst) = widen4(r[v]);
    }
  }
};

// acc += A * B over k in [0, Kext): gemm_tile_accum's two loops (DEEP = false: one register set,
// loads of K-tile t+1 issued at the top of iteration t; DEEP = true: deep_issue_first + deep_run).
// Same K-tile order and the same compute_ktile: bit-identical to the float32 loops on the
// widened operands.  Ends with a barrier.
template <class LdA, class LdB, int LA, int LB, int BK, bool DEEP>
__device__ inline void gemm_tile_accum_ld(const typename LdA::Op& A, const typename LdB::Op& B,
                                          int Kext, float* smem, f32x16 (&acc)[2][2]) {
  constexpr int OPS = SmemCfg<BK>::op_size(LA);
  constexpr int STG = SmemCfg<BK>::op_size(LA) + SmemCfg<BK>::op_size(LB);
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int wm = wave >> 1;
  const int wn = wave & 1;
  const int nk = (Kext + BK - 1) / BK;
  if constexpr (!DEEP) {
    typename LdA::Reg ra[LdA::NV];
    typename LdB::Reg rb[LdB::NV];
    LdA::load(A, 0, tid, ra);
    LdB::load(B, 0, tid, rb);
    LdA::store(smem, tid, ra);
    LdB::store(smem + OPS, tid, rb);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      float* cur = smem + (kt & 1) * STG;
      float* nxt = smem + ((kt + 1) & 1) * STG;
      const bool more = kt + 1 < nk;
      if (more) {
        LdA::load(A, (kt + 1) * BK, tid, ra);
        LdB::load(B, (kt + 1) * BK, tid, rb);
      }
      compute_ktile<LA, LB, BK>(cur, cur + OPS, acc, wm, wn, lane);
      if (more) {
        LdA::store(nxt, tid, ra);
        LdB::store(nxt + OPS, tid, rb);
      }
      __syncthreads();
    }
  } else {
    // two register sets; the loads are unconditional (see deep_run in gemm_core.hip.h)
    typename LdA::Reg ra0[LdA::NV], ra1[LdA::NV];
    typename LdB::Reg rb0[LdB::NV], rb1[LdB::NV];
    LdA::load(A, 0, tid, ra0);
    LdB::load(B, 0, tid, rb0);
    const int k1 = nk > 1 ? BK : 0;
    LdA::load(A, k1, tid, ra1);
    LdB::load(B, k1, tid, rb1);
    LdA::store(smem, tid, ra0);
    LdB::store(smem + OPS, tid, rb0);
    __syncthreads();
    float* s0 = smem;
    float* s1 = smem + STG;
    for (int kt = 0; kt < nk; kt += 2) {
      LdA::load(A, min(kt + 2, nk - 1) * BK, tid, ra0);
      LdB::load(B, min(kt + 2, nk - 1) * BK, tid, rb0);
      compute_ktile<LA, LB, BK>(s0, s0 + OPS, acc, wm, wn, lane);
      if (kt + 1 < nk) {
        LdA::store(s1, tid, ra1);
        LdB::store(s1 + OPS, tid, rb1);
      }
      __syncthreads();
      if (kt + 1 >= nk) break;
      LdA::load(A, min(kt + 3, nk - 1) * BK, tid, ra1);
      LdB::load(B, min(kt + 3, nk - 1) * BK, tid, rb1);
      compute_ktile<LA, LB, BK>(s1, s1 + OPS, acc, wm, wn, lane);
      if (kt + 2 < nk) {
        LdA::store(s0, tid, ra0);
        LdB::store(s0 + OPS, tid, rb0);
      }
      __syncthreads();
    }
  }
}

}  // namespace psk
