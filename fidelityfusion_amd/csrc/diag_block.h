// The LDS block image of a 128 x 128 symmetric block and the stage-loop primitives on it, shared by the factorisation's diagonal-block
// kernel (ffgp_potrf_diag128_v4, potrf.hip) and the one-launch trainer (tr_body, train.hip), whose stage loop it came from.
#pragma once
#include "ffgp_internal.h"
#include "f16_steps.h"

// Only the 36 lower 16 x 16 blocks, each [16][17] doubles (the pad makes the MFMA operand reads bank-conflict-free).  78 KiB instead of
// 130 KiB for the dense image: the kernel must fit beside ONE resident GEMM workgroup (72 KiB of the CU's 160 KiB), otherwise the
// look-ahead panel factor would never be scheduled while the trailing update occupies the chip.
#define BLD 17
#define BLKSZ (16 * BLD)
#define NBLK_LOWER 36

__device__ __forceinline__ int blk_off(int bi, int bj) { return (bi * (bi + 1) / 2 + bj) * BLKSZ; }

// t-th block of the row-major enumeration of the lower block triangle -> (bi, bj).  (ffgp_potrf_diag128_v4 spells it out: as calls it
// compiled to a different schedule of that kernel.)
__device__ __forceinline__ void blk_unrank(int t, int& bi, int& bj) {
  bi = 0;
#pragma unroll
  for (int q = 1; q < 8; ++q) bi += (t >= q * (q + 1) / 2) ? 1 : 0;
  bj = t - bi * (bi + 1) / 2;
}

__device__ __forceinline__ double rsqrt_nr(double d) {
  double y = __builtin_amdgcn_rsq(d);
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const double e = __builtin_fma(-d * y, y, 1.0);
    y = __builtin_fma(0.5 * y, e, y);
  }
  return y;
}

// 16x16 MFMA tile product helper: acc += Arows(16 x 16, K-major at pa[row*lda_ + k]) * B
//   KB = true : B given K-major  (B^T stored: element (n,k) at pb[n*ldb_ + k])
//   KB = false: B given N-major  (element (k,n) at pb[k*ldb_ + n])
template <bool KB>
__device__ __forceinline__ void mma16(d4_t& acc, const double* pa, int lda_, const double* pb, int ldb_, int lane) {
#pragma unroll
  for (int kq = 0; kq < 4; ++kq) {
    const int k = kq * 4 + (lane >> 4);
    const double a = pa[(lane & 15) * lda_ + k];
    const double b = KB ? pb[(lane & 15) * ldb_ + k] : pb[k * ldb_ + (lane & 15)];
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
}

// workgroup barrier that publishes LDS only: __syncthreads() also drains the wave's GLOBAL stores (L, the Dinv store, the trainer's
// parked kernel values), which nobody inside the kernel reads, and would expose their round trip to L2 at every barrier behind them
#define LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

__device__ __forceinline__ int simd_id() {
  return (int)__builtin_amdgcn_s_getreg((1 << 11) | (4 << 6) | 4) & 3;     // HW_REG_HW_ID (4), SIMD_ID = bits 5:4
}

// The helper waves of stage [A]: the waves that do not share wave 0's SIMD (fp64 MFMAs and the pivot loop's DP-ALU work share a pipe),
// six with two waves per SIMD.  simd[w] = simd_id() of wave w, published behind a barrier.  Declares hidx (this wave's index among the
// helpers, -1 for the others) and nh (their number).  The stage loops need nh >= 4 (the inverse's row blocks take two columns per helper
// and have up to seven): a placement that leaves fewer makes all seven other waves helpers.  (A macro: as an inlined function the same
// code compiled to a different instruction order, in wave 0's pivot loop of ffgp_small_mfma_kernel among other places.)
#define HELPER_ROLES(simd, wave, hidx, nh)          \
  int hidx = -1, nh = 0;                            \
  {                                                 \
    const int s0_ = (simd)[0];                      \
    for (int w_ = 1; w_ < 8; ++w_) {                \
      const bool is_h_ = (simd)[w_] != s0_;         \
      if (is_h_ && w_ == (wave)) hidx = nh;         \
      nh += is_h_ ? 1 : 0;                          \
    }                                               \
    if (nh < 4) {                                   \
      nh = 7;                                       \
      hidx = (wave) - 1;                            \
    }                                               \
    hidx = __builtin_amdgcn_readfirstlane(hidx);    \
    nh = __builtin_amdgcn_readfirstlane(nh);        \
  }
