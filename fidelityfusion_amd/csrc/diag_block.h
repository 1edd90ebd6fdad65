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

// HELPER_ROLES(simd, wave, hidx, nh): the helper waves of stage [A] from the eight waves' SIMDs -- helper_roles.h, which the CPU test of
// the hand-out (tests/test_helper_roles_host.py: all 4^8 tables) includes as well.  The kernels that expand it -- ffgp_potrf_diag128_v4
// (potrf.hip), tr_body (train.hip), ttl_body (train_tree_lds.h) -- publish wave_simd(wave) per wave and call ROLES_SEEN behind it.
#include "helper_roles.h"

// The SIMD of wave `w` as HELPER_ROLES is to see it, and the roles it handed out.  Product build: the hardware's id, and nothing.
// -DFFGP_TEST_ROLES (libffgp_roles.so, `make roles`; tests/test_gpu_helper_roles.py): the SIMD comes from a table the test sets, 2 bits
// per wave, and lane 0 of every wave records the hidx and nh it got -- bits 3w..3w+2: hidx + 1 of wave w, bits 24..26: nh, bit 31: set
// by every writer -- so that a test which forces a placement also sees that the stage loops ran under it.  One table and one record
// per translation unit (FFGP_ROLES_TU names it in the two entry points below); the hardware hands out a placement like any of these
// whenever other workgroups share the CU.
#ifdef FFGP_TEST_ROLES
static __device__ unsigned ffgp_roles_table = 0xE4E4u;      // 0 1 2 3 0 1 2 3: two waves per SIMD
static __device__ unsigned ffgp_roles_seen = 0u;
__device__ __forceinline__ int wave_simd(int w) { return (int)(ffgp_roles_table >> (2 * w)) & 3; }
#define ROLES_SEEN(lane, wave, hidx, nh) \
  if ((lane) == 0) atomicOr(&ffgp_roles_seen, 0x80000000u | ((unsigned)(nh) << 24) | ((unsigned)((hidx) + 1) << (3 * (wave))))
#ifdef FFGP_ROLES_TU
#define FFGP_ROLES_CAT2(a, b) a##b
#define FFGP_ROLES_CAT(a, b) FFGP_ROLES_CAT2(a, b)
// set the table (bits 2w..2w+1: the SIMD of wave w) for every later launch of this translation unit's kernels
extern "C" __attribute__((visibility("default"))) int FFGP_ROLES_CAT(ffgp_test_roles_set_, FFGP_ROLES_TU)(unsigned table) {
  if (hipDeviceSynchronize() != hipSuccess) return FFGP_ERR_HIP;
  if (hipMemcpyToSymbol(HIP_SYMBOL(ffgp_roles_table), &table, sizeof(table)) != hipSuccess) return FFGP_ERR_HIP;
  return hipDeviceSynchronize() == hipSuccess ? 0 : FFGP_ERR_HIP;
}
// the record of the launches since the last call (0: none of this translation unit's kernels ran), which it clears
extern "C" __attribute__((visibility("default"))) int FFGP_ROLES_CAT(ffgp_test_roles_seen_, FFGP_ROLES_TU)(unsigned* seen) {
  const unsigned zero = 0u;
  if (hipDeviceSynchronize() != hipSuccess) return FFGP_ERR_HIP;
  if (hipMemcpyFromSymbol(seen, HIP_SYMBOL(ffgp_roles_seen), sizeof(*seen)) != hipSuccess) return FFGP_ERR_HIP;
  if (hipMemcpyToSymbol(HIP_SYMBOL(ffgp_roles_seen), &zero, sizeof(zero)) != hipSuccess) return FFGP_ERR_HIP;
  return hipDeviceSynchronize() == hipSuccess ? 0 : FFGP_ERR_HIP;
}
#endif
#else
__device__ __forceinline__ int wave_simd(int) { return simd_id(); }
#define ROLES_SEEN(lane, wave, hidx, nh)
#endif

// The function form of the hand-out and its report, for a kernel that has no measured register allocation to keep (the macros above
// are spelled out in the three kernels that were measured with them): simd[w] as HELPER_ROLES wants it, published behind a barrier.
__device__ __forceinline__ void helper_roles(const int* simd, int lane, int wave, int& hidx_out, int& nh_out) {
  HELPER_ROLES(simd, wave, hidx, nh);
  ROLES_SEEN(lane, wave, hidx, nh);
  hidx_out = hidx;
  nh_out = nh;
}
