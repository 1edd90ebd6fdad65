// The tile arithmetic shared by the acquisition optimisers' kernels (acq.hip: one frozen posterior; acq_stack.hip: a stack of them):
// a 256-thread workgroup owns 16 query points, K_s / V / B live in LDS as [np][16] images, and V = L^-1 K_s, B = L^-T V are
// v_mfma_f64_16x16x4_f64 block chains whose A operand, L^-1, is read from global memory / L2 with one block of prefetch.
#pragma once
#include "drivers.h"

#define ACQ_T 256
#define ACQ_TILE 16

// acc += sum_{kb = k0}^{k1 - 1} op(A block) * Bm block kb.  A = L^-1 in global memory: block (bi, kb) as it stands, or (TA) block (kb, bi)
// transposed.  Bm: an [np][16] LDS image.  The next block's operands are requested before this block's four MFMAs (tr_chain's pattern,
// train.hip).
template <bool TA>
__device__ __forceinline__ void acq_chain(d4_t& acc, int k0, int k1, const double* __restrict__ A, int bi, int lda, const double* Bm, int lane) {
  if (k0 >= k1) return;
  const int m = lane & 15, g = lane >> 4;
  double a[4], b[4];
  {
    const double* pa = TA ? A + (size_t)(16 * k0) * lda + 16 * bi : A + (size_t)(16 * bi) * lda + 16 * k0;
    const double* pb = Bm + k0 * 256;
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {
      const int k = kq * 4 + g;
      a[kq] = TA ? pa[k * lda + m] : pa[m * lda + k];
      b[kq] = pb[k * 16 + m];
    }
  }
  for (int kb = k0; kb < k1; ++kb) {
    double an[4], bn[4];
    const int kn = min(kb + 1, k1 - 1);      // (the last round re-reads its own block)
    const double* pa = TA ? A + (size_t)(16 * kn) * lda + 16 * bi : A + (size_t)(16 * bi) * lda + 16 * kn;
    const double* pb = Bm + kn * 256;
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {
      const int k = kq * 4 + g;
      an[kq] = TA ? pa[k * lda + m] : pa[m * lda + k];
      bn[kq] = pb[k * 16 + m];
    }
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kq], b[kq], acc, 0, 0, 0);
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {
      a[kq] = an[kq];
      b[kq] = bn[kq];
    }
  }
}
// block dealt to `wave` in round q: forwards and backwards in turn, so that the chains' lengths (bi + 1, nb - bi) even out
__device__ __forceinline__ int acq_deal(int q, int wave) { return 4 * q + ((q & 1) ? 3 - wave : wave); }
