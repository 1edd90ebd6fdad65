// What the acquisition optimisers' kernels share (acq.hip: one frozen posterior; acq_stack.hip: a stack of them; acq_tree.hip: one
// posterior on a composed kernel; acq_chain.hip: a chain of them, each fed the mean of the one below): a 256-thread
// workgroup owns 16 query points, K_s / V / B live in LDS as [np][16] images, and V = L^-1 K_s, B = L^-T V are v_mfma_f64_16x16x4_f64
// block chains whose A operand, L^-1, is read from global memory / L2 with one block of prefetch.  The host side exists once: acq_run
// (acq_stack.hip) serves both entries, a single posterior as the stack of one member.
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

// LDS of either kernel, in doubles, sized by the largest posterior of the call: three [np][16] images (the second at least 256 DM: it
// also carries the gradient partials), X [np][DM], alpha [np], the tile's points [16][DM], w^2 [DM], two [16][16] reduction pads
static constexpr size_t acq_lds_doubles(int np, int DM) {
  const size_t img = (size_t)np * 16, img1 = img > (size_t)256 * DM ? img : (size_t)256 * DM;
  return 2 * img + img1 + (size_t)np * DM + np + 16 * DM + DM + 512;
}
static_assert(acq_lds_doubles(FFGP_ACQ_MAX_N, FFGP_ACQ_MAX_D) * sizeof(double) <= 160 * 1024, "the acquisition kernels' LDS exceeds a CU's 160 KiB");

// ---- the host side: one driver (acq_run, acq_stack.hip) for both entries; the stack kernel takes AcqStackArgs as it stands
struct AcqStackMember {
  const double* X;       // [n, D]
  const double* Linv;    // [np, np], zero above the diagonal and in the padding
  const double* alpha;   // [n]
  const double* w;       // [D]
  const double* amp;
  double clamp, rinv, var_add, mean_coef, var_coef;
  int n, np, kfun, pad;
};
struct AcqStackArgs {
  AcqStackMember m[FFGP_ACQ_MAX_MEMBERS];
  const int* level;      // [Q] or null
  const double* bc;      // [2 steps] bias corrections
  double* Xq;            // [Q, D]
  double* state;         // [2 or 3, Q, D] or null (evaluate mode)
  double* trace;         // [max(steps, 1), Q]
  double* hist;          // [steps + 1, Q, D] or null
  double* grad;          // [Q, D] or null
  int F, npmax, D, Q, steps, acq, accumulate;
  double var_floor, kappa, xi, f_best, lr, b1, b2, eps;
};
// Checks the call, forms every member's L^-1 and the bias-correction table in handle workspace, launches through `launch` and waits.
// `tree` (ffgp_acq_optimize_tree only, checked by that entry): the one member's kernel is this composition, so the member carries no
// w_dev / amp_dev / kfun of its own and those three checks are skipped; it is handed on to `launch`.
// `chain` (ffgp_acq_optimize_chain only): the per-member dimension rule is members[0].D = D <= FFGP_ACQ_MAX_D - 1 and D + 1 above it,
// instead of one D for all; AcqStackArgs.D stays the D of the query points.
typedef int (*acq_launch_fn)(ffgp_handle* h, const AcqStackArgs& a, int grid, const ffgp_ktree* tree);
int acq_run(ffgp_handle* h, const ffgp_acq_stack* s, acq_launch_fn launch, double* Xq_dev, int Q, int steps, const ffgp_adam* opt, double* state_dev,
            long step0, double* trace_dev, double* hist_dev, double* grad_dev, const ffgp_ktree* tree = nullptr, bool chain = false);
