// The device pieces of the one-launch trainers, shared by train.hip (one radial kernel: tr_body) and train_tree_lds.h (a SumKernel /
// ProductKernel tree: ttl_body): the wave sum, the 16 x 16 block chains on the LDS block image of diag_block.h, the deal of the blocks to
// the waves, and the phases of a step that do not depend on how Sigma was assembled -- the blocked Cholesky with its inverse, the last
// row block of the inverse, Gamma = L^-1 Y and A = L^-T Gamma.  The arithmetic is train.hip's, moved here unchanged.  Also what the two
// kernels and their host drivers (train_host.h) agree on: the head of the LDS layout and the step loop's arguments.
#pragma once
#include "ffgp_internal.h"
#include "diag_block.h"

#define TR_T 512
#define TR_N 128
#define TR_D 16
#define TR_Y 16

// The head of both kernels' LDS (doubles), the layout the stage functions below assume: S 36 * 272 | Xs [128][17] | Ym, Gam, Am [128][16]
// each | piv [128] | dvec [128]; a kernel's own tail begins at TR_OFF_TAIL.
#define TR_OFF_XS (NBLK_LOWER * BLKSZ)
#define TR_OFF_YM (TR_OFF_XS + TR_N * (TR_D + 1))
#define TR_OFF_GAM (TR_OFF_YM + TR_N * TR_Y)
#define TR_OFF_AM (TR_OFF_GAM + TR_N * TR_Y)
#define TR_OFF_PIV (TR_OFF_AM + TR_N * TR_Y)
#define TR_OFF_DVEC (TR_OFF_PIV + TR_N)
#define TR_OFF_TAIL (TR_OFF_DVEC + TR_N)

// The step loop's arguments, by value to every one-launch trainer's kernel; filled in one place (train_block_open, train_host.h).
struct TrainLoop {
  int steps;
  double lr, b1, b2, eps;
  const double* bc;                      // [steps][2]: 1 - beta1^t, sqrt(1 - beta2^t) (ffgp_adam_bc_table, drivers.h)
  int* info;                             // [models] status: 0, or the 1-based index of the first non-positive pivot of the step that failed
  int* fail_step;                        // [models] the step at which it happened
};

// sum over the 64 lanes of the wave, in all of them: four DPP steps inside the rows of 16 lanes, then the rows exchanged by gfx950's
// row swaps (the shuffle form, ds_bpermute, is an LDS crossbar round trip per step: 6 dependent trips per value)
template <int CTRL>
__device__ __forceinline__ double tr_dpp_add(double x) {
  int lo = __double2loint(x), hi = __double2hiint(x);
  lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xf, 0xf, true);
  hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xf, 0xf, true);
  return x + __hiloint2double(hi, lo);
}
__device__ __forceinline__ double tr_wsum(double x) {
  x = tr_dpp_add<0xB1>(x);
  x = tr_dpp_add<0x4E>(x);
  x = tr_dpp_add<0x141>(x);
  x = tr_dpp_add<0x140>(x);
  {
    const int lo = __double2loint(x), hi = __double2hiint(x);
    const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    x = __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
  }
  const int lo = __double2loint(x), hi = __double2hiint(x);
  const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
}

// block dealt to `wave` in round q of the assembly / the Sigma^-1 pass: the row-major enumeration has the expensive blocks of the Sigma^-1
// pass first (block (bi, bj) costs nst - bi products), so the rounds run forwards and backwards in turn -- 16 products for the busiest
// wave at n = 128 instead of 19.  Both passes MUST deal alike: the kernel values travel from one to the other by (block, lane) slot.
__device__ __forceinline__ int tr_deal(int q, int wave) { return 8 * q + ((q & 1) ? 7 - wave : wave); }
// acc += sum_{kb = k0}^{k1 - 1} op(P_kb) * Q_kb over 16 x 16 blocks, the NEXT block's operands requested before this block's four MFMAs
// (a runtime loop of load-then-multiply rounds waits one LDS round trip per block).  P_kb at baseA + offA(kb): element (m, k) at
// [m * lda + k], or (TA) the transposed block: (m, k) at [k * lda + m]; Q_kb at baseB + offB(kb): element (k, n) at [k * ldb + n].
template <bool TA, class OA, class OB>
__device__ __forceinline__ void tr_chain(d4_t& acc, int k0, int k1, const double* baseA, OA offA, int lda, const double* baseB, OB offB,
                                         int ldb, int lane) {
  if (k0 >= k1) return;
  const int m = lane & 15, g = lane >> 4;
  double a[4], b[4];
  {
    const double* pa = baseA + offA(k0);
    const double* pb = baseB + offB(k0);
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {
      const int k = kq * 4 + g;
      a[kq] = TA ? pa[k * lda + m] : pa[m * lda + k];
      b[kq] = pb[k * ldb + m];
    }
  }
  for (int kb = k0; kb < k1; ++kb) {
    double an[4], bn[4];
    const int kn = min(kb + 1, k1 - 1);      // (the last round re-reads its own block)
    const double* pa = baseA + offA(kn);
    const double* pb = baseB + offB(kn);
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {
      const int k = kq * 4 + g;
      an[kq] = TA ? pa[k * lda + m] : pa[m * lda + k];
      bn[kq] = pb[k * ldb + m];
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
// accumulator (lane (g, c), register r = entry (g + 4 r, c)) -> the block's [16][17] home
__device__ __forceinline__ void tr_store(double* dst, const d4_t& acc, int g, int c, double sign) {
#pragma unroll
  for (int r = 0; r < 4; ++r) dst[(g + 4 * r) * BLD + c] = sign * acc[r];
}

// a uniform word / pointer parked in LDS, read where it is used: loop-invariant values hoisted out of the step loop stay in scalar
// registers for the whole kernel, and the scalar file is full (its spills take vector registers the step's phases need)
__device__ __forceinline__ int tr_lds_int(const int* p) { return __builtin_amdgcn_readfirstlane(*reinterpret_cast<const volatile int*>(p)); }
__device__ __forceinline__ double* tr_lds_ptr(const int* p) {
  const unsigned lo = (unsigned)tr_lds_int(p), hi = (unsigned)tr_lds_int(p + 1);
  return reinterpret_cast<double*>(((unsigned long long)hi << 32) | lo);
}

// ---- blocked Cholesky over 16-column stages AND the inverse, two barriers per stage, on the block image S (Sigma in its lower block
//      triangle, diagonal blocks symmetric-full, identity beyond n; nst = ceil(n / 16) stages).
//   [A] wave 0 applies column jj - 1 to its diagonal block (jj, jj) and factors + inverts it in registers (F: the slot receives
//       inv(L_jj), the pivots go to piv[]); in its shadow the helper waves -- every wave that does not share wave 0's SIMD: fp64
//       MFMAs and the pivot loop's fp64 vector instructions use the same pipe -- apply column jj - 1 to all the other blocks and
//       compute row block jj - 1 of the inverse, X[s][j] = -inv(L_s) sum_{k=j}^{s-1} L[s][k] X[k][j], into registers;
//   [B] the inverse's row is stored over row jj - 1 of L (nobody reads it any more) and column jj is solved by all waves.
// flags[0] receives the 1-based index of the first non-positive pivot among the first n (it is left alone when already set).
// hidx / nh: HELPER_ROLES of diag_block.h.  PROF(k): the caller's phase timer, behind the barrier of [A] (2) and of [B] (3).
// (A macro, as HELPER_ROLES is: as an inlined function the same loop compiled to another register allocation of train.hip's kernels,
//  226 instead of 242 registers in <8> and other spills in <16>; as text they keep the allocation they were measured with.)
#define TR_F16(JJ) f16_step_dpp<JJ>(v, w, rowA, rowW, hA, hW, pRow, pt, ptw, dcur, ycur, cc, gg);
#define TR_FACTOR_STAGES(S, piv, flags, n, nst, lane, wave, g, c, hidx, nh, PROF)                                                                \
  for (int jj = 0; jj < nst; ++jj) {                                                                                                             \
    d4_t Xn[2];                                                                                                                                  \
    if (wave == 0) {                                                                                                                             \
      double* Dj = S + blk_off(jj, jj);                                                                                                          \
      d4_t upd = {0.0, 0.0, 0.0, 0.0};                                                                                                           \
      if (jj > 0) mma16<true>(upd, S + blk_off(jj, jj - 1), BLD, S + blk_off(jj, jj - 1), BLD, lane);                                            \
      int cc = c, gg = g;                                                                                                                        \
      asm volatile("" : "+v"(cc), "+v"(gg));                                                                                                     \
      double v[4], w[4];                                                                                                                         \
  _Pragma("unroll")                                                                                                                              \
      for (int r = 0; r < 4; ++r) {                                                                                                              \
        v[r] = Dj[(gg + 4 * r) * BLD + cc] - upd[r];                                                                                             \
        w[r] = (gg + 4 * r == cc) ? 1.0 : 0.0;                                                                                                   \
      }                                                                                                                                          \
      double rowA = bperm_d(v[0], cc);                                                                                                           \
      double rowW = (cc == 0) ? 1.0 : 0.0;                                                                                                       \
      {                                                                                                                                          \
        double hA = bperm_d(v[0], 16 + cc), hW = (cc == 1) ? 1.0 : 0.0;                                                                          \
        double pRow = 0.0, pt = 0.0, ptw = 0.0;                                                                                                  \
        double dcur = row_bcast64<0>(rowA), ycur = __builtin_amdgcn_rcp(dcur);                                                                   \
        TR_F16(0) TR_F16(1) TR_F16(2) TR_F16(3) TR_F16(4) TR_F16(5) TR_F16(6) TR_F16(7) TR_F16(8) TR_F16(9) TR_F16(10) TR_F16(11)                \
        TR_F16(12) TR_F16(13) TR_F16(14) TR_F16(15)                                                                                              \
      }                                                                                                                                          \
      const int q = c >> 2;                                                                                                                      \
      const double dsel = (q == 0) ? v[0] : (q == 1) ? v[1] : (q == 2) ? v[2] : v[3];                                                            \
      const double dcol = bperm_d(dsel, 16 * (c & 3) + c);                                                                                       \
      const double rs = rsqrt_nr(dcol);                                                                                                          \
      const unsigned long long nonpos = __ballot(!(dcol > 0.0)) & 0xffffull;                                                                     \
      const int bad = nonpos ? __ffsll((long long)nonpos) : 0;                                                                                   \
      if (g == 0) piv[jj * 16 + c] = dcol;                                                                                                       \
  _Pragma("unroll")                                                                                                                              \
      for (int r = 0; r < 4; ++r) {                                                                                                              \
        const int i = g + 4 * r;                                                                                                                 \
        const double rsi = bperm_d(rs, i);                                                                                                       \
        Dj[i * BLD + c] = (i >= c) ? w[r] * rsi : 0.0;                                                                                           \
      }                                                                                                                                          \
      if (bad && lane == 0 && jj * 16 + bad <= n && flags[0] == 0) flags[0] = jj * 16 + bad;                                                     \
    } else if (hidx >= 0 && jj > 0) {                                                                                                            \
      const int m = nst - jj;                                                                                                                    \
      for (int t = 1 + hidx; t < m * (m + 1) / 2; t += nh) {                                                                                     \
        int a, b;                                                                                                                                \
        blk_unrank(t, a, b);                                                                                                                     \
        const int i = jj + a, k = jj + b;                                                                                                        \
        d4_t acc = {0.0, 0.0, 0.0, 0.0};                                                                                                         \
        mma16<true>(acc, S + blk_off(i, jj - 1), BLD, S + blk_off(k, jj - 1), BLD, lane);                                                        \
        double* dst = S + blk_off(i, k);                                                                                                         \
  _Pragma("unroll")                                                                                                                              \
        for (int r = 0; r < 4; ++r) dst[(g + 4 * r) * BLD + c] -= acc[r];                                                                        \
      }                                                                                                                                          \
      const int s_ = jj - 1;                                                                                                                     \
  _Pragma("unroll")                                                                                                                              \
      for (int q2 = 0; q2 < 2; ++q2) {                                                                                                           \
        const int j = hidx + q2 * nh;                                                                                                            \
        if (j >= s_) continue;                                                                                                                   \
        d4_t T = {0.0, 0.0, 0.0, 0.0};                                                                                                           \
        tr_chain<false>(T, j, s_, S + blk_off(s_, 0), [](int k) { return k * BLKSZ; }, BLD, S, [j](int k) { return blk_off(k, j); }, BLD, lane); \
        d4_t acc = {0.0, 0.0, 0.0, 0.0};                                                                                                         \
        const double* Ws = S + blk_off(s_, s_);                                                                                                  \
  _Pragma("unroll")                                                                                                                              \
        for (int kq = 0; kq < 4; ++kq) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ws[c * BLD + kq * 4 + g], T[kq], acc, 0, 0, 0);                \
        Xn[q2] = acc;                                                                                                                            \
      }                                                                                                                                          \
    }                                                                                                                                            \
    LDS_BARRIER();                                                                                                                               \
    PROF(2);                                                                                                                                     \
    if (hidx >= 0 && jj > 0) {                                                                                                                   \
  _Pragma("unroll")                                                                                                                              \
      for (int q2 = 0; q2 < 2; ++q2) {                                                                                                           \
        const int j = hidx + q2 * nh;                                                                                                            \
        if (j < jj - 1) tr_store(S + blk_off(jj - 1, j), Xn[q2], g, c, -1.0);                                                                    \
      }                                                                                                                                          \
    }                                                                                                                                            \
    for (int i = jj + 1 + wave; i < nst; i += 8) {                                                                                               \
      d4_t acc = {0.0, 0.0, 0.0, 0.0};                                                                                                           \
      mma16<true>(acc, S + blk_off(i, jj), BLD, S + blk_off(jj, jj), BLD, lane);                                                                 \
      tr_store(S + blk_off(i, jj), acc, g, c, 1.0);                                                                                              \
    }                                                                                                                                            \
    LDS_BARRIER();                                                                                                                               \
    PROF(3);                                                                                                                                     \
  }

// ---- the last row block of the inverse (s = nst - 1), one column per wave
__device__ __forceinline__ void tr_inverse_last_row(double* S, int nst, int lane, int wave, int g, int c) {
  if (nst > 1) {
    const int s_ = nst - 1, j = wave;
    d4_t X = {0.0, 0.0, 0.0, 0.0};
    if (j < s_) {
      d4_t T = {0.0, 0.0, 0.0, 0.0};
      tr_chain<false>(T, j, s_, S + blk_off(s_, 0), [](int k) { return k * BLKSZ; }, BLD, S, [j](int k) { return blk_off(k, j); }, BLD, lane);
      const double* Ws = S + blk_off(s_, s_);
#pragma unroll
      for (int kq = 0; kq < 4; ++kq) X = __builtin_amdgcn_mfma_f64_16x16x4f64(Ws[c * BLD + kq * 4 + g], T[kq], X, 0, 0, 0);
    }
    LDS_BARRIER();
    if (j < s_) tr_store(S + blk_off(s_, j), X, g, c, -1.0);
    LDS_BARRIER();
  }
}

// ---- Gamma = W Y and A = W^T Gamma on the matrix cores (W = L^-1, lower, in S; the d <= 16 target columns are one block column of the
//      zero-padded [128][16] images): wave w owns block row w of Gamma (w + 1 products) and block row 7 - w of A (w + 1 products).
//      The caller puts a barrier between the two, and one behind A.
__device__ __forceinline__ void tr_gamma_rows(const double* S, const double* Ym, double* Gam, int nst, int lane, int wave, int g, int c) {
  if (wave < nst) {
    const int bi = wave;
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    tr_chain<false>(acc, 0, bi + 1, S + blk_off(bi, 0), [](int kb) { return kb * BLKSZ; }, BLD, Ym, [](int kb) { return kb * 16 * TR_Y; },
                    TR_Y, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) Gam[(bi * 16 + g + 4 * r) * TR_Y + c] = acc[r];
  }
}
// (acc: the wave's block of A, for a caller that has more to do with it; false: this wave has no block row)
__device__ __forceinline__ bool tr_alpha_rows(const double* S, const double* Gam, double* Am, int nst, int lane, int wave, int g, int c, d4_t& acc) {
  if (7 - wave >= nst) return false;
  const int bi = 7 - wave;
  tr_chain<true>(acc, bi, nst, S, [bi](int kb) { return blk_off(kb, bi); }, BLD, Gam, [](int kb) { return kb * 16 * TR_Y; }, TR_Y, lane);
#pragma unroll
  for (int r = 0; r < 4; ++r) Am[(bi * 16 + g + 4 * r) * TR_Y + c] = acc[r];
  return true;
}

// ---- CAR members (ffgp_train_car_raw): the Monte-Carlo fidelity integral of fidelity_kernel_MCMC and its partials, by ONE wave (all 64
//      lanes call; z1 / z2: the samples as doubles -- fp32 draws widened, f32 set, or fp64 draws).  With l = |lz| + zeps, w2 = (hf - lf)^2:
//        e_i = u_i - 1/2 ((z1_i - z2_i) / l)^2,  m = mean_i exp(e_i),  s = |sz| m w2
//      u_i in binary32, as torch evaluates `-b * (z1 - hf) - b * (z2 - hf)` (a 0-dim fp64 parameter times an fp32 tensor), never
//      contracted; z1 / l - z2 / l two fp64 divisions of the widened samples; from exp on fp64.  fp64 draws (!f32; torch's default
//      dtype float64): u_i is the same expression in fp64.  The partials are plain fp64.
//      out[0] = s, out[1] = ds/db, out[2] = ds/dlz, out[3] = ds/dsz (sgn(0) = 0), the same in every lane.  The one copy: the one-launch
//      trainer (train.hip) and the launch-per-stage loop (train_loop.hip) both call it, so the two routes form the same s bit for bit.
__device__ __forceinline__ void car_scale_wave(double b, double lz, double sz, double zeps, const double* z1, const double* z2, bool f32,
                                               int nz, double lf, double hf, int lane, double out[4]) {
  const double l = fabs(lz) + zeps;
  const float nb = -(float)b, hff = (float)hf;
  double se = 0.0, sb = 0.0, sl = 0.0;
  for (int i = lane; i < nz; i += 64) {
    const double x1 = z1[i], x2 = z2[i];
    double u;
    if (f32) {      // (the widened samples convert back exactly)
      const float a1 = __fsub_rn((float)x1, hff), a2 = __fsub_rn((float)x2, hff);
      u = (double)__fadd_rn(__fmul_rn(nb, a1), __fmul_rn(nb, a2));
    } else {
      u = __dadd_rn(__dmul_rn(-b, __dsub_rn(x1, hf)), __dmul_rn(-b, __dsub_rn(x2, hf)));
    }
    const double dd = __dsub_rn(x1 / l, x2 / l);
    const double ex = exp(__dsub_rn(u, 0.5 * __dmul_rn(dd, dd)));
    const double dz = x1 - x2;
    se += ex;
    sb += ex * ((x1 - hf) + (x2 - hf));
    sl += ex * (dz * dz);
  }
  se = tr_wsum(se);
  sb = tr_wsum(sb);
  sl = tr_wsum(sl);
  const double dlt = hf - lf, asz = fabs(sz);
  const double m = se / (double)nz;
  const double mw = __dmul_rn(__dmul_rn(m, dlt), dlt);      // z_part.mean() * (hf - lf) * (hf - lf)
  out[0] = asz * mw;
  out[1] = -asz * dlt * dlt * (sb / (double)nz);
  out[2] = asz * dlt * dlt * ((lz > 0.0) ? 1.0 : ((lz < 0.0) ? -1.0 : 0.0)) * (sl / (double)nz) / (l * l * l);
  out[3] = ((sz > 0.0) ? 1.0 : ((sz < 0.0) ? -1.0 : 0.0)) * mw;
}
