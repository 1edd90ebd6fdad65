// K Adam steps of F WIDE-output models -- more than 16 target columns, at most 128 points -- in ONE launch: ffgp_train_wide_raw
// (include/ffgp.h).  The persistent workgroup of train.hip (one per model, 512 threads, every step inside the kernel) with a loop over
// 16-column blocks of the targets between the factorisation and the gradient pass.  The V1 likelihood and all its gradients see the
// targets only through inner products of their rows, so the caller passes Z_eff [m, r] with Z_eff Z_eff^T = Z Z^T (Z = Y, or
// [y_high; y_low] of a residual member; r = m <= 256 whatever d is: train.py::compress_targets) and the likelihood's own d apart
// (d_true): a step costs ceil(r / 16) column blocks, 1-8 for a plain member and up to 16 for a residual one.
// Per step:
//   links, Sigma into LDS, blocked Cholesky AND inverse      -- train.hip's phases P0-P2 on the pieces of train_tile.h, once
//   for every column block cb:                                  three workgroup barriers per block
//     Gamma = W Y_cb (tr_gamma_rows)                          | the block sits in the targets' [128][16] image
//     |Gamma|^2 into the value, A = W^T Gamma (tr_alpha_rows),  a residual member's part of sum A .* y_low
//     A_bi A_bj^T, ONE MFMA group per block the wave owns in the gradient pass (tr_deal: up to five), added to five accumulators
//       that live across the column loop; the NEXT column block, requested from global memory at the top of this one, goes into the image
//   the five accumulators parked in a per-model global scratch with kbuf's layout (same lane, same slot), then train.hip's gradient
//   pass with aa read back from there, G = d_true / 2 Sigma^-1 - 1/2 A A^T; the reduction, the links' chain rule, Adam.
// (The A A^T image stays in accumulators only ACROSS THE COLUMN LOOP, where nothing else needs registers; kept across the gradient
//  pass as well it would need that pass unrolled five-fold around statically indexed accumulators, 40 more live registers under the
//  phase that already fills the file in train.hip's kernels.  One store and one load per entry and step buy that back.)
// One kernel serves plain and residual members (a word in LDS tells them apart, as in train.hip's residual launches).  Failure
// semantics are the one-launch form's: a Sigma that is not positive definite stops THAT model at that step.
// Covers n <= 128, D <= 16, SE / Matern 1/2, 3/2, 5/2, the V1 likelihood, diag_add and diag_vec, up to 128 columns passed for a plain
// member and 256 for a residual one, F <= 16.  Host side: train_host.h's scaffold.
#include "train_host.h"

#define TW_NRED 21        // values of the step's one workgroup reduction: ss, s_amp, tr G, log-det, tot[16], dloss/drho
#define TW_MAX_COLS 128   // columns passed, a plain member
#define TW_MAX_COLS_RES 256

struct WideModel {
  int n, D, d, nw;                       // d: the columns PASSED (the column loop runs over them); nw: raw length scales
  int dt;                                // the likelihood's d
  int res;                               // 0 plain member, 1 residual, 2 residual with the two variance diagonals
  const double* X;
  const double* ya;                      // [n, d] the targets (a residual member: y_high)
  const double* yl;                      // [n, d] a residual member's y_low
  const double* vl; const double* vh;    // a residual member's optional diagonals: entry i at vl[i * vl_stride], vh[i * vh_stride]
  long vl_stride, vh_stride;
  double* w; double* amp; double* dadd;  // RAW parameters, updated in place when the kernel ends
  double* rho; double* rho_last;         // a residual member's raw rho; optional: rho at the start of the last step taken
  const double* diag_vec; long diag_stride;
  ffgp_links l;
  double clamp, rinv, pi_const;
  int kfun;
  double* state;                         // [exp_avg (nw + 2 (+ 1)) | exp_avg_sq (nw + 2 (+ 1))]
  double* trace;                         // [steps]
  double* kbuf;                          // [36][4][64] kernel values K / amp: written by the assembly, read by the gradient pass (same lane, same slot)
  double* abuf;                          // [36][4][64] (A A^T) entries: written behind the column loop, read by the gradient pass (same lane, same slot)
};

// LDS (doubles): the shared head of train_tile.h (S | Xs | Ym, Gam, Am | piv | dvec) | small | vl | vh | sgv | diag G [128] each | rsum [8] |
// rho at the start of the step | the parked words
#define TW_OFF_SMALL TR_OFF_TAIL
#define TW_SMALL_DOUBLES (16 + 3 * 20 + 8 + 8 * TW_NRED + TW_NRED + 16)
#define TW_OFF_RES (TW_OFF_SMALL + TW_SMALL_DOUBLES + 3)
#define TW_LDS_DOUBLES (TW_OFF_RES + 4 * TR_N + 8 + 2 + 8)
static_assert(TW_LDS_DOUBLES * sizeof(double) <= 160 * 1024, "the wide trainer's LDS exceeds a CU's 160 KiB");

// One 16-column block of the targets, global memory -> registers -> the [128][16] image: entry idx = tid + 512 u of the image, u < 4.
// fetch only requests (a residual member: y_high and y_low; zero beyond (n, d)), put forms r = y_high - rho y_low -- rounded as torch's
// `y_high - rho * y_low`: a product, then a difference, never contracted -- and stores the rows below n (the others stay zero).
#define TW_FETCH (TR_N * TR_Y / TR_T)
__device__ __forceinline__ void tw_fetch(double (&fa)[TW_FETCH], double (&fb)[TW_FETCH], const double* ya, const double* yl, int isres, int n,
                                         int d, int c0, int tid) {
#pragma unroll
  for (int u = 0; u < TW_FETCH; ++u) {
    const int idx = tid + TR_T * u, i = idx >> 4, q = c0 + (idx & 15);
    const bool ok = i < n && q < d;
    fa[u] = ok ? ya[(size_t)i * d + q] : 0.0;
    fb[u] = (ok && isres) ? yl[(size_t)i * d + q] : 0.0;
  }
}
__device__ __forceinline__ void tw_put(double* Ym, const double (&fa)[TW_FETCH], const double (&fb)[TW_FETCH], int isres, double rho, int n, int tid) {
#pragma unroll
  for (int u = 0; u < TW_FETCH; ++u) {
    const int idx = tid + TR_T * u;
    if ((idx >> 4) < n) Ym[idx] = isres ? __dsub_rn(fa[u], __dmul_rn(rho, fb[u])) : fa[u];
  }
}

// DM: the input dimensions the per-entry loops are unrolled for (8 or 16: every model of the launch has D <= DM)
template <int DM>
__device__ __forceinline__ void tw_body(const WideModel& M, const TrainLoop& cm) {
  constexpr int NRED = TW_NRED;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* S = lds;
  double* Xs = lds + TR_OFF_XS;
  double* Ym = lds + TR_OFF_YM;
  double* Gam = lds + TR_OFF_GAM;
  double* Am = lds + TR_OFF_AM;
  double* piv = lds + TR_OFF_PIV;
  double* dvec = lds + TR_OFF_DVEC;
  double* wv = lds + TW_OFF_SMALL;         // [16] effective inverse length scales
  double* raw = wv + 16;                   // [20] raw parameters: w (nw) | amp | dadd | rho
  double* mom = raw + 20;                  // [20] exp_avg
  double* mo2 = mom + 20;                  // [20] exp_avg_sq
  double* sc = mo2 + 20;                   // [8]  amp, dadd
  double* red = sc + 8;                    // [8][NRED] per-wave partial sums
  double* tot = red + 8 * NRED;            // [NRED] the step's totals
  int* flags = reinterpret_cast<int*>(tot + NRED);        // [0] bad pivot of the current step; [8..15] the waves' SIMDs
  double* rvl = lds + TW_OFF_RES;          // residual members: [128] v_low diagonal
  double* rvh = rvl + TR_N;                // [128] v_high diagonal
  double* sgv = rvh + TR_N;                // [128] sgn(s_i) v_low,ii of the current step
  double* gdg = sgv + TR_N;                // [128] G_ii of the current step
  double* rsum = gdg + TR_N;               // [8]   per-wave sums of A .* y_low
  double* rho0 = rsum + 8;                 // [1]   rho at the start of the current step
  int* rmode = reinterpret_cast<int*>(rho0 + 2);      // [0] M.res; [1] the columns passed; [2..11] targets / y_high, y_low, rho, rho_last, abuf
                                                      // (read through tr_lds_int / tr_lds_ptr)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int n = M.n, D = M.D, nw = M.nw;
  const int nst = (n + 15) >> 4, nblk = nst * (nst + 1) / 2;
  const int npar = nw + 2 + (M.res ? 1 : 0);      // (a residual member's rho is raw[nw + 2])
  const double oscale = (M.l.out_scale != 0.0) ? M.l.out_scale : 1.0;
  ExpCoef ec;
  ffgp_exp_load(ec);

  // ---- once: the diagonal extra, parameters and moments into LDS; identity padding of the blocks the factorisation never touches
  // targets, Gamma and A live as [128][16] images, zero beyond n: the matrix-core products read them without guards
  for (int idx = tid; idx < TR_N * TR_Y; idx += TR_T) {
    Ym[idx] = 0.0;      // (a column block is loaded at the top of every step and under the block before it)
    Gam[idx] = 0.0;
    Am[idx] = 0.0;
  }
  for (int idx = tid; idx < TR_N * (TR_D + 1); idx += TR_T) Xs[idx] = 0.0;      // (columns >= D and rows >= n stay zero: the unrolled loops read them)
  for (int i = tid; i < TR_N; i += TR_T) {
    dvec[i] = (!M.res && M.diag_vec && i < n) ? M.diag_vec[(size_t)i * M.diag_stride] : 0.0;      // (a residual member's: formed at every step from rho)
    sgv[i] = 0.0;
    gdg[i] = 0.0;
    rvl[i] = (M.res == 2 && i < n) ? M.vl[(size_t)i * M.vl_stride] : 0.0;
    rvh[i] = (M.res == 2 && i < n) ? M.vh[(size_t)i * M.vh_stride] : 0.0;
  }
  if (tid < npar) {
    if (M.res && tid == nw + 2) raw[tid] = M.rho[0];
    else raw[tid] = (tid < nw) ? M.w[tid] : (tid == nw ? M.amp[0] : M.dadd[0]);
    mom[tid] = M.state[tid];
    mo2[tid] = M.state[npar + tid];
  }
  for (int t = wave; t < NBLK_LOWER; t += 8) {
    int bi, bj;
    blk_unrank(t, bi, bj);
    if (bi < nst) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) S[blk_off(bi, bj) + (g + 4 * r) * BLD + c] = (bi == bj && g + 4 * r == c) ? 1.0 : 0.0;
  }
  if (tid == 0) flags[0] = 0;
  if (lane == 0) flags[8 + wave] = wave_simd(wave);
  if (tid == 0) {
    rmode[0] = M.res;
    rmode[1] = M.d;
    const double* pv[5] = {M.ya, M.yl, M.rho, M.rho_last, M.abuf};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const unsigned long long u = reinterpret_cast<unsigned long long>(pv[k]);
      rmode[2 + 2 * k] = (int)(unsigned)u;
      rmode[3 + 2 * k] = (int)(unsigned)(u >> 32);
    }
  }
  __syncthreads();
  int hidx, nh;      // helpers of the factorisation's stage [A]
  helper_roles(flags + 8, lane, wave, hidx, nh);
  if (tid < D) wv[tid] = ffgp_link_val(M.l.w_link, raw[M.l.w_broadcast ? 0 : tid], M.l.w_c);
  if (tid == 64) sc[0] = ffgp_link_val(M.l.amp_link, raw[nw], M.l.amp_c);
  if (tid == 65) sc[1] = ffgp_link_val(M.l.dadd_link, raw[nw + 1], M.l.dadd_c);
  __syncthreads();

  const int lane_k = lane, wave_k = wave;
  for (int step = 0; step < cm.steps; ++step) {
    // (the lane coordinates opaque per iteration, as in train.hip: otherwise every per-lane offset of every phase is hoisted out of the
    //  step loop and kept alive across it)
    int lane = lane_k, wave = wave_k;
    asm volatile("" : "+v"(lane), "+s"(wave));
    const int g = lane >> 4, c = lane & 15;
    const int isres = tr_lds_int(rmode);
    const int d = tr_lds_int(rmode + 1), ncb = (d + 15) >> 4;
    // ---- P0: scaled inputs; column block 0 of the targets -- a residual member's r = y_high - rho y_low, rounded as torch's
    //      `y_high - rho * y_low` (a product, then a difference: never contracted) -- and its diagonal extra |s|, s = v_high - rho v_low
    for (int idx = tid; idx < n * D; idx += TR_T) {      // (shifted by the first point: only differences enter the kernel)
      const int i = idx / D, k = idx - i * D;
      Xs[i * (TR_D + 1) + k] = (M.X[idx] - M.X[k]) * wv[k];
    }
    {
      const double rho = isres ? raw[nw + 2] : 0.0;
      double fa[TW_FETCH], fb[TW_FETCH];
      tw_fetch(fa, fb, tr_lds_ptr(rmode + 2), tr_lds_ptr(rmode + 4), isres, n, d, 0, tid);
      tw_put(Ym, fa, fb, isres, rho, n, tid);
      if (isres == 2) {
        for (int i = tid; i < n; i += TR_T) {
          const double s = __dsub_rn(rvh[i], __dmul_rn(rho, rvl[i]));
          dvec[i] = fabs(s);
          sgv[i] = (s > 0.0) ? rvl[i] : ((s < 0.0) ? -rvl[i] : 0.0);      // (torch's abs backward: sgn(0) = 0)
        }
      }
      if (isres && tid == 0) rho0[0] = rho;
    }
    LDS_BARRIER();
    const double amp = sc[0], dadd = sc[1];

    // ---- P1: Sigma, lower block triangle (diagonal blocks symmetric-full); rows / columns beyond n are identity
    for (int q_ = 0; q_ < 5; ++q_) {
      const int t = tr_deal(q_, wave);
      if (t >= nblk) continue;
      int bi, bj;
      blk_unrank(t, bi, bj);
      double* dst = S + blk_off(bi, bj);
      const int j = bj * 16 + c;
      double xj[DM], sq[4];
#pragma unroll
      for (int k = 0; k < DM; ++k) xj[k] = Xs[j * (TR_D + 1) + k];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double* xi = Xs + (bi * 16 + g + 4 * r) * (TR_D + 1);
        sq[r] = 0.0;
#pragma unroll
        for (int k = 0; k < DM; ++k) {
          const double df = xi[k] - xj[k];
          sq[r] = __builtin_fma(df, df, sq[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = bi * 16 + g + 4 * r;
        const double s_ = fmax(sq[r], M.clamp);
        const double ev = (M.kfun == FFGP_KFUN_SE) ? ffgp_exp_fast(-0.5 * s_, ec) : ffgp_kfun_val(M.kfun, M.rinv, s_);
        M.kbuf[(t * 4 + r) * 64 + lane] = ev;
        double kv = amp * ev;
        if (i == j) kv += dadd + dvec[i];
        if (i >= n || j >= n) kv = (i == j) ? 1.0 : 0.0;
        dst[(g + 4 * r) * BLD + c] = kv;
      }
    }
    LDS_BARRIER();

    // ---- P2: blocked Cholesky over 16-column stages AND the inverse, two barriers per stage (train_tile.h)
#define TW_NOPROF(k)
    TR_FACTOR_STAGES(S, piv, flags, n, nst, lane, wave, g, c, hidx, nh, TW_NOPROF)
    if (flags[0] != 0) {       // (uniform: every thread reads the same word behind the barrier)
      if (tid == 0) {
        cm.info[blockIdx.x] = flags[0];
        cm.fail_step[blockIdx.x] = step;
      }
      for (int k = step + tid; k < cm.steps; k += TR_T) M.trace[k] = __builtin_nan("");
      break;
    }
    tr_inverse_last_row(S, nst, lane, wave, g, c);

    // ---- P3: the column loop.  Per block: Gamma = W Y_cb | |Gamma|^2, A = W^T Gamma, sum A .* y_low | A_bi A_bj^T into the wave's
    //      accumulators and the next block into the targets' image
    double ss = 0.0, ay = 0.0;
    d4_t aacc[5];
#pragma unroll
    for (int q_ = 0; q_ < 5; ++q_) aacc[q_] = d4_t{0.0, 0.0, 0.0, 0.0};
    for (int cb = 0; cb < ncb; ++cb) {
      // the next block's entries requested now, stored behind the products: their way from global memory runs under the two chains
      // (requested where they are stored, each of the four rounds waited for its own round trip: 11 us per block at n = 128)
      double fa[TW_FETCH], fb[TW_FETCH];
      if (cb + 1 < ncb) tw_fetch(fa, fb, tr_lds_ptr(rmode + 2), tr_lds_ptr(rmode + 4), isres, n, d, (cb + 1) * 16, tid);
      tr_gamma_rows(S, Ym, Gam, nst, lane, wave, g, c);
      LDS_BARRIER();
#pragma unroll
      for (int q = 0; q < TR_N * TR_Y / TR_T; ++q) {      // Y^T Sigma^-1 Y = |Gamma|^2 (rows beyond the stages were never written: zero)
        const double e_ = Gam[tid + TR_T * q];
        ss = __builtin_fma(e_, e_, ss);
      }
      d4_t acc = {0.0, 0.0, 0.0, 0.0};
      if (tr_alpha_rows(S, Gam, Am, nst, lane, wave, g, c, acc)) {
        if (isres) {      // (y_low requested after the chain, not under it, as in train.hip)
          const int bi = 7 - wave, col = cb * 16 + c;
          const double* yl = tr_lds_ptr(rmode + 4);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = bi * 16 + g + 4 * r;
            ay = __builtin_fma(acc[r], (i < n && col < d) ? yl[(size_t)i * d + col] : 0.0, ay);
          }
        }
      }
      LDS_BARRIER();
#pragma unroll
      for (int q_ = 0; q_ < 5; ++q_) {
        const int t = tr_deal(q_, wave);
        if (t >= nblk) continue;
        int bi, bj;
        blk_unrank(t, bi, bj);
        // A_bi A_bj^T: lane (c, g) brings columns 4 g .. 4 g + 3 of its row of either block -- one 32-byte read per operand -- and MFMA kq
        // takes column 4 g + kq from both: the sum over the 16 columns does not care which lane group brings which four.  (The
        // operand layout's own columns kq * 4 + g are a 16-way bank conflict on the [128][16] image.)
        const double* pa = Am + (bi * 16 + c) * TR_Y + 4 * g;
        const double* pb = Am + (bj * 16 + c) * TR_Y + 4 * g;
        double av[4], bv[4];
#pragma unroll
        for (int kq = 0; kq < 4; ++kq) {
          av[kq] = pa[kq];
          bv[kq] = pb[kq];
        }
#pragma unroll
        for (int kq = 0; kq < 4; ++kq) aacc[q_] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[kq], bv[kq], aacc[q_], 0, 0, 0);
      }
      if (cb + 1 < ncb) tw_put(Ym, fa, fb, isres, isres ? raw[nw + 2] : 0.0, n, tid);      // (nobody reads the targets' image between these two barriers)
      LDS_BARRIER();
    }
    {      // the A A^T image to its scratch, for this very lane to read back in the gradient pass
      double* ab = tr_lds_ptr(rmode + 10);
#pragma unroll
      for (int q_ = 0; q_ < 5; ++q_) {
        const int t = tr_deal(q_, wave);
        if (t >= nblk) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) ab[(t * 4 + r) * 64 + lane] = aacc[q_][r];
      }
    }
    if (isres) {
      ay = tr_wsum(ay);
      if (lane == 0) rsum[wave] = ay;
    }

    // ---- P5: per lane partial sums -- s_amp, tr G, tot[k] (length scales); Sigma^-1 block by block on the matrix cores
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this lane's parked kernel values and A A^T entries have landed
    const int dt = M.dt;
    double s_amp = 0.0, trg = 0.0, tk[DM];
#pragma unroll
    for (int k = 0; k < DM; ++k) tk[k] = 0.0;
    const double lpiv = (tid < n) ? log(piv[tid]) : 0.0;
    for (int q_ = 0; q_ < 5; ++q_) {
      const int t = tr_deal(q_, wave);
      if (t >= nblk) continue;
      int bi, bj;
      blk_unrank(t, bi, bj);
      double evs[4], aas[4];      // (requested before the block's products: the loads fly under the MFMA chain; written by this very lane)
      {
        const double* ab = tr_lds_ptr(rmode + 10);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          evs[r] = M.kbuf[(t * 4 + r) * 64 + lane];
          aas[r] = ab[(t * 4 + r) * 64 + lane];
        }
      }
      d4_t acc = {0.0, 0.0, 0.0, 0.0};
      tr_chain<true>(acc, bi, nst, S, [bi](int kb) { return blk_off(kb, bi); }, BLD, S, [bj](int kb) { return blk_off(kb, bj); }, BLD, lane);
      const int j = bj * 16 + c;
      double xj[DM];
#pragma unroll
      for (int k = 0; k < DM; ++k) xj[k] = Xs[j * (TR_D + 1) + k];
#pragma unroll 1
      for (int r = 0; r < 4; ++r) {      // (one row at a time, as in train.hip)
        const int i = bi * 16 + g + 4 * r;
        const double* xi = Xs + i * (TR_D + 1);
        const double accr = (r == 0) ? acc[0] : (r == 1) ? acc[1] : (r == 2) ? acc[2] : acc[3];
        const double ev = (r == 0) ? evs[0] : (r == 1) ? evs[1] : (r == 2) ? evs[2] : evs[3];
        const double aa = (r == 0) ? aas[0] : (r == 1) ? aas[1] : (r == 2) ? aas[2] : aas[3];
        double dsq[DM], sq = 0.0;
#pragma unroll
        for (int k = 0; k < DM; ++k) {
          const double df = xi[k] - xj[k];
          dsq[k] = df * df;
          sq += dsq[k];
        }
        const bool live = (i < n && j <= i);
        const double gv = live ? 0.5 * (double)dt * accr - 0.5 * aa : 0.0;      // G = d_true / 2 Sigma^-1 - 1/2 A A^T
        const double sym = (i == j) ? 1.0 : 2.0;
        double m2 = ev;
        if (M.kfun != FFGP_KFUN_SE) m2 = ffgp_kfun_m2d(M.kfun, M.rinv, fmax(sq, M.clamp));
        s_amp = __builtin_fma(sym * gv, ev, s_amp);
        if (i == j) {
          trg += gv;
          gdg[i] = gv;      // (residual members: the diagonal term of dloss/drho, summed behind the reduction's barrier)
        }
        const double wl = (sq >= M.clamp) ? sym * gv * amp * m2 : 0.0;
#pragma unroll
        for (int k = 0; k < DM; ++k) tk[k] = __builtin_fma(wl, dsq[k], tk[k]);
      }
    }
    // ---- one workgroup reduction for all of them (and the log-determinant: one pivot per thread)
    {
      constexpr int NV = 4 + DM;
      double vals[NV];
      vals[0] = ss; vals[1] = s_amp; vals[2] = trg;
      vals[3] = lpiv;
#pragma unroll
      for (int k = 0; k < DM; ++k) vals[4 + k] = tk[k];
#pragma unroll
      for (int q = 0; q < NV; ++q) vals[q] = tr_wsum(vals[q]);
      if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) red[wave * NRED + q] = vals[q];
      }
      LDS_BARRIER();
      if (tid < NV) {
        double x = 0.0;
#pragma unroll
        for (int wv_ = 0; wv_ < 8; ++wv_) x += red[wv_ * NRED + tid];
        tot[tid] = x;
      }
      if (isres && wave == 1) {      // dloss/drho (before the output scale) = -sum A .* y_low - sum_i G_ii sgn(s_i) v_low,ii, beside wave 0's totals
        double x = 0.0;
        if (isres == 2)
          for (int i = lane; i < n; i += 64) x = __builtin_fma(gdg[i], sgv[i], x);
        x = tr_wsum(x);
        if (lane == 0) {
          double a = 0.0;
#pragma unroll
          for (int wv_ = 0; wv_ < 8; ++wv_) a += (7 - wv_ < nst) ? rsum[wv_] : 0.0;
          tot[NRED - 1] = -a - x;
        }
      }
      LDS_BARRIER();
    }
    // ---- P6: the loss of this step (before the update), the raw gradients through the links, Adam
    const double value = oscale * (0.5 * tot[0] + (double)dt * 0.5 * tot[3] + 0.5 * (double)n * (double)dt * log(2.0 * M.pi_const));
    if (tid == 0) M.trace[step] = value;
    if (tid < nw + 2 + (isres ? 1 : 0)) {
      double gr;
      if (tid < nw) {
        if (!M.l.w_broadcast) {
          gr = oscale * (-tot[4 + tid] / wv[tid]) * ffgp_link_der(M.l.w_link, raw[tid], M.l.w_c);
        } else {
          double sg = 0.0;
          for (int k = 0; k < D; ++k) sg += -tot[4 + k] / wv[k];
          gr = oscale * sg * ffgp_link_der(M.l.w_link, raw[0], M.l.w_c);
        }
      } else if (tid == nw) {
        gr = oscale * tot[1] * ffgp_link_der(M.l.amp_link, raw[nw], M.l.amp_c);
      } else if (tid == nw + 1) {
        gr = oscale * tot[2] * ffgp_link_der(M.l.dadd_link, raw[nw + 1], M.l.dadd_c);
      } else {
        gr = oscale * tot[NRED - 1];      // rho (raw = effective)
      }
      const double bc1 = cm.bc[2 * step], bc2s = cm.bc[2 * step + 1];
      ffgp_adam_update(raw + tid, mom + tid, mo2 + tid, gr, cm.lr, cm.b1, cm.b2, cm.eps, bc1, bc2s);
      const double pnew = raw[tid];
      // the next step's effective value (nobody reads wv / sc between the reduction's barrier and the one below)
      if (tid < nw) {
        if (!M.l.w_broadcast) {
          wv[tid] = ffgp_link_val(M.l.w_link, pnew, M.l.w_c);
        } else {
          const double e_ = ffgp_link_val(M.l.w_link, pnew, M.l.w_c);
          for (int k = 0; k < D; ++k) wv[k] = e_;
        }
      } else if (tid == nw) {
        sc[0] = ffgp_link_val(M.l.amp_link, pnew, M.l.amp_c);
      } else if (tid == nw + 1) {
        sc[1] = ffgp_link_val(M.l.dadd_link, pnew, M.l.dadd_c);
      }
    }
    LDS_BARRIER();
  }
  // ---- parameters and moments back to the caller's tensors (a failed step left them as they were when it began)
  const int isres = tr_lds_int(rmode);
  const int npe = nw + 2 + (isres ? 1 : 0);
  if (tid < npe) {
    if (tid < nw) M.w[tid] = raw[tid];
    else if (tid == nw) M.amp[0] = raw[tid];
    else if (tid == nw + 1) M.dadd[0] = raw[tid];
    else {
      tr_lds_ptr(rmode + 6)[0] = raw[tid];
      double* rl = tr_lds_ptr(rmode + 8);
      if (rl) rl[0] = rho0[0];
    }
    M.state[tid] = mom[tid];
    M.state[npe + tid] = mo2[tid];
  }
}

template <int DM>
__global__ __launch_bounds__(TR_T) void ffgp_train_wide_kernel(const WideModel* __restrict__ tab, TrainLoop cm) {
  const WideModel M = tab[blockIdx.x];
  tw_body<DM>(M, cm);
}

// ---- host side ------------------------------------------------------------------------------------------------------
// model f within the kernel's limits (see the head of this file); everything else is refused, never trained another way
static bool tw_member_ok(const ffgp_problem& q, const ffgp_links& l, const ffgp_residual* r, int d_true, long state_stride) {
  const bool res = r && r->rho_dev;
  if (q.n <= 0 || q.n > TR_N || q.D <= 0 || q.D > TR_D) return false;
  if (d_true <= TR_Y || q.d <= 0 || q.d > d_true || q.d > (res ? TW_MAX_COLS_RES : TW_MAX_COLS)) return false;
  if (q.cov_dev || q.pair || q.tree || q.add_mat_dev || q.add_all != 0.0 || q.mean_jitter != 0.0) return false;
  if (!q.X_dev || (!res && !q.Y_dev) || !q.w_dev || !q.amp_dev || !q.diag_add_dev) return false;
  if (q.kfun < FFGP_KFUN_SE || q.kfun > FFGP_KFUN_MATERN52 || q.ll_variant != FFGP_LL_V1) return false;
  if (res && (!r->y_low_dev || !r->y_high_dev || (!r->v_low_dev) != (!r->v_high_dev) ||
              (r->v_low_dev && (r->v_low_stride < 0 || r->v_high_stride < 0))))
    return false;
  if (!res && q.diag_vec_dev && q.diag_stride < 0) return false;
  const int nw = l.w_broadcast ? 1 : q.D;
  return state_stride >= 2 * (nw + 2 + (res ? 1 : 0));
}

extern "C" int ffgp_train_wide_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* l, const ffgp_residual* r, const int* d_true,
                                   int steps, const ffgp_adam* opt, double* state_dev, long state_stride, long step0, double* trace_dev,
                                   long trace_stride, int* info) {
  if (!ffgp_train_args_ok(h, p, l, opt, state_dev, trace_dev, F, steps, step0, trace_stride) || !d_true) return FFGP_ERR_ARG;
  int Dmax = 0;
  for (int f = 0; f < F; ++f) {      // (every member is checked before anything is allocated or enqueued)
    if (!tw_member_ok(p[f], l[f], r ? r + f : nullptr, d_true[f], state_stride)) return FFGP_ERR_ARG;
    Dmax = std::max(Dmax, p[f].D);
  }
  FFGP_HIP(hipSetDevice(h->device));
  // the call's block (train_host.h); the table: F models, the scratch: F x 2 x 36 x 256 (kernel values | A A^T)
  TrainLayout lay;
  const size_t tab_off = lay.take((size_t)F * sizeof(WideModel));
  TrainBlock blk;
  FFGP_CHECK(train_block_open(h, lay, F, steps, opt, step0, (size_t)F * 2 * NBLK_LOWER * 256 * sizeof(double), &blk));
  WideModel* tm = reinterpret_cast<WideModel*>(blk.host + tab_off);
  for (int f = 0; f < F; ++f) {
    const ffgp_problem& q = p[f];
    WideModel& m = tm[f];
    const bool res = r && r[f].rho_dev;
    m.n = q.n; m.D = q.D; m.d = q.d; m.nw = l[f].w_broadcast ? 1 : q.D;
    m.dt = d_true[f];
    m.res = res ? (r[f].v_low_dev ? 2 : 1) : 0;
    m.X = q.X_dev;
    m.ya = res ? r[f].y_high_dev : q.Y_dev;
    m.w = const_cast<double*>(q.w_dev); m.amp = const_cast<double*>(q.amp_dev); m.dadd = const_cast<double*>(q.diag_add_dev);
    if (res) {
      m.yl = r[f].y_low_dev;
      m.vl = r[f].v_low_dev; m.vh = r[f].v_high_dev; m.vl_stride = r[f].v_low_stride; m.vh_stride = r[f].v_high_stride;
      m.rho = r[f].rho_dev; m.rho_last = r[f].rho_last_dev;
    } else {
      m.diag_vec = q.diag_vec_dev; m.diag_stride = q.diag_stride;
    }
    m.l = l[f];
    m.clamp = q.clamp_min; m.rinv = (q.kparam != 0.0) ? 1.0 / q.kparam : 1.0; m.pi_const = q.pi_const; m.kfun = q.kfun;
    m.state = state_dev + (size_t)f * state_stride;
    m.trace = trace_dev + (size_t)f * trace_stride;
    m.kbuf = reinterpret_cast<double*>(blk.dev + blk.scratch_off) + (size_t)f * 2 * NBLK_LOWER * 256;
    m.abuf = m.kbuf + NBLK_LOWER * 256;
  }
  FFGP_HIP(hipMemcpyAsync(blk.dev, blk.host, blk.head, hipMemcpyHostToDevice, h->stream));
  const WideModel* tab = reinterpret_cast<const WideModel*>(blk.dev + tab_off);
  FFGP_CHECK(tr_by_dm(Dmax, [&](auto dm) {
    return train_launch(h, ffgp_train_wide_kernel<dm()>, TW_LDS_DOUBLES * sizeof(double), F, tab, blk.loop);
  }));
  const int rc = train_block_finish(h, blk, F, nullptr);      // (the table is in the caller's order)
  if (info && rc >= 0) {
    const int* st = reinterpret_cast<const int*>(blk.host + blk.info_off);
    for (int f = 0; f < F; ++f) info[f] = st[f];
  }
  return rc;
}
