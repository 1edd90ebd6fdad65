// The posteriors of F small GPs at their own test points in ONE launch: ffgp_predict_small_batch.
// The reference's experiment drivers end with one `gpr(x_train, y_train, x_test)` per fidelity, seed and training size
// (Experiments/GAR_Aligned/exp_aligned.py:63-107, ResGP.py:48-65, AR_autoRegression.py:56-89, CAR_ContinuousAutoRegression.py:94-114); through
// ffgp_predict each of them is an assembly, a factorisation, two solves and the output launches of its own.  Here the grid is (F, S): every
// workgroup runs the stages of the one-launch trainer (train_tile.h) ONCE, in the trainer's order -- links, Sigma into the LDS block image,
// factor + inverse (W = L^-1 in S), Gamma = W Y, A = W^T Gamma -- and then walks its share of the model's tiles of 16 test points:
//
//   K_s [nst * 16][16] into the targets' image (dead once A exists), by the profile functions the trainer's assembly uses
//   mean  = K_s^T A                one MFMA block chain of one wave (K_s as the transposed A operand, A as B)
//   V     = W K_s                  block row w by wave w, never stored: the squares of the accumulators go to vsq[4 w + g][16]
//   var   = k(x, x) - sum_q vsq[q][c] (q ascending) [+ the noise]
//
// The S workgroups of one model each factor it themselves (sixteen models are sixteen workgroups on 256 CUs: the chip is otherwise
// idle); workgroup s takes tiles s, s + S, ...: no cross-workgroup traffic, no atomics.  A test point is ONE column of the 16-column
// images: every sum that forms its mean and variance runs over the training points in an order fixed by the model's size alone, so the
// results do not depend on S, on the point's tile or on the other points, bit for bit.
// A member whose Sigma is not positive definite stops alone: NaN outputs, its status word set by its workgroup 0.
#include "predict_small.h"

struct PredictModel {
  int n, D, d;
  const double* X; const double* Y;
  const double* w; const double* amp; const double* dadd;      // raw parameters (effective ones under identity links)
  ffgp_links l;
  double clamp, rinv;
  int kfun;
  const double* Xs; int nt;
  double* mean; double* var;
  int add_noise;
};

// LDS (doubles): the shared head of train_tile.h (S | Xs | Ym, Gam, Am | piv | dvec) | wv [16] | sc [8] | flags [8] | xt [16][17] | vsq [32][16]
#define PS_OFF_WV TR_OFF_TAIL
#define PS_OFF_SC (PS_OFF_WV + 16)
#define PS_OFF_FLAGS (PS_OFF_SC + 8)
#define PS_OFF_XT (PS_OFF_FLAGS + 8)
#define PS_OFF_VSQ (PS_OFF_XT + 16 * (TR_D + 1))
#define PS_LDS_DOUBLES (PS_OFF_VSQ + 32 * 16)
static_assert(PS_LDS_DOUBLES * sizeof(double) <= 160 * 1024, "the predict launch's LDS exceeds a CU's 160 KiB");
#define PS_NOPROF(k) (void)0

// DM: the input dimensions the per-entry loops are unrolled for (8 or 16: every model of the launch has D <= DM)
template <int DM>
__global__ __launch_bounds__(TR_T) void ffgp_predict_small_kernel(const PredictModel* __restrict__ tab, int* __restrict__ info) {
  const PredictModel M = tab[blockIdx.x];
  const int nt = M.nt, ntile = (nt + 15) >> 4;
  if ((int)blockIdx.y >= ntile) return;      // (uniform: this model has fewer tiles than the call's largest)
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* S = lds;
  double* Xs = lds + TR_OFF_XS;
  double* Ym = lds + TR_OFF_YM;            // the targets, then K_s of the current tile
  double* Gam = lds + TR_OFF_GAM;
  double* Am = lds + TR_OFF_AM;
  double* piv = lds + TR_OFF_PIV;
  double* wv = lds + PS_OFF_WV;            // [16] effective inverse length scales
  double* sc = lds + PS_OFF_SC;            // amp, dadd, the noise added to the variance
  int* flags = reinterpret_cast<int*>(lds + PS_OFF_FLAGS);      // [0] bad pivot; [8..15] the waves' SIMDs
  double* xt = lds + PS_OFF_XT;            // [16][17] the tile's scaled test points
  double* vsq = lds + PS_OFF_VSQ;          // [4 nst][16] partial column sums of V^2
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int n = M.n, D = M.D, d = M.d;
  const int nst = (n + 15) >> 4, nblk = nst * (nst + 1) / 2;
  ExpCoef ec;
  ffgp_exp_load(ec);

  // ---- once: the trainer's set-up.  Targets, Gamma and A as [128][16] images, zero beyond (n, d); identity in the blocks the factorisation never touches
  for (int idx = tid; idx < TR_N * TR_Y; idx += TR_T) {
    const int i = idx >> 4, q = idx & 15;
    Ym[idx] = (i < n && q < d) ? M.Y[i * d + q] : 0.0;
    Gam[idx] = 0.0;
    Am[idx] = 0.0;
  }
  for (int idx = tid; idx < TR_N * (TR_D + 1); idx += TR_T) Xs[idx] = 0.0;
  for (int t = wave; t < NBLK_LOWER; t += 8) {
    int bi, bj;
    blk_unrank(t, bi, bj);
    if (bi < nst) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) S[blk_off(bi, bj) + (g + 4 * r) * BLD + c] = (bi == bj && g + 4 * r == c) ? 1.0 : 0.0;
  }
  if (tid == 0) flags[0] = 0;
  if (lane == 0) flags[8 + wave] = wave_simd(wave);
  if (tid < D) wv[tid] = ffgp_link_val(M.l.w_link, M.w[M.l.w_broadcast ? 0 : tid], M.l.w_c);
  if (tid == 64) sc[0] = ffgp_link_val(M.l.amp_link, M.amp[0], M.l.amp_c);
  if (tid == 65) {
    sc[1] = M.dadd ? ffgp_link_val(M.l.dadd_link, M.dadd[0], M.l.dadd_c) : 0.0;
    sc[2] = (M.dadd && M.add_noise) ? ffgp_link_val(M.l.dadd_link, M.dadd[0], 0.0) : 0.0;
  }
  __syncthreads();
  int hidx, nh;
  helper_roles(flags + 8, lane, wave, hidx, nh);
  for (int idx = tid; idx < n * D; idx += TR_T) {      // scaled inputs, shifted by the first point: only differences enter the kernel
    const int i = idx / D, k = idx - i * D;
    Xs[i * (TR_D + 1) + k] = (M.X[idx] - M.X[k]) * wv[k];
  }
  LDS_BARRIER();
  const double amp = sc[0], dadd = sc[1], noise = sc[2];

  // ---- Sigma, lower block triangle (diagonal blocks symmetric-full), identity beyond n: the trainer's assembly without its parked values
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
      double kv = amp * ev;
      if (i == j) kv += dadd;
      if (i >= n || j >= n) kv = (i == j) ? 1.0 : 0.0;
      dst[(g + 4 * r) * BLD + c] = kv;
    }
  }
  LDS_BARRIER();

  // ---- blocked Cholesky AND the inverse (train_tile.h); a Sigma that is not positive definite ends this member here
  TR_FACTOR_STAGES(S, piv, flags, n, nst, lane, wave, g, c, hidx, nh, PS_NOPROF)
  if (flags[0] != 0) {      // (uniform: every thread reads the same word behind the barrier)
    if (tid == 0 && blockIdx.y == 0) info[blockIdx.x] = flags[0];
    for (int tile = blockIdx.y; tile < ntile; tile += gridDim.y) {
      const int p0 = tile * 16, np = min(16, nt - p0);
      for (int idx = tid; idx < np * d; idx += TR_T) M.mean[(size_t)p0 * d + idx] = __builtin_nan("");
      if (tid < np) M.var[p0 + tid] = __builtin_nan("");
    }
    return;
  }
  tr_inverse_last_row(S, nst, lane, wave, g, c);
  tr_gamma_rows(S, Ym, Gam, nst, lane, wave, g, c);
  LDS_BARRIER();
  {
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    tr_alpha_rows(S, Gam, Am, nst, lane, wave, g, c, acc);
  }
  LDS_BARRIER();

  // ---- this workgroup's tiles of 16 test points
  double* Ks = Ym;
  const double kss = amp * ((M.kfun == FFGP_KFUN_SE) ? ffgp_exp_fast(-0.5 * fmax(0.0, M.clamp), ec) : ffgp_kfun_val(M.kfun, M.rinv, fmax(0.0, M.clamp)));
  const int mean_wave = (nst < 8) ? 7 : 0;      // (a wave without a block row of V when there is one)
  for (int tile = blockIdx.y; tile < ntile; tile += gridDim.y) {
    const int p0 = tile * 16;
    for (int idx = tid; idx < 16 * (TR_D + 1); idx += TR_T) {      // columns beyond nt repeat the last point (never stored)
      const int cc = idx / (TR_D + 1), k = idx - cc * (TR_D + 1);
      const int p = min(p0 + cc, nt - 1);
      xt[idx] = (k < D) ? (M.Xs[(size_t)p * D + k] - M.X[k]) * wv[k] : 0.0;
    }
    LDS_BARRIER();
    {      // K_s: thread (i0 = tid / 16, c) forms rows i0, i0 + 32, ... of column c; zero rows from n up to the last block's end
      const int cc = tid & 15, i0 = tid >> 4;
      double xj[DM];
#pragma unroll
      for (int k = 0; k < DM; ++k) xj[k] = xt[cc * (TR_D + 1) + k];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 32 * r;
        if (i >= nst * 16) continue;
        const double* xi = Xs + i * (TR_D + 1);
        double sq = 0.0;
#pragma unroll
        for (int k = 0; k < DM; ++k) {
          const double df = xi[k] - xj[k];
          sq = __builtin_fma(df, df, sq);
        }
        const double s_ = fmax(sq, M.clamp);
        const double ev = (M.kfun == FFGP_KFUN_SE) ? ffgp_exp_fast(-0.5 * s_, ec) : ffgp_kfun_val(M.kfun, M.rinv, s_);
        Ks[i * TR_Y + cc] = (i < n) ? amp * ev : 0.0;
      }
    }
    LDS_BARRIER();
    if (wave < nst) {      // block row `wave` of V = W K_s (wave + 1 products), consumed in its accumulators
      d4_t acc = {0.0, 0.0, 0.0, 0.0};
      tr_chain<false>(acc, 0, wave + 1, S + blk_off(wave, 0), [](int kb) { return kb * BLKSZ; }, BLD, Ks, [](int kb) { return kb * 16 * TR_Y; }, TR_Y,
                      lane);
      double s_ = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) s_ = __builtin_fma(acc[r], acc[r], s_);
      vsq[(wave * 4 + g) * 16 + c] = s_;
    }
    if (wave == mean_wave) {      // mean = K_s^T A: entry (point g + 4 r, column c)
      d4_t acc = {0.0, 0.0, 0.0, 0.0};
      tr_chain<true>(acc, 0, nst, Ks, [](int kb) { return kb * 16 * TR_Y; }, TR_Y, Am, [](int kb) { return kb * 16 * TR_Y; }, TR_Y, lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = p0 + g + 4 * r;
        if (p < nt && c < d) M.mean[(size_t)p * d + c] = acc[r];
      }
    }
    LDS_BARRIER();
    if (tid < 16 && p0 + tid < nt) {      // the column's partial sums in one fixed order
      double s_ = 0.0;
      for (int q = 0; q < 4 * nst; ++q) s_ += vsq[q * 16 + tid];
      M.var[p0 + tid] = kss - s_ + noise;
    }
  }
}

static bool ps_member_ok(const ffgp_problem& q, const ffgp_predict_member& m) {
  if (!ps_sizes_ok(q, m)) return false;
  if (q.cov_dev || q.pair || q.tree || q.add_mat_dev || q.diag_vec_dev || q.add_all != 0.0 || q.mean_jitter != 0.0) return false;
  if (!q.X_dev || !q.Y_dev || !q.w_dev || !q.amp_dev) return false;
  if (q.kfun < FFGP_KFUN_SE || q.kfun > FFGP_KFUN_RQ) return false;
  return true;
}

extern "C" int ffgp_predict_small_batch(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* l, const ffgp_predict_member* m, int* status) {
  if (!h || !p || !m || F < 1 || F > FFGP_PREDICT_SMALL_MAX_F) return FFGP_ERR_ARG;
  int Dmax = 0, tiles = 1;
  for (int f = 0; f < F; ++f) {      // (every member is checked before anything is allocated or enqueued)
    if (!ps_member_ok(p[f], m[f])) return FFGP_ERR_ARG;
    Dmax = std::max(Dmax, p[f].D);
    tiles = std::max(tiles, (m[f].nt + 15) / 16);
  }
  const int split = ps_split(F, tiles);
  FFGP_HIP(hipSetDevice(h->device));
  // the call's block (train_host.h): the table of F models and the status words; no steps, no scratch
  TrainLayout lay;
  const size_t tab_off = lay.take((size_t)F * sizeof(PredictModel));
  TrainBlock blk;
  const ffgp_adam no_opt = {0.0, 0.0, 0.0, 0.0};
  FFGP_CHECK(train_block_open(h, lay, F, 0, &no_opt, 0, 0, &blk));
  PredictModel* tm = reinterpret_cast<PredictModel*>(blk.host + tab_off);
  for (int f = 0; f < F; ++f) {
    const ffgp_problem& q = p[f];
    PredictModel& t = tm[f];
    t.n = q.n; t.D = q.D; t.d = q.d;
    t.X = q.X_dev; t.Y = q.Y_dev;
    t.w = q.w_dev; t.amp = q.amp_dev; t.dadd = q.diag_add_dev;
    if (l) {
      t.l = l[f];
    } else {      // effective parameters: identity links
      memset(&t.l, 0, sizeof(t.l));
      t.l.w_link = t.l.amp_link = t.l.dadd_link = FFGP_LINK_ID;
    }
    t.clamp = q.clamp_min; t.rinv = (q.kparam != 0.0) ? 1.0 / q.kparam : 1.0; t.kfun = q.kfun;
    t.Xs = m[f].Xs_dev; t.nt = m[f].nt;
    t.mean = m[f].mean_dev; t.var = m[f].var_dev;
    t.add_noise = m[f].var_add_noise;
  }
  FFGP_HIP(hipMemcpyAsync(blk.dev, blk.host, blk.head, hipMemcpyHostToDevice, h->stream));
  const PredictModel* tab = reinterpret_cast<const PredictModel*>(blk.dev + tab_off);
  int* info = blk.loop.info;
  const size_t lds_bytes = PS_LDS_DOUBLES * sizeof(double);
  FFGP_CHECK(tr_by_dm(Dmax, [&](auto dm) -> int {
    auto kernel = ffgp_predict_small_kernel<dm()>;
    FFGP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    hipLaunchKernelGGL(kernel, dim3(F, split), dim3(TR_T), lds_bytes, h->stream, tab, info);
    return hipGetLastError() == hipSuccess ? FFGP_OK : FFGP_ERR_HIP;
  }));
  return ps_finish(h, blk, F, status);
}
