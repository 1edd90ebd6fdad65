// One workgroup, one small GP: K Adam steps of F models in ONE launch, and the per-step likelihood + gradient call (round 6).
// The reference's hot loop runs at the sizes of its experiments (FidelityFusion_Models/ResGP.py:78-112, GaussianProcess/cigp_v10.py:92-104:
// per fidelity 100-1000 iterations of zero_grad / loss = -negative_log_likelihood / backward / Adam step at N = 16 ... 128;
// Experiments/GAR_Aligned/exp_aligned.py:66-74: 100 low- against 4..32 high-fidelity points).  ffgp_train_raw used to enqueue 13 dependent
// launches per step at n = 128 (0.096 ms per step, two thirds of it launch floors).  Here one PERSISTENT workgroup per model
// (gridDim.x = models, 512 threads) runs every step inside the kernel:
//
//   links (raw -> effective parameters)  ->  Sigma assembled straight into LDS as 16 x 16 blocks [16][17] (lower block triangle, 78 KiB),
//       the kernel values parked in a global scratch for the gradient pass
//   ->  blocked Cholesky AND inverse, two workgroup barriers per 16-column stage: wave 0 factors + inverts the diagonal block in
//       registers on the DP-ALU DPP pivot step of f16_steps.h while the helper waves apply the previous column and form the previous row
//       of the inverse; then all eight waves solve the column.  Only ceil(n / 16) stages run: n = 32 costs a quarter of n = 128.
//       (This loop became the factorisation's diagonal-block kernel, ffgp_potrf_diag128_v4 in potrf.hip; the two share diag_block.h.)
//   ->  Gamma = L^-1 Y, A = L^-T Gamma as MFMA block chains on zero-padded [128][16] images, the value
//   ->  Sigma^-1 = L^-T L^-1 block by block on the matrix cores, each 16 x 16 block consumed in its accumulators: G = d/2 Sigma^-1 - 1/2 A A^T,
//       the gradient sums of grad.hip (amplitude, length scales, trace) -- Sigma^-1 is never stored
//   ->  one workgroup reduction, the links' chain rule and torch.optim.Adam's update (operation for operation as ffgp_adam_kernel) on
//       parameters and moments that live in LDS for the whole call; the step's loss goes to the trace.
// A Sigma that is not positive definite stops THAT model at that step (its status word, NaN in its trace from there on, parameters as
// they were when the step began); the other models of the launch train on.
// EVALUATE mode (tr_body<DM, false>, ffgp_small_mfma_kernel): the same pass once, without Adam -- value, raw-parameter gradients, dL/dY and
// diag G written out -- for ffgp_nlml_fused_small_batch and ffgp_nlml_fused_raw at n <= 128.
// RESIDUAL members (tr_body<DM, true, true>, ffgp_train_resid_kernel; train_AR's fidelities above 0, AR_autoRegression.py:123-137):
// the targets are r = y_high - rho y_low and the diagonal extra |v_high,ii - rho v_low,ii|, re-formed at every step from a learnable rho
// that lives in LDS beside the other raw parameters; dloss/drho = -sum A .* y_low - sum_i G_ii sgn(s_i) v_low,ii is one more total of
// the step's reduction and rho is a fourth Adam parameter.  y_low / y_high are read from global memory (no room for two more [128][16]
// images), the two diagonals sit in LDS.  Plain members may share the launch: the residual code is skipped for them.
// V2 members (tr_body<DM, true, false, true>, ffgp_train_v2_kernel; GP_basic's likelihood, GaussianProcess/gp_basic.py:130-143): the value is
// 1/2 |A|^2 + d sum log L_ii + 1/2 n d log(2 pi) with A = Sigma^-1 Y, so the step needs B = Sigma^-1 A as well: G = d/2 Sigma^-1 -
// 1/2 (A B^T + B A^T).  There is no room for a fourth [128][16] image: L^-1 A goes over Gamma, B over the targets, and Y is read
// again from global memory at the start of every step.  V1 and V2 members of one call are launched separately.
// CAR members (tr_body<DM, true, false, V2, true>, ffgp_train_car_kernel; train_CAR's fidelities above 0, CAR_ContinuousAutoRegression.py:
// 116-142): the targets r = y_high - exp(b) y_low and the effective amplitude link(amp_raw) * s(b, l_z, sigma_z) -- the Monte-Carlo fidelity
// integral, car_scale_wave in train_tile.h -- are re-formed at every step; b, l_z, sigma_z are three more Adam parameters, kept with their
// moments, the samples and the partials of s behind the reduction's extra total (dloss/db needs sum dloss/dr .* y_low).  Launches of their own.
// TENSOR-LINEAR members (tr_body<DM, true, false, false, false, true>, ffgp_train_tlin_kernel; train_CIGAR's fidelities above 0, CIGAR.py:116-133):
// the targets are R = y_high - y_low V^T with V [h, l] (h = d <= 16, l <= h) the map's matrix, re-formed at every step into the zero-padded
// target image; V, its two moments, dloss/dV = -A^T y_low and V as the step began stay in LDS for the whole call (5 x 256 doubles) and V's
// h l entries are Adam parameters nw + 2 ... of the member.  The diagonal extra |diag(v_high) - diag(v_low)| is constant -- the member's
// diag_vec -- so none of the residual class's four [128] arrays is needed; y_low / y_high are read from global memory.  Launches of their own.
// Covers: n <= 128, D <= 16, d <= 16, one radial-profile kernel, V1 likelihood (V2: plain and CAR members), diag_add and diag_vec (no matrix / all-entries /
// mean(K) extras, no learnable profile parameter): what cigp_v10 produces.  Everything else keeps the paths it had.
// HOST side: the scaffold of train_host.h, shared with train_tree_lds.hip -- the call's block on the handle with its pinned mirror, the
// bias corrections, the loop's arguments, the <8> / <16> dispatch, the launch, the status epilogue.  ffgp_train_persist adds what is its
// own: the four classes of members, their tables, a launch per class.  The links and Adam's update are the copies of drivers.h.
#include "train_host.h"

#define TR_NRED 20        // values of the step's one workgroup reduction: ss, s_amp, tr G, log-det, tot[16]

struct TrainModel {
  int n, D, d, nw;                       // nw: raw length scales (1 = one value broadcast over the D dimensions)
  const double* X; const double* Y;
  double* w; double* amp; double* dadd;  // RAW parameters, updated in place when the kernel ends
  const double* diag_vec; long diag_stride;
  ffgp_links l;
  double clamp, rinv, pi_const;
  int kfun;
  double* state;                         // [exp_avg (nw + 2) | exp_avg_sq (nw + 2)]
  double* trace;                         // [steps]
  // evaluate mode (one likelihood + gradient call, no Adam: ffgp_nlml_fused_small_batch / ffgp_nlml_fused_raw at n <= 128)
  double* nll;                           // [1] value
  double* g_w; double* g_amp; double* g_dadd; double* g_Y; double* g_dvec;   // gradients (raw parameters, Y, diag_vec); any may be null
  int want_grad;
  double* kbuf;                          // [36][4][64] this model's kernel values K / amp, written by the assembly and read back by the
                                         // gradient pass of the same step (same lane, same slot: the exp is evaluated once per entry and step)
};
// a residual member's link (ffgp_residual): rho == nullptr is a plain model
struct TrainResid {
  double* rho;                           // [1] RAW rho, updated in place when the kernel ends
  const double* yl; const double* yh;    // [n, d]
  const double* vl; const double* vh;    // optional diagonals: entry i at vl[i * vl_stride], vh[i * vh_stride] (both or neither)
  long vl_stride, vh_stride;
  double* rho_last;                      // optional [1]: rho at the start of the last step taken
};
// a CAR member's link (ffgp_car_link): every member of a CAR launch has one
struct TrainCar {
  double* b; double* zls; double* zamp;  // [1] each, RAW, updated in place when the kernel ends
  double zeps, lf, hf;
  const float* z1; const float* z2; int nz;
  const double* z1d; const double* z2d;  // the samples as fp64 draws (then z1 / z2 are not read)
  const double* yl; const double* yh;    // [n, d]
  double* b_last;                        // optional [1]: b at the start of the last step taken
};
// a tensor-linear member's link (ffgp_tlin_link): every member of a tensor-linear launch has one
struct TrainTlin {
  double* V; long rs, cs;                // [h, l] RAW, element (a, b) at V[a * rs + b * cs], updated in place when the kernel ends
  int l;
  const double* yl; const double* yh;    // [n, l], [n, h]
  double* V_last;                        // optional [h, l] row-major: V at the start of the last step taken
};
struct TrainCommon : TrainLoop {         // (the loop's arguments first: the layout the kernels were compiled against)
  int* shared_info;                      // evaluate mode: the handle's status word (batch: atomicMax of the failing pivot; single: plain store)
  int info_max;
  long* prof;                            // development (FFGP_TRAIN_TRACE=1): [12] wall_clock64 ticks per phase, summed over model 0's steps
};
#define TR_PROF(k)                                                   \
  do {                                                               \
    if (cm.prof && tid == 0 && blockIdx.x == 0) {                    \
      const long now_ = wall_clock64();                              \
      cm.prof[k] += now_ - t_prof;                                   \
      t_prof = now_;                                                 \
    }                                                                \
  } while (0)

// LDS (doubles): the shared head of train_tile.h (S | Xs | Ym, Gam, Am | piv | dvec) | small
#define TR_OFF_SMALL TR_OFF_TAIL
#define TR_SMALL_DOUBLES (16 + 3 * 20 + 8 + 8 * TR_NRED + TR_NRED + 16)
#define TR_LDS_DOUBLES (TR_OFF_SMALL + TR_SMALL_DOUBLES)
// residual launches: the reduction has one more total (dloss/drho), then vl | vh | sgv = sgn(s) vl | diag G [128] each, rsum [8] (per-wave
// sums of A .* y_low), rho at the start of the step [1]
#define TR_NRED_RES (TR_NRED + 1)
#define TR_OFF_RES (TR_OFF_SMALL + TR_SMALL_DOUBLES + 9 * (TR_NRED_RES - TR_NRED))
#define TR_LDS_DOUBLES_RES (TR_OFF_RES + 4 * TR_N + 16)
static_assert(TR_LDS_DOUBLES_RES * sizeof(double) <= 160 * 1024, "the residual launch's LDS exceeds a CU's 160 KiB");
// CAR launches: the reduction has one more total as well (sum dloss/dr .* y_low), then z1 | z2 [128] each (fp32 draws widened, or fp64 draws),
// b, l_z, sigma_z with their moments [4] x 3 (raw / mom / mo2 have no room for nw + 5 parameters), s and its partials, b at the start of
// the step and zeps, lf, hf [8], rsum [8], the parked words [8]: y_low, y_high, b, l_z, sigma_z, b_last, nz, the samples' format
#define TR_OFF_CAR TR_OFF_RES
#define TR_LDS_DOUBLES_CAR (TR_OFF_CAR + 2 * TR_N + 12 + 8 + 8 + 8)
static_assert(TR_LDS_DOUBLES_CAR * sizeof(double) <= 160 * 1024, "the CAR launch's LDS exceeds a CU's 160 KiB");

// tensor-linear launches: V | exp_avg | exp_avg_sq | dV | V at the start of the step, [16 x 16] each, row-major [h][l]; the parked words [8]:
// y_low, y_high (read through tr_lds_ptr), l
#define TR_OFF_TLIN TR_OFF_RES
#define TR_LDS_DOUBLES_TLIN (TR_OFF_TLIN + 5 * TR_Y * TR_Y + 8)
static_assert(TR_LDS_DOUBLES_TLIN * sizeof(double) <= 160 * 1024, "the tensor-linear launch's LDS exceeds a CU's 160 KiB");

// DM: the input dimensions the per-entry loops are unrolled for (8 or 16: every model of the launch has D <= DM)
// TRAIN: every step of the loop with Adam inside; !TRAIN ("evaluate"): ONE pass that writes the value and the gradients out
// RESID (with TRAIN only): members with R.rho set are residual models (see the head of this file)
// V2 (with TRAIN, without RESID): the FFGP_LL_V2 likelihood of GP_basic (see the head of this file)
// CAR (with TRAIN, without RESID): every member is a CAR member (see the head of this file)
// TLIN (with TRAIN alone): every member is a tensor-linear member (see the head of this file)
template <int DM, bool TRAIN, bool RESID = false, bool V2 = false, bool CAR = false, bool TLIN = false>
__device__ __forceinline__ void tr_body(const TrainModel& M, const TrainCommon& cm, const TrainResid* Rp = nullptr, const TrainCar* Cp = nullptr,
                                        const TrainTlin* Tp = nullptr) {
  static_assert(!TLIN || (TRAIN && !RESID && !V2 && !CAR), "tensor-linear members train on the V1 likelihood, in launches of their own");
  static_assert(TRAIN || !RESID, "residual members train");
  static_assert(!V2 || (TRAIN && !RESID), "the V2 likelihood: plain and CAR members of the training loop");
  static_assert(!CAR || (TRAIN && !RESID), "CAR members train, in launches of their own");
  constexpr int NRED = (RESID || CAR) ? TR_NRED_RES : TR_NRED;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* S = lds;
  double* Xs = lds + TR_OFF_XS;
  double* Ym = lds + TR_OFF_YM;
  double* Gam = lds + TR_OFF_GAM;
  double* Am = lds + TR_OFF_AM;
  double* piv = lds + TR_OFF_PIV;
  double* dvec = lds + TR_OFF_DVEC;
  double* wv = lds + TR_OFF_SMALL;         // [16] effective inverse length scales
  double* raw = wv + 16;                   // [20] raw parameters: w (nw) | amp | dadd
  double* mom = raw + 20;                  // [20] exp_avg
  double* mo2 = mom + 20;                  // [20] exp_avg_sq
  double* sc = mo2 + 20;                   // [8]  amp, dadd, logdet
  double* red = sc + 8;                    // [8][NRED] per-wave partial sums
  double* tot = red + 8 * NRED;            // [NRED] the step's totals
  int* flags = reinterpret_cast<int*>(tot + NRED);        // [0] bad pivot of the current step
  double* rvl = lds + TR_OFF_RES;          // residual members: [128] v_low diagonal
  double* rvh = rvl + TR_N;                // [128] v_high diagonal
  double* sgv = rvh + TR_N;                // [128] sgn(s_i) v_low,ii of the current step
  double* gdg = sgv + TR_N;                // [128] G_ii of the current step
  double* rsum = gdg + TR_N;               // [8]   per-wave sums of A .* y_low
  double* rho0 = rsum + 8;                 // [1]   rho at the start of the current step
  int* rmode = reinterpret_cast<int*>(rho0 + 1);      // [0] 0 plain member, 1 residual, 2 residual with diagonals; [2..9] y_low, y_high,
                                                      // rho, rho_last (read through tr_lds_int / tr_lds_ptr)
  double* zs = lds + TR_OFF_CAR;           // CAR members: z1 [128] | z2 [128]
  double* craw = zs + 2 * TR_N;            // [4] raw b, l_z, sigma_z (parameters nw + 2 .. nw + 4)
  double* cmom = craw + 4;                 // [4] their exp_avg
  double* cmo2 = cmom + 4;                 // [4] their exp_avg_sq
  double* cs = cmo2 + 4;                   // [8] s, ds/db, ds/dl_z, ds/dsigma_z of the current step, b at its start; zeps, lf, hf
  double* ceb = cmo2 + 3;                  // [1] exp(b) of the current step (the fourth slot of cmo2)
  double* csum = cs + 8;                   // [8] per-wave sums of dloss/dr .* y_low
  int* cptr = reinterpret_cast<int*>(csum + 8);       // [0..11] y_low, y_high, b, l_z, sigma_z, b_last (read through tr_lds_ptr); [12] nz,
                                                      // [13] 1: fp32 draws (the link is not read again after the set-up)
  double* tV = lds + TR_OFF_TLIN;          // tensor-linear members: [h][l] V
  double* tmV = tV + TR_Y * TR_Y;          // its exp_avg
  double* tvV = tmV + TR_Y * TR_Y;         // its exp_avg_sq
  double* tdV = tvV + TR_Y * TR_Y;         // dloss/dV of the current step (before the output scale)
  double* tV0 = tdV + TR_Y * TR_Y;         // V at the start of the current step
  int* tptr = reinterpret_cast<int*>(tV0 + TR_Y * TR_Y);      // [0..3] y_low, y_high (read through tr_lds_ptr); [4] l
  bool isres = RESID && Rp->rho != nullptr;           // (for the set-up only: the step loop reads rmode)
  bool hasv = isres && Rp->vl != nullptr;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int n = M.n, D = M.D, d = M.d, nw = M.nw;
  const int nst = (n + 15) >> 4, nblk = nst * (nst + 1) / 2;
  const int npar = nw + 2 + (isres ? 1 : 0) + (CAR ? 3 : 0);      // (a residual member's rho is raw[nw + 2]; a CAR member's three: craw)
  const double oscale = (M.l.out_scale != 0.0) ? M.l.out_scale : 1.0;
  ExpCoef ec;
  ffgp_exp_load(ec);

  // ---- once: targets, the diagonal extra, parameters and moments into LDS; identity padding of the blocks the factorisation never touches
  // targets, Gamma and A live as [128][16] images, zero beyond (n, d): the matrix-core products read them without guards
  for (int idx = tid; idx < TR_N * TR_Y; idx += TR_T) {
    const int i = idx >> 4, q = idx & 15;
    Ym[idx] = (!CAR && !TLIN && !isres && i < n && q < d) ? M.Y[i * d + q] : 0.0;      // (a residual, CAR or tensor-linear member's are formed at every step)
    Gam[idx] = 0.0;
    Am[idx] = 0.0;
  }
  for (int idx = tid; idx < TR_N * (TR_D + 1); idx += TR_T) Xs[idx] = 0.0;      // (columns >= D and rows >= n stay zero: the unrolled loops read them)
  if (!isres) {
    for (int i = tid; i < TR_N; i += TR_T) dvec[i] = (M.diag_vec && i < n) ? M.diag_vec[(size_t)i * M.diag_stride] : 0.0;
  } else {      // (formed at every step from rho; zero beyond n and without diagonals)
    for (int i = tid; i < TR_N; i += TR_T) {
      dvec[i] = 0.0;
      sgv[i] = 0.0;
      gdg[i] = 0.0;
      rvl[i] = (hasv && i < n) ? Rp->vl[(size_t)i * Rp->vl_stride] : 0.0;
      rvh[i] = (hasv && i < n) ? Rp->vh[(size_t)i * Rp->vh_stride] : 0.0;
    }
  }
  if (tid < npar) {
    if (CAR && tid >= nw + 2) {
      const int k = tid - nw - 2;
      craw[k] = (k == 0) ? Cp->b[0] : ((k == 1) ? Cp->zls[0] : Cp->zamp[0]);
      cmom[k] = M.state[tid];
      cmo2[k] = M.state[npar + tid];
      if (k == 0) ceb[0] = exp(craw[0]);
    } else {
      if (isres && tid == nw + 2) raw[tid] = Rp->rho[0];
      else raw[tid] = (tid < nw) ? M.w[tid] : (tid == nw ? M.amp[0] : (M.dadd ? M.dadd[0] : 0.0));
      if (TRAIN) {
        mom[tid] = M.state[tid];
        mo2[tid] = M.state[npar + (TLIN ? d * Tp->l : 0) + tid];      // (a tensor-linear member: [exp_avg (P) | exp_avg_sq (P)], P = nw + 2 + h l)
      }
    }
  }
  if constexpr (TLIN) {
    const int tl_ = Tp->l, hl = d * tl_;
    if (tid < hl) {      // V through its strides into the row-major image; its moments behind the three parameters'
      tV[tid] = Tp->V[(tid / tl_) * Tp->rs + (tid % tl_) * Tp->cs];
      tmV[tid] = M.state[nw + 2 + tid];
      tvV[tid] = M.state[nw + 2 + hl + nw + 2 + tid];
    }
    if (tid == 0) {
      const double* pv[2] = {Tp->yl, Tp->yh};
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const unsigned long long u = reinterpret_cast<unsigned long long>(pv[k]);
        tptr[2 * k] = (int)(unsigned)u;
        tptr[2 * k + 1] = (int)(unsigned)(u >> 32);
      }
      tptr[4] = tl_;
    }
  }
  if constexpr (CAR) {
    if (tid < 2 * TR_N) {      // the samples, zero beyond nz (never read there)
      const int k = tid & (TR_N - 1);
      if (Cp->z1d) zs[tid] = (k < Cp->nz) ? ((tid < TR_N) ? Cp->z1d[k] : Cp->z2d[k]) : 0.0;
      else zs[tid] = (k < Cp->nz) ? (double)((tid < TR_N) ? Cp->z1[k] : Cp->z2[k]) : 0.0;
    }
    if (tid == 0) {
      const double* pv[6] = {Cp->yl, Cp->yh, Cp->b, Cp->zls, Cp->zamp, Cp->b_last};
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const unsigned long long u = reinterpret_cast<unsigned long long>(pv[k]);
        cptr[2 * k] = (int)(unsigned)u;
        cptr[2 * k + 1] = (int)(unsigned)(u >> 32);
      }
      cptr[12] = Cp->nz;
      cptr[13] = Cp->z1d == nullptr ? 1 : 0;
      cs[5] = Cp->zeps; cs[6] = Cp->lf; cs[7] = Cp->hf;
    }
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
  if (RESID && tid == 0) {
    rmode[0] = hasv ? 2 : (isres ? 1 : 0);
    const double* pv[4] = {isres ? Rp->yl : nullptr, isres ? Rp->yh : nullptr, Rp->rho, Rp->rho_last};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned long long u = reinterpret_cast<unsigned long long>(pv[k]);
      rmode[2 + 2 * k] = (int)(unsigned)u;
      rmode[3 + 2 * k] = (int)(unsigned)(u >> 32);
    }
  }
  __syncthreads();
  HELPER_ROLES(flags + 8, wave, hidx, nh);      // helpers of the factorisation's stage [A]
  ROLES_SEEN(lane, wave, hidx, nh);
  if (tid < D) wv[tid] = ffgp_link_val(M.l.w_link, raw[M.l.w_broadcast ? 0 : tid], M.l.w_c);
  if (tid == 64) sc[0] = ffgp_link_val(M.l.amp_link, raw[nw], M.l.amp_c);
  if (tid == 65) sc[1] = M.dadd ? ffgp_link_val(M.l.dadd_link, raw[nw + 1], M.l.dadd_c) : 0.0;
  __syncthreads();

  int failed = 0;
  long t_prof = cm.prof ? wall_clock64() : 0;
  const int nsteps = TRAIN ? cm.steps : 1;
  const int lane_k = lane, wave_k = wave;
  for (int step = 0; step < nsteps; ++step) {
    // (the lane coordinates opaque per iteration: otherwise every per-lane offset of every phase is hoisted out of the step loop and kept
    //  alive across it -- 256 registers and 79 spilled ones, reloaded inside the phases)
    int lane = lane_k, wave = wave_k;
    asm volatile("" : "+v"(lane), "+s"(wave));
    const int g = lane >> 4, c = lane & 15;
    // ---- P0: scaled inputs (the effective parameters were refreshed by the threads that updated the raw ones)
    for (int idx = tid; idx < n * D; idx += TR_T) {      // (shifted by the first point: only differences enter the kernel)
      const int i = idx / D, k = idx - i * D;
      Xs[i * (TR_D + 1) + k] = (M.X[idx] - M.X[k]) * wv[k];
    }
    if constexpr (V2 && !CAR) {      // (B took the targets' image in the previous step: Y again from global memory, as residual members re-form theirs)
      for (int idx = tid; idx < n * TR_Y; idx += TR_T) {
        const int i = idx >> 4, q = idx & 15;
        if (q < d) Ym[idx] = M.Y[i * d + q];
      }
    }
    if constexpr (CAR) {      // this step's targets r = y_high - exp(b) y_low (a product, then a difference: never contracted), and by wave 1 the
                              // fidelity integral s with its partials: the effective amplitude link(amp_raw) * s
      const double* yl = tr_lds_ptr(cptr);
      const double* yh = tr_lds_ptr(cptr + 2);
      const double eb = ceb[0];      // exp(b), refreshed by the thread that updated b
      for (int idx = tid; idx < n * TR_Y; idx += TR_T) {
        const int i = idx >> 4, q = idx & 15;
        if (q < d) Ym[idx] = __dsub_rn(yh[i * d + q], __dmul_rn(eb, yl[i * d + q]));
      }
      if (wave == 1) {
        double o[4];
        car_scale_wave(craw[0], craw[1], craw[2], cs[5], zs, zs + TR_N, tr_lds_int(cptr + 13) != 0, tr_lds_int(cptr + 12), cs[6], cs[7], lane, o);
        if (lane == 0) {
          cs[0] = o[0]; cs[1] = o[1]; cs[2] = o[2]; cs[3] = o[3];
          cs[4] = craw[0];
          sc[0] = ffgp_link_val(M.l.amp_link, raw[nw], M.l.amp_c) * o[0];
        }
      }
    }
    if constexpr (TLIN) {      // this step's targets R = y_high - y_low V^T: per entry one chain of fused multiply-adds over l, then the difference
      const double* yl = tr_lds_ptr(tptr);
      const double* yh = tr_lds_ptr(tptr + 2);
      const int tl_ = tr_lds_int(tptr + 4);
      int t0_ = tid;      // (opaque per step: the loop's offsets into y_low, y_high and V are otherwise hoisted out of the step loop and spilled across it)
      asm volatile("" : "+v"(t0_));
      for (int idx = t0_; idx < n * TR_Y; idx += TR_T) {
        const int i = idx >> 4, q = idx & 15;
        if (q < d) {
          double s_ = 0.0;
#pragma unroll 4
          for (int b = 0; b < tl_; ++b) s_ = __builtin_fma(yl[i * tl_ + b], tV[q * tl_ + b], s_);
          Ym[idx] = __dsub_rn(yh[i * d + q], s_);
        }
      }
      if (t0_ < d * tl_) tV0[t0_] = tV[t0_];
    }
    isres = RESID && tr_lds_int(rmode) != 0;
    if (isres) {      // this step's targets r = y_high - rho y_low and diagonal extra |s|, s = v_high - rho v_low, rounded as torch's
                      // `y_high - rho * y_low` (a product, then a difference: never contracted)
      hasv = tr_lds_int(rmode) == 2;
      const double* yl = tr_lds_ptr(rmode + 2);
      const double* yh = tr_lds_ptr(rmode + 4);
      const double rho = raw[nw + 2];
      for (int idx = tid; idx < n * TR_Y; idx += TR_T) {      // (over the image: no division by d)
        const int i = idx >> 4, q = idx & 15;
        if (q < d) Ym[idx] = __dsub_rn(yh[i * d + q], __dmul_rn(rho, yl[i * d + q]));
      }
      if (hasv) {
        for (int i = tid; i < n; i += TR_T) {
          const double s = __dsub_rn(rvh[i], __dmul_rn(rho, rvl[i]));
          dvec[i] = fabs(s);
          sgv[i] = (s > 0.0) ? rvl[i] : ((s < 0.0) ? -rvl[i] : 0.0);      // (torch's abs backward: sgn(0) = 0)
        }
      }
      if (tid == 0) rho0[0] = rho;
    }
    LDS_BARRIER();
    const double amp = sc[0], dadd = sc[1];
    TR_PROF(0);

    // ---- P1: Sigma, lower block triangle (diagonal blocks symmetric-full: the in-register factor wants both halves); rows / columns
    //      beyond n are identity
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
    TR_PROF(1);

    // ---- P2: blocked Cholesky over 16-column stages AND the inverse, two barriers per stage (train_tile.h)
    TR_FACTOR_STAGES(S, piv, flags, n, nst, lane, wave, g, c, hidx, nh, TR_PROF)
    if (flags[0] != 0) {       // (uniform: every thread reads the same word behind the barrier)
      failed = flags[0];
      if (TRAIN) {
        if (tid == 0) {
          cm.info[blockIdx.x] = failed;
          cm.fail_step[blockIdx.x] = step;
        }
        for (int k = step + tid; k < cm.steps; k += TR_T) M.trace[k] = __builtin_nan("");
      } else if (tid == 0) {      // (the blocked path goes on with a unit pivot and returns garbage; here the value is NaN)
        if (cm.info_max) atomicMax(cm.shared_info, failed);
        else cm.shared_info[0] = failed;
        M.nll[0] = __builtin_nan("");
      }
      break;
    }
    tr_inverse_last_row(S, nst, lane, wave, g, c);
    TR_PROF(5);

    // ---- P3: Gamma = W Y, A = W^T Gamma on the matrix cores (W = L^-1, lower; the d <= 16 target columns are one block column): wave w
    //      owns block row w of Gamma (w + 1 products) and block row 7 - w of A (w + 1 products)
    {
      tr_gamma_rows(S, Ym, Gam, nst, lane, wave, g, c);
      LDS_BARRIER();
      if constexpr (TLIN) {      // the targets' image is dead until the next step: y_low takes it, [n][16] zero beyond l, for dloss/dV below
        const double* yl = tr_lds_ptr(tptr);
        const int tl_ = tr_lds_int(tptr + 4);
        int t0_ = tid;
        asm volatile("" : "+v"(t0_));
        for (int idx = t0_; idx < n * TR_Y; idx += TR_T) {
          const int i = idx >> 4, q = idx & 15;
          Ym[idx] = (q < tl_) ? yl[i * tl_ + q] : 0.0;
        }
      }
      double ay = 0.0;      // residual members: this lane's part of sum A .* y_low
      isres = RESID && tr_lds_int(rmode) != 0;
      d4_t acc = {0.0, 0.0, 0.0, 0.0};
      if (tr_alpha_rows(S, Gam, Am, nst, lane, wave, g, c, acc)) {
        if (isres) {      // (y_low requested after the chain, not under it: four more live values there cost the <8> instantiation its
                          //  spill-free allocation)
          const int bi = 7 - wave;
          const double* yl = tr_lds_ptr(rmode + 2);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = bi * 16 + g + 4 * r;
            ay = __builtin_fma(acc[r], (i < n && c < d) ? yl[i * d + c] : 0.0, ay);
          }
        }
      }
      if (isres) {
        ay = tr_wsum(ay);
        if (lane == 0) rsum[wave] = ay;
      }
      LDS_BARRIER();
    }
    if constexpr (TLIN) {      // dloss/dV[a][b] = -sum_i A[i][a] y_low[i][b], i ascending: one thread per entry, both operands in LDS
      const int tl_ = tr_lds_int(tptr + 4);
      int t0_ = tid;
      asm volatile("" : "+v"(t0_));
      if (t0_ < d * tl_) {
        const int a_ = t0_ / tl_, b_ = t0_ - a_ * tl_;
        double s_ = 0.0;
#pragma unroll 4
        for (int i = 0; i < n; ++i) s_ = __builtin_fma(Am[i * TR_Y + a_], Ym[i * TR_Y + b_], s_);
        tdV[t0_] = -s_;
      }
    }
    if constexpr (V2) {      // B = Sigma^-1 A: the same two chains once more -- W A over Gamma (dead once A exists), B over the targets' image
      tr_gamma_rows(S, Am, Gam, nst, lane, wave, g, c);
      LDS_BARRIER();
      d4_t accb = {0.0, 0.0, 0.0, 0.0};
      tr_alpha_rows(S, Gam, Ym, nst, lane, wave, g, c, accb);
      LDS_BARRIER();
    }
    TR_PROF(6);

    // ---- P5: per lane partial sums -- ss (value), s_amp, tr G, tot[k] (length scales); Sigma^-1 block by block on the matrix cores.
    // (The length-scale sums through the matrix cores as well -- tot_k = sum_j [V_jk + x_jk^2 c_j - 2 x_jk U_jk] with U | V = W_low^T [X | X^2]
    //  as one MFMA group per block, the block's weights used as the A operand straight from the accumulator layout, added into an LDS
    //  image -- was built, passed every test and measured SLOWER: 12.4 against 10.2 us at n = 128, D = 5; four LDS atomics per lane and block
    //  and two more barriers cost more than the 24 vector instructions per entry they replace.)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this lane's parked kernel values have landed (long ago)
    double ss = 0.0, s_amp = 0.0, trg = 0.0, tk[DM];
#pragma unroll
    for (int k = 0; k < DM; ++k) tk[k] = 0.0;
    const double lpiv = (tid < n) ? log(piv[tid]) : 0.0;
#pragma unroll
    for (int q = 0; q < TR_N * TR_Y / TR_T; ++q) {      // V1: Y^T Sigma^-1 Y = |Gamma|^2; V2: |Sigma^-1 Y|^2 = |A|^2
      const double e_ = V2 ? Am[tid + TR_T * q] : Gam[tid + TR_T * q];
      ss = __builtin_fma(e_, e_, ss);
    }
    if constexpr (CAR) {      // this wave's part of sum dloss/dr .* y_low (dloss/dr = A, V2: B in the targets' image), over the image
      const double* yl = tr_lds_ptr(cptr);
      const double* dr = V2 ? Ym : Am;
      double cy = 0.0;
      int t0_ = tid;      // (opaque per step: the loop's offsets into y_low are otherwise hoisted out of the step loop and spilled across it)
      asm volatile("" : "+v"(t0_));
      for (int idx = t0_; idx < n * TR_Y; idx += TR_T) {
        const int i = idx >> 4, q = idx & 15;
        if (q < d) cy = __builtin_fma(dr[idx], yl[i * d + q], cy);
      }
      cy = tr_wsum(cy);
      if (lane == 0) csum[wave] = cy;
    }
    for (int q_ = 0; q_ < 5 && (TRAIN || M.want_grad); ++q_) {
      const int t = tr_deal(q_, wave);
      if (t >= nblk) continue;
      int bi, bj;
    blk_unrank(t, bi, bj);
      double evs[4];      // (requested before the block's products: the loads fly under the MFMA chain; written by this very lane)
#pragma unroll
      for (int r = 0; r < 4; ++r) evs[r] = M.kbuf[(t * 4 + r) * 64 + lane];
      d4_t acc = {0.0, 0.0, 0.0, 0.0};
      tr_chain<true>(acc, bi, nst, S, [bi](int kb) { return blk_off(kb, bi); }, BLD, S, [bj](int kb) { return blk_off(kb, bj); }, BLD, lane);
      const int j = bj * 16 + c;
      double xj[DM];
#pragma unroll
      for (int k = 0; k < DM; ++k) xj[k] = Xs[j * (TR_D + 1) + k];
#pragma unroll 1
      for (int r = 0; r < 4; ++r) {      // (one row at a time: four rows' differences in flight at once cost more registers than the chip has)
        const int i = bi * 16 + g + 4 * r;
        const double* xi = Xs + i * (TR_D + 1);
        const double accr = (r == 0) ? acc[0] : (r == 1) ? acc[1] : (r == 2) ? acc[2] : acc[3];
        const double ev = (r == 0) ? evs[0] : (r == 1) ? evs[1] : (r == 2) ? evs[2] : evs[3];
        double dsq[DM], sq = 0.0;
#pragma unroll
        for (int k = 0; k < DM; ++k) {
          const double df = xi[k] - xj[k];
          dsq[k] = df * df;
          sq += dsq[k];
        }
        double aa = 0.0;
        if constexpr (V2) {      // G = d/2 Sigma^-1 - 1/2 (A B^T + B A^T), B in the targets' image
          for (int q = 0; q < d; ++q) aa = __builtin_fma(Am[i * TR_Y + q], Ym[j * TR_Y + q], __builtin_fma(Ym[i * TR_Y + q], Am[j * TR_Y + q], aa));
        } else {
          for (int q = 0; q < d; ++q) aa = __builtin_fma(Am[i * TR_Y + q], Am[j * TR_Y + q], aa);
        }
        const bool live = (i < n && j <= i);
        const double gv = live ? 0.5 * (double)d * accr - 0.5 * aa : 0.0;
        const double sym = (i == j) ? 1.0 : 2.0;
        double m2 = ev;
        if (M.kfun != FFGP_KFUN_SE) m2 = ffgp_kfun_m2d(M.kfun, M.rinv, fmax(sq, M.clamp));
        s_amp = __builtin_fma(sym * gv, ev, s_amp);
        if (i == j) {
          trg += gv;
          if (!TRAIN && live) dvec[i] = gv;      // (evaluate mode: diag G for g_diag_vec; the diagonal extra was consumed by the assembly)
          if (RESID) gdg[i] = gv;                 // (residual members: the diagonal term of dloss/drho, summed behind the reduction's barrier)
        }
        const double wl = (sq >= M.clamp) ? sym * gv * amp * m2 : 0.0;
#pragma unroll
        for (int k = 0; k < DM; ++k) tk[k] = __builtin_fma(wl, dsq[k], tk[k]);
      }
    }
    TR_PROF(7);
    // ---- one workgroup reduction for all of them (and the log-determinant: one pivot per thread)
    {
      constexpr int NV = 4 + DM;
      double vals[NV];
      vals[0] = ss; vals[1] = s_amp; vals[2] = trg;
      vals[3] = lpiv;
#pragma unroll
      for (int k = 0; k < DM; ++k) vals[4 + k] = tk[k];
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        vals[q] = tr_wsum(vals[q]);
      }
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
      isres = RESID && tr_lds_int(rmode) != 0;
      hasv = RESID && tr_lds_int(rmode) == 2;
      if (isres && wave == 1) {      // dloss/drho (before the output scale) = -sum A .* y_low - sum_i G_ii sgn(s_i) v_low,ii, beside wave 0's totals
        double x = 0.0;
        if (hasv)
          for (int i = lane; i < n; i += 64) x = __builtin_fma(gdg[i], sgv[i], x);
        x = tr_wsum(x);
        if (lane == 0) {
          double a = 0.0;
#pragma unroll
          for (int wv_ = 0; wv_ < 8; ++wv_) a += rsum[wv_];
          tot[NRED - 1] = -a - x;
        }
      }
      if constexpr (CAR) {
        if (tid == 64) {      // sum dloss/dr .* y_low, beside wave 0's totals
          double a = 0.0;
#pragma unroll
          for (int wv_ = 0; wv_ < 8; ++wv_) a += csum[wv_];
          tot[NRED - 1] = a;
        }
      }
      LDS_BARRIER();
    }
    TR_PROF(8);
    // ---- P6: the loss of this step (before the update), the raw gradients through the links, Adam
    const double value = oscale * (0.5 * tot[0] + (double)d * 0.5 * tot[3] + 0.5 * (double)n * (double)d * log(2.0 * M.pi_const));
    if (!TRAIN) {
      if (tid == 0) M.nll[0] = value;
      if (M.want_grad) {
        if (tid < npar) {
          double gr;
          if (tid < nw) {
            if (!M.l.w_broadcast) {
              gr = oscale * (-tot[4 + tid] / wv[tid]) * ffgp_link_der(M.l.w_link, raw[tid], M.l.w_c);
            } else {
              double sg = 0.0;
              for (int k = 0; k < D; ++k) sg += -tot[4 + k] / wv[k];
              gr = oscale * sg * ffgp_link_der(M.l.w_link, raw[0], M.l.w_c);
            }
            if (M.g_w) M.g_w[tid] = gr;
          } else if (tid == nw) {
            if (M.g_amp) M.g_amp[0] = oscale * tot[1] * ffgp_link_der(M.l.amp_link, raw[nw], M.l.amp_c);
          } else if (M.g_dadd) {
            M.g_dadd[0] = oscale * tot[2] * (M.dadd ? ffgp_link_der(M.l.dadd_link, raw[nw + 1], M.l.dadd_c) : 1.0);
          }
        }
        if (M.g_Y)
          for (int idx = tid; idx < n * d; idx += TR_T) M.g_Y[idx] = oscale * Am[(idx / d) * TR_Y + (idx % d)];
        if (M.g_dvec)
          for (int i = tid; i < n; i += TR_T) M.g_dvec[i] = oscale * dvec[i];
      }
      break;
    }
    if (tid == 0) M.trace[step] = value;
    isres = RESID && tr_lds_int(rmode) != 0;
    if (tid < nw + 2 + (isres ? 1 : 0) + (CAR ? 3 : 0) + (TLIN ? d * tr_lds_int(tptr + 4) : 0)) {
      // (CAR: the slot opaque per step -- the loop-invariant addresses of a member's last three parameters, their moments and partials are
      //  otherwise hoisted out of the step loop and spilled across it)
      int slot_ = tid;
      if constexpr (CAR || TLIN) asm volatile("" : "+v"(slot_));
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
        if constexpr (CAR) gr *= cs[0];      // (tot[1] = T, with respect to the effective amplitude link(amp_raw) * s)
      } else if (CAR && slot_ > nw + 1) {      // b, l_z, sigma_z: dloss/ds = T link(amp_raw) times the partials of s; b's targets term
        const double dls = tot[1] * ffgp_link_val(M.l.amp_link, raw[nw], M.l.amp_c);
        const int k = slot_ - nw - 2;
        gr = oscale * dls * cs[1 + k];
        if (k == 0) gr = oscale * (dls * cs[1] - ceb[0] * tot[NRED - 1]);
      } else if (TLIN && slot_ > nw + 1) {     // V's entry slot - nw - 2 (raw = effective; tdV was written before the reduction's barriers)
        gr = oscale * tdV[slot_ - nw - 2];
      } else if (!isres || tid == nw + 1) {
        gr = oscale * tot[2] * ffgp_link_der(M.l.dadd_link, raw[nw + 1], M.l.dadd_c);
      } else {
        gr = oscale * tot[NRED - 1];      // rho (raw = effective)
      }
      // (a CAR member's last three parameters and their moments live in craw / cmom / cmo2)
      // (... a tensor-linear member's V entries and theirs in tV / tmV / tvV)
      double* const pr_ = ((CAR || TLIN) && slot_ > nw + 1) ? (TLIN ? tV : craw) + (slot_ - nw - 2) : raw + slot_;
      double* const pm_ = ((CAR || TLIN) && slot_ > nw + 1) ? (TLIN ? tmV : cmom) + (slot_ - nw - 2) : mom + slot_;
      double* const pv_ = ((CAR || TLIN) && slot_ > nw + 1) ? (TLIN ? tvV : cmo2) + (slot_ - nw - 2) : mo2 + slot_;
      const double bc1 = cm.bc[2 * step], bc2s = cm.bc[2 * step + 1];
      ffgp_adam_update(pr_, pm_, pv_, gr, cm.lr, cm.b1, cm.b2, cm.eps, bc1, bc2s);
      const double pnew = pr_[0];
      if (CAR && tid == nw + 2) ceb[0] = exp(pnew);
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
      } else if ((!isres && !((CAR || TLIN) && tid > nw + 1)) || tid == nw + 1) {      // (a CAR member's s is re-formed at the start of the step)
        sc[1] = ffgp_link_val(M.l.dadd_link, pnew, M.l.dadd_c);
      }
    }
    LDS_BARRIER();
    TR_PROF(9);
  }
  // ---- parameters and moments back to the caller's tensors (a failed step left them as they were when it began)
  if (RESID) isres = tr_lds_int(rmode) != 0;
  const int npe = nw + 2 + (isres ? 1 : 0) + (CAR ? 3 : 0);
  if (CAR && tid > nw + 1) {
    if (tid < npe) {
      const int k = tid - nw - 2;
      // (a pointer per lane: tr_lds_ptr makes its word wave-uniform)
      const unsigned long long u = ((unsigned long long)(unsigned)cptr[5 + 2 * k] << 32) | (unsigned)cptr[4 + 2 * k];
      reinterpret_cast<double*>(u)[0] = craw[k];
      if (k == 0) {
        double* bl = tr_lds_ptr(cptr + 10);
        if (bl) bl[0] = cs[4];
      }
      M.state[tid] = cmom[k];
      M.state[npe + tid] = cmo2[k];
    }
  } else if (TRAIN && tid < npe) {
    if (tid < nw) M.w[tid] = raw[tid];
    else if (tid == nw) M.amp[0] = raw[tid];
    else if (!isres || tid == nw + 1) M.dadd[0] = raw[tid];
    else {
      tr_lds_ptr(rmode + 6)[0] = raw[tid];
      double* rl = tr_lds_ptr(rmode + 8);
      if (rl) rl[0] = rho0[0];
    }
    M.state[tid] = mom[tid];
    M.state[npe + (TLIN ? d * Tp->l : 0) + tid] = mo2[tid];
  }
  if constexpr (TLIN) {      // V through its strides, its moments, and V as the last step taken began (a failed step left all of them as they were)
    const int tl_ = Tp->l, hl = d * tl_;
    if (tid < hl) {
      Tp->V[(tid / tl_) * Tp->rs + (tid % tl_) * Tp->cs] = tV[tid];
      M.state[nw + 2 + tid] = tmV[tid];
      M.state[nw + 2 + hl + nw + 2 + tid] = tvV[tid];
      if (Tp->V_last) Tp->V_last[tid] = tV0[tid];
    }
  }
  (void)failed;
}

template <int DM>
__global__ __launch_bounds__(TR_T) void ffgp_train_persist_kernel(const TrainModel* __restrict__ tab, TrainCommon cm) {
  const TrainModel M = tab[blockIdx.x];
  tr_body<DM, true>(M, cm);
}
// a launch with at least one residual member (rtab[f].rho == nullptr: a plain member)
template <int DM>
__global__ __launch_bounds__(TR_T) void ffgp_train_resid_kernel(const TrainModel* __restrict__ tab, const TrainResid* __restrict__ rtab,
                                                                TrainCommon cm) {
  const TrainModel M = tab[blockIdx.x];
  tr_body<DM, true, true>(M, cm, rtab + blockIdx.x);
}
// FFGP_LL_V2 members (GP_basic): a launch of their own, so that the V1 kernels keep their code and registers
template <int DM>
__global__ __launch_bounds__(TR_T) void ffgp_train_v2_kernel(const TrainModel* __restrict__ tab, TrainCommon cm) {
  const TrainModel M = tab[blockIdx.x];
  tr_body<DM, true, false, true>(M, cm);
}
// CAR members (ffgp_train_car_raw), by likelihood; ctab[f] is member f's link
template <int DM, bool V2>
__global__ __launch_bounds__(TR_T) void ffgp_train_car_kernel(const TrainModel* __restrict__ tab, const TrainCar* __restrict__ ctab,
                                                              TrainCommon cm) {
  const TrainModel M = tab[blockIdx.x];
  tr_body<DM, true, false, V2, true>(M, cm, nullptr, ctab + blockIdx.x);
}
// tensor-linear members (ffgp_train_tlin_raw); ttab[f] is member f's link
template <int DM>
__global__ __launch_bounds__(TR_T) void ffgp_train_tlin_kernel(const TrainModel* __restrict__ tab, const TrainTlin* __restrict__ ttab,
                                                               TrainCommon cm) {
  const TrainModel M = tab[blockIdx.x];
  tr_body<DM, true, false, false, false, true>(M, cm, nullptr, nullptr, ttab + blockIdx.x);
}
// evaluate mode: up to eight models per launch, their descriptions by value (the enqueue-only entry points must not stage anything in
// host memory that a later call could overwrite)
#define TR_EVAL_BATCH 8
struct TrainEvalBatch {
  TrainModel m[TR_EVAL_BATCH];
};
template <int DM>
__global__ __launch_bounds__(TR_T) void ffgp_small_mfma_kernel(TrainEvalBatch b, TrainCommon cm) {
  tr_body<DM, false>(b.m[blockIdx.x], cm);
}

// ---- host side ------------------------------------------------------------------------------------------------------
bool ffgp_train_persist_ok(const ffgp_handle* h, const ffgp_problem* p, const ffgp_links* l, const ffgp_residual* r, const ffgp_car_link* cr,
                           const ffgp_tlin_link* tl) {
  if (h->train_persist_off || h->use_naive || h->timing) return false;
  if (p->n <= 0 || p->n > TR_N || p->D <= 0 || p->D > TR_D || p->d <= 0 || p->d > TR_Y) return false;
  if (p->cov_dev || p->pair || p->tree || p->add_mat_dev || p->add_all != 0.0 || p->mean_jitter != 0.0) return false;
  const bool car = cr && cr->b_dev;
  if (car && (r || cr->nz <= 0 || cr->nz > TR_N)) return false;
  const bool lin = tl && tl->V_dev;      // (l <= h = d <= 16: train_impl has checked the link)
  if (lin && p->ll_variant != FFGP_LL_V1) return false;
  const bool res = (r && r->rho_dev) || car || lin;      // (a residual, CAR or tensor-linear member's targets come from its link: its Y_dev is ignored)
  if (!p->X_dev || (!res && !p->Y_dev) || !p->w_dev || !p->amp_dev || !p->diag_add_dev) return false;
  if (p->kfun < FFGP_KFUN_SE || p->kfun > FFGP_KFUN_RQ) return false;
  if (p->ll_variant == FFGP_LL_V2) return !res || car;      // (ffgp_train_v2_kernel: plain members, diag_add under any link; CAR members)
  if (p->ll_variant != FFGP_LL_V1) return false;
  (void)l;
  return true;
}

// steps of F models (each must pass ffgp_train_persist_ok), one launch; synchronous.  Returns 0 or the pivot status of the first
// model (in the caller's order) whose Sigma was not positive definite at some step.
int ffgp_train_persist(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* l, int steps, const ffgp_adam* opt, double* state_dev,
                       long state_stride, long step0, double* trace_dev, long trace_stride, const ffgp_residual* r, const ffgp_car_link* cr,
                       const ffgp_tlin_link* tl) {
  bool any_res = false, any_car = false, any_lin = false;
  for (int f = 0; f < F && tl; ++f) any_lin = any_lin || tl[f].V_dev != nullptr;
  for (int f = 0; f < F && r; ++f) any_res = any_res || r[f].rho_dev != nullptr;
  for (int f = 0; f < F && cr; ++f) any_car = any_car || cr[f].b_dev != nullptr;
  // five classes of members, a launch each: V1 (plain and residual), V2, CAR on V1, CAR on V2, tensor-linear.  pos[f] = model f's row of the tables and
  // of the status words: class after class, the caller's order inside a class; cbeg[k] = the first row of class k
  auto cls = [&](int f) { return (tl && tl[f].V_dev) ? 4 : ((cr && cr[f].b_dev) ? 2 : 0) + (p[f].ll_variant == FFGP_LL_V2 ? 1 : 0); };
  std::vector<int> pos(F);
  int cbeg[6] = {0, 0, 0, 0, 0, 0};
  for (int k = 0, q = 0; k < 5; ++k) {
    cbeg[k] = q;
    for (int f = 0; f < F; ++f)
      if (cls(f) == k) pos[f] = q++;
    cbeg[k + 1] = q;
  }
  // the call's block (train_host.h); the tables: [F models | F residual links (residual launches) | F CAR links (CAR launches)], the
  // scratch: F x 36 x 256 kernel values
  TrainLayout lay;
  const size_t tab_off = lay.take((size_t)F * sizeof(TrainModel));
  const size_t res_off = any_res ? lay.take((size_t)F * sizeof(TrainResid)) : 0;
  const size_t car_off = any_car ? lay.take((size_t)F * sizeof(TrainCar)) : 0;
  const size_t lin_off = any_lin ? lay.take((size_t)F * sizeof(TrainTlin)) : 0;
  TrainBlock blk;
  FFGP_CHECK(train_block_open(h, lay, F, steps, opt, step0, (size_t)F * NBLK_LOWER * 256 * sizeof(double), &blk));
  char* const host = blk.host;
  char* const dev = blk.dev;
  TrainModel* tm = reinterpret_cast<TrainModel*>(host + tab_off);
  for (int f = 0; f < F; ++f) {
    const ffgp_problem& q = p[f];
    TrainModel& m = tm[pos[f]];
    m.n = q.n; m.D = q.D; m.d = q.d; m.nw = l[f].w_broadcast ? 1 : q.D;
    m.X = q.X_dev; m.Y = q.Y_dev;
    m.w = const_cast<double*>(q.w_dev); m.amp = const_cast<double*>(q.amp_dev); m.dadd = const_cast<double*>(q.diag_add_dev);
    m.diag_vec = q.diag_vec_dev; m.diag_stride = q.diag_stride;
    m.l = l[f];
    m.clamp = q.clamp_min; m.rinv = (q.kparam != 0.0) ? 1.0 / q.kparam : 1.0; m.pi_const = q.pi_const; m.kfun = q.kfun;
    m.state = state_dev + (size_t)f * state_stride;
    m.trace = trace_dev + (size_t)f * trace_stride;
    m.kbuf = reinterpret_cast<double*>(dev + blk.scratch_off) + (size_t)pos[f] * NBLK_LOWER * 256;
    m.want_grad = 1;
  }
  if (any_res) {
    TrainResid* tr = reinterpret_cast<TrainResid*>(host + res_off);
    for (int f = 0; f < F; ++f) {
      const ffgp_residual& q = r[f];
      TrainResid& t = tr[pos[f]];
      t.rho = q.rho_dev;
      if (!q.rho_dev) continue;
      t.yl = q.y_low_dev; t.yh = q.y_high_dev;
      t.vl = q.v_low_dev; t.vh = q.v_high_dev; t.vl_stride = q.v_low_stride; t.vh_stride = q.v_high_stride;
      t.rho_last = q.rho_last_dev;
    }
  }
  if (any_car) {
    TrainCar* tc = reinterpret_cast<TrainCar*>(host + car_off);
    for (int f = 0; f < F; ++f) {
      const ffgp_car_link& q = cr[f];
      if (!q.b_dev) continue;
      TrainCar& t = tc[pos[f]];
      t.b = q.b_dev; t.zls = q.zls_dev; t.zamp = q.zamp_dev;
      t.zeps = q.zeps; t.lf = q.lf; t.hf = q.hf;
      t.z1 = q.z1_dev; t.z2 = q.z2_dev; t.nz = q.nz;
      t.z1d = q.z1d_dev; t.z2d = q.z2d_dev;
      t.yl = q.y_low_dev; t.yh = q.y_high_dev;
      t.b_last = q.b_last_dev;
    }
  }
  if (any_lin) {
    TrainTlin* tt = reinterpret_cast<TrainTlin*>(host + lin_off);
    for (int f = 0; f < F; ++f) {
      const ffgp_tlin_link& q = tl[f];
      if (!q.V_dev) continue;
      TrainTlin& t = tt[pos[f]];
      t.V = q.V_dev; t.rs = q.V_row_stride; t.cs = q.V_col_stride; t.l = q.l;
      if (t.rs == 0 && t.cs == 0) { t.rs = q.l; t.cs = 1; }
      t.yl = q.y_low_dev; t.yh = q.y_high_dev;
      t.V_last = q.V_last_dev;
    }
  }
  FFGP_HIP(hipMemcpyAsync(dev, host, blk.head, hipMemcpyHostToDevice, h->stream));
  TrainCommon cm;
  static_cast<TrainLoop&>(cm) = blk.loop;
  cm.shared_info = nullptr;
  cm.info_max = 0;
  cm.prof = nullptr;
  static const bool trace_on = getenv("FFGP_TRAIN_TRACE") && atoi(getenv("FFGP_TRAIN_TRACE")) != 0;
  if (trace_on) {
    FFGP_HIP(hipMalloc(&cm.prof, 12 * sizeof(long)));
    FFGP_HIP(hipMemset(cm.prof, 0, 12 * sizeof(long)));
  }
  int Dm[5] = {0, 0, 0, 0, 0};
  for (int f = 0; f < F; ++f) Dm[cls(f)] = std::max(Dm[cls(f)], p[f].D);
  for (int k = 0; k < 5; ++k) {      // class k: rows cbeg[k] .. cbeg[k + 1] - 1 of the tables and of the status words
    const int nk = cbeg[k + 1] - cbeg[k];
    if (nk == 0) continue;
    TrainCommon c2 = cm;
    c2.info = cm.info + cbeg[k];
    c2.fail_step = cm.fail_step + cbeg[k];
    const TrainModel* tab = reinterpret_cast<const TrainModel*>(dev + tab_off) + cbeg[k];
    const TrainResid* rtab = reinterpret_cast<const TrainResid*>(dev + res_off);      // (class 0 begins at row 0)
    const TrainCar* ctab = reinterpret_cast<const TrainCar*>(dev + car_off) + cbeg[k];
    const TrainTlin* ttab = reinterpret_cast<const TrainTlin*>(dev + lin_off) + cbeg[k];
    const size_t lds = TR_LDS_DOUBLES * sizeof(double), lds_res = TR_LDS_DOUBLES_RES * sizeof(double), lds_car = TR_LDS_DOUBLES_CAR * sizeof(double);
    const size_t lds_lin = TR_LDS_DOUBLES_TLIN * sizeof(double);
    // (a lambda per kernel, in this order: the instantiations are emitted kernel by kernel, <8> then <16>, as they always were)
    int rc;
    if (k == 0 && !any_res) rc = tr_by_dm(Dm[k], [&](auto dm) { return train_launch(h, ffgp_train_persist_kernel<dm()>, lds, nk, tab, c2); });
    else if (k == 0) rc = tr_by_dm(Dm[k], [&](auto dm) { return train_launch(h, ffgp_train_resid_kernel<dm()>, lds_res, nk, tab, rtab, c2); });
    else if (k == 1) rc = tr_by_dm(Dm[k], [&](auto dm) { return train_launch(h, ffgp_train_v2_kernel<dm()>, lds, nk, tab, c2); });
    else if (k == 2) rc = tr_by_dm(Dm[k], [&](auto dm) { return train_launch(h, ffgp_train_car_kernel<dm(), false>, lds_car, nk, tab, ctab, c2); });
    else if (k == 3) rc = tr_by_dm(Dm[k], [&](auto dm) { return train_launch(h, ffgp_train_car_kernel<dm(), true>, lds_car, nk, tab, ctab, c2); });
    else rc = tr_by_dm(Dm[k], [&](auto dm) { return train_launch(h, ffgp_train_tlin_kernel<dm()>, lds_lin, nk, tab, ttab, c2); });
    FFGP_CHECK(rc);
  }
  const int rc = train_block_finish(h, blk, F, pos.data());
  if (cm.prof) {
    long pr[12];
    hipMemcpy(pr, cm.prof, sizeof(pr), hipMemcpyDeviceToHost);
    hipFree(cm.prof);
    static const char* const nm[10] = {"links+Xs", "assemble", "F(jj)", "solve", "update", "inverse", "Gamma/A", "Sigma^-1+grad", "reduce", "adam"};
    fprintf(stderr, "[ffgp] train_persist n=%d D=%d d=%d steps=%d, us per step:", p[0].n, p[0].D, p[0].d, steps);
    double tot = 0.0;
    for (int k = 0; k < 10; ++k) {
      fprintf(stderr, " %s %.2f", nm[k], pr[k] * 0.01 / steps);
      tot += pr[k] * 0.01 / steps;
    }
    fprintf(stderr, " | sum %.2f\n", tot);
  }
  return rc;
}

// ---- evaluate mode: one likelihood (+ gradients) of F small problems, ONE launch per eight of them ---------------------------------
// What ffgp_nlml_fused_small_batch and, for 40 < n <= 128, ffgp_nlml_fused_raw run instead of the scalar one-workgroup kernel of
// small.hip (0.58 ms at n = 128) or ~13 launches of the blocked path (0.098 ms): the trainer's pass without Adam.
bool ffgp_small_mfma_ok(const ffgp_handle* h, const ffgp_problem* p, const ffgp_grads* g) {
  if (h->train_persist_off || h->use_naive || h->timing || h->small_off) return false;
  if (p->n <= 0 || p->n > TR_N || p->D <= 0 || p->D > TR_D || p->d <= 0 || p->d > TR_Y) return false;
  if (p->cov_dev || p->pair || p->tree || p->add_mat_dev || p->add_all != 0.0 || p->mean_jitter != 0.0) return false;
  if (!p->X_dev || !p->Y_dev || !p->w_dev || !p->amp_dev) return false;
  if (p->kfun < FFGP_KFUN_SE || p->kfun > FFGP_KFUN_RQ || p->ll_variant != FFGP_LL_V1) return false;
  if (g && (g->g_cov_dev || g->g_pair || g->g_kparam_dev)) return false;
  return true;
}

int ffgp_small_mfma_enqueue(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* l, double* nll_dev, const ffgp_grads* g,
                            int info_max) {
  static bool attr_set[64] = {false};
  if (h->device >= 0 && h->device < 64 && !attr_set[h->device]) {
    FFGP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ffgp_small_mfma_kernel<8>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 TR_LDS_DOUBLES * (int)sizeof(double)));
    FFGP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ffgp_small_mfma_kernel<16>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 TR_LDS_DOUBLES * (int)sizeof(double)));
    attr_set[h->device] = true;
  }
  if (!h->small_kbuf) FFGP_HIP(hipMalloc(&h->small_kbuf, (size_t)TR_EVAL_BATCH * NBLK_LOWER * 256 * sizeof(double)));
  TrainCommon cm;
  memset(&cm, 0, sizeof(cm));
  cm.steps = 1;
  cm.shared_info = h->d_info;
  cm.info_max = info_max;
  for (int f0 = 0; f0 < F; f0 += TR_EVAL_BATCH) {
    const int nb = std::min(TR_EVAL_BATCH, F - f0);
    TrainEvalBatch b;
    memset(&b, 0, sizeof(b));
    int Dmax = 0;
    for (int z = 0; z < nb; ++z) {
      const ffgp_problem& q = p[f0 + z];
      const ffgp_grads* gg = g ? g + f0 + z : nullptr;
      TrainModel& m = b.m[z];
      m.n = q.n; m.D = q.D; m.d = q.d;
      m.X = q.X_dev; m.Y = q.Y_dev;
      m.w = const_cast<double*>(q.w_dev); m.amp = const_cast<double*>(q.amp_dev); m.dadd = const_cast<double*>(q.diag_add_dev);
      m.diag_vec = q.diag_vec_dev; m.diag_stride = q.diag_stride;
      if (l) {
        m.l = l[f0 + z];
      } else {      // effective parameters: identity links
        memset(&m.l, 0, sizeof(m.l));
        m.l.w_link = m.l.amp_link = m.l.dadd_link = FFGP_LINK_ID;
      }
      m.nw = m.l.w_broadcast ? 1 : q.D;
      m.clamp = q.clamp_min; m.rinv = (q.kparam != 0.0) ? 1.0 / q.kparam : 1.0; m.pi_const = q.pi_const; m.kfun = q.kfun;
      m.nll = nll_dev + f0 + z;
      if (gg) {
        m.g_w = gg->g_w_dev; m.g_amp = gg->g_amp_dev; m.g_dadd = gg->g_diag_add_dev; m.g_Y = gg->g_Y_dev; m.g_dvec = gg->g_diag_vec_dev;
      }
      m.want_grad = (m.g_w || m.g_amp || m.g_dadd || m.g_Y || m.g_dvec) ? 1 : 0;
      m.kbuf = h->small_kbuf + (size_t)z * NBLK_LOWER * 256;
      Dmax = std::max(Dmax, q.D);
    }
    if (Dmax <= 8)
      hipLaunchKernelGGL(ffgp_small_mfma_kernel<8>, dim3(nb), dim3(TR_T), TR_LDS_DOUBLES * sizeof(double), h->stream, b, cm);
    else
      hipLaunchKernelGGL(ffgp_small_mfma_kernel<16>, dim3(nb), dim3(TR_T), TR_LDS_DOUBLES * sizeof(double), h->stream, b, cm);
  }
  return hipGetLastError() == hipSuccess ? FFGP_OK : FFGP_ERR_HIP;
}
