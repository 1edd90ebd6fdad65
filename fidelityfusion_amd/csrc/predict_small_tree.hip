// The posteriors of F small COMPOSED-kernel GPs -- SumKernel / ProductKernel trees of 2-4 leaves (ffgp_ktree) -- at their own test points in
// ONE launch: ffgp_predict_small_tree_batch.  Every cigp demo of the reference, its BO model and its two-fidelity models run on
// SumKernel(LinearKernel, MaternKernel) (GaussianProcess/cigp_v10.py:81,111,147; Bayesian_optimization/cigp.py:119); they are trained in
// one launch (train_tree_lds.h) and until now predicted model by model.  This is predict_small.hip's launch -- grid (F, S), every
// workgroup runs the set-up once and walks tiles s, s + S, ... of 16 test points; its header describes the stages and why a point's
// results depend on nothing but its model -- with the assembly of the one-launch tree trainer in place of the radial one:
//
//   X sits in LDS as given, neither scaled nor shifted (ttl_body's reason: four scaled copies do not fit, and a difference of given
//   coordinates is exact); per leaf w_e, w_e^2, the centre and (amp, clamp, 1 / kparam), through the links with ffgp_link_val;
//   per entry and leaf ttl_form, then amp_e phi_e (ffgp_kfun_val; a linear leaf: amp_e times the form), then ffgp_tree_eval;
//   diag_add on Sigma's diagonal.  K_s: the same per (training row, test point), the test points unscaled in xt.
//   k(x, x): the tree on the leaves' self values -- radial amp_e phi_e(max(0, clamp_e)), linear amp_e sum_k w_ek^2 (x_k - c_k)^2, so it is
//   formed per column (by the thread that holds the column's point from the K_s stage), not once per model.
//
// The entry itself -- the leaf loop and the tree -- is ttl_entry of train_tree_lds.h, the function phase P1 of ttl_body calls too: moving
// P1's entry into it left the two trainer units' code as it was up to register names, the order of adjacent zero moves and the operand
// order of the tree's (commutative) multiplies and adds -- the same opcodes, the same register counts, no spill.  Also shared: ttl_form,
// TTL_PUT, the leaf tables' layout, ffgp_tree_eval, the member description and its checks (ttl_describe: ffgp_tree_form_ok,
// ffgp_tree_leaf_trainable), train_tile.h's stages and predict_small.h's host side.  The block walk around the entry (tr_deal, the
// diagonal, the identity beyond n) is the few lines every user of train_tile.h writes.
#include <vector>

#include "predict_small.h"
#include "train_tree_lds.h"

struct PstModel {
  TtlModel t;                              // ttl_describe's description; P, state, trace, wbuf, oscale and pi_const are not read
  const double* Xs; int nt;
  double* mean; double* var;
  int add_noise;
};

// LDS (doubles): the shared head of train_tile.h | per leaf wv, w2, cen [4][16] each and (amp, clamp, 1 / kparam, -) [4][4] (the
// trainer's leaf tables) | sc [8] | xt [16][17] | vsq [32][16] | ints: leaf kfun [4], tree [5], pad, flags + SIMD words [16]
#define PST_OFF_LEAF TR_OFF_TAIL
#define PST_OFF_SC (PST_OFF_LEAF + 3 * TTL_L * TR_D + 4 * TTL_L)
#define PST_OFF_XT (PST_OFF_SC + 8)
#define PST_OFF_VSQ (PST_OFF_XT + 16 * (TR_D + 1))
#define PST_OFF_INT (PST_OFF_VSQ + 32 * 16)
#define PST_INTS (4 + 5 + 3 + 16)
#define PST_LDS_DOUBLES (PST_OFF_INT + PST_INTS / 2)
static_assert(PST_INTS % 2 == 0, "the int table ends on a double");
static_assert(PST_LDS_DOUBLES * sizeof(double) <= 160 * 1024, "the tree predict launch's LDS exceeds a CU's 160 KiB");
#define PST_NOPROF(k) (void)0

// DM: the input dimensions the per-entry loops are unrolled for (8 or 16: every model of the launch has D <= DM)
template <int DM>
__global__ __launch_bounds__(TR_T) void ffgp_predict_small_tree_kernel(const PstModel* __restrict__ tab, int* __restrict__ info) {
  const PstModel* __restrict__ M = tab + blockIdx.x;
  const int nt = M->nt, ntile = (nt + 15) >> 4;
  if ((int)blockIdx.y >= ntile) return;      // (uniform: this model has fewer tiles than the call's largest)
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* S = lds;
  double* Xs = lds + TR_OFF_XS;
  double* Ym = lds + TR_OFF_YM;            // the targets, then K_s of the current tile
  double* Gam = lds + TR_OFF_GAM;
  double* Am = lds + TR_OFF_AM;
  double* piv = lds + TR_OFF_PIV;
  double* wv = lds + PST_OFF_LEAF;         // [leaf][16] effective inverse length scales
  double* w2 = wv + TTL_L * TR_D;          // [leaf][16] their squares (zero past D)
  double* cen = w2 + TTL_L * TR_D;         // [leaf][16] a linear leaf's centre (zero past D, and for the origin)
  double* lp = cen + TTL_L * TR_D;         // [leaf][4]  effective amplitude, clamp, 1 / kparam
  double* sc = lds + PST_OFF_SC;           // [0] effective diag_add, [1] the noise added to the variance
  double* xt = lds + PST_OFF_XT;           // [16][17] the tile's test points, as given
  double* vsq = lds + PST_OFF_VSQ;         // [4 nst][16] partial column sums of V^2
  int* kfi = reinterpret_cast<int*>(lds + PST_OFF_INT);      // [leaf] FFGP_KFUN_*
  int* tri = kfi + 4;                      // nl, shape, op[3]
  int* flags = tri + 8;                    // [0] bad pivot; [8 + wave] the waves' SIMDs
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int n = M->t.n, D = M->t.D, d = M->t.d;
  const int nst = (n + 15) >> 4, nblk = nst * (nst + 1) / 2;
  double* const mean_out = M->mean;
  double* const var_out = M->var;

  // ---- once: the trainer's set-up.  Targets, Gamma and A as [128][16] images, zero beyond (n, d); X as [128][17], zero beyond (n, D);
  //      identity in the blocks the factorisation never touches
  for (int idx = tid; idx < TR_N * TR_Y; idx += TR_T) {
    const int i = idx >> 4, q = idx & 15;
    Ym[idx] = (i < n && q < d) ? M->t.Y[i * d + q] : 0.0;
    Gam[idx] = 0.0;
    Am[idx] = 0.0;
  }
  for (int idx = tid; idx < TR_N * (TR_D + 1); idx += TR_T) {
    const int i = idx / (TR_D + 1), k = idx - i * (TR_D + 1);
    Xs[idx] = (i < n && k < D) ? M->t.X[i * D + k] : 0.0;
  }
  for (int t = wave; t < NBLK_LOWER; t += 8) {
    int bi, bj;
    blk_unrank(t, bi, bj);
    if (bi < nst) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) S[blk_off(bi, bj) + (g + 4 * r) * BLD + c] = (bi == bj && g + 4 * r == c) ? 1.0 : 0.0;
  }
  if (tid == 0) {
    flags[0] = 0;
    tri[0] = M->t.nl; tri[1] = M->t.shape; tri[2] = M->t.op[0]; tri[3] = M->t.op[1]; tri[4] = M->t.op[2];
  }
  if (tid < TTL_L) kfi[tid] = (tid < M->t.nl) ? M->t.k[tid].kfun : FFGP_KFUN_SE;
  if (lane == 0) flags[8 + wave] = wave_simd(wave);
  if (tid < TTL_L * TR_D) {      // the leaves' effective parameters through the links: ttl_body's, from the caller's tensors
    const int e = tid >> 4, k = tid & 15;
    double v = 0.0, cv = 0.0;
    if (e < M->t.nl && k < D) {
      const TtlLeaf& lf = M->t.k[e];
      v = ffgp_link_val(lf.w_link, lf.w[(lf.nw == D) ? k : 0], lf.w_c);
      if (lf.kfun == FFGP_KFUN_LINEAR && lf.cen) cv = lf.cen[k];
    }
    wv[tid] = v;
    w2[tid] = v * v;
    cen[tid] = cv;
  } else if (tid < TTL_L * TR_D + TTL_L) {
    const int e = tid - TTL_L * TR_D;
    const bool on = e < M->t.nl;
    const TtlLeaf& lf = M->t.k[on ? e : 0];
    lp[4 * e] = on ? ffgp_link_val(lf.amp_link, lf.amp[0], lf.amp_c) : 0.0;
    lp[4 * e + 1] = lf.clamp;
    lp[4 * e + 2] = lf.rinv;
    lp[4 * e + 3] = 0.0;
  } else if (tid == TTL_L * TR_D + TTL_L) {
    sc[0] = ffgp_link_val(M->t.dadd_link, M->t.dadd[0], M->t.dadd_c);
    sc[1] = M->add_noise ? ffgp_link_val(M->t.dadd_link, M->t.dadd[0], 0.0) : 0.0;
  }
  __syncthreads();
  int hidx, nh;
  helper_roles(flags + 8, lane, wave, hidx, nh);
  TtlTree tr;
  tr.nl = tr_lds_int(tri); tr.shape = tr_lds_int(tri + 1); tr.op[0] = tr_lds_int(tri + 2); tr.op[1] = tr_lds_int(tri + 3);
  tr.op[2] = tr_lds_int(tri + 4);

  // ---- Sigma, lower block triangle (diagonal blocks symmetric-full), identity beyond n: phase P1 of ttl_body without diag_vec
  {
    const double dadd = sc[0];
    for (int q_ = 0; q_ < 5; ++q_) {
      const int t = tr_deal(q_, wave);
      if (t >= nblk) continue;
      int bi, bj;
      blk_unrank(t, bi, bj);
      double* dst = S + blk_off(bi, bj);
      const int j = bj * 16 + c;
      double xj[DM];
#pragma unroll
      for (int k = 0; k < DM; ++k) xj[k] = Xs[j * (TR_D + 1) + k];
#pragma unroll 1
      for (int r = 0; r < 4; ++r) {
        const int i = bi * 16 + g + 4 * r;
        double kv = ttl_entry<DM>(tr, kfi, lp, w2, cen, Xs + i * (TR_D + 1), xj);
        if (i == j) kv += dadd;
        if (i >= n || j >= n) kv = (i == j) ? 1.0 : 0.0;
        dst[(g + 4 * r) * BLD + c] = kv;
      }
    }
  }
  LDS_BARRIER();

  // ---- blocked Cholesky AND the inverse (train_tile.h); a Sigma that is not positive definite ends this member here
  TR_FACTOR_STAGES(S, piv, flags, n, nst, lane, wave, g, c, hidx, nh, PST_NOPROF)
  if (flags[0] != 0) {      // (uniform: every thread reads the same word behind the barrier)
    if (tid == 0 && blockIdx.y == 0) info[blockIdx.x] = flags[0];
    for (int tile = blockIdx.y; tile < ntile; tile += gridDim.y) {
      const int p0 = tile * 16, np = min(16, nt - p0);
      for (int idx = tid; idx < np * d; idx += TR_T) mean_out[(size_t)p0 * d + idx] = __builtin_nan("");
      if (tid < np) var_out[p0 + tid] = __builtin_nan("");
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
  const double noise = sc[1];
  const double* Xt_in = M->Xs;
  const int mean_wave = (nst < 8) ? 7 : 0;      // (a wave without a block row of V when there is one)
  for (int tile = blockIdx.y; tile < ntile; tile += gridDim.y) {
    const int p0 = tile * 16;
    for (int idx = tid; idx < 16 * (TR_D + 1); idx += TR_T) {      // columns beyond nt repeat the last point (never stored)
      const int cc = idx / (TR_D + 1), k = idx - cc * (TR_D + 1);
      const int p = min(p0 + cc, nt - 1);
      xt[idx] = (k < D) ? Xt_in[(size_t)p * D + k] : 0.0;
    }
    LDS_BARRIER();
    double kself = 0.0;      // k(x, x) of column tid, in the threads tid < 16 that store the variance
    {      // K_s: thread (i0 = tid / 16, c) forms rows i0, i0 + 32, ... of column c; zero rows from n up to the last block's end
      const int cc = tid & 15, i0 = tid >> 4;
      double xj[DM];
#pragma unroll
      for (int k = 0; k < DM; ++k) xj[k] = xt[cc * (TR_D + 1) + k];
#pragma unroll 1
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 32 * r;
        if (i >= nst * 16) continue;
        const double kv = ttl_entry<DM>(tr, kfi, lp, w2, cen, Xs + i * (TR_D + 1), xj);
        Ks[i * TR_Y + cc] = (i < n) ? kv : 0.0;
      }
      if (tid < 16) {      // (i0 = 0, cc = tid) the leaves' self values: phi_e at max(0, clamp_e), a linear leaf's form at the point itself
        double v[TTL_L] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
        for (int e = 0; e < tr.nl; ++e) {
          const int kf = tr_lds_int(kfi + e);
          const bool lin = kf == FFGP_KFUN_LINEAR;
          const double s = lin ? ttl_form<DM>(true, xt + cc * (TR_D + 1), xj, w2 + e * TR_D, cen + e * TR_D) : fmax(0.0, lp[4 * e + 1]);
          const double val = lp[4 * e] * (lin ? s : ffgp_kfun_val(kf, lp[4 * e + 2], s));
          TTL_PUT(v, e, val);
        }
        kself = ffgp_tree_eval(tr, v);
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
        if (p < nt && c < d) mean_out[(size_t)p * d + c] = acc[r];
      }
    }
    LDS_BARRIER();
    if (tid < 16 && p0 + tid < nt) {      // the column's partial sums in one fixed order
      double s_ = 0.0;
      for (int q = 0; q < 4 * nst; ++q) s_ += vsq[q * 16 + tid];
      var_out[p0 + tid] = kself - s_ + noise;
    }
  }
}

// the member's description (ttl_describe: the tree's form, the leaves), or false when it is outside what the kernel covers
static bool pst_describe(const ffgp_problem& q, const ffgp_tree_links& l, const ffgp_predict_member& m, PstModel& t) {
  if (!ps_sizes_ok(q, m) || !q.Y_dev || q.diag_vec_dev) return false;
  ffgp_problem qq = q;
  qq.ll_variant = FFGP_LL_V1;      // (ignored here, as in ffgp_predict; ttl_describe is asked about the rest)
  if (!ttl_describe(qq, l, 2 * (TTL_PMAX + 1), t.t)) return false;
  t.Xs = m.Xs_dev; t.nt = m.nt;
  t.mean = m.mean_dev; t.var = m.var_dev;
  t.add_noise = m.var_add_noise;
  return true;
}

extern "C" int ffgp_predict_small_tree_batch(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_tree_links* l, const ffgp_predict_member* m,
                                             int* status) {
  if (!h || !p || !m || F < 1 || F > FFGP_PREDICT_SMALL_MAX_F) return FFGP_ERR_ARG;
  ffgp_tree_links idl;      // effective parameters: identity links (w_dev holds D values, no trained centre)
  memset(&idl, 0, sizeof(idl));
  for (int e = 0; e < 4; ++e) idl.leaf[e].w_link = idl.leaf[e].amp_link = FFGP_LINK_ID;
  idl.dadd_link = FFGP_LINK_ID;
  std::vector<PstModel> tm((size_t)F);
  int Dmax = 0, tiles = 1;
  for (int f = 0; f < F; ++f) {      // (every member is checked before anything is allocated on the device, enqueued or written)
    if (!pst_describe(p[f], l ? l[f] : idl, m[f], tm[f])) return FFGP_ERR_ARG;
    Dmax = std::max(Dmax, p[f].D);
    tiles = std::max(tiles, (m[f].nt + 15) / 16);
  }
  const int split = ps_split(F, tiles);
  FFGP_HIP(hipSetDevice(h->device));
  // the call's block (train_host.h): the table of F models and the status words; no steps, no scratch
  TrainLayout lay;
  const size_t tab_off = lay.take((size_t)F * sizeof(PstModel));
  TrainBlock blk;
  const ffgp_adam no_opt = {0.0, 0.0, 0.0, 0.0};
  FFGP_CHECK(train_block_open(h, lay, F, 0, &no_opt, 0, 0, &blk));
  memcpy(blk.host + tab_off, tm.data(), (size_t)F * sizeof(PstModel));
  FFGP_HIP(hipMemcpyAsync(blk.dev, blk.host, blk.head, hipMemcpyHostToDevice, h->stream));
  const PstModel* tab = reinterpret_cast<const PstModel*>(blk.dev + tab_off);
  int* info = blk.loop.info;
  const size_t lds_bytes = PST_LDS_DOUBLES * sizeof(double);
  FFGP_CHECK(tr_by_dm(Dmax, [&](auto dm) -> int {
    auto kernel = ffgp_predict_small_tree_kernel<dm()>;
    FFGP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    hipLaunchKernelGGL(kernel, dim3(F, split), dim3(TR_T), lds_bytes, h->stream, tab, info);
    return hipGetLastError() == hipSuccess ? FFGP_OK : FFGP_ERR_HIP;
  }));
  return ps_finish(h, blk, F, status);
}
