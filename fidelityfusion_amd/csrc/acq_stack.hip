// The acquisition optimiser's Adam loop on a STACK of frozen posteriors in one launch (ffgp_acq_optimize_stack, include/ffgp.h).
// Reference: MF_BayesianOptimization/Discrete/DMF_acq.py:226-262 optimises acq_mf(X, s) on the posterior of AR / ResGP / CAR
// (FidelityFusion_Models/AR_autoRegression.py:56-89): mean = sum_f c_f m_f, var = sum_f c'_f v_f over the per-fidelity GPs up to
// `to_fidelity`.  The plan is ffgp_acq_kernel's (acq.hip): a workgroup owns 16 query points and runs all the steps; what is new is
// the loop over the members inside a step.
//
// Per step and tile (thread (rg = tid >> 4, j = tid & 15) works on query column j), for every member f up to the tile's largest level:
//   0. X_f, alpha_f and w_f^2 are reloaded into LDS (at most 32 KiB from L2, against ~256 KiB of L_f^-1 traffic for the same member),
//      every row up to np_f written: a member smaller than its predecessor must not see the predecessor's rows
//   1.-3. K_s, the derivative factors, mean_f, V = L_f^-1 K_s, |V_j|^2, B = L_f^-T V: acq.hip's stages on images of np_f rows
//         (the load, the reductions, stages 2 and 3, the acquisition value and the owner's step are acq_tile.h's, one copy for all four kernels)
//   4. mean += on c_f mean_f, var += on c'_f (amp_f - |V_j|^2 + var_add_f), on = (f <= level_j) as an exact 0 / 1 factor, and the two
//      running gradient partials over this thread's rows,
//          Gm += on c_f  w_f^2 o sum_i alpha_i amp (-2 phi') (x_j - X_i),    Gv += on c'_f w_f^2 o sum_i B_i amp (-2 phi') (x_j - X_i)
//      (da/dmean and da/dvar are known only after the last member)
// then the acquisition value, d(-a)/dx_j = da/dmean Gm - 2 da/dvar Gv (dk_i/dx_j = -amp (-2 phi') w^2 o (x_j - X_i)) reduced over the
// 16 row groups through LDS in a fixed order, and torch.optim.Adam's update by the owner of (j, dim) -- on the accumulated gradient
// when the caller's loop never zeroes it.
// A switched-off member adds exact zeros, so nothing of a point's arithmetic depends on its column, its tile or its neighbours' levels.
#include <climits>
#include <cmath>
#include <vector>

#include "acq_tile.h"

template <int DM>
__global__ __launch_bounds__(ACQ_T) void ffgp_stack_acq_kernel(AcqStackArgs a) {
  extern __shared__ double acq_lds[];
  AcqLoop c = a.c;
  acq_park_pointers(c);      // (acq_tile.h: the scalar file does not hold them beside the member table's fields)
  const int D = c.D;
  const size_t imgmax = (size_t)a.npmax * 16;
  double* img0 = acq_lds;                                                 // K_s, then B = Sigma^-1 K_s
  double* img1 = img0 + imgmax;                                           // V = L^-1 K_s; after the members the gradient partials
  double* img2 = img1 + (imgmax > (size_t)256 * DM ? imgmax : (size_t)256 * DM);   // amp (-2 phi'), 0 on the clamp
  double* Xs = img2 + imgmax;
  double* al = Xs + (size_t)a.npmax * DM;
  double* xq = al + a.npmax;
  double* w2 = xq + 16 * DM;
  double* redm = w2 + DM;
  double* redv = redm + 256;

  const int tid = threadIdx.x, j = tid & 15, rg = tid >> 4;
  const int q0 = blockIdx.x * ACQ_TILE;
  // this column's level, and the number of members the tile needs: the same for every thread of the workgroup (the columns of a
  // ragged last tile repeat the last point)
  int lev = a.F - 1, fcount = a.F;
  if (c.level) {
    lev = min(c.level[min(q0 + j, c.Q - 1)], a.F - 1);
    int top = -1;
    for (int cc = 0; cc < ACQ_TILE; ++cc) top = max(top, c.level[min(q0 + cc, c.Q - 1)]);
    fcount = min(top, a.F - 1) + 1;
  }
  AcqOwner o = acq_owner_load<DM>(c, xq, tid);
  __syncthreads();
  acq_park_constants(c);

  const int iters = c.steps > 0 ? c.steps : 1;
  for (int k = 0; k < iters; ++k) {
    double xj[DM], Gm[DM], Gv[DM];
#pragma unroll
    for (int dd = 0; dd < DM; ++dd) {
      xj[dd] = xq[j * DM + dd];
      Gm[dd] = 0.0;
      Gv[dd] = 0.0;
    }
    double mean = 0.0, var = 0.0;
    for (int f = 0; f < fcount; ++f) {
      const AcqStackMember& mb = a.m[f];
      const int n = mb.n, np = mb.np, nb = np >> 4, kfun = mb.kfun;
      const double amp = acq_in_vgpr(mb.amp[0]), clamp = acq_in_vgpr(mb.clamp), rinv = acq_in_vgpr(mb.rinv), vadd = acq_in_vgpr(mb.var_add);
      const double* const mX = acq_in_vgpr(mb.X);
      const double* const malpha = acq_in_vgpr(mb.alpha);
      const double* const mw = acq_in_vgpr(mb.w);
      const bool on = f <= lev;
      const double cm = on ? mb.mean_coef : 0.0, cv = on ? mb.var_coef : 0.0;

      // ---- 0. this member's X, alpha, w^2 (the previous member's gradient pass has to be done with them)
      __syncthreads();
      acq_load_rows<DM>(Xs, al, mX, malpha, n, np, D, tid);
      acq_load_w2<DM>(w2, mw, D, tid);
      __syncthreads();

      // ---- 1. K_s, derivative factors, mean_f (every row below np_f is written)
      double msum = 0.0;
      for (int p = 0; p < nb; ++p) {
        const int i = 16 * p + rg;
        const double s = acq_sqdist<DM>(Xs + i * DM, xj, w2);
        const double sc = fmax(s, clamp);
        const bool in = i < n;
        const double kv = in ? amp * ffgp_kfun_val(kfun, rinv, sc) : 0.0;
        img0[i * 16 + j] = kv;
        img2[i * 16 + j] = (in && s >= clamp) ? amp * ffgp_kfun_m2d(kfun, rinv, sc) : 0.0;
        msum = __builtin_fma(kv, al[i], msum);
      }
      const double mf = acq_rowgroup_sum(redm, msum, rg, j);

      // ---- 2. V = L^-1 K_s, |V_j|^2;  3. B = L^-T V (into the image of K_s)
      const double vv = acq_solve_images(mb.Linv, np, nb, img0, img1, redv, tid);
      __syncthreads();

      // ---- 4. the member's share of mean, variance and the two gradient partials
      mean = __builtin_fma(cm, mf, mean);
      var = __builtin_fma(cv, amp - vv + vadd, var);      // phi(0) = 1 for every radial profile
      for (int p = 0; p < nb; ++p) {
        const int i = 16 * p + rg;
        const double dk = img2[i * 16 + j];
        const double wm = cm * al[i] * dk, wv = cv * img0[i * 16 + j] * dk;
#pragma unroll
        for (int dd = 0; dd < DM; ++dd) {
          const double t = w2[dd] * (xj[dd] - Xs[i * DM + dd]);
          Gm[dd] = __builtin_fma(wm, t, Gm[dd]);
          Gv[dd] = __builtin_fma(wv, t, Gv[dd]);
        }
      }
    }

    // ---- the acquisition value and its derivatives with respect to mean and variance
    double av, gm, gv;
    acq_value(c.acq, mean, var, c.var_floor, c.kappa, c.xi, c.f_best, av, gm, gv);
    // the last member's V has been read (the barrier after stage 3): its image takes the partials of d(-a)/dx
#pragma unroll
    for (int dd = 0; dd < DM; ++dd) img1[(rg * DM + dd) * 16 + j] = gm * Gm[dd] - 2.0 * gv * Gv[dd];
    __syncthreads();

    // ---- outputs and Adam, by the owner of (j, rg)
    if (o.owner) acq_owner_step<DM>(c, o, xq, k, iters, av, acq_partial_sum<DM>(img1, rg, j), tid);
    __syncthreads();
  }
  acq_owner_store(c, o, tid);
}

static int acq_stack_launch_by_d(ffgp_handle* h, const AcqStackArgs& a, int grid, const AcqTrees&) {
  return acq_by_dm(a.c.D, [&](auto dm) { return acq_launch<dm()>(h, ffgp_stack_acq_kernel<dm()>, acq_lds_doubles, a.npmax, a, grid); });
}

// member p's kernel as a leaf record: its tree (checked by the entry), or the one leaf of its own radial kernel
AcqMemberTree acq_member_tree(const ffgp_acq_member& p, const ffgp_ktree* t) {
  AcqMemberTree r = {};
  r.nl = t ? t->n_leaves : 1;
  r.shape = (t && t->n_leaves == 4) ? t->shape : FFGP_TREE_CHAIN;
  for (int i = 0; i < 3; ++i) r.op[i] = (t && i + 1 < t->n_leaves) ? t->op[i] : FFGP_KOP_SUM;
  for (int e = 0; e < r.nl; ++e) {
    AcqLeaf& k = r.k[e];
    if (t) {
      const ffgp_kdesc& d = t->leaf[e];
      k.w = d.w_dev; k.amp = d.amp_dev; k.center = (d.kfun == FFGP_KFUN_LINEAR) ? d.center_dev : nullptr;
      k.clamp = d.clamp_min; k.rinv = (d.kparam != 0.0) ? 1.0 / d.kparam : 1.0; k.kfun = d.kfun;
    } else {
      k.w = p.w_dev; k.amp = p.amp_dev; k.center = nullptr;
      k.clamp = p.clamp_min; k.rinv = (p.kparam != 0.0) ? 1.0 / p.kparam : 1.0; k.kfun = p.kfun;
    }
  }
  return r;
}

int acq_run(ffgp_handle* h, const ffgp_acq_stack* s, acq_launch_fn launch, double* Xq_dev, int Q, int steps, const ffgp_adam* opt, double* state_dev,
            long step0, double* trace_dev, double* hist_dev, double* grad_dev, const ffgp_ktree* const* trees, bool chain, bool leaf_table) {
  if (!h || !s || !Xq_dev || !trace_dev || Q <= 0 || steps < 0 || steps > FFGP_ACQ_MAX_STEPS || step0 < 0) return FFGP_ERR_ARG;
  if (steps > 0 && (!opt || !state_dev)) return FFGP_ERR_ARG;
  if (s->F < 1 || s->F > FFGP_ACQ_MAX_MEMBERS || !s->members) return FFGP_ERR_ARG;
  if (s->acq != FFGP_ACQ_UCB && s->acq != FFGP_ACQ_EI && s->acq != FFGP_ACQ_UCB_VAR) return FFGP_ERR_ARG;
  const int F = s->F, D = s->members[0].D;
  if (chain && D > FFGP_ACQ_MAX_D - 1) return FFGP_ERR_ARG;      // the members above the first take [x, mean below]: D + 1 inputs
  for (int f = 0; f < F; ++f) {
    const ffgp_acq_member& p = s->members[f];
    const bool tree = trees && trees[f];
    if (!p.X_dev || !p.L_dev || !p.alpha_dev || (!tree && (!p.w_dev || !p.amp_dev))) return FFGP_ERR_ARG;
    if (p.n < 1 || p.n > FFGP_ACQ_MAX_N || p.D < 1 || p.D > FFGP_ACQ_MAX_D || p.D != ((chain && f > 0) ? D + 1 : D) || p.d != 1) return FFGP_ERR_ARG;
    if (p.ldl < p.n || p.ldl > INT_MAX) return FFGP_ERR_ARG;
    if (!tree && (p.kfun < FFGP_KFUN_SE || p.kfun > FFGP_KFUN_RQ)) return FFGP_ERR_ARG;      // (the linear kernel's k(x, x) depends on x)
  }
  FFGP_HIP(hipSetDevice(h->device));
  const int iters = steps > 0 ? steps : 1;
  // workspace: [L_f^-1 (np_f x np_f, zero-padded), f = 0..F-1 | TRTRI scratch per member | bias corrections | leaf_table: the records]
  size_t xd = 0, td = 0;
  int npmax = 0;
  for (int f = 0; f < F; ++f) {
    const size_t n = (size_t)s->members[f].n, np = (size_t)ffgp_round_up((int)n, 16);
    xd += np * np;
    td += n * n / 4 + n * FFGP_NB + 16;
    npmax = (int)np > npmax ? (int)np : npmax;
  }
  FFGP_CHECK(ffgp_ensure_ws(h, (xd + td + 2 * (size_t)iters) * sizeof(double) + (leaf_table ? F * sizeof(AcqMemberTree) : 0)));
  double* X = h->ws;
  double* T = X + xd;
  double* bc_dev = T + td;
  FFGP_CHECK(ffgp_zero_async(h, X, xd * sizeof(double)));
  AcqStackArgs a;
  for (int f = 0; f < F; ++f) {
    const ffgp_acq_member& p = s->members[f];
    const int n = p.n, np = ffgp_round_up(n, 16);
    AcqStackMember& m = a.m[f];
    m.X = p.X_dev; m.Linv = X; m.alpha = p.alpha_dev; m.w = p.w_dev; m.amp = p.amp_dev;
    m.clamp = p.clamp_min; m.rinv = (p.kparam != 0.0) ? 1.0 / p.kparam : 1.0; m.var_add = p.var_add_all;
    m.mean_coef = p.mean_coef; m.var_coef = p.var_coef; m.n = n; m.np = np; m.kfun = p.kfun; m.pad = 0;
    // The handle's inverted diagonal blocks are rebuilt from each factor on every call: the blocks a factorisation leaves behind and the
    // ones ffgp_refresh_dinv forms from the finished factor differ by rounding, and which of the two the store holds depends on what else
    // the handle served in between -- a trajectory must depend on the factors alone (12 + 18 steps = 30 steps bit for bit).  It also
    // makes the call independent of the cached-inverse contract: the store is left keyed on the last L_dev with content that matches it.
    ffgp_invalidate(h);
    FFGP_CHECK(ffgp_trtri_impl(h, p.L_dev, n, (int)p.ldl, X, np, T));
    X += (size_t)np * np;
    T += (size_t)n * n / 4 + (size_t)n * FFGP_NB + 16;
  }
  for (int f = F; f < FFGP_ACQ_MAX_MEMBERS; ++f) a.m[f] = a.m[0];      // never read: the member loop ends at F
  std::vector<double> bc(2 * (size_t)iters, 1.0);
  ffgp_adam_bc_table(opt, step0, steps, bc.data());
  FFGP_HIP(hipMemcpyAsync(bc_dev, bc.data(), bc.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  std::vector<AcqMemberTree> table(leaf_table ? F : 0);      // (lives until the wait below, as bc does)
  AcqMemberTree* const table_dev = leaf_table ? reinterpret_cast<AcqMemberTree*>(bc_dev + bc.size()) : nullptr;
  if (leaf_table) {
    for (int f = 0; f < F; ++f) table[f] = acq_member_tree(s->members[f], trees ? trees[f] : nullptr);
    FFGP_HIP(hipMemcpyAsync(table_dev, table.data(), table.size() * sizeof(AcqMemberTree), hipMemcpyHostToDevice, h->stream));
  }
  AcqLoop& c = a.c;
  c.level = s->level_dev; c.bc = bc_dev;
  c.Xq = Xq_dev; c.state = state_dev; c.trace = trace_dev; c.hist = hist_dev; c.grad = grad_dev;
  a.F = F; a.npmax = npmax; c.D = D; c.Q = Q; c.steps = steps; c.acq = s->acq; c.accumulate = s->accumulate_grad ? 1 : 0; c.pad = 0;
  c.var_floor = s->var_floor; c.kappa = s->kappa; c.xi = s->xi; c.f_best = s->f_best;
  c.lr = opt ? opt->lr : 0.0; c.b1 = opt ? opt->beta1 : 0.0; c.b2 = opt ? opt->beta2 : 0.0; c.eps = opt ? opt->eps : 0.0;
  const int grid = (Q + ACQ_TILE - 1) / ACQ_TILE;
  FFGP_CHECK(launch(h, a, grid, AcqTrees{trees, table_dev}));
  FFGP_HIP(hipStreamSynchronize(h->stream));
  return FFGP_OK;
}

int ffgp_acq_optimize_stack(ffgp_handle* h, const ffgp_acq_stack* s, double* Xq_dev, int Q, int steps, const ffgp_adam* opt, double* state_dev,
                            long step0, double* trace_dev, double* hist_dev, double* grad_dev) {
  return acq_run(h, s, acq_stack_launch_by_d, Xq_dev, Q, steps, opt, state_dev, step0, trace_dev, hist_dev, grad_dev);
}
