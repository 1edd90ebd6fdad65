// The acquisition optimiser's Adam loop on a frozen posterior whose kernel is a COMPOSITION -- a SumKernel / ProductKernel tree of 2-4
// leaves, radial profiles and LinearKernel alike -- in one launch (ffgp_acq_optimize_tree, include/ffgp.h).
// Reference: Bayesian_optimization/cigp.py:119, GaussianProcess/cigp_v10.py:81 and the two-fidelity models run on
// SumKernel(LinearKernel(1), MaternKernel(1)); the loop is Bayesian_optimization/acq.py:48-68.  The plan is ffgp_acq_kernel's (acq.hip):
// a 256-thread workgroup owns 16 query points and runs all the steps, V = L^-1 K_s and B = L^-T V are acq_tile.h's block chains on
// [np][16] LDS images.  What differs:
//   * k(X_i, x_j) is the tree of the leaves' values, its nodes rounded one by one as pair.hip's tree_op rounds them (tree_ops.h);
//   * there is no derivative image: up to four leaves' factors do not fit beside the three images, so the gradient pass re-evaluates the
//     leaves from Xs (stage 1's arithmetic again, small beside the two chain passes) and runs the tree's reverse sweep per row.  Two
//     images remain: K_s -> B, and V -> the gradient partials;
//   * the leaves' length scales differ, so w_e^2 is folded into every term before the row sum; da/dmean and da/dvar are known before
//     the gradient pass, so a thread still carries ONE partial of DM doubles;
//   * k(x, x) depends on x through the linear leaves: var = k(x, x) - |V|^2 + var_add, and the owner of (j, dim) adds
//     -(da/dvar) dk(x, x)/dx to the loss gradient.  A radial leaf's self value amp phi(max(0, clamp)) is a constant.
// Per-row derivative of leaf e with respect to x_j (dk/dv_e from the reverse sweep in front):
//     radial:  -amp_e (-2 phi_e'(s_e)) w_e^2 o (x_j - X_i), zero where s_e < clamp_e;      linear:  amp_e w_e^2 o (X_i - c_e)
// Nothing of a point's arithmetic depends on its column or tile: a point run alone follows the same trajectory bit for bit.
#include <climits>

#include "acq_tile.h"
#include "tree_ops.h"

#define ACQ_TREE_MAX FFGP_TREE_LEAVES

struct AcqTreeArgs {
  AcqStackMember m;      // X, Linv, alpha, n, np, var_add of the one posterior; its kernel is the tree below
  AcqLoop c;
  AcqLeaf k[ACQ_TREE_MAX];
  int nl, shape, op[3];
};

// LDS in doubles: two [np][16] images (the second at least 256 DM: it also carries the gradient partials), X [np][DM], alpha [np], the
// tile's points [16][DM], per leaf w^2 [DM] and centre [DM], per leaf (amp, clamp, 1 / kparam, self value) [4], two [16][16] reduction pads
static constexpr size_t acq_tree_lds_doubles(int np, int DM) {
  const size_t img = (size_t)np * 16, img1 = img > (size_t)256 * DM ? img : (size_t)256 * DM;
  return img + img1 + (size_t)np * DM + np + 16 * DM + 2 * ACQ_TREE_MAX * DM + 4 * ACQ_TREE_MAX + 512;
}
static_assert(acq_tree_lds_doubles(FFGP_ACQ_MAX_N, FFGP_ACQ_MAX_D) * sizeof(double) <= 160 * 1024,
              "the tree acquisition kernel's LDS exceeds a CU's 160 KiB");

// a leaf's bilinear form on (training row xr, query point xj): the squared scaled distance, or the scaled dot product about the centre
template <int DM>
__device__ __forceinline__ double acq_tree_form(bool lin, const double* xr, const double (&xj)[DM], const double* w2, const double* cen) {
  if (!lin) return acq_sqdist<DM>(xr, xj, w2);
  double s = 0.0;
#pragma unroll
  for (int dd = 0; dd < DM; ++dd) s = __builtin_fma(w2[dd] * (xj[dd] - cen[dd]), xr[dd] - cen[dd], s);
  return s;
}

template <int DM>
__global__ __launch_bounds__(ACQ_T) void ffgp_tree_acq_kernel(AcqTreeArgs a) {
  extern __shared__ double acq_lds[];
  const AcqLoop& c = a.c;
  const int np = a.m.np, nb = np >> 4, n = a.m.n, D = c.D, nl = a.nl;
  const size_t img = (size_t)np * 16;
  double* img0 = acq_lds;                                              // K_s, then B = Sigma^-1 K_s
  double* img1 = img0 + img;                                           // V = L^-1 K_s, then the gradient partials
  double* Xs = img1 + (img > (size_t)256 * DM ? img : (size_t)256 * DM);
  double* al = Xs + (size_t)np * DM;
  double* xq = al + np;
  double* w2 = xq + 16 * DM;                                           // [leaf][DM]
  double* cen = w2 + ACQ_TREE_MAX * DM;                                // [leaf][DM]
  double* lp = cen + ACQ_TREE_MAX * DM;                                // [leaf][amp, clamp, 1 / kparam, radial self value]
  double* redm = lp + 4 * ACQ_TREE_MAX;
  double* redv = redm + 256;

  const int tid = threadIdx.x, j = tid & 15, rg = tid >> 4;
  bool lin[ACQ_TREE_MAX];
#pragma unroll
  for (int e = 0; e < ACQ_TREE_MAX; ++e) lin[e] = a.k[e].kfun == FFGP_KFUN_LINEAR;

  acq_load_rows<DM>(Xs, al, a.m.X, a.m.alpha, n, np, D, tid);
#pragma unroll
  for (int e = 0; e < ACQ_TREE_MAX; ++e) {
    if (e < nl) acq_load_w2<DM>(w2 + e * DM, a.k[e].w, D, tid);
    if (e < nl && tid < DM) cen[e * DM + tid] = (tid < D && lin[e] && a.k[e].center) ? a.k[e].center[tid] : 0.0;
    if (e < nl && tid == 0) {
      const double amp = a.k[e].amp[0];
      lp[4 * e] = amp;
      lp[4 * e + 1] = a.k[e].clamp;
      lp[4 * e + 2] = a.k[e].rinv;
      lp[4 * e + 3] = lin[e] ? 0.0 : amp * ffgp_kfun_val(a.k[e].kfun, a.k[e].rinv, fmax(0.0, a.k[e].clamp));
    }
  }
  AcqOwner o = acq_owner_load<DM>(c, xq, tid);
  __syncthreads();

  const int iters = c.steps > 0 ? c.steps : 1;
  for (int k = 0; k < iters; ++k) {
    // ---- 1. K_s, mean; k(x, x) and its reverse sweep
    double xj[DM];
#pragma unroll
    for (int dd = 0; dd < DM; ++dd) xj[dd] = xq[j * DM + dd];
    double msum = 0.0;
    for (int p = 0; p < nb; ++p) {
      const int i = 16 * p + rg;
      double v[ACQ_TREE_MAX];
#pragma unroll
      for (int e = 0; e < ACQ_TREE_MAX; ++e) {
        v[e] = 0.0;
        if (e < nl) {
          const double s = acq_tree_form<DM>(lin[e], Xs + i * DM, xj, w2 + e * DM, cen + e * DM);
          v[e] = lp[4 * e] * (lin[e] ? s : ffgp_kfun_val(a.k[e].kfun, lp[4 * e + 2], fmax(s, lp[4 * e + 1])));
        }
      }
      const double kv = (i < n) ? ffgp_tree_eval(a, v) : 0.0;
      img0[i * 16 + j] = kv;
      msum = __builtin_fma(kv, al[i], msum);
    }
    double sv[ACQ_TREE_MAX], gs[ACQ_TREE_MAX];
#pragma unroll
    for (int e = 0; e < ACQ_TREE_MAX; ++e) {
      sv[e] = 0.0;
      if (e < nl) {
        sv[e] = lp[4 * e + 3];
        if (lin[e]) {
          double s = 0.0;
#pragma unroll
          for (int dd = 0; dd < DM; ++dd) {
            const double df = xj[dd] - cen[e * DM + dd];
            s = __builtin_fma(w2[e * DM + dd] * df, df, s);
          }
          sv[e] = lp[4 * e] * s;
        }
      }
    }
    const double kss = ffgp_tree_eval(a, sv);
    ffgp_tree_back(a, sv, gs);
    const double mean = acq_rowgroup_sum(redm, msum, rg, j);

    // ---- 2. V = L^-1 K_s, |V_j|^2;  3. B = L^-T V (into the image of K_s)
    const double vv = acq_solve_images(a.m.Linv, np, nb, img0, img1, redv, tid);

    // ---- 4. the acquisition value and its derivatives with respect to mean and variance
    const double var = kss - vv + a.m.var_add;
    double av, gm, gv;
    acq_value(c.acq, mean, var, c.var_floor, c.kappa, c.xi, c.f_best, av, gm, gv);
    __syncthreads();

    // ---- the input gradient: the leaves again from Xs, the reverse sweep per row; partial sums over this thread's rows, then over the
    //      16 row groups in a fixed order
    double ga[DM];
#pragma unroll
    for (int dd = 0; dd < DM; ++dd) ga[dd] = 0.0;
    for (int p = 0; p < nb; ++p) {
      const int i = 16 * p + rg;
      const double ci = (i < n) ? -(gm * al[i] - 2.0 * gv * img0[i * 16 + j]) : 0.0;
      double v[ACQ_TREE_MAX], dv[ACQ_TREE_MAX], gl[ACQ_TREE_MAX];
#pragma unroll
      for (int e = 0; e < ACQ_TREE_MAX; ++e) {
        v[e] = 0.0;
        dv[e] = 0.0;
        if (e < nl) {
          const double s = acq_tree_form<DM>(lin[e], Xs + i * DM, xj, w2 + e * DM, cen + e * DM);
          const double amp = lp[4 * e];
          if (lin[e]) {
            v[e] = amp * s;
            dv[e] = amp;
          } else {
            const double cl = lp[4 * e + 1], sc = fmax(s, cl);
            v[e] = amp * ffgp_kfun_val(a.k[e].kfun, lp[4 * e + 2], sc);
            dv[e] = (i < n && s >= cl) ? -(amp * ffgp_kfun_m2d(a.k[e].kfun, lp[4 * e + 2], sc)) : 0.0;
          }
        }
      }
      ffgp_tree_back(a, v, gl);
#pragma unroll
      for (int e = 0; e < ACQ_TREE_MAX; ++e) {
        if (e < nl) {
          const double wt = ci * gl[e] * dv[e];
          if (lin[e]) {
#pragma unroll
            for (int dd = 0; dd < DM; ++dd) ga[dd] = __builtin_fma(wt, w2[e * DM + dd] * (Xs[i * DM + dd] - cen[e * DM + dd]), ga[dd]);
          } else {
#pragma unroll
            for (int dd = 0; dd < DM; ++dd) ga[dd] = __builtin_fma(wt, w2[e * DM + dd] * (xj[dd] - Xs[i * DM + dd]), ga[dd]);
          }
        }
      }
    }
#pragma unroll
    for (int dd = 0; dd < DM; ++dd) img1[(rg * DM + dd) * 16 + j] = ga[dd];
    __syncthreads();

    // ---- 5. outputs and Adam, by the owner of (j, rg): the row sum, and the self term -(da/dvar) dk(x, x)/dx of the linear leaves
    if (o.owner) {
      double gx = acq_partial_sum<DM>(img1, rg, j);
      double ds = 0.0;
#pragma unroll
      for (int e = 0; e < ACQ_TREE_MAX; ++e)
        if (e < nl && lin[e]) ds = __builtin_fma(gs[e] * (2.0 * lp[4 * e]), w2[e * DM + rg] * (o.x - cen[e * DM + rg]), ds);
      gx -= gv * ds;
      acq_owner_step<DM>(c, o, xq, k, iters, av, gx, tid);
    }
    __syncthreads();
  }
  acq_owner_store(c, o, tid);
}

// the leaf table travels by value in the kernel's arguments
static int acq_tree_launch_by_d(ffgp_handle* h, const AcqStackArgs& s, int grid, const AcqTrees& trees) {
  const ffgp_ktree* t = trees.host[0];
  AcqTreeArgs a = {};
  a.m = s.m[0];
  a.c = s.c;
  for (int e = 0; e < ACQ_TREE_MAX; ++e) {
    const ffgp_kdesc& k = t->leaf[e < t->n_leaves ? e : 0];      // (the entries past the last leaf are never read)
    a.k[e].w = k.w_dev; a.k[e].amp = k.amp_dev; a.k[e].center = (k.kfun == FFGP_KFUN_LINEAR) ? k.center_dev : nullptr;
    a.k[e].clamp = k.clamp_min; a.k[e].rinv = (k.kparam != 0.0) ? 1.0 / k.kparam : 1.0; a.k[e].kfun = k.kfun; a.k[e].pad = 0;
  }
  a.nl = t->n_leaves; a.shape = (t->n_leaves == 4) ? t->shape : FFGP_TREE_CHAIN;
  for (int i = 0; i < 3; ++i) a.op[i] = (i + 1 < t->n_leaves) ? t->op[i] : FFGP_KOP_SUM;
  return acq_by_dm(s.c.D, [&](auto dm) { return acq_launch<dm()>(h, ffgp_tree_acq_kernel<dm()>, acq_tree_lds_doubles, a.m.np, a, grid); });
}

// The tree is checked here; everything else -- the remaining checks, the workspace, the triangular inverse, the bias corrections,
// launch and wait -- is the stack entry's driver on a stack of one member (acq_run, acq_stack.hip), told that the member's kernel is `tree`.
int ffgp_acq_optimize_tree(ffgp_handle* h, const ffgp_acq_tree_problem* p, double* Xq_dev, int Q, int steps, const ffgp_adam* opt,
                           double* state_dev, long step0, double* trace_dev, double* hist_dev, double* grad_dev) {
  if (!p || (p->acq != FFGP_ACQ_UCB && p->acq != FFGP_ACQ_EI)) return FFGP_ERR_ARG;      // FFGP_ACQ_UCB_VAR: the stack entry only
  const ffgp_ktree* t = p->tree;
  if (!t || !acq_tree_ok(t)) return FFGP_ERR_ARG;
  ffgp_acq_member m = {};
  m.n = p->n; m.D = p->D; m.d = p->d;
  m.X_dev = p->X_dev; m.L_dev = p->L_dev; m.ldl = p->ldl; m.alpha_dev = p->alpha_dev;
  m.var_add_all = p->var_add_all; m.mean_coef = 1.0; m.var_coef = 1.0;
  ffgp_acq_stack s = {};
  s.F = 1; s.members = &m; s.level_dev = nullptr;
  s.var_floor = p->var_floor; s.acq = p->acq; s.kappa = p->kappa; s.xi = p->xi; s.f_best = p->f_best; s.accumulate_grad = 0;
  return acq_run(h, &s, acq_tree_launch_by_d, Xq_dev, Q, steps, opt, state_dev, step0, trace_dev, hist_dev, grad_dev, &t);
}
