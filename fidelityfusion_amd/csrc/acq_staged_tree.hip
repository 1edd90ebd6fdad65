// The staged acquisition loop (acq_staged.hip: launch per stage, every step enqueued by one library call) for stacks whose members may
// carry COMPOSED kernels (ffgp_acq_optimize_stack_tree_staged, include/ffgp.h).  Reference: the Bayesian-optimisation model is cigp on
// SumKernel(LinearKernel, MaternKernel) (Bayesian_optimization/cigp.py:119), the two-fidelity AR and ResGP put that kernel on every
// fidelity (two_fidelity_models/AR_autoRegression.py:31-34, ResGP.py:25-28), and a run that appends a point per iteration passes the
// one-launch kernels' 256 training points on its own.  The mathematics, the argument structs and the output layouts are
// ffgp_acq_optimize_stack_tree's (acq_stack_tree.hip); the plan, the tile, the driver, the column-sum kernel and the owner kernel are
// acq_staged.hip's (acq_staged_run, acq_staged.h).  This file holds the three stages that differ, still 5 + 2 F launches per step:
//   1. ffgp_acq_staged_tree_ks_kernel     K_s,f = tree_f on the leaves' values at (X_f,i, x_q), all members in one launch.  The workgroup
//                                         copies its member's leaf record (w^2, centres, amp / clamp / 1 / kparam per leaf, zeros past nl)
//                                         from the table in handle workspace into LDS.  A member with one radial kernel is the one-leaf
//                                         record: the two-leaf sum whose second value is an exact 0.0 (acq_stack_tree.hip).
//   4. ffgp_acq_staged_tree_value_kernel  per point and member k_f(x, x) = tree_f on the self values -- linear: amp sum w^2 (x - c)^2; a
//                                         tree's radial leaf: amp phi(max(0, clamp)); a one-leaf member: amp -- var += c'_f (k_f(x, x) -
//                                         |V|^2 + var_add_f), acq_value, and S = sum_f c'_f dk_f(x, x)/dx from the tree's reverse sweep
//   5. ffgp_acq_staged_tree_grad_kernel   there is no derivative image: the leaves of each row are evaluated again from the chunk's X in
//                                         LDS, ffgp_tree_back gives dk/dv_e, and u_iq = da/dmean c_f alpha_i - 2 da/dvar c'_f B_iq times
//                                         sum_e (dk/dv_e) (-dv_e/dx_q) goes straight into the running sums: -dv_e/dx_q is
//                                         amp (-2 phi') w_e^2 o (x_q - X_i) for a radial leaf (zero below its clamp) and
//                                         amp w_e^2 o (c_e - X_i) for a linear one; every leaf has its own w^2, so it is applied per term
// The owner (acq_staged.hip) adds the partials in the order (member, chunk) and then -da/dvar S.  Three images per member (K_s, V, B)
// where the radial entry keeps four.
#include <climits>

#include "acq_staged.h"

// ---- 1. K_s through the tree; the columns Q..Qp-1 are written as zeros
template <int DM>
__global__ __launch_bounds__(AS_T) void ffgp_acq_staged_tree_ks_kernel(AcqStagedArgs a) {
  __shared__ double Xs[AS_ROWS * DM];
  __shared__ double w2[AST_NL * DM], cen[AST_NL * DM], lp[4 * AST_NL];
  const AcqStagedMember& mb = a.m[blockIdx.z];
  const int n = mb.n, r0 = blockIdx.y * AS_ROWS;
  if (r0 >= n) return;
  const AcqMemberTree& mt = a.tab[blockIdx.z];
  const int rows = min(AS_ROWS, n - r0), tid = threadIdx.x, D = a.D, nl = mt.nl;
  for (int idx = tid; idx < rows * DM; idx += AS_T) {
    const int i = idx / DM, dd = idx % DM;
    Xs[idx] = (dd < D) ? mb.X[(size_t)(r0 + i) * D + dd] : 0.0;
  }
  ast_load_record<DM>(mt, D, tid, w2, cen, lp);
  __syncthreads();
  const AstTree tr = ast_tree(mt);
  int kf[AST_NL];
  bool lin[AST_NL];
#pragma unroll
  for (int e = 0; e < AST_NL; ++e) {
    kf[e] = (e < nl) ? mt.k[e].kfun : FFGP_KFUN_SE;
    lin[e] = kf[e] == FFGP_KFUN_LINEAR;
  }
  const int q = blockIdx.x * AS_COLS + (tid & 63), lane = tid >> 6;
  const bool live = q < a.Q;
  double xj[DM];
#pragma unroll
  for (int dd = 0; dd < DM; ++dd) xj[dd] = (live && dd < D) ? a.Xq[(size_t)q * D + dd] : 0.0;
  for (int i = lane; i < rows; i += AS_LANES) {
    const double* xr = Xs + i * DM;
    double v[AST_NL];
#pragma unroll
    for (int e = 0; e < AST_NL; ++e) {
      v[e] = 0.0;
      if (e < nl) {
        const int o = e * DM + ast_opaque0();
        const double *w2e = w2 + o, *ce = cen + o;
        double s = 0.0;
        if (lin[e]) {
#pragma unroll
          for (int dd = 0; dd < DM; ++dd) s = __builtin_fma(w2e[dd] * (xj[dd] - ce[dd]), xr[dd] - ce[dd], s);
        } else {
          s = ffgp_kfun_val(kf[e], lp[4 * e + 2], fmax(acq_sqdist<DM>(xr, xj, w2e), lp[4 * e + 1]));
        }
        v[e] = lp[4 * e] * s;
      }
    }
    mb.Ks[(size_t)(r0 + i) * a.Qp + q] = live ? ffgp_tree_eval(tr, v) : 0.0;
  }
}

// ---- 4. mean, variance with k_f(x, x) through the tree, the acquisition value and its two derivatives, and the self gradient S, per point
__global__ __launch_bounds__(AS_T) void ffgp_acq_staged_tree_value_kernel(AcqStagedArgs a) {
  const int q = blockIdx.x * AS_T + threadIdx.x;
  if (q >= a.Q) return;
  const int lev = as_level(a, q), D = a.D;
  const double* x = a.Xq + (size_t)q * D;
  double* S = a.self + (size_t)q * D;
  double mean = 0.0, var = 0.0;
  for (int f = 0; f < a.F; ++f) {
    const AcqStagedMember& mb = a.m[f];
    const AcqMemberTree& mt = a.tab[f];
    const int nch = as_chunks(mb.n), nl = mt.nl;
    double mf = 0.0, vv = 0.0;
    for (int ch = 0; ch < nch; ++ch) {
      const size_t e = ((size_t)f * a.nch + ch) * a.Qp + q;
      mf += a.pm[e];
      vv += a.pv[e];
    }
    const bool on = f <= lev;
    const double cm = on ? mb.mean_coef : 0.0, cv = on ? mb.var_coef : 0.0;
    // the self values: a radial member amp (phi(0) = 1, what the radial entries take), a tree's radial leaf amp phi(max(0, clamp))
    double sv[AST_NL], gs[AST_NL], amp[AST_NL];
    bool lin[AST_NL];
#pragma unroll
    for (int e = 0; e < AST_NL; ++e) {
      sv[e] = 0.0;
      amp[e] = 0.0;
      lin[e] = false;
      if (e < nl) {
        const AcqLeaf& k = mt.k[e];
        amp[e] = k.amp[0];
        lin[e] = k.kfun == FFGP_KFUN_LINEAR;
        if (lin[e]) {
          double s = 0.0;
          for (int dd = 0; dd < D; ++dd) {
            const double wv = k.w[dd], df = x[dd] - (k.center ? k.center[dd] : 0.0);
            s = __builtin_fma(wv * wv * df, df, s);
          }
          sv[e] = amp[e] * s;
        } else {
          sv[e] = (nl == 1) ? amp[e] : amp[e] * ffgp_kfun_val(k.kfun, k.rinv, fmax(0.0, k.clamp));
        }
      }
    }
    const AstTree tr = ast_tree(mt);
    const double kss = ffgp_tree_eval(tr, sv);
    ffgp_tree_back(tr, sv, gs);
    mean = __builtin_fma(cm, mf, mean);
    var = __builtin_fma(cv, kss - vv + mb.var_add, var);
    for (int dd = 0; dd < D; ++dd) {
      double ds = 0.0;
#pragma unroll
      for (int e = 0; e < AST_NL; ++e)
        if (e < nl && lin[e]) {
          const AcqLeaf& k = mt.k[e];
          const double wv = k.w[dd];
          ds = __builtin_fma(gs[e] * (2.0 * amp[e]), wv * wv * (x[dd] - (k.center ? k.center[dd] : 0.0)), ds);
        }
      S[dd] = __builtin_fma(cv, ds, f == 0 ? 0.0 : S[dd]);
    }
  }
  double av, gm, gv;
  acq_value(a.acq, mean, var, a.var_floor, a.kappa, a.xi, a.f_best, av, gm, gv);
  a.av[q] = av;
  a.gm[q] = gm;
  a.gv[q] = gv;
}

// ---- 5. the input gradient's chunk sums.  u_iq = da/dmean c_f alpha_i - 2 da/dvar c'_f B_iq is minus the upstream on k_i, and each leaf's
// -dv_e/dx_q carries the other sign: the two cancel.  The thread keeps x_q and the running sums; a leaf's term goes straight into them.
template <int DM>
__global__ __launch_bounds__(AS_T) void ffgp_acq_staged_tree_grad_kernel(AcqStagedArgs a) {
  __shared__ double Xs[AS_ROWS * DM];
  __shared__ double al[AS_ROWS];
  __shared__ double w2[AST_NL * DM], cen[AST_NL * DM], lp[4 * AST_NL];
  __shared__ double red[AS_LANES][AS_COLS * DM];
  const AcqStagedMember& mb = a.m[blockIdx.z];
  const int n = mb.n, r0 = blockIdx.y * AS_ROWS;
  if (r0 >= n) return;
  const AcqMemberTree& mt = a.tab[blockIdx.z];
  const int rows = min(AS_ROWS, n - r0), tid = threadIdx.x, D = a.D, f = blockIdx.z, nl = mt.nl;
  for (int idx = tid; idx < rows * DM; idx += AS_T) {
    const int i = idx / DM, dd = idx % DM;
    Xs[idx] = (dd < D) ? mb.X[(size_t)(r0 + i) * D + dd] : 0.0;
  }
  for (int i = tid; i < rows; i += AS_T) al[i] = mb.alpha[r0 + i];
  ast_load_record<DM>(mt, D, tid, w2, cen, lp);
  __syncthreads();
  const AstTree tr = ast_tree(mt);
  int kf[AST_NL];
  bool lin[AST_NL];
#pragma unroll
  for (int e = 0; e < AST_NL; ++e) {
    kf[e] = (e < nl) ? mt.k[e].kfun : FFGP_KFUN_SE;
    lin[e] = kf[e] == FFGP_KFUN_LINEAR;
  }
  const int c = tid & 63, lane = tid >> 6, q0 = blockIdx.x * AS_COLS, q = q0 + c;
  const bool live = q < a.Q;
  double xj[DM], G[DM];
#pragma unroll
  for (int dd = 0; dd < DM; ++dd) {
    xj[dd] = (live && dd < D) ? a.Xq[(size_t)q * D + dd] : 0.0;
    G[dd] = 0.0;
  }
  double cA = 0.0, cB = 0.0;
  if (live) {
    const bool on = f <= as_level(a, q);
    cA = a.gm[q] * (on ? mb.mean_coef : 0.0);
    cB = -2.0 * a.gv[q] * (on ? mb.var_coef : 0.0);
  }
  for (int i = lane; i < rows; i += AS_LANES) {
    const double* xr = Xs + i * DM;
    double v[AST_NL], dv[AST_NL], gl[AST_NL];
#pragma unroll
    for (int e = 0; e < AST_NL; ++e) {
      v[e] = 0.0;
      dv[e] = 0.0;
      if (e < nl) {
        const double amp = lp[4 * e];
        const int o = e * DM + ast_opaque0();
        const double *w2e = w2 + o, *ce = cen + o;
        if (lin[e]) {
          double s = 0.0;
#pragma unroll
          for (int dd = 0; dd < DM; ++dd) s = __builtin_fma(w2e[dd] * (xj[dd] - ce[dd]), xr[dd] - ce[dd], s);
          v[e] = amp * s;
          dv[e] = amp;
        } else {
          const double s = acq_sqdist<DM>(xr, xj, w2e), cl = lp[4 * e + 1], sc = fmax(s, cl);
          v[e] = amp * ffgp_kfun_val(kf[e], lp[4 * e + 2], sc);
          dv[e] = (s >= cl) ? amp * ffgp_kfun_m2d(kf[e], lp[4 * e + 2], sc) : 0.0;
        }
      }
    }
    ffgp_tree_back(tr, v, gl);
    const double u = cA * al[i] + cB * mb.B[(size_t)(r0 + i) * a.Qp + q];
#pragma unroll
    for (int e = 0; e < AST_NL; ++e) {
      if (e < nl) {
        const double wt = u * (gl[e] * dv[e]);
        const int o = e * DM + ast_opaque0();
        const double *w2e = w2 + o, *ce = cen + o;
        if (lin[e]) {
#pragma unroll
          for (int dd = 0; dd < DM; ++dd) G[dd] = __builtin_fma(wt, w2e[dd] * (ce[dd] - xr[dd]), G[dd]);
        } else {
#pragma unroll
          for (int dd = 0; dd < DM; ++dd) G[dd] = __builtin_fma(wt, w2e[dd] * (xj[dd] - xr[dd]), G[dd]);
        }
      }
    }
  }
#pragma unroll
  for (int dd = 0; dd < DM; ++dd) red[lane][c * DM + dd] = G[dd];
  __syncthreads();
  double* out = a.part + (((size_t)f * a.nch + blockIdx.y) * a.Qp + q0) * DM;
  for (int idx = tid; idx < AS_COLS * DM; idx += AS_T) {
    double s = 0.0;
#pragma unroll
    for (int l = 0; l < AS_LANES; ++l) s += red[l][idx];
    out[idx] = s;
  }
}

template <int DM>
static int ast_ks_launch(ffgp_handle* h, const AcqStagedArgs& a, dim3 grid) {
  hipLaunchKernelGGL(ffgp_acq_staged_tree_ks_kernel<DM>, grid, dim3(AS_T), 0, h->stream, a);
  return as_launched();
}
template <int DM>
static int ast_grad_launch(ffgp_handle* h, const AcqStagedArgs& a, dim3 grid) {
  hipLaunchKernelGGL(ffgp_acq_staged_tree_grad_kernel<DM>, grid, dim3(AS_T), 0, h->stream, a);
  return as_launched();
}
static int ast_ks_stage(ffgp_handle* h, const AcqStagedArgs& a, dim3 tiles) {
  return acq_by_dm(a.D, [&](auto dm) { return ast_ks_launch<dm()>(h, a, tiles); });
}
static int ast_value_stage(ffgp_handle* h, const AcqStagedArgs& a) {
  hipLaunchKernelGGL(ffgp_acq_staged_tree_value_kernel, dim3((a.Q + AS_T - 1) / AS_T), dim3(AS_T), 0, h->stream, a);
  return as_launched();
}
static int ast_grad_stage(ffgp_handle* h, const AcqStagedArgs& a, dim3 tiles) {
  return acq_by_dm(a.D, [&](auto dm) { return ast_grad_launch<dm()>(h, a, tiles); });
}

// The trees are checked here, as ffgp_acq_optimize_stack_tree checks them; everything else is the staged driver's (acq_staged_run).
int ffgp_acq_optimize_stack_tree_staged(ffgp_handle* h, const ffgp_acq_stack* s, const ffgp_ktree* const* trees, double* Xq_dev, int Q, int steps,
                                        const ffgp_adam* opt, double* state_dev, long step0, double* trace_dev, double* hist_dev,
                                        double* grad_dev) {
  if (!s || !trees || s->F < 1 || s->F > FFGP_ACQ_MAX_MEMBERS) return FFGP_ERR_ARG;
  for (int f = 0; f < s->F; ++f)
    if (trees[f] && !acq_tree_ok(trees[f])) return FFGP_ERR_ARG;
  static const AcqStagedStages stages = {3, ast_ks_stage, ast_value_stage, ast_grad_stage};
  return acq_staged_run(h, s, trees, stages, Xq_dev, Q, steps, opt, state_dev, step0, trace_dev, hist_dev, grad_dev);
}
