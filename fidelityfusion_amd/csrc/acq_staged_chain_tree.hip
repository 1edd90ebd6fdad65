// The staged acquisition loop on a CHAIN of frozen posteriors whose members may carry COMPOSED kernels, past the one-launch kernel's
// LDS-tile limit (ffgp_acq_optimize_chain_tree_staged, include/ffgp.h).  Reference: the two-fidelity NAR is built on
// SumKernel(LinearKernel, MaternKernel) on both fidelities (FidelityFusion_Models/two_fidelity_models/NAR_NonlinearAR.py:23-26), NAR's
// demo trains on 300 / 300 / 250 points (FidelityFusion_Models/NAR.py:119-128), and the loop is
// MF_BayesianOptimization/Discrete/DMF_acq.py:226-262.  The model, the arguments and the outputs are ffgp_acq_optimize_chain_tree's
// (acq_chain_tree.hip).  The step loop is acq_staged_chain.hip's: the members in sequence, one launch per member and stage, the census
// of the levels once per call (acq_staged_chain_census), 3 (top + 1) + 2 |tops| + 2 launches per step.  The per-row work is
// acq_staged_tree.hip's: the member's leaf record copied into LDS, K_s = the tree on the leaves' values, no derivative image -- the
// gradient tiles evaluate the leaves again and run the tree's reverse sweep per row, each leaf's own w^2 per term.  The prologue, the
// GEMMs, the column sums and the owner kernel are acq_staged.hip's (acq_staged.h).
//
// What neither staged parent has is where they meet (acq_chain_tree.hip derives it): in a chain a linear leaf sees the lower member's
// mean u as coordinate D of z = [x, u], so k_s(z, z) depends on u and the variance's self term feeds the chain as well as x.  The value
// stage keeps, per point, S = dk_s(z, z)/dx (a.self, which the owner subtracts as gv S) and su = dk_s(z, z)/du; the gradient launch of
// member s - 1 reads gu = (member s's partials of slot D summed in chunk order) - gv su, in that order.
//   forward, f = 0 .. top
//     1. ffgp_acq_staged_chain_tree_ks_kernel     K_s,f through the tree on z_f = [x_q, u_q], u_q = the chunk sums of m_{f-1} in chunk order
//                                                 (asc_load_z: the expression the value stage reads); the columns Q..Qp-1 as zeros
//     2. as_solve_stage, only if f in tops;  3. as_col_stage
//   4. ffgp_acq_staged_chain_tree_value_kernel    per point, s = level: k_s(z_s, z_s) = the tree on the self values (linear: amp sum w^2
//                                                 (z - c)^2 over all D_s coordinates; a tree's radial leaf: amp phi(max(0, clamp)); a
//                                                 one-leaf member: amp), var = k_s(z, z) - |V|^2 + var_add_s, acq_value, S and su
//   reverse, f = top .. 0
//     5. ffgp_acq_staged_chain_tree_grad_kernel   the upstream on k_i is acq_staged_chain.hip's select (level == f: gm alpha_i - 2 gv B_iq;
//                                                 level > f: -gu alpha_i; otherwise an exact 0); slot D of part[f] is this member's
//                                                 contribution to d(-a)/dm_{f-1}
//   6. as_owner_stage
// Every sum is taken in an order that depends on n alone (chunk order, member order); no atomics.  The templates are chosen on D + 1.
#include <climits>
#include <cmath>

#include "acq_staged.h"

// ---- 1. K_s of member f through its tree on z_f; the columns Q..Qp-1 are written as zeros
template <int DM>
__global__ __launch_bounds__(AS_T) void ffgp_acq_staged_chain_tree_ks_kernel(AcqStagedArgs a, int f) {
  __shared__ double Xs[AS_ROWS * DM];
  __shared__ double w2[AST_NL * DM], cen[AST_NL * DM], lp[4 * AST_NL];
  const AcqStagedMember& mb = a.m[f];
  const int n = mb.n, r0 = blockIdx.y * AS_ROWS;
  if (r0 >= n) return;
  const AcqMemberTree& mt = a.tab[f];
  const int rows = min(AS_ROWS, n - r0), tid = threadIdx.x, Df = f ? a.D + 1 : a.D, nl = mt.nl;
  asc_load_rows<DM>(Xs, mb.X, r0, rows, Df, tid);
  ast_load_record<DM>(mt, Df, tid, w2, cen, lp);
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
  asc_load_z<DM>(xj, a, f, q, live);
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

// ---- 4. per point, the member s it stops at: the mean, k_s(z, z) through the tree, the acquisition value and its two derivatives, and
// the self term's two shares S[q][dd < D] = dk_s(z, z)/dx_dd and su[q] = dk_s(z, z)/du (0 for s = 0).  A negative level stops at no
// member: value 0, gm = gv = 0, S = 0, su = 0.
__global__ __launch_bounds__(AS_T) void ffgp_acq_staged_chain_tree_value_kernel(AcqStagedArgs a, double* su) {
  const int q = blockIdx.x * AS_T + threadIdx.x;
  if (q >= a.Q) return;
  const int lev = as_level(a, q), D = a.D;
  const double* x = a.Xq + (size_t)q * D;
  double* S = a.self + (size_t)q * D;
  double av = 0.0, gm = 0.0, gv = 0.0, dsu = 0.0;
  if (lev < 0) {
    for (int dd = 0; dd < D; ++dd) S[dd] = 0.0;
  } else {
    const AcqStagedMember& mb = a.m[lev];
    const AcqMemberTree& mt = a.tab[lev];
    const int nl = mt.nl, Ds = lev ? D + 1 : D;
    const double mean = asc_chunk_sum(a.pm, a, lev, q), vv = asc_chunk_sum(a.pv, a, lev, q);
    const double u = lev ? asc_chunk_sum(a.pm, a, lev - 1, q) : 0.0;      // the expression the K_s stage fed forward
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
          for (int dd = 0; dd < Ds; ++dd) {
            const double wv = k.w[dd], df = (dd < D ? x[dd] : u) - (k.center ? k.center[dd] : 0.0);
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
    acq_value(a.acq, mean, kss - vv + mb.var_add, a.var_floor, a.kappa, a.xi, a.f_best, av, gm, gv);
    for (int dd = 0; dd < Ds; ++dd) {
      double ds = 0.0;
#pragma unroll
      for (int e = 0; e < AST_NL; ++e)
        if (e < nl && lin[e]) {
          const AcqLeaf& k = mt.k[e];
          const double wv = k.w[dd];
          ds = __builtin_fma(gs[e] * (2.0 * amp[e]), wv * wv * ((dd < D ? x[dd] : u) - (k.center ? k.center[dd] : 0.0)), ds);
        }
      if (dd < D)
        S[dd] = ds;
      else
        dsu = ds;
    }
  }
  a.av[q] = av;
  a.gm[q] = gm;
  a.gv[q] = gv;
  su[q] = dsu;
}

// ---- 5. member f's share of the input gradient, as chunk sums over the coordinates of z_f.  The upstream on k_i and each leaf's
// -dv_e/dz carry opposite signs, as in acq_staged_tree.hip: -dv_e/dz is amp (-2 phi') w_e^2 o (z - Z_i) for a radial leaf (zero below its
// clamp) and amp w_e^2 o (c_e - Z_i) for a linear one, over all D_f coordinates.  Slot D is this member's contribution to
// d(-a)/dm_{f-1}, which the launch of member f - 1 reads as gu.
template <int DM>
__global__ __launch_bounds__(AS_T) void ffgp_acq_staged_chain_tree_grad_kernel(AcqStagedArgs a, int f, const double* su) {
  __shared__ double Xs[AS_ROWS * DM];
  __shared__ double al[AS_ROWS];
  __shared__ double w2[AST_NL * DM], cen[AST_NL * DM], lp[4 * AST_NL];
  __shared__ double red[AS_LANES][AS_COLS * DM];
  const AcqStagedMember& mb = a.m[f];
  const int n = mb.n, r0 = blockIdx.y * AS_ROWS;
  if (r0 >= n) return;
  const AcqMemberTree& mt = a.tab[f];
  const int rows = min(AS_ROWS, n - r0), tid = threadIdx.x, D = a.D, Df = f ? D + 1 : D, nl = mt.nl;
  asc_load_rows<DM>(Xs, mb.X, r0, rows, Df, tid);
  for (int i = tid; i < rows; i += AS_T) al[i] = mb.alpha[r0 + i];
  ast_load_record<DM>(mt, Df, tid, w2, cen, lp);
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
  asc_load_z<DM>(xj, a, f, q, live);
#pragma unroll
  for (int dd = 0; dd < DM; ++dd) G[dd] = 0.0;
  const int lev = live ? as_level(a, q) : -1;
  const bool top = lev == f, below = lev > f;
  double gm = 0.0, gv2 = 0.0, gu = 0.0;
  if (top) {
    gm = a.gm[q];
    gv2 = 2.0 * a.gv[q];
  }
  if (below) {      // member f + 1 <= level has run before this launch: its chunk sums first, then the self term of the point's own member
    const int nch = as_chunks(a.m[f + 1].n);
    for (int ch = 0; ch < nch; ++ch) gu += a.part[(((size_t)(f + 1) * a.nch + ch) * a.Qp + q) * DM + D];
    if (lev == f + 1) gu = gu - a.gv[q] * su[q];
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
    const double up = top ? gm * al[i] - gv2 * mb.B[(size_t)(r0 + i) * a.Qp + q] : -gu * al[i];
    const double ci = (top || below) ? up : 0.0;      // a select, not a product: a switched-off column may carry anything
#pragma unroll
    for (int e = 0; e < AST_NL; ++e) {
      if (e < nl) {
        const double wt = ci * (gl[e] * dv[e]);
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
static int asct_ks_launch(ffgp_handle* h, const AcqStagedArgs& a, dim3 grid, int f) {
  hipLaunchKernelGGL(ffgp_acq_staged_chain_tree_ks_kernel<DM>, grid, dim3(AS_T), 0, h->stream, a, f);
  return as_launched();
}
template <int DM>
static int asct_grad_launch(ffgp_handle* h, const AcqStagedArgs& a, dim3 grid, int f, const double* su) {
  hipLaunchKernelGGL(ffgp_acq_staged_chain_tree_grad_kernel<DM>, grid, dim3(AS_T), 0, h->stream, a, f, su);
  return as_launched();
}
// the templates are chosen on D + 1, the upper members' input dimension, as the one-launch chain entries choose (a.DM holds it)
static int asct_ks_stage(ffgp_handle* h, const AcqStagedArgs& a, dim3 tiles, int f) {
  return acq_by_dm(a.D + 1, [&](auto dm) { return asct_ks_launch<dm()>(h, a, tiles, f); });
}
static int asct_grad_stage(ffgp_handle* h, const AcqStagedArgs& a, dim3 tiles, int f, const double* su) {
  return acq_by_dm(a.D + 1, [&](auto dm) { return asct_grad_launch<dm()>(h, a, tiles, f, su); });
}
static int asct_value_stage(ffgp_handle* h, const AcqStagedArgs& a, double* su) {
  hipLaunchKernelGGL(ffgp_acq_staged_chain_tree_value_kernel, dim3((a.Q + AS_T - 1) / AS_T), dim3(AS_T), 0, h->stream, a, su);
  return as_launched();
}

// step k: a refused launch ends it there, before a later stage reads what it did not write
static int asct_step(ffgp_handle* h, const AcqStagedPlan& pl, int top, unsigned tops, double* su, int k) {
  const AcqStagedArgs& a = pl.a;
  int rc;
  for (int f = 0; f <= top; ++f) {
    const dim3 tiles(pl.qt, (a.m[f].n + AS_ROWS - 1) / AS_ROWS, 1);
    if ((rc = asct_ks_stage(h, a, tiles, f)) != FFGP_OK) return rc;
    if ((tops >> f) & 1u)
      if ((rc = as_solve_stage(h, pl, f)) != FFGP_OK) return rc;
    if ((rc = as_col_stage(h, a, tiles, f)) != FFGP_OK) return rc;
  }
  if ((rc = asct_value_stage(h, a, su)) != FFGP_OK) return rc;
  for (int f = top; f >= 0; --f) {
    const dim3 tiles(pl.qt, (a.m[f].n + AS_ROWS - 1) / AS_ROWS, 1);
    if ((rc = asct_grad_stage(h, a, tiles, f, su)) != FFGP_OK) return rc;
  }
  return as_owner_stage(h, pl, k);
}

// The coefficients and the trees are checked here, as ffgp_acq_optimize_chain_tree checks them; everything else the staged prologue
// refuses, told that the members above the first take one more input.  The entry's extra doubles: the census word, then su [Qp].
int ffgp_acq_optimize_chain_tree_staged(ffgp_handle* h, const ffgp_acq_chain* c, const ffgp_ktree* const* trees, double* Xq_dev, int Q, int steps,
                                        const ffgp_adam* opt, double* state_dev, long step0, double* trace_dev, double* hist_dev,
                                        double* grad_dev) {
  if (!c || !trees || c->F < 1 || c->F > FFGP_ACQ_MAX_MEMBERS) return FFGP_ERR_ARG;
  for (int f = 0; f < c->F; ++f) {
    if (c->members && (c->members[f].mean_coef != 1.0 || c->members[f].var_coef != 1.0)) return FFGP_ERR_ARG;
    if (trees[f] && !acq_tree_ok(trees[f])) return FFGP_ERR_ARG;
  }
  if (Q <= 0) return FFGP_ERR_ARG;
  ffgp_acq_stack s = {};
  s.F = c->F; s.members = c->members; s.level_dev = c->level_dev;
  s.var_floor = c->var_floor; s.acq = c->acq; s.kappa = c->kappa; s.xi = c->xi; s.f_best = c->f_best; s.accumulate_grad = c->accumulate_grad;
  const size_t Qp = ((size_t)Q + AS_COLS - 1) / AS_COLS * AS_COLS;
  AcqStagedPlan pl;
  FFGP_CHECK(acq_staged_prepare(h, &s, trees, 3, true, 1 + Qp, Xq_dev, Q, steps, opt, state_dev, step0, trace_dev, hist_dev, grad_dev, pl));
  double* const su = pl.extra + 1;
  unsigned tops;
  int top;
  int rc = acq_staged_chain_census(h, pl, tops, top);
  for (int k = 0; k < pl.iters && rc == FFGP_OK; ++k) rc = asct_step(h, pl, top, tops, su, k);
  return acq_staged_finish(h, rc);
}
