// The acquisition optimiser's Adam loop on a STACK of frozen posteriors whose members may carry COMPOSED kernels, in one launch
// (ffgp_acq_optimize_stack_tree, include/ffgp.h).  Reference: the two-fidelity AR and ResGP are built on
// SumKernel(LinearKernel(1), MaternKernel(1)) for both fidelities (FidelityFusion_Models/two_fidelity_models/AR_autoRegression.py:31-34,
// ResGP.py:25-28), and the multi-fidelity models take any kernel_list; the loop is MF_BayesianOptimization/Discrete/DMF_acq.py:226-262.
// The plan is ffgp_stack_acq_kernel's (acq_stack.hip): a workgroup owns 16 query points and runs all the steps, the member loop inside
// the step.  The per-row work is ffgp_tree_acq_kernel's (acq_tree.hip): k(X_i, x_j) is the tree of the leaves' values, and there is no
// derivative image -- two images, K_s -> B and V -> the gradient partials, sized by the largest member; the gradient pass
// re-evaluates the leaves from Xs and runs the tree's reverse sweep per row.  What is this kernel's own:
//   * stage 0 reloads, per member, X, alpha AND the member's leaf record (w^2, centres, leaf constants, self values) from the table in
//     handle workspace; every slot a later stage reads is written -- rows up to np_f, all DM columns, all four leaf slots (zeros past
//     nl) -- so nothing of the previous member survives;
//   * a member with one radial library kernel runs as the one-leaf record: the two-leaf sum whose second leaf is an exact 0.0 and
//     is never evaluated; its self value is amp (phi(0) = 1), as the radial stack kernel has it;
//   * da/dmean and da/dvar are known only after the last member, so the per-row vector t = -dk_i/dx_j = sum_e (dk_i/dv_e) (-dv_e/dx_j)
//     is formed once and added into BOTH running partials, Gm += (c_f alpha_i) t and Gv += (c'_f B_i) t;
//   * k_f(x, x) depends on x through the linear leaves: var += c'_f (k_f(x, x) - |V|^2 + var_add_f), and the owner of (j, dim) keeps
//     S = sum_f c'_f dk_f(x, x)/dx_dim across the members; the loss gradient is da/dmean Gm - 2 da/dvar Gv - da/dvar S.
// `on_f` = (f <= level_j) is an exact 0 / 1 factor on c_f and c'_f: a switched-off member adds exact zeros, so nothing of a point's
// arithmetic depends on its column, its tile, its neighbours or their levels.
#include <climits>

#include "acq_tile.h"

struct AcqStackTreeArgs {
  AcqStackArgs s;
  const AcqMemberTree* tab;      // [F] in handle workspace
};
// the tree that tree_ops.h evaluates: a one-leaf record as the sum of its leaf and 0.0 (exact)
struct AcqTreeShape {
  int nl, shape, op[3];
};

// LDS in doubles, sized by the largest member: two [np][16] images (the second at least 256 DM: it also carries the gradient partials),
// X [np][DM], alpha [np], the tile's points [16][DM], per leaf w^2 [DM] and centre [DM], per leaf (amp, clamp, 1 / kparam, self value)
// [4], two [16][16] reduction pads
static constexpr size_t acq_stack_tree_lds_doubles(int np, int DM) {
  const size_t img = (size_t)np * 16, img1 = img > (size_t)256 * DM ? img : (size_t)256 * DM;
  return img + img1 + (size_t)np * DM + np + 16 * DM + 2 * FFGP_TREE_LEAVES * DM + 4 * FFGP_TREE_LEAVES + 512;
}
static_assert(acq_stack_tree_lds_doubles(FFGP_ACQ_MAX_N, FFGP_ACQ_MAX_D) * sizeof(double) <= 160 * 1024,
              "the stack-of-trees acquisition kernel's LDS exceeds a CU's 160 KiB");

template <int DM>
__global__ __launch_bounds__(ACQ_T) void ffgp_stack_tree_acq_kernel(AcqStackTreeArgs a) {
  constexpr int NL = FFGP_TREE_LEAVES;
  extern __shared__ double acq_lds[];
  AcqLoop c = a.s.c;
  acq_park_pointers(c);
  const int D = c.D, F = a.s.F;
  const size_t imgmax = (size_t)a.s.npmax * 16;
  double* img0 = acq_lds;                                                 // K_s, then B = Sigma^-1 K_s
  double* img1 = img0 + imgmax;                                           // V = L^-1 K_s; after the members the gradient partials
  double* Xs = img1 + (imgmax > (size_t)256 * DM ? imgmax : (size_t)256 * DM);
  double* al = Xs + (size_t)a.s.npmax * DM;
  double* xq = al + a.s.npmax;
  double* w2 = xq + 16 * DM;                                              // [leaf][DM]
  double* cen = w2 + NL * DM;                                             // [leaf][DM]
  double* lp = cen + NL * DM;                                             // [leaf][amp, clamp, 1 / kparam, self value of a radial leaf]
  double* redm = lp + 4 * NL;
  double* redv = redm + 256;

  const int tid = threadIdx.x, j = tid & 15, rg = tid >> 4;
  const int q0 = blockIdx.x * ACQ_TILE;
  // this column's level, and the number of members the tile needs: the same for every thread of the workgroup (the columns of a
  // ragged last tile repeat the last point)
  int lev = F - 1, fcount = F;
  if (c.level) {
    lev = min(c.level[min(q0 + j, c.Q - 1)], F - 1);
    int top = -1;
    for (int cc = 0; cc < ACQ_TILE; ++cc) top = max(top, c.level[min(q0 + cc, c.Q - 1)]);
    fcount = min(top, F - 1) + 1;
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
    double mean = 0.0, var = 0.0, self = 0.0;      // self: the owner's sum_f c'_f dk_f(x, x)/dx of its dimension
    for (int f = 0; f < fcount; ++f) {
      const AcqStackMember& mb = a.s.m[f];
      const AcqMemberTree& mt = a.tab[f];
      const int n = mb.n, np = mb.np, nb = np >> 4, nl = mt.nl;
      const double vadd = acq_in_vgpr(mb.var_add);
      const double* const mX = acq_in_vgpr(mb.X);
      const double* const malpha = acq_in_vgpr(mb.alpha);
      const bool on = f <= lev;
      const double cm = on ? mb.mean_coef : 0.0, cv = on ? mb.var_coef : 0.0;
      AcqTreeShape tr;
      tr.nl = max(nl, 2); tr.shape = mt.shape; tr.op[0] = mt.op[0]; tr.op[1] = mt.op[1]; tr.op[2] = mt.op[2];
      int kf[NL];
      bool lin[NL];
#pragma unroll
      for (int e = 0; e < NL; ++e) {
        kf[e] = (e < nl) ? mt.k[e].kfun : FFGP_KFUN_SE;
        lin[e] = kf[e] == FFGP_KFUN_LINEAR;
      }

      // ---- 0. this member's X, alpha and leaf record (the previous member's gradient pass has to be done with them); all four leaf
      //      slots are written, zeros past nl
      __syncthreads();
      acq_load_rows<DM>(Xs, al, mX, malpha, n, np, D, tid);
#pragma unroll
      for (int e = 0; e < NL; ++e) {
        const bool live = e < nl;
        if (tid < DM) {
          const double wv = (live && tid < D) ? mt.k[e].w[tid] : 0.0;
          w2[e * DM + tid] = wv * wv;
          cen[e * DM + tid] = (live && tid < D && lin[e] && mt.k[e].center) ? mt.k[e].center[tid] : 0.0;
        }
        if (tid == 0) {
          const double amp = live ? mt.k[e].amp[0] : 0.0, cl = live ? mt.k[e].clamp : 0.0, ri = live ? mt.k[e].rinv : 1.0;
          lp[4 * e] = amp;
          lp[4 * e + 1] = cl;
          lp[4 * e + 2] = ri;
          // a radial member: amp (phi(0) = 1, what acq_stack.hip takes); a tree's radial leaf: amp phi(max(0, clamp)), acq_tree.hip's
          lp[4 * e + 3] = (!live || lin[e]) ? 0.0 : (nl == 1 ? amp : amp * ffgp_kfun_val(kf[e], ri, fmax(0.0, cl)));
        }
      }
      __syncthreads();

      // ---- 1. K_s and mean_f (every row below np_f is written); k_f(x, x) and its reverse sweep
      double msum = 0.0;
      for (int p = 0; p < nb; ++p) {
        const int i = 16 * p + rg;
        double v[NL];
#pragma unroll
        for (int e = 0; e < NL; ++e) {
          v[e] = 0.0;
          if (e < nl) {
            const double* xr = Xs + i * DM;
            double s = 0.0;
            if (lin[e]) {
#pragma unroll
              for (int dd = 0; dd < DM; ++dd) s = __builtin_fma(w2[e * DM + dd] * (xj[dd] - cen[e * DM + dd]), xr[dd] - cen[e * DM + dd], s);
            } else {
              s = ffgp_kfun_val(kf[e], lp[4 * e + 2], fmax(acq_sqdist<DM>(xr, xj, w2 + e * DM), lp[4 * e + 1]));
            }
            v[e] = lp[4 * e] * s;
          }
        }
        const double kv = (i < n) ? ffgp_tree_eval(tr, v) : 0.0;
        img0[i * 16 + j] = kv;
        msum = __builtin_fma(kv, al[i], msum);
      }
      double sv[NL], gs[NL];
#pragma unroll
      for (int e = 0; e < NL; ++e) {
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
      const double kss = ffgp_tree_eval(tr, sv);
      ffgp_tree_back(tr, sv, gs);
      const double mf = acq_rowgroup_sum(redm, msum, rg, j);

      // ---- 2. V = L^-1 K_s, |V_j|^2;  3. B = L^-T V (into the image of K_s)
      const double vv = acq_solve_images(mb.Linv, np, nb, img0, img1, redv, tid);
      __syncthreads();

      // ---- 4. the member's share of mean, variance, the self term and the two gradient partials
      mean = __builtin_fma(cm, mf, mean);
      var = __builtin_fma(cv, kss - vv + vadd, var);
      if (o.owner) {
        double ds = 0.0;
#pragma unroll
        for (int e = 0; e < NL; ++e)
          if (e < nl && lin[e]) ds = __builtin_fma(gs[e] * (2.0 * lp[4 * e]), w2[e * DM + rg] * (o.x - cen[e * DM + rg]), ds);
        self = __builtin_fma(cv, ds, self);
      }
      for (int p = 0; p < nb; ++p) {
        const int i = 16 * p + rg;
        const bool in = i < n;
        const double* xr = Xs + i * DM;
        double v[NL], dv[NL], gl[NL];
#pragma unroll
        for (int e = 0; e < NL; ++e) {
          v[e] = 0.0;
          dv[e] = 0.0;
          if (e < nl) {
            const double amp = lp[4 * e];
            if (lin[e]) {
              double s = 0.0;
#pragma unroll
              for (int dd = 0; dd < DM; ++dd) s = __builtin_fma(w2[e * DM + dd] * (xj[dd] - cen[e * DM + dd]), xr[dd] - cen[e * DM + dd], s);
              v[e] = amp * s;
              dv[e] = amp;
            } else {
              const double s = acq_sqdist<DM>(xr, xj, w2 + e * DM), cl = lp[4 * e + 1], sc = fmax(s, cl);
              v[e] = amp * ffgp_kfun_val(kf[e], lp[4 * e + 2], sc);
              dv[e] = (in && s >= cl) ? amp * ffgp_kfun_m2d(kf[e], lp[4 * e + 2], sc) : 0.0;
            }
          }
        }
        ffgp_tree_back(tr, v, gl);
        // t = -dk_i/dx_j: radial leaf  amp (-2 phi') w^2 o (x_j - X_i);  linear leaf  -amp w^2 o (X_i - c) = amp w^2 o (c - X_i)
        double t[DM];
#pragma unroll
        for (int dd = 0; dd < DM; ++dd) t[dd] = 0.0;
#pragma unroll
        for (int e = 0; e < NL; ++e) {
          if (e < nl) {
            const double wt = gl[e] * dv[e];
            if (lin[e]) {
#pragma unroll
              for (int dd = 0; dd < DM; ++dd) t[dd] = __builtin_fma(wt, w2[e * DM + dd] * (cen[e * DM + dd] - xr[dd]), t[dd]);
            } else {
#pragma unroll
              for (int dd = 0; dd < DM; ++dd) t[dd] = __builtin_fma(wt, w2[e * DM + dd] * (xj[dd] - xr[dd]), t[dd]);
            }
          }
        }
        const double wm = in ? cm * al[i] : 0.0, wv = in ? cv * img0[i * 16 + j] : 0.0;
#pragma unroll
        for (int dd = 0; dd < DM; ++dd) {
          Gm[dd] = __builtin_fma(wm, t[dd], Gm[dd]);
          Gv[dd] = __builtin_fma(wv, t[dd], Gv[dd]);
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

    // ---- outputs and Adam, by the owner of (j, rg): the row sum and the self term -(da/dvar) sum_f c'_f dk_f(x, x)/dx
    if (o.owner) acq_owner_step<DM>(c, o, xq, k, iters, av, acq_partial_sum<DM>(img1, rg, j) - gv * self, tid);
    __syncthreads();
  }
  acq_owner_store(c, o, tid);
}

static int acq_stack_tree_launch_by_d(ffgp_handle* h, const AcqStackArgs& s, int grid, const AcqTrees& t) {
  const AcqStackTreeArgs a = {s, t.table_dev};
  return acq_by_dm(s.c.D, [&](auto dm) {
    return acq_launch<dm()>(h, ffgp_stack_tree_acq_kernel<dm()>, acq_stack_tree_lds_doubles, s.npmax, a, grid);
  });
}

// The trees are checked here; everything else -- the remaining checks, the workspace, the triangular inverses, the bias corrections, the
// upload of the leaf records, launch and wait -- is the stack entry's driver (acq_run, acq_stack.hip).
int ffgp_acq_optimize_stack_tree(ffgp_handle* h, const ffgp_acq_stack* s, const ffgp_ktree* const* trees, double* Xq_dev, int Q, int steps,
                                 const ffgp_adam* opt, double* state_dev, long step0, double* trace_dev, double* hist_dev, double* grad_dev) {
  if (!s || !trees || s->F < 1 || s->F > FFGP_ACQ_MAX_MEMBERS) return FFGP_ERR_ARG;
  for (int f = 0; f < s->F; ++f)
    if (trees[f] && !acq_tree_ok(trees[f])) return FFGP_ERR_ARG;
  return acq_run(h, s, acq_stack_tree_launch_by_d, Xq_dev, Q, steps, opt, state_dev, step0, trace_dev, hist_dev, grad_dev, trees, false, true);
}
