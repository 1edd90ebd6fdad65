// The acquisition optimiser's Adam loop on a CHAIN of frozen posteriors whose members may carry COMPOSED kernels, in one launch
// (ffgp_acq_optimize_chain_tree, include/ffgp.h).  Reference: the two-fidelity NAR is built on SumKernel(LinearKernel(1), MaternKernel(1))
// below and SumKernel(LinearKernel(2), MaternKernel(2)) above (FidelityFusion_Models/two_fidelity_models/NAR_NonlinearAR.py:23-26), and
// NAR(fidelity_num, kernel_list) takes any kernel list (FidelityFusion_Models/NAR.py:30-61); the loop is
// MF_BayesianOptimization/Discrete/DMF_acq.py:226-262.
// The plan is ffgp_chain_acq_kernel's (acq_chain.hip): a workgroup owns 16 query points and runs all the steps, the forward and the
// reverse sweep over the members as one loop, the `tops` mask that lets only a member some column stops at run the triangular solves,
// the [F][16] pad of the u's.  The per-member work is ffgp_stack_tree_acq_kernel's (acq_stack_tree.hip): stage 0 reloads X (row length
// D_f = D, or D + 1 above member 0), alpha and the member's leaf record from the table in handle workspace, every slot a later stage
// reads written (zeros past nl, zeros from D_f on); a radial member runs as the one-leaf record with self value amp; there is no
// derivative image -- the gradient pass re-evaluates the leaves and runs the tree's reverse sweep per row.
// What is this kernel's own is their meeting point: in a chain the linear leaves see the lower member's mean u as an input coordinate,
// so k_f(z, z), z = [x, u], depends on u, and the variance's self term puts a gradient into the chain as well as into x.
// With t_i = -dk_f(Z_i, z)/dz over all D_f coordinates (thread (rg = tid >> 4, j = tid & 15) on query column j; s_j = min(level_j, F - 1)):
//   forward, member f:   K_s through the tree, m_f = sum_i alpha_i k_i (the next member's u)
//     only if some column of the tile has s_j = f:  k_f(z, z) = tree(sv) with its reverse sweep gs, V, |V|^2, B; for the columns with
//     s_j = f  var = k_f(z, z) - |V|^2 + var_add_f, the acquisition value, gm = da/dmean, gv = da/dvar, and with c_i = gm alpha_i - 2 gv B_i
//         G += c_i t_i  over x,      gu = sum_i c_i t_i[D] - gv dk_f(z, z)/du,
//         dk_f(z, z)/du = sum over the linear leaves of gs[e] 2 amp_e w_e^2[D] (u - cen_e[D])
//     and the owner of (j, dim) keeps self = dk_f(z, z)/dx_dim, which it subtracts as gv self in its step
//   reverse, member f < s_j:   c_i = -gu alpha_i; no variance term and no self term (the lower variances are discarded); the x part goes
//     into the same G, the u part is the next gu
// A chain of radial members has no linear leaf: both self terms are exact zeros.  Switched-off columns are selects, not products, and add
// exact zeros, so a point's trajectory does not depend on its tile, its neighbours or their levels, level = k everywhere is the chain cut
// after member k, and a negative level gives value 0, gradient 0 and a point that does not move.
#include <climits>

#include "acq_tile.h"

struct AcqChainTreeArgs {
  AcqStackArgs s;
  const AcqMemberTree* tab;      // [F] in handle workspace
};
// the tree that tree_ops.h evaluates: a one-leaf record as the sum of its leaf and 0.0 (exact)
struct AcqChainTreeShape {
  int nl, shape, op[3];
};

// LDS in doubles, sized by the largest member: two [np][16] images (K_s then B; V, at least 256 DM: it also carries the gradient
// partials), X [np][DM], alpha [np], the tile's points [16][DM], per leaf w^2 [DM] and centre [DM], per leaf (amp, clamp, 1 / kparam,
// self value) [4], two [16][16] reduction pads, the [F][16] pad of the u's
static constexpr size_t acq_chain_tree_lds_doubles(int np, int DM) {
  const size_t img = (size_t)np * 16, img1 = img > (size_t)256 * DM ? img : (size_t)256 * DM;
  return img + img1 + (size_t)np * DM + np + 16 * DM + 2 * FFGP_TREE_LEAVES * DM + 4 * FFGP_TREE_LEAVES + 512 + 16 * FFGP_ACQ_MAX_MEMBERS;
}
static_assert(acq_chain_tree_lds_doubles(FFGP_ACQ_MAX_N, FFGP_ACQ_MAX_D) * sizeof(double) <= 160 * 1024,
              "the chain-of-trees acquisition kernel's LDS exceeds a CU's 160 KiB");

template <int DM>
__global__ __launch_bounds__(ACQ_T) void ffgp_chain_tree_acq_kernel(AcqChainTreeArgs a) {
  constexpr int NL = FFGP_TREE_LEAVES;
  extern __shared__ double acq_lds[];
  AcqLoop c = a.s.c;
  acq_park_pointers(c);
  const int D = c.D, F = a.s.F;                                           // the coordinates of x; members above 0 have D + 1 <= DM inputs
  const size_t imgmax = (size_t)a.s.npmax * 16;
  double* img0 = acq_lds;                                                 // K_s, then B = Sigma^-1 K_s
  double* img1 = img0 + imgmax;                                           // V = L^-1 K_s; after the sweeps the gradient partials
  double* Xs = img1 + (imgmax > (size_t)256 * DM ? imgmax : (size_t)256 * DM);
  double* al = Xs + (size_t)a.s.npmax * DM;
  double* xq = al + a.s.npmax;
  double* w2 = xq + 16 * DM;                                              // [leaf][DM]
  double* cen = w2 + NL * DM;                                             // [leaf][DM]
  double* lp = cen + NL * DM;                                             // [leaf][amp, clamp, 1 / kparam, self value of a radial leaf]
  double* redm = lp + 4 * NL;
  double* redv = redm + 256;
  double* upad = redv + 256;                                              // [F][16]: u = m_{f-1} per column

  const int tid = threadIdx.x, j = tid & 15, rg = tid >> 4;
  const int q0 = blockIdx.x * ACQ_TILE;
  // this column's level, the number of members the tile needs and the set of levels its columns stop at: the same for every thread
  // of the workgroup (the columns of a ragged last tile repeat the last point).  A negative level matches no member: value 0, gradient 0
  int lev = F - 1, fcount = F;
  unsigned tops = 1u << (F - 1);
  if (c.level) {
    lev = min(c.level[min(q0 + j, c.Q - 1)], F - 1);
    int top = -1;
    tops = 0u;
    for (int cc = 0; cc < ACQ_TILE; ++cc) {
      const int l = min(c.level[min(q0 + cc, c.Q - 1)], F - 1);
      top = max(top, l);
      if (l >= 0) tops |= 1u << l;
    }
    fcount = top + 1;
  }
  // (D, Q, steps, acq) arrive as one scalar tuple; kept whole across the step loop it is given a spill slot that nothing reads in the
  // end, and the kernel a private segment with it.  Q, the owners' business from here on, moves to the vector file
  c.Q = acq_in_vgpr(c.Q);
  AcqOwner o = acq_owner_load<DM>(c, xq, tid);
  __syncthreads();
  acq_park_constants(c);

  const int iters = c.steps > 0 ? c.steps : 1;
  for (int k = 0; k < iters; ++k) {
    double xj[DM], G[DM];
#pragma unroll
    for (int dd = 0; dd < DM; ++dd) {
      xj[dd] = xq[j * DM + dd];      // 0 from D on
      G[dd] = 0.0;
    }
    // gvt, self: da/dvar and (the owner's) dk_f(z, z)/dx of its dimension, of the member this column stops at
    double u = 0.0, gu = 0.0, av = 0.0, gvt = 0.0, self = 0.0;
    // the two sweeps as one loop: t < fcount is the forward pass of member t, the rest the reverse pass of member 2 fcount - 2 - t
    for (int t = 0; t < 2 * fcount - 1; ++t) {
      const bool fwd = t < fcount;
      const int f = fwd ? t : 2 * fcount - 2 - t;
      const AcqStackMember& mb = a.s.m[f];
      const AcqMemberTree& mt = a.tab[f];
      const int n = mb.n, np = mb.np, nb = np >> 4, nl = mt.nl, Df = f ? D + 1 : D;
      const double vadd = acq_in_vgpr(mb.var_add);
      const double* const mX = acq_in_vgpr(mb.X);
      const double* const malpha = acq_in_vgpr(mb.alpha);
      const double* const mLinv = acq_in_vgpr(mb.Linv);
      AcqChainTreeShape tr;
      tr.nl = max(nl, 2); tr.shape = mt.shape; tr.op[0] = mt.op[0]; tr.op[1] = mt.op[1]; tr.op[2] = mt.op[2];
      // the leaves' profiles packed into one word, a byte each (FFGP_KFUN_SE past nl): one uniform value across both sweeps where
      // two four-element arrays would stand, and nothing that could end up in private memory
      unsigned kfs = 0u;
#pragma unroll
      for (int e = 0; e < NL; ++e) kfs |= (unsigned)((e < nl) ? mt.k[e].kfun : FFGP_KFUN_SE) << (8 * e);
      const auto kf = [kfs](int e) { return (int)((kfs >> (8 * e)) & 255u); };
      const auto lin = [kfs](int e) { return (int)((kfs >> (8 * e)) & 255u) == FFGP_KFUN_LINEAR; };

      // ---- 0. this member's X, alpha and leaf record (the previous pass has to be done with them); all four leaf slots are written,
      //      zeros past nl and from D_f on
      __syncthreads();
      acq_load_rows<DM>(Xs, al, mX, malpha, n, np, Df, tid);
#pragma unroll
      for (int e = 0; e < NL; ++e) {
        const bool live = e < nl;
        if (tid < DM) {
          const double wv = (live && tid < Df) ? mt.k[e].w[tid] : 0.0;
          w2[e * DM + tid] = wv * wv;
          cen[e * DM + tid] = (live && tid < Df && lin(e) && mt.k[e].center) ? mt.k[e].center[tid] : 0.0;
        }
        if (tid == 0) {
          const double amp = live ? mt.k[e].amp[0] : 0.0, cl = live ? mt.k[e].clamp : 0.0, ri = live ? mt.k[e].rinv : 1.0;
          lp[4 * e] = amp;
          lp[4 * e + 1] = cl;
          lp[4 * e + 2] = ri;
          // a radial member: amp (phi(0) = 1, what acq_chain.hip takes); a tree's radial leaf: amp phi(max(0, clamp)), acq_tree.hip's
          lp[4 * e + 3] = (!live || lin(e)) ? 0.0 : (nl == 1 ? amp : amp * ffgp_kfun_val(kf(e), ri, fmax(0.0, cl)));
        }
      }
      if (fwd) {
        if (rg == 0) upad[f * 16 + j] = u;
      } else {
        u = upad[f * 16 + j];      // written a forward pass, and several barriers, ago
      }
      __syncthreads();
      // z_f = [x, u]: the coordinate D (member 0: every w^2 is 0 there and u = 0)
#pragma unroll
      for (int dd = 0; dd < DM; ++dd) xj[dd] = (dd == D) ? u : xj[dd];

      bool on;
      double gm = 0.0, gv = 0.0, dsu = 0.0;
      if (fwd) {
        // ---- 1. K_s and m_f (every row below np_f is written)
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
              if (lin(e)) {
#pragma unroll
                for (int dd = 0; dd < DM; ++dd) s = __builtin_fma(w2[e * DM + dd] * (xj[dd] - cen[e * DM + dd]), xr[dd] - cen[e * DM + dd], s);
              } else {
                s = ffgp_kfun_val(kf(e), lp[4 * e + 2], fmax(acq_sqdist<DM>(xr, xj, w2 + e * DM), lp[4 * e + 1]));
              }
              v[e] = lp[4 * e] * s;
            }
          }
          const double kv = (i < n) ? ffgp_tree_eval(tr, v) : 0.0;
          img0[i * 16 + j] = kv;
          msum = __builtin_fma(kv, al[i], msum);
        }
        const double mf = acq_rowgroup_sum(redm, msum, rg, j);
        const double uf = u;      // this member's last input
        u = mf;                   // the next member's
        if (!((tops >> f) & 1u)) continue;      // no column of the tile stops here: neither the chains nor k_f(z, z) are needed

        // k_f(z, z) and its reverse sweep
        double sv[NL], gs[NL];
#pragma unroll
        for (int e = 0; e < NL; ++e) {
          sv[e] = 0.0;
          if (e < nl) {
            sv[e] = lp[4 * e + 3];
            if (lin(e)) {
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

        // ---- 2. V = L^-1 K_s, |V_j|^2;  3. B = L^-T V (into the image of K_s)
        const double vv = acq_solve_images(mLinv, np, nb, img0, img1, redv, tid);
        __syncthreads();

        // ---- 4. the acquisition value and its derivatives with respect to mean and variance, for the columns that stop here; the self
        //      term's derivative along u (every thread of the column) and along x (the owner of (j, dim))
        on = lev == f;
        double avf;
        acq_value(c.acq, mf, kss - vv + vadd, c.var_floor, c.kappa, c.xi, c.f_best, avf, gm, gv);
        av = on ? avf : av;
        gvt = on ? gv : gvt;
#pragma unroll
        for (int e = 0; e < NL; ++e)
          if (e < nl && lin(e)) dsu = __builtin_fma(gs[e] * (2.0 * lp[4 * e]), w2[e * DM + D] * (uf - cen[e * DM + D]), dsu);
        if (o.owner && rg < D) {
          double ds = 0.0;
#pragma unroll
          for (int e = 0; e < NL; ++e)
            if (e < nl && lin(e)) ds = __builtin_fma(gs[e] * (2.0 * lp[4 * e]), w2[e * DM + rg] * (o.x - cen[e * DM + rg]), ds);
          self = on ? ds : self;
        }
      } else {
        on = lev > f;
      }

      // ---- the gradient pass of member f: direct (forward, the top member of a column) or carried (reverse)
      double gua = 0.0;
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
            if (lin(e)) {
              double s = 0.0;
#pragma unroll
              for (int dd = 0; dd < DM; ++dd) s = __builtin_fma(w2[e * DM + dd] * (xj[dd] - cen[e * DM + dd]), xr[dd] - cen[e * DM + dd], s);
              v[e] = amp * s;
              dv[e] = amp;
            } else {
              const double s = acq_sqdist<DM>(xr, xj, w2 + e * DM), cl = lp[4 * e + 1], sc = fmax(s, cl);
              v[e] = amp * ffgp_kfun_val(kf(e), lp[4 * e + 2], sc);
              dv[e] = (in && s >= cl) ? amp * ffgp_kfun_m2d(kf(e), lp[4 * e + 2], sc) : 0.0;
            }
          }
        }
        ffgp_tree_back(tr, v, gl);
        // t = -dk_i/dz_j: radial leaf  amp (-2 phi') w^2 o (z_j - Z_i);  linear leaf  -amp w^2 o (Z_i - c) = amp w^2 o (c - Z_i)
        double tt[DM];
#pragma unroll
        for (int dd = 0; dd < DM; ++dd) tt[dd] = 0.0;
#pragma unroll
        for (int e = 0; e < NL; ++e) {
          if (e < nl) {
            const double wt = gl[e] * dv[e];
            if (lin(e)) {
#pragma unroll
              for (int dd = 0; dd < DM; ++dd) tt[dd] = __builtin_fma(wt, w2[e * DM + dd] * (cen[e * DM + dd] - xr[dd]), tt[dd]);
            } else {
#pragma unroll
              for (int dd = 0; dd < DM; ++dd) tt[dd] = __builtin_fma(wt, w2[e * DM + dd] * (xj[dd] - xr[dd]), tt[dd]);
            }
          }
        }
        const double up = fwd ? gm * al[i] - 2.0 * gv * img0[i * 16 + j] : -gu * al[i];
        const double ci = (on && in) ? up : 0.0;      // a select, not a product: a switched-off column may carry anything
#pragma unroll
        for (int dd = 0; dd < DM; ++dd) {
          G[dd] = __builtin_fma(ci, tt[dd], G[dd]);
          gua = (dd == D) ? __builtin_fma(ci, tt[dd], gua) : gua;
        }
      }
      if (f > 0) {      // d(-a)/dm_{f-1}: the u part, over the 16 row groups in a fixed order, and (forward) the self term's share
        const double gsum = acq_rowgroup_sum(redm, gua, rg, j);
        gu = on ? gsum - gv * dsu : gu;
      }
    }

    // the last V has been read (the barrier after stage 3): its image takes the partials of d(-a)/dx
#pragma unroll
    for (int dd = 0; dd < DM; ++dd) img1[(rg * DM + dd) * 16 + j] = G[dd];
    __syncthreads();

    // ---- outputs and Adam, by the owner of (j, rg): the row sum and the self term -(da/dvar) dk_f(z, z)/dx of the column's member
    if (o.owner) acq_owner_step<DM>(c, o, xq, k, iters, av, acq_partial_sum<DM>(img1, rg, j) - gvt * self, tid);
    __syncthreads();
  }
  acq_owner_store(c, o, tid);
}

// the template is chosen on D + 1, the upper members' input dimension (acq_run has checked D <= FFGP_ACQ_MAX_D - 1)
static int acq_chain_tree_launch_by_d(ffgp_handle* h, const AcqStackArgs& s, int grid, const AcqTrees& t) {
  const AcqChainTreeArgs a = {s, t.table_dev};
  return acq_by_dm(s.c.D + 1, [&](auto dm) {
    return acq_launch<dm()>(h, ffgp_chain_tree_acq_kernel<dm()>, acq_chain_tree_lds_doubles, s.npmax, a, grid);
  });
}

// The coefficients (reserved: a chain member has no weight of its own) and the trees are checked here; everything else -- the remaining
// checks with the chain's dimension rule, the workspace, the triangular inverses, the bias corrections, the upload of the leaf records,
// launch and wait -- is the stack entry's driver (acq_run, acq_stack.hip).
int ffgp_acq_optimize_chain_tree(ffgp_handle* h, const ffgp_acq_chain* c, const ffgp_ktree* const* trees, double* Xq_dev, int Q, int steps,
                                 const ffgp_adam* opt, double* state_dev, long step0, double* trace_dev, double* hist_dev, double* grad_dev) {
  if (!c || !trees || c->F < 1 || c->F > FFGP_ACQ_MAX_MEMBERS) return FFGP_ERR_ARG;
  for (int f = 0; f < c->F; ++f) {
    if (c->members && (c->members[f].mean_coef != 1.0 || c->members[f].var_coef != 1.0)) return FFGP_ERR_ARG;
    if (trees[f] && !acq_tree_ok(trees[f])) return FFGP_ERR_ARG;
  }
  ffgp_acq_stack s = {};
  s.F = c->F; s.members = c->members; s.level_dev = c->level_dev;
  s.var_floor = c->var_floor; s.acq = c->acq; s.kappa = c->kappa; s.xi = c->xi; s.f_best = c->f_best; s.accumulate_grad = c->accumulate_grad;
  return acq_run(h, &s, acq_chain_tree_launch_by_d, Xq_dev, Q, steps, opt, state_dev, step0, trace_dev, hist_dev, grad_dev, trees, true, true);
}
