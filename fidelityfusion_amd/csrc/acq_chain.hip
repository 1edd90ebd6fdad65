// The acquisition optimiser's Adam loop on a CHAIN of frozen posteriors in one launch (ffgp_acq_optimize_chain, include/ffgp.h).
// Reference: MF_BayesianOptimization/Discrete/DMF_acq.py:226-262 on NAR (FidelityFusion_Models/NAR.py:30-61): member f > 0 is a GP on
// z_f = [x, m_{f-1}(x)], the lower fidelity's predicted MEAN as one more input column, and the model reports the mean and the variance
// of the member a point stops at (its `to_fidelity`); the lower members' variances are discarded.  The plan is ffgp_stack_acq_kernel's
// (acq_stack.hip): a workgroup owns 16 query points and runs all the steps; what is new is the data flow between the members.
//
// Per step and tile (thread (rg = tid >> 4, j = tid & 15) works on query column j; s_j = min(level_j, F - 1)):
//   forward, f = 0 .. the tile's largest level
//     0. X_f (row length D_f = D, or D + 1 above member 0), alpha_f and w_f^2 are reloaded into LDS, every row up to np_f written and
//        every column from D_f on zeroed; u = m_{f-1} of this column (0 for f = 0) is kept in a [F][16] pad for the way back
//     1. K_s on z_f = [x, u] and m_f = K_s^T alpha_f, reduced over the 16 row groups in a fixed order
//     2. only if some column of the tile has s_j = f (the same for the whole workgroup): V = L_f^-1 K_s, |V_j|^2, B = L_f^-T V as in the
//        stack kernel; for the columns with s_j = f the variance amp_f - |V_j|^2 + var_add_f, the acquisition value, da/dmean, da/dvar,
//        and the direct gradient over the coordinates of z_f with c_i = (da/dmean alpha_i - 2 da/dvar B_i) amp (-2 phi')_i:
//            G += c_i w_f^2 o (z_f - Z_i)  over x,      gu = sum_i c_i w_fD^2 (u - Z_iD) = d(-a)/dm_{f-1}   (reduced like m_f)
//        the other columns add exact zeros and keep their gu
//   reverse, f = the tile's largest level - 1 .. 0
//     X_f, alpha_f, w_f^2 again; s_ij and amp (-2 phi') are re-evaluated in registers (no derivative image is kept); the upstream on
//     k_i is gu alpha_i, so c_i = -gu alpha_i amp (-2 phi')_i for the columns with s_j > f and 0 for the others; the x part goes into
//     the same G, the u part is the next gu
// then the one fixed-order reduction of G over the 16 row groups and torch.optim.Adam's update by the owner of (j, dim), as in the stack
// kernel.  The chains, O(n^2) per member, run for ONE member per point; every other member costs O(n D) twice.
// A column's arithmetic never reads another column's values and a switched-off pass adds exact zeros, so a point's trajectory does not
// depend on its tile, its neighbours or their levels, and level = k everywhere is the chain cut after member k.
#include <climits>
#include <cmath>
#include <vector>

#include "acq_tile.h"

// LDS in doubles, sized by the largest member: two [np][16] images (K_s then B; V, at least 256 DM: it also carries the gradient
// partials), X [np][DM], alpha [np], the tile's points [16][DM], w^2 [DM], two [16][16] reduction pads, the [F][16] pad of the u's
static constexpr size_t acq_chain_lds_doubles(int np, int DM) {
  const size_t img = (size_t)np * 16, img1 = img > (size_t)256 * DM ? img : (size_t)256 * DM;
  return img + img1 + (size_t)np * DM + np + 16 * DM + DM + 512 + 16 * FFGP_ACQ_MAX_MEMBERS;
}
static_assert(acq_chain_lds_doubles(FFGP_ACQ_MAX_N, FFGP_ACQ_MAX_D) * sizeof(double) <= 160 * 1024, "the chain kernel's LDS exceeds a CU's 160 KiB");

template <int DM>
__global__ __launch_bounds__(ACQ_T) void ffgp_chain_acq_kernel(AcqStackArgs a) {
  extern __shared__ double acq_lds[];
  AcqLoop c = a.c;
  acq_park_pointers(c);      // (acq_tile.h: the scalar file does not hold them beside the member table's fields)
  const int D = c.D;                                                      // the coordinates of x; members above 0 have D + 1 <= DM inputs
  const size_t imgmax = (size_t)a.npmax * 16;
  double* img0 = acq_lds;                                                 // K_s, then B = Sigma^-1 K_s
  double* img1 = img0 + imgmax;                                           // V = L^-1 K_s; after the sweeps the gradient partials
  double* Xs = img1 + (imgmax > (size_t)256 * DM ? imgmax : (size_t)256 * DM);
  double* al = Xs + (size_t)a.npmax * DM;
  double* xq = al + a.npmax;
  double* w2 = xq + 16 * DM;
  double* redm = w2 + DM;
  double* redv = redm + 256;
  double* upad = redv + 256;                                              // [F][16]: u = m_{f-1} per column

  const int tid = threadIdx.x, j = tid & 15, rg = tid >> 4;
  const int q0 = blockIdx.x * ACQ_TILE;
  // this column's level, the number of members the tile needs and the set of levels its columns stop at: the same for every thread
  // of the workgroup (the columns of a ragged last tile repeat the last point).  A negative level matches no member: value 0, gradient 0
  int lev = a.F - 1, fcount = a.F;
  unsigned tops = 1u << (a.F - 1);
  if (c.level) {
    lev = min(c.level[min(q0 + j, c.Q - 1)], a.F - 1);
    int top = -1;
    tops = 0u;
    for (int cc = 0; cc < ACQ_TILE; ++cc) {
      const int l = min(c.level[min(q0 + cc, c.Q - 1)], a.F - 1);
      top = max(top, l);
      if (l >= 0) tops |= 1u << l;
    }
    fcount = top + 1;
  }
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
    double u = 0.0, gu = 0.0, av = 0.0;
    // the two sweeps as one loop: t < fcount is the forward pass of member t, the rest the reverse pass of member 2 fcount - 2 - t
    for (int t = 0; t < 2 * fcount - 1; ++t) {
      const bool fwd = t < fcount;
      const int f = fwd ? t : 2 * fcount - 2 - t;
      const AcqStackMember& mb = a.m[f];
      const int n = mb.n, np = mb.np, nb = np >> 4, kfun = mb.kfun, Df = f ? D + 1 : D;
      const double amp = acq_in_vgpr(mb.amp[0]), clamp = acq_in_vgpr(mb.clamp), rinv = acq_in_vgpr(mb.rinv), vadd = acq_in_vgpr(mb.var_add);
      const double* const mX = acq_in_vgpr(mb.X);
      const double* const malpha = acq_in_vgpr(mb.alpha);
      const double* const mw = acq_in_vgpr(mb.w);

      // ---- 0. this member's X, alpha, w^2 (the previous pass has to be done with them)
      __syncthreads();
      acq_load_rows<DM>(Xs, al, mX, malpha, n, np, Df, tid);
      acq_load_w2<DM>(w2, mw, Df, tid);
      if (fwd) {
        if (rg == 0) upad[f * 16 + j] = u;
      } else {
        u = upad[f * 16 + j];      // written a forward pass, and several barriers, ago
      }
      __syncthreads();
      // z_f = [x, u]: the coordinate D (member 0: w^2 = 0 there and u = 0)
#pragma unroll
      for (int dd = 0; dd < DM; ++dd) xj[dd] = (dd == D) ? u : xj[dd];

      bool on;
      double gm = 0.0, gv = 0.0;
      if (fwd) {
        // ---- 1. K_s and m_f (every row below np_f is written)
        double msum = 0.0;
        for (int p = 0; p < nb; ++p) {
          const int i = 16 * p + rg;
          const double s = acq_sqdist<DM>(Xs + i * DM, xj, w2);
          const double kv = (i < n) ? amp * ffgp_kfun_val(kfun, rinv, fmax(s, clamp)) : 0.0;
          img0[i * 16 + j] = kv;
          msum = __builtin_fma(kv, al[i], msum);
        }
        const double mf = acq_rowgroup_sum(redm, msum, rg, j);
        u = mf;      // the next member's last input
        if (!((tops >> f) & 1u)) continue;      // no column of the tile stops here: the chains are not needed

        // ---- 2. V = L^-1 K_s, |V_j|^2;  3. B = L^-T V (into the image of K_s)
        const double vv = acq_solve_images(mb.Linv, np, nb, img0, img1, redv, tid);
        __syncthreads();

        // ---- 4. the acquisition value and its derivatives with respect to mean and variance, for the columns that stop here
        on = lev == f;
        double avf;
        acq_value(c.acq, mf, amp - vv + vadd, c.var_floor, c.kappa, c.xi, c.f_best, avf, gm, gv);      // phi(0) = 1 for every radial profile
        av = on ? avf : av;
      } else {
        on = lev > f;
      }

      // ---- the gradient pass of member f: direct (forward, the top member of a column) or carried (reverse)
      double gua = 0.0;
      for (int p = 0; p < nb; ++p) {
        const int i = 16 * p + rg;
        const double s = acq_sqdist<DM>(Xs + i * DM, xj, w2);
        const double dk = (i < n && s >= clamp) ? amp * ffgp_kfun_m2d(kfun, rinv, fmax(s, clamp)) : 0.0;
        const double up = fwd ? gm * al[i] - 2.0 * gv * img0[i * 16 + j] : -gu * al[i];
        const double ci = on ? up * dk : 0.0;      // a select, not a product: a switched-off column may carry anything
#pragma unroll
        for (int dd = 0; dd < DM; ++dd) {
          const double tt = w2[dd] * (xj[dd] - Xs[i * DM + dd]);
          G[dd] = __builtin_fma(ci, tt, G[dd]);
          gua = (dd == D) ? __builtin_fma(ci, tt, gua) : gua;
        }
      }
      if (f > 0) {      // d(-a)/dm_{f-1}: the u part, over the 16 row groups in a fixed order
        const double gs = acq_rowgroup_sum(redm, gua, rg, j);
        gu = on ? gs : gu;
      }
    }

    // the last V has been read (the barrier after stage 3): its image takes the partials of d(-a)/dx
#pragma unroll
    for (int dd = 0; dd < DM; ++dd) img1[(rg * DM + dd) * 16 + j] = G[dd];
    __syncthreads();

    // ---- outputs and Adam, by the owner of (j, rg)
    if (o.owner) acq_owner_step<DM>(c, o, xq, k, iters, av, acq_partial_sum<DM>(img1, rg, j), tid);
    __syncthreads();
  }
  acq_owner_store(c, o, tid);
}

// the template is chosen on D + 1, the upper members' input dimension (acq_run has checked D <= FFGP_ACQ_MAX_D - 1)
static int acq_chain_launch_by_d(ffgp_handle* h, const AcqStackArgs& a, int grid, const AcqTrees&) {
  return acq_by_dm(a.c.D + 1, [&](auto dm) { return acq_launch<dm()>(h, ffgp_chain_acq_kernel<dm()>, acq_chain_lds_doubles, a.npmax, a, grid); });
}

// The coefficients are checked here (reserved: a chain member has no weight of its own); everything else is the stack entry's driver
// (acq_run, acq_stack.hip), told that the members above the first take one more input.
int ffgp_acq_optimize_chain(ffgp_handle* h, const ffgp_acq_chain* c, double* Xq_dev, int Q, int steps, const ffgp_adam* opt, double* state_dev,
                            long step0, double* trace_dev, double* hist_dev, double* grad_dev) {
  if (!c) return FFGP_ERR_ARG;
  if (c->members && c->F >= 1 && c->F <= FFGP_ACQ_MAX_MEMBERS)
    for (int f = 0; f < c->F; ++f)
      if (c->members[f].mean_coef != 1.0 || c->members[f].var_coef != 1.0) return FFGP_ERR_ARG;
  ffgp_acq_stack s = {};
  s.F = c->F; s.members = c->members; s.level_dev = c->level_dev;
  s.var_floor = c->var_floor; s.acq = c->acq; s.kappa = c->kappa; s.xi = c->xi; s.f_best = c->f_best; s.accumulate_grad = c->accumulate_grad;
  return acq_run(h, &s, acq_chain_launch_by_d, Xq_dev, Q, steps, opt, state_dev, step0, trace_dev, hist_dev, grad_dev, nullptr, true);
}
