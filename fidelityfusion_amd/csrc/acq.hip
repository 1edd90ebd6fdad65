// The acquisition optimiser's Adam loop on a FROZEN posterior in one launch (ffgp_acq_optimize, include/ffgp.h).
// Reference: Bayesian_optimization/acq.py:48-68 -- `num_restarts` iterations of zero_grad(); loss = -acq(X).sum(); loss.backward();
// Adam.step() on `raw_samples` query points, the model untouched.  The loss is a sum of per-point terms and Adam is element-wise, so every
// query point's trajectory is its own: a workgroup owns a tile of 16 points and runs all the steps without talking to any other.
//
// Per step and tile (256 threads = 4 waves; thread (rg = tid >> 4, j = tid & 15) works on query column j):
//   1. K_s [np][16] (np = n rounded up to 16) and the derivative factors amp (-2 phi') into LDS images, mean_j = K_s^T alpha
//   2. V = L^-1 K_s as v_mfma_f64_16x16x4_f64 block chains: L^-1 (formed once per call, global memory / L2) is the A operand, the
//      [np][16] image the B operand (lane (g, m) reads element [4 kq + g][m]: 64 consecutive doubles, no bank conflict); the 16-row
//      blocks are independent and dealt to the waves so that each runs the same number of products; |V_j|^2 rides along
//   3. B = L^-T V the same way (transposed A blocks), into the image K_s no longer needs
//   4. the acquisition value and its two derivatives, c_i = -(da/dmean alpha_i - 2 da/dvar B_i), the input gradient
//      dx_j = -w^2 o sum_i c_i amp (-2 phi'(s_ij)) (x_j - X_i), reduced over the 16 row groups through LDS in a fixed order
//   5. torch.optim.Adam's update (ffgp_adam_update) by the thread that owns (j, dim): x, exp_avg and exp_avg_sq live in its registers
//      for the whole call
// Nothing of a point's arithmetic depends on its column or tile: a point run alone follows the same trajectory bit for bit.
// The load, the reductions, stages 2 and 3, the acquisition value, the owner's prologue, step and write-back and the launch are
// acq_tile.h's, one copy for this kernel and its three descendants; stage 1 and the gradient pass are written out here.
#include "acq_tile.h"

// the one posterior as a stack member (its two coefficients are not read) and the loop's arguments
struct AcqArgs {
  AcqStackMember m;
  AcqLoop c;
};

template <int DM>
__global__ __launch_bounds__(ACQ_T) void ffgp_acq_kernel(AcqArgs a) {
  extern __shared__ double acq_lds[];
  const AcqLoop& c = a.c;
  const int np = a.m.np, nb = np >> 4, n = a.m.n;
  const size_t img = (size_t)np * 16;
  double* img0 = acq_lds;                                              // K_s, then B = Sigma^-1 K_s
  double* img1 = img0 + img;                                           // V = L^-1 K_s, then the gradient partials
  double* img2 = img1 + (img > (size_t)256 * DM ? img : (size_t)256 * DM);   // amp (-2 phi'), 0 on the clamp
  double* Xs = img2 + img;
  double* al = Xs + (size_t)np * DM;
  double* xq = al + np;
  double* w2 = xq + 16 * DM;
  double* redm = w2 + DM;
  double* redv = redm + 256;

  const int tid = threadIdx.x, j = tid & 15, rg = tid >> 4;
  const double amp = a.m.amp[0];

  acq_load_rows<DM>(Xs, al, a.m.X, a.m.alpha, n, np, c.D, tid);
  acq_load_w2<DM>(w2, a.m.w, c.D, tid);
  AcqOwner o = acq_owner_load<DM>(c, xq, tid);
  __syncthreads();

  const int iters = c.steps > 0 ? c.steps : 1;
  for (int k = 0; k < iters; ++k) {
    // ---- 1. K_s, derivative factors, mean
    double xj[DM];
#pragma unroll
    for (int dd = 0; dd < DM; ++dd) xj[dd] = xq[j * DM + dd];
    double msum = 0.0;
    for (int p = 0; p < nb; ++p) {
      const int i = 16 * p + rg;
      const double s = acq_sqdist<DM>(Xs + i * DM, xj, w2);
      const double sc = fmax(s, a.m.clamp);
      const bool in = i < n;
      const double kv = in ? amp * ffgp_kfun_val(a.m.kfun, a.m.rinv, sc) : 0.0;
      img0[i * 16 + j] = kv;
      img2[i * 16 + j] = (in && s >= a.m.clamp) ? amp * ffgp_kfun_m2d(a.m.kfun, a.m.rinv, sc) : 0.0;
      msum = __builtin_fma(kv, al[i], msum);
    }
    const double mean = acq_rowgroup_sum(redm, msum, rg, j);

    // ---- 2. V = L^-1 K_s, |V_j|^2;  3. B = L^-T V (into the image of K_s)
    const double vv = acq_solve_images(a.m.Linv, np, nb, img0, img1, redv, tid);

    // ---- 4. the acquisition value and its derivatives with respect to mean and variance
    const double var = amp - vv + a.m.var_add;      // phi(0) = 1 for every radial profile
    double av, gm, gv;
    acq_value(c.acq, mean, var, c.var_floor, c.kappa, c.xi, c.f_best, av, gm, gv);
    __syncthreads();

    // ---- the input gradient: partial sums over this thread's rows, then over the 16 row groups in a fixed order
    double ga[DM];
#pragma unroll
    for (int dd = 0; dd < DM; ++dd) ga[dd] = 0.0;
    for (int p = 0; p < nb; ++p) {
      const int i = 16 * p + rg;
      const double ci = -(gm * al[i] - 2.0 * gv * img0[i * 16 + j]);
      const double wt = ci * img2[i * 16 + j];
#pragma unroll
      for (int dd = 0; dd < DM; ++dd) ga[dd] = __builtin_fma(wt, xj[dd] - Xs[i * DM + dd], ga[dd]);
    }
#pragma unroll
    for (int dd = 0; dd < DM; ++dd) img1[(rg * DM + dd) * 16 + j] = ga[dd];
    __syncthreads();

    // ---- 5. outputs and Adam, by the owner of (j, rg): w^2 is the one kernel's, so it multiplies the row sum
    if (o.owner) acq_owner_step<DM>(c, o, xq, k, iters, av, -w2[rg] * acq_partial_sum<DM>(img1, rg, j), tid);
    __syncthreads();
  }
  acq_owner_store(c, o, tid);
}

static int acq_single_launch(ffgp_handle* h, const AcqStackArgs& s, int grid, const AcqTrees&) {
  const AcqArgs a = {s.m[0], s.c};
  return acq_by_dm(s.c.D, [&](auto dm) { return acq_launch<dm()>(h, ffgp_acq_kernel<dm()>, acq_lds_doubles, a.m.np, a, grid); });
}

// One posterior is the stack of one member with both coefficients 1, no levels and no accumulation: the checks, the workspace, the
// triangular inverse and the bias corrections are the stack entry's (acq_run, acq_stack.hip); only the kernel and its launch are this file's.
int ffgp_acq_optimize(ffgp_handle* h, const ffgp_acq_problem* p, double* Xq_dev, int Q, int steps, const ffgp_adam* opt, double* state_dev,
                      long step0, double* trace_dev, double* hist_dev, double* grad_dev) {
  if (!p || (p->acq != FFGP_ACQ_UCB && p->acq != FFGP_ACQ_EI)) return FFGP_ERR_ARG;      // FFGP_ACQ_UCB_VAR: the stack entry only
  ffgp_acq_member m = {};
  m.n = p->n; m.D = p->D; m.d = p->d;
  m.X_dev = p->X_dev; m.L_dev = p->L_dev; m.ldl = p->ldl; m.alpha_dev = p->alpha_dev; m.w_dev = p->w_dev; m.amp_dev = p->amp_dev;
  m.clamp_min = p->clamp_min; m.kfun = p->kfun; m.kparam = p->kparam; m.var_add_all = p->var_add_all;
  m.mean_coef = 1.0; m.var_coef = 1.0;
  ffgp_acq_stack s = {};
  s.F = 1; s.members = &m; s.level_dev = nullptr;
  s.var_floor = p->var_floor; s.acq = p->acq; s.kappa = p->kappa; s.xi = p->xi; s.f_best = p->f_best; s.accumulate_grad = 0;
  return acq_run(h, &s, acq_single_launch, Xq_dev, Q, steps, opt, state_dev, step0, trace_dev, hist_dev, grad_dev);
}
