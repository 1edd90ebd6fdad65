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
#include "acq_tile.h"

struct AcqArgs {
  const double* X;       // [n, D]
  const double* Linv;    // [np, ldx], zero above the diagonal and in the padding
  const double* alpha;   // [n]
  const double* w;       // [D]
  const double* amp;
  const double* bc;      // [2 steps] bias corrections
  double* Xq;            // [Q, D]
  double* state;         // [2, Q, D] or null (evaluate mode)
  double* trace;         // [max(steps, 1), Q]
  double* hist;          // [steps + 1, Q, D] or null
  double* grad;          // [Q, D] or null
  int n, np, D, ldx, Q, steps, kfun, acq;
  double clamp, rinv, var_add, var_floor, kappa, xi, f_best, lr, b1, b2, eps;
};

template <int DM>
__global__ __launch_bounds__(ACQ_T) void ffgp_acq_kernel(AcqArgs a) {
  extern __shared__ double acq_lds[];
  const int np = a.np, nb = np >> 4, n = a.n, D = a.D;
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

  const int tid = threadIdx.x, j = tid & 15, rg = tid >> 4, wave = tid >> 6, lane = tid & 63, g = lane >> 4;
  const int q0 = blockIdx.x * ACQ_TILE;
  const double amp = a.amp[0];

  for (int idx = tid; idx < np * DM; idx += ACQ_T) {
    const int i = idx / DM, dd = idx % DM;
    Xs[idx] = (i < n && dd < D) ? a.X[(size_t)i * D + dd] : 0.0;
  }
  for (int i = tid; i < np; i += ACQ_T) al[i] = (i < n) ? a.alpha[i] : 0.0;
  if (tid < DM) {
    const double wv = (tid < D) ? a.w[tid] : 0.0;
    w2[tid] = wv * wv;
  }
  // the owner of (point j, dimension rg) keeps that coordinate and its Adam moments in registers for the whole call; the columns of a
  // ragged last tile repeat the last point and write nothing
  const int qo = q0 + j;
  const bool owner = rg < DM, live = owner && rg < D && qo < a.Q;
  double xo = 0.0, mo = 0.0, vo = 0.0;
  if (owner) {
    const size_t e = (size_t)min(qo, a.Q - 1) * D + rg;
    if (rg < D) {
      xo = a.Xq[e];
      if (a.steps > 0) {
        mo = a.state[e];
        vo = a.state[(size_t)a.Q * D + e];
      }
    }
    xq[j * DM + rg] = xo;
  }
  __syncthreads();

  const int iters = a.steps > 0 ? a.steps : 1;
  for (int k = 0; k < iters; ++k) {
    // ---- 1. K_s, derivative factors, mean
    double xj[DM];
#pragma unroll
    for (int dd = 0; dd < DM; ++dd) xj[dd] = xq[j * DM + dd];
    double msum = 0.0;
    for (int p = 0; p < nb; ++p) {
      const int i = 16 * p + rg;
      double s = 0.0;
#pragma unroll
      for (int dd = 0; dd < DM; ++dd) {
        const double df = Xs[i * DM + dd] - xj[dd];
        s = __builtin_fma(w2[dd] * df, df, s);
      }
      const double sc = fmax(s, a.clamp);
      const bool in = i < n;
      const double kv = in ? amp * ffgp_kfun_val(a.kfun, a.rinv, sc) : 0.0;
      img0[i * 16 + j] = kv;
      img2[i * 16 + j] = (in && s >= a.clamp) ? amp * ffgp_kfun_m2d(a.kfun, a.rinv, sc) : 0.0;
      msum = __builtin_fma(kv, al[i], msum);
    }
    redm[rg * 16 + j] = msum;
    __syncthreads();
    double mean = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) mean += redm[r * 16 + j];

    // ---- 2. V = L^-1 K_s, |V_j|^2
    double vvp = 0.0;
    for (int q = 0; q < 4; ++q) {
      const int bi = acq_deal(q, wave);
      if (bi >= nb) continue;
      d4_t acc = {0.0, 0.0, 0.0, 0.0};
      acq_chain<false>(acc, 0, bi + 1, a.Linv, bi, a.ldx, img0, lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        img1[(16 * bi + g + 4 * r) * 16 + j] = acc[r];
        vvp = __builtin_fma(acc[r], acc[r], vvp);
      }
    }
    redv[rg * 16 + j] = vvp;
    __syncthreads();
    double vv = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) vv += redv[r * 16 + j];

    // ---- 3. B = L^-T V (into the image of K_s)
    for (int q = 0; q < 4; ++q) {
      const int bi = acq_deal(q, wave);
      if (bi >= nb) continue;
      d4_t acc = {0.0, 0.0, 0.0, 0.0};
      acq_chain<true>(acc, bi, nb, a.Linv, bi, a.ldx, img1, lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) img0[(16 * bi + g + 4 * r) * 16 + j] = acc[r];
    }

    // ---- 4. the acquisition value and its derivatives with respect to mean and variance
    const double var = amp - vv + a.var_add;      // phi(0) = 1 for every radial profile
    double av, gm, gv;
    if (a.acq == FFGP_ACQ_UCB) {
      const double sd = sqrt(fmax(var, a.var_floor));
      av = mean + a.kappa * sd;
      gm = 1.0;
      gv = (var >= a.var_floor) ? a.kappa * 0.5 / sd : 0.0;      // torch's clamp_min: no gradient below the floor
    } else {
      const double sd = sqrt(var), s = fmax(sd, 1e-9), u = mean - a.f_best - a.xi, Z = u / s;
      const double Phi = 0.5 * erfc(-Z * 0.70710678118654752440), phi = exp(-0.5 * Z * Z) * 0.39894228040143267794;
      av = u * Phi + s * phi;
      gm = Phi;                                   // Phi and phi are constants of the reference's backward pass: exact all the same
      gv = (sd >= 1e-9) ? phi * 0.5 / sd : 0.0;
    }
    __syncthreads();

    // ---- the input gradient: partial sums over this thread's rows, then over the 16 row groups in a fixed order
    double ga[DM];
#pragma unroll
    for (int dd = 0; dd < DM; ++dd) ga[dd] = 0.0;
    for (int p = 0; p < nb; ++p) {
      const int i = 16 * p + rg;
      const double c = -(gm * al[i] - 2.0 * gv * img0[i * 16 + j]);
      const double wt = c * img2[i * 16 + j];
#pragma unroll
      for (int dd = 0; dd < DM; ++dd) ga[dd] = __builtin_fma(wt, xj[dd] - Xs[i * DM + dd], ga[dd]);
    }
#pragma unroll
    for (int dd = 0; dd < DM; ++dd) img1[(rg * DM + dd) * 16 + j] = ga[dd];
    __syncthreads();

    // ---- 5. outputs and Adam, by the owner of (j, rg)
    if (owner) {
      double gsum = 0.0;
#pragma unroll
      for (int r = 0; r < 16; ++r) gsum += img1[(r * DM + rg) * 16 + j];
      const double gx = -w2[rg] * gsum;
      if (live) {
        const size_t e = (size_t)qo * D + rg;
        if (rg == 0) a.trace[(size_t)k * a.Q + qo] = av;
        if (a.hist) a.hist[(size_t)k * a.Q * D + e] = xo;
        if (a.grad && k == iters - 1) a.grad[e] = gx;
      }
      if (a.steps > 0 && rg < D)
        ffgp_adam_update(&xo, &mo, &vo, gx, a.lr, a.b1, a.b2, a.eps, a.bc[2 * k], a.bc[2 * k + 1]);
      xq[j * DM + rg] = xo;
    }
    __syncthreads();
  }
  if (live && a.steps > 0) {
    const size_t e = (size_t)qo * D + rg;
    a.Xq[e] = xo;
    a.state[e] = mo;
    a.state[(size_t)a.Q * D + e] = vo;
    if (a.hist) a.hist[(size_t)a.steps * a.Q * D + e] = xo;
  }
}

template <int DM>
static int acq_launch(ffgp_handle* h, const AcqArgs& a, int grid) {
  const size_t lds = acq_lds_doubles(FFGP_ACQ_MAX_N, DM) * sizeof(double);
  // set on every call: the attribute belongs to the current device, and a host-side "already set" table would be shared state between
  // the threads of different handles (a host-side call, nothing is enqueued)
  FFGP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ffgp_acq_kernel<DM>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(ffgp_acq_kernel<DM>, dim3(grid), dim3(ACQ_T), acq_lds_doubles(a.np, DM) * sizeof(double), h->stream, a);
  if (hipGetLastError() != hipSuccess) return FFGP_ERR_HIP;
  return FFGP_OK;
}

static int acq_single_launch(ffgp_handle* h, const AcqStackArgs& s, int grid, const ffgp_ktree*) {
  const AcqStackMember& m = s.m[0];
  AcqArgs a;
  a.X = m.X; a.Linv = m.Linv; a.alpha = m.alpha; a.w = m.w; a.amp = m.amp; a.bc = s.bc;
  a.Xq = s.Xq; a.state = s.state; a.trace = s.trace; a.hist = s.hist; a.grad = s.grad;
  a.n = m.n; a.np = m.np; a.D = s.D; a.ldx = m.np; a.Q = s.Q; a.steps = s.steps; a.kfun = m.kfun; a.acq = s.acq;
  a.clamp = m.clamp; a.rinv = m.rinv; a.var_add = m.var_add; a.var_floor = s.var_floor; a.kappa = s.kappa; a.xi = s.xi; a.f_best = s.f_best;
  a.lr = s.lr; a.b1 = s.b1; a.b2 = s.b2; a.eps = s.eps;
  if (s.D <= 2) return acq_launch<2>(h, a, grid);
  if (s.D <= 8) return acq_launch<8>(h, a, grid);
  return acq_launch<16>(h, a, grid);
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
