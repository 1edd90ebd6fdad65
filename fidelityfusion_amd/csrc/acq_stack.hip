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

// A workgroup-uniform value kept in a vector register: the member table's fields on top of acq.hip's arguments are more uniform
// values than the scalar file holds, and the vector file has the room (a scalar spill would cost the kernel a private segment).
template <class T>
__device__ __forceinline__ T acq_in_vgpr(T x) {
  asm volatile("" : "+v"(x));
  return x;
}

template <int DM>
__global__ __launch_bounds__(ACQ_T) void ffgp_stack_acq_kernel(AcqStackArgs a) {
  extern __shared__ double acq_lds[];
  const int D = a.D;
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

  double* const trace = acq_in_vgpr(a.trace);
  double* const hist = acq_in_vgpr(a.hist);
  double* const grad = acq_in_vgpr(a.grad);
  double* const state = acq_in_vgpr(a.state);
  double* const Xq = acq_in_vgpr(a.Xq);
  const double* const bc = acq_in_vgpr(a.bc);

  const int tid = threadIdx.x, j = tid & 15, rg = tid >> 4, wave = tid >> 6, lane = tid & 63, g = lane >> 4;
  const int q0 = blockIdx.x * ACQ_TILE;
  // this column's level, and the number of members the tile needs: the same for every thread of the workgroup (the columns of a
  // ragged last tile repeat the last point)
  int lev = a.F - 1, fcount = a.F;
  if (a.level) {
    lev = min(a.level[min(q0 + j, a.Q - 1)], a.F - 1);
    int top = -1;
    for (int c = 0; c < ACQ_TILE; ++c) top = max(top, a.level[min(q0 + c, a.Q - 1)]);
    fcount = min(top, a.F - 1) + 1;
  }
  // the owner of (point j, dimension rg) keeps that coordinate, its Adam moments and its gradient accumulator in registers
  const int qo = q0 + j;
  const bool owner = rg < DM, live = owner && rg < D && qo < a.Q;
  const size_t plane = (size_t)a.Q * D;
  double xo = 0.0, mo = 0.0, vo = 0.0, go = 0.0;
  if (owner) {
    const size_t e = (size_t)min(qo, a.Q - 1) * D + rg;
    if (rg < D) {
      xo = Xq[e];
      if (a.steps > 0) {
        mo = state[e];
        vo = state[plane + e];
        if (a.accumulate) go = state[2 * plane + e];
      }
    }
    xq[j * DM + rg] = xo;
  }
  __syncthreads();

  const double var_floor = acq_in_vgpr(a.var_floor), kappa = acq_in_vgpr(a.kappa), xi = acq_in_vgpr(a.xi), f_best = acq_in_vgpr(a.f_best);
  const double lr = acq_in_vgpr(a.lr), b1 = acq_in_vgpr(a.b1), b2 = acq_in_vgpr(a.b2), eps = acq_in_vgpr(a.eps);
  const int iters = a.steps > 0 ? a.steps : 1;
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
      for (int idx = tid; idx < np * DM; idx += ACQ_T) {
        const int i = idx / DM, dd = idx % DM;
        Xs[idx] = (i < n && dd < D) ? mX[(size_t)i * D + dd] : 0.0;
      }
      for (int i = tid; i < np; i += ACQ_T) al[i] = (i < n) ? malpha[i] : 0.0;
      if (tid < DM) {
        const double wv = (tid < D) ? mw[tid] : 0.0;
        w2[tid] = wv * wv;
      }
      __syncthreads();

      // ---- 1. K_s, derivative factors, mean_f (every row below np_f is written)
      double msum = 0.0;
      for (int p = 0; p < nb; ++p) {
        const int i = 16 * p + rg;
        double s = 0.0;
#pragma unroll
        for (int dd = 0; dd < DM; ++dd) {
          const double df = Xs[i * DM + dd] - xj[dd];
          s = __builtin_fma(w2[dd] * df, df, s);
        }
        const double sc = fmax(s, clamp);
        const bool in = i < n;
        const double kv = in ? amp * ffgp_kfun_val(kfun, rinv, sc) : 0.0;
        img0[i * 16 + j] = kv;
        img2[i * 16 + j] = (in && s >= clamp) ? amp * ffgp_kfun_m2d(kfun, rinv, sc) : 0.0;
        msum = __builtin_fma(kv, al[i], msum);
      }
      redm[rg * 16 + j] = msum;
      __syncthreads();
      double mf = 0.0;
#pragma unroll
      for (int r = 0; r < 16; ++r) mf += redm[r * 16 + j];

      // ---- 2. V = L^-1 K_s, |V_j|^2
      double vvp = 0.0;
      for (int q = 0; q < 4; ++q) {
        const int bi = acq_deal(q, wave);
        if (bi >= nb) continue;
        d4_t acc = {0.0, 0.0, 0.0, 0.0};
        acq_chain<false>(acc, 0, bi + 1, mb.Linv, bi, np, img0, lane);
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
        acq_chain<true>(acc, bi, nb, mb.Linv, bi, np, img1, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) img0[(16 * bi + g + 4 * r) * 16 + j] = acc[r];
      }
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
    if (a.acq == FFGP_ACQ_UCB) {
      const double sd = sqrt(fmax(var, var_floor));
      av = mean + kappa * sd;
      gm = 1.0;
      gv = (var >= var_floor) ? kappa * 0.5 / sd : 0.0;      // torch's clamp_min: no gradient below the floor
    } else if (a.acq == FFGP_ACQ_UCB_VAR) {
      av = mean + kappa * var;
      gm = 1.0;
      gv = kappa;
    } else {
      const double sd = sqrt(var), s = fmax(sd, 1e-9), u = mean - f_best - xi, Z = u / s;
      const double Phi = 0.5 * erfc(-Z * 0.70710678118654752440), phi = exp(-0.5 * Z * Z) * 0.39894228040143267794;
      av = u * Phi + s * phi;
      gm = Phi;                                   // Phi and phi are constants of the reference's backward pass: exact all the same
      gv = (sd >= 1e-9) ? phi * 0.5 / sd : 0.0;
    }
    // the last member's V has been read (the barrier after stage 3): its image takes the partials of d(-a)/dx
#pragma unroll
    for (int dd = 0; dd < DM; ++dd) img1[(rg * DM + dd) * 16 + j] = gm * Gm[dd] - 2.0 * gv * Gv[dd];
    __syncthreads();

    // ---- outputs and Adam, by the owner of (j, rg)
    if (owner) {
      double gx = 0.0;
#pragma unroll
      for (int r = 0; r < 16; ++r) gx += img1[(r * DM + rg) * 16 + j];
      if (live) {
        const size_t e = (size_t)qo * D + rg;
        if (rg == 0) trace[(size_t)k * a.Q + qo] = av;
        if (hist) hist[(size_t)k * a.Q * D + e] = xo;
        if (grad && k == iters - 1) grad[e] = gx;
      }
      if (a.steps > 0 && rg < D) {
        if (a.accumulate) {
          go += gx;
          gx = go;
        }
        ffgp_adam_update(&xo, &mo, &vo, gx, lr, b1, b2, eps, bc[2 * k], bc[2 * k + 1]);
      }
      xq[j * DM + rg] = xo;
    }
    __syncthreads();
  }
  if (live && a.steps > 0) {
    const size_t e = (size_t)qo * D + rg;
    Xq[e] = xo;
    state[e] = mo;
    state[plane + e] = vo;
    if (a.accumulate) state[2 * plane + e] = go;
    if (hist) hist[(size_t)a.steps * a.Q * D + e] = xo;
  }
}

template <int DM>
static int acq_stack_launch(ffgp_handle* h, const AcqStackArgs& a, int grid) {
  const size_t lds = acq_lds_doubles(FFGP_ACQ_MAX_N, DM) * sizeof(double);
  // set on every call, as acq.hip does: the attribute belongs to the current device
  FFGP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ffgp_stack_acq_kernel<DM>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(ffgp_stack_acq_kernel<DM>, dim3(grid), dim3(ACQ_T), acq_lds_doubles(a.npmax, DM) * sizeof(double), h->stream, a);
  if (hipGetLastError() != hipSuccess) return FFGP_ERR_HIP;
  return FFGP_OK;
}

static int acq_stack_launch_by_d(ffgp_handle* h, const AcqStackArgs& a, int grid, const ffgp_ktree*) {
  if (a.D <= 2) return acq_stack_launch<2>(h, a, grid);
  if (a.D <= 8) return acq_stack_launch<8>(h, a, grid);
  return acq_stack_launch<16>(h, a, grid);
}

int acq_run(ffgp_handle* h, const ffgp_acq_stack* s, acq_launch_fn launch, double* Xq_dev, int Q, int steps, const ffgp_adam* opt, double* state_dev,
            long step0, double* trace_dev, double* hist_dev, double* grad_dev, const ffgp_ktree* tree, bool chain) {
  if (!h || !s || !Xq_dev || !trace_dev || Q <= 0 || steps < 0 || steps > FFGP_ACQ_MAX_STEPS || step0 < 0) return FFGP_ERR_ARG;
  if (steps > 0 && (!opt || !state_dev)) return FFGP_ERR_ARG;
  if (s->F < 1 || s->F > FFGP_ACQ_MAX_MEMBERS || !s->members || (tree && s->F != 1)) return FFGP_ERR_ARG;
  if (s->acq != FFGP_ACQ_UCB && s->acq != FFGP_ACQ_EI && s->acq != FFGP_ACQ_UCB_VAR) return FFGP_ERR_ARG;
  const int F = s->F, D = s->members[0].D;
  if (chain && D > FFGP_ACQ_MAX_D - 1) return FFGP_ERR_ARG;      // the members above the first take [x, mean below]: D + 1 inputs
  for (int f = 0; f < F; ++f) {
    const ffgp_acq_member& p = s->members[f];
    if (!p.X_dev || !p.L_dev || !p.alpha_dev || (!tree && (!p.w_dev || !p.amp_dev))) return FFGP_ERR_ARG;
    if (p.n < 1 || p.n > FFGP_ACQ_MAX_N || p.D < 1 || p.D > FFGP_ACQ_MAX_D || p.D != ((chain && f > 0) ? D + 1 : D) || p.d != 1) return FFGP_ERR_ARG;
    if (p.ldl < p.n || p.ldl > INT_MAX) return FFGP_ERR_ARG;
    if (!tree && (p.kfun < FFGP_KFUN_SE || p.kfun > FFGP_KFUN_RQ)) return FFGP_ERR_ARG;      // (the linear kernel's k(x, x) depends on x)
  }
  FFGP_HIP(hipSetDevice(h->device));
  const int iters = steps > 0 ? steps : 1;
  // workspace: [L_f^-1 (np_f x np_f, zero-padded), f = 0..F-1 | TRTRI scratch per member | bias corrections]
  size_t xd = 0, td = 0;
  int npmax = 0;
  for (int f = 0; f < F; ++f) {
    const size_t n = (size_t)s->members[f].n, np = (size_t)ffgp_round_up((int)n, 16);
    xd += np * np;
    td += n * n / 4 + n * FFGP_NB + 16;
    npmax = (int)np > npmax ? (int)np : npmax;
  }
  FFGP_CHECK(ffgp_ensure_ws(h, (xd + td + 2 * (size_t)iters) * sizeof(double)));
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
  for (int k = 0; k < steps; ++k) {
    const double t = (double)(step0 + k + 1);
    bc[2 * k] = 1.0 - std::pow(opt->beta1, t);
    bc[2 * k + 1] = std::sqrt(1.0 - std::pow(opt->beta2, t));
  }
  FFGP_HIP(hipMemcpyAsync(bc_dev, bc.data(), bc.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  a.level = s->level_dev; a.bc = bc_dev;
  a.Xq = Xq_dev; a.state = state_dev; a.trace = trace_dev; a.hist = hist_dev; a.grad = grad_dev;
  a.F = F; a.npmax = npmax; a.D = D; a.Q = Q; a.steps = steps; a.acq = s->acq; a.accumulate = s->accumulate_grad ? 1 : 0;
  a.var_floor = s->var_floor; a.kappa = s->kappa; a.xi = s->xi; a.f_best = s->f_best;
  a.lr = opt ? opt->lr : 0.0; a.b1 = opt ? opt->beta1 : 0.0; a.b2 = opt ? opt->beta2 : 0.0; a.eps = opt ? opt->eps : 0.0;
  const int grid = (Q + ACQ_TILE - 1) / ACQ_TILE;
  FFGP_CHECK(launch(h, a, grid, tree));
  FFGP_HIP(hipStreamSynchronize(h->stream));
  return FFGP_OK;
}

int ffgp_acq_optimize_stack(ffgp_handle* h, const ffgp_acq_stack* s, double* Xq_dev, int Q, int steps, const ffgp_adam* opt, double* state_dev,
                            long step0, double* trace_dev, double* hist_dev, double* grad_dev) {
  return acq_run(h, s, acq_stack_launch_by_d, Xq_dev, Q, steps, opt, state_dev, step0, trace_dev, hist_dev, grad_dev);
}
