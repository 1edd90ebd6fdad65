// ffgp_train_tree_raw with RESIDUAL members -- train_AR's fidelities above 0 on a composed kernel (SumKernel(LinearKernel,
// MaternKernel): FidelityFusion_Models/AR_autoRegression.py:123-137, two_fidelity_models/AR_autoRegression.py:31-37) -- launch per stage
// at every size, both likelihood variants: ffgp_train_tree_res_raw.  The loop is train_tree.hip's (ffgp_train_tree_impl, train_tree.h);
// this file adds the two launches a residual member needs per step (ffgp_tree_resid_form_launch, ffgp_tree_res_adam_launch).  Before the likelihoods ONE launch forms, for every residual
// member, r = y_high - rho y_low and |s| = |v_high - rho v_low| in the handle's scratch, where the shadow problem's Y_dev / diag_vec_dev
// point.  The likelihood runs as it stands and leaves dloss/dr (A for V1, B for V2) and dloss/ddvec (G_ii) beside them.  The Adam
// launch then reduces dloss/drho member by member in a fixed order -- the trajectory of a member does not depend on its companions --
// and updates P + 1 parameters of a residual member, P of a plain one.  See include/ffgp.h.
#include "train_tree.h"

// r = y_high - rho y_low, dvec = |v_high - rho v_low| (a product, then a difference: torch's rounding); rho_last = rho
extern "C" __global__ __launch_bounds__(256) void ffgp_tree_resid_form(ffgp_tree_resid rs) {
  const int f = blockIdx.y;
  if (!rs.rho[f]) return;
  const double rho = rs.rho[f][0];
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t < rs.nd[f]) rs.r[f][t] = __dsub_rn(rs.yh[f][t], __dmul_rn(rho, rs.yl[f][t]));
  if (rs.vl[f] && t < rs.n[f]) rs.dv[f][t] = fabs(__dsub_rn(rs.vh[f][t * rs.vhs[f]], __dmul_rn(rho, rs.vl[f][t * rs.vls[f]])));
  if (t == 0 && rs.rho_last[f]) rs.rho_last[f][0] = rho;
}

// ffgp_tree_adam_kernel for a call with residual members: the same upkeep of the status words and the same chain rule
// (ffgp_tree_raw_grad), and in front of the updates dloss/drho = -sum gY .* y_low - sum_i gdv_i sgn(s_i) v_low,ii of every residual
// member, each reduced by the whole workgroup in one fixed order (256 strided partial sums, then a halving tree).  rho is parameter P
// of its member: moments at [P] and [2 P + 1] of a state laid out for P + 1 parameters.
extern "C" __global__ __launch_bounds__(256) void ffgp_tree_res_adam_kernel(int F, int pmax, ffgp_tree_resid rs, const ffgp_tree_member* __restrict__ tab,
                                                     const double* __restrict__ scratch, double* __restrict__ state, long state_stride, double lr,
                                                     double b1, double b2, double eps, double bc1, double bc2_sqrt, const double* __restrict__ loss,
                                                     double* __restrict__ trace, long trace_stride, int step, int* __restrict__ info) {
  __shared__ double part[256];
  __shared__ double drho[FFGP_TRAIN_MAXF];
  const int i0 = info[0], i1 = info[1];
  const int bad = i0 | i1;
  __syncthreads();
  if (threadIdx.x == 0) {      // sticky first failure, current word cleared for the next step's factorisations
    if (i1 == 0 && i0 != 0) info[1] = i0;
    info[0] = 0;
  }
  for (int f = threadIdx.x; f < F; f += blockDim.x)
    trace[(size_t)f * trace_stride + step] = bad ? __builtin_nan("") : tab[f].sc * loss[f];
  if (bad) return;      // (uniform: every thread read the same two words)
  for (int f = 0; f < F; ++f) {
    if (!rs.rho[f]) continue;
    const double rho = rs.rho[f][0];
    double x = 0.0;
    for (long t = threadIdx.x; t < rs.nd[f]; t += 256) x = __builtin_fma(rs.gY[f][t], rs.yl[f][t], x);
    if (rs.vl[f]) {
      for (int i = threadIdx.x; i < rs.n[f]; i += 256) {
        const double vl = rs.vl[f][(long)i * rs.vls[f]];
        const double s = __dsub_rn(rs.vh[f][(long)i * rs.vhs[f]], __dmul_rn(rho, vl));
        x = __builtin_fma(rs.gdv[f][i], (s > 0.0) ? vl : ((s < 0.0) ? -vl : 0.0), x);      // (sgn(0) = 0: torch's abs backward)
      }
    }
    part[threadIdx.x] = x;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) drho[f] = -part[0];
    __syncthreads();      // (part is free again, drho[f] visible, and every read of rho is behind us before any parameter moves)
  }
  const int per = pmax + 1, items = F * per;
  for (int j = threadIdx.x; j < items; j += blockDim.x) {
    const int f = j / per, i = j - f * per;
    const ffgp_tree_member* M = tab + f;
    const int P = M->P, Pt = P + (rs.rho[f] ? 1 : 0);
    if (i >= Pt) continue;
    double* par;
    double g;
    if (i < P) {
      g = ffgp_tree_raw_grad(M, scratch, i, &par);
    } else {
      par = rs.rho[f];
      g = M->sc * drho[f];
    }
    double* m = state + (size_t)f * state_stride + i;
    ffgp_adam_update(par, m, m + Pt, g, lr, b1, b2, eps, bc1, bc2_sqrt);
  }
}

void ffgp_tree_resid_form_launch(hipStream_t s, int F, const ffgp_tree_resid& rs, long rmax) {
  hipLaunchKernelGGL(ffgp_tree_resid_form, dim3((unsigned)((rmax + 255) / 256), F), dim3(256), 0, s, rs);
}
void ffgp_tree_res_adam_launch(hipStream_t s, int F, int pmax, const ffgp_tree_resid& rs, const ffgp_tree_member* tab, const double* scratch,
                               double* state, long state_stride, const ffgp_adam* opt, double bc1, double bc2_sqrt, const double* loss,
                               double* trace, long trace_stride, int step, int* info) {
  hipLaunchKernelGGL(ffgp_tree_res_adam_kernel, dim3(1), dim3(256), 0, s, F, pmax, rs, tab, scratch, state, state_stride, opt->lr, opt->beta1,
                     opt->beta2, opt->eps, bc1, bc2_sqrt, loss, trace, trace_stride, step, info);
}

// (a call without a residual member enqueues exactly ffgp_train_tree_raw's launches)
extern "C" int ffgp_train_tree_res_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_tree_links* l, const ffgp_residual* r, int steps,
                                       const ffgp_adam* opt, double* state_dev, long state_stride, long step0, double* trace_dev,
                                       long trace_stride) {
  return ffgp_train_tree_impl(h, F, p, l, r, steps, opt, state_dev, state_stride, step0, trace_dev, trace_stride);
}
