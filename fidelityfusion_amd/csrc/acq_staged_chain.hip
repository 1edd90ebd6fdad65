// The acquisition optimiser's Adam loop on a CHAIN of frozen posteriors past the one-launch kernel's LDS-tile limit: launch per stage,
// every step enqueued by ONE library call (ffgp_acq_optimize_chain_staged, include/ffgp.h).  Reference: MF_BayesianOptimization/
// Discrete/DMF_acq.py:226-262 on NAR (FidelityFusion_Models/NAR.py:30-61), whose demo trains on 300 / 300 / 250 points (NAR.py:119-128).
// The model, the argument struct and the output layouts are ffgp_acq_optimize_chain's (acq_chain.hip); the images, the tile shape, the
// host prologue, the GEMMs, the column-sum kernel and the owner kernel are the staged stack loop's (acq_staged.h, acq_staged.hip).
//
// What differs from the stack loop is the data flow: member f > 0 is queried at z_f = [x, m_{f-1}(x)], so the members run in sequence --
// one launch per member and stage, the member index an argument -- and the gradient returns through the chain in reverse,
// gu = d(-a)/dm_{f-1} handed down member by member.  Only the member a point stops at contributes a variance, so the triangular
// products, the O(n^2 Q) part, run for the members some point stops at and for no others.
//
// Per call, after the shared prologue: a census of level_dev (ffgp_acq_staged_chain_census_kernel) -- `tops`, the bit set of the
// members at which some point stops; `top`, the highest of them -- read back once (4 bytes) before the step loop; levels do not change
// during a call.  level_dev NULL: tops = {F - 1}, nothing is read back.  The gradient partials of the members above `top`, which no
// launch covers and the owner kernel sums, are zero-filled.  Per step, 3 (top + 1) + 2 |tops| + 2 launches whatever Q and n:
//   forward, f = 0 .. top
//     1. ffgp_acq_staged_chain_ks_kernel    K_s,f and the derivative factors on z_f = [x_q, u_q], u_q = the chunk sums of m_{f-1} added in
//                                           chunk order (asc_chunk_sum: the expression the value stage uses, so the mean fed forward is
//                                           the mean reported, to the last bit); f = 0: row length D, coordinate D carries w^2 = 0
//     2. as_solve_stage, only if f in tops  V_f = L_f^-1 K_s,f and B_f = L_f^-T V_f, as the stack loop calls them
//     3. as_col_stage                       the chunk sums of K_s,f^T alpha_f and |V_f|^2 (V_f of a member outside tops: the prologue's zeros)
//   4. ffgp_acq_staged_chain_value_kernel   mean and variance amp_f - |V|^2 + var_add_f of the member the point stops at, acq_value
//   reverse, f = top .. 0
//     5. ffgp_acq_staged_chain_grad_kernel  per column the upstream on k_i: gm alpha_i - 2 gv B_iq if level == f, -gu_q alpha_i if
//                                           level > f (gu_q = the chunk sums of member f + 1's slot D, in chunk order), an exact 0
//                                           otherwise -- a select, as in acq_chain.hip: a switched-off column may carry anything;
//                                           c_i = upstream DK_iq, and w^2 o sum_i c_i (z_f - Z_i) goes to part[f][chunk][q][0..D]
//   6. as_owner_stage                       the partials summed in order (member, chunk) over the coordinates below D, the outputs, Adam
// The tiles are acq_staged.hip's: 64 query columns x 128 training rows on 256 threads, thread (lane = tid >> 6, c = tid & 63) on rows
// lane, lane + 4, ... of the chunk for column c, a wave on 64 consecutive doubles of an image row, the four lanes' sums added through
// LDS in the order 0..3.  Every sum is taken in an order that depends on n alone (chunk order, member order); no atomics; nothing depends
// on Q, on the grid or on timing except the GEMM's tile choice.
#include <climits>
#include <cmath>

#include "acq_staged.h"

// ---- the census of the levels: bit l of *out = some point stops at member l (levels clipped to F - 1, negative ones match no member)
__global__ __launch_bounds__(AS_T) void ffgp_acq_staged_chain_census_kernel(const int* level, int Q, int F, unsigned* out) {
  __shared__ unsigned bits[AS_T];
  unsigned b = 0u;
  for (int q = threadIdx.x; q < Q; q += AS_T) {
    const int l = min(level[q], F - 1);
    if (l >= 0) b |= 1u << l;
  }
  bits[threadIdx.x] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned all = 0u;
    for (int t = 0; t < AS_T; ++t) all |= bits[t];
    *out = all;
  }
}

// ---- 1. K_s and the derivative factors of member f on z_f; the columns Q..Qp-1 are written as zeros
template <int DM>
__global__ __launch_bounds__(AS_T) void ffgp_acq_staged_chain_ks_kernel(AcqStagedArgs a, int f) {
  __shared__ double Xs[AS_ROWS * DM];
  __shared__ double w2[DM];
  const AcqStagedMember& mb = a.m[f];
  const int n = mb.n, r0 = blockIdx.y * AS_ROWS;
  if (r0 >= n) return;
  const int rows = min(AS_ROWS, n - r0), tid = threadIdx.x, Df = f ? a.D + 1 : a.D;
  asc_load_rows<DM>(Xs, mb.X, r0, rows, Df, tid);
  acq_load_w2<DM>(w2, mb.w, Df, tid);
  __syncthreads();
  const int q = blockIdx.x * AS_COLS + (tid & 63), lane = tid >> 6;
  const bool live = q < a.Q;
  double xj[DM];
  asc_load_z<DM>(xj, a, f, q, live);
  const double amp = mb.amp[0], clamp = mb.clamp, rinv = mb.rinv;
  const int kfun = mb.kfun;
  for (int i = lane; i < rows; i += AS_LANES) {
    const double s = acq_sqdist<DM>(Xs + i * DM, xj, w2);
    const double sc = fmax(s, clamp);
    const size_t e = (size_t)(r0 + i) * a.Qp + q;
    mb.Ks[e] = live ? amp * ffgp_kfun_val(kfun, rinv, sc) : 0.0;
    mb.DK[e] = (live && s >= clamp) ? amp * ffgp_kfun_m2d(kfun, rinv, sc) : 0.0;
  }
}

// ---- 4. the mean and the variance of the member a point stops at, the acquisition value and its two derivatives
__global__ __launch_bounds__(AS_T) void ffgp_acq_staged_chain_value_kernel(AcqStagedArgs a) {
  const int q = blockIdx.x * AS_T + threadIdx.x;
  if (q >= a.Q) return;
  const int lev = as_level(a, q);
  double av = 0.0, gm = 0.0, gv = 0.0;      // a negative level stops at no member: value 0, gradient 0
  if (lev >= 0) {
    const AcqStagedMember& mb = a.m[lev];
    const double mean = asc_chunk_sum(a.pm, a, lev, q), vv = asc_chunk_sum(a.pv, a, lev, q);
    acq_value(a.acq, mean, mb.amp[0] - vv + mb.var_add, a.var_floor, a.kappa, a.xi, a.f_best, av, gm, gv);      // phi(0) = 1 for every radial profile
  }
  a.av[q] = av;
  a.gm[q] = gm;
  a.gv[q] = gv;
}

// ---- 5. member f's share of the input gradient, as chunk sums over the coordinates of z_f.  dk_i/dz = -amp (-2 phi') w^2 o (z - Z_i)
// and the loss is -a: the two signs cancel, w^2 is applied to the chunk's sum.  Slot D is this member's contribution to
// d(-a)/dm_{f-1}, which the launch of member f - 1 reads as gu.
template <int DM>
__global__ __launch_bounds__(AS_T) void ffgp_acq_staged_chain_grad_kernel(AcqStagedArgs a, int f) {
  __shared__ double Xs[AS_ROWS * DM];
  __shared__ double al[AS_ROWS];
  __shared__ double w2[DM];
  __shared__ double red[AS_LANES][AS_COLS * DM];
  const AcqStagedMember& mb = a.m[f];
  const int n = mb.n, r0 = blockIdx.y * AS_ROWS;
  if (r0 >= n) return;
  const int rows = min(AS_ROWS, n - r0), tid = threadIdx.x, D = a.D, Df = f ? D + 1 : D;
  asc_load_rows<DM>(Xs, mb.X, r0, rows, Df, tid);
  for (int i = tid; i < rows; i += AS_T) al[i] = mb.alpha[r0 + i];
  acq_load_w2<DM>(w2, mb.w, Df, tid);
  __syncthreads();
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
  if (below) {      // member f + 1 <= level has run before this launch
    const int nch = as_chunks(a.m[f + 1].n);
    for (int ch = 0; ch < nch; ++ch) gu += a.part[(((size_t)(f + 1) * a.nch + ch) * a.Qp + q) * DM + D];
  }
  for (int i = lane; i < rows; i += AS_LANES) {
    const size_t e = (size_t)(r0 + i) * a.Qp + q;
    const double up = top ? gm * al[i] - gv2 * mb.B[e] : -gu * al[i];
    const double ci = (top || below) ? up * mb.DK[e] : 0.0;      // a select, not a product: a switched-off column may carry anything
#pragma unroll
    for (int dd = 0; dd < DM; ++dd) G[dd] = __builtin_fma(ci, xj[dd] - Xs[i * DM + dd], G[dd]);
  }
#pragma unroll
  for (int dd = 0; dd < DM; ++dd) red[lane][c * DM + dd] = G[dd];
  __syncthreads();
  double* out = a.part + (((size_t)f * a.nch + blockIdx.y) * a.Qp + q0) * DM;
  for (int idx = tid; idx < AS_COLS * DM; idx += AS_T) {
    double s = 0.0;
#pragma unroll
    for (int l = 0; l < AS_LANES; ++l) s += red[l][idx];
    out[idx] = w2[idx % DM] * s;
  }
}

template <int DM>
static int asc_ks_launch(ffgp_handle* h, const AcqStagedArgs& a, dim3 grid, int f) {
  hipLaunchKernelGGL(ffgp_acq_staged_chain_ks_kernel<DM>, grid, dim3(AS_T), 0, h->stream, a, f);
  return as_launched();
}
template <int DM>
static int asc_grad_launch(ffgp_handle* h, const AcqStagedArgs& a, dim3 grid, int f) {
  hipLaunchKernelGGL(ffgp_acq_staged_chain_grad_kernel<DM>, grid, dim3(AS_T), 0, h->stream, a, f);
  return as_launched();
}
// the templates are chosen on D + 1, the upper members' input dimension, as the one-launch chain entry chooses (a.DM holds it)
static int asc_ks_stage(ffgp_handle* h, const AcqStagedArgs& a, dim3 tiles, int f) {
  return acq_by_dm(a.D + 1, [&](auto dm) { return asc_ks_launch<dm()>(h, a, tiles, f); });
}
static int asc_grad_stage(ffgp_handle* h, const AcqStagedArgs& a, dim3 tiles, int f) {
  return acq_by_dm(a.D + 1, [&](auto dm) { return asc_grad_launch<dm()>(h, a, tiles, f); });
}
static int asc_value_stage(ffgp_handle* h, const AcqStagedArgs& a) {
  hipLaunchKernelGGL(ffgp_acq_staged_chain_value_kernel, dim3((a.Q + AS_T - 1) / AS_T), dim3(AS_T), 0, h->stream, a);
  return as_launched();
}

// step k: a refused launch ends it there, before a later stage reads what it did not write
static int asc_step(ffgp_handle* h, const AcqStagedPlan& pl, int top, unsigned tops, int k) {
  const AcqStagedArgs& a = pl.a;
  int rc;
  for (int f = 0; f <= top; ++f) {
    const dim3 tiles(pl.qt, (a.m[f].n + AS_ROWS - 1) / AS_ROWS, 1);
    if ((rc = asc_ks_stage(h, a, tiles, f)) != FFGP_OK) return rc;
    if ((tops >> f) & 1u)
      if ((rc = as_solve_stage(h, pl, f)) != FFGP_OK) return rc;
    if ((rc = as_col_stage(h, a, tiles, f)) != FFGP_OK) return rc;
  }
  if ((rc = asc_value_stage(h, a)) != FFGP_OK) return rc;
  for (int f = top; f >= 0; --f) {
    const dim3 tiles(pl.qt, (a.m[f].n + AS_ROWS - 1) / AS_ROWS, 1);
    if ((rc = asc_grad_stage(h, a, tiles, f)) != FFGP_OK) return rc;
  }
  return as_owner_stage(h, pl, k);
}

// The census of a call (acq_staged.h): `tops`, `top`, and the zero-fill of the gradient partials above `top`.  The census word is the
// first of the entry's extra doubles.  A refused launch or copy is returned for the caller's acq_staged_finish.
int acq_staged_chain_census(ffgp_handle* h, const AcqStagedPlan& pl, unsigned& tops, int& top) {
  const AcqStagedArgs& a = pl.a;
  const int F = a.F;
  tops = 1u << (F - 1);
  top = F - 1;
  if (a.level) {
    unsigned* const census = reinterpret_cast<unsigned*>(pl.extra);
    hipLaunchKernelGGL(ffgp_acq_staged_chain_census_kernel, dim3(1), dim3(AS_T), 0, h->stream, a.level, a.Q, F, census);
    int rc = as_launched();
    if (rc == FFGP_OK && hipMemcpyAsync(&tops, census, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream) != hipSuccess) rc = FFGP_ERR_HIP;
    if (rc != FFGP_OK) return rc;
    FFGP_HIP(hipStreamSynchronize(h->stream));      // the one wait before the step loop
    tops &= (1u << F) - 1u;
  }
  top = -1;
  for (int f = 0; f < F; ++f)
    if ((tops >> f) & 1u) top = f;
  if (top < F - 1) {      // no launch writes these members' partials, and the owner kernel sums over every member
    const size_t per_member = (size_t)a.nch * a.Qp * a.DM;
    return ffgp_zero_async(h, a.part + (size_t)(top + 1) * per_member, (size_t)(F - 1 - top) * per_member * sizeof(double));
  }
  return FFGP_OK;
}

// The coefficients are checked here, as ffgp_acq_optimize_chain checks them (reserved: a chain member has no weight of its own);
// everything else the staged prologue refuses, told that the members above the first take one more input.
int ffgp_acq_optimize_chain_staged(ffgp_handle* h, const ffgp_acq_chain* c, double* Xq_dev, int Q, int steps, const ffgp_adam* opt,
                                   double* state_dev, long step0, double* trace_dev, double* hist_dev, double* grad_dev) {
  if (!c) return FFGP_ERR_ARG;
  if (c->members && c->F >= 1 && c->F <= FFGP_ACQ_MAX_MEMBERS)
    for (int f = 0; f < c->F; ++f)
      if (c->members[f].mean_coef != 1.0 || c->members[f].var_coef != 1.0) return FFGP_ERR_ARG;
  ffgp_acq_stack s = {};
  s.F = c->F; s.members = c->members; s.level_dev = c->level_dev;
  s.var_floor = c->var_floor; s.acq = c->acq; s.kappa = c->kappa; s.xi = c->xi; s.f_best = c->f_best; s.accumulate_grad = c->accumulate_grad;
  AcqStagedPlan pl;
  FFGP_CHECK(acq_staged_prepare(h, &s, nullptr, 4, true, 1, Xq_dev, Q, steps, opt, state_dev, step0, trace_dev, hist_dev, grad_dev, pl));
  unsigned tops;
  int top;
  int rc = acq_staged_chain_census(h, pl, tops, top);
  for (int k = 0; k < pl.iters && rc == FFGP_OK; ++k) rc = asc_step(h, pl, top, tops, k);
  return acq_staged_finish(h, rc);
}
