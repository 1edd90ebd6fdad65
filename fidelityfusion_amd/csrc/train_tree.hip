// K training steps in one call for models whose kernel is a composition (ffgp_ktree: SumKernel / ProductKernel trees of 2-4 leaves),
// launch per stage at every size: ffgp_train_tree_raw.  Per step: ONE launch maps every member's raw leaf parameters to the effective
// w / amp / diag_add the tile pass reads, the likelihood and its gradients are ffgp_nlml_fused_async's own launches on a shadow
// problem that points at those values, and ONE launch carries the gradients back through the links and takes Adam's step (the
// update function of ffgp_adam_kernel, drivers.h).  See include/ffgp.h.
#include <cmath>
#include <vector>

#include "train_tree.h"
#include "tree_ops.h"

// raw -> effective, one workgroup per member (ffgp_link_fwd's arithmetic for every leaf)
extern "C" __global__ void ffgp_tree_link_fwd(const ffgp_tree_member* __restrict__ tab, double* __restrict__ scratch) {
  const ffgp_tree_member* M = tab + blockIdx.x;
  const int D = M->D, per = D + 1, tot = M->nl * per + 1;
  double* eff = scratch + M->eff;
  for (int i = threadIdx.x; i < tot; i += blockDim.x) {
    double val;
    if (i == tot - 1) {
      val = ffgp_link_val(M->dadd_link, M->dadd[0], M->dadd_c);
    } else {
      const int e = i / per, k = i - e * per;
      if (k < D) val = ffgp_link_val(M->w_link[e], M->w[e][(M->nw[e] == D) ? k : 0], M->w_c[e]);
      else val = ffgp_link_val(M->amp_link[e], M->amp[e][0], M->amp_c[e]);
    }
    eff[i] = val;
  }
}

// the links' chain rule (ffgp_link_bwd's arithmetic; a broadcast length scale: the D effective gradients summed in index order
// first), the step's losses into the trace, Adam's step on every raw parameter of every member, and the upkeep of the status words
// as ffgp_adam_kernel does it with `fold` -- ONE workgroup, so that the words are read by every thread before thread 0 rewrites
// them; the threads run over (member, raw parameter) pairs, pmax = the largest P of the call.
extern "C" __global__ void ffgp_tree_adam_kernel(int F, int pmax, const ffgp_tree_member* __restrict__ tab, const double* __restrict__ scratch,
                                                 double* __restrict__ state, long state_stride, double lr, double b1, double b2, double eps,
                                                 double bc1, double bc2_sqrt, const double* __restrict__ loss, double* __restrict__ trace,
                                                 long trace_stride, int step, int* __restrict__ info) {
  const int i0 = info[0], i1 = info[1];
  const int bad = i0 | i1;
  __syncthreads();
  if (threadIdx.x == 0) {      // sticky first failure, current word cleared for the next step's factorisations
    if (i1 == 0 && i0 != 0) info[1] = i0;
    info[0] = 0;
  }
  for (int f = threadIdx.x; f < F; f += blockDim.x)
    trace[(size_t)f * trace_stride + step] = bad ? __builtin_nan("") : tab[f].sc * loss[f];
  if (bad) return;
  const int items = F * pmax;
  for (int j = threadIdx.x; j < items; j += blockDim.x) {
    const int f = j / pmax, i = j - f * pmax;
    const ffgp_tree_member* M = tab + f;
    const int P = M->P;
    if (i >= P) continue;
    double* par;
    const double g = ffgp_tree_raw_grad(M, scratch, i, &par);
    double* m = state + (size_t)f * state_stride + i;
    ffgp_adam_update(par, m, m + P, g, lr, b1, b2, eps, bc1, bc2_sqrt);
  }
}

// the loop of ffgp_train_tree_raw and ffgp_train_tree_res_raw (train_tree.h): with r, the members whose r[f].rho_dev is set train on
// targets (and a diagonal extra) that ffgp_tree_resid_form_launch writes into the scratch before each step's likelihoods, the likelihood
// delivers dloss/dr and dloss/ddvec beside them, and ffgp_tree_res_adam_launch takes the step in ffgp_tree_adam_kernel's place
int ffgp_train_tree_impl(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_tree_links* l, const ffgp_residual* r, int steps,
                         const ffgp_adam* opt, double* state_dev, long state_stride, long step0, double* trace_dev, long trace_stride) {
  if (!ffgp_train_args_ok(h, p, l, opt, state_dev, trace_dev, F, steps, step0, trace_stride)) return FFGP_ERR_ARG;
  std::vector<ffgp_tree_member> tab(F);
  std::vector<ffgp_problem> pq(p, p + F);                        // the shadow problems: trees whose leaves read the effective parameters
  std::vector<ffgp_ktree> tq(F);
  std::vector<ffgp_kdesc> kq((size_t)F * FFGP_TREE_MAXL);
  std::vector<ffgp_kdesc_grads> gk((size_t)F * FFGP_TREE_MAXL);
  std::vector<ffgp_grads> g(F);
  const size_t tab_doubles = ((size_t)F * sizeof(ffgp_tree_member) + sizeof(double) - 1) / sizeof(double);
  size_t off = tab_doubles + FFGP_TRAIN_MAXF;                    // [table | losses | per member: effective parameters, gradients]
  int pmax = 0;
  for (int f = 0; f < F; ++f) {
    const ffgp_problem& q = p[f];
    const ffgp_ktree* t = q.tree;
    if (!t || q.pair || q.cov_dev || !t->leaf || t->n_leaves < 2 || t->n_leaves > FFGP_TREE_MAXL || q.D <= 0 || q.D > 128 || q.n <= 0 ||
        q.d <= 0 || !q.X_dev || !q.diag_add_dev || (q.ll_variant != FFGP_LL_V1 && q.ll_variant != FFGP_LL_V2))
      return FFGP_ERR_ARG;
    const bool resid = r && r[f].rho_dev;
    if (resid ? (!r[f].y_low_dev || !r[f].y_high_dev || (!r[f].v_low_dev) != (!r[f].v_high_dev) ||
                 (r[f].v_low_dev && (r[f].v_low_stride < 0 || r[f].v_high_stride < 0)))
              : !q.Y_dev)
      return FFGP_ERR_ARG;
    const int D = q.D, nl = t->n_leaves;
    ffgp_tree_member& M = tab[f];
    memset(&M, 0, sizeof(M));
    int P = 1;
    for (int e = 0; e < nl; ++e) {
      const ffgp_kdesc& k = t->leaf[e];
      const ffgp_leaf_links& ll = l[f].leaf[e];
      if (!ffgp_tree_leaf_trainable(k, ll)) return FFGP_ERR_ARG;
      M.w[e] = const_cast<double*>(k.w_dev);
      M.amp[e] = const_cast<double*>(k.amp_dev);
      M.cen[e] = ll.center_train ? const_cast<double*>(k.center_dev) : nullptr;
      M.w_link[e] = ll.w_link; M.w_c[e] = ll.w_c;
      M.amp_link[e] = ll.amp_link; M.amp_c[e] = ll.amp_c;
      M.nw[e] = ll.w_broadcast ? 1 : D;
      P += M.nw[e] + 1 + (ll.center_train ? D : 0);
    }
    if (state_stride < 2 * (long)(P + (resid ? 1 : 0))) return FFGP_ERR_ARG;
    M.dadd = const_cast<double*>(q.diag_add_dev);
    M.dadd_link = l[f].dadd_link; M.dadd_c = l[f].dadd_c;
    M.sc = (l[f].out_scale == 0.0) ? 1.0 : l[f].out_scale;
    M.D = D; M.nl = nl; M.P = P;
    M.eff = (long)off; off += (size_t)nl * (D + 1) + 1;
    M.geff = (long)off; off += (size_t)nl * (2 * D + 1) + 1;
    pmax = std::max(pmax, P);
  }
  // per residual member [r (n d) | dvec (n) | dloss/dr (n d) | dloss/ddvec (n)], behind the members' parameters
  ffgp_tree_resid rs;
  memset(&rs, 0, sizeof(rs));
  long rmax = 0, res_off[FFGP_TRAIN_MAXF];
  bool any_res = false;
  for (int f = 0; f < F; ++f) {
    if (!(r && r[f].rho_dev)) continue;
    const long n = p[f].n, nd = n * p[f].d;
    res_off[f] = (long)off;
    off += 2 * (size_t)(nd + n);
    rmax = std::max(rmax, std::max(nd, n));
    any_res = true;
  }
  FFGP_HIP(hipSetDevice(h->device));
  if (h->train_tree_bytes < off * sizeof(double)) {      // (every earlier call on this handle has returned: nothing reads the old buffer)
    if (h->train_tree) FFGP_HIP(hipFree(h->train_tree));
    h->train_tree = nullptr;
    h->train_tree_bytes = 0;
    if (hipMalloc(&h->train_tree, off * sizeof(double)) != hipSuccess) {
      (void)hipGetLastError();
      return FFGP_ERR_ALLOC;
    }
    h->train_tree_bytes = off * sizeof(double);
  }
  double* scratch = h->train_tree;
  const ffgp_tree_member* tab_dev = reinterpret_cast<const ffgp_tree_member*>(scratch);
  double* loss = scratch + tab_doubles;
  for (int f = 0; f < F; ++f) {
    const ffgp_tree_member& M = tab[f];
    const int D = M.D;
    double* eff = scratch + M.eff;
    double* ge = scratch + M.geff;
    tq[f] = *p[f].tree;
    tq[f].leaf = &kq[(size_t)f * FFGP_TREE_MAXL];
    for (int e = 0; e < M.nl; ++e) {
      ffgp_kdesc& k = kq[(size_t)f * FFGP_TREE_MAXL + e];
      k = p[f].tree->leaf[e];
      k.w_dev = eff + (size_t)e * (D + 1);
      k.amp_dev = k.w_dev + D;
      ffgp_kdesc_grads& ke = gk[(size_t)f * FFGP_TREE_MAXL + e];
      memset(&ke, 0, sizeof(ke));
      ke.g_w_dev = ge + (size_t)e * (2 * D + 1);
      ke.g_amp_dev = ke.g_w_dev + D;
      if (M.cen[e]) ke.g_center_dev = ke.g_amp_dev + 1;
    }
    pq[f].tree = &tq[f];
    pq[f].diag_add_dev = eff + (size_t)M.nl * (D + 1);
    memset(&g[f], 0, sizeof(ffgp_grads));
    g[f].g_diag_add_dev = ge + (size_t)M.nl * (2 * D + 1);
    g[f].g_pair = &gk[(size_t)f * FFGP_TREE_MAXL];
    if (r && r[f].rho_dev) {
      const long n = p[f].n, nd = n * p[f].d;
      rs.rho[f] = r[f].rho_dev;
      rs.yl[f] = r[f].y_low_dev; rs.yh[f] = r[f].y_high_dev;
      rs.vl[f] = r[f].v_low_dev; rs.vh[f] = r[f].v_high_dev; rs.vls[f] = r[f].v_low_stride; rs.vhs[f] = r[f].v_high_stride;
      rs.r[f] = scratch + res_off[f]; rs.dv[f] = rs.r[f] + nd;
      rs.gY[f] = rs.dv[f] + n; rs.gdv[f] = rs.gY[f] + nd;
      rs.rho_last[f] = r[f].rho_last_dev;
      rs.nd[f] = nd; rs.n[f] = (int)n;
      pq[f].Y_dev = rs.r[f];
      pq[f].diag_vec_dev = rs.vl[f] ? rs.dv[f] : nullptr;
      pq[f].diag_stride = 1;
      g[f].g_Y_dev = rs.gY[f];
      if (rs.vl[f]) g[f].g_diag_vec_dev = rs.gdv[f];
    }
  }
  // (the table's host copy lives until the call's synchronisation below, on every way out)
  if (hipMemcpyAsync(scratch, tab.data(), (size_t)F * sizeof(ffgp_tree_member), hipMemcpyHostToDevice, h->stream) != hipSuccess) {
    hipStreamSynchronize(h->stream);
    return FFGP_ERR_HIP;
  }
  // the sticky status word starts clean: a failure of an EARLIER call on this handle is that call's to report
  int lrc = ffgp_zero_async(h, h->d_info, 2 * sizeof(int));
  h->defer_info_copy = 1;      // (the per-call read-back of the status word: once, after the loop)
  h->fold_info = 1;            // the Adam kernel clears / accumulates the status words; the factorisations of a step share info[0]
  for (int k = 0; k < steps && lrc == FFGP_OK; ++k) {
    hipLaunchKernelGGL(ffgp_tree_link_fwd, dim3(F), dim3(256), 0, h->stream, tab_dev, scratch);
    if (any_res) ffgp_tree_resid_form_launch(h->stream, F, rs, rmax);
    for (int f = 0; f < F && lrc == FFGP_OK; ++f) lrc = ffgp_nlml_fused_async(h, &pq[f], loss + f, &g[f]);
    if (lrc != FFGP_OK) break;
    double bc1, bc2_sqrt;
    ffgp_adam_bc(opt, step0, k, &bc1, &bc2_sqrt);
    if (any_res) {
      ffgp_tree_res_adam_launch(h->stream, F, pmax, rs, tab_dev, scratch, state_dev, state_stride, opt, bc1, bc2_sqrt, loss, trace_dev,
                                trace_stride, k, h->d_info);
      continue;
    }
    hipLaunchKernelGGL(ffgp_tree_adam_kernel, dim3(1), dim3(256), 0, h->stream, F, pmax, tab_dev, scratch, state_dev, state_stride, opt->lr,
                       opt->beta1, opt->beta2, opt->eps, bc1, bc2_sqrt, loss, trace_dev, trace_stride, k, h->d_info);
  }
  h->defer_info_copy = 0;
  h->fold_info = 0;
  if (lrc != FFGP_OK) {
    hipStreamSynchronize(h->stream);
    return lrc;
  }
  if (hipGetLastError() != hipSuccess) {
    hipStreamSynchronize(h->stream);
    return FFGP_ERR_HIP;
  }
  FFGP_HIP(hipMemcpyAsync(h->h_info, h->d_info, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  ffgp_invalidate(h);
  return ffgp_wait(h);
}

extern "C" int ffgp_train_tree_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_tree_links* l, int steps, const ffgp_adam* opt,
                                   double* state_dev, long state_stride, long step0, double* trace_dev, long trace_stride) {
  return ffgp_train_tree_impl(h, F, p, l, nullptr, steps, opt, state_dev, state_stride, step0, trace_dev, trace_stride);
}
