// Fused NLML (+ gradients) of one problem: the links around the raw-parameter call, the single-problem drivers (blocked path and the
// small-N paths), the forward call as a captured graph -- and the pieces the batch driver (nlml_batch.hip) and the training loop
// (train_loop.hip) share with them.  See include/ffgp.h.
#include "drivers.h"

__global__ void ffgp_copy_lower_kernel(const double* __restrict__ src, int lds_, double* __restrict__ dst, int ldd, int n) {
  const int c = blockIdx.x * 32 + (threadIdx.x & 31), r = blockIdx.y * 32 + (threadIdx.x >> 5) * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int rr = r + k;
    if (rr < n && c <= rr) dst[(size_t)rr * ldd + c] = src[(size_t)rr * lds_ + c];
  }
}

// lower triangle -> full symmetric matrix (gradient w.r.t. a caller-built covariance)
__global__ void ffgp_symmetrize_kernel(const double* __restrict__ Gl, int ldg, double* __restrict__ out, int ldo, int n,
                                       double scale) {
  const int c = blockIdx.x * 32 + (threadIdx.x & 31), r = blockIdx.y * 32 + (threadIdx.x >> 5) * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int rr = r + k;
    if (rr < n && c < n) out[(size_t)rr * ldo + c] = scale * ((c <= rr) ? Gl[(size_t)rr * ldg + c] : Gl[(size_t)c * ldg + rr]);
  }
}

// ---- raw parameters: elementwise links around the fused call (ffgp_link_val / ffgp_link_der: drivers.h)
// eff = [w (D) | amp | dadd]
extern "C" __global__ void ffgp_link_fwd(ffgp_links l, int D, const double* __restrict__ rw, const double* __restrict__ ramp,
                              const double* __restrict__ rdadd, double* __restrict__ eff) {
  const int t = threadIdx.x;
  if (t < D) eff[t] = ffgp_link_val(l.w_link, rw[l.w_broadcast ? 0 : t], l.w_c);
  if (t == 0) {
    eff[D] = ffgp_link_val(l.amp_link, ramp[0], l.amp_c);
    if (rdadd) eff[D + 1] = ffgp_link_val(l.dadd_link, rdadd[0], l.dadd_c);
  }
}
// geff = [g_w (D) | g_amp | g_dadd] -> gradients with respect to the raw parameters (any output pointer may be null)
extern "C" __global__ void ffgp_link_bwd(ffgp_links l, int D, const double* __restrict__ rw, const double* __restrict__ ramp,
                              const double* __restrict__ rdadd, const double* __restrict__ geff, double* __restrict__ g_rw,
                              double* __restrict__ g_ramp, double* __restrict__ g_rdadd, double sc) {
  const int t = threadIdx.x;
  if (g_rw) {
    if (!l.w_broadcast) {
      if (t < D) g_rw[t] = sc * geff[t] * ffgp_link_der(l.w_link, rw[t], l.w_c);
    } else if (t == 0) {
      double s = 0.0;
      for (int k = 0; k < D; ++k) s += geff[k];
      g_rw[0] = sc * s * ffgp_link_der(l.w_link, rw[0], l.w_c);
    }
  }
  if (t == 0) {
    if (g_ramp) g_ramp[0] = sc * geff[D] * ffgp_link_der(l.amp_link, ramp[0], l.amp_c);
    if (g_rdadd && rdadd) g_rdadd[0] = sc * geff[D + 1] * ffgp_link_der(l.dadd_link, rdadd[0], l.dadd_c);
  }
}

// info[1] is sticky: the first failing pivot of any fused call enqueued since the last ffgp_wait
extern "C" __global__ void ffgp_sticky_info_kernel(int* info) {
  if (info[1] == 0 && info[0] != 0) info[1] = info[0];
}

extern "C" __global__ void ffgp_scale_outputs(double sc, double* __restrict__ nll, double* __restrict__ gY, long nY, double* __restrict__ gv, long nv,
                                   double* __restrict__ gk) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t == 0) {
    nll[0] *= sc;
    if (gk) gk[0] *= sc;
  }
  if (gY && t < nY) gY[t] *= sc;
  if (gv && t < nv) gv[t] *= sc;
}

// ---- shared pieces (drivers.h) ---------------------------------------------------------------------------------------------
int ffgp_finish_info(ffgp_handle* h) {
  if (!h->fold_info) hipLaunchKernelGGL(ffgp_sticky_info_kernel, dim3(1), dim3(1), 0, h->stream, h->d_info);
  if (!h->defer_info_copy) FFGP_HIP(hipMemcpyAsync(h->h_info, h->d_info, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  return FFGP_OK;
}

bool ffgp_links_redirect(const ffgp_problem* p, const ffgp_links* l, const ffgp_grads* g, double* eff, double* geff, ffgp_problem* q,
                         ffgp_grads* gq) {
  const int D = p->D;
  *q = *p;
  if (l) {
    q->w_dev = eff;
    q->amp_dev = eff + D;
    if (p->diag_add_dev) q->diag_add_dev = eff + D + 1;
  }
  if (!g) return false;
  *gq = *g;
  if (!l) return false;
  if (g->g_w_dev) gq->g_w_dev = geff;
  if (g->g_amp_dev) gq->g_amp_dev = geff + D;
  if (g->g_diag_add_dev) gq->g_diag_add_dev = geff + D + 1;
  return g->g_w_dev || g->g_amp_dev || g->g_diag_add_dev;
}

void ffgp_links_finish(ffgp_handle* h, const ffgp_problem* p, const ffgp_links* l, const ffgp_grads* g, const double* geff, bool chain,
                       double* nll_dev) {
  const double sc = (l->out_scale == 0.0) ? 1.0 : l->out_scale;
  if (chain)
    hipLaunchKernelGGL(ffgp_link_bwd, dim3(1), dim3(128), 0, h->stream, *l, p->D, p->w_dev, p->amp_dev, p->diag_add_dev, geff, g->g_w_dev,
                       g->g_amp_dev, g->g_diag_add_dev, sc);
  if (sc != 1.0) {
    const long nY = (g && g->g_Y_dev) ? (long)p->n * p->d : 0, nv = (g && g->g_diag_vec_dev) ? p->n : 0;
    const long tot = nY > nv ? nY : nv;
    hipLaunchKernelGGL(ffgp_scale_outputs, dim3((unsigned)((tot > 0 ? tot : 1) + 255) / 256), dim3(256), 0, h->stream, sc, nll_dev,
                       g ? g->g_Y_dev : nullptr, nY, g ? g->g_diag_vec_dev : nullptr, nv, g ? g->g_kparam_dev : nullptr);
  }
}

ffgp_grad_scratch ffgp_grad_scratch_sizes(int n, int d, int D, int ll_variant, int pair_leaves) {
  const size_t ld = ffgp_round_up(n, 16);
  const size_t n1 = ffgp_round_up((n + 1) / 2, FFGP_NB);      // the top level's split of the triangular inverse
  ffgp_grad_scratch s;
  s.X = (size_t)n * ld;
  s.S = (size_t)n * ld;
  s.T = 2 * (n1 * n1 + 16);
  s.At = (size_t)d * ld;
  s.P = (pair_leaves ? ffgp_grad_pair_partial_doubles(n, n, D, 0, pair_leaves) : ffgp_grad_partial_doubles(n, D)) + 16;
  s.Ct = s.Bt = (ll_variant == FFGP_LL_V2) ? (size_t)d * ld : 0;
  return s;
}

int ffgp_grad_v1_stages(ffgp_handle* h, const ffgp_problem* q, const ffgp_grads* gq, int D, double mean_jitter, const double* Gt,
                        const double* X, double* S, double* At, double* P, int ld) {
  const int n = q->n, d = q->d;
  // A^T = Gamma^T L^-1   (d x n)
  FFGP_CHECK(ffgp_gemm_launch(h, OP_KMAJOR, OP_MNMAJOR, TILES_FULL, 0, Gt, ld, X, ld, At, ld, d, n, n, 1.0, 0.0, TRI_LO_J));
  // G = d/2 Sigma^-1 - 1/2 A A^T   (lower, in place of Sigma^-1)
  FFGP_CHECK(ffgp_gemm_launch(h, OP_MNMAJOR, OP_MNMAJOR, TILES_LOWER, 0, At, ld, At, ld, S, ld, n, n, d, -0.5, 0.5 * (double)d));
  return ffgp_grad_impl(h, q->X_dev, n, D, q->w_dev, q->amp_dev, q->clamp_min, S, ld, mean_jitter, gq->g_w_dev, gq->g_amp_dev,
                        gq->g_diag_add_dev, gq->g_diag_vec_dev, P, q->kfun, q->kparam, gq->g_kparam_dev);
}

// ---- one problem -----------------------------------------------------------------------------------------------------------
// 40 < n <= 128 (one diagonal block): assemble and factor with the blocked path's kernels, then ONE finishing kernel (small.hip,
// FROM_FACTOR) for everything else -- links of the raw-parameter call included.  p holds the raw parameters when l is given.
static int small2_enqueue(ffgp_handle* h, const ffgp_problem* p, const ffgp_links* l, double* nll_dev, const ffgp_grads* g) {
  FFGP_HIP(hipSetDevice(h->device));
  const int n = p->n, D = p->D;
  const size_t ld = ffgp_round_up(n, 16);
  FFGP_CHECK(ffgp_ensure_ws(h, (size_t)(n + 16) * ld * sizeof(double)));
  h->n_stages = 0;
  if (l) {
    if (!h->d_link) FFGP_HIP(hipMalloc(&h->d_link, 512 * sizeof(double)));
    hipLaunchKernelGGL(ffgp_link_fwd, dim3(1), dim3(128), 0, h->stream, *l, D, p->w_dev, p->amp_dev, p->diag_add_dev, h->d_link);
  }
  ffgp_problem q;      // (the assembly reads the effective parameters; the finishing kernel takes the raw ones and the links)
  ffgp_links_redirect(p, l, nullptr, h->d_link, nullptr, &q, nullptr);
  FFGP_CHECK(ffgp_assemble_impl(h, p->X_dev, n, p->X_dev, n, D, q.w_dev, q.amp_dev, p->clamp_min, q.diag_add_dev, p->diag_vec_dev,
                                p->diag_stride, p->add_mat_dev, p->ld_add, p->add_all, p->mean_jitter, h->ws, (int)ld, 1, p->kfun, p->kparam));
  FFGP_CHECK(ffgp_potrf_impl(h, h->ws, n, n, (int)ld, 0));
  FFGP_CHECK(ffgp_small_enqueue(h, p, l, nll_dev, g, h->dinv));
  return ffgp_finish_info(h);
}

static int nlml_fused_plain(ffgp_handle* h, const ffgp_problem* p, double* nll_dev, const ffgp_grads* g) {
  if (!h || !p || !nll_dev) return FFGP_ERR_ARG;
  const bool given_cov = (p->cov_dev != nullptr);
  if (p->n <= 0 || p->d <= 0 || !p->Y_dev) return FFGP_ERR_ARG;
  const bool pair = (!given_cov && (p->pair != nullptr || p->tree != nullptr));
  const ffgp_ktree pair2 = {2, FFGP_TREE_CHAIN, {p->pair_op, 0, 0}, p->pair};
  const ffgp_ktree* tree = p->tree ? p->tree : &pair2;
  if (pair && (tree->n_leaves < 2 || tree->n_leaves > 4 || !tree->leaf)) return FFGP_ERR_ARG;
  if (!given_cov && (p->D <= 0 || !p->X_dev)) return FFGP_ERR_ARG;
  if (!given_cov && !pair && (!p->w_dev || !p->amp_dev)) return FFGP_ERR_ARG;
  if (given_cov && p->ld_cov < p->n) return FFGP_ERR_ARG;
  if (p->ll_variant != FFGP_LL_V1 && p->ll_variant != FFGP_LL_V2) return FFGP_ERR_ARG;
  if (!pair && (p->kfun < FFGP_KFUN_SE || p->kfun > FFGP_KFUN_RQ)) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  const int n = p->n, D = given_cov ? 1 : p->D, d = p->d;
  const bool want_grad = ffgp_wants_grad(g) || (g && (g->g_cov_dev || (pair && g->g_pair)));
  if (pair && g && (g->g_w_dev || g->g_amp_dev || g->g_kparam_dev)) return FFGP_ERR_ARG;   // a pair's kernel gradients travel in g_pair
  if (given_cov && g && (g->g_w_dev || g->g_amp_dev || g->g_kparam_dev)) return FFGP_ERR_ARG;
  if (g && g->g_cov_dev && g->ld_gcov < p->n) return FFGP_ERR_ARG;
  const bool v2 = (p->ll_variant == FFGP_LL_V2);
  const size_t ld = ffgp_round_up(n, 16);
  const size_t w0 = (size_t)(n + d) * ld;          // Sigma | Y^T  ->  L | Gamma^T
  size_t total = w0;
  size_t o_X = 0, o_S = 0, o_T = 0, o_Ttop = 0, o_At = 0, o_P = 0, o_A = 0, o_Ct = 0, o_Bt = 0;
  if (want_grad) {
    const ffgp_grad_scratch gs = ffgp_grad_scratch_sizes(n, d, D, p->ll_variant, pair ? tree->n_leaves : 0);
    o_X = total; total += gs.X;
    o_S = total; total += gs.S;
    o_T = total; total += gs.T;
    o_Ttop = o_T + gs.T / 2;           // (the second half: the top level's L21 X11 when the inverse is split)
    o_At = total; total += gs.At;
    o_P = total; total += gs.P;
    o_Ct = total; total += gs.Ct;      // (V2 only: both are empty otherwise)
    o_Bt = total; total += gs.Bt;
  }
  if (v2 && !want_grad) {
    o_A = total; total += (size_t)n * ffgp_round_up(d, 2) + 16;
  }
  if (ffgp_small_ok(h, p, g)) {   // the sizes of the reference's own demos: one workgroup, one launch (small.hip)
    h->n_stages = 0;
    FFGP_CHECK(ffgp_small_enqueue(h, p, nullptr, nll_dev, g));
    return ffgp_finish_info(h);
  }
  if (ffgp_small2_ok(h, p, g)) return small2_enqueue(h, p, nullptr, nll_dev, g);
  FFGP_CHECK(ffgp_ensure_ws(h, total * sizeof(double)));
  double* W0 = h->ws;
  double* Gt = W0 + (size_t)n * ld;  // passenger rows: Gamma^T (d x n)

  h->n_stages = 0;
  stage_mark(h, 0);
  if (given_cov) {
    hipLaunchKernelGGL(ffgp_copy_lower_kernel, dim3((n + 31) / 32, (n + 31) / 32), dim3(256), 0, h->stream, p->cov_dev, p->ld_cov,
                       W0, (int)ld, n);
  } else if (pair) {
    FFGP_CHECK(ffgp_assemble_pair_impl(h, p->X_dev, n, p->X_dev, n, D, tree, p->diag_add_dev, p->diag_vec_dev,
                                       p->diag_stride, p->add_mat_dev, p->ld_add, p->add_all, p->mean_jitter, W0, (int)ld, 1));
  } else {
    FFGP_CHECK(ffgp_assemble_impl(h, p->X_dev, n, p->X_dev, n, D, p->w_dev, p->amp_dev, p->clamp_min, p->diag_add_dev,
                                  p->diag_vec_dev, p->diag_stride, p->add_mat_dev, p->ld_add, p->add_all, p->mean_jitter,
                                  W0, (int)ld, 1, p->kfun, p->kparam));
  }
  FFGP_CHECK(ffgp_transpose(h, p->Y_dev, n, d, d, Gt, (int)ld, 1.0));
  stage_mark(h, 1);
  // forward + gradients of a large block: the head of the triangular inverse (everything that only needs the factor's first n1s
  // columns: 3/4 of its flops) runs on a third stream under the factorisation's chain-bound tail
  int n1s = 0;
  if (want_grad && h->trtri_overlap && h->lookahead && !h->use_naive && n >= 4096 && n > h->la_min_n) {
    n1s = FFGP_NB;
    while (2 * n1s < n) n1s *= 2;
    if (n1s % h->nb_outer != 0) n1s = 0;
  }
  h->tri_hook_fired = 0;
  h->tri_hook_col = n1s;
  if (n1s) FFGP_CHECK(ffgp_ensure_aux2(h));
  const int prc = ffgp_potrf_impl(h, W0, n, n + d, (int)ld, 0);
  h->tri_hook_col = 0;
  FFGP_CHECK(prc);
  const bool split_inv = n1s && h->tri_hook_fired;
  if (split_inv) {
    hipStream_t main_s = h->stream;
    FFGP_HIP(hipStreamWaitEvent(h->aux2, h->tri_ev[0], 0));
    h->stream = h->aux2;
    const int hrc = ffgp_trtri_head(h, W0, n, (int)ld, h->ws + o_X, (int)ld, h->ws + o_T, h->ws + o_Ttop, n1s);
    h->stream = main_s;
    FFGP_CHECK(hrc);
    FFGP_HIP(hipEventRecord(h->tri_ev[1], h->aux2));
  }
  stage_mark(h, 2);
  if (!v2) {
    FFGP_CHECK(ffgp_nll_reduce_impl(h, FFGP_LL_V1, W0, n, (int)ld, Gt, d, n, (int)ld, d, p->pi_const, nll_dev));
  } else if (!want_grad) {
    // A = L^-T Gamma  (n x d), then ||A||^2
    double* A = h->ws + o_A;
    const int lda2 = ffgp_round_up(d, 2);
    FFGP_CHECK(ffgp_transpose(h, Gt, d, n, (int)ld, A, lda2, 1.0));
    FFGP_CHECK(ffgp_trsm_lower_t_impl(h, W0, n, (int)ld, A, d, lda2));
    FFGP_CHECK(ffgp_nll_reduce_impl(h, FFGP_LL_V2, W0, n, (int)ld, A, n, d, lda2, d, p->pi_const, nll_dev));
  }
  stage_mark(h, 3);
  if (want_grad) {
    double* X = h->ws + o_X;
    double* S = h->ws + o_S;
    double* T = h->ws + o_T;
    double* At = h->ws + o_At;
    double* P = h->ws + o_P;
    if (split_inv) {
      FFGP_HIP(hipStreamWaitEvent(h->stream, h->tri_ev[1], 0));
      FFGP_CHECK(ffgp_trtri_tail(h, W0, n, (int)ld, X, (int)ld, T, h->ws + o_Ttop, n1s));
    } else {
      FFGP_CHECK(ffgp_trtri_impl(h, W0, n, (int)ld, X, (int)ld, T));
    }
    stage_mark(h, 4);
    FFGP_CHECK(ffgp_lauum_impl(h, X, n, (int)ld, S, (int)ld));
    stage_mark(h, 5);
    const double* gYt = At;  // V1: d nll / dY = A
    const double mj = given_cov ? 0.0 : p->mean_jitter;
    // (a pair: only the trace / diagonal part of the parameter gradients runs in either branch, tr G lands in d_scal[4])
    if (!v2) {
      FFGP_CHECK(ffgp_grad_v1_stages(h, p, g, D, mj, Gt, X, S, At, P, (int)ld));
    } else {
      // A^T = Gamma^T L^-1   (d x n)
      FFGP_CHECK(ffgp_gemm_launch(h, OP_KMAJOR, OP_MNMAJOR, TILES_FULL, 0, Gt, (int)ld, X, (int)ld, At, (int)ld, d, n, n, 1.0, 0.0,
                                  TRI_LO_J));
      // V2 (Sigma^-2 quadratic form): value from ||A||^2; B = Sigma^-1 A = L^-T (L^-1 A);
      // G = d/2 Sigma^-1 - 1/2 (A B^T + B A^T);  d(-LL)/dY = B       
      double* Ct = h->ws + o_Ct;
      double* Bt = h->ws + o_Bt;
      FFGP_CHECK(ffgp_nll_reduce_impl(h, FFGP_LL_V2, W0, n, (int)ld, At, d, n, (int)ld, d, p->pi_const, nll_dev));
      FFGP_CHECK(ffgp_gemm_launch(h, OP_KMAJOR, OP_KMAJOR, TILES_FULL, 0, At, (int)ld, X, (int)ld, Ct, (int)ld, d, n, n, 1.0, 0.0,
                                  TRI_HI_J));
      FFGP_CHECK(ffgp_gemm_launch(h, OP_KMAJOR, OP_MNMAJOR, TILES_FULL, 0, Ct, (int)ld, X, (int)ld, Bt, (int)ld, d, n, n, 1.0,
                                  0.0, TRI_LO_J));
      FFGP_CHECK(ffgp_gemm_launch(h, OP_MNMAJOR, OP_MNMAJOR, TILES_LOWER, 0, At, (int)ld, Bt, (int)ld, S, (int)ld, n, n, d,
                                  -0.5, 0.5 * (double)d));
      FFGP_CHECK(ffgp_gemm_launch(h, OP_MNMAJOR, OP_MNMAJOR, TILES_LOWER, 0, Bt, (int)ld, At, (int)ld, S, (int)ld, n, n, d,
                                  -0.5, 1.0));
      FFGP_CHECK(ffgp_grad_impl(h, p->X_dev, n, D, p->w_dev, p->amp_dev, p->clamp_min, S, (int)ld, mj, g->g_w_dev, g->g_amp_dev,
                                g->g_diag_add_dev, g->g_diag_vec_dev, P, p->kfun, p->kparam, g->g_kparam_dev));
      gYt = Bt;
    }
    if (pair && g->g_pair)
      FFGP_CHECK(ffgp_grad_pair_impl(h, p->X_dev, n, p->X_dev, n, D, tree, S, (int)ld, 0, h->d_scal + 4,
                                     (p->mean_jitter != 0.0) ? p->mean_jitter / ((double)n * (double)n) : 0.0, P, g->g_pair));
    if (g->g_cov_dev)
      hipLaunchKernelGGL(ffgp_symmetrize_kernel, dim3((n + 31) / 32, (n + 31) / 32), dim3(256), 0, h->stream, S, (int)ld,
                         g->g_cov_dev, g->ld_gcov, n, 1.0);
    if (g->g_Y_dev) FFGP_CHECK(ffgp_transpose(h, gYt, d, n, (int)ld, g->g_Y_dev, d, 1.0));
    stage_mark(h, 6);
  }
  return ffgp_finish_info(h);
}

// copies a captured graph's staged outputs (value, then an optional gradient block) into the caller's buffers (the forward graph
// below)
extern "C" __global__ void ffgp_rawg_copy_out(const double* __restrict__ stage, long len, double* __restrict__ nll, double* __restrict__ gbase) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t == 0) nll[0] = stage[0];
  if (t < len) gbase[t] = stage[1 + t];
}

// ---- the forward call as one captured graph (option "fwd_graph", default 0) ---------------------------------------------------
// A likelihood at N = 16384 is ~400 launches on two streams, issued by ONE host thread a few microseconds ahead of the GPU: on a busy
// host the step stretches (29 -> 35 ms was seen).  With the option on, the second identical forward-only call (same
// problem struct: same device buffers, sizes, options) is captured -- both streams: the side stream forks from and joins the capturing
// stream through the look-ahead's own events -- into a hipGraph that writes its value to a handle-owned slot, and from then on every
// such call is ONE hipGraphLaunch plus a one-word copy into the caller's output.  Same kernels, same order per stream, same values
// (test_forward_graph_replay); dropped with any option or buffer change.  Calls with gradients, with stage timing, or on the small-N
// paths are never captured.
// MEASURED (tools/host_load_probe.py, ROCm 7.2): idle host 28.65-29.02 ms launch by launch, 28.83-29.12 ms as a graph at N = 16384;
// 1.84 against 2.25-2.32 ms at N = 4096; with the pod's CPU quota exhausted by spinning processes both take exactly one cgroup period
// (100.0 ms) per step.  The runtime walks the graph's nodes on a host thread and issues them one by one: a graph does not take the host
// out of the step here.  What does help a multi-rank run is bench.py's per-rank CPU affinity.  Default off.
extern "C" int ffgp_nlml_fused_async(ffgp_handle* h, const ffgp_problem* p, double* nll_dev, const ffgp_grads* g) {
  if (!h || !p || !nll_dev) return FFGP_ERR_ARG;
  const bool wants_grad = ffgp_wants_grad(g) || (g && (g->g_cov_dev || g->g_pair));
  const bool eligible = h->fwd_graph && !wants_grad && h->timing == 0 && p->n > FFGP_NB && !h->use_naive;
  if (!eligible) return nlml_fused_plain(h, p, nll_dev, g);
  if (!h->fwdg) {
    h->fwdg = new RawGraph();
    memset(h->fwdg, 0, sizeof(RawGraph));
  }
  RawGraph* r = h->fwdg;
  const bool same = (r->seen || r->valid) && !memcmp(&r->p, p, sizeof(ffgp_problem)) && r->epoch == h->alloc_epoch;
  FFGP_HIP(hipSetDevice(h->device));
  auto replay = [&]() -> int {
    FFGP_HIP(hipGraphLaunch(r->exec, h->stream));
    hipLaunchKernelGGL(ffgp_rawg_copy_out, dim3(1), dim3(256), 0, h->stream, r->stage, 0L, nll_dev, (double*)nullptr);
    ffgp_invalidate(h);     // the replay rewrote the handle's factor on the device; the host-side keys do not know
    h->graph_replays += 1;
    return hipGetLastError() == hipSuccess ? FFGP_OK : FFGP_ERR_HIP;
  };
  if (same && r->valid) return replay();
  if (!same) {              // first sight of this call: run it plainly (sizes every buffer, sets every kernel attribute), remember it
    ffgp_rawg_drop(r);
    const int rc = nlml_fused_plain(h, p, nll_dev, g);
    r->p = *p;
    r->epoch = h->alloc_epoch;
    r->seen = (rc == FFGP_OK) ? 1 : 0;
    return rc;
  }
  if (!r->stage) {
    FFGP_HIP(hipMalloc(&r->stage, 2 * sizeof(double)));
  }
  r->seen = 0;
  if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    return nlml_fused_plain(h, p, nll_dev, g);
  }
  const int rc = nlml_fused_plain(h, p, r->stage, nullptr);
  hipGraph_t graph = nullptr;
  const hipError_t ec = hipStreamEndCapture(h->stream, &graph);
  if (rc != FFGP_OK || ec != hipSuccess || !graph || r->epoch != h->alloc_epoch) {
    (void)hipGetLastError();
    if (graph) hipGraphDestroy(graph);
    if (getenv("FFGP_GRAPH_DEBUG")) fprintf(stderr, "[ffgp] forward graph: capture failed (rc %d, hip %d)\n", rc, (int)ec);
    return nlml_fused_plain(h, p, nll_dev, g);
  }
  hipGraphExec_t exec = nullptr;
  if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
    (void)hipGetLastError();
    hipGraphDestroy(graph);
    return nlml_fused_plain(h, p, nll_dev, g);
  }
  r->graph = graph;
  r->exec = exec;
  r->valid = true;
  return replay();
}

extern "C" int ffgp_nlml_fused_raw_async(ffgp_handle* h, const ffgp_problem* p, const ffgp_links* l, double* nll_dev, const ffgp_grads* g) {
  if (!h || !p || !l || !nll_dev) return FFGP_ERR_ARG;
  if (p->cov_dev || p->pair || p->tree || !p->w_dev || !p->amp_dev || p->D <= 0 || p->D > 128) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  if (p->n <= 0 || p->d <= 0 || !p->X_dev || !p->Y_dev || (p->ll_variant != FFGP_LL_V1 && p->ll_variant != FFGP_LL_V2)) return FFGP_ERR_ARG;
  if (!h->fold_info && ffgp_small_mfma_ok(h, p, g)) {   // n <= 128: ONE launch on the matrix cores (train.hip, evaluate mode) instead of the scalar one-workgroup
                                                        // kernel (n <= 40) or ~13 launches of the blocked path
    h->n_stages = 0;
    FFGP_CHECK(ffgp_zero_async(h, h->d_info, sizeof(int)));
    FFGP_CHECK(ffgp_small_mfma_enqueue(h, 1, p, l, nll_dev, g, 0));
    FFGP_CHECK(ffgp_finish_info(h));      // (fold_info is off on this path)
    ffgp_invalidate(h);
    return FFGP_OK;
  }
  if (ffgp_small_ok(h, p, g)) {   // one kernel: links, likelihood, gradients, chain rule, output scale
    h->n_stages = 0;
    FFGP_CHECK(ffgp_small_enqueue(h, p, l, nll_dev, g));
    return ffgp_finish_info(h);
  }
  if (ffgp_small2_ok(h, p, g)) return small2_enqueue(h, p, l, nll_dev, g);
  if (!h->d_link) FFGP_HIP(hipMalloc(&h->d_link, 512 * sizeof(double)));
  double* eff = h->d_link;
  double* geff = h->d_link + 256;
  hipLaunchKernelGGL(ffgp_link_fwd, dim3(1), dim3(128), 0, h->stream, *l, p->D, p->w_dev, p->amp_dev, p->diag_add_dev, eff);
  ffgp_problem q;
  ffgp_grads gq;
  const bool chain = ffgp_links_redirect(p, l, g, eff, geff, &q, &gq);
  FFGP_CHECK(ffgp_nlml_fused_async(h, &q, nll_dev, g ? &gq : nullptr));
  // (ffgp_train_raw with one model, fold_info: the Adam kernel applies the links' chain rule itself)
  ffgp_links_finish(h, p, l, g, geff, chain && !h->fold_info, nll_dev);
  if (hipGetLastError() != hipSuccess) return FFGP_ERR_HIP;
  return FFGP_OK;
}

extern "C" {

int ffgp_wait(ffgp_handle* h) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  FFGP_HIP(hipStreamSynchronize(h->stream));
  stage_collect(h);
  const int rc = h->h_info[1] ? h->h_info[1] : h->h_info[0];
  if (h->h_info[1]) {
    h->h_info[1] = 0;
    FFGP_HIP(hipMemsetAsync(h->d_info + 1, 0, sizeof(int), h->stream));
  }
  return ffgp_map_info(rc);
}

int ffgp_nlml_fused(ffgp_handle* h, const ffgp_problem* p, double* nll_dev, const ffgp_grads* g) {
  FFGP_CHECK(ffgp_nlml_fused_async(h, p, nll_dev, g));
  return ffgp_wait(h);
}

int ffgp_nlml_fused_raw(ffgp_handle* h, const ffgp_problem* p, const ffgp_links* l, double* nll_dev, const ffgp_grads* g) {
  FFGP_CHECK(ffgp_nlml_fused_raw_async(h, p, l, nll_dev, g));
  return ffgp_wait(h);
}

int ffgp_nlml_fused_small_batch_async(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* l, double* nll_dev,
                                      const ffgp_grads* g) {
  if (!h || !p || !nll_dev || F <= 0) return FFGP_ERR_ARG;
  for (int f = 0; f < F; ++f)
    if (!ffgp_small_batch_ok(p + f, g ? g + f : nullptr)) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  h->n_stages = 0;
  FFGP_CHECK(ffgp_zero_async(h, h->d_info, sizeof(int)));
  bool mfma = true;      // (round 6: the one-workgroup MFMA kernel of train.hip, when every problem is within its limits)
  for (int f = 0; f < F && mfma; ++f) mfma = ffgp_small_mfma_ok(h, p + f, g ? g + f : nullptr);
  if (mfma) FFGP_CHECK(ffgp_small_mfma_enqueue(h, F, p, l, nll_dev, g, 1));
  else FFGP_CHECK(ffgp_small_batch_enqueue(h, F, p, l, nll_dev, g));
  return ffgp_finish_info(h);
}

int ffgp_nlml_fused_small_batch(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* l, double* nll_dev, const ffgp_grads* g) {
  FFGP_CHECK(ffgp_nlml_fused_small_batch_async(h, F, p, l, nll_dev, g));
  return ffgp_wait(h);
}

}  // extern "C"
