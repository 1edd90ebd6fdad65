// libffgp C ABI: the thin entry points around the kernels' launchers, the explicit inverse, RCCL, the posterior.  The handle lives in
// handle.hip, the likelihood drivers in nlml.hip / nlml_batch.hip, the training loop in train_loop.hip.  See include/ffgp.h.
#include "drivers.h"

extern "C" {

int ffgp_assemble(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const double* w,
                  const double* amp, double clamp_min, const double* diag_add, const double* diag_vec, long diag_stride,
                  const double* add_mat, int ld_add, double add_all, double mean_jitter, double* K, int ldk,
                  int lower_only, int kfun, double kparam) {
  if (!h) return FFGP_ERR_ARG;
  if (kfun < FFGP_KFUN_SE || kfun > FFGP_KFUN_RQ) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_assemble_impl(h, X1, n1, X2, n2, D, w, amp, clamp_min, diag_add, diag_vec, diag_stride, add_mat, ld_add,
                            add_all, mean_jitter, K, ldk, lower_only, kfun, kparam);
}

int ffgp_potrf_rows(ffgp_handle* h, double* A, int n, int mtot, int lda) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_potrf_impl(h, A, n, mtot, lda, 1);
}

int ffgp_potrf(ffgp_handle* h, double* A, int n, int lda) { return ffgp_potrf_rows(h, A, n, n, lda); }

int ffgp_trsm_lower(ffgp_handle* h, const double* L, int n, int ldl, double* B, int nrhs, int ldb) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_trsm_lower_impl(h, L, n, ldl, B, nrhs, ldb);
}

int ffgp_trsm_lower_t(ffgp_handle* h, const double* L, int n, int ldl, double* B, int nrhs, int ldb) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_trsm_lower_t_impl(h, L, n, ldl, B, nrhs, ldb);
}

int ffgp_potrs(ffgp_handle* h, const double* L, int n, int ldl, double* B, int nrhs, int ldb) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  FFGP_CHECK(ffgp_trsm_lower_impl(h, L, n, ldl, B, nrhs, ldb));
  return ffgp_trsm_lower_t_impl(h, L, n, ldl, B, nrhs, ldb);
}

int ffgp_nll_reduce(ffgp_handle* h, int variant, const double* L, int n, int ldl, const double* M, int d, int ldm,
                    double pi_const, double* out_dev) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_nll_reduce_impl(h, variant, L, n, ldl, M, n, d, ldm, d, pi_const, out_dev);
}

int ffgp_gemm(ffgp_handle* h, int opa, int opb, int lower_tiles, int tri, const double* A, int lda, const double* B, int ldb,
              double* C, int ldc, int m, int n, int k, double alpha, double beta) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_gemm_launch(h, opa ? OP_MNMAJOR : OP_KMAJOR, opb ? OP_MNMAJOR : OP_KMAJOR, lower_tiles ? TILES_LOWER : TILES_FULL,
                          0, A, lda, B, ldb, C, ldc, m, n, k, alpha, beta, tri);
}

int ffgp_kernel_input_weights(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const double* w,
                              const double* amp, double clamp_min, int kfun, double kparam, const double* dK, int ldk,
                              double* Wt, int ldw) {
  if (!h) return FFGP_ERR_ARG;
  if (kfun < FFGP_KFUN_SE || kfun > FFGP_KFUN_RQ) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_kernel_wt_impl(h, X1, n1, X2, n2, D, w, amp, clamp_min, kfun, kparam, dK, ldk, Wt, ldw);
}

int ffgp_syevj_small(ffgp_handle* h, const double* M, int n, int ldm, int batch, long strideM, double* Q, int ldq, long strideQ,
                     double* evals, long strideE, int descending) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_syevj_small_impl(h, M, n, ldm, batch, strideM, Q, ldq, strideQ, evals, strideE, descending);
}

int ffgp_syev_lds(ffgp_handle* h, const double* M, int n, int ldm, int batch, long strideM, double* Q, int ldq, long strideQ,
                  double* evals, long strideE, int descending, int* info) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_syev_lds_impl(h, M, n, ldm, batch, strideM, Q, ldq, strideQ, evals, strideE, descending, info);
}

int ffgp_gemm_batched(ffgp_handle* h, int opa, int opb, int lower_tiles, const double* A, int lda, long strideA, const double* B,
                      int ldb, long strideB, double* C, int ldc, long strideC, int m, int n, int k, double alpha, double beta,
                      int batch) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_gemm_launch(h, opa ? OP_MNMAJOR : OP_KMAJOR, opb ? OP_MNMAJOR : OP_KMAJOR, lower_tiles ? TILES_LOWER : TILES_FULL,
                          0, A, lda, B, ldb, C, ldc, m, n, k, alpha, beta, 0, ALIAS_NONE, batch, strideA, strideB, strideC);
}

int ffgp_rows_in(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, unsigned char* found) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_rows_in_impl(h, X1, n1, X2, n2, D, found);
}

int ffgp_kernel_grad(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const double* w,
                     const double* amp, double clamp_min, int kfun, double kparam, const double* dK, int ldk, double* g_w,
                     double* g_amp, double* g_kparam) {
  if (!h) return FFGP_ERR_ARG;
  if (kfun < FFGP_KFUN_SE || kfun > FFGP_KFUN_RQ) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_kernel_grad_impl(h, X1, n1, X2, n2, D, w, amp, clamp_min, kfun, kparam, dK, ldk, g_w, g_amp, g_kparam);
}

int ffgp_assemble_pair(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const ffgp_kdesc* k, int op,
                       const double* diag_add, const double* diag_vec, long diag_stride, const double* add_mat, int ld_add,
                       double add_all, double mean_jitter, double* K, int ldk, int lower_only) {
  if (!h || !k) return FFGP_ERR_ARG;
  const ffgp_ktree t = {2, FFGP_TREE_CHAIN, {op, 0, 0}, k};
  return ffgp_assemble_tree(h, X1, n1, X2, n2, D, &t, diag_add, diag_vec, diag_stride, add_mat, ld_add, add_all, mean_jitter, K, ldk,
                            lower_only);
}

int ffgp_assemble_tree(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const ffgp_ktree* t,
                       const double* diag_add, const double* diag_vec, long diag_stride, const double* add_mat, int ld_add,
                       double add_all, double mean_jitter, double* K, int ldk, int lower_only) {
  if (!h || !t) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_assemble_pair_impl(h, X1, n1, X2, n2, D, t, diag_add, diag_vec, diag_stride, add_mat, ld_add, add_all,
                                 mean_jitter, K, ldk, lower_only);
}

int ffgp_kernel_grad_pair(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const ffgp_kdesc* k, int op,
                          const double* dK, int ldk, const ffgp_kdesc_grads* g) {
  if (!h || !k || !g) return FFGP_ERR_ARG;
  const ffgp_ktree t = {2, FFGP_TREE_CHAIN, {op, 0, 0}, k};
  return ffgp_kernel_grad_tree(h, X1, n1, X2, n2, D, &t, dK, ldk, g);
}

int ffgp_kernel_grad_tree(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const ffgp_ktree* t,
                          const double* dK, int ldk, const ffgp_kdesc_grads* g) {
  if (!h || !t || !g || t->n_leaves < 2 || t->n_leaves > 4) return FFGP_ERR_ARG;
  if (n1 <= 0 || n2 <= 0) return FFGP_OK;
  if (D <= 0 || ldk < n2) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  FFGP_CHECK(ffgp_ensure_ws(h, (ffgp_grad_pair_partial_doubles(n1, n2, D, 1, t->n_leaves) + 16) * sizeof(double)));
  return ffgp_grad_pair_impl(h, X1, n1, X2, n2, D, t, dK, ldk, 1, nullptr, 0.0, h->ws, g);
}

int ffgp_kernel_input_weights_tree(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const ffgp_ktree* t,
                                   const double* dK, int ldk, double* Wt, int ldw, long leaf_stride) {
  if (!h || !t) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_pair_wt_impl(h, X1, n1, X2, n2, D, t, dK, ldk, Wt, ldw, leaf_stride);
}

/* (re)build the inverted 128x128 diagonal blocks of a factor.  The call is the caller saying "this buffer changed behind the handle's
   back": both keys are dropped first, so the rebuild starts at block 0 and the super-block inverses are rebuilt by the next sweep that
   wants them.  (The incremental "the factor only grew" route of ffgp_refresh_dinv is for the solves' own ensure_* path: a refill with
   MORE rows at a keyed address would otherwise keep the old factor's leading blocks.) */
int ffgp_trtri_diag(ffgp_handle* h, const double* L, int n, int ldl) {
  if (!h || !L) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  h->dinv_L = nullptr;
  h->sinv_L = nullptr;
  return ffgp_refresh_dinv(h, L, n, ldl);
}

// ---- RCCL, resolved at run time ------------------------------------------------------------------------------
#include <dlfcn.h>
typedef int (*ffgp_nccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
static ffgp_nccl_allreduce_fn ffgp_resolve_allreduce() {
  // resolved exactly once, whichever host thread (one per handle / GPU) gets here first: a function-local static's
  // initialiser runs under the language's own lock
  static const ffgp_nccl_allreduce_fn fn = [] {
    ffgp_nccl_allreduce_fn f = nullptr;
    void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);   // the copy already in the process, if any (same SONAME)
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (lib) f = reinterpret_cast<ffgp_nccl_allreduce_fn>(dlsym(lib, "ncclAllReduce"));
    if (!f) fprintf(stderr, "[ffgp] ffgp_allreduce_sum: cannot resolve ncclAllReduce from librccl.so.1 (%s)\n", dlerror());
    return f;
  }();
  return fn;
}

int ffgp_allreduce_sum(ffgp_handle* h, void* comm, double* buf_dev, int count) {
  if (!h || !comm || !buf_dev || count <= 0) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  ffgp_nccl_allreduce_fn fn = ffgp_resolve_allreduce();
  if (!fn) return FFGP_ERR_HIP;
  const int nccl_double = 8, nccl_sum = 0;   // ncclFloat64, ncclSum (rccl.h)
  const int rc = fn(buf_dev, buf_dev, (size_t)count, nccl_double, nccl_sum, comm, h->stream);
  if (rc != 0) {
    fprintf(stderr, "[ffgp] ncclAllReduce failed with %d\n", rc);
    return FFGP_ERR_HIP;
  }
  return FFGP_OK;
}

int ffgp_invalidate(ffgp_handle* h) {
  if (!h) return FFGP_ERR_ARG;
  h->dinv_L = nullptr;   // both stores are keyed on the factor's address: forget it, the next solve rebuilds them
  h->dinv_n = 0;
  h->sinv_L = nullptr;
  h->sinv_n = 0;
  return FFGP_OK;
}

int ffgp_potri(ffgp_handle* h, double* L, int n, int ldl) {
  if (!h || !L || n <= 0) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  const size_t ld = ffgp_round_up(n, 16);
  const size_t n1 = ffgp_round_up((n + 1) / 2, FFGP_NB);
  const size_t xd = (size_t)n * ld, td = n1 * n1 + 16;
  FFGP_CHECK(ffgp_ensure_ws(h, (xd + td) * sizeof(double)));
  double* X = h->ws;
  double* T = h->ws + xd;
  FFGP_CHECK(ffgp_trtri_impl(h, L, n, ldl, X, (int)ld, T));
  FFGP_CHECK(ffgp_lauum_impl(h, X, n, (int)ld, L, ldl));
  h->dinv_L = nullptr;  // the buffer no longer holds the factor
  h->sinv_L = nullptr;
  return FFGP_OK;
}


// ------------------------------------------------------------------------------------------------------------
// posterior
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ffgp_var_diag_kernel(const double* __restrict__ Vt, int nt, int n, int ld,
                                                            const double* __restrict__ amp, double clamp, double add,
                                                            double* __restrict__ var, int kfun, double rinv) {
  // one wave per test point: var[t] = k(x*,x*) - sum_i Vt[t][i]^2 + add
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= nt) return;
  const int lane = threadIdx.x & 63;
  double s = 0.0;
  for (int i = lane; i < n; i += 64) {
    const double v = Vt[(size_t)t * ld + i];
    s = __builtin_fma(v, v, s);
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
  if (lane == 0) var[t] = amp[0] * ffgp_kfun_val(kfun, rinv, fmax(0.0, clamp)) - s + add;
}

int ffgp_predict(ffgp_handle* h, const ffgp_problem* p, const double* Xs, int nt, int var_mode, double var_add_all,
                 double* mean_dev, double* var_dev, int ldv) {
  if (!h || !p || !Xs || nt <= 0 || !mean_dev) return FFGP_ERR_ARG;
  if (p->n <= 0 || p->D <= 0 || p->d <= 0 || !p->X_dev || !p->Y_dev || !p->w_dev || !p->amp_dev) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  const int n = p->n, D = p->D, d = p->d;
  const size_t ld = ffgp_round_up(n, 16);
  const size_t total = (size_t)(n + d + nt) * ld;
  FFGP_CHECK(ffgp_ensure_ws(h, total * sizeof(double)));
  double* W0 = h->ws;
  double* Gt = W0 + (size_t)n * ld;        // Gamma^T (d x n)
  double* Vt = Gt + (size_t)d * ld;        // V^T = K_*^T L^-T (nt x n)
  h->n_stages = 0;
  stage_mark(h, 0);
  FFGP_CHECK(ffgp_assemble_impl(h, p->X_dev, n, p->X_dev, n, D, p->w_dev, p->amp_dev, p->clamp_min, p->diag_add_dev,
                                p->diag_vec_dev, p->diag_stride, p->add_mat_dev, p->ld_add, p->add_all, p->mean_jitter,
                                W0, (int)ld, 1, p->kfun, p->kparam));
  FFGP_CHECK(ffgp_transpose(h, p->Y_dev, n, d, d, Gt, (int)ld, 1.0));
  FFGP_CHECK(ffgp_assemble_impl(h, Xs, nt, p->X_dev, n, D, p->w_dev, p->amp_dev, p->clamp_min, nullptr, nullptr, 0, nullptr, 0,
                                0.0, 0.0, Vt, (int)ld, 0, p->kfun, p->kparam));
  stage_mark(h, 1);
  FFGP_CHECK(ffgp_potrf_impl(h, W0, n, n + d + nt, (int)ld, 0));
  stage_mark(h, 2);
  // mean = V^T Gamma   ([nt, n] x [n, d])
  FFGP_CHECK(ffgp_gemm_launch(h, OP_KMAJOR, OP_KMAJOR, TILES_FULL, 0, Vt, (int)ld, Gt, (int)ld, mean_dev, d, nt, d, n, 1.0, 0.0));
  if (var_dev) {
    if (var_mode == FFGP_VAR_FULL) {
      if (ldv < nt) return FFGP_ERR_ARG;
      FFGP_CHECK(ffgp_assemble_impl(h, Xs, nt, Xs, nt, D, p->w_dev, p->amp_dev, p->clamp_min, nullptr, nullptr, 0, nullptr, 0,
                                    var_add_all, 0.0, var_dev, ldv, 0, p->kfun, p->kparam));
      FFGP_CHECK(ffgp_gemm_launch(h, OP_KMAJOR, OP_KMAJOR, TILES_FULL, 0, Vt, (int)ld, Vt, (int)ld, var_dev, ldv, nt, nt, n, -1.0,
                                  1.0));
    } else {
      hipLaunchKernelGGL(ffgp_var_diag_kernel, dim3((nt + 3) / 4), dim3(256), 0, h->stream, Vt, nt, n, (int)ld, p->amp_dev,
                         p->clamp_min, var_add_all, var_dev, p->kfun, (p->kparam != 0.0) ? 1.0 / p->kparam : 1.0);
    }
  }
  stage_mark(h, 3);
  FFGP_HIP(hipMemcpyAsync(h->h_info, h->d_info, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  FFGP_HIP(hipStreamSynchronize(h->stream));
  stage_collect(h);
  return ffgp_map_info(h->h_info[0]);
}


}  // extern "C"
