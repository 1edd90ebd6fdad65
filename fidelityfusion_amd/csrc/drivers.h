// What the host-driver translation units (handle.hip, nlml.hip, nlml_batch.hip, train_loop.hip, api.hip) need from each other.
#pragma once
#include <cmath>

#include "ffgp_internal.h"

// ---- handle.hip
void stage_mark(ffgp_handle* h, int idx);      // records stage timer idx on the handle's stream (option "timing")
void stage_collect(ffgp_handle* h);
struct RawGraph {          // the captured forward call (option "fwd_graph", ffgp_nlml_fused_async in nlml.hip)
  ffgp_problem p;
  unsigned long epoch;
  int seen;               // 1 = this signature was enqueued plainly last time (buffers are warm): capture next
  hipGraph_t graph;
  hipGraphExec_t exec;
  bool valid;
  double* stage;          // the value the graph writes
};
void ffgp_rawg_drop(RawGraph* r);      // forgets the captured call (null: nothing to do); the struct and its staging slot stay

// ---- raw parameters: elementwise links around the fused call (kernels in nlml.hip / nlml_batch.hip, the Adam kernel of train_loop.hip)
//      and inside the one-launch trainers (train.hip; ttl_body of train_tree_lds.h)
__device__ __forceinline__ double ffgp_link_val(int kind, double p, double c) {
  switch (kind) {
    case FFGP_LINK_INV_ABS_EPS: return 1.0 / (fabs(p) + c);
    case FFGP_LINK_EXP_NEG: return exp(-p) + c;
    case FFGP_LINK_INV: return 1.0 / p + c;
    case FFGP_LINK_ABS: return fabs(p);
    case FFGP_LINK_EXP_SQ: { const double e = exp(p); return e * e; }
    case FFGP_LINK_SQUARE: return p * p + c;
    default: return p;
  }
}
__device__ __forceinline__ double ffgp_link_der(int kind, double p, double c) {
  switch (kind) {
    case FFGP_LINK_INV_ABS_EPS: { const double a = fabs(p) + c; return ((p > 0.0) ? -1.0 : ((p < 0.0) ? 1.0 : 0.0)) / (a * a); }
    case FFGP_LINK_EXP_NEG: return -exp(-p);
    case FFGP_LINK_INV: return -1.0 / (p * p);
    case FFGP_LINK_ABS: return (p > 0.0) ? 1.0 : ((p < 0.0) ? -1.0 : 0.0);
    case FFGP_LINK_EXP_SQ: { const double e = exp(p); return 2.0 * e * e; }
    case FFGP_LINK_SQUARE: return 2.0 * p;
    default: return 1.0;
  }
}

// ---- torch.optim.Adam's update of ONE parameter with gradient g (no weight decay, no amsgrad), operation for operation; bc1 and
// bc2_sqrt = 1 - beta1^t and sqrt(1 - beta2^t), computed on the host (ffgp_adam_bc below).  The one copy; its callers: ffgp_adam_kernel and
// ffgp_adam_car_kernel (train_loop.hip), ffgp_tree_adam_kernel (train_tree.hip), ffgp_hogp_adam_kernel (train_hogp.hip), tr_body
// (train.hip), ttl_body (train_tree_lds.h) and acq_owner_step (acq_tile.h).
__device__ __forceinline__ void ffgp_adam_update(double* par, double* m, double* v, double g, double lr, double b1, double b2, double eps,
                                                 double bc1, double bc2_sqrt) {
  const double m1 = m[0] + (g - m[0]) * (1.0 - b1);        // exp_avg.lerp_(grad, 1 - beta1)
  const double v1 = v[0] * b2 + (1.0 - b2) * g * g;        // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
  m[0] = m1;
  v[0] = v1;
  const double denom = sqrt(v1) / bc2_sqrt + eps;
  par[0] = par[0] + (-(lr / bc1)) * (m1 / denom);          // param.addcdiv_(exp_avg, denom, value = -step_size)
}
// ... and its bias corrections at step t = step0 + k + 1, on the host with the C library's pow, as Python computes `1 - beta ** t`: the
// trajectories are compared with torch's bit for bit, so every driver forms them here.  The table: [steps][2].
static inline void ffgp_adam_bc(const ffgp_adam* opt, long step0, int k, double* bc1, double* bc2_sqrt) {
  const double t = (double)(step0 + k + 1);
  *bc1 = 1.0 - std::pow(opt->beta1, t);
  *bc2_sqrt = std::sqrt(1.0 - std::pow(opt->beta2, t));
}
static inline void ffgp_adam_bc_table(const ffgp_adam* opt, long step0, int steps, double* bc) {
  for (int k = 0; k < steps; ++k) ffgp_adam_bc(opt, step0, k, bc + 2 * k, bc + 2 * k + 1);
}
// what every K-steps-per-call trainer refuses about its own arguments (l: the members' links, of the entry's type)
static inline bool ffgp_train_args_ok(const ffgp_handle* h, const void* p, const void* l, const ffgp_adam* opt, const double* state_dev,
                                      const double* trace_dev, int F, int steps, long step0, long trace_stride) {
  return h && p && l && opt && state_dev && trace_dev && F > 0 && F <= FFGP_TRAIN_MAXF && steps > 0 && step0 >= 0 && trace_stride >= steps;
}

// ---- nlml.hip: the pieces every likelihood driver shares
// the six gradients every driver knows (g_cov_dev / g_pair: the drivers that accept them test them next to this)
static inline bool ffgp_wants_grad(const ffgp_grads* g) {
  return g && (g->g_w_dev || g->g_amp_dev || g->g_diag_add_dev || g->g_Y_dev || g->g_diag_vec_dev || g->g_kparam_dev);
}
// status epilogue of an enqueued likelihood: sticky first failure, read-back (ffgp_train_raw's loop switches either off: fold_info / defer_info_copy)
int ffgp_finish_info(ffgp_handle* h);
// Links scaffold.  eff / geff = [w (D) | amp | diag_add]: the effective parameters ffgp_link_fwd writes and the gradients with respect
// to them.  *q = *p, and with links its w / amp / diag_add point into eff; *gq = *g (when g is given), and with links the three
// parameter gradients that were asked for point into geff.  Returns whether ffgp_link_bwd has anything to carry back.
bool ffgp_links_redirect(const ffgp_problem* p, const ffgp_links* l, const ffgp_grads* g, double* eff, double* geff, ffgp_problem* q,
                         ffgp_grads* gq);
// ... and after the likelihood: the chain rule geff -> raw gradients (when chain), then the output scale.  p, g: the caller's own; g may be null
void ffgp_links_finish(ffgp_handle* h, const ffgp_problem* p, const ffgp_links* l, const ffgp_grads* g, const double* geff, bool chain,
                       double* nll_dev);
// scratch of the gradient stages, in doubles: L^-1, Sigma^-1 -> G, TRTRI scratch + the top level's L21 X11 when the inverse is split,
// A^T = (Sigma^-1 Y)^T, partial sums of the parameter gradients; V2 only: (L^-1 A)^T and B^T = (Sigma^-1 A)^T
struct ffgp_grad_scratch {
  size_t X, S, T, At, P, Ct, Bt;
};
ffgp_grad_scratch ffgp_grad_scratch_sizes(int n, int d, int D, int ll_variant, int pair_leaves);      // pair_leaves 0: one radial profile
// V1 gradient stages once X = L^-1 and S = Sigma^-1 are there: A^T = Gamma^T L^-1 (d x n), G = d/2 Sigma^-1 - 1/2 A A^T (lower, in
// place of Sigma^-1), the parameter gradients from G.  d nll / dY = A is left in At for the caller to transpose.
int ffgp_grad_v1_stages(ffgp_handle* h, const ffgp_problem* q, const ffgp_grads* gq, int D, double mean_jitter, const double* Gt,
                        const double* X, double* S, double* At, double* P, int ld);
