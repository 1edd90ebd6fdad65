// What the launch-per-stage composed-kernel trainers share: train_tree.hip (ffgp_train_tree_raw: the loop, raw -> effective, Adam for
// plain members) and train_tree_res.hip (ffgp_train_tree_res_raw: the same loop with RESIDUAL members -- their targets formed before
// the likelihood, dloss/drho reduced and rho updated in the Adam launch).  One member table, one copy of the links' chain rule.
#pragma once
#include "drivers.h"

#define FFGP_TREE_MAXL 4
// one member, as the kernels read it from device memory (F <= 16 of them: too large for a kernel argument)
struct ffgp_tree_member {
  double* w[FFGP_TREE_MAXL];       // raw parameter storages, leaf by leaf
  double* amp[FFGP_TREE_MAXL];
  double* cen[FFGP_TREE_MAXL];     // a trained centre (linear leaf), else null
  double* dadd;
  double w_c[FFGP_TREE_MAXL], amp_c[FFGP_TREE_MAXL];
  double dadd_c, sc;
  long eff, geff;                  // where this member's effective parameters / their gradients start in the scratch (doubles)
  int w_link[FFGP_TREE_MAXL], amp_link[FFGP_TREE_MAXL], nw[FFGP_TREE_MAXL];
  int dadd_link, D, nl, P;
};
// effective parameters of a member: leaf e at e (D + 1) as [w (D) | amp], then diag_add at nl (D + 1);
// their gradients: leaf e at e (2 D + 1) as [g_w (D) | g_amp | g_center (D)], then g_diag_add at nl (2 D + 1)

// raw parameter i (< P, canonical order) of member M: its storage in *par, and the loss's gradient with respect to it -- the links'
// chain rule (ffgp_link_bwd's arithmetic; a broadcast length scale: the D effective gradients summed in index order first)
__device__ __forceinline__ double ffgp_tree_raw_grad(const ffgp_tree_member* M, const double* __restrict__ scratch, int i, double** par_out) {
  const int P = M->P;
  const int D = M->D, gper = 2 * D + 1;
  const double sc = M->sc;
  const double* ge = scratch + M->geff;
  double* par;
  double g;
  if (i == P - 1) {
    par = M->dadd;
    g = sc * ge[M->nl * gper] * ffgp_link_der(M->dadd_link, par[0], M->dadd_c);
  } else {
    int e = 0, k = i;
    for (; e < M->nl - 1; ++e) {
      const int cnt = M->nw[e] + 1 + (M->cen[e] ? D : 0);
      if (k < cnt) break;
      k -= cnt;
    }
    const double* gl = ge + e * gper;
    const int nw = M->nw[e];
    if (k < nw) {
      par = M->w[e] + k;
      if (nw == D) {
        g = sc * gl[k] * ffgp_link_der(M->w_link[e], par[0], M->w_c[e]);
      } else {
        double sg = 0.0;
        for (int q = 0; q < D; ++q) sg += gl[q];
        g = sc * sg * ffgp_link_der(M->w_link[e], par[0], M->w_c[e]);
      }
    } else if (k == nw) {
      par = M->amp[e];
      g = sc * gl[D] * ffgp_link_der(M->amp_link[e], par[0], M->amp_c[e]);
    } else {
      par = M->cen[e] + (k - nw - 1);
      g = sc * gl[D + 1 + (k - nw - 1)];      // (identity link)
    }
  }
  *par_out = par;
  return g;
}

// the residual members of a call, by value to the two kernels of train_tree_res.hip (rho[f] null: a plain member)
struct ffgp_tree_resid {
  double* rho[FFGP_TRAIN_MAXF];
  const double* yl[FFGP_TRAIN_MAXF];
  const double* yh[FFGP_TRAIN_MAXF];
  const double* vl[FFGP_TRAIN_MAXF];     // null: the subset form
  const double* vh[FFGP_TRAIN_MAXF];
  long vls[FFGP_TRAIN_MAXF], vhs[FFGP_TRAIN_MAXF];
  double* r[FFGP_TRAIN_MAXF];            // [n, d] targets                 } in the handle's scratch, behind the members'
  double* dv[FFGP_TRAIN_MAXF];           // [n] |s|                        } effective parameters and gradients
  double* gY[FFGP_TRAIN_MAXF];           // [n, d] dloss/dr (A for V1, B for V2)
  double* gdv[FFGP_TRAIN_MAXF];          // [n] dloss/ddvec = G_ii
  double* rho_last[FFGP_TRAIN_MAXF];
  long nd[FFGP_TRAIN_MAXF];
  int n[FFGP_TRAIN_MAXF];
};
// the two launches a call with residual members adds per step (train_tree_res.hip holds the kernels): the targets before the
// likelihoods (rmax: the largest max(n d, n) of the residual members), and the Adam step in ffgp_tree_adam_kernel's place
void ffgp_tree_resid_form_launch(hipStream_t s, int F, const ffgp_tree_resid& rs, long rmax);
void ffgp_tree_res_adam_launch(hipStream_t s, int F, int pmax, const ffgp_tree_resid& rs, const ffgp_tree_member* tab, const double* scratch,
                               double* state, long state_stride, const ffgp_adam* opt, double bc1, double bc2_sqrt, const double* loss,
                               double* trace, long trace_stride, int step, int* info);
// ffgp_train_tree_raw's body (train_tree.hip); r null, or r[f].rho_dev null: a plain member
int ffgp_train_tree_impl(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_tree_links* l, const ffgp_residual* r, int steps,
                         const ffgp_adam* opt, double* state_dev, long state_stride, long step0, double* trace_dev, long trace_stride);
