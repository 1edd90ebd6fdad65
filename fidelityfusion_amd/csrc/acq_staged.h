// What the two launch-per-stage acquisition entries share (acq_staged.hip: members with one radial kernel; acq_staged_tree.hip: members
// that may carry composed kernels): the tile shape, the argument structs, the chunk and level rules, and ONE host driver
// (acq_staged_run, acq_staged.hip) -- the argument checks, the workspace carve-up, the zero-fill, the per-member ffgp_invalidate +
// ffgp_trtri_impl prologue, the bias-correction table, the step loop with its two GEMMs per member, the column-sum kernel and the owner
// kernel.  What an entry brings is its three stage launches: K_s, the value and the gradient tiles.
#pragma once
#include "acq_tile.h"

#define AS_T 256
#define AS_COLS 64
#define AS_LANES 4
#define AS_ROWS 128

struct AcqStagedMember {
  const double *X, *alpha, *w, *amp;      // w, amp: the member's own radial kernel (null for a member on a tree)
  double *Ks, *DK, *V, *B;                // [n][Qp] each; DK (the derivative factors) exists on the radial entry only
  double clamp, rinv, var_add, mean_coef, var_coef;
  int n, kfun;
};
struct AcqStagedArgs {
  AcqStagedMember m[FFGP_ACQ_MAX_MEMBERS];
  const int* level;      // [Q] or null
  double *Xq, *state, *trace, *hist, *grad;
  double *pm, *pv;       // [F][nch][Qp] chunk sums of K_s^T alpha and |V|^2
  double *av, *gm, *gv;  // [Qp] the acquisition value, da/dmean, da/dvar
  double* part;          // [F][nch][Qp][DM] chunk sums of d(-a)/dx
  const AcqMemberTree* tab;      // [F] the members' leaf records in handle workspace (the tree entry), or null
  double* self;          // [Q][D] sum_f c'_f dk_f(x, x)/dx (the tree entry), or null: a radial kernel's k(x, x) does not depend on x
  int F, D, DM, Q, Qp, nch, steps, acq, accumulate;
  double var_floor, kappa, xi, f_best, lr, b1, b2, eps;
};

__device__ __forceinline__ int as_chunks(int n) { return (n + AS_ROWS - 1) / AS_ROWS; }
// this point's weights of member f: an exact 0 / 1 factor on its two coefficients (acq_stack.hip, Levels)
__device__ __forceinline__ int as_level(const AcqStagedArgs& a, int q) { return a.level ? min(a.level[q], a.F - 1) : a.F - 1; }

// one stage of the step loop: a refused launch ends the call there, before a later stage reads what it did not write
#define AS_STAGE(call) \
  if ((rc = (call)) != FFGP_OK) break
static inline int as_launched() { return hipGetLastError() == hipSuccess ? FFGP_OK : FFGP_ERR_HIP; }

// an entry's own stages; `images` [n][Qp] matrices per member (K_s, V, B and, on the radial entry, the derivative factors)
struct AcqStagedStages {
  int images;
  int (*ks)(ffgp_handle* h, const AcqStagedArgs& a, dim3 tiles);
  int (*value)(ffgp_handle* h, const AcqStagedArgs& a);
  int (*grad)(ffgp_handle* h, const AcqStagedArgs& a, dim3 tiles);
};
// `trees` (the tree entry, which checks the trees itself): host array [F] as acq_run takes it -- member f's kernel is trees[f], a null
// entry is a member with its own radial kernel -- and the members' leaf records are uploaded behind the rest of the workspace.
int acq_staged_run(ffgp_handle* h, const ffgp_acq_stack* s, const ffgp_ktree* const* trees, const AcqStagedStages& st, double* Xq_dev, int Q,
                   int steps, const ffgp_adam* opt, double* state_dev, long step0, double* trace_dev, double* hist_dev, double* grad_dev);
