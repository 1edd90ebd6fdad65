// What the launch-per-stage acquisition entries share (acq_staged.hip: stacks of members with one radial kernel; acq_staged_tree.hip:
// stacks whose members may carry composed kernels; acq_staged_chain.hip: the NAR chain; acq_staged_chain_tree.hip: the NAR chain whose
// members may carry composed kernels): the tile shape, the argument structs, the chunk
// and level rules, ONE host prologue (acq_staged_prepare, acq_staged.hip) -- the argument checks, the workspace carve-up, the zero-fill,
// the per-member ffgp_invalidate + ffgp_trtri_impl, the bias-correction table --, the two GEMMs per member, the column-sum kernel and the
// owner kernel.  The two stack entries also share their step loop (acq_staged_run) and bring its three stage launches: K_s, the value
// and the gradient tiles.  The chain's members run in sequence, so it has a step loop of its own on the same prologue and stages.
#pragma once
#include <vector>

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

// ---- device helpers of the chain loops (acq_staged_chain.hip, acq_staged_chain_tree.hip)
// the chunk sums p[f][0 .. chunks(n_f) - 1][q] added in chunk order: a member's mean (p = pm) or |V|^2 (p = pv)
__device__ __forceinline__ double asc_chunk_sum(const double* p, const AcqStagedArgs& a, int f, int q) {
  const int nch = as_chunks(a.m[f].n);
  double s = 0.0;
  for (int ch = 0; ch < nch; ++ch) s += p[((size_t)f * a.nch + ch) * a.Qp + q];
  return s;
}
// member f's rows r0 .. r0 + rows - 1 into LDS, row length Df padded to DM with zeros
template <int DM>
__device__ __forceinline__ void asc_load_rows(double* Xs, const double* X, int r0, int rows, int Df, int tid) {
  for (int idx = tid; idx < rows * DM; idx += AS_T) {
    const int i = idx / DM, dd = idx % DM;
    Xs[idx] = (dd < Df) ? X[(size_t)(r0 + i) * Df + dd] : 0.0;
  }
}
// z_f = [x_q, u_q] of a live column, zeros beyond; u_q = m_{f-1}(x_q), and for f = 0 the coordinate D stays 0 under w^2 = 0
template <int DM>
__device__ __forceinline__ void asc_load_z(double (&xj)[DM], const AcqStagedArgs& a, int f, int q, bool live) {
  const int D = a.D;
  const double u = (live && f > 0) ? asc_chunk_sum(a.pm, a, f - 1, q) : 0.0;
#pragma unroll
  for (int dd = 0; dd < DM; ++dd) xj[dd] = (live && dd < D) ? a.Xq[(size_t)q * D + dd] : (dd == D ? u : 0.0);
}

// ---- device helpers of the loops for composed kernels (acq_staged_tree.hip, acq_staged_chain_tree.hip)
#define AST_NL FFGP_TREE_LEAVES

// the tree that tree_ops.h evaluates: a one-leaf record as the sum of its leaf and 0.0 (exact)
struct AstTree {
  int nl, shape, op[3];
};
__device__ __forceinline__ AstTree ast_tree(const AcqMemberTree& mt) {
  AstTree tr;
  tr.nl = max(mt.nl, 2); tr.shape = mt.shape; tr.op[0] = mt.op[0]; tr.op[1] = mt.op[1]; tr.op[2] = mt.op[2];
  return tr;
}

// An offset of zero the compiler cannot see through.  The leaf record in LDS is workgroup-uniform and loop-invariant, and hoisting its
// 2 x 4 x DM doubles out of the row loop into registers is what the compiler does when it can: at DM = 16 that is 256 registers beside
// x_q and the running sums, and a private segment.  Each use of a leaf's w^2 and centre goes through its own opaque offset, so the
// values are read from LDS (a broadcast read) where they are used and live no longer than one leaf's term.
__device__ __forceinline__ int ast_opaque0() {
  int o = 0;
  asm volatile("" : "+v"(o));
  return o;
}

// member's leaf record into LDS: per leaf w^2 [DM] and centre [DM] (zero from D on, zero past nl, the centre zero unless linear and
// given) and lp = (amp, clamp, 1 / kparam, 0.0: padding); all four leaf slots are written.  The caller's barrier publishes it.
template <int DM>
__device__ __forceinline__ void ast_load_record(const AcqMemberTree& mt, int D, int tid, double* w2, double* cen, double* lp) {
  const int nl = mt.nl;
#pragma unroll
  for (int e = 0; e < AST_NL; ++e) {
    const bool live = e < nl;
    const bool lin = live && mt.k[e].kfun == FFGP_KFUN_LINEAR;
    if (tid < DM) {
      const double wv = (live && tid < D) ? mt.k[e].w[tid] : 0.0;
      w2[e * DM + tid] = wv * wv;
      cen[e * DM + tid] = (lin && tid < D && mt.k[e].center) ? mt.k[e].center[tid] : 0.0;
    }
    if (tid == 0) {
      lp[4 * e] = live ? mt.k[e].amp[0] : 0.0;
      lp[4 * e + 1] = live ? mt.k[e].clamp : 0.0;
      lp[4 * e + 2] = live ? mt.k[e].rinv : 1.0;
      lp[4 * e + 3] = 0.0;
    }
  }
}

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

// What acq_staged_prepare leaves for a step loop: the kernels' arguments, each member's L^-1 in handle workspace, the Adam bias
// corrections per step, and the host copy of the leaf records, which has to outlive the upload (acq_staged_finish waits).
struct AcqStagedPlan {
  AcqStagedArgs a;
  const double* Linv[FFGP_ACQ_MAX_MEMBERS];
  int np_of[FFGP_ACQ_MAX_MEMBERS];
  std::vector<double> bc;      // [2 iters]
  std::vector<AcqMemberTree> table;
  double* extra;               // the entry's own `extra_doubles` behind everything else, or null
  int iters, qt;               // max(steps, 1); Qp / AS_COLS
};
// The prologue of every staged loop: the argument checks (`chain`: the dimension rule is ffgp_acq_optimize_chain's -- members[0].D = D <=
// FFGP_ACQ_MAX_D - 1 and D + 1 above it, the kernels' DM then holds D + 1 -- instead of one D for all), the workspace carve-up with
// `images` [n][Qp] matrices per member, the zero-fill of L^-1 and the images, ffgp_invalidate + ffgp_trtri_impl per member, the
// bias-correction table, the upload of the leaf records (`trees` non-null) and the filling of AcqStagedArgs.  FFGP_ERR_ARG is returned
// before anything is enqueued.
int acq_staged_prepare(ffgp_handle* h, const ffgp_acq_stack* s, const ffgp_ktree* const* trees, int images, bool chain, size_t extra_doubles,
                       double* Xq_dev, int Q, int steps, const ffgp_adam* opt, double* state_dev, long step0, double* trace_dev, double* hist_dev,
                       double* grad_dev, AcqStagedPlan& pl);
// the stages that are the same in every loop: V_f = L_f^-1 K_s,f and B_f = L_f^-T V_f (two clipped GEMMs), the column sums of members
// f0 .. f0 + tiles.z - 1, step k's owner launch; and the wait that ends the call, which returns `rc` if that is a failure
int as_solve_stage(ffgp_handle* h, const AcqStagedPlan& pl, int f);
int as_col_stage(ffgp_handle* h, const AcqStagedArgs& a, dim3 tiles, int f0);
int as_owner_stage(ffgp_handle* h, const AcqStagedPlan& pl, int k);
int acq_staged_finish(ffgp_handle* h, int rc);
// the chain loops' census of level_dev, once per call behind the prologue (acq_staged_chain.hip, where its kernel stands): `tops`, the
// bit set of the members at which some point stops (level_dev null: {F - 1}, nothing is read back), `top`, the highest of them, and the
// zero-fill of `part` above `top`.  The census word is the first of the entry's extra doubles.
int acq_staged_chain_census(ffgp_handle* h, const AcqStagedPlan& pl, unsigned& tops, int& top);

// The step loop of the two stack entries: one launch per stage over all members (blockIdx.z is the member).
// `trees` (the tree entry, which checks the trees itself): host array [F] as acq_run takes it -- member f's kernel is trees[f], a null
// entry is a member with its own radial kernel -- and the members' leaf records are uploaded behind the rest of the workspace.
int acq_staged_run(ffgp_handle* h, const ffgp_acq_stack* s, const ffgp_ktree* const* trees, const AcqStagedStages& st, double* Xq_dev, int Q,
                   int steps, const ffgp_adam* opt, double* state_dev, long step0, double* trace_dev, double* hist_dev, double* grad_dev);
