// What the acquisition optimisers' kernels share (acq.hip: one frozen posterior; acq_stack.hip: a stack of them; acq_tree.hip: one
// posterior on a composed kernel; acq_chain.hip: a chain of them, each fed the mean of the one below; acq_stack_tree.hip: a stack whose
// members may carry composed kernels; acq_chain_tree.hip: such a chain): a 256-thread
// workgroup owns 16 query points, K_s / V / B live in LDS as [np][16] images, and V = L^-1 K_s, B = L^-T V are v_mfma_f64_16x16x4_f64
// block chains whose A operand, L^-1, is read from global memory / L2 with one block of prefetch.  Every stage that is the same in its
// callers stands here once, as a __device__ __forceinline__ function of thread (rg = tid >> 4, j = tid & 15) on query column j: the
// member load, the squared distance, the row-group reduction, the two chain passes, the acquisition value, the owner thread's
// prologue, step and write-back, and the launch.  What differs in substance -- the K_s row loop, the gradient pass, the loop over
// members or leaves -- stays in the six files.  The host side exists once too: acq_run (acq_stack.hip) serves every entry, a single
// posterior as the stack of one member.
#pragma once
#include <type_traits>

#include "drivers.h"
#include "tree_ops.h"

#define ACQ_T 256
#define ACQ_TILE 16

// ---- the arguments
// What holds for the whole call, whatever the posterior: acq_run fills it once and every kernel's argument struct embeds it.
struct AcqLoop {
  const int* level;      // [Q] or null (stack and chain)
  const double* bc;      // [2 steps] bias corrections
  double* Xq;            // [Q, D]
  double* state;         // [2 or 3, Q, D] or null (evaluate mode); the third plane is the accumulated gradient
  double* trace;         // [max(steps, 1), Q]
  double* hist;          // [steps + 1, Q, D] or null
  double* grad;          // [Q, D] or null
  int D, Q, steps, acq, pad;
  int accumulate;        // 1: state has the third plane.  The single and tree entries always pass 0: their state has two planes
  double var_floor, kappa, xi, f_best, lr, b1, b2, eps;
};
struct AcqStackMember {
  const double* X;       // [n, D]
  const double* Linv;    // [np, np], zero above the diagonal and in the padding
  const double* alpha;   // [n]
  const double* w;       // [D]
  const double* amp;
  double clamp, rinv, var_add, mean_coef, var_coef;
  int n, np, kfun, pad;
};
struct AcqStackArgs {
  AcqStackMember m[FFGP_ACQ_MAX_MEMBERS];
  AcqLoop c;
  int F, npmax;
};

// A workgroup-uniform value kept in a vector register: the member table's fields on top of the loop's arguments are more uniform
// values than the scalar file holds, and the vector file has the room (a scalar spill would cost the kernel a private segment).
template <class T>
__device__ __forceinline__ T acq_in_vgpr(T x) {
  asm volatile("" : "+v"(x));
  return x;
}
// the loop's arguments parked so (stack and chain kernels), in two steps: the pointers before the level scan and the owner's load, the
// acquisition's and Adam's constants behind the barrier that follows them, where the step loop begins
__device__ __forceinline__ void acq_park_pointers(AcqLoop& c) {
  c.trace = acq_in_vgpr(c.trace); c.hist = acq_in_vgpr(c.hist); c.grad = acq_in_vgpr(c.grad);
  c.state = acq_in_vgpr(c.state); c.Xq = acq_in_vgpr(c.Xq); c.bc = acq_in_vgpr(c.bc);
}
__device__ __forceinline__ void acq_park_constants(AcqLoop& c) {
  c.var_floor = acq_in_vgpr(c.var_floor); c.kappa = acq_in_vgpr(c.kappa); c.xi = acq_in_vgpr(c.xi); c.f_best = acq_in_vgpr(c.f_best);
  c.lr = acq_in_vgpr(c.lr); c.b1 = acq_in_vgpr(c.b1); c.b2 = acq_in_vgpr(c.b2); c.eps = acq_in_vgpr(c.eps);
}

// ---- a posterior's data into LDS
// X (row length Df, padded to DM) and alpha: every row below np and every column below DM is written, the padding as zeros, so that a
// posterior smaller than the one loaded before it never sees that one's rows.  The caller's barrier publishes it.
template <int DM>
__device__ __forceinline__ void acq_load_rows(double* Xs, double* al, const double* X, const double* alpha, int n, int np, int Df, int tid) {
  for (int idx = tid; idx < np * DM; idx += ACQ_T) {
    const int i = idx / DM, dd = idx % DM;
    Xs[idx] = (i < n && dd < Df) ? X[(size_t)i * Df + dd] : 0.0;
  }
  for (int i = tid; i < np; i += ACQ_T) al[i] = (i < n) ? alpha[i] : 0.0;
}
// w^2 [DM] of one kernel, zero from Df on
template <int DM>
__device__ __forceinline__ void acq_load_w2(double* w2, const double* w, int Df, int tid) {
  if (tid < DM) {
    const double wv = (tid < Df) ? w[tid] : 0.0;
    w2[tid] = wv * wv;
  }
}
// the weighted squared distance of training row xr to the query point xj, one fused multiply-add per dimension in the order of dd
template <int DM>
__device__ __forceinline__ double acq_sqdist(const double* xr, const double (&xj)[DM], const double* w2) {
  double s = 0.0;
#pragma unroll
  for (int dd = 0; dd < DM; ++dd) {
    const double df = xr[dd] - xj[dd];
    s = __builtin_fma(w2[dd] * df, df, s);
  }
  return s;
}

// ---- reductions over the 16 row groups
// The sum of x over the 16 threads of column j, through a [16][16] pad in the fixed order r = 0..15: the same bits whatever the tile.
// Holds a barrier: every thread of the workgroup calls it.  The pad is free again after the caller's next barrier.
__device__ __forceinline__ double acq_rowgroup_sum(double* pad, double x, int rg, int j) {
  pad[rg * 16 + j] = x;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < 16; ++r) s += pad[r * 16 + j];
  return s;
}
// the same sum of the gradient partials part[(rg * DM + dd) * 16 + j] for dd = dim, behind the caller's barrier
template <int DM>
__device__ __forceinline__ double acq_partial_sum(const double* part, int dim, int j) {
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < 16; ++r) s += part[(r * DM + dim) * 16 + j];
  return s;
}

// ---- the block chains
// acc += sum_{kb = k0}^{k1 - 1} op(A block) * Bm block kb.  A = L^-1 in global memory: block (bi, kb) as it stands, or (TA) block (kb, bi)
// transposed.  Bm: an [np][16] LDS image.  The next block's operands are requested before this block's four MFMAs (tr_chain's pattern,
// train.hip).
template <bool TA>
__device__ __forceinline__ void acq_chain(d4_t& acc, int k0, int k1, const double* __restrict__ A, int bi, int lda, const double* Bm, int lane) {
  if (k0 >= k1) return;
  const int m = lane & 15, g = lane >> 4;
  double a[4], b[4];
  {
    const double* pa = TA ? A + (size_t)(16 * k0) * lda + 16 * bi : A + (size_t)(16 * bi) * lda + 16 * k0;
    const double* pb = Bm + k0 * 256;
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {
      const int k = kq * 4 + g;
      a[kq] = TA ? pa[k * lda + m] : pa[m * lda + k];
      b[kq] = pb[k * 16 + m];
    }
  }
  for (int kb = k0; kb < k1; ++kb) {
    double an[4], bn[4];
    const int kn = min(kb + 1, k1 - 1);      // (the last round re-reads its own block)
    const double* pa = TA ? A + (size_t)(16 * kn) * lda + 16 * bi : A + (size_t)(16 * bi) * lda + 16 * kn;
    const double* pb = Bm + kn * 256;
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {
      const int k = kq * 4 + g;
      an[kq] = TA ? pa[k * lda + m] : pa[m * lda + k];
      bn[kq] = pb[k * 16 + m];
    }
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kq], b[kq], acc, 0, 0, 0);
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {
      a[kq] = an[kq];
      b[kq] = bn[kq];
    }
  }
}
// block dealt to `wave` in round q: forwards and backwards in turn, so that the chains' lengths (bi + 1, nb - bi) even out
__device__ __forceinline__ int acq_deal(int q, int wave) { return 4 * q + ((q & 1) ? 3 - wave : wave); }

// Stages 2 and 3 on a posterior of nb row blocks whose K_s stands in img0 (published by a barrier): V = L^-1 K_s into img1, |V_j|^2
// (returned), B = L^-T V into img0, which K_s no longer needs.  Holds the barrier of the |V_j|^2 reduction, so every thread of the
// workgroup calls it; it ends without one -- B is not published until the caller's next barrier.
__device__ __forceinline__ double acq_solve_images(const double* Linv, int lda, int nb, double* img0, double* img1, double* redv, int tid) {
  const int j = tid & 15, rg = tid >> 4, wave = tid >> 6, lane = tid & 63, g = lane >> 4;
  double vvp = 0.0;
  for (int q = 0; q < 4; ++q) {
    const int bi = acq_deal(q, wave);
    if (bi >= nb) continue;
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    acq_chain<false>(acc, 0, bi + 1, Linv, bi, lda, img0, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      img1[(16 * bi + g + 4 * r) * 16 + j] = acc[r];
      vvp = __builtin_fma(acc[r], acc[r], vvp);
    }
  }
  const double vv = acq_rowgroup_sum(redv, vvp, rg, j);
  for (int q = 0; q < 4; ++q) {
    const int bi = acq_deal(q, wave);
    if (bi >= nb) continue;
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    acq_chain<true>(acc, bi, nb, Linv, bi, lda, img1, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) img0[(16 * bi + g + 4 * r) * 16 + j] = acc[r];
  }
  return vv;
}

// ---- the acquisition value av with gm = da/dmean and gv = da/dvar (FFGP_ACQ_UCB_VAR: the entries that do not offer it refuse it on
// the host)
__device__ __forceinline__ void acq_value(int acq, double mean, double var, double var_floor, double kappa, double xi, double f_best, double& av,
                                          double& gm, double& gv) {
  if (acq == FFGP_ACQ_UCB) {
    const double sd = sqrt(fmax(var, var_floor));
    av = mean + kappa * sd;
    gm = 1.0;
    gv = (var >= var_floor) ? kappa * 0.5 / sd : 0.0;      // torch's clamp_min: no gradient below the floor
  } else if (acq == FFGP_ACQ_UCB_VAR) {
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
}

// ---- the owner of (point j, dimension rg = tid >> 4 < DM) keeps that coordinate, its Adam moments and (accumulate) its gradient sum in
// registers for the whole call; the columns of a ragged last tile repeat the last point and write nothing
struct AcqOwner {
  double x, m, v, g;
  int qo;                // the point
  bool owner, live;      // rg < DM; and a coordinate of a point of the call
};
// loads the owner's values and writes the tile's points xq [16][DM] (zero from D on); the caller's barrier publishes them
template <int DM>
__device__ __forceinline__ AcqOwner acq_owner_load(const AcqLoop& c, double* xq, int tid) {
  const int j = tid & 15, rg = tid >> 4;
  AcqOwner o = {0.0, 0.0, 0.0, 0.0, (int)blockIdx.x * ACQ_TILE + j, rg < DM, false};
  o.live = o.owner && rg < c.D && o.qo < c.Q;
  if (o.owner) {
    const size_t plane = (size_t)c.Q * c.D, e = (size_t)min(o.qo, c.Q - 1) * c.D + rg;
    if (rg < c.D) {
      o.x = c.Xq[e];
      if (c.steps > 0) {
        o.m = c.state[e];
        o.v = c.state[plane + e];
        if (c.accumulate) o.g = c.state[2 * plane + e];
      }
    }
    xq[j * DM + rg] = o.x;
  }
  return o;
}
// step k of `iters`, by the owner threads alone, with gx = this coordinate's d(-a)/dx: the outputs, torch.optim.Adam's update (on the
// accumulated gradient when the caller's loop never zeroes it) and the point's new coordinate into xq.  The caller's barrier follows.
template <int DM>
__device__ __forceinline__ void acq_owner_step(const AcqLoop& c, AcqOwner& o, double* xq, int k, int iters, double av, double gx, int tid) {
  const int j = tid & 15, rg = tid >> 4;
  if (o.live) {
    const size_t e = (size_t)o.qo * c.D + rg;
    if (rg == 0) c.trace[(size_t)k * c.Q + o.qo] = av;
    if (c.hist) c.hist[(size_t)k * c.Q * c.D + e] = o.x;
    if (c.grad && k == iters - 1) c.grad[e] = gx;
  }
  if (c.steps > 0 && rg < c.D) {
    if (c.accumulate) {
      o.g += gx;
      gx = o.g;
    }
    ffgp_adam_update(&o.x, &o.m, &o.v, gx, c.lr, c.b1, c.b2, c.eps, c.bc[2 * k], c.bc[2 * k + 1]);
  }
  xq[j * DM + rg] = o.x;
}
// after the last step: the point, the optimiser's state and the last row of the history
__device__ __forceinline__ void acq_owner_store(const AcqLoop& c, const AcqOwner& o, int tid) {
  if (o.live && c.steps > 0) {
    const size_t plane = (size_t)c.Q * c.D, e = (size_t)o.qo * c.D + (tid >> 4);
    c.Xq[e] = o.x;
    c.state[e] = o.m;
    c.state[plane + e] = o.v;
    if (c.accumulate) c.state[2 * plane + e] = o.g;
    if (c.hist) c.hist[(size_t)c.steps * c.Q * c.D + e] = o.x;
  }
}

// LDS of the single and the stack kernel, in doubles, sized by the largest posterior of the call: three [np][16] images (the second at
// least 256 DM: it also carries the gradient partials), X [np][DM], alpha [np], the tile's points [16][DM], w^2 [DM], two [16][16]
// reduction pads
static constexpr size_t acq_lds_doubles(int np, int DM) {
  const size_t img = (size_t)np * 16, img1 = img > (size_t)256 * DM ? img : (size_t)256 * DM;
  return 2 * img + img1 + (size_t)np * DM + np + 16 * DM + DM + 512;
}
static_assert(acq_lds_doubles(FFGP_ACQ_MAX_N, FFGP_ACQ_MAX_D) * sizeof(double) <= 160 * 1024, "the acquisition kernels' LDS exceeds a CU's 160 KiB");

// ---- the host side
// One launch: `kernel` is an instantiation for DM, lds_doubles(np, DM) its LDS.  The attribute is set on every call: it belongs to the
// current device, and a host-side "already set" table would be shared state between the threads of different handles (a host-side
// call, nothing is enqueued).
template <int DM, class Args>
static int acq_launch(ffgp_handle* h, void (*kernel)(Args), size_t (*lds_doubles)(int, int), int np, const Args& a, int grid) {
  const size_t lds = lds_doubles(FFGP_ACQ_MAX_N, DM) * sizeof(double);
  FFGP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(ACQ_T), lds_doubles(np, DM) * sizeof(double), h->stream, a);
  if (hipGetLastError() != hipSuccess) return FFGP_ERR_HIP;
  return FFGP_OK;
}
// the template class of an input dimension d: f(std::integral_constant<int, DM>) with DM = 2, 8 or 16
template <class F>
static int acq_by_dm(int d, F f) {
  if (d <= 2) return f(std::integral_constant<int, 2>());
  if (d <= 8) return f(std::integral_constant<int, 8>());
  return f(std::integral_constant<int, 16>());
}

// One leaf of a composed kernel as the tree kernels read it (acq_tree.hip: four by value in the kernel's arguments), and a member's
// kernel as a record of leaves in device memory (ffgp_acq_optimize_stack_tree), one record per member.  A member with one radial library kernel is the one-leaf record nl = 1 of its own w / amp / clamp /
// kfun / kparam.  Eight members of four leaves by value would be more uniform state than the scalar file holds (see acq_park_*), so
// acq_run uploads the records into handle workspace behind the bias corrections and the kernel copies member f's into LDS.
struct AcqLeaf {
  const double* w;       // [D]
  const double* amp;
  const double* center;  // [D] or null (the origin); linear leaves only
  double clamp, rinv;
  int kfun, pad;
};
struct AcqMemberTree {
  AcqLeaf k[FFGP_TREE_LEAVES];
  int nl, shape, op[3], pad[3];
};
// what the entries that take an ffgp_ktree from the caller refuse about it (the tree itself is not null)
static inline bool acq_tree_ok(const ffgp_ktree* t) {
  if (!ffgp_tree_form_ok(t)) return false;
  for (int e = 0; e < t->n_leaves; ++e)
    if (t->leaf[e].kfun < FFGP_KFUN_SE || t->leaf[e].kfun > FFGP_KFUN_LINEAR || !t->leaf[e].w_dev || !t->leaf[e].amp_dev) return false;
  return true;
}
// member p's kernel as a leaf record (acq_stack.hip): its tree, checked by the entry, or the one leaf of its own radial kernel
AcqMemberTree acq_member_tree(const ffgp_acq_member& p, const ffgp_ktree* t);
// what acq_run hands to `launch` beside the kernel's arguments
struct AcqTrees {
  const ffgp_ktree* const* host;      // [F] the members' trees as the caller gave them (null entry: a radial member), or null
  const AcqMemberTree* table_dev;     // [F] in handle workspace, or null when the entry did not ask for it
};

// One driver (acq_run, acq_stack.hip) for every entry.
// Checks the call, forms every member's L^-1 and the bias-correction table in handle workspace, launches through `launch` and waits.
// `trees` (ffgp_acq_optimize_tree, ffgp_acq_optimize_stack_tree and ffgp_acq_optimize_chain_tree, which check the trees themselves): host array [F]; member f's kernel
// is the composition trees[f], so the member carries no w_dev / amp_dev / kfun of its own and those three checks are skipped; a null
// entry is a member with its own radial kernel.  It is handed on to `launch`.  `leaf_table`: the members' AcqMemberTree records are
// uploaded behind the bias corrections and handed on as well.
// `chain` (ffgp_acq_optimize_chain and ffgp_acq_optimize_chain_tree): the per-member dimension rule is members[0].D = D <=
// FFGP_ACQ_MAX_D - 1 and D + 1 above it, instead of one D for all; AcqLoop.D stays the D of the query points.  The three compose
// (ffgp_acq_optimize_chain_tree passes all of them): the dimension rule applies to a member with a tree as to any other, the radial
// checks are skipped for it, and a leaf record holds pointers only -- the row length D_f of w and centre is the kernel's to apply.
typedef int (*acq_launch_fn)(ffgp_handle* h, const AcqStackArgs& a, int grid, const AcqTrees& t);
int acq_run(ffgp_handle* h, const ffgp_acq_stack* s, acq_launch_fn launch, double* Xq_dev, int Q, int steps, const ffgp_adam* opt, double* state_dev,
            long step0, double* trace_dev, double* hist_dev, double* grad_dev, const ffgp_ktree* const* trees = nullptr, bool chain = false,
            bool leaf_table = false);
