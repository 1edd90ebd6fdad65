// The acquisition optimiser's Adam loop past the one-launch kernels' LDS-tile limit: launch per stage, every step enqueued by ONE
// library call (ffgp_acq_optimize_stack_staged, include/ffgp.h).  Reference: Bayesian_optimization/acq.py:48-68 and
// MF_BayesianOptimization/Discrete/DMF_acq.py:226-262 on models of a few hundred to a few thousand points (the multi-fidelity demo
// trains on 300 / 300 / 250).  The mathematics, the argument structs and the output layouts are ffgp_acq_optimize_stack's
// (acq_stack.hip); what differs is where the images live: K_s, V and B of EVERY query point stand in handle workspace as [n][Qp]
// matrices, so n is bounded by workspace and not by a CU's LDS.
//
// Per call: L_f^-1 of every member (ffgp_trtri_impl, the handle's inverted diagonal blocks rebuilt before each, as acq_run does).
// Per step, 5 + 2 F launches whatever Q and n:
//   1. ffgp_acq_staged_ks_kernel     K_s,f = k_f(X_f, Xq) and the derivative factors amp (-2 phi'), all members in one launch
//   2. ffgp_gemm_launch x 2 F        V_f = L_f^-1 K_s,f and B_f = L_f^-T V_f on the fp64 MFMA GEMM, k clipped to the triangle
//   3. ffgp_acq_staged_col_kernel    partial sums of mean_f = K_s,f^T alpha_f and |V_f|^2 over chunks of 128 rows
//   4. ffgp_acq_staged_value_kernel  the chunks summed in order, the level-masked mean and variance, acq_value (acq_tile.h)
//   5. ffgp_acq_staged_grad_kernel   d(-a)/dx_q = sum_f w_f^2 o sum_i (da/dmean c_f alpha_i - 2 da/dvar c'_f B_iq) amp (-2 phi') (x_q - X_i)
//                                    as partial sums per (member, chunk of 128 rows)
//   6. ffgp_acq_staged_owner_kernel  the partials summed in order (member, chunk), the outputs, ffgp_adam_update (drivers.h)
// A tile of the three tile kernels is 64 query columns x 128 training rows on 256 threads: thread (lane = tid >> 6, c = tid & 63)
// walks rows lane, lane + 4, ... of the chunk for column c, a wave reads and writes 64 consecutive doubles of a matrix row, and the
// four lanes' sums are added through LDS in the order 0..3.  The chunking is a function of n alone, no sum is taken in an order that
// depends on Q, on the grid or on timing, and there are no atomics: what can differ between two ways of cutting Q is the GEMM's
// tile choice alone.
// The step loop (acq_staged_run, acq_staged.h), the column-sum kernel and the owner kernel also serve the entry for composed kernels
// (acq_staged_tree.hip), which brings its own stages 1, 4 and 5.  The host prologue (acq_staged_prepare), the GEMM stage, the column-sum
// kernel and the owner kernel serve the chain's loop too (acq_staged_chain.hip), which runs its members in sequence.
#include <climits>
#include <cmath>
#include <vector>

#include "acq_staged.h"

// ---- 1. K_s and the derivative factors; the columns Q..Qp-1 are written as zeros
template <int DM>
__global__ __launch_bounds__(AS_T) void ffgp_acq_staged_ks_kernel(AcqStagedArgs a) {
  __shared__ double Xs[AS_ROWS * DM];
  __shared__ double w2[DM];
  const AcqStagedMember& mb = a.m[blockIdx.z];
  const int n = mb.n, r0 = blockIdx.y * AS_ROWS;
  if (r0 >= n) return;
  const int rows = min(AS_ROWS, n - r0), tid = threadIdx.x, D = a.D;
  for (int idx = tid; idx < rows * DM; idx += AS_T) {
    const int i = idx / DM, dd = idx % DM;
    Xs[idx] = (dd < D) ? mb.X[(size_t)(r0 + i) * D + dd] : 0.0;
  }
  acq_load_w2<DM>(w2, mb.w, D, tid);
  __syncthreads();
  const int q = blockIdx.x * AS_COLS + (tid & 63), lane = tid >> 6;
  const bool live = q < a.Q;
  double xj[DM];
#pragma unroll
  for (int dd = 0; dd < DM; ++dd) xj[dd] = (live && dd < D) ? a.Xq[(size_t)q * D + dd] : 0.0;
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

// ---- 3. chunk sums of K_s^T alpha and |V|^2, per column, of member f0 + blockIdx.z (the stack loops: every member in one launch; the
// chain loop: one member per launch)
__global__ __launch_bounds__(AS_T) void ffgp_acq_staged_col_kernel(AcqStagedArgs a, int f0) {
  __shared__ double red[2][AS_LANES][AS_COLS];
  const int f = f0 + blockIdx.z;
  const AcqStagedMember& mb = a.m[f];
  const int n = mb.n, r0 = blockIdx.y * AS_ROWS;
  if (r0 >= n) return;
  const int rows = min(AS_ROWS, n - r0), tid = threadIdx.x, c = tid & 63, lane = tid >> 6;
  const int q = blockIdx.x * AS_COLS + c;
  double sm = 0.0, sv = 0.0;
  for (int i = lane; i < rows; i += AS_LANES) {
    const size_t e = (size_t)(r0 + i) * a.Qp + q;
    const double v = mb.V[e];
    sm = __builtin_fma(mb.Ks[e], mb.alpha[r0 + i], sm);
    sv = __builtin_fma(v, v, sv);
  }
  red[0][lane][c] = sm;
  red[1][lane][c] = sv;
  __syncthreads();
  if (tid < 2 * AS_COLS) {
    const int which = tid >> 6;
    double s = 0.0;
#pragma unroll
    for (int l = 0; l < AS_LANES; ++l) s += red[which][l][c];
    (which ? a.pv : a.pm)[((size_t)f * a.nch + blockIdx.y) * a.Qp + q] = s;
  }
}

// ---- 4. mean, variance, the acquisition value and its two derivatives, per point
__global__ __launch_bounds__(AS_T) void ffgp_acq_staged_value_kernel(AcqStagedArgs a) {
  const int q = blockIdx.x * AS_T + threadIdx.x;
  if (q >= a.Q) return;
  const int lev = as_level(a, q);
  double mean = 0.0, var = 0.0;
  for (int f = 0; f < a.F; ++f) {
    const AcqStagedMember& mb = a.m[f];
    const int nch = as_chunks(mb.n);
    double mf = 0.0, vv = 0.0;
    for (int ch = 0; ch < nch; ++ch) {
      const size_t e = ((size_t)f * a.nch + ch) * a.Qp + q;
      mf += a.pm[e];
      vv += a.pv[e];
    }
    const bool on = f <= lev;
    const double cm = on ? mb.mean_coef : 0.0, cv = on ? mb.var_coef : 0.0;
    mean = __builtin_fma(cm, mf, mean);
    var = __builtin_fma(cv, mb.amp[0] - vv + mb.var_add, var);      // phi(0) = 1 for every radial profile
  }
  double av, gm, gv;
  acq_value(a.acq, mean, var, a.var_floor, a.kappa, a.xi, a.f_best, av, gm, gv);
  a.av[q] = av;
  a.gm[q] = gm;
  a.gv[q] = gv;
}

// ---- 5. the input gradient's chunk sums.  c_iq = -(da/dmean c_f alpha_i - 2 da/dvar c'_f B_iq) is the upstream on k_i, and
// dk_i/dx_q = -amp (-2 phi') w^2 o (x_q - X_i): the two signs cancel, w^2 is applied to the chunk's sum.
template <int DM>
__global__ __launch_bounds__(AS_T) void ffgp_acq_staged_grad_kernel(AcqStagedArgs a) {
  __shared__ double Xs[AS_ROWS * DM];
  __shared__ double al[AS_ROWS];
  __shared__ double w2[DM];
  __shared__ double red[AS_LANES][AS_COLS * DM];
  const AcqStagedMember& mb = a.m[blockIdx.z];
  const int n = mb.n, r0 = blockIdx.y * AS_ROWS;
  if (r0 >= n) return;
  const int rows = min(AS_ROWS, n - r0), tid = threadIdx.x, D = a.D, f = blockIdx.z;
  for (int idx = tid; idx < rows * DM; idx += AS_T) {
    const int i = idx / DM, dd = idx % DM;
    Xs[idx] = (dd < D) ? mb.X[(size_t)(r0 + i) * D + dd] : 0.0;
  }
  for (int i = tid; i < rows; i += AS_T) al[i] = mb.alpha[r0 + i];
  acq_load_w2<DM>(w2, mb.w, D, tid);
  __syncthreads();
  const int c = tid & 63, lane = tid >> 6, q0 = blockIdx.x * AS_COLS, q = q0 + c;
  const bool live = q < a.Q;
  double xj[DM], G[DM];
#pragma unroll
  for (int dd = 0; dd < DM; ++dd) {
    xj[dd] = (live && dd < D) ? a.Xq[(size_t)q * D + dd] : 0.0;
    G[dd] = 0.0;
  }
  double cA = 0.0, cB = 0.0;
  if (live) {
    const bool on = f <= as_level(a, q);
    cA = a.gm[q] * (on ? mb.mean_coef : 0.0);
    cB = -2.0 * a.gv[q] * (on ? mb.var_coef : 0.0);
  }
  for (int i = lane; i < rows; i += AS_LANES) {
    const size_t e = (size_t)(r0 + i) * a.Qp + q;
    const double u = (cA * al[i] + cB * mb.B[e]) * mb.DK[e];
#pragma unroll
    for (int dd = 0; dd < DM; ++dd) G[dd] = __builtin_fma(u, xj[dd] - Xs[i * DM + dd], G[dd]);
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

// ---- 6. step k by the owner of (point, dimension): the outputs as acq_owner_step / acq_owner_store (acq_tile.h) write them, and
// torch.optim.Adam's update on the gradient or, when the caller's loop never zeroes it, on the running sum kept in state's third plane
__global__ __launch_bounds__(AS_T) void ffgp_acq_staged_owner_kernel(AcqStagedArgs a, int k, int last, double bc1, double bc2_sqrt) {
  const size_t plane = (size_t)a.Q * a.D, e = (size_t)blockIdx.x * AS_T + threadIdx.x;
  if (e >= plane) return;
  const int q = (int)(e / a.D), dd = (int)(e % a.D);
  double gx = 0.0;
  for (int f = 0; f < a.F; ++f) {
    const int nch = as_chunks(a.m[f].n);
    for (int ch = 0; ch < nch; ++ch) gx += a.part[(((size_t)f * a.nch + ch) * a.Qp + q) * a.DM + dd];
  }
  if (a.self) gx -= a.gv[q] * a.self[e];      // the tree entry: -(da/dvar) sum_f c'_f dk_f(x, x)/dx, non-zero through linear leaves
  double x = a.Xq[e];
  if (dd == 0) a.trace[(size_t)k * a.Q + q] = a.av[q];
  if (a.hist) a.hist[(size_t)k * plane + e] = x;
  if (a.grad && last) a.grad[e] = gx;
  if (a.steps > 0) {
    double m = a.state[e], v = a.state[plane + e];
    if (a.accumulate) {
      gx += a.state[2 * plane + e];
      a.state[2 * plane + e] = gx;
    }
    ffgp_adam_update(&x, &m, &v, gx, a.lr, a.b1, a.b2, a.eps, bc1, bc2_sqrt);
    a.Xq[e] = x;
    a.state[e] = m;
    a.state[plane + e] = v;
    if (a.hist && last) a.hist[(size_t)a.steps * plane + e] = x;
  }
}

template <int DM>
static int as_ks_launch(ffgp_handle* h, const AcqStagedArgs& a, dim3 grid) {
  hipLaunchKernelGGL(ffgp_acq_staged_ks_kernel<DM>, grid, dim3(AS_T), 0, h->stream, a);
  return as_launched();
}
template <int DM>
static int as_grad_launch(ffgp_handle* h, const AcqStagedArgs& a, dim3 grid) {
  hipLaunchKernelGGL(ffgp_acq_staged_grad_kernel<DM>, grid, dim3(AS_T), 0, h->stream, a);
  return as_launched();
}
static int as_ks_stage(ffgp_handle* h, const AcqStagedArgs& a, dim3 tiles) {
  return acq_by_dm(a.D, [&](auto dm) { return as_ks_launch<dm()>(h, a, tiles); });
}
static int as_value_stage(ffgp_handle* h, const AcqStagedArgs& a) {
  hipLaunchKernelGGL(ffgp_acq_staged_value_kernel, dim3((a.Q + AS_T - 1) / AS_T), dim3(AS_T), 0, h->stream, a);
  return as_launched();
}
static int as_grad_stage(ffgp_handle* h, const AcqStagedArgs& a, dim3 tiles) {
  return acq_by_dm(a.D, [&](auto dm) { return as_grad_launch<dm()>(h, a, tiles); });
}

// ---- the host side that every staged loop shares (acq_staged.h)
int as_col_stage(ffgp_handle* h, const AcqStagedArgs& a, dim3 tiles, int f0) {
  hipLaunchKernelGGL(ffgp_acq_staged_col_kernel, tiles, dim3(AS_T), 0, h->stream, a, f0);
  return as_launched();
}
int as_owner_stage(ffgp_handle* h, const AcqStagedPlan& pl, int k) {
  const size_t plane = (size_t)pl.a.Q * pl.a.D;
  hipLaunchKernelGGL(ffgp_acq_staged_owner_kernel, dim3((unsigned)((plane + AS_T - 1) / AS_T)), dim3(AS_T), 0, h->stream, pl.a, k,
                     k == pl.iters - 1 ? 1 : 0, pl.bc[2 * k], pl.bc[2 * k + 1]);
  return as_launched();
}
int as_solve_stage(ffgp_handle* h, const AcqStagedPlan& pl, int f) {
  const AcqStagedMember& m = pl.a.m[f];
  const int Q = pl.a.Q, Qp = pl.a.Qp;
  // V = L^-1 K_s (L^-1 lower: k ends at the tile row), B = L^-T V (k starts at it)
  int rc = ffgp_gemm_launch(h, OP_KMAJOR, OP_MNMAJOR, TILES_FULL, 0, pl.Linv[f], pl.np_of[f], m.Ks, Qp, m.V, Qp, m.n, Q, m.n, 1.0, 0.0, TRI_HI_I);
  if (rc == FFGP_OK)
    rc = ffgp_gemm_launch(h, OP_MNMAJOR, OP_MNMAJOR, TILES_FULL, 0, pl.Linv[f], pl.np_of[f], m.V, Qp, m.B, Qp, m.n, Q, m.n, 1.0, 0.0, TRI_LO_I);
  return rc;
}

int acq_staged_prepare(ffgp_handle* h, const ffgp_acq_stack* s, const ffgp_ktree* const* trees, int images, bool chain, size_t extra_doubles,
                       double* Xq_dev, int Q, int steps, const ffgp_adam* opt, double* state_dev, long step0, double* trace_dev, double* hist_dev,
                       double* grad_dev, AcqStagedPlan& pl) {
  // the argument classes acq_run refuses (acq_stack.hip), with these entries' own limit on n
  if (!h || !s || !Xq_dev || !trace_dev || Q <= 0 || steps < 0 || steps > FFGP_ACQ_MAX_STEPS || step0 < 0) return FFGP_ERR_ARG;
  if (steps > 0 && (!opt || !state_dev)) return FFGP_ERR_ARG;
  if (s->F < 1 || s->F > FFGP_ACQ_MAX_MEMBERS || !s->members) return FFGP_ERR_ARG;
  if (s->acq != FFGP_ACQ_UCB && s->acq != FFGP_ACQ_EI && s->acq != FFGP_ACQ_UCB_VAR) return FFGP_ERR_ARG;
  const int F = s->F, D = s->members[0].D;
  if (chain && D > FFGP_ACQ_MAX_D - 1) return FFGP_ERR_ARG;      // the members above the first take [x, mean below]: D + 1 inputs
  for (int f = 0; f < F; ++f) {
    const ffgp_acq_member& p = s->members[f];
    const bool tree = trees && trees[f];      // such a member carries no w_dev / amp_dev / kfun of its own
    if (!p.X_dev || !p.L_dev || !p.alpha_dev || (!tree && (!p.w_dev || !p.amp_dev))) return FFGP_ERR_ARG;
    if (p.n < 1 || p.n > FFGP_ACQ_STAGED_MAX_N || p.D < 1 || p.D > FFGP_ACQ_MAX_D || p.D != ((chain && f > 0) ? D + 1 : D) || p.d != 1)
      return FFGP_ERR_ARG;
    if (p.ldl < p.n || p.ldl > INT_MAX) return FFGP_ERR_ARG;
    if (!tree && (p.kfun < FFGP_KFUN_SE || p.kfun > FFGP_KFUN_RQ)) return FFGP_ERR_ARG;      // (the linear kernel's k(x, x) depends on x)
  }
  if ((size_t)Q * D > (size_t)INT_MAX || Q > INT_MAX - AS_COLS) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  AcqStagedArgs& a = pl.a;
  pl.iters = steps > 0 ? steps : 1;
  const int DM = acq_by_dm(chain ? D + 1 : D, [](auto dm) { return (int)dm(); });
  const int Qp = ffgp_round_up(Q, AS_COLS);
  pl.qt = Qp / AS_COLS;
  const size_t imgs = (size_t)images;
  // workspace, in doubles (the arithmetic beside FFGP_ACQ_STAGED_MAX_N in ffgp.h):
  //   [L_f^-1 (np_f x np_f) | the images of member f (K_s, DK, V, B: 4 n_f Qp; without DK 3 n_f Qp), f = 0..F-1 | TRTRI scratch per member
  //    | pm, pv | av, gm, gv | part | trees: self (Qp DM), the leaf records | the entry's own extra doubles]
  size_t xd = 0, md = 0, td = 0;
  int nch = 0;
  for (int f = 0; f < F; ++f) {
    const size_t n = (size_t)s->members[f].n, np = (size_t)ffgp_round_up((int)n, 16);
    xd += np * np;
    md += imgs * n * Qp;
    td += n * n / 4 + n * FFGP_NB + 16;
    nch = max(nch, (int)((n + AS_ROWS - 1) / AS_ROWS));
  }
  const size_t pd = (size_t)F * nch * Qp, sd = trees ? (size_t)Qp * DM : 0;
  // (the leaf records are 224 bytes each: a multiple of a double, so what follows them stays aligned)
  static_assert(sizeof(AcqMemberTree) % sizeof(double) == 0, "the leaf records end on a double");
  FFGP_CHECK(ffgp_ensure_ws(h, (xd + md + td + 2 * pd + 3 * (size_t)Qp + pd * DM + sd + extra_doubles) * sizeof(double) +
                                   (trees ? F * sizeof(AcqMemberTree) : 0)));
  double* X = h->ws;
  double* M = X + xd;
  double* T = M + md;
  a.pm = T + td; a.pv = a.pm + pd; a.av = a.pv + pd; a.gm = a.av + Qp; a.gv = a.gm + Qp; a.part = a.gv + Qp;
  a.self = trees ? a.part + pd * DM : nullptr;
  AcqMemberTree* const table_dev = trees ? reinterpret_cast<AcqMemberTree*>(a.part + pd * DM + sd) : nullptr;
  a.tab = table_dev;
  pl.extra = extra_doubles ? reinterpret_cast<double*>(reinterpret_cast<char*>(a.part + pd * DM + sd) + (trees ? F * sizeof(AcqMemberTree) : 0)) : nullptr;
  // zeros: L^-1 above the diagonal and in its padding, and the columns Q..Qp-1 of V and B, which no GEMM writes
  FFGP_CHECK(ffgp_zero_async(h, X, (xd + md) * sizeof(double)));
  for (int f = 0; f < F; ++f) {
    const ffgp_acq_member& p = s->members[f];
    const int n = p.n, np = ffgp_round_up(n, 16);
    const size_t img = (size_t)n * Qp;
    AcqStagedMember& m = a.m[f];
    m.X = p.X_dev; m.alpha = p.alpha_dev; m.w = p.w_dev; m.amp = p.amp_dev;
    m.Ks = M;
    if (imgs == 4) {
      m.DK = M + img; m.V = M + 2 * img; m.B = M + 3 * img;
    } else {
      m.DK = nullptr; m.V = M + img; m.B = M + 2 * img;
    }
    m.clamp = p.clamp_min; m.rinv = (p.kparam != 0.0) ? 1.0 / p.kparam : 1.0; m.var_add = p.var_add_all;
    m.mean_coef = p.mean_coef; m.var_coef = p.var_coef; m.n = n; m.kfun = p.kfun;
    pl.Linv[f] = X; pl.np_of[f] = np;
    // the handle's inverted diagonal blocks are rebuilt from each factor, for acq_run's reason: a trajectory depends on the factors alone
    ffgp_invalidate(h);
    FFGP_CHECK(ffgp_trtri_impl(h, p.L_dev, n, (int)p.ldl, X, np, T));
    X += (size_t)np * np;
    M += imgs * img;
    T += (size_t)n * n / 4 + (size_t)n * FFGP_NB + 16;
  }
  for (int f = F; f < FFGP_ACQ_MAX_MEMBERS; ++f) a.m[f] = a.m[0];      // never read: every member loop ends at F
  pl.bc.assign(2 * (size_t)pl.iters, 1.0);
  ffgp_adam_bc_table(opt, step0, steps, pl.bc.data());
  pl.table.resize(trees ? F : 0);      // (lives until the caller's wait)
  if (trees) {
    for (int f = 0; f < F; ++f) pl.table[f] = acq_member_tree(s->members[f], trees[f]);
    FFGP_HIP(hipMemcpyAsync(table_dev, pl.table.data(), pl.table.size() * sizeof(AcqMemberTree), hipMemcpyHostToDevice, h->stream));
  }
  a.level = s->level_dev;
  a.Xq = Xq_dev; a.state = state_dev; a.trace = trace_dev; a.hist = hist_dev; a.grad = grad_dev;
  a.F = F; a.D = D; a.DM = DM; a.Q = Q; a.Qp = Qp; a.nch = nch; a.steps = steps; a.acq = s->acq; a.accumulate = s->accumulate_grad ? 1 : 0;
  a.var_floor = s->var_floor; a.kappa = s->kappa; a.xi = s->xi; a.f_best = s->f_best;
  a.lr = opt ? opt->lr : 0.0; a.b1 = opt ? opt->beta1 : 0.0; a.b2 = opt ? opt->beta2 : 0.0; a.eps = opt ? opt->eps : 0.0;
  return FFGP_OK;
}

int acq_staged_finish(ffgp_handle* h, int rc) {
  // nothing waited inside the loop; the call itself is synchronous, as the one-launch entries are
  const hipError_t e = hipStreamSynchronize(h->stream);
  if (rc != FFGP_OK) return rc;
  return e == hipSuccess ? FFGP_OK : FFGP_ERR_HIP;
}

// The step loop of the two stack entries (acq_staged.h).
int acq_staged_run(ffgp_handle* h, const ffgp_acq_stack* s, const ffgp_ktree* const* trees, const AcqStagedStages& st, double* Xq_dev, int Q,
                   int steps, const ffgp_adam* opt, double* state_dev, long step0, double* trace_dev, double* hist_dev, double* grad_dev) {
  AcqStagedPlan pl;
  FFGP_CHECK(acq_staged_prepare(h, s, trees, st.images, false, 0, Xq_dev, Q, steps, opt, state_dev, step0, trace_dev, hist_dev, grad_dev, pl));
  const AcqStagedArgs& a = pl.a;
  const dim3 tiles(pl.qt, a.nch, a.F);
  int rc = FFGP_OK;
  for (int k = 0; k < pl.iters; ++k) {
    AS_STAGE(st.ks(h, a, tiles));
    for (int f = 0; f < a.F && rc == FFGP_OK; ++f) rc = as_solve_stage(h, pl, f);
    if (rc != FFGP_OK) break;
    AS_STAGE(as_col_stage(h, a, tiles, 0));
    AS_STAGE(st.value(h, a));
    AS_STAGE(st.grad(h, a, tiles));
    AS_STAGE(as_owner_stage(h, pl, k));
  }
  return acq_staged_finish(h, rc);
}

int ffgp_acq_optimize_stack_staged(ffgp_handle* h, const ffgp_acq_stack* s, double* Xq_dev, int Q, int steps, const ffgp_adam* opt,
                                   double* state_dev, long step0, double* trace_dev, double* hist_dev, double* grad_dev) {
  static const AcqStagedStages stages = {4, as_ks_stage, as_value_stage, as_grad_stage};
  return acq_staged_run(h, s, nullptr, stages, Xq_dev, Q, steps, opt, state_dev, step0, trace_dev, hist_dev, grad_dev);
}

