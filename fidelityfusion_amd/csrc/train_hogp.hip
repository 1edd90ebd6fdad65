// K Adam steps of HOGP blocks (GAR's fidelities) in one call, launch per stage: the Kronecker likelihood of
// hogp_simple._KronNLL and its closed-form backward as device code on raw parameters, the mode-product kernels under them and
// the loop around them.  Assembly, eigensolvers, kernel gradients and the Adam update are the library's existing launchers
// (ffgp_assemble_impl through the handle's collector, ffgp_syevj_small_impl / ffgp_syev_lds_impl, ffgp_kernel_grad_impl,
// ffgp_adam_update).  See include/ffgp.h (ffgp_train_hogp_raw) and DESIGN.md 4.8.
#include <cmath>

#include "drivers.h"

#define HG_MAXM 3          // output modes
#define HG_MAXD 64         // points per output mode
#define HG_MAXP FFGP_HOGP_MAX_OUT       // prod d: two images of a sample's tensor must fit in LDS (2 * 4096 * 8 B = 64 KiB of the CU's 160)
#define HG_WS_HEAD 2048    // doubles at the head of the handle's workspace left to ffgp_kernel_grad_impl's partial sums
#define HG_TILE 16         // tile edge of the sample-mode product

// ---- grids 0..d-1 as [d, nw] columns (HOGP_simple.grid, broadcast to an ARD kernel's D columns as HOGP_simple._kernel does)
__global__ void ffgp_hogp_grid_kernel(double* __restrict__ G, int d, int nw) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < d * nw) G[t] = (double)(t / nw);
}

// ---- per step: raw -> effective parameters, and a residual block's targets r = y_high - y_low x_last V
struct HogpPrep {
  const double* w; const double* amp; const double* noise;
  double* eff;               // [w (D) | amp | tau | noise]
  int D, bcast;
  int w_link, amp_link; double w_c, amp_c;
  const double* V; const double* yl; const double* yh; double* r;      // V null: a plain block
  long nd; int hh, ll; long vrs, vcs;      // V element (a, b) at V[a * vrs + b * vcs]
};
__global__ __launch_bounds__(256) void ffgp_hogp_prep_kernel(HogpPrep a) {
  if (blockIdx.x == 0) {
    const int t = threadIdx.x;
    if (t < a.D) a.eff[t] = ffgp_link_val(a.w_link, a.w[a.bcast ? 0 : t], a.w_c);
    if (t == 0) {
      const double nv = a.noise[0];
      a.eff[a.D] = ffgp_link_val(a.amp_link, a.amp[0], a.amp_c);
      a.eff[a.D + 1] = 1.0 / nv;
      a.eff[a.D + 2] = nv;
    }
  }
  if (!a.V) return;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < a.nd; t += (long)gridDim.x * 256) {
    const long rest = t / a.hh;
    const int hi = (int)(t - rest * a.hh);
    const double* __restrict__ yl = a.yl + rest * a.ll;
    const double* __restrict__ v = a.V + (size_t)hi * a.vrs;
    double acc = 0.0;
    for (int b = 0; b < a.ll; ++b) acc = __builtin_fma(yl[b], v[b * a.vcs], acc);
    a.r[t] = __dsub_rn(a.yh[t], acc);
  }
}

// ---- sample-mode product  out[i, q] = sum_j F(i, j) in[j, q],  F = Mat (trans = 0) or Mat^T (trans = 1), Mat [n, n], in / out [n, P]:
// 16 x 16 output tiles, the two operand tiles staged through LDS, j ascending -- one fixed summation order whatever the grid.  (The inner
// loop reads sf[ty][jj], one address per row of the wave, and sb[jj][tx], contiguous: neither conflicts; the 17-double rows only keep the
// transposed fill of sf, trans = 1, off one bank.)
__global__ __launch_bounds__(256) void ffgp_hogp_gemm0_kernel(const double* __restrict__ Mat, int trans, const double* __restrict__ in,
                                                              double* __restrict__ out, int n, int P) {
  __shared__ double sf[HG_TILE][HG_TILE + 1];
  __shared__ double sb[HG_TILE][HG_TILE + 1];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int tq = blockIdx.x, ti = blockIdx.y;
  const int i = ti * HG_TILE + ty, q = tq * HG_TILE + tx;
  double acc = 0.0;
  for (int j0 = 0; j0 < n; j0 += HG_TILE) {
    {   // sf[ty][tx] = F(ti * 16 + ty, j0 + tx)
      const int fi = ti * HG_TILE + ty, fj = j0 + tx;
      double v = 0.0;
      if (fi < n && fj < n) v = trans ? Mat[(size_t)fj * n + fi] : Mat[(size_t)fi * n + fj];
      sf[ty][tx] = v;
      const int bj = j0 + ty;
      sb[ty][tx] = (bj < n && q < P) ? in[(size_t)bj * P + q] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < HG_TILE; ++jj) acc = __builtin_fma(sf[ty][jj], sb[jj][tx], acc);
    __syncthreads();
  }
  if (i < n && q < P) out[(size_t)i * P + q] = acc;
}

// ---- the output modes of ONE sample per workgroup: its d_1 x d_2 (x d_3) tensor lives in LDS (two images, ping-pong) and the mode
// factors are applied in turn.  (For the LAST mode, inner = 1, the lanes of a wave read cur + o d_m + b: a stride of d_m doubles, a 4- to 8-way
// bank conflict at d_m = 8 or 16.  Left as it is: forward and backward together are ~5 % of a step.)  fwd = 0: out = in x_{m in mask} mat_m (mat or mat^T).  fwd = 1, the likelihood's middle:
//   T_1 = in x_m U_m^T (in = Y x_0 U_0^T),  A = ((lambda_0 lambda_1) ...) + tau,  W = T_1 (1 / A),  out = W x_m U_m,
//   part[i] = (sum log A, sum T_1 W, sum (1/A - W^2)) of this sample -- per-thread strided sums, a shuffle butterfly, four wave sums in order.
struct HogpModes {
  const double* in; double* out;
  int M, P; int d[HG_MAXM];
  const double* mat[HG_MAXM];
  int trans; unsigned mask; int fwd;
  const double* lam[HG_MAXM + 1]; const double* tau;
  double* A; double* part;
};
__device__ __forceinline__ void hg_apply_modes(const HogpModes& a, int trans, unsigned mask, double*& cur, double*& nxt, int tid) {
  int inner = a.P;
  for (int m = 0; m < a.M; ++m) {
    const int dm = a.d[m];
    inner /= dm;
    if (!((mask >> m) & 1u)) continue;
    const double* __restrict__ mat = a.mat[m];
    const int blk = dm * inner;
    for (int e = tid; e < a.P; e += 256) {
      const int o = e / blk, rem = e - o * blk;
      const int ai = rem / inner, q = rem - ai * inner;
      const double* __restrict__ src = cur + o * blk + q;
      double acc = 0.0;
      if (trans) {
        for (int b = 0; b < dm; ++b) acc = __builtin_fma(mat[b * dm + ai], src[b * inner], acc);
      } else {
        for (int b = 0; b < dm; ++b) acc = __builtin_fma(mat[ai * dm + b], src[b * inner], acc);
      }
      nxt[e] = acc;
    }
    __syncthreads();
    double* t = cur; cur = nxt; nxt = t;
  }
}
extern __shared__ double hg_lds[];
__global__ __launch_bounds__(256) void ffgp_hogp_modes_kernel(HogpModes a) {
  double* cur = hg_lds;
  double* nxt = hg_lds + a.P;
  double* red = hg_lds + 2 * a.P;      // [3][4]
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * a.P;
  for (int e = tid; e < a.P; e += 256) cur[e] = a.in[base + e];
  __syncthreads();
  hg_apply_modes(a, a.trans, a.mask, cur, nxt, tid);
  if (!a.fwd) {
    for (int e = tid; e < a.P; e += 256) a.out[base + e] = cur[e];
    return;
  }
  const double tau = a.tau[0], lam0 = a.lam[0][blockIdx.x];
  double s_log = 0.0, s_q = 0.0, s_dt = 0.0;
  for (int e = tid; e < a.P; e += 256) {
    int rem = e, inner = a.P;
    double v = lam0;
    for (int m = 0; m < a.M; ++m) {
      inner /= a.d[m];
      const int ai = rem / inner;
      rem -= ai * inner;
      v = v * a.lam[m + 1][ai];
    }
    const double A = v + tau;
    const double Ainv = 1.0 / A;
    const double t1 = cur[e];
    const double w = t1 * Ainv;
    s_log += log(A);
    s_q = __builtin_fma(t1, w, s_q);
    s_dt += Ainv - w * w;
    a.A[base + e] = A;
    cur[e] = w;
  }
  for (int o = 32; o > 0; o >>= 1) {
    s_log += __shfl_xor(s_log, o);
    s_q += __shfl_xor(s_q, o);
    s_dt += __shfl_xor(s_dt, o);
  }
  if ((tid & 63) == 0) {
    red[tid >> 6] = s_log;
    red[4 + (tid >> 6)] = s_q;
    red[8 + (tid >> 6)] = s_dt;
  }
  __syncthreads();      // (also: every W is in `cur` before the second rotation reads it)
  if (tid < 3) a.part[(size_t)blockIdx.x * 3 + tid] = ((red[4 * tid] + red[4 * tid + 1]) + red[4 * tid + 2]) + red[4 * tid + 3];
  hg_apply_modes(a, 0, (1u << a.M) - 1u, cur, nxt, tid);
  for (int e = tid; e < a.P; e += 256) a.out[base + e] = cur[e];
}

// ---- c_m[k] = sum over every other index of (prod_{m' != m} lambda_m') / A, and the three scalar sums of the per-sample parts: one wave
// per entry, lanes stride the reduction index, a shuffle butterfly at the end (every lane holds the same sum)
struct HogpCvec {
  const double* A; const double* part; double* scal;
  int nm;                    // matrices: M + 1
  int dim[HG_MAXM + 1];      // n, d_1, ...
  long nd;
  const double* lam[HG_MAXM + 1];
  double* c[HG_MAXM + 1];
};
__global__ __launch_bounds__(256) void ffgp_hogp_cvec_kernel(HogpCvec a) {
  const int lane = threadIdx.x & 63;
  int ent = blockIdx.x * 4 + (threadIdx.x >> 6);
  int m = 0;
  while (m < a.nm && ent >= a.dim[m]) { ent -= a.dim[m]; ++m; }
  double x = 0.0;
  if (m == a.nm) {
    if (ent >= 3) return;
    for (int i = lane; i < a.dim[0]; i += 64) x += a.part[(size_t)i * 3 + ent];
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    if (lane == 0) a.scal[ent] = x;
    return;
  }
  const int k = ent;
  long stride[HG_MAXM + 1];      // row-major strides of [n, d_1, ...]
  {
    long s = 1;
    for (int q = a.nm - 1; q >= 0; --q) { stride[q] = s; s *= a.dim[q]; }
  }
  const long R = a.nd / a.dim[m];
  for (long r = lane; r < R; r += 64) {
    // decode r over the dimensions other than m (row-major), multiplying the eigenvalues in ascending mode order
    long rem = r, inner = R, off = (long)k * stride[m];
    double lamv[HG_MAXM + 1];
    for (int q = 0; q < a.nm; ++q) {
      if (q == m) continue;
      inner /= a.dim[q];
      const long iq = rem / inner;
      rem -= iq * inner;
      off += iq * stride[q];
      lamv[q] = a.lam[q][iq];
    }
    double t = 1.0 / a.A[off];
    for (int q = 0; q < a.nm; ++q)
      if (q != m) t = t * lamv[q];
    x += t;
  }
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  if (lane == 0) a.c[m][k] = x;
}

// ---- out[a, b] = scale * (sum_k U[a, k] c[k] U[b, k]  -  sum_{o, q} X[o, a, q] Y[o, b, q])   (U null: the second sum alone)
// X viewed [outer, da, inner], Y [outer, db, inner]; one wave per output, lanes stride the reduction index, shuffle butterfly.
// dK_m of the Kronecker likelihood (X = g, Y = P, U = U_m) and the residual map's gradient (X = g, Y = y_low, inner = 1).
struct HogpDk {
  const double* X; const double* Y; const double* U; const double* c;
  double* out;
  int da, db; long outer, inner;
  double scale;
};
__global__ __launch_bounds__(256) void ffgp_hogp_dk_kernel(HogpDk a) {
  const int lane = threadIdx.x & 63;
  const long ent = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ent >= (long)a.da * a.db) return;
  const int ai = (int)(ent / a.db), bi = (int)(ent - (long)ai * a.db);
  double t1 = 0.0, t2 = 0.0;
  if (a.U) {
    for (int k = lane; k < a.da; k += 64) t1 = __builtin_fma(a.U[(size_t)ai * a.da + k] * a.c[k], a.U[(size_t)bi * a.da + k], t1);
  }
  const long R = a.outer * a.inner;
  for (long r = lane; r < R; r += 64) {
    const long o = r / a.inner, q = r - o * a.inner;
    t2 = __builtin_fma(a.X[(o * a.da + ai) * a.inner + q], a.Y[(o * a.db + bi) * a.inner + q], t2);
  }
  for (int o = 32; o > 0; o >>= 1) {
    t1 += __shfl_xor(t1, o);
    t2 += __shfl_xor(t2, o);
  }
  if (lane == 0) a.out[ent] = a.scale * (t1 - t2);
}

// ---- the step's tail for ONE model: loss from the scalar sums, the failure rule, the links' chain rule on the summed kernel
// gradients, d noise, and torch.optim.Adam's update of [w (nw) | amp | noise | V (hl)] in place
struct HogpAdam {
  double* w; double* amp; double* noise; double* V;
  int nw, D, bcast, hl, nm, ll; long vrs, vcs;
  int w_link, amp_link; double w_c, amp_c;
  const double* gk;          // [nm][D + 2]: g_w (D or nw) | g_amp per matrix
  const double* gV;
  const double* scal;
  const int* info;           // [nm] the eigensolvers' status words
  int* st;                   // sticky: 0, or 1 + the failing step
  double nd;
  double* state;
  double lr, b1, b2, eps, bc1, bc2_sqrt;
  double* trace; int step;
};
__global__ __launch_bounds__(256) void ffgp_hogp_adam_kernel(HogpAdam a) {
  const double loss = ((0.5 * a.nd * 1.8378770664093453) + 0.5 * a.scal[0] + 0.5 * a.scal[1]) / a.nd;
  int bad = a.st[0];
  if (!bad) {
    bool now = !(fabs(loss) <= 1.79769313486231570815e308);      // NaN or Inf
    for (int q = 0; q < a.nm; ++q) now = now || a.info[q] != 0;
    bad = now ? a.step + 1 : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.st[0] = bad;
    a.trace[a.step] = bad ? __builtin_nan("") : loss;
  }
  if (bad) return;
  const int P = a.nw + 2 + a.hl;
  const int gs = a.D + 2;
  for (int i = threadIdx.x; i < P; i += 256) {
    double* par;
    double g;
    if (i < a.nw) {
      par = a.w + i;
      double s;
      if (a.bcast) {
        s = 0.0;
        for (int k = 0; k < a.D; ++k) s += a.gk[k];
      } else {
        s = a.gk[i];
      }
      for (int q = 1; q < a.nm; ++q) s += a.gk[(size_t)q * gs + i];
      g = s * ffgp_link_der(a.w_link, par[0], a.w_c);
    } else if (i == a.nw) {
      par = a.amp;
      double s = a.gk[a.D];
      for (int q = 1; q < a.nm; ++q) s += a.gk[(size_t)q * gs + a.D];
      g = s * ffgp_link_der(a.amp_link, par[0], a.amp_c);
    } else if (i == a.nw + 1) {
      par = a.noise;
      const double dtau = 0.5 * a.scal[2] / a.nd;
      g = -dtau / (par[0] * par[0]);
    } else {
      const int j = i - a.nw - 2;      // (row-major over [h, l], whatever V's strides)
      par = a.V + (size_t)(j / a.ll) * a.vrs + (size_t)(j % a.ll) * a.vcs;
      g = a.gV[i - a.nw - 2];
    }
    double* m = a.state + i;
    ffgp_adam_update(par, m, m + P, g, a.lr, a.b1, a.b2, a.eps, a.bc1, a.bc2_sqrt);
  }
}

// ---- host: one model's workspace and stage list
struct HogpWork {
  int n, D, nw, M, nm; int dim[HG_MAXM + 1];      // dim[0] = n
  int P; long nd;
  bool res; int hh, ll;
  double *eff, *grid[HG_MAXM], *K[HG_MAXM + 1], *U[HG_MAXM + 1], *lam[HG_MAXM + 1], *c[HG_MAXM + 1], *dK, *gk, *R, *A, *g, *Pb, *Q0, *part,
      *scal, *gV;
  int *info, *st;
};
static size_t hg_up(size_t x) { return (x + 7) / 8 * 8; }      // (64-byte steps)

static int hogp_modes_launch(ffgp_handle* h, const HogpWork& w, const double* in, double* out, double* const* mat, int trans, unsigned mask,
                             int fwd) {
  HogpModes a;
  memset(&a, 0, sizeof(a));
  a.in = in; a.out = out; a.M = w.M; a.P = w.P;
  for (int m = 0; m < w.M; ++m) { a.d[m] = w.dim[m + 1]; a.mat[m] = mat[m + 1]; }
  a.trans = trans; a.mask = mask; a.fwd = fwd;
  for (int q = 0; q < w.nm; ++q) a.lam[q] = w.lam[q];
  a.tau = w.eff + w.D + 1;
  a.A = w.A; a.part = w.part;
  hipLaunchKernelGGL(ffgp_hogp_modes_kernel, dim3(w.n), dim3(256), (size_t)(2 * w.P + 16) * sizeof(double), h->stream, a);
  return hipGetLastError() == hipSuccess ? FFGP_OK : FFGP_ERR_HIP;
}

static int hogp_dk_launch(ffgp_handle* h, const double* X, const double* Y, const double* U, const double* c, double* out, int da, int db,
                          long outer, long inner, double scale) {
  HogpDk a;
  a.X = X; a.Y = Y; a.U = U; a.c = c; a.out = out; a.da = da; a.db = db; a.outer = outer; a.inner = inner; a.scale = scale;
  hipLaunchKernelGGL(ffgp_hogp_dk_kernel, dim3((unsigned)(((long)da * db + 3) / 4)), dim3(256), 0, h->stream, a);
  return hipGetLastError() == hipSuccess ? FFGP_OK : FFGP_ERR_HIP;
}

static int hogp_gemm0_launch(ffgp_handle* h, const HogpWork& w, const double* Mat, int trans, const double* in, double* out) {
  const dim3 g0((w.P + HG_TILE - 1) / HG_TILE, (w.n + HG_TILE - 1) / HG_TILE);
  hipLaunchKernelGGL(ffgp_hogp_gemm0_kernel, g0, dim3(256), 0, h->stream, Mat, trans, in, out, w.n, w.P);
  return hipGetLastError() == hipSuccess ? FFGP_OK : FFGP_ERR_HIP;
}

// one stage of the step loop: a refused launch ends the call there, before a later stage reads what it did not write
#define HG_STAGE(call)                      \
  if ((lrc = (call)) != FFGP_OK) break

extern "C" {

int ffgp_train_hogp_raw(ffgp_handle* h, int F, const ffgp_hogp_model* mo, const ffgp_links* l, const ffgp_hogp_residual* r, int steps,
                        const ffgp_adam* opt, double* state_dev, long state_stride, const long* step0, double* trace_dev,
                        long trace_stride, const ffgp_hogp_cache* cache, int* fail_step) {
  if (!h || !mo || !l || !opt || !state_dev || !step0 || !trace_dev || F < 1 || F > FFGP_TRAIN_MAXF || steps <= 0 || trace_stride < steps)
    return FFGP_ERR_ARG;
  std::vector<HogpWork> W(F);
  std::vector<long> vrs(F, 0), vcs(F, 0);
  size_t tot = 0;
  for (int f = 0; f < F; ++f) {
    const ffgp_hogp_model& q = mo[f];
    HogpWork& w = W[f];
    if (q.n < 1 || q.n > FFGP_SYEV_LDS_MAX_N || q.D < 1 || q.D > 128 || q.nmodes < 1 || q.nmodes > HG_MAXM || !q.X_dev || !q.w_dev ||
        !q.amp_dev || !q.noise_dev || q.kfun < FFGP_KFUN_SE || q.kfun > FFGP_KFUN_MATERN52 || step0[f] < 0)
      return FFGP_ERR_ARG;
    if (l[f].w_broadcast && q.D == 1) return FFGP_ERR_ARG;      // (a broadcast link names ONE raw value for D > 1 columns)
    w.n = q.n; w.D = q.D; w.nw = l[f].w_broadcast ? 1 : q.D; w.M = q.nmodes; w.nm = q.nmodes + 1;
    w.dim[0] = q.n;
    w.P = 1;
    for (int m = 0; m < q.nmodes; ++m) {
      if (q.dims[m] < 1 || q.dims[m] > HG_MAXD) return FFGP_ERR_ARG;
      w.dim[m + 1] = q.dims[m];
      w.P *= q.dims[m];
    }
    if (w.P > HG_MAXP) return FFGP_ERR_ARG;
    w.nd = (long)w.n * w.P;
    w.res = r && r[f].V_dev;
    w.hh = w.dim[w.M]; w.ll = 0;
    if (w.res) {
      if (!r[f].y_low_dev || !r[f].y_high_dev || r[f].l < 1 || r[f].l > HG_MAXD) return FFGP_ERR_ARG;
      w.ll = r[f].l;
      const bool dflt = r[f].V_row_stride == 0 && r[f].V_col_stride == 0;
      vrs[f] = dflt ? w.ll : r[f].V_row_stride;
      vcs[f] = dflt ? 1 : r[f].V_col_stride;
      if (vrs[f] < 1 || vcs[f] < 1) return FFGP_ERR_ARG;
    } else if (!q.Y_dev) {
      return FFGP_ERR_ARG;
    }
    if (state_stride < 2 * (long)(w.nw + 2 + (w.res ? w.hh * w.ll : 0))) return FFGP_ERR_ARG;
    // workspace, in doubles
    size_t need = hg_up(w.D + 4) + hg_up(w.nm * (w.D + 2)) + hg_up(3 * (size_t)w.n) + 8 + hg_up((size_t)HG_MAXD * HG_MAXD) + 16;
    for (int q2 = 0; q2 < w.nm; ++q2) need += 2 * hg_up((size_t)w.dim[q2] * w.dim[q2]) + 2 * hg_up(w.dim[q2]);
    for (int m = 0; m < w.M; ++m) need += hg_up((size_t)w.dim[m + 1] * w.nw);
    need += hg_up((size_t)std::max(w.n, HG_MAXD) * std::max(w.n, HG_MAXD));
    need += (size_t)(w.res ? 5 : 4) * hg_up((size_t)w.nd);
    tot += need;
  }
  FFGP_HIP(hipSetDevice(h->device));
  // the handle's workspace, kept between calls: its head stays ffgp_kernel_grad_impl's (whose own ffgp_ensure_ws then never reallocates)
  FFGP_CHECK(ffgp_ensure_ws(h, (HG_WS_HEAD + tot) * sizeof(double)));
  {
    double* p = h->ws + HG_WS_HEAD;
    auto take = [&](size_t cnt) { double* q = p; p += hg_up(cnt); return q; };
    for (int f = 0; f < F; ++f) {
      HogpWork& w = W[f];
      w.eff = take(w.D + 4);
      w.gk = take((size_t)w.nm * (w.D + 2));
      w.part = take(3 * (size_t)w.n);
      w.scal = take(8);
      w.gV = take((size_t)HG_MAXD * HG_MAXD);
      w.info = reinterpret_cast<int*>(take(8));      // [info (8 doubles) | st (8 doubles)]: the only words that must start at zero
      w.st = reinterpret_cast<int*>(take(8));
      FFGP_HIP(hipMemsetAsync(w.info, 0, 16 * sizeof(double), h->stream));
      for (int q = 0; q < w.nm; ++q) {
        const size_t sq = (size_t)w.dim[q] * w.dim[q];
        w.K[q] = take(sq); w.U[q] = take(sq); w.lam[q] = take(w.dim[q]); w.c[q] = take(w.dim[q]);
      }
      for (int m = 0; m < w.M; ++m) w.grid[m] = take((size_t)w.dim[m + 1] * w.nw);
      w.dK = take((size_t)std::max(w.n, HG_MAXD) * std::max(w.n, HG_MAXD));
      w.A = take(w.nd); w.g = take(w.nd); w.Pb = take(w.nd); w.Q0 = take(w.nd);
      w.R = w.res ? take(w.nd) : nullptr;
    }
  }
  // (unsynchronised on purpose, as eig_lds.hip's: setting the same attribute twice is harmless)
  static bool attr_set[64] = {false};
  if (h->device < 0 || h->device >= 64 || !attr_set[h->device]) {
    FFGP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ffgp_hogp_modes_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)((2 * HG_MAXD * HG_MAXD + 16) * sizeof(double))));
    if (h->device >= 0 && h->device < 64) attr_set[h->device] = true;
  }
  for (int f = 0; f < F; ++f)
    for (int m = 0; m < W[f].M; ++m) {
      const int cnt = W[f].dim[m + 1] * W[f].nw;
      hipLaunchKernelGGL(ffgp_hogp_grid_kernel, dim3((cnt + 255) / 256), dim3(256), 0, h->stream, W[f].grid[m], W[f].dim[m + 1], W[f].nw);
    }
  const bool timed = h->timing >= 1 && F == 1;      // (the per-stage split of the LAST step of a one-model call: ffgp_last_timings)
  // The eigensolvers are one workgroup per matrix and latency-bound (a millisecond each: the Jacobi sweeps), and the M + 1 matrices of a
  // step -- of all F models -- are independent: they are dealt round robin onto the call's stream and the handle's two side streams
  // (the lanes of ffgp_nlml_fused_batch: fork and join by events, per step), so up to three run side by side.
  FFGP_CHECK(ffgp_ensure_aux2(h));
  for (int z = 0; z < 3; ++z)
    if (!h->lane_ev[z]) FFGP_HIP(hipEventCreateWithFlags(&h->lane_ev[z], hipEventDisableTiming));
  hipStream_t const main_stream = h->stream;
  hipStream_t const lanes[3] = {main_stream, h->aux2, h->aux3};
  int lrc = FFGP_OK;
  for (int k = 0; k < steps && lrc == FFGP_OK; ++k) {
    const bool mark = timed && k == steps - 1;
    if (mark) { h->n_stages = 0; stage_mark(h, 0); }
    for (int f = 0; f < F && lrc == FFGP_OK; ++f) {
      const HogpWork& w = W[f];
      const ffgp_hogp_model& q = mo[f];
      // 1. effective parameters and targets
      HogpPrep pa;
      memset(&pa, 0, sizeof(pa));
      pa.w = q.w_dev; pa.amp = q.amp_dev; pa.noise = q.noise_dev; pa.eff = w.eff; pa.D = w.D; pa.bcast = l[f].w_broadcast ? 1 : 0;
      pa.w_link = l[f].w_link; pa.amp_link = l[f].amp_link; pa.w_c = l[f].w_c; pa.amp_c = l[f].amp_c;
      pa.nd = w.nd; pa.hh = w.hh; pa.ll = w.ll;
      if (w.res) { pa.vrs = vrs[f]; pa.vcs = vcs[f]; pa.V = r[f].V_dev; pa.yl = r[f].y_low_dev; pa.yh = r[f].y_high_dev; pa.r = w.R; }
      const unsigned pblocks = w.res ? (unsigned)std::min<long>((w.nd + 255) / 256, 1024) : 1u;
      hipLaunchKernelGGL(ffgp_hogp_prep_kernel, dim3(pblocks), dim3(256), 0, h->stream, pa);
      if (hipGetLastError() != hipSuccess) { lrc = FFGP_ERR_HIP; break; }
      // 2. K_0 ... K_M in one launch (the handle's collector parks the M + 1 assemblies and flushes them together)
      ffgp_assemble_collect_begin(h);
      lrc = ffgp_assemble_impl(h, q.X_dev, w.n, q.X_dev, w.n, w.D, w.eff, w.eff + w.D, q.clamp_min, nullptr, nullptr, 0, nullptr, 0, 0.0, 0.0,
                               w.K[0], w.n, 0, q.kfun, q.kparam);
      for (int m = 0; m < w.M && lrc == FFGP_OK; ++m)
        lrc = ffgp_assemble_impl(h, w.grid[m], w.dim[m + 1], w.grid[m], w.dim[m + 1], w.nw, w.eff, w.eff + w.D, q.clamp_min, nullptr, nullptr, 0,
                                 nullptr, 0, 0.0, 0.0, w.K[m + 1], w.dim[m + 1], 0, q.kfun, q.kparam);
      const int erc = ffgp_assemble_collect_end(h);
      if (lrc == FFGP_OK) lrc = erc;
      if (lrc != FFGP_OK) break;
    }
    if (lrc != FFGP_OK) break;
    if (mark) stage_mark(h, 1);
    // 3. eigenpairs: hogp_simple.eigen_pairs' routing, the matrices of all models over the three lanes
    {
      bool ok = hipEventRecord(h->lane_ev[0], main_stream) == hipSuccess;
      for (int z = 1; z < 3 && ok; ++z) ok = hipStreamWaitEvent(lanes[z], h->lane_ev[0], 0) == hipSuccess;
      int j = 0;
      for (int f = 0; f < F && ok && lrc == FFGP_OK; ++f) {
        const HogpWork& w = W[f];
        for (int m = 0; m < w.nm && lrc == FFGP_OK; ++m, ++j) {
          const int dm = w.dim[m];
          h->stream = lanes[j % 3];
          if (dm <= 64) lrc = ffgp_syevj_small_impl(h, w.K[m], dm, dm, 1, 0, w.U[m], dm, 0, w.lam[m], 0, 0);
          else lrc = ffgp_syev_lds_impl(h, w.K[m], dm, dm, 1, 0, w.U[m], dm, 0, w.lam[m], 0, 0, w.info + m);
        }
      }
      h->stream = main_stream;
      for (int z = 1; z < 3 && ok; ++z)      // (joined on every way out: the workspace is freed behind the call's stream)
        ok = hipEventRecord(h->lane_ev[z], lanes[z]) == hipSuccess && hipStreamWaitEvent(main_stream, h->lane_ev[z], 0) == hipSuccess;
      if (!ok && lrc == FFGP_OK) lrc = FFGP_ERR_HIP;
    }
    if (lrc != FFGP_OK) break;
    if (mark) stage_mark(h, 2);
    for (int f = 0; f < F && lrc == FFGP_OK; ++f) {
      const HogpWork& w = W[f];
      const ffgp_hogp_model& q = mo[f];
      const double s = 1.0 / (double)w.nd;
      const double* Y = w.res ? w.R : q.Y_dev;
      // 4. forward: Z = Y x_0 U_0^T; T_1, A, W, the per-sample sums and G' = W x_{m >= 1} U_m; g = G' x_0 U_0
      HG_STAGE(hogp_gemm0_launch(h, w, w.U[0], 1, Y, w.Q0));
      HG_STAGE(hogp_modes_launch(h, w, w.Q0, w.Pb, w.U, 1, (1u << w.M) - 1u, 1));
      HG_STAGE(hogp_gemm0_launch(h, w, w.U[0], 0, w.Pb, w.g));
      if (mark) stage_mark(h, 3);
      // 5. backward: the c vectors and scalar sums, then dK_m and its chain onto the effective kernel parameters, matrix by matrix
      {
        HogpCvec ca;
        memset(&ca, 0, sizeof(ca));
        ca.A = w.A; ca.part = w.part; ca.scal = w.scal; ca.nm = w.nm; ca.nd = w.nd;
        int ents = 3;
        for (int m = 0; m < w.nm; ++m) { ca.dim[m] = w.dim[m]; ca.lam[m] = w.lam[m]; ca.c[m] = w.c[m]; ents += w.dim[m]; }
        hipLaunchKernelGGL(ffgp_hogp_cvec_kernel, dim3((ents + 3) / 4), dim3(256), 0, h->stream, ca);
      }
      HG_STAGE(hipGetLastError() == hipSuccess ? FFGP_OK : FFGP_ERR_HIP);
      const int gs = w.D + 2;
      // matrix 0: P = g x_{m >= 1} K_m
      HG_STAGE(hogp_modes_launch(h, w, w.g, w.Pb, w.K, 0, (1u << w.M) - 1u, 0));
      HG_STAGE(hogp_dk_launch(h, w.g, w.Pb, w.U[0], w.c[0], w.dK, w.n, w.n, 1, w.P, 0.5 * s));
      lrc = ffgp_kernel_grad_impl(h, q.X_dev, w.n, q.X_dev, w.n, w.D, w.eff, w.eff + w.D, q.clamp_min, q.kfun, q.kparam, w.dK, w.n, w.gk,
                                  w.gk + w.D, nullptr);
      if (lrc != FFGP_OK) break;
      // modes: Q0 = g x_0 K_0 is shared; P_m = Q0 x_{m' >= 1, m' != m} K_m'
      HG_STAGE(hogp_gemm0_launch(h, w, w.K[0], 0, w.g, w.Q0));
      long outer = w.n;
      for (int m = 1; m <= w.M && lrc == FFGP_OK; ++m) {
        const int dm = w.dim[m];
        const long inner = w.nd / (outer * dm);
        const double* Pm = w.Q0;
        if (w.M > 1) {
          HG_STAGE(hogp_modes_launch(h, w, w.Q0, w.Pb, w.K, 0, ((1u << w.M) - 1u) & ~(1u << (m - 1)), 0));
          Pm = w.Pb;
        }
        HG_STAGE(hogp_dk_launch(h, w.g, Pm, w.U[m], w.c[m], w.dK, dm, dm, outer, inner, 0.5 * s));
        lrc = ffgp_kernel_grad_impl(h, w.grid[m - 1], dm, w.grid[m - 1], dm, w.nw, w.eff, w.eff + w.D, q.clamp_min, q.kfun, q.kparam, w.dK, dm,
                                    w.gk + (size_t)m * gs, w.gk + (size_t)m * gs + w.D, nullptr);
        outer *= dm;
      }
      if (lrc != FFGP_OK) break;
      if (w.res) HG_STAGE(hogp_dk_launch(h, w.g, r[f].y_low_dev, nullptr, nullptr, w.gV, w.hh, w.ll, w.nd / w.hh, 1, s));
      if (mark) stage_mark(h, 4);
      // 6. chain rule, Adam, trace
      HogpAdam aa;
      memset(&aa, 0, sizeof(aa));
      aa.w = q.w_dev; aa.amp = q.amp_dev; aa.noise = q.noise_dev; aa.V = w.res ? r[f].V_dev : nullptr;
      aa.ll = w.res ? w.ll : 1; aa.vrs = vrs[f]; aa.vcs = vcs[f];
      aa.nw = w.nw; aa.D = w.D; aa.bcast = l[f].w_broadcast ? 1 : 0; aa.hl = w.res ? w.hh * w.ll : 0; aa.nm = w.nm;
      aa.w_link = l[f].w_link; aa.amp_link = l[f].amp_link; aa.w_c = l[f].w_c; aa.amp_c = l[f].amp_c;
      aa.gk = w.gk; aa.gV = w.gV; aa.scal = w.scal; aa.info = w.info; aa.st = w.st; aa.nd = (double)w.nd;
      aa.state = state_dev + (size_t)f * state_stride;
      aa.lr = opt->lr; aa.b1 = opt->beta1; aa.b2 = opt->beta2; aa.eps = opt->eps;
      ffgp_adam_bc(opt, step0[f], k, &aa.bc1, &aa.bc2_sqrt);
      aa.trace = trace_dev + (size_t)f * trace_stride; aa.step = k;
      hipLaunchKernelGGL(ffgp_hogp_adam_kernel, dim3(1), dim3(256), 0, h->stream, aa);
      HG_STAGE(hipGetLastError() == hipSuccess ? FFGP_OK : FFGP_ERR_HIP);
      if (mark) stage_mark(h, 5);
    }
  }
  if (lrc != FFGP_OK || hipGetLastError() != hipSuccess) {
    hipStreamSynchronize(h->aux2);
    hipStreamSynchronize(h->aux3);
    hipStreamSynchronize(h->stream);
    return lrc != FFGP_OK ? lrc : FFGP_ERR_HIP;
  }
  if (cache) {      // the last step's matrices, eigenpairs, A and g: what HOGP_simple.forward reads
    for (int f = 0; f < F; ++f) {
      const HogpWork& w = W[f];
      const ffgp_hogp_cache& c = cache[f];
      for (int m = 0; m < w.nm; ++m) {
        const size_t sq = (size_t)w.dim[m] * w.dim[m] * sizeof(double);
        if (c.K_dev[m]) FFGP_HIP(hipMemcpyAsync(c.K_dev[m], w.K[m], sq, hipMemcpyDeviceToDevice, h->stream));
        if (c.evecs_dev[m]) FFGP_HIP(hipMemcpyAsync(c.evecs_dev[m], w.U[m], sq, hipMemcpyDeviceToDevice, h->stream));
        if (c.evals_dev[m]) FFGP_HIP(hipMemcpyAsync(c.evals_dev[m], w.lam[m], w.dim[m] * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
      }
      if (c.A_dev) FFGP_HIP(hipMemcpyAsync(c.A_dev, w.A, w.nd * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
      if (c.g_dev) FFGP_HIP(hipMemcpyAsync(c.g_dev, w.g, w.nd * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    }
  }
  std::vector<int> st(F, 0);
  for (int f = 0; f < F; ++f) FFGP_HIP(hipMemcpyAsync(&st[f], W[f].st, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  FFGP_HIP(hipStreamSynchronize(h->stream));
  if (timed) stage_collect(h);
  int rc = 0, best = -1;
  for (int f = 0; f < F; ++f) {
    if (fail_step) fail_step[f] = st[f] - 1;
    if (st[f] && (best < 0 || st[f] < best)) {
      best = st[f];
      rc = 1 + f + FFGP_TRAIN_MAXF * (st[f] - 1);
    }
  }
  return rc;
}

}  // extern "C"
