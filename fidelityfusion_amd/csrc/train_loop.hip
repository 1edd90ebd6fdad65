// K training steps in one call, launch per stage: the loop around the likelihood drivers with Adam on the device, and the residual
// members' kernels.  (train.hip is the one-launch trainer this falls through to when every model is small.)  See include/ffgp.h.
#include <climits>
#include <cmath>
#include <memory>

#include "drivers.h"
#include "train_tile.h"

// ---- K training steps in ONE call -------------------------------------------------------------------------------------------
// The reference's hot loop (FidelityFusion_Models/ResGP.py:78-112: per fidelity 100-1000 iterations of zero_grad / loss =
// -negative_log_likelihood / backward / Adam step at N = 16 ... 500) costs one Python round trip, one autograd graph and one status
// read-back per iteration through the drop-in modules -- 0.28-0.32 ms at N <= 128, of which 0.125 ms is GPU work.  Here the whole
// loop is enqueued by one call: per step the likelihood + closed-form gradients on the raw parameters (the same launches as
// ffgp_nlml_fused_raw, or ONE launch for all models when they are small: ffgp_nlml_fused_small_batch's kernel) and one Adam
// kernel that updates the raw parameters IN PLACE on the device (torch.optim.Adam's arithmetic, operation for operation: lerp,
// mul + addcmul, bias corrections computed on the host with the C library's pow as Python does, sqrt / div / add eps, addcdiv) and
// stores the step's loss in the trace.  No host synchronisation inside the loop; the factorisation status is sticky and read once
// at the end (the first step whose Sigma was not positive definite; the parameters stop moving from that step on).
extern "C" __global__ void ffgp_adam_kernel(int F, ffgp_train_slot sl, const double* __restrict__ gbuf, double* __restrict__ state, long state_stride,
                                 double lr, double b1, double b2, double eps, double bc1, double bc2_sqrt, const double* __restrict__ loss,
                                 double* __restrict__ trace, long trace_stride, int step, int* __restrict__ info, int fold,
                                 const double* __restrict__ geff, ffgp_links lk, int lD, double lsc) {
  const int f = blockIdx.x;
  if (f >= F) return;
  const int i0 = info[0], i1 = info[1];
  const int bad = i0 | i1;
  if (fold) {      // (one model per call: this kernel also keeps the status words -- sticky first failure, current word cleared for the
    __syncthreads();   //  next step's factorisation -- two single-thread launches per step otherwise)
    if (threadIdx.x == 0) {
      if (i1 == 0 && i0 != 0) info[1] = i0;
      info[0] = 0;
    }
  }
  const int nw = sl.nw[f];
  const int npar = nw + 2 + (sl.rho[f] ? 1 : 0);      // (a residual member's rho is the last parameter; its gradient is in gbuf)
  if (threadIdx.x == 0) trace[(size_t)f * trace_stride + step] = bad ? __builtin_nan("") : loss[f];
  if (bad) return;
  const int i = threadIdx.x;
  if (i >= npar) return;
  double* par = (i < nw) ? sl.w[f] + i : (i == nw ? sl.amp[f] : (i == nw + 1 ? sl.dadd[f] : sl.rho[f]));
  double g;
  if (i == nw + 2) {
    g = gbuf[(size_t)f * FFGP_TRAIN_GSTRIDE + i];
  } else if (geff) {
    // (one model, blocked path: the gradients arrive with respect to the EFFECTIVE parameters [w (D) | amp | diag_add]; the links'
    //  chain rule -- ffgp_link_bwd's arithmetic -- is applied here instead of in a launch of its own)
    if (i < nw) {
      if (!lk.w_broadcast) {
        g = lsc * geff[i] * ffgp_link_der(lk.w_link, par[0], lk.w_c);
      } else {
        double sg = 0.0;
        for (int k = 0; k < lD; ++k) sg += geff[k];
        g = lsc * sg * ffgp_link_der(lk.w_link, par[0], lk.w_c);
      }
    } else if (i == nw) {
      g = lsc * geff[lD] * ffgp_link_der(lk.amp_link, par[0], lk.amp_c);
    } else {
      g = lsc * geff[lD + 1] * ffgp_link_der(lk.dadd_link, par[0], lk.dadd_c);
    }
  } else {
    g = gbuf[(size_t)f * FFGP_TRAIN_GSTRIDE + i];
  }
  double* m = state + (size_t)f * state_stride + i;
  double* v = m + npar;
  ffgp_adam_update(par, m, v, g, lr, b1, b2, eps, bc1, bc2_sqrt);
}

// residual members of the launch-per-stage loop (ffgp_train_residual_raw): per step their targets and diagonal extra are formed from rho
// before the likelihood call, and dloss/drho is reduced from its dloss/dY and dloss/ddiag_vec after it
struct ffgp_resid_slot {
  const double* rho[FFGP_TRAIN_MAXF];
  const double* yl[FFGP_TRAIN_MAXF];
  const double* yh[FFGP_TRAIN_MAXF];
  const double* vl[FFGP_TRAIN_MAXF];
  const double* vh[FFGP_TRAIN_MAXF];
  long vls[FFGP_TRAIN_MAXF], vhs[FFGP_TRAIN_MAXF];
  double* r[FFGP_TRAIN_MAXF];            // [n, d] targets
  double* dv[FFGP_TRAIN_MAXF];           // [n] |s|
  const double* gY[FFGP_TRAIN_MAXF];     // [n, d] dloss/dr
  const double* gdv[FFGP_TRAIN_MAXF];    // [n] dloss/ddvec
  double* rho_last[FFGP_TRAIN_MAXF];
  long nd[FFGP_TRAIN_MAXF];
  int n[FFGP_TRAIN_MAXF], nw[FFGP_TRAIN_MAXF];
};
// r = y_high - rho y_low, dvec = |v_high - rho v_low| (a product, then a difference: torch's rounding); rho_last = rho
extern "C" __global__ void ffgp_resid_form(ffgp_resid_slot rs) {
  const int f = blockIdx.y;
  if (!rs.rho[f]) return;
  const double rho = rs.rho[f][0];
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t < rs.nd[f]) rs.r[f][t] = __dsub_rn(rs.yh[f][t], __dmul_rn(rho, rs.yl[f][t]));
  if (rs.vl[f] && t < rs.n[f]) rs.dv[f][t] = fabs(__dsub_rn(rs.vh[f][t * rs.vhs[f]], __dmul_rn(rho, rs.vl[f][t * rs.vls[f]])));
  if (t == 0 && rs.rho_last[f]) rs.rho_last[f][0] = rho;
}
// gbuf slot nw + 2 <- dloss/drho = -sum gY .* y_low - sum_i gdv_i sgn(s_i) v_low,ii (one workgroup per member, fixed order)
extern "C" __global__ void ffgp_resid_grad(ffgp_resid_slot rs, double* __restrict__ gbuf) {
  const int f = blockIdx.x;
  if (!rs.rho[f]) return;
  __shared__ double part[256];
  const double rho = rs.rho[f][0];
  double x = 0.0;
  for (long t = threadIdx.x; t < rs.nd[f]; t += 256) x = __builtin_fma(rs.gY[f][t], rs.yl[f][t], x);
  if (rs.vl[f]) {
    for (int i = threadIdx.x; i < rs.n[f]; i += 256) {
      const double vl = rs.vl[f][(long)i * rs.vls[f]];
      const double s = __dsub_rn(rs.vh[f][(long)i * rs.vhs[f]], __dmul_rn(rho, vl));
      x = __builtin_fma(rs.gdv[f][i], (s > 0.0) ? vl : ((s < 0.0) ? -vl : 0.0), x);      // (sgn(0) = 0: torch's abs backward)
    }
  }
  part[threadIdx.x] = x;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) gbuf[(size_t)f * FFGP_TRAIN_GSTRIDE + rs.nw[f] + 2] = -part[0];
}

// CAR members of the launch-per-stage loop (ffgp_train_car_raw): per step their targets r = y_high - exp(b) y_low and the effective
// amplitude link(amp_raw) * s are formed before the likelihood call -- which reads that amplitude under the identity link -- and
// dloss/db is reduced and the chain rule for amp, l_z, sigma_z applied after it
struct ffgp_car_slot {
  double* b[FFGP_TRAIN_MAXF];            // null: a plain member
  double* zls[FFGP_TRAIN_MAXF];
  double* zamp[FFGP_TRAIN_MAXF];
  const double* amp_raw[FFGP_TRAIN_MAXF];
  const float* z1[FFGP_TRAIN_MAXF];
  const float* z2[FFGP_TRAIN_MAXF];
  const double* z1d[FFGP_TRAIN_MAXF];    // fp64 draws (then z1 / z2 are not read)
  const double* z2d[FFGP_TRAIN_MAXF];
  const double* yl[FFGP_TRAIN_MAXF];
  const double* yh[FFGP_TRAIN_MAXF];
  double* r[FFGP_TRAIN_MAXF];            // [n, d] targets
  const double* gY[FFGP_TRAIN_MAXF];     // [n, d] dloss/dr
  double* sv[FFGP_TRAIN_MAXF];           // [8] link(amp_raw) * s (the likelihood's amplitude) | s, ds/db, ds/dl_z, ds/dsigma_z | exp(b)
  double* b_last[FFGP_TRAIN_MAXF];
  double zeps[FFGP_TRAIN_MAXF], lf[FFGP_TRAIN_MAXF], hf[FFGP_TRAIN_MAXF], amp_c[FFGP_TRAIN_MAXF];
  long nd[FFGP_TRAIN_MAXF];
  int nz[FFGP_TRAIN_MAXF], nw[FFGP_TRAIN_MAXF], amp_link[FFGP_TRAIN_MAXF];
};
extern "C" __global__ void ffgp_car_form(ffgp_car_slot cs) {
  const int f = blockIdx.y;
  if (!cs.b[f]) return;
  __shared__ double zs[256];      // z1 [128] | z2 [128]: fp32 draws widened, or fp64 draws
  const double b = cs.b[f][0];
  const double eb = exp(b);
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t < cs.nd[f]) cs.r[f][t] = __dsub_rn(cs.yh[f][t], __dmul_rn(eb, cs.yl[f][t]));
  if (blockIdx.x != 0) return;
  {
    const int k = threadIdx.x & 127, hi = threadIdx.x >> 7;
    double z = 0.0;
    if (k < cs.nz[f]) z = cs.z1d[f] ? (hi ? cs.z2d[f][k] : cs.z1d[f][k]) : (double)(hi ? cs.z2[f][k] : cs.z1[f][k]);
    zs[threadIdx.x] = z;
  }
  __syncthreads();
  if (threadIdx.x < 64) {      // (one wave: the fidelity integral, train_tile.h)
    double o[4];
    car_scale_wave(b, cs.zls[f][0], cs.zamp[f][0], cs.zeps[f], zs, zs + 128, cs.z1d[f] == nullptr, cs.nz[f], cs.lf[f], cs.hf[f],
                   (int)threadIdx.x, o);
    if (threadIdx.x == 0) {
      double* sv = cs.sv[f];
      sv[0] = ffgp_link_val(cs.amp_link[f], cs.amp_raw[f][0], cs.amp_c[f]) * o[0];
      sv[1] = o[0]; sv[2] = o[1]; sv[3] = o[2]; sv[4] = o[3];
      sv[5] = eb;
      if (cs.b_last[f]) cs.b_last[f][0] = b;
    }
  }
}
// gbuf slot nw holds T = dloss/d(effective amplitude) (the likelihood ran under the identity link; the output scale is inside):
// slots nw, nw + 2 .. nw + 4 <- the gradients of amp_raw, b, l_z, sigma_z (one workgroup per member, fixed order)
extern "C" __global__ void ffgp_car_grad(ffgp_car_slot cs, double* __restrict__ gbuf) {
  const int f = blockIdx.x;
  if (!cs.b[f]) return;
  __shared__ double part[256];
  double x = 0.0;
  for (long t = threadIdx.x; t < cs.nd[f]; t += 256) x = __builtin_fma(cs.gY[f][t], cs.yl[f][t], x);
  part[threadIdx.x] = x;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double* g = gbuf + (size_t)f * FFGP_TRAIN_GSTRIDE + cs.nw[f];
    const double* sv = cs.sv[f];
    const double T = g[0], ar = cs.amp_raw[f][0];
    const double dls = T * ffgp_link_val(cs.amp_link[f], ar, cs.amp_c[f]);
    g[0] = T * ffgp_link_der(cs.amp_link[f], ar, cs.amp_c[f]) * sv[1];
    g[2] = dls * sv[2] - sv[5] * part[0];
    g[3] = dls * sv[3];
    g[4] = dls * sv[4];
  }
}
// ffgp_adam_kernel for a call with CAR members: raw gradients from gbuf, nw + 5 parameters for a CAR member (w, amp, diag_add, b, l_z,
// sigma_z), nw + 2 for a plain one; the status words are kept by the likelihood's own epilogue
extern "C" __global__ void ffgp_adam_car_kernel(int F, ffgp_train_slot sl, ffgp_car_slot cs, const double* __restrict__ gbuf,
                                                double* __restrict__ state, long state_stride, double lr, double b1, double b2, double eps,
                                                double bc1, double bc2_sqrt, const double* __restrict__ loss, double* __restrict__ trace,
                                                long trace_stride, int step, const int* __restrict__ info) {
  const int f = blockIdx.x;
  if (f >= F) return;
  const int bad = info[0] | info[1];
  const int nw = sl.nw[f];
  const int npar = nw + 2 + (cs.b[f] ? 3 : 0);
  if (threadIdx.x == 0) trace[(size_t)f * trace_stride + step] = bad ? __builtin_nan("") : loss[f];
  if (bad) return;
  const int i = threadIdx.x;
  if (i >= npar) return;
  double* par = (i < nw) ? sl.w[f] + i
                         : (i == nw ? sl.amp[f] : (i == nw + 1 ? sl.dadd[f] : (i == nw + 2 ? cs.b[f] : (i == nw + 3 ? cs.zls[f] : cs.zamp[f]))));
  double* m = state + (size_t)f * state_stride + i;
  ffgp_adam_update(par, m, m + npar, gbuf[(size_t)f * FFGP_TRAIN_GSTRIDE + i], lr, b1, b2, eps, bc1, bc2_sqrt);
}

// tensor-linear members of the launch-per-stage loop (ffgp_train_tlin_raw; train_CIGAR's fidelities above 0, CIGAR.py:116-133): per step
// their targets R = y_high - y_low V^T are formed before the likelihood call and dloss/dV = -(dloss/dR)^T y_low after it; V's h l entries
// are Adam parameters nw + 2 ... of the member.  Members with gemm[f] set run both products on the fp64 GEMM (train_impl enqueues them:
// T = y_low V^T into the gY buffer, which is dead until the likelihood writes it), the others in the plain kernels below.
struct ffgp_tlin_slot {
  double* V[FFGP_TRAIN_MAXF];            // null: a plain member
  long rs[FFGP_TRAIN_MAXF], cs[FFGP_TRAIN_MAXF];
  const double* yl[FFGP_TRAIN_MAXF];     // [n, l]
  const double* yh[FFGP_TRAIN_MAXF];     // [n, h]
  double* r[FFGP_TRAIN_MAXF];            // [n, h] targets
  double* gY[FFGP_TRAIN_MAXF];           // [n, h] dloss/dR (GEMM members: y_low V^T before the likelihood call)
  double* dV[FFGP_TRAIN_MAXF];           // [h, l] row-major
  double* V_last[FFGP_TRAIN_MAXF];       // optional [h, l] row-major
  int n[FFGP_TRAIN_MAXF], l[FFGP_TRAIN_MAXF], h[FFGP_TRAIN_MAXF], gemm[FFGP_TRAIN_MAXF];
};
// R[i, a] = y_high[i, a] - sum_b y_low[i, b] V[a, b] (b ascending, one chain of fused multiply-adds, then the difference); V_last = V
extern "C" __global__ void ffgp_tlin_form(ffgp_tlin_slot ts) {
  const int f = blockIdx.y;
  if (!ts.V[f]) return;
  const int l = ts.l[f], h = ts.h[f];
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t < (long)ts.n[f] * h) {
    if (ts.gemm[f]) {
      ts.r[f][t] = __dsub_rn(ts.yh[f][t], ts.gY[f][t]);
    } else {
      const long i = t / h;
      const double* yl = ts.yl[f] + i * l;
      const double* v = ts.V[f] + (t - i * h) * ts.rs[f];
      double s = 0.0;
      for (int b = 0; b < l; ++b) s = __builtin_fma(yl[b], v[b * ts.cs[f]], s);
      ts.r[f][t] = __dsub_rn(ts.yh[f][t], s);
    }
  }
  if (ts.V_last[f] && t < (long)h * l) ts.V_last[f][t] = ts.V[f][(t / l) * ts.rs[f] + (t % l) * ts.cs[f]];
}
// dV[a, b] = -sum_i gY[i, a] y_low[i, b], i ascending: one thread per entry (the members below the GEMM switch)
extern "C" __global__ void ffgp_tlin_grad(ffgp_tlin_slot ts) {
  const int f = blockIdx.y;
  if (!ts.V[f] || ts.gemm[f]) return;
  const int l = ts.l[f], h = ts.h[f], n = ts.n[f];
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= h * l) return;
  const double* g = ts.gY[f] + t / l;
  const double* yl = ts.yl[f] + t % l;
  double s = 0.0;
  for (int i = 0; i < n; ++i) s = __builtin_fma(g[(long)i * h], yl[(long)i * l], s);
  ts.dV[f][t] = -s;
}
// Adam for a call with tensor-linear members: block x = 0 of member f moves w, amp, diag_add (raw gradients from gbuf) and stores the loss,
// blocks x >= 1 move V's entries 256 each through V's strides; the moments of parameter q at state[q] and state[P + q], P = nw + 2 + h l.
// The status words are kept by the likelihood's own epilogue.
extern "C" __global__ void ffgp_adam_tlin_kernel(ffgp_train_slot sl, ffgp_tlin_slot ts, const double* __restrict__ gbuf, double* __restrict__ state,
                                                 long state_stride, double lr, double b1, double b2, double eps, double bc1, double bc2_sqrt,
                                                 const double* __restrict__ loss, double* __restrict__ trace, long trace_stride, int step,
                                                 const int* __restrict__ info) {
  const int f = blockIdx.y;
  const int bad = info[0] | info[1];
  const int nw = sl.nw[f];
  const long hl = ts.V[f] ? (long)ts.h[f] * ts.l[f] : 0;
  const long npar = nw + 2 + hl;
  double* m0 = state + (size_t)f * state_stride;
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) trace[(size_t)f * trace_stride + step] = bad ? __builtin_nan("") : loss[f];
    if (bad) return;
    const int i = threadIdx.x;
    if (i >= nw + 2) return;
    double* par = (i < nw) ? sl.w[f] + i : (i == nw ? sl.amp[f] : sl.dadd[f]);
    ffgp_adam_update(par, m0 + i, m0 + npar + i, gbuf[(size_t)f * FFGP_TRAIN_GSTRIDE + i], lr, b1, b2, eps, bc1, bc2_sqrt);
    return;
  }
  if (bad) return;
  const long e = (long)(blockIdx.x - 1) * 256 + threadIdx.x;
  if (e >= hl) return;
  const int l = ts.l[f];
  double* par = ts.V[f] + (e / l) * ts.rs[f] + (e % l) * ts.cs[f];
  double* m = m0 + nw + 2 + e;
  ffgp_adam_update(par, m, m + npar, ts.dV[f][e], lr, b1, b2, eps, bc1, bc2_sqrt);
}

static int train_impl(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* l, const ffgp_residual* r, int steps,
                      const ffgp_adam* opt, double* state_dev, long state_stride, long step0, double* trace_dev, long trace_stride,
                      const ffgp_car_link* cr = nullptr, const ffgp_tlin_link* tl = nullptr) {
  if (!ffgp_train_args_ok(h, p, l, opt, state_dev, trace_dev, F, steps, step0, trace_stride)) return FFGP_ERR_ARG;
  ffgp_train_slot sl;
  bool all_small = true, any_res = false, any_car = false, any_lin = false;
  for (int f = 0; f < F; ++f) {
    const ffgp_problem& q = p[f];
    if (!q.w_dev || !q.amp_dev || !q.diag_add_dev || q.cov_dev || q.pair || q.tree || q.D <= 0 || q.D > 128 || q.n <= 0 || q.d <= 0) return FFGP_ERR_ARG;
    const bool res = r && r[f].rho_dev;
    if (res && (!r[f].y_low_dev || !r[f].y_high_dev || !q.X_dev || (!r[f].v_low_dev) != (!r[f].v_high_dev) ||
                (r[f].v_low_dev && (r[f].v_low_stride < 0 || r[f].v_high_stride < 0))))
      return FFGP_ERR_ARG;
    const bool car = cr && cr[f].b_dev;
    if (car && (r || !cr[f].zls_dev || !cr[f].zamp_dev || (!cr[f].z1d_dev) != (!cr[f].z2d_dev) ||
                (!cr[f].z1d_dev && (!cr[f].z1_dev || !cr[f].z2_dev)) || cr[f].nz <= 0 || cr[f].nz > 128 ||
                !cr[f].y_low_dev || !cr[f].y_high_dev || !q.X_dev))
      return FFGP_ERR_ARG;
    any_car = any_car || car;
    const bool lin = tl && tl[f].V_dev;
    if (lin && (r || cr || !tl[f].y_low_dev || !tl[f].y_high_dev || !q.X_dev || tl[f].l < 1 || tl[f].l > q.d || tl[f].V_row_stride < 0 ||
                tl[f].V_col_stride < 0 || q.ll_variant != FFGP_LL_V1))
      return FFGP_ERR_ARG;
    any_lin = any_lin || lin;
    const int nw = l[f].w_broadcast ? 1 : q.D;
    if (state_stride < 2 * (nw + 2 + (res ? 1 : 0) + (car ? 3 : 0) + (lin ? (long)q.d * tl[f].l : 0L))) return FFGP_ERR_ARG;
    sl.w[f] = const_cast<double*>(q.w_dev);
    sl.amp[f] = const_cast<double*>(q.amp_dev);
    sl.dadd[f] = const_cast<double*>(q.diag_add_dev);
    sl.rho[f] = res ? r[f].rho_dev : nullptr;
    sl.nw[f] = nw;
    any_res = any_res || res;
  }
  FFGP_HIP(hipSetDevice(h->device));
  {   // every model small enough for one workgroup: the whole loop is ONE launch (train.hip)
    bool persist = true;
    for (int f = 0; f < F && persist; ++f)
      persist = ffgp_train_persist_ok(h, p + f, l + f, r ? r + f : nullptr, cr ? cr + f : nullptr, tl ? tl + f : nullptr);
    if (persist) return ffgp_train_persist(h, F, p, l, steps, opt, state_dev, state_stride, step0, trace_dev, trace_stride, r, cr, tl);
  }
  if (!h->train_g) {
    FFGP_HIP(hipMalloc(&h->train_g, (size_t)FFGP_TRAIN_MAXF * (FFGP_TRAIN_GSTRIDE + 1) * sizeof(double)));
  }
  double* gbuf = h->train_g;
  double* loss = h->train_g + (size_t)FFGP_TRAIN_MAXF * FFGP_TRAIN_GSTRIDE;
  std::vector<ffgp_grads> g(F);
  std::vector<ffgp_links> lk(l, l + F);
  std::vector<ffgp_problem> pq(p, p + F);      // (residual members: targets and diagonal extra in the call's own buffers)
  ffgp_resid_slot rs;
  memset(&rs, 0, sizeof(rs));
  double* rbuf = nullptr;
  std::unique_ptr<double, hipError_t (*)(void*)> rbuf_owner(nullptr, hipFree);      // frees rbuf on every way out, after its synchronisation
  long rmax = 0;
  if (any_res) {      // per residual member [r (n d) | dvec (n) | dloss/dr (n d) | dloss/ddvec (n)], freed when the call returns
    size_t tot = 0;
    for (int f = 0; f < F; ++f)
      if (sl.rho[f]) tot += 2 * ((size_t)p[f].n * p[f].d + p[f].n);
    FFGP_HIP(hipMalloc(&rbuf, tot * sizeof(double)));
    rbuf_owner.reset(rbuf);
    size_t off = 0;
    for (int f = 0; f < F; ++f) {
      if (!sl.rho[f]) continue;
      const long n = p[f].n, nd = n * p[f].d;
      rs.rho[f] = sl.rho[f];
      rs.yl[f] = r[f].y_low_dev; rs.yh[f] = r[f].y_high_dev;
      rs.vl[f] = r[f].v_low_dev; rs.vh[f] = r[f].v_high_dev; rs.vls[f] = r[f].v_low_stride; rs.vhs[f] = r[f].v_high_stride;
      rs.r[f] = rbuf + off; rs.dv[f] = rs.r[f] + nd;
      rs.gY[f] = rs.dv[f] + n; rs.gdv[f] = rs.gY[f] + nd;
      rs.rho_last[f] = r[f].rho_last_dev;
      rs.nd[f] = nd; rs.n[f] = (int)n; rs.nw[f] = sl.nw[f];
      off += 2 * (nd + n);
      rmax = std::max(rmax, std::max(nd, n));
      pq[f].Y_dev = rs.r[f];
      pq[f].diag_vec_dev = rs.vl[f] ? rs.dv[f] : nullptr;
      pq[f].diag_stride = 1;
    }
  }
  ffgp_car_slot cs;
  memset(&cs, 0, sizeof(cs));
  if (any_car) {      // per CAR member [r (n d) | dloss/dr (n d) | sv (8)], freed when the call returns
    size_t tot = 0;
    for (int f = 0; f < F; ++f)
      if (cr[f].b_dev) tot += 2 * (size_t)p[f].n * p[f].d + 8;
    FFGP_HIP(hipMalloc(&rbuf, tot * sizeof(double)));
    rbuf_owner.reset(rbuf);
    size_t off = 0;
    for (int f = 0; f < F; ++f) {
      if (!cr[f].b_dev) continue;
      const long nd = (long)p[f].n * p[f].d;
      cs.b[f] = cr[f].b_dev; cs.zls[f] = cr[f].zls_dev; cs.zamp[f] = cr[f].zamp_dev;
      cs.amp_raw[f] = p[f].amp_dev; cs.amp_link[f] = l[f].amp_link; cs.amp_c[f] = l[f].amp_c;
      cs.z1[f] = cr[f].z1_dev; cs.z2[f] = cr[f].z2_dev; cs.nz[f] = cr[f].nz;
      cs.z1d[f] = cr[f].z1d_dev; cs.z2d[f] = cr[f].z2d_dev;
      cs.zeps[f] = cr[f].zeps; cs.lf[f] = cr[f].lf; cs.hf[f] = cr[f].hf;
      cs.yl[f] = cr[f].y_low_dev; cs.yh[f] = cr[f].y_high_dev;
      cs.r[f] = rbuf + off; cs.gY[f] = cs.r[f] + nd; cs.sv[f] = cs.r[f] + 2 * nd;
      cs.b_last[f] = cr[f].b_last_dev;
      cs.nd[f] = nd; cs.nw[f] = sl.nw[f];
      off += 2 * nd + 8;
      rmax = std::max(rmax, nd);
      pq[f].Y_dev = cs.r[f];
      pq[f].amp_dev = cs.sv[f];          // link(amp_raw) * s, read under the identity link: its gradient slot receives T
      lk[f].amp_link = FFGP_LINK_ID;
      lk[f].amp_c = 0.0;
    }
  }
  ffgp_tlin_slot ts;
  memset(&ts, 0, sizeof(ts));
  long vmax = 0;
  bool lin_plain = false;
  if (any_lin) {      // per tensor-linear member [R (n h) | dloss/dR (n h) | dV (h l)], each on a 16-byte boundary, freed when the call returns
    auto even = [](size_t x) { return (x + 1) & ~(size_t)1; };
    size_t tot = 0;
    for (int f = 0; f < F; ++f)
      if (tl[f].V_dev) tot += 2 * even((size_t)p[f].n * p[f].d) + even((size_t)p[f].d * tl[f].l);
    FFGP_HIP(hipMalloc(&rbuf, tot * sizeof(double)));
    rbuf_owner.reset(rbuf);
    size_t off = 0;
    for (int f = 0; f < F; ++f) {
      if (!tl[f].V_dev) continue;
      const long n = p[f].n, hh = p[f].d, ll = tl[f].l, nh = n * hh;
      ts.V[f] = tl[f].V_dev;
      ts.rs[f] = tl[f].V_row_stride; ts.cs[f] = tl[f].V_col_stride;
      if (ts.rs[f] == 0 && ts.cs[f] == 0) { ts.rs[f] = ll; ts.cs[f] = 1; }
      ts.yl[f] = tl[f].y_low_dev; ts.yh[f] = tl[f].y_high_dev;
      ts.r[f] = rbuf + off; ts.gY[f] = ts.r[f] + even(nh); ts.dV[f] = ts.gY[f] + even(nh);
      ts.V_last[f] = tl[f].V_last_dev;
      ts.n[f] = (int)n; ts.l[f] = (int)ll; ts.h[f] = (int)hh;
      // the fp64 GEMM reads V K-major (unit column stride) or MN-major (unit row stride: the bilinear initialisation's transposed view)
      ts.gemm[f] = (h->tlin_gemm_min > 0 && (double)n * ll * hh >= (double)h->tlin_gemm_min && (ts.cs[f] == 1 || ts.rs[f] == 1) &&
                    std::max(ts.rs[f], ts.cs[f]) <= INT_MAX) ? 1 : 0;
      lin_plain = lin_plain || !ts.gemm[f];
      off += 2 * even(nh) + even(hh * ll);
      rmax = std::max(rmax, std::max(nh, hh * ll));
      vmax = std::max(vmax, hh * ll);
      pq[f].Y_dev = ts.r[f];
    }
  }
  for (int f = 0; f < F; ++f) {
    memset(&g[f], 0, sizeof(ffgp_grads));
    g[f].g_w_dev = gbuf + (size_t)f * FFGP_TRAIN_GSTRIDE;
    g[f].g_amp_dev = g[f].g_w_dev + sl.nw[f];
    g[f].g_diag_add_dev = g[f].g_amp_dev + 1;
    if (sl.rho[f]) {
      g[f].g_Y_dev = const_cast<double*>(rs.gY[f]);
      if (rs.vl[f]) g[f].g_diag_vec_dev = const_cast<double*>(rs.gdv[f]);
    }
    if (cs.b[f]) g[f].g_Y_dev = const_cast<double*>(cs.gY[f]);
    if (ts.V[f]) g[f].g_Y_dev = ts.gY[f];
    all_small = all_small && ffgp_small_batch_ok(&pq[f], &g[f]);
  }
  p = pq.data();
  // the sticky status word starts clean: a failure of an EARLIER call on this handle is that call's to report
  FFGP_CHECK(ffgp_zero_async(h, h->d_info, 2 * sizeof(int)));
  // (the one-kernel paths -- n <= 40, or option small_finish -- apply the links inside their kernel and write raw gradients)
  const bool one_kernel = ffgp_small_ok(h, p, &g[0]) || ffgp_small2_ok(h, p, &g[0]);
  h->defer_info_copy = 1;      // (the per-call read-back of the status word: once, after the loop)
  h->fold_info = (F == 1 && !any_car && !any_lin) ? 1 : 0;   // one model: the Adam kernel clears / accumulates the status words (see ffgp_adam_kernel;
                                                  // a call with CAR members leaves them to the likelihood's epilogue)
  int lrc = FFGP_OK;
  for (int k = 0; k < steps && lrc == FFGP_OK; ++k) {
    if (any_res) hipLaunchKernelGGL(ffgp_resid_form, dim3((unsigned)((rmax + 255) / 256), F), dim3(256), 0, h->stream, rs);
    if (any_car) hipLaunchKernelGGL(ffgp_car_form, dim3((unsigned)((rmax + 255) / 256), F), dim3(256), 0, h->stream, cs);
    if (any_lin) {
      for (int f = 0; f < F && lrc == FFGP_OK; ++f)      // T = y_low V^T [n, h] into the gY buffer
        if (ts.gemm[f])
          lrc = ffgp_gemm_launch(h, OP_KMAJOR, ts.cs[f] == 1 ? OP_KMAJOR : OP_MNMAJOR, TILES_FULL, 0, ts.yl[f], ts.l[f], ts.V[f],
                                 (int)(ts.cs[f] == 1 ? ts.rs[f] : ts.cs[f]), ts.gY[f], ts.h[f], ts.n[f], ts.h[f], ts.l[f], 1.0, 0.0);
      if (lrc != FFGP_OK) break;
      hipLaunchKernelGGL(ffgp_tlin_form, dim3((unsigned)((rmax + 255) / 256), F), dim3(256), 0, h->stream, ts);
    }
    if (all_small && F > 1) {
      if ((lrc = ffgp_zero_async(h, h->d_info, sizeof(int))) != FFGP_OK) break;
      if ((lrc = ffgp_small_batch_enqueue(h, F, p, lk.data(), loss, g.data())) != FFGP_OK) break;
      if ((lrc = ffgp_finish_info(h)) != FFGP_OK) break;      // (several models: fold_info is off, the read-back deferred -- the sticky word's launch alone)
    } else {
      for (int f = 0; f < F && lrc == FFGP_OK; ++f) lrc = ffgp_nlml_fused_raw_async(h, p + f, &lk[f], loss + f, &g[f]);
      if (lrc != FFGP_OK) break;
    }
    if (any_res) hipLaunchKernelGGL(ffgp_resid_grad, dim3(F), dim3(256), 0, h->stream, rs, gbuf);
    double bc1, bc2_sqrt;
    ffgp_adam_bc(opt, step0, k, &bc1, &bc2_sqrt);
    if (any_lin) {
      for (int f = 0; f < F && lrc == FFGP_OK; ++f)      // dV = -gY^T y_low [h, l]
        if (ts.gemm[f])
          lrc = ffgp_gemm_launch(h, OP_MNMAJOR, OP_MNMAJOR, TILES_FULL, 0, ts.gY[f], ts.h[f], ts.yl[f], ts.l[f], ts.dV[f], ts.l[f], ts.h[f],
                                 ts.l[f], ts.n[f], -1.0, 0.0);
      if (lrc != FFGP_OK) break;
      if (lin_plain) hipLaunchKernelGGL(ffgp_tlin_grad, dim3((unsigned)((vmax + 255) / 256), F), dim3(256), 0, h->stream, ts);
      hipLaunchKernelGGL(ffgp_adam_tlin_kernel, dim3((unsigned)(1 + (vmax + 255) / 256), F), dim3(256), 0, h->stream, sl, ts, gbuf, state_dev,
                         state_stride, opt->lr, opt->beta1, opt->beta2, opt->eps, bc1, bc2_sqrt, loss, trace_dev, trace_stride, k, h->d_info);
      continue;
    }
    if (any_car) {
      hipLaunchKernelGGL(ffgp_car_grad, dim3(F), dim3(256), 0, h->stream, cs, gbuf);
      hipLaunchKernelGGL(ffgp_adam_car_kernel, dim3(F), dim3(192), 0, h->stream, F, sl, cs, gbuf, state_dev, state_stride, opt->lr, opt->beta1,
                         opt->beta2, opt->eps, bc1, bc2_sqrt, loss, trace_dev, trace_stride, k, h->d_info);
      continue;
    }
    hipLaunchKernelGGL(ffgp_adam_kernel, dim3(F), dim3(192), 0, h->stream, F, sl, gbuf, state_dev, state_stride, opt->lr, opt->beta1,
                       opt->beta2, opt->eps, bc1, bc2_sqrt, loss, trace_dev, trace_stride, k, h->d_info, h->fold_info,
                       (h->fold_info && !one_kernel) ? h->d_link + 256 : (const double*)nullptr, lk[0], p[0].D,
                       (lk[0].out_scale == 0.0) ? 1.0 : lk[0].out_scale);
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

extern "C" {

int ffgp_train_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* l, int steps, const ffgp_adam* opt, double* state_dev,
                   long state_stride, long step0, double* trace_dev, long trace_stride) {
  return train_impl(h, F, p, l, nullptr, steps, opt, state_dev, state_stride, step0, trace_dev, trace_stride);
}

int ffgp_train_residual_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* l, const ffgp_residual* r, int steps,
                            const ffgp_adam* opt, double* state_dev, long state_stride, long step0, double* trace_dev, long trace_stride) {
  if (!r) return FFGP_ERR_ARG;
  return train_impl(h, F, p, l, r, steps, opt, state_dev, state_stride, step0, trace_dev, trace_stride);
}

int ffgp_train_tlin_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* l, const ffgp_tlin_link* t, int steps,
                        const ffgp_adam* opt, double* state_dev, long state_stride, long step0, double* trace_dev, long trace_stride) {
  if (!t) return FFGP_ERR_ARG;
  return train_impl(h, F, p, l, nullptr, steps, opt, state_dev, state_stride, step0, trace_dev, trace_stride, nullptr, t);
}

int ffgp_train_car_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* l, const ffgp_car_link* c, int steps,
                       const ffgp_adam* opt, double* state_dev, long state_stride, long step0, double* trace_dev, long trace_stride) {
  if (!c) return FFGP_ERR_ARG;
  return train_impl(h, F, p, l, nullptr, steps, opt, state_dev, state_stride, step0, trace_dev, trace_stride, c);
}

}  // extern "C"
