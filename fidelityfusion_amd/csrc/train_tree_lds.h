// K Adam steps of F composed-kernel models -- SumKernel / ProductKernel trees of 2-4 leaves (ffgp_ktree) -- in ONE launch: the step loop
// ttl_body<DM, V2, RESID, MODEL>, its LDS layout and the member description (ttl_describe) of ffgp_train_tree_lds_raw (train_tree_lds.hip:
// V1, plain members) and ffgp_train_tree_lds_res_raw (train_tree_lds_res.hip: V2 and residual members, added here under `if constexpr`).
// Six instantiations in those two units; this is their one text.  The reference trains SumKernel(LinearKernel, MaternKernel) at N = 16 ... 128
// (Bayesian_optimization/cigp.py:119-124: 300 Adam steps; con_mace_acq_demo.py:95-96: 100 per BO iteration; GaussianProcess/cigp_v10.py:81),
// and ffgp_train_tree_raw (train_tree.hip) pays a launch chain per step at every size.  Here one PERSISTENT workgroup per model
// (gridDim.x = models, 512 threads) runs every step inside the kernel, as tr_body<DM, true> of train.hip does for one radial kernel;
// the phases between the assembly and the gradient pass ARE train.hip's (train_tile.h).  Per step:
//
//   Sigma  straight into the LDS block image (lower block triangle, identity beyond n).  X sits in LDS ONCE, as given (no per-leaf
//          scaled copy: four do not fit, and a difference of given coordinates is formed exactly where a difference of scaled ones is
//          not -- nor is it shifted by the first point as train.hip's scaled image is: that only protects scaled differences); each leaf
//          keeps w_e^2 [16] and, a linear leaf, its centre [16].  Per entry and leaf the argument
//              radial:  sum_k w_ek^2 (x_ik - x_jk)^2, clamped with the leaf's clamp_min        linear:  sum_k w_ek^2 (x_ik - c_k)(x_jk - c_k)
//          then amp_e phi_e, then the tree, node by node as pair.hip rounds it (tree_ops.h); diag_add, then diag_vec, on the diagonal.
//   ->     train_tile.h: blocked Cholesky and inverse, Gamma = L^-1 Y, A = L^-T Gamma.
//   ->     gradient pass 1: Sigma^-1 block by block in the accumulators, G = d/2 Sigma^-1 - 1/2 A A^T; per entry the leaves are EVALUATED
//          AGAIN and the tree's reverse sweep gives every leaf's upstream weight.  Out of it: tr G, every leaf's amplitude sum, and the
//          entry's weight for each leaf's per-dimension sums, W_e = sym G dk/dv_e amp_e (-2 phi_e') (radial, 0 on the clamp) or
//          sym G dk/dv_e amp_e (linear), parked in this model's global scratch [leaf][36][4][64] (L2-resident; written and read by the
//          same lane).
//          (Why the leaves are evaluated again instead of parked by the assembly as train.hip's kbuf parks them: the derivative
//           -2 phi' needs the clamped argument and its own exponential whatever is parked -- train.hip's non-SE profiles evaluate it
//           afresh too -- so parking would save one of two profile evaluations for two more global round trips per leaf and entry, and
//           the scratch is wanted for the weights.)
//   ->     gradient pass 2, LEAF BY LEAF: sum_entries W_e (x_ik - x_jk)^2 (radial), W_e (x_ik - c_k)(x_jk - c_k) and
//          W_e ((x_ik - c_k) + (x_jk - c_k)) (linear: w and centre) -- one leaf's D (+ D) accumulators live at a time.
//   ->     ONE workgroup reduction of all of it (the per-wave partial sums use Gamma's image: it is dead behind A), the links' chain rule
//          (ffgp_link_der; a broadcast length scale: the D effective gradients summed in index order first) and torch.optim.Adam's
//          update (ffgp_adam_update) on raw parameters and moments that live in LDS for the whole call; the loss before the update goes
//          to the trace.  With p = (x - c) w these are pair.hip's gradients: g_w = (linear ? 2 : -1) w_k sum, g_c = -w_k^2 sum.
// A Sigma that is not positive definite stops THAT model at that step (its status word, NaN in its trace from there on, parameters
// and moments as they were when the step began); the other models of the launch train on -- train.hip's rule.
// Covers n <= 128, D <= 16, d <= 16, diag_add and diag_vec, leaves SE/ARD, Matern 1/2, 3/2, 5/2 and linear; the V2 likelihood and
// residual members (rho trained as one more parameter) where the template's V2 / RESID are set -- described at ttl_body.
// HOST side: the scaffold of train_host.h, shared with train.hip (block and pinned mirror on the handle, bias corrections, loop arguments,
// dispatch, launch, status epilogue); this file adds the member description (ttl_describe), each entry its one table.  LDS: train_tile.h's
// head, then this kernel's tail.
#pragma once
#include "train_host.h"
#include "tree_ops.h"

#define TTL_L FFGP_TREE_LEAVES
#define TTL_PMAX (TTL_L * (2 * TR_D + 1) + 1)      // raw parameters of a model at most: four linear leaves with D = 16 and trained centres
#define TTL_PPAD 136
#define TTL_NSC 7                                  // scalars of the step's reduction: ss, tr G, log-det, s_amp[4]
#define TTL_RW(DM) (TTL_NSC + TTL_L * 2 * (DM))    // ... then per leaf: w-sums [DM] | centre-sums [DM]
#define TTL_WBUF (TTL_L * NBLK_LOWER * 256)        // doubles of global scratch per model

struct TtlLeaf {
  double* w; double* amp;                // RAW parameters, updated in place when the kernel ends
  double* cen;                           // the centre of a linear leaf: trained (cen_train), given, or null (the origin)
  double w_c, amp_c, clamp, rinv;
  int w_link, amp_link, nw, cen_train, kfun, poff;      // nw: raw length scales (1 = broadcast); poff: the leaf's first raw parameter
};
struct TtlModel {
  int n, D, d, P;                        // P raw parameters: leaf by leaf (w, amp, trained centre), then diag_add
  int nl, shape, op[3];                  // the tree (tree_ops.h)
  int dadd_link;
  const double* X; const double* Y;
  const double* diag_vec; long diag_stride;
  double* dadd;
  double dadd_c, oscale, pi_const;
  double* state;                         // [exp_avg (P) | exp_avg_sq (P)]
  double* trace;                         // [steps]
  double* wbuf;                          // [TTL_WBUF] the entries' per-leaf weights, pass 1 -> pass 2 of the same step
  TtlLeaf k[TTL_L];
  // (a plain member has no residual link: what ttl_body's RESID branches ask of a MODEL)
  __device__ double y_low_at(int) const { return 0.0; }
  __device__ double y_high_at(int) const { return 0.0; }
  __device__ double* rho_last_ptr() const { return nullptr; }
};
// a member of ffgp_train_tree_lds_res_raw: rho null = a plain member
struct TtlResModel : TtlModel {
  double* rho;                           // [1] raw rho: parameter P of a residual member, state [exp_avg (P + 1) | exp_avg_sq (P + 1)]
  const double* y_low; const double* y_high;            // [n, d]
  const double* v_low; const double* v_high;            // entry i at [i * stride]; null: the subset form
  long v_low_stride, v_high_stride;
  double* rho_last;                      // optional [1]
  __device__ double y_low_at(int t) const { return y_low[t]; }
  __device__ double y_high_at(int t) const { return y_high[t]; }
  __device__ double* rho_last_ptr() const { return rho_last; }
};
struct TtlCommon : TrainLoop {};         // (the loop's arguments under the name the kernel's symbol was built with)
struct TtlTree {
  int nl, shape, op[3];
};

// LDS (doubles): the shared head of train_tile.h (S | Xs | Ym, Gam, Am | piv | dvec) | per leaf wv, w2, cen [4][16] each and
// (amp, clamp, 1 / kparam, -) [4][4] | raw, exp_avg, exp_avg_sq, totals [136] each | dadd [8] | ints: parameter map [136], leaf kfun [4],
// tree [5], pad, flags + SIMD words [16]
#define TTL_OFF_LEAF TR_OFF_TAIL
#define TTL_OFF_PAR (TTL_OFF_LEAF + 3 * TTL_L * TR_D + 4 * TTL_L)
#define TTL_OFF_SC (TTL_OFF_PAR + 4 * TTL_PPAD)
#define TTL_OFF_INT (TTL_OFF_SC + 8)
#define TTL_INTS (TTL_PPAD + 4 + 5 + 3 + 16)
#define TTL_LDS_DOUBLES (TTL_OFF_INT + TTL_INTS / 2)
#define TTL_OFF_VAR TTL_LDS_DOUBLES                // RESID: v_low | v_high, [128] each, behind the int table
#define TTL_RES_LDS_DOUBLES (TTL_OFF_VAR + 2 * TR_N)
static_assert(TTL_INTS % 2 == 0, "the int table ends on a double");
static_assert(TTL_PMAX + 1 <= TTL_PPAD && TTL_RW(TR_D) + 1 <= TTL_PPAD, "rho and its total fit the rows as they are");
static_assert(8 * (TTL_RW(TR_D) + 1) <= TR_N * TR_Y, "the waves' partial sums, dloss/drho included, fit Gamma's image");
static_assert(TTL_RES_LDS_DOUBLES * sizeof(double) <= 160 * 1024, "the tree trainers' LDS (the larger, residual request) exceeds a CU's 160 KiB");

// a leaf's bilinear form on rows xi, xj of X
template <int DM>
__device__ __forceinline__ double ttl_form(bool lin, const double* xi, const double (&xj)[DM], const double* w2, const double* cen) {
  double s = 0.0;
  if (lin) {
#pragma unroll
    for (int k = 0; k < DM; ++k) s = __builtin_fma(w2[k] * (xi[k] - cen[k]), xj[k] - cen[k], s);
  } else {
#pragma unroll
    for (int k = 0; k < DM; ++k) {
      const double df = xi[k] - xj[k];
      s = __builtin_fma(w2[k] * df, df, s);
    }
  }
  return s;
}
#define TTL_PUT(arr, e, x)            \
  do {                                \
    arr[0] = (e) == 0 ? (x) : arr[0]; \
    arr[1] = (e) == 1 ? (x) : arr[1]; \
    arr[2] = (e) == 2 ? (x) : arr[2]; \
    arr[3] = (e) == 3 ? (x) : arr[3]; \
  } while (0)

// One entry of the composed covariance: per leaf the form on rows xi, xj, amp_e phi_e of it (a linear leaf: amp_e times the form), then the
// tree -- the assembly's entry (phase P1 of ttl_body) and, in predict_small_tree.hip, Sigma's and K_s's.  tr: nl, shape, op[3]; kfi, lp, w2,
// cen: the leaf tables in LDS.  The leaf loop is not unrolled: one leaf's form is live at a time.
template <int DM, class TREE>
__device__ __forceinline__ double ttl_entry(const TREE& tr, const int* kfi, const double* lp, const double* w2, const double* cen, const double* xi,
                                            const double (&xj)[DM]) {
  double v[TTL_L] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int e = 0; e < tr.nl; ++e) {
    const int kf = tr_lds_int(kfi + e);
    const bool lin = kf == FFGP_KFUN_LINEAR;
    const double s = ttl_form<DM>(lin, xi, xj, w2 + e * TR_D, cen + e * TR_D);
    const double val = lp[4 * e] * (lin ? s : ffgp_kfun_val(kf, lp[4 * e + 2], fmax(s, lp[4 * e + 1])));
    TTL_PUT(v, e, val);
  }
  return ffgp_tree_eval(tr, v);
}

// DM: the input dimensions the per-entry loops are unrolled for (8 or 16: every model of the launch has D <= DM; the padded
// dimensions hold zeros and add nothing, so a model's arithmetic does not depend on which instantiation runs it)
// V2: the FFGP_LL_V2 likelihood (B = Sigma^-1 A by the two block chains once more; the targets' image receives B, so the targets are
// read again at the top of every step).  RESID: MODEL is TtlResModel and a member with rho set is a residual member (its targets and
// diagonal extra re-formed from rho at the top of every step, rho its (P + 1)-th Adam parameter); train_tree_lds.hip's instantiations
// (V2 = RESID = false, MODEL = TtlModel) see `if constexpr (false)` at every such place.
template <int DM, bool V2, bool RESID, class MODEL>
__device__ __forceinline__ void ttl_body(const MODEL* __restrict__ tab, TtlCommon cm) {
  constexpr int RW = TTL_RW(DM) + (RESID ? 1 : 0);      // RESID: one more total, dloss/drho, behind the leaves' sums
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const MODEL* __restrict__ M = tab + blockIdx.x;
  double* S = lds;
  double* Xs = lds + TR_OFF_XS;
  double* Ym = lds + TR_OFF_YM;
  double* Gam = lds + TR_OFF_GAM;
  double* Am = lds + TR_OFF_AM;
  double* piv = lds + TR_OFF_PIV;
  double* dvec = lds + TR_OFF_DVEC;
  double* wv = lds + TTL_OFF_LEAF;         // [leaf][16] effective inverse length scales
  double* w2 = wv + TTL_L * TR_D;          // [leaf][16] their squares (zero past D)
  double* cen = w2 + TTL_L * TR_D;         // [leaf][16] a linear leaf's centre (zero past D, and for the origin)
  double* lp = cen + TTL_L * TR_D;         // [leaf][4]  effective amplitude, clamp, 1 / kparam
  double* raw = lds + TTL_OFF_PAR;         // [P] raw parameters in the canonical order
  double* mom = raw + TTL_PPAD;            // [P] exp_avg
  double* mo2 = mom + TTL_PPAD;            // [P] exp_avg_sq
  double* tot = mo2 + TTL_PPAD;            // [TTL_RW] the step's totals
  double* sc = lds + TTL_OFF_SC;           // [0] effective diag_add, [1] the value's constant term
  int* pmap = reinterpret_cast<int*>(lds + TTL_OFF_INT);      // [P] leaf | kind << 4 | index << 8; kind 0 w, 1 amp, 2 centre, 3 diag_add
  int* kfi = pmap + TTL_PPAD;              // [leaf] FFGP_KFUN_*
  int* tri = kfi + 4;                      // nl, shape, op[3]
  int* flags = tri + 8;                    // [0] bad pivot of the current step; [1] RESID: 0 plain, 1 subset, 2 with variances; [8 + wave] SIMD words
  double* vlo = lds + TTL_OFF_VAR;         // RESID: [128] v_low,ii (zero past n, and in the subset form)
  double* vhi = vlo + TR_N;                //        [128] v_high,ii
  double* red = Gam;                       // [8][RW] per-wave partial sums (Gamma is dead between A and the next step's Gamma)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int n = M->n, D = M->D, d = M->d, P = M->P;
  int rmode_ = 0;
  if constexpr (RESID) rmode_ = M->rho ? (M->v_low ? 2 : 1) : 0;
  int Pt_ = P;                             // the Adam parameters: a residual member's rho is parameter P
  if constexpr (RESID) Pt_ += rmode_ ? 1 : 0;
  const int Pt = Pt_;
  const int nst = (n + 15) >> 4, nblk = nst * (nst + 1) / 2;

  // ---- once: inputs, targets, the diagonal extra, parameters and moments into LDS; identity padding of the blocks the factorisation
  //      never touches.  Targets, Gamma and A live as [128][16] images, zero beyond (n, d); X as [128][17], zero beyond (n, D).
  for (int idx = tid; idx < TR_N * TR_Y; idx += TR_T) {
    const int i = idx >> 4, q = idx & 15;
    Ym[idx] = (i < n && q < d && (!RESID || !rmode_)) ? M->Y[i * d + q] : 0.0;      // (a residual member's targets: formed at the top of every step)
    Gam[idx] = 0.0;
    Am[idx] = 0.0;
  }
  for (int idx = tid; idx < TR_N * (TR_D + 1); idx += TR_T) {
    const int i = idx / (TR_D + 1), k = idx - i * (TR_D + 1);
    Xs[idx] = (i < n && k < D) ? M->X[i * D + k] : 0.0;
  }
  for (int i = tid; i < TR_N; i += TR_T) dvec[i] = (M->diag_vec && i < n) ? M->diag_vec[(size_t)i * M->diag_stride] : 0.0;
  if constexpr (RESID) {
    for (int i = tid; i < TR_N; i += TR_T) {
      const bool on = rmode_ == 2 && i < n;
      vlo[i] = on ? M->v_low[(size_t)i * M->v_low_stride] : 0.0;
      vhi[i] = on ? M->v_high[(size_t)i * M->v_high_stride] : 0.0;
    }
  }
  if (tid < Pt) {
    int e = 0, kind = 3, kk = 0;
    if constexpr (RESID) kind = (tid == P) ? 4 : 3;
    if (tid < P - 1) {
      while (e < M->nl - 1 && tid >= M->k[e + 1].poff) ++e;
      kk = tid - M->k[e].poff;
      const int nw = M->k[e].nw;
      kind = (kk < nw) ? 0 : ((kk == nw) ? 1 : 2);
      if (kind == 2) kk -= nw + 1;
      if (kind == 1) kk = 0;
    }
    pmap[tid] = e | (kind << 4) | (kk << 8);
    const double* src = (kind == 0) ? M->k[e].w + kk : (kind == 1) ? M->k[e].amp : (kind == 2) ? M->k[e].cen + kk : M->dadd;
    if constexpr (RESID) src = (kind == 4) ? M->rho : src;
    raw[tid] = src[0];
    mom[tid] = M->state[tid];
    mo2[tid] = M->state[Pt + tid];
  }
  for (int t = wave; t < NBLK_LOWER; t += 8) {
    int bi, bj;
    blk_unrank(t, bi, bj);
    if (bi < nst) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) S[blk_off(bi, bj) + (g + 4 * r) * BLD + c] = (bi == bj && g + 4 * r == c) ? 1.0 : 0.0;
  }
  if (tid == 0) {
    flags[0] = 0;
    if constexpr (RESID) {
      flags[1] = rmode_;
      flags[2] = P;
    }
    tri[0] = M->nl; tri[1] = M->shape; tri[2] = M->op[0]; tri[3] = M->op[1]; tri[4] = M->op[2];
  }
  if (tid < TTL_L) kfi[tid] = (tid < M->nl) ? M->k[tid].kfun : FFGP_KFUN_SE;
  if (lane == 0) flags[8 + wave] = wave_simd(wave);
  __syncthreads();
  HELPER_ROLES(flags + 8, wave, hidx, nh);      // helpers of the factorisation's stage [A]
  ROLES_SEEN(lane, wave, hidx, nh);
  if (tid < TTL_L * TR_D) {      // the effective parameters of the first step (later ones: by the threads that update the raw ones)
    const int e = tid >> 4, k = tid & 15;
    double v = 0.0, cv = 0.0;
    if (e < M->nl && k < D) {
      const TtlLeaf& lf = M->k[e];
      v = ffgp_link_val(lf.w_link, raw[lf.poff + ((lf.nw == D) ? k : 0)], lf.w_c);
      if (lf.kfun == FFGP_KFUN_LINEAR && lf.cen) cv = lf.cen_train ? raw[lf.poff + lf.nw + 1 + k] : lf.cen[k];
    }
    wv[tid] = v;
    w2[tid] = v * v;
    cen[tid] = cv;
  } else if (tid < TTL_L * TR_D + TTL_L) {
    const int e = tid - TTL_L * TR_D;
    const bool on = e < M->nl;
    const TtlLeaf& lf = M->k[on ? e : 0];
    lp[4 * e] = on ? ffgp_link_val(lf.amp_link, raw[lf.poff + lf.nw], lf.amp_c) : 0.0;
    lp[4 * e + 1] = lf.clamp;
    lp[4 * e + 2] = lf.rinv;
    lp[4 * e + 3] = 0.0;
  } else if (tid == TTL_L * TR_D + TTL_L) {
    sc[0] = ffgp_link_val(M->dadd_link, raw[P - 1], M->dadd_c);
    sc[1] = 0.5 * (double)n * (double)d * log(2.0 * M->pi_const);      // the value's constant term (read where it is used: not a register
                                                                       // kept across the step loop)
  }
  __syncthreads();

  const int lane_k = lane, wave_k = wave, tid_k = tid;
  for (int step = 0; step < cm.steps; ++step) {
    // (the thread's coordinates opaque per iteration, as in tr_body: otherwise every per-lane offset of every phase is hoisted out of
    //  the step loop and kept alive across it -- 13 spilled registers in the <16> instantiation)
    int lane = lane_k, wave = wave_k, tid = tid_k;
    asm volatile("" : "+v"(lane), "+s"(wave), "+v"(tid));
    const int g = lane >> 4, c = lane & 15;
    TtlTree tr;
    tr.nl = tr_lds_int(tri); tr.shape = tr_lds_int(tri + 1); tr.op[0] = tr_lds_int(tri + 2); tr.op[1] = tr_lds_int(tri + 3);
    tr.op[2] = tr_lds_int(tri + 4);

    // ---- P0 (V2, RESID): the targets' image again -- B overwrote it (V2) -- or, a residual member, re-formed from the current rho with
    //      the diagonal extra: r = y_high - rho y_low, dvec = |v_high - rho v_low| (a product, then a difference: torch's rounding)
    int rmode = 0;
    if constexpr (RESID) rmode = tr_lds_int(flags + 1);
    if constexpr (V2 || RESID) {
      if (rmode) {
        const double rho = raw[tr_lds_int(flags + 2)];
        for (int idx = tid; idx < n * TR_Y; idx += TR_T) {
          const int i = idx >> 4, q = idx & 15;
          if (q < d) Ym[idx] = __dsub_rn(M->y_high_at(i * d + q), __dmul_rn(rho, M->y_low_at(i * d + q)));
        }
        if (rmode == 2 && tid < n) dvec[tid] = fabs(__dsub_rn(vhi[tid], __dmul_rn(rho, vlo[tid])));
        if (tid == 0 && M->rho_last_ptr()) M->rho_last_ptr()[0] = rho;
      } else if (V2) {
        for (int idx = tid; idx < n * TR_Y; idx += TR_T) {
          const int i = idx >> 4, q = idx & 15;
          if (q < d) Ym[idx] = M->Y[i * d + q];
        }
      }
      LDS_BARRIER();
    }

    // ---- P1: Sigma, lower block triangle (diagonal blocks symmetric-full: the in-register factor wants both halves); rows / columns
    //      beyond n are identity
    {
      const double dadd = sc[0];
      for (int q_ = 0; q_ < 5; ++q_) {
        const int t = tr_deal(q_, wave);
        if (t >= nblk) continue;
        int bi, bj;
        blk_unrank(t, bi, bj);
        double* dst = S + blk_off(bi, bj);
        const int j = bj * 16 + c;
        double xj[DM];
#pragma unroll
        for (int k = 0; k < DM; ++k) xj[k] = Xs[j * (TR_D + 1) + k];
#pragma unroll 1
        for (int r = 0; r < 4; ++r) {
          const int i = bi * 16 + g + 4 * r;
          double kv = ttl_entry<DM>(tr, kfi, lp, w2, cen, Xs + i * (TR_D + 1), xj);
          if (i == j) {
            kv += dadd;
            kv += dvec[i];
          }
          if (i >= n || j >= n) kv = (i == j) ? 1.0 : 0.0;
          dst[(g + 4 * r) * BLD + c] = kv;
        }
      }
    }
    LDS_BARRIER();

    // ---- P2: blocked Cholesky AND the inverse (train_tile.h)
#define TTL_NOPROF(k)
    TR_FACTOR_STAGES(S, piv, flags, n, nst, lane, wave, g, c, hidx, nh, TTL_NOPROF)
#undef TTL_NOPROF
    if (flags[0] != 0) {       // (uniform: every thread reads the same word behind the barrier)
      if (tid == 0) {
        cm.info[blockIdx.x] = flags[0];
        cm.fail_step[blockIdx.x] = step;
      }
      for (int k = step + tid; k < cm.steps; k += TR_T) M->trace[k] = __builtin_nan("");
      break;
    }
    tr_inverse_last_row(S, nst, lane, wave, g, c);

    // ---- P3: Gamma = W Y, the value's sum of squares, A = W^T Gamma
    tr_gamma_rows(S, Ym, Gam, nst, lane, wave, g, c);
    LDS_BARRIER();
    double ss = 0.0;      // (over the rows the stages wrote: the rest of the image is zero, or holds the last step's partial sums)
    if constexpr (!V2) {    // V1: Y^T Sigma^-1 Y = |Gamma|^2
#pragma unroll
      for (int q = 0; q < TR_N * TR_Y / TR_T; ++q) {
        const int idx = tid + TR_T * q;
        const double gq = (idx < nst * 16 * TR_Y) ? Gam[idx] : 0.0;
        ss = __builtin_fma(gq, gq, ss);
      }
    }
    {
      d4_t acc = {0.0, 0.0, 0.0, 0.0};
      tr_alpha_rows(S, Gam, Am, nst, lane, wave, g, c, acc);
    }
    LDS_BARRIER();
    if constexpr (V2) {     // |Sigma^-1 Y|^2 = |A|^2; then B = Sigma^-1 A: the two chains once more -- W A over Gamma's image (dead once A
                            // exists), B over the targets' image
#pragma unroll
      for (int q = 0; q < TR_N * TR_Y / TR_T; ++q) {
        const int idx = tid + TR_T * q;
        const double aq = (idx < nst * 16 * TR_Y) ? Am[idx] : 0.0;
        ss = __builtin_fma(aq, aq, ss);
      }
      tr_gamma_rows(S, Am, Gam, nst, lane, wave, g, c);
      LDS_BARRIER();
      d4_t accb = {0.0, 0.0, 0.0, 0.0};
      tr_alpha_rows(S, Gam, Ym, nst, lane, wave, g, c, accb);
      LDS_BARRIER();
    }
    // RESID: this thread's part of -dloss/drho = sum (dloss/dr) .* y_low (dloss/dr = A, V2: B in the targets' image) + sum_i G_ii sgn(s_i) v_low,ii
    // (the diagonal term joins it in pass 1, where G_ii stands in the accumulators)
    [[maybe_unused]] double drho = 0.0;
    if constexpr (RESID) {
      if (rmode) {
        const double* dr = V2 ? Ym : Am;
        for (int idx = tid; idx < n * TR_Y; idx += TR_T) {
          const int i = idx >> 4, q = idx & 15;
          if (q < d) drho = __builtin_fma(dr[idx], M->y_low_at(i * d + q), drho);
        }
      }
    }

    // ---- P5, pass 1: Sigma^-1 block by block on the matrix cores; per entry G, the leaves again, the reverse sweep
    const double lpiv = (tid < n) ? log(piv[tid]) : 0.0;
    double trg = 0.0, sa[TTL_L] = {0.0, 0.0, 0.0, 0.0};
    for (int q_ = 0; q_ < 5; ++q_) {
      const int t = tr_deal(q_, wave);
      if (t >= nblk) continue;
      int bi, bj;
      blk_unrank(t, bi, bj);
      d4_t acc = {0.0, 0.0, 0.0, 0.0};
      tr_chain<true>(acc, bi, nst, S, [bi](int kb) { return blk_off(kb, bi); }, BLD, S, [bj](int kb) { return blk_off(kb, bj); }, BLD, lane);
      const int j = bj * 16 + c;
      double xj[DM];
#pragma unroll
      for (int k = 0; k < DM; ++k) xj[k] = Xs[j * (TR_D + 1) + k];
#pragma unroll 1
      for (int r = 0; r < 4; ++r) {
        const int i = bi * 16 + g + 4 * r;
        const double* xi = Xs + i * (TR_D + 1);
        const double accr = (r == 0) ? acc[0] : (r == 1) ? acc[1] : (r == 2) ? acc[2] : acc[3];
        double aa = 0.0;
        if constexpr (V2) {      // G = d/2 Sigma^-1 - 1/2 (A B^T + B A^T), B in the targets' image
          for (int q = 0; q < d; ++q) aa = __builtin_fma(Am[i * TR_Y + q], Ym[j * TR_Y + q], __builtin_fma(Ym[i * TR_Y + q], Am[j * TR_Y + q], aa));
        } else {
          for (int q = 0; q < d; ++q) aa = __builtin_fma(Am[i * TR_Y + q], Am[j * TR_Y + q], aa);
        }
        const bool live = (i < n && j <= i);
        const double gv = live ? 0.5 * (double)d * accr - 0.5 * aa : 0.0;
        const double sym = (i == j) ? 1.0 : 2.0;
        double v[TTL_L] = {0.0, 0.0, 0.0, 0.0}, ev[TTL_L] = {0.0, 0.0, 0.0, 0.0}, dv[TTL_L] = {0.0, 0.0, 0.0, 0.0}, gl[TTL_L];
#pragma unroll 1
        for (int e = 0; e < tr.nl; ++e) {
          const int kf = tr_lds_int(kfi + e);
          const bool lin = kf == FFGP_KFUN_LINEAR;
          const double s = ttl_form<DM>(lin, xi, xj, w2 + e * TR_D, cen + e * TR_D);
          const double amp = lp[4 * e];
          double evx = s, dvx = amp;
          if (!lin) {
            const double cl = lp[4 * e + 1], sq = fmax(s, cl);
            evx = ffgp_kfun_val(kf, lp[4 * e + 2], sq);
            dvx = (s >= cl) ? amp * ffgp_kfun_m2d(kf, lp[4 * e + 2], sq) : 0.0;
          }
          TTL_PUT(ev, e, evx);
          TTL_PUT(dv, e, dvx);
          TTL_PUT(v, e, amp * evx);
        }
        ffgp_tree_back(tr, v, gl);
        if (i == j) trg += gv;
        if constexpr (RESID) {
          if (i == j && rmode == 2) {      // (sgn(0) = 0: torch's abs backward)
            const double vl = vlo[i], s_ = __dsub_rn(vhi[i], __dmul_rn(raw[tr_lds_int(flags + 2)], vl));
            drho = __builtin_fma(gv, (s_ > 0.0) ? vl : ((s_ < 0.0) ? -vl : 0.0), drho);
          }
        }
#pragma unroll
        for (int e = 0; e < TTL_L; ++e) {
          if (e < tr.nl) {
            const double ge = sym * gv * gl[e];
            sa[e] = __builtin_fma(ge, ev[e], sa[e]);
            M->wbuf[((e * NBLK_LOWER + t) * 4 + r) * 64 + lane] = live ? ge * dv[e] : 0.0;
          }
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this lane's parked weights have landed

    // ---- P5, pass 2: the per-dimension sums, leaf by leaf (one leaf's accumulators live at a time)
#pragma unroll 1
    for (int e = 0; e < tr.nl; ++e) {
      const bool lin = tr_lds_int(kfi + e) == FFGP_KFUN_LINEAR;
      const double* ce = cen + e * TR_D;
      double tk[DM], tc[DM];
#pragma unroll
      for (int k = 0; k < DM; ++k) tk[k] = tc[k] = 0.0;
      for (int q_ = 0; q_ < 5; ++q_) {
        const int t = tr_deal(q_, wave);
        if (t >= nblk) continue;
        int bi, bj;
        blk_unrank(t, bi, bj);
        double wts[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) wts[r] = M->wbuf[((e * NBLK_LOWER + t) * 4 + r) * 64 + lane];
        const int j = bj * 16 + c;
        double xj[DM];
#pragma unroll
        for (int k = 0; k < DM; ++k) xj[k] = Xs[j * (TR_D + 1) + k] - (lin ? ce[k] : 0.0);
#pragma unroll 1
        for (int r = 0; r < 4; ++r) {
          const double* xi = Xs + (bi * 16 + g + 4 * r) * (TR_D + 1);
          const double wt = (r == 0) ? wts[0] : (r == 1) ? wts[1] : (r == 2) ? wts[2] : wts[3];
          if (lin) {
#pragma unroll
            for (int k = 0; k < DM; ++k) {
              const double a = xi[k] - ce[k];
              tk[k] = __builtin_fma(wt * a, xj[k], tk[k]);
              tc[k] = __builtin_fma(wt, a + xj[k], tc[k]);
            }
          } else {
#pragma unroll
            for (int k = 0; k < DM; ++k) {
              const double df = xi[k] - xj[k];
              tk[k] = __builtin_fma(wt * df, df, tk[k]);
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < DM; ++k) {
        const double a = tr_wsum(tk[k]), b = tr_wsum(tc[k]);
        if (lane == 0) {
          red[wave * RW + TTL_NSC + e * 2 * DM + k] = a;
          red[wave * RW + TTL_NSC + e * 2 * DM + DM + k] = b;
        }
      }
    }
    // ---- one workgroup reduction for all of them (and the log-determinant: one pivot per thread)
    {
      double vals[TTL_NSC] = {ss, trg, lpiv, sa[0], sa[1], sa[2], sa[3]};
#pragma unroll
      for (int q = 0; q < TTL_NSC; ++q) vals[q] = tr_wsum(vals[q]);
      if (lane == 0) {
#pragma unroll
        for (int q = 0; q < TTL_NSC; ++q) red[wave * RW + q] = vals[q];
      }
      if constexpr (RESID) {
        drho = tr_wsum(drho);
        if (lane == 0) red[wave * RW + TTL_RW(DM)] = drho;
      }
      LDS_BARRIER();
      if (tid < TTL_NSC + tr.nl * 2 * DM || (RESID && tid == TTL_RW(DM))) {
        double x = 0.0;
#pragma unroll
        for (int wv_ = 0; wv_ < 8; ++wv_) x += red[wv_ * RW + tid];
        tot[tid] = x;
      }
      LDS_BARRIER();
    }

    // ---- P6: the loss of this step (before the update), the raw gradients through the links, Adam
    const double oscale = M->oscale;
    if (tid == 0)
      M->trace[step] = oscale * (0.5 * tot[0] + (double)d * 0.5 * tot[2] + sc[1]);
    double gr = 0.0;
    int pe = 0, pkind = 0, pk = 0;
    int Pt = P;
    if constexpr (RESID) Pt = tr_lds_int(flags + 2) + (rmode ? 1 : 0);
    if (tid < Pt) {
      const int pm = pmap[tid];
      pe = pm & 15; pkind = (pm >> 4) & 15; pk = pm >> 8;
      const TtlLeaf& lf = M->k[pe];
      const double* tk = tot + TTL_NSC + pe * 2 * DM;
      const bool lin = lf.kfun == FFGP_KFUN_LINEAR;
      if (pkind == 0) {
        double ge;
        if (lf.nw == D) {
          const double s = wv[pe * TR_D + pk] * tk[pk];
          ge = lin ? 2.0 * s : -s;
        } else {      // a broadcast length scale: the D effective gradients summed in index order, then one derivative
          ge = 0.0;
          for (int k = 0; k < D; ++k) {
            const double s = wv[pe * TR_D + k] * tk[k];
            ge += lin ? 2.0 * s : -s;
          }
        }
        gr = oscale * ge * ffgp_link_der(lf.w_link, raw[tid], lf.w_c);
      } else if (pkind == 1) {
        gr = oscale * tot[3 + pe] * ffgp_link_der(lf.amp_link, raw[tid], lf.amp_c);
      } else if (pkind == 2) {
        gr = oscale * -(w2[pe * TR_D + pk] * tk[DM + pk]);      // (identity link)
      } else if (!RESID || pkind == 3) {
        gr = oscale * tot[1] * ffgp_link_der(M->dadd_link, raw[tid], M->dadd_c);
      } else {
        gr = oscale * -tot[TTL_RW(DM)];      // rho (identity link)
      }
    }
    const double bc1 = cm.bc[2 * step], bc2s = cm.bc[2 * step + 1];      // (uniform: scalar loads)
    LDS_BARRIER();      // (every gradient is formed from this step's effective values before any of them moves)
    if (tid < Pt) {
      ffgp_adam_update(raw + tid, mom + tid, mo2 + tid, gr, cm.lr, cm.b1, cm.b2, cm.eps, bc1, bc2s);
      const double pnew = raw[tid];
      const TtlLeaf& lf = M->k[pe];
      if (pkind == 0) {      // the next step's effective values
        const double e_ = ffgp_link_val(lf.w_link, pnew, lf.w_c);
        if (lf.nw == D) {
          wv[pe * TR_D + pk] = e_;
          w2[pe * TR_D + pk] = e_ * e_;
        } else {
          for (int k = 0; k < D; ++k) {
            wv[pe * TR_D + k] = e_;
            w2[pe * TR_D + k] = e_ * e_;
          }
        }
      } else if (pkind == 1) {
        lp[4 * pe] = ffgp_link_val(lf.amp_link, pnew, lf.amp_c);
      } else if (pkind == 2) {
        cen[pe * TR_D + pk] = pnew;
      } else if (!RESID || pkind == 3) {
        sc[0] = ffgp_link_val(M->dadd_link, pnew, M->dadd_c);
      }
    }
    LDS_BARRIER();
  }
  // ---- parameters and moments back to the caller's tensors (a failed step left them as they were when it began)
  int tid_e = tid_k;
  asm volatile("" : "+v"(tid_e));      // (nothing of this epilogue is to be prepared in front of the step loop and kept across it)
  if (tid_e < Pt) {
    const int tid = tid_e;
    const int pm = pmap[tid];
    const int e = pm & 15, kind = (pm >> 4) & 15, kk = pm >> 8;
    double* dst = (kind == 0) ? M->k[e].w + kk : (kind == 1) ? M->k[e].amp : (kind == 2) ? M->k[e].cen + kk : M->dadd;
    if constexpr (RESID) dst = (kind == 4) ? M->rho : dst;
    dst[0] = raw[tid];
    M->state[tid] = mom[tid];
    M->state[Pt + tid] = mo2[tid];
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
// the member's description, or false when it is outside what the kernel covers
// (v2_ok: the entry trains FFGP_LL_V2 members too; resid: the member's targets come from its residual link, Y_dev is not read)
static bool ttl_describe(const ffgp_problem& q, const ffgp_tree_links& l, long state_stride, TtlModel& m, bool v2_ok = false, bool resid = false) {
  const ffgp_ktree* t = q.tree;
  if (!t || q.pair || q.cov_dev || q.add_mat_dev || q.add_all != 0.0 || q.mean_jitter != 0.0) return false;
  if (q.ll_variant != FFGP_LL_V1 && !(v2_ok && q.ll_variant == FFGP_LL_V2)) return false;
  if (q.n <= 0 || q.n > TR_N || q.D <= 0 || q.D > TR_D || q.d <= 0 || q.d > TR_Y || !q.X_dev || (!q.Y_dev && !resid) || !q.diag_add_dev) return false;
  if (!ffgp_tree_form_ok(t)) return false;
  memset(static_cast<void*>(&m), 0, sizeof(TtlModel));
  m.n = q.n; m.D = q.D; m.d = q.d;
  m.nl = t->n_leaves; m.shape = (t->n_leaves == 4) ? t->shape : FFGP_TREE_CHAIN;
  for (int i = 0; i < 3; ++i) m.op[i] = (i + 1 < t->n_leaves) ? t->op[i] : FFGP_KOP_SUM;
  int P = 0;
  for (int e = 0; e < t->n_leaves; ++e) {
    const ffgp_kdesc& k = t->leaf[e];
    const ffgp_leaf_links& ll = l.leaf[e];
    const bool linear = (k.kfun == FFGP_KFUN_LINEAR);
    if (!ffgp_tree_leaf_trainable(k, ll)) return false;
    TtlLeaf& lf = m.k[e];
    lf.w = const_cast<double*>(k.w_dev); lf.amp = const_cast<double*>(k.amp_dev);
    lf.cen = linear ? const_cast<double*>(k.center_dev) : nullptr;
    lf.w_c = ll.w_c; lf.amp_c = ll.amp_c; lf.clamp = k.clamp_min; lf.rinv = (k.kparam != 0.0) ? 1.0 / k.kparam : 1.0;
    lf.w_link = ll.w_link; lf.amp_link = ll.amp_link; lf.nw = ll.w_broadcast ? 1 : q.D; lf.cen_train = ll.center_train ? 1 : 0;
    lf.kfun = k.kfun; lf.poff = P;
    P += lf.nw + 1 + (lf.cen_train ? q.D : 0);
  }
  m.P = P + 1;
  if (state_stride < 2 * (long)(m.P + (resid ? 1 : 0))) return false;
  m.dadd_link = l.dadd_link; m.dadd_c = l.dadd_c;
  m.X = q.X_dev; m.Y = q.Y_dev; m.diag_vec = q.diag_vec_dev; m.diag_stride = q.diag_stride;
  m.dadd = const_cast<double*>(q.diag_add_dev);
  m.oscale = (l.out_scale == 0.0) ? 1.0 : l.out_scale; m.pi_const = q.pi_const;
  return true;
}
