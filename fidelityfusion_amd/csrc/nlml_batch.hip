// Fused NLML (+ gradients) of F blocks in ONE chain of launches: ffgp_nlml_fused_batch and its gradient lanes.  See include/ffgp.h.
#include <algorithm>

#include "drivers.h"

// ffgp_link_fwd (nlml.hip) for up to FFGP_MULTI_MAX models per launch (the members of a shared-chain batch)
struct ffgp_multi_link {
  ffgp_links l[FFGP_MULTI_MAX];
  const double* rw[FFGP_MULTI_MAX];
  const double* ramp[FFGP_MULTI_MAX];
  const double* rdadd[FFGP_MULTI_MAX];
  double* eff[FFGP_MULTI_MAX];
  int D[FFGP_MULTI_MAX];
};
extern "C" __global__ void ffgp_link_fwd_multi(ffgp_multi_link q) {
  const int z = blockIdx.x, t = threadIdx.x, D = q.D[z];
  const ffgp_links& l = q.l[z];
  double* __restrict__ eff = q.eff[z];
  if (t < D) eff[t] = ffgp_link_val(l.w_link, q.rw[z][l.w_broadcast ? 0 : t], l.w_c);
  if (t == 0) {
    eff[D] = ffgp_link_val(l.amp_link, q.ramp[z][0], l.amp_c);
    if (q.rdadd[z]) eff[D + 1] = ffgp_link_val(l.dadd_link, q.rdadd[z][0], l.dadd_c);
  }
}

// the handle's stream and per-lane scratch pointers while one member's stages are enqueued on a lane (lane 0: the call's own stream)
struct LaneGuard {
  ffgp_handle* h; int lane; hipStream_t main_s; double* skw0; size_t skwb0; double* scal0;
  LaneGuard(ffgp_handle* h_, int lane_, hipStream_t m) : h(h_), lane(lane_), main_s(m), skw0(h_->skw), skwb0(h_->skw_bytes), scal0(h_->d_scal) {
    if (lane > 0) {
      h->stream = h->lane_st[lane];
      h->skw = h->lane_skw[lane]; h->skw_bytes = h->lane_skw_bytes[lane];
      h->d_scal = h->lane_scal + (size_t)lane * 64;
    }
  }
  ~LaneGuard() {
    if (lane > 0) {
      h->lane_skw[lane] = h->skw; h->lane_skw_bytes[lane] = h->skw_bytes;      // (it may have grown)
      h->skw = skw0; h->skw_bytes = skwb0; h->d_scal = scal0;
      h->stream = main_s;
    }
  }
};

struct BatchMember {
  int n, d, ld, nblk;
  size_t off, doff;      // in doubles: [Sigma | Y^T] -> [L | Gamma^T] in h->ws; the member's slice of the Dinv store
  bool wants_grad;
  int lane;              // gradient lane (0 = the call's stream)
  ffgp_problem q;        // the problem, its parameters redirected to the effective slots when there are links ...
  ffgp_grads gq;         // ... and the gradients, the three parameter gradients redirected to geff
  bool chain;
};
// the call's arguments and what it decides before it enqueues anything (zero-initialised); offsets (o_) and sizes (s) in doubles of h->ws
struct BatchPlan {
  int F;
  const ffgp_problem* p;
  const ffgp_links* l;
  const ffgp_grads* g;
  double* nll_dev;
  bool uniform, want_grad, all_grad;
  int nl;                  // gradient lanes (1 = member after member)
  size_t blk;              // uniform batches: the stride between the blocks
  size_t dinv_blocks, total;
  size_t o_link, o_red, o_X, o_S, o_T, o_At, o_P;
  size_t sX, sT, sAt, sP;  // member-wise maxima of the gradient scratch
  hipStream_t main_stream;
  double* dinv0;           // the handle's Dinv store (h->dinv points at one member's slice while its inverse is formed)
};
// effective parameters / their gradients, 256 + 256 doubles per block
static double* batch_eff(const ffgp_handle* h, const BatchPlan& b, int f) { return h->ws + b.o_link + (size_t)f * 512; }

static int batch_validate(const ffgp_handle* h, BatchPlan& b, std::vector<BatchMember>& mem) {
  const ffgp_problem* p = b.p;
  b.uniform = true;
  for (int f = 0; f < b.F; ++f) {
    const ffgp_problem& q = p[f];
    if (q.n <= FFGP_NB || q.d <= 0 || q.cov_dev || q.pair || q.tree || !q.X_dev || !q.Y_dev || !q.w_dev || !q.amp_dev || q.D <= 0 || q.D > 128 ||
        q.ll_variant != FFGP_LL_V1 || q.kfun < FFGP_KFUN_SE || q.kfun > FFGP_KFUN_RQ)
      return FFGP_ERR_ARG;
    b.uniform = b.uniform && q.n == p[0].n && q.d == p[0].d;
    if (b.g) {
      if (b.g[f].g_cov_dev || b.g[f].g_pair) return FFGP_ERR_ARG;
      mem[f].wants_grad = ffgp_wants_grad(&b.g[f]);
      b.want_grad = b.want_grad || mem[f].wants_grad;
    }
  }
  if (!b.uniform) {      // members of different sizes: the ragged chain's own limits (ffgp_potrf_ragged)
    for (int f = 0; f < b.F; ++f)
      if (h->lookahead && p[f].n > h->nb_outer && p[f].n > h->la_min_n && !(h->la_carry == 1 || (h->la_carry == 2 && p[f].n <= h->la_carry_n)))
        return FFGP_ERR_ARG;
  }
  return FFGP_OK;
}

// per-member layout: [Sigma | Y^T] -> [L | Gamma^T] blocks one after the other, each with its own leading dimension; then the links'
// slots, the reductions' partial sums and the gradient scratch (all_grad: one copy per block; else one per lane)
static void batch_layout(const ffgp_handle* h, BatchPlan& b, std::vector<BatchMember>& mem) {
  const int F = b.F;
  size_t total = 0;
  int n_grad = 0, nmax_all = 0;
  b.all_grad = b.want_grad && h->batch_grad_ob && b.uniform;
  for (int f = 0; f < F; ++f) {
    BatchMember& m = mem[f];
    m.n = b.p[f].n;
    m.d = b.p[f].d;
    m.ld = ffgp_round_up(m.n, 16);
    m.off = total;
    total += (size_t)(m.n + m.d) * m.ld;
    m.nblk = (m.n + FFGP_NB - 1) / FFGP_NB;
    m.doff = b.dinv_blocks * FFGP_NB * FFGP_NB;
    b.dinv_blocks += m.nblk;
    const ffgp_grad_scratch gs = ffgp_grad_scratch_sizes(m.n, m.d, b.p[f].D, FFGP_LL_V1, 0);
    b.sX = std::max(b.sX, gs.X);
    b.sT = std::max(b.sT, gs.T);
    b.sAt = std::max(b.sAt, gs.At);
    b.sP = std::max(b.sP, gs.P);
    b.all_grad = b.all_grad && m.wants_grad;
    n_grad += m.wants_grad ? 1 : 0;
    nmax_all = std::max(nmax_all, m.n);
  }
  b.blk = mem[1].off - mem[0].off;
  b.o_link = total; total += (size_t)F * 512;
  b.o_red = total; total += (size_t)F * 2 * FFGP_RED_BLOCKS;
  // gradient stage: when EVERY block of an equal-shape batch wants gradients (and the inverses fit), Sigma_f^-1 of all blocks come out
  // of one sequence of launches with an outer batch index (ffgp_trtri_lauum_ob) -- a lone N = 4096 inverse underfills the chip at its
  // lower levels; otherwise block after block through one set of buffers
  if (b.all_grad && (size_t)F * (2 * b.sX + b.sT) * sizeof(double) > ((size_t)48 << 30)) b.all_grad = false;
  // Members whose gradient stages cannot share launches (different sizes) run them SIDE BY SIDE instead (round 6): up to three lanes, each
  // a stream with its own scratch (inverse, Sigma^-1, TRTRI workspace, A^T, partial sums, split-K workspace, trace scalar), every member's
  // stage sequence exactly its single call's -- so its bits are too.  For three blocks of 300 / 300 / 250 points the three latency-bound
  // chains of ~12 launches overlap; larger members fill one another's gaps.  Option "grad_lanes" (default 3; 1 = member after member).
  // measured (tools/ragged_probe.py, FFGP_OPTS=grad_lanes=1 / 3): (300, 300, 250) 0.839 -> 0.789 ms, (4096, 3000, 2000) 5.32 -> 5.02,
  // (2048, 2048, 1024, 1500) 2.77 -> 2.69; (8192, 4096, 2048, 1024) 16.3 -> 17.0 -- a throughput-bound member gains nothing from
  // neighbours on its chip, so sets with a member above 6144 rows stay member after member.  Small members are bound by the HOST's
  // launch rate (15 launches per member), which lanes do not change: the gate of 1.4 x the largest member is not met (1.66 x).
  b.nl = (!b.all_grad && n_grad >= 2 && h->grad_lanes > 1 && h->timing == 0 && nmax_all <= 6144) ? std::min(std::min(n_grad, h->grad_lanes), 3) : 1;
  b.sT = (b.sT + 15) / 16 * 16; b.sAt = (b.sAt + 15) / 16 * 16; b.sP = (b.sP + 15) / 16 * 16;
  if (b.nl > 1 && (size_t)b.nl * (2 * b.sX + b.sT) * sizeof(double) > ((size_t)48 << 30)) b.nl = 1;
  const size_t copies = b.all_grad ? (size_t)F : (size_t)b.nl;
  if (b.want_grad) {
    b.o_X = total; total += copies * b.sX;
    b.o_S = total; total += copies * b.sX;
    b.o_T = total; total += copies * b.sT;
    b.o_At = total; total += (size_t)b.nl * b.sAt;
    b.o_P = total; total += (size_t)b.nl * b.sP;
  }
  b.total = total;
}

// ---- links, assembly, passenger rows: block after block (each a few launches that fill the chip by themselves)
// (the tiny per-member stages -- links, target transposes, the reductions further down -- are issued for eight members per launch:
// F x 5 launches of a few microseconds each were a third of a 300 / 300 / 250 batch's time)
static int batch_assemble(ffgp_handle* h, const BatchPlan& b, std::vector<BatchMember>& mem) {
  const int F = b.F;
  const ffgp_problem* p = b.p;
  const ffgp_links* l = b.l;
  for (int f = 0; f < F; ++f) {
    double* eff = batch_eff(h, b, f);
    mem[f].chain = ffgp_links_redirect(&p[f], l ? &l[f] : nullptr, b.g ? &b.g[f] : nullptr, eff, eff + 256, &mem[f].q, &mem[f].gq);
  }
  if (l) {
    for (int f0 = 0; f0 < F; f0 += FFGP_MULTI_MAX) {
      const int cnt = F - f0 < FFGP_MULTI_MAX ? F - f0 : FFGP_MULTI_MAX;
      ffgp_multi_link ml;
      for (int z = 0; z < FFGP_MULTI_MAX; ++z) {
        const int f = f0 + (z < cnt ? z : 0);
        ml.l[z] = l[f]; ml.rw[z] = p[f].w_dev; ml.ramp[z] = p[f].amp_dev; ml.rdadd[z] = p[f].diag_add_dev;
        ml.eff[z] = batch_eff(h, b, f); ml.D[z] = p[f].D;
      }
      hipLaunchKernelGGL(ffgp_link_fwd_multi, dim3(cnt), dim3(128), 0, h->stream, ml);
    }
  }
  std::vector<const double*> tsrc(F);
  std::vector<double*> tdst(F);
  std::vector<int> trows(F), tcols(F), tlds(F), tldd(F);
  ffgp_assemble_collect_begin(h);      // (small members' assemblies: parked, then eight per launch)
  int arc = FFGP_OK;
  for (int f = 0; f < F && arc == FFGP_OK; ++f) {
    const BatchMember& m = mem[f];
    const ffgp_problem& q = m.q;
    double* W0 = h->ws + m.off;
    arc = ffgp_assemble_impl(h, q.X_dev, m.n, q.X_dev, m.n, q.D, q.w_dev, q.amp_dev, q.clamp_min, q.diag_add_dev, q.diag_vec_dev, q.diag_stride,
                             q.add_mat_dev, q.ld_add, q.add_all, q.mean_jitter, W0, m.ld, 1, q.kfun, q.kparam);
    tsrc[f] = q.Y_dev; tdst[f] = W0 + (size_t)m.n * m.ld; trows[f] = m.n; tcols[f] = m.d; tlds[f] = m.d; tldd[f] = m.ld;
  }
  const int erc = ffgp_assemble_collect_end(h);      // (always: the handle must not stay in collecting mode)
  FFGP_CHECK(arc);
  FFGP_CHECK(erc);
  return ffgp_transpose_multi(h, F, tsrc.data(), trows.data(), tcols.data(), tlds.data(), tdst.data(), tldd.data());
}

// ---- ONE factorisation chain for all F blocks
static int batch_factor(ffgp_handle* h, const BatchPlan& b, const std::vector<BatchMember>& mem) {
  h->tri_hook_col = 0;
  h->tri_hook_fired = 0;
  int prc;
  if (b.uniform) {
    h->bt_F = b.F;
    h->bt_sA = (long)b.blk;
    h->bt_sD = (long)mem[0].nblk * FFGP_NB * FFGP_NB;
    prc = ffgp_potrf_impl(h, h->ws, mem[0].n, mem[0].n + mem[0].d, mem[0].ld, 0);
    h->bt_F = 0;
  } else {
    std::vector<ffgp_rag_block> rag(b.F);
    for (int f = 0; f < b.F; ++f) rag[f] = ffgp_rag_block{h->ws + mem[f].off, mem[f].n, mem[f].n + mem[f].d, mem[f].ld, h->dinv + mem[f].doff, f};
    prc = ffgp_potrf_ragged(h, b.F, rag.data());
  }
  h->dinv_L = nullptr;          // (the store holds F factors' inverses: it belongs to none of them as far as the cache is concerned)
  h->sinv_L = nullptr;
  return prc;
}

static int batch_reduce(ffgp_handle* h, const BatchPlan& b, const std::vector<BatchMember>& mem) {
  const int F = b.F;
  std::vector<const double*> rL(F), rM(F);
  std::vector<double*> rout(F);
  std::vector<int> rn(F), rld(F), rd(F);
  std::vector<double> rpi(F), rsc(F);
  for (int f = 0; f < F; ++f) {
    const BatchMember& m = mem[f];
    rL[f] = h->ws + m.off; rM[f] = h->ws + m.off + (size_t)m.n * m.ld; rout[f] = b.nll_dev + f;
    rn[f] = m.n; rld[f] = m.ld; rd[f] = m.d; rpi[f] = m.q.pi_const;
    // forward only: the output scale (the sign of the reference's +LL) is folded into the reduction's last step
    rsc[f] = (b.l && !b.want_grad && b.l[f].out_scale != 0.0) ? b.l[f].out_scale : 1.0;
  }
  return ffgp_nll_reduce_multi(h, F, rL.data(), rn.data(), rld.data(), rM.data(), rd.data(), rn.data(), rld.data(), rd.data(), rpi.data(),
                               rsc.data(), rout.data(), h->ws + b.o_red);
}

// lanes: their streams, events and scalar scratch are created at first use; members are dealt longest-first to the lane with the least
// work so far, lane 0 is the call's own stream.  order: the members in the order their gradient stages are enqueued.
static int batch_plan_lanes(ffgp_handle* h, const BatchPlan& b, std::vector<BatchMember>& mem, std::vector<int>& order) {
  if (!h->lane_scal) {
    FFGP_HIP(hipMalloc(&h->lane_scal, (size_t)FFGP_GRAD_LANES * 64 * sizeof(double)));
    FFGP_HIP(hipMemsetAsync(h->lane_scal, 0, (size_t)FFGP_GRAD_LANES * 64 * sizeof(double), h->stream));
  }
  // the lanes are the handle's side streams (idle during the gradient stages): they own hardware queues already -- a stream created
  // now would be dealt onto one of the few queues round robin, quite possibly the call's own, and run BEHIND it
  FFGP_CHECK(ffgp_ensure_aux2(h));
  h->lane_st[1] = h->aux2;
  h->lane_st[2] = h->aux3;      // (not the chain's stream h->aux: the GEMM launcher treats launches on it specially -- priority, no split-K)
  for (int z = 0; z < b.nl; ++z)
    if (!h->lane_ev[z]) FFGP_HIP(hipEventCreateWithFlags(&h->lane_ev[z], hipEventDisableTiming));
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return mem[x].n > mem[y].n; });
  double load[FFGP_GRAD_LANES] = {0.0, 0.0, 0.0, 0.0};
  for (int f : order) {
    int best = 0;
    for (int z = 1; z < b.nl; ++z)
      if (load[z] < load[best]) best = z;
    mem[f].lane = best;
    load[best] += (double)mem[f].n * mem[f].n * mem[f].n + 1e6;      // (+ a launch-count term: small members are chains of launches)
  }
  if (hipEventRecord(h->lane_ev[0], b.main_stream) != hipSuccess) return FFGP_ERR_HIP;
  for (int z = 1; z < b.nl; ++z)
    if (hipStreamWaitEvent(h->lane_st[z], h->lane_ev[0], 0) != hipSuccess) return FFGP_ERR_HIP;
  return FFGP_OK;
}


// one member's inverse / gradient stages on its lane, its single call's launch sequence
static int batch_member_grad(ffgp_handle* h, const BatchPlan& b, const BatchMember& m, int f) {
  const int n = m.n, d = m.d, ld = m.ld;
  double* W0 = h->ws + m.off;
  double* Gt = W0 + (size_t)n * ld;
  const int lane = (b.nl > 1) ? m.lane : 0;
  LaneGuard lg(h, lane, b.main_stream);
  // the block's own slice of the Dinv store, presented as "the" store of this factor while its inverse is formed
  h->dinv = b.dinv0 + m.doff;
  h->dinv_L = W0; h->dinv_n = n; h->dinv_ld = ld;
  double* X = h->ws + b.o_X + (b.all_grad ? (size_t)f * b.sX : (size_t)lane * b.sX);
  double* S = h->ws + b.o_S + (b.all_grad ? (size_t)f * b.sX : (size_t)lane * b.sX);
  double* T = h->ws + b.o_T + (b.all_grad ? 0 : (size_t)lane * b.sT);
  double* At = h->ws + b.o_At + (size_t)lane * b.sAt;
  double* P = h->ws + b.o_P + (size_t)lane * b.sP;
  const ffgp_grads& gg = b.g[f];
  if (!b.all_grad) {
    FFGP_CHECK(ffgp_trtri_impl(h, W0, n, ld, X, ld, T));
    FFGP_CHECK(ffgp_lauum_impl(h, X, n, ld, S, ld));
  }
  FFGP_CHECK(ffgp_grad_v1_stages(h, &m.q, &m.gq, m.q.D, m.q.mean_jitter, Gt, X, S, At, P, ld));
  if (gg.g_Y_dev) FFGP_CHECK(ffgp_transpose(h, At, d, n, ld, gg.g_Y_dev, d, 1.0));
  if (b.l) ffgp_links_finish(h, &b.p[f], &b.l[f], &gg, batch_eff(h, b, f) + 256, m.chain, b.nll_dev + f);
  return FFGP_OK;
}

// the call's stream waits for every lane (also on an error path: nothing of this call may still be running on a lane)
static void batch_join_lanes(ffgp_handle* h, const BatchPlan& b) {
  for (int z = 1; z < b.nl; ++z) {
    if (hipEventRecord(h->lane_ev[z], h->lane_st[z]) != hipSuccess || hipStreamWaitEvent(b.main_stream, h->lane_ev[z], 0) != hipSuccess) {
      (void)hipGetLastError();
      hipStreamSynchronize(h->lane_st[z]);
    }
  }
}

// per-block status words: read back, mapped; the call returns the first failure
static int batch_status(ffgp_handle* h, const BatchPlan& b, int* status) {
  if (hipGetLastError() != hipSuccess) return FFGP_ERR_HIP;
  FFGP_HIP(hipMemcpyAsync(h->bt_info_host, h->bt_info, (size_t)b.F * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  FFGP_HIP(hipStreamSynchronize(h->stream));
  if (h->timing) stage_collect(h);
  int first = FFGP_OK;
  for (int f = 0; f < b.F; ++f) {
    const int v = ffgp_map_info(h->bt_info_host[f]);
    if (status) status[f] = v;
    if (v != 0 && first == FFGP_OK) first = v;
  }
  return first;
}

extern "C" {

// ---- F blocks of ONE shape in one chain of launches ----------------------------------------------------------------------------
// The reference's per-fidelity / per-seed loops evaluate independent blocks of equal size one after the other
// (Experiments/GAR_Aligned/exp_aligned.py:58-126, FidelityFusion_Models/ResGP.py:78-112).  Below N ~ 6000 a block's
// factorisation is a dependency chain of a few hundred short launches (32 diagonal blocks x (factor 32 us + solve 11 + update 8) at
// N = 4096: 1.9 of the 2.0 ms); overlapping blocks through streams gives each block its own chain on a shared chip (eight C2 blocks:
// 1.5 ms each).  Here the F blocks sit at a fixed stride in one workspace and every launch of the chain covers all of them -- the
// diagonal-block kernel runs one workgroup per block, the GEMMs carry the block index in gridDim.y -- so F blocks share ONE chain
// and fill its gaps with F times the matrix-core work.  The per-block arithmetic is the single call's, instruction for instruction
// (same kernels, same k order): the values are bit-identical to F separate calls.
// Conditions (else FFGP_ERR_ARG, and the caller falls back to separate calls): 2 <= F <= 256 blocks with n > 128, V1
// likelihood, one radial-profile kernel each (no pair / tree / caller-built covariance), not the naive kernels.
// Round 5: the blocks may have DIFFERENT n and d (the reference's fidelities are ragged by nature, FidelityFusion_Models/ResGP.py:121-136):
// every member follows its own single call's launch sequence and launches of the same kind at the same chain step are merged
// (ffgp_potrf_ragged, ffgp_gemm_launch_rag), members drop out as their columns run out; members above 12288 rows are refused.
// Gradients: the factorisation is shared, the inverse / gradient stages run block after block on the shared scratch.
int ffgp_nlml_fused_batch(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* l, double* nll_dev, const ffgp_grads* g,
                          int* status) {
  if (!h || !p || !nll_dev || F < 2 || F > 256) return FFGP_ERR_ARG;
  if (h->use_naive) return FFGP_ERR_ARG;
  BatchPlan b = {};
  b.F = F; b.p = p; b.l = l; b.g = g; b.nll_dev = nll_dev;
  std::vector<BatchMember> mem(F);
  FFGP_CHECK(batch_validate(h, b, mem));
  FFGP_HIP(hipSetDevice(h->device));
  batch_layout(h, b, mem);
  FFGP_CHECK(ffgp_ensure_ws(h, b.total * sizeof(double)));
  if (!h->bt_info) {
    FFGP_HIP(hipMalloc(&h->bt_info, 256 * sizeof(int)));
    FFGP_HIP(hipHostMalloc(&h->bt_info_host, 256 * sizeof(int)));
  }
  FFGP_CHECK(ffgp_ensure_dinv(h, (int)(b.dinv_blocks * FFGP_NB)));
  FFGP_CHECK(ffgp_zero_async(h, h->bt_info, (size_t)b.F * sizeof(int)));
  h->n_stages = 0;
  stage_mark(h, 0);
  FFGP_CHECK(batch_assemble(h, b, mem));
  stage_mark(h, 1);
  FFGP_CHECK(batch_factor(h, b, mem));
  stage_mark(h, 2);
  b.dinv0 = h->dinv;
  b.main_stream = h->stream;
  int rc = FFGP_OK;
  if (b.all_grad)      // every block's Sigma^-1 from one outer-batched sequence of launches
    rc = ffgp_trtri_lauum_ob(h, F, h->ws, (long)b.blk, mem[0].n, mem[0].ld, h->ws + b.o_X, (long)b.sX, mem[0].ld, h->ws + b.o_T, (long)b.sT,
                             h->ws + b.o_S, (long)b.sX, mem[0].ld, b.dinv0, (long)mem[0].nblk * FFGP_NB * FFGP_NB);
  if (rc == FFGP_OK) rc = batch_reduce(h, b, mem);
  std::vector<int> order(F);
  for (int f = 0; f < F; ++f) order[f] = f;
  if (b.nl > 1 && rc == FFGP_OK) rc = batch_plan_lanes(h, b, mem, order);
  for (int oi = 0; oi < F && rc == FFGP_OK; ++oi)
    if (mem[order[oi]].wants_grad) rc = batch_member_grad(h, b, mem[order[oi]], order[oi]);
  h->dinv = b.dinv0;
  h->dinv_L = nullptr;
  batch_join_lanes(h, b);
  FFGP_CHECK(rc);
  // blocks without gradients of their own inside a gradient batch (forward only: the output scale was applied by the reduction)
  if (l && b.want_grad)
    for (int f = 0; f < F; ++f)
      if (!mem[f].wants_grad) ffgp_links_finish(h, &p[f], &l[f], &g[f], nullptr, false, nll_dev + f);
  stage_mark(h, 3);
  return batch_status(h, b, status);
}

}  // extern "C"
