// ffgp_train_tree_lds_raw's job with the FFGP_LL_V2 likelihood and with RESIDUAL members -- train_AR's fidelities above 0 and GP_basic
// blocks on a composed kernel, n <= 128 -- in ONE launch per likelihood class: ffgp_train_tree_lds_res_raw (include/ffgp.h).  The
// persistent workgroup's step loop is train_tree_lds.h's ttl_body, instantiated here with RESID (a member whose rho is set re-forms its
// targets r = y_high - rho y_low and its diagonal extra |v_high - rho v_low| at the top of every step, the variances as two [128] rows
// in LDS behind the plain members' layout, and trains rho as parameter P) and with V2 (B = Sigma^-1 A by the two block chains once
// more, G = d/2 Sigma^-1 - 1/2 (A B^T + B A^T)).  V1 and V2 members of one call get a launch each, class after class, as in
// ffgp_train_persist; plain and residual members share a launch.  Host side: train_host.h's scaffold.
#include "train_tree_lds.h"

template <int DM, bool V2>
__global__ __launch_bounds__(TR_T) void ffgp_train_tree_lds_res_kernel(const TtlResModel* __restrict__ tab, TtlCommon cm) {
  ttl_body<DM, V2, true>(tab, cm);
}

extern "C" int ffgp_train_tree_lds_res_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_tree_links* l, const ffgp_residual* r,
                                           int steps, const ffgp_adam* opt, double* state_dev, long state_stride, long step0,
                                           double* trace_dev, long trace_stride) {
  if (!ffgp_train_args_ok(h, p, l, opt, state_dev, trace_dev, F, steps, step0, trace_stride)) return FFGP_ERR_ARG;
  TtlResModel tm[FFGP_TRAIN_MAXF];
  int pos[FFGP_TRAIN_MAXF], nv[2] = {0, 0}, Dmax[2] = {0, 0};
  // two classes of members, a launch each: V1, then V2.  pos[f] = model f's row of the table and of the status words
  for (int f = 0; f < F; ++f) nv[p[f].ll_variant == FFGP_LL_V2 ? 1 : 0]++;
  {
    int q[2] = {0, nv[0]};
    for (int f = 0; f < F; ++f) pos[f] = q[p[f].ll_variant == FFGP_LL_V2 ? 1 : 0]++;
  }
  for (int f = 0; f < F; ++f) {      // (every member is checked before anything is allocated or enqueued)
    const bool res = r && r[f].rho_dev;
    if (res && (!r[f].y_low_dev || !r[f].y_high_dev || (!r[f].v_low_dev) != (!r[f].v_high_dev) ||
                (r[f].v_low_dev && (r[f].v_low_stride < 0 || r[f].v_high_stride < 0))))
      return FFGP_ERR_ARG;
    TtlResModel& m = tm[pos[f]];
    if (!ttl_describe(p[f], l[f], state_stride, m, true, res)) return FFGP_ERR_ARG;
    m.rho = res ? r[f].rho_dev : nullptr;
    m.y_low = res ? r[f].y_low_dev : nullptr; m.y_high = res ? r[f].y_high_dev : nullptr;
    m.v_low = res ? r[f].v_low_dev : nullptr; m.v_high = res ? r[f].v_high_dev : nullptr;
    m.v_low_stride = res ? r[f].v_low_stride : 0; m.v_high_stride = res ? r[f].v_high_stride : 0;
    m.rho_last = res ? r[f].rho_last_dev : nullptr;
    if (res) { m.Y = nullptr; m.diag_vec = nullptr; }      // (ignored for a residual member)
    const int k = p[f].ll_variant == FFGP_LL_V2 ? 1 : 0;
    Dmax[k] = std::max(Dmax[k], p[f].D);
  }
  FFGP_HIP(hipSetDevice(h->device));
  TrainLayout lay;
  const size_t tab_off = lay.take((size_t)F * sizeof(TtlResModel));
  TrainBlock blk;
  FFGP_CHECK(train_block_open(h, lay, F, steps, opt, step0, (size_t)F * TTL_WBUF * sizeof(double), &blk));
  for (int f = 0; f < F; ++f) {
    TtlResModel& m = tm[pos[f]];
    m.state = state_dev + (size_t)f * state_stride;
    m.trace = trace_dev + (size_t)f * trace_stride;
    m.wbuf = reinterpret_cast<double*>(blk.dev + blk.scratch_off) + (size_t)pos[f] * TTL_WBUF;
  }
  memcpy(blk.host + tab_off, tm, (size_t)F * sizeof(TtlResModel));
  FFGP_HIP(hipMemcpyAsync(blk.dev, blk.host, blk.head, hipMemcpyHostToDevice, h->stream));
  const TtlResModel* tab = reinterpret_cast<const TtlResModel*>(blk.dev + tab_off);
  for (int k = 0; k < 2; ++k) {
    if (!nv[k]) continue;
    const int row0 = k ? nv[0] : 0;
    TtlCommon cm;
    static_cast<TrainLoop&>(cm) = blk.loop;
    cm.info += row0;
    cm.fail_step += row0;
    FFGP_CHECK(tr_by_dm(Dmax[k], [&](auto dm) {
      if (k) return train_launch(h, ffgp_train_tree_lds_res_kernel<dm(), true>, TTL_RES_LDS_DOUBLES * sizeof(double), nv[k], tab + row0, cm);
      return train_launch(h, ffgp_train_tree_lds_res_kernel<dm(), false>, TTL_RES_LDS_DOUBLES * sizeof(double), nv[k], tab + row0, cm);
    }));
  }
  return train_block_finish(h, blk, F, pos);
}
