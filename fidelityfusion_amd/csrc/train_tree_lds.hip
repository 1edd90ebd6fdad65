// K Adam steps of F composed-kernel models -- SumKernel / ProductKernel trees of 2-4 leaves (ffgp_ktree) -- in ONE launch:
// ffgp_train_tree_lds_raw (include/ffgp.h): one PERSISTENT workgroup per model (gridDim.x = models, 512 threads) runs every step inside the
// kernel.  The step loop, its phases, the LDS layout and the member description are train_tree_lds.h's (ttl_body, ttl_describe); this unit
// instantiates the body for plain V1 members -- no V2 block chains, no residual link -- and keeps the entry, which refuses V2
// (ffgp_train_tree_lds_res_raw, train_tree_lds_res.hip, trains those).  Host side: train_host.h's scaffold.
#include "train_tree_lds.h"

// DM: the input dimensions the per-entry loops are unrolled for (8 or 16: every model of the launch has D <= DM)
template <int DM>
__global__ __launch_bounds__(TR_T) void ffgp_train_tree_lds_kernel(const TtlModel* __restrict__ tab, TtlCommon cm) {
  ttl_body<DM, false, false>(tab, cm);
}

extern "C" int ffgp_train_tree_lds_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_tree_links* l, int steps, const ffgp_adam* opt,
                                       double* state_dev, long state_stride, long step0, double* trace_dev, long trace_stride) {
  if (!ffgp_train_args_ok(h, p, l, opt, state_dev, trace_dev, F, steps, step0, trace_stride)) return FFGP_ERR_ARG;
  TtlModel tm[FFGP_TRAIN_MAXF];
  int Dmax = 0;
  for (int f = 0; f < F; ++f) {      // (every member is checked before anything is allocated or enqueued)
    if (!ttl_describe(p[f], l[f], state_stride, tm[f])) return FFGP_ERR_ARG;
    Dmax = std::max(Dmax, p[f].D);
  }
  FFGP_HIP(hipSetDevice(h->device));
  // the call's block (train_host.h); the table: F models, the scratch: F x TTL_WBUF weights
  TrainLayout lay;
  const size_t tab_off = lay.take((size_t)F * sizeof(TtlModel));
  TrainBlock blk;
  FFGP_CHECK(train_block_open(h, lay, F, steps, opt, step0, (size_t)F * TTL_WBUF * sizeof(double), &blk));
  for (int f = 0; f < F; ++f) {
    tm[f].state = state_dev + (size_t)f * state_stride;
    tm[f].trace = trace_dev + (size_t)f * trace_stride;
    tm[f].wbuf = reinterpret_cast<double*>(blk.dev + blk.scratch_off) + (size_t)f * TTL_WBUF;
  }
  memcpy(blk.host + tab_off, tm, (size_t)F * sizeof(TtlModel));
  FFGP_HIP(hipMemcpyAsync(blk.dev, blk.host, blk.head, hipMemcpyHostToDevice, h->stream));
  TtlCommon cm;
  static_cast<TrainLoop&>(cm) = blk.loop;
  const TtlModel* tab = reinterpret_cast<const TtlModel*>(blk.dev + tab_off);
  FFGP_CHECK(tr_by_dm(Dmax, [&](auto dm) {
    return train_launch(h, ffgp_train_tree_lds_kernel<dm()>, TTL_LDS_DOUBLES * sizeof(double), F, tab, cm);
  }));
  return train_block_finish(h, blk, F, nullptr);      // (the table is in the caller's order)
}
