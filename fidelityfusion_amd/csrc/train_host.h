// The host side of the one-launch trainers, shared by ffgp_train_persist (train.hip) and the tree trainers ffgp_train_tree_lds_raw /
// ffgp_train_tree_lds_res_raw (train_tree_lds.hip, train_tree_lds_res.hip; their one text: train_tree_lds.h).
// A call of either is synchronous and works in ONE device block on the handle, every part at a 256-byte step:
//   [ the driver's tables | 2 steps bias corrections | 2 F status ints ]  <- the head: staged in a pinned mirror, copied up in one piece
//   [ the kernels' per-model scratch ]                                    <- never staged
// A driver takes its tables from a TrainLayout, opens the block (train_block_open: the rest of the layout, growth, bias corrections,
// the loop's arguments), fills its tables in the mirror, copies the head up, launches (tr_by_dm + train_launch) and finishes
// (train_block_finish).  A new trainer variant is a kernel and a member description on top of this.
#pragma once
#include <algorithm>
#include <type_traits>

#include "drivers.h"
#include "train_tile.h"

// offsets of the block's parts, handed out in order, each at the next 256-byte step
struct TrainLayout {
  size_t size = 0;
  size_t take(size_t bytes) { return (size = (size + 255) / 256 * 256 + bytes) - bytes; }
};
struct TrainBlock {
  char* host;                 // the pinned mirror of the head
  char* dev;                  // the device block
  size_t head, info_off, scratch_off;
  TrainLoop loop;             // (bc, info, fail_step point into dev)
};

// The handle's block holds `need` bytes and its mirror `head`: grown behind the stream's work (the call before was synchronous, so
// nothing of ours is in flight; the stream may be shared), never shrunk.  The mirror is sized from the head, which grows with the
// steps: at least 64 KiB, so that a short first call does not make the next, longer one allocate again (0.3 ms).  alloc_epoch stays
// out of it: no captured graph holds these pointers.
static inline int train_block_grow(ffgp_handle* h, size_t need, size_t head) {
  if (need <= h->train_blk_bytes && head <= h->train_blk_host_bytes) return FFGP_OK;
  FFGP_HIP(hipStreamSynchronize(h->stream));
  const size_t cap = std::max(h->train_blk_bytes, need + need / 2), hcap = std::max({h->train_blk_host_bytes, 2 * head, (size_t)65536});
  if (h->train_blk) hipFree(h->train_blk);
  if (h->train_blk_host) hipHostFree(h->train_blk_host);
  h->train_blk = h->train_blk_host = nullptr;
  h->train_blk_bytes = h->train_blk_host_bytes = 0;
  if (hipMalloc(&h->train_blk, cap) != hipSuccess || hipHostMalloc(&h->train_blk_host, hcap, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    if (h->train_blk) hipFree(h->train_blk);
    h->train_blk = nullptr;
    return FFGP_ERR_ALLOC;
  }
  h->train_blk_bytes = cap;
  h->train_blk_host_bytes = hcap;
  return FFGP_OK;
}

// `lay` holds the driver's tables.  Adds the bias corrections, the status words and scratch_bytes of scratch, makes room, zeroes the
// mirror's head, fills the bias corrections there and the loop's arguments in b->loop.
static inline int train_block_open(ffgp_handle* h, TrainLayout lay, int F, int steps, const ffgp_adam* opt, long step0, size_t scratch_bytes,
                                   TrainBlock* b) {
  const size_t bc_off = lay.take((size_t)2 * steps * sizeof(double));
  b->info_off = lay.take((size_t)2 * F * sizeof(int));
  b->head = lay.size;
  b->scratch_off = lay.take(scratch_bytes);
  FFGP_CHECK(train_block_grow(h, lay.size, b->head));
  b->host = reinterpret_cast<char*>(h->train_blk_host);
  b->dev = reinterpret_cast<char*>(h->train_blk);
  memset(b->host, 0, b->head);
  ffgp_adam_bc_table(opt, step0, steps, reinterpret_cast<double*>(b->host + bc_off));
  TrainLoop& c = b->loop;
  c.steps = steps; c.lr = opt->lr; c.b1 = opt->beta1; c.b2 = opt->beta2; c.eps = opt->eps;
  c.bc = reinterpret_cast<const double*>(b->dev + bc_off);
  c.info = reinterpret_cast<int*>(b->dev + b->info_off);
  c.fail_step = c.info + F;
  return FFGP_OK;
}

// the template class of the call's largest input dimension: f(std::integral_constant<int, DM>) with DM = 8 or 16
template <class Fn>
static int tr_by_dm(int Dmax, Fn f) {
  if (Dmax <= 8) return f(std::integral_constant<int, 8>());
  return f(std::integral_constant<int, 16>());
}
// One launch of `grid` models, TR_T threads each, with lds_bytes of dynamic LDS.  The attribute is set on every call, as acq_launch
// (acq_tile.h) does and for its reason: it belongs to the current device, and a host-side "already set" table would be state shared
// between handles -- train_many trains from several host threads.
template <class... P, class... A>
static int train_launch(ffgp_handle* h, void (*kernel)(P...), size_t lds_bytes, int grid, const A&... a) {
  FFGP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(TR_T), lds_bytes, h->stream, a...);
  return hipGetLastError() == hipSuccess ? FFGP_OK : FFGP_ERR_HIP;
}

// The call's end: the 2 F status ints into the mirror, the wait, and 0 or the pivot status of the first model -- in the caller's
// order: model f's status word is row pos[f] (null: row f) -- whose Sigma was not positive definite at some step.
static inline int train_block_finish(ffgp_handle* h, const TrainBlock& b, int F, const int* pos) {
  const int* st = reinterpret_cast<const int*>(b.host + b.info_off);
  FFGP_HIP(hipMemcpyAsync(b.host + b.info_off, b.loop.info, (size_t)2 * F * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  FFGP_HIP(hipStreamSynchronize(h->stream));
  ffgp_invalidate(h);
  for (int f = 0; f < F; ++f)
    if (st[pos ? pos[f] : f] != 0) return st[pos ? pos[f] : f];
  return FFGP_OK;
}
