// The host side that the one-launch prediction entries share: ffgp_predict_small_batch (predict_small.hip, one radial kernel per member)
// and ffgp_predict_small_tree_batch (predict_small_tree.hip, a Sum / Product tree per member).  Both launch a grid (F, S) of TR_T
// threads, keep their table and status words in the handle's train block (train_host.h) and end the same way.
#pragma once
#include "train_host.h"

static_assert(FFGP_PREDICT_SMALL_MAX_N == TR_N && FFGP_PREDICT_SMALL_MAX_D == TR_D && FFGP_PREDICT_SMALL_MAX_d == TR_Y, "the header's limits are the trainer's images");

// what both entries ask of a member's sizes and of its test points and outputs
static inline bool ps_sizes_ok(const ffgp_problem& q, const ffgp_predict_member& m) {
  if (q.n <= 0 || q.n > FFGP_PREDICT_SMALL_MAX_N || q.D <= 0 || q.D > FFGP_PREDICT_SMALL_MAX_D || q.d <= 0 || q.d > FFGP_PREDICT_SMALL_MAX_d) return false;
  return m.Xs_dev && m.mean_dev && m.var_dev && m.nt >= 1;
}

// S: enough workgroups for the chip's 256 CUs when the models alone do not fill it, never more than the largest member has tiles
// (FFGP_PREDICT_SPLIT=k in the environment, read at every call, forces S = min(k, tiles): for tests)
static inline int ps_split(int F, int tiles) {
  int split = std::min(tiles, std::max(1, 256 / F));
  if (const char* e = getenv("FFGP_PREDICT_SPLIT"))
    if (atoi(e) > 0) split = std::min(tiles, atoi(e));
  return split;
}

// the status words back (the models' parameters did not move: the handle's cached factors stay valid); the first non-zero one
static inline int ps_finish(ffgp_handle* h, const TrainBlock& blk, int F, int* status) {
  int* st = reinterpret_cast<int*>(blk.host + blk.info_off);
  FFGP_HIP(hipMemcpyAsync(st, blk.loop.info, (size_t)F * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  FFGP_HIP(hipStreamSynchronize(h->stream));
  int rc = FFGP_OK;
  for (int f = 0; f < F; ++f) {
    if (status) status[f] = st[f];
    if (rc == FFGP_OK && st[f] != 0) rc = st[f];
  }
  return rc;
}
