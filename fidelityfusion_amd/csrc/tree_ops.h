// The canonical Sum / Product trees of include/ffgp.h (2-4 leaves) on the leaves' values, for the kernels that evaluate a composed kernel
// entry by entry in registers: the acquisition loop (acq_tree.hip) and the one-launch trainers (ttl_body, train_tree_lds.h).  A: any struct with
// nl, shape and op[3] (FFGP_KOP_*; shape = FFGP_TREE_CHAIN | FFGP_TREE_BALANCED, read at nl = 4).  At the end, the hosts' checks of a tree.
#pragma once
#include "ffgp_internal.h"

#define FFGP_TREE_LEAVES 4

// one node: separately rounded product / sum (pair.hip's tree_op)
__device__ __forceinline__ double ffgp_tree_op(int op, double x, double y) {
#pragma clang fp contract(off)
  const double pr = x * y, sm = x + y;
  return op == FFGP_KOP_PRODUCT ? pr : sm;
}
// the canonical trees of include/ffgp.h on the leaves' values (v[e] = 0 past the last leaf)
template <class A>
__device__ __forceinline__ double ffgp_tree_eval(const A& a, const double (&v)[FFGP_TREE_LEAVES]) {
  const double t0 = ffgp_tree_op(a.op[0], v[0], v[1]);
  if (a.nl == 2) return t0;
  if (a.nl == 3) return ffgp_tree_op(a.op[1], t0, v[2]);
  if (a.shape == FFGP_TREE_BALANCED) return ffgp_tree_op(a.op[2], t0, ffgp_tree_op(a.op[1], v[2], v[3]));
  return ffgp_tree_op(a.op[2], ffgp_tree_op(a.op[1], t0, v[2]), v[3]);
}
// d root / d leaf values (pair.hip's tree_back with upstream 1)
template <class A>
__device__ __forceinline__ void ffgp_tree_back(const A& a, const double (&v)[FFGP_TREE_LEAVES], double (&gv)[FFGP_TREE_LEAVES]) {
  const double t0 = ffgp_tree_op(a.op[0], v[0], v[1]);
  double gt0 = 1.0;
  gv[2] = 0.0;
  gv[3] = 0.0;
  if (a.nl == 3) {
    const bool pr = a.op[1] == FFGP_KOP_PRODUCT;
    gt0 = pr ? v[2] : 1.0;
    gv[2] = pr ? t0 : 1.0;
  }
  if (a.nl == 4) {
    const bool p1 = a.op[1] == FFGP_KOP_PRODUCT, p2 = a.op[2] == FFGP_KOP_PRODUCT;
    if (a.shape == FFGP_TREE_BALANCED) {
      const double t1 = ffgp_tree_op(a.op[1], v[2], v[3]);
      gt0 = p2 ? t1 : 1.0;
      const double gt1 = p2 ? t0 : 1.0;
      gv[2] = p1 ? gt1 * v[3] : gt1;
      gv[3] = p1 ? gt1 * v[2] : gt1;
    } else {
      const double t1 = ffgp_tree_op(a.op[1], t0, v[2]);
      const double gt1 = p2 ? v[3] : 1.0;
      gv[3] = p2 ? t1 : 1.0;
      gt0 = p1 ? gt1 * v[2] : gt1;
      gv[2] = p1 ? gt1 * t0 : gt1;
    }
  }
  const bool p0 = a.op[0] == FFGP_KOP_PRODUCT;
  gv[0] = p0 ? gt0 * v[1] : gt0;
  gv[1] = p0 ? gt0 * v[0] : gt0;
}

// ---- the host side: what every entry that is handed an ffgp_ktree (not null) refuses about its form -- 2-4 leaves, one of the two
//      shapes at four, Sum / Product nodes -- and what the tree trainers refuse about a leaf they are to train
static inline bool ffgp_tree_form_ok(const ffgp_ktree* t) {
  if (!t->leaf || t->n_leaves < 2 || t->n_leaves > FFGP_TREE_LEAVES) return false;
  if (t->n_leaves == 4 && t->shape != FFGP_TREE_CHAIN && t->shape != FFGP_TREE_BALANCED) return false;
  for (int i = 0; i + 1 < t->n_leaves; ++i)
    if (t->op[i] != FFGP_KOP_SUM && t->op[i] != FFGP_KOP_PRODUCT) return false;
  return true;
}
static inline bool ffgp_tree_leaf_trainable(const ffgp_kdesc& k, const ffgp_leaf_links& ll) {
  const bool linear = (k.kfun == FFGP_KFUN_LINEAR);
  if (!k.w_dev || !k.amp_dev || !(linear || (k.kfun >= FFGP_KFUN_SE && k.kfun <= FFGP_KFUN_MATERN52))) return false;
  return !ll.center_train || (linear && k.center_dev);
}
