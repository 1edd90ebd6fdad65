// Host-side AddressSanitizer walk of libffgp's launch / bookkeeping code (make asan; CPU box only).
// Without a GPU every entry point must fail cleanly: ffgp_create reports FFGP_ERR_NODEVICE and leaves *out untouched,
// a NULL handle is FFGP_ERR_ARG everywhere, ffgp_destroy(NULL) is a no-op.  With a GPU visible the same binary also
// runs one small fused NLML so that the workspace bookkeeping (grow, reuse, destroy) is walked under ASAN's allocator.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ffgp.h"

#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::fprintf(stderr, "asan_host_check: %s failed (line %d)\n", #cond, __LINE__); \
      return 1;                                                               \
    }                                                                         \
  } while (0)

int main() {
  EXPECT(std::strstr(ffgp_version(), "ffgp") != nullptr);
  EXPECT(ffgp_create(0, nullptr) == FFGP_ERR_ARG);
  EXPECT(ffgp_destroy(nullptr) == FFGP_OK);
  ffgp_handle* h = reinterpret_cast<ffgp_handle*>(0x1);   // must come back untouched when there is no device
  const int rc = ffgp_create(0, &h);
  if (rc == FFGP_ERR_NODEVICE) {
    EXPECT(h == reinterpret_cast<ffgp_handle*>(0x1));
    EXPECT(ffgp_create(-1, &h) == FFGP_ERR_NODEVICE);
    // NULL-handle argument checks never dereference
    double x = 0.0;
    ffgp_problem p;
    std::memset(&p, 0, sizeof p);
    EXPECT(ffgp_set_option(nullptr, "timing", 1.0) < 0);
    EXPECT(ffgp_set_stream(nullptr, nullptr) < 0);
    EXPECT(ffgp_potrf(nullptr, &x, 1, 2) < 0);
    EXPECT(ffgp_nlml_fused(nullptr, &p, &x, nullptr) < 0);
    EXPECT(ffgp_wait(nullptr) < 0);
    // round 5: the batched / ragged likelihood and the K-steps-per-call training entry refuse a NULL handle before touching anything
    ffgp_links lk;
    std::memset(&lk, 0, sizeof lk);
    ffgp_adam ad = {1e-2, 0.9, 0.999, 1e-8};
    int st[2] = {0, 0};
    EXPECT(ffgp_nlml_fused_batch(nullptr, 2, &p, &lk, &x, nullptr, st) < 0);
    EXPECT(ffgp_train_raw(nullptr, 1, &p, &lk, 3, &ad, &x, 8, 0, &x, 3) < 0);
    ffgp_residual rs;
    std::memset(&rs, 0, sizeof rs);
    EXPECT(ffgp_train_residual_raw(nullptr, 1, &p, &lk, &rs, 3, &ad, &x, 8, 0, &x, 3) < 0);
    // the tensor-linear trainer: a NULL handle, and with a handle that must never be dereferenced the link's own refusals
    {
      ffgp_handle* fk = reinterpret_cast<ffgp_handle*>(0x1);
      ffgp_problem pt;
      std::memset(&pt, 0, sizeof pt);
      pt.n = 8; pt.D = 2; pt.d = 3; pt.X_dev = pt.w_dev = pt.amp_dev = pt.diag_add_dev = &x;
      pt.kfun = FFGP_KFUN_SE; pt.kparam = 1.0; pt.ll_variant = FFGP_LL_V1;
      ffgp_tlin_link tk;
      std::memset(&tk, 0, sizeof tk);
      tk.V_dev = &x; tk.l = 2; tk.y_low_dev = tk.y_high_dev = &x;
      EXPECT(ffgp_train_tlin_raw(nullptr, 1, &pt, &lk, &tk, 3, &ad, &x, 20, 0, &x, 3) < 0);
      EXPECT(ffgp_train_tlin_raw(fk, 1, &pt, &lk, nullptr, 3, &ad, &x, 20, 0, &x, 3) == FFGP_ERR_ARG);
      EXPECT(ffgp_train_tlin_raw(fk, 1, &pt, &lk, &tk, 3, &ad, &x, 19, 0, &x, 3) == FFGP_ERR_ARG);      // state_stride < 2 (D + 2 + h l)
      tk.l = 4;      // l > h
      EXPECT(ffgp_train_tlin_raw(fk, 1, &pt, &lk, &tk, 3, &ad, &x, 20, 0, &x, 3) == FFGP_ERR_ARG);
      tk.l = 2; tk.y_low_dev = nullptr;
      EXPECT(ffgp_train_tlin_raw(fk, 1, &pt, &lk, &tk, 3, &ad, &x, 20, 0, &x, 3) == FFGP_ERR_ARG);
      tk.y_low_dev = &x; tk.V_row_stride = -1;
      EXPECT(ffgp_train_tlin_raw(fk, 1, &pt, &lk, &tk, 3, &ad, &x, 20, 0, &x, 3) == FFGP_ERR_ARG);
      tk.V_row_stride = 0; pt.ll_variant = FFGP_LL_V2;
      EXPECT(ffgp_train_tlin_raw(fk, 1, &pt, &lk, &tk, 3, &ad, &x, 20, 0, &x, 3) == FFGP_ERR_ARG);
    }
    // the wide-output one-launch trainer: every refusal comes before the handle is dereferenced or anything is enqueued
    {
      ffgp_handle* fk = reinterpret_cast<ffgp_handle*>(0x1);
      ffgp_problem pw;
      std::memset(&pw, 0, sizeof pw);
      pw.n = 8; pw.D = 2; pw.d = 8; pw.X_dev = pw.Y_dev = pw.w_dev = pw.amp_dev = pw.diag_add_dev = &x;
      pw.kfun = FFGP_KFUN_SE; pw.kparam = 1.0; pw.ll_variant = FFGP_LL_V1;
      int dt = 40, inf = 7;
      EXPECT(ffgp_train_wide_raw(nullptr, 1, &pw, &lk, nullptr, &dt, 3, &ad, &x, 8, 0, &x, 3, &inf) == FFGP_ERR_ARG);
      EXPECT(ffgp_train_wide_raw(fk, 1, &pw, &lk, nullptr, nullptr, 3, &ad, &x, 8, 0, &x, 3, &inf) == FFGP_ERR_ARG);
      EXPECT(ffgp_train_wide_raw(fk, 17, &pw, &lk, nullptr, &dt, 3, &ad, &x, 8, 0, &x, 3, &inf) == FFGP_ERR_ARG);
      EXPECT(ffgp_train_wide_raw(fk, 1, &pw, &lk, nullptr, &dt, 3, &ad, &x, 8, 0, &x, 2, &inf) == FFGP_ERR_ARG);      // trace_stride < steps
      EXPECT(ffgp_train_wide_raw(fk, 1, &pw, &lk, nullptr, &dt, 3, &ad, &x, 7, 0, &x, 3, &inf) == FFGP_ERR_ARG);      // state_stride < 2 (D + 2)
      dt = 16;      // not a wide model
      EXPECT(ffgp_train_wide_raw(fk, 1, &pw, &lk, nullptr, &dt, 3, &ad, &x, 8, 0, &x, 3, &inf) == FFGP_ERR_ARG);
      dt = 40; pw.d = 41;      // more columns passed than the likelihood has
      EXPECT(ffgp_train_wide_raw(fk, 1, &pw, &lk, nullptr, &dt, 3, &ad, &x, 8, 0, &x, 3, &inf) == FFGP_ERR_ARG);
      dt = 400; pw.d = 129;      // a plain member passes at most 128 columns
      EXPECT(ffgp_train_wide_raw(fk, 1, &pw, &lk, nullptr, &dt, 3, &ad, &x, 8, 0, &x, 3, &inf) == FFGP_ERR_ARG);
      pw.d = 8; pw.n = 129;
      EXPECT(ffgp_train_wide_raw(fk, 1, &pw, &lk, nullptr, &dt, 3, &ad, &x, 8, 0, &x, 3, &inf) == FFGP_ERR_ARG);
      pw.n = 8; pw.D = 17;
      EXPECT(ffgp_train_wide_raw(fk, 1, &pw, &lk, nullptr, &dt, 3, &ad, &x, 40, 0, &x, 3, &inf) == FFGP_ERR_ARG);
      pw.D = 2; pw.ll_variant = FFGP_LL_V2;
      EXPECT(ffgp_train_wide_raw(fk, 1, &pw, &lk, nullptr, &dt, 3, &ad, &x, 8, 0, &x, 3, &inf) == FFGP_ERR_ARG);
      pw.ll_variant = FFGP_LL_V1; pw.kfun = FFGP_KFUN_RQ;
      EXPECT(ffgp_train_wide_raw(fk, 1, &pw, &lk, nullptr, &dt, 3, &ad, &x, 8, 0, &x, 3, &inf) == FFGP_ERR_ARG);
      pw.kfun = FFGP_KFUN_SE; pw.cov_dev = &x;
      EXPECT(ffgp_train_wide_raw(fk, 1, &pw, &lk, nullptr, &dt, 3, &ad, &x, 8, 0, &x, 3, &inf) == FFGP_ERR_ARG);
      pw.cov_dev = nullptr;
      ffgp_residual rw;
      std::memset(&rw, 0, sizeof rw);
      rw.rho_dev = &x; rw.y_low_dev = &x;      // a residual member without y_high
      EXPECT(ffgp_train_wide_raw(fk, 1, &pw, &lk, &rw, &dt, 3, &ad, &x, 10, 0, &x, 3, &inf) == FFGP_ERR_ARG);
      rw.y_high_dev = &x; rw.v_low_dev = &x;      // one variance diagonal without the other
      EXPECT(ffgp_train_wide_raw(fk, 1, &pw, &lk, &rw, &dt, 3, &ad, &x, 10, 0, &x, 3, &inf) == FFGP_ERR_ARG);
      rw.v_low_dev = nullptr;      // rho is a fourth parameter: the state holds 2 (D + 3)
      EXPECT(ffgp_train_wide_raw(fk, 1, &pw, &lk, &rw, &dt, 3, &ad, &x, 8, 0, &x, 3, &inf) == FFGP_ERR_ARG);
      EXPECT(inf == 7);      // (a refused call writes nothing)
    }
    // the batched prediction: every refusal comes before the handle is dereferenced or anything is enqueued or written
    {
      ffgp_handle* fk = reinterpret_cast<ffgp_handle*>(0x1);
      ffgp_problem pp;
      std::memset(&pp, 0, sizeof pp);
      pp.n = 8; pp.D = 2; pp.d = 3; pp.X_dev = pp.Y_dev = pp.w_dev = pp.amp_dev = pp.diag_add_dev = &x;
      pp.kfun = FFGP_KFUN_SE; pp.kparam = 1.0;
      double out[2] = {7.0, 7.0};
      ffgp_predict_member pm = {&x, 5, &out[0], &out[1], 1};
      int sp = 7;
      EXPECT(ffgp_predict_small_batch(nullptr, 1, &pp, &lk, &pm, &sp) == FFGP_ERR_ARG);
      EXPECT(ffgp_predict_small_batch(fk, 1, nullptr, &lk, &pm, &sp) == FFGP_ERR_ARG);
      EXPECT(ffgp_predict_small_batch(fk, 1, &pp, &lk, nullptr, &sp) == FFGP_ERR_ARG);
      EXPECT(ffgp_predict_small_batch(fk, 0, &pp, &lk, &pm, &sp) == FFGP_ERR_ARG);
      EXPECT(ffgp_predict_small_batch(fk, FFGP_PREDICT_SMALL_MAX_F + 1, &pp, &lk, &pm, &sp) == FFGP_ERR_ARG);
      pm.nt = 0;
      EXPECT(ffgp_predict_small_batch(fk, 1, &pp, nullptr, &pm, &sp) == FFGP_ERR_ARG);
      pm.nt = 5; pm.mean_dev = nullptr;
      EXPECT(ffgp_predict_small_batch(fk, 1, &pp, nullptr, &pm, &sp) == FFGP_ERR_ARG);
      pm.mean_dev = &out[0]; pm.Xs_dev = nullptr;
      EXPECT(ffgp_predict_small_batch(fk, 1, &pp, nullptr, &pm, &sp) == FFGP_ERR_ARG);
      pm.Xs_dev = &x; pp.n = FFGP_PREDICT_SMALL_MAX_N + 1;
      EXPECT(ffgp_predict_small_batch(fk, 1, &pp, &lk, &pm, &sp) == FFGP_ERR_ARG);
      pp.n = 8; pp.D = FFGP_PREDICT_SMALL_MAX_D + 1;
      EXPECT(ffgp_predict_small_batch(fk, 1, &pp, &lk, &pm, &sp) == FFGP_ERR_ARG);
      pp.D = 2; pp.d = FFGP_PREDICT_SMALL_MAX_d + 1;
      EXPECT(ffgp_predict_small_batch(fk, 1, &pp, &lk, &pm, &sp) == FFGP_ERR_ARG);
      pp.d = 3; pp.diag_vec_dev = &x;      // the predict paths drop y_var
      EXPECT(ffgp_predict_small_batch(fk, 1, &pp, &lk, &pm, &sp) == FFGP_ERR_ARG);
      pp.diag_vec_dev = nullptr; pp.add_all = 0.5;
      EXPECT(ffgp_predict_small_batch(fk, 1, &pp, &lk, &pm, &sp) == FFGP_ERR_ARG);
      pp.add_all = 0.0; pp.kfun = FFGP_KFUN_RQ + 1;
      EXPECT(ffgp_predict_small_batch(fk, 1, &pp, &lk, &pm, &sp) == FFGP_ERR_ARG);
      pp.kfun = FFGP_KFUN_SE; pp.Y_dev = nullptr;
      EXPECT(ffgp_predict_small_batch(fk, 1, &pp, &lk, &pm, &sp) == FFGP_ERR_ARG);
      EXPECT(sp == 7 && out[0] == 7.0 && out[1] == 7.0);      // (a refused call writes nothing)
    }
    // ... and its composed-kernel form: the same refusals, and those about the tree
    {
      ffgp_handle* fk = reinterpret_cast<ffgp_handle*>(0x1);
      ffgp_kdesc lf[5];
      std::memset(lf, 0, sizeof lf);
      for (auto& k : lf) { k.kfun = FFGP_KFUN_MATERN52; k.w_dev = k.amp_dev = &x; k.kparam = 1.0; }
      lf[0].kfun = FFGP_KFUN_LINEAR; lf[0].center_dev = &x;
      ffgp_ktree tq;
      std::memset(&tq, 0, sizeof tq);
      tq.n_leaves = 2; tq.leaf = lf;
      ffgp_tree_links tlk;
      std::memset(&tlk, 0, sizeof tlk);
      ffgp_problem pp;
      std::memset(&pp, 0, sizeof pp);
      pp.n = 8; pp.D = 2; pp.d = 3; pp.X_dev = pp.Y_dev = pp.diag_add_dev = &x;
      pp.tree = &tq;
      double out[2] = {7.0, 7.0};
      ffgp_predict_member pm = {&x, 5, &out[0], &out[1], 1};
      int sp = 7;
      EXPECT(ffgp_predict_small_tree_batch(nullptr, 1, &pp, &tlk, &pm, &sp) == FFGP_ERR_ARG);
      EXPECT(ffgp_predict_small_tree_batch(fk, 1, nullptr, &tlk, &pm, &sp) == FFGP_ERR_ARG);
      EXPECT(ffgp_predict_small_tree_batch(fk, 1, &pp, &tlk, nullptr, &sp) == FFGP_ERR_ARG);
      EXPECT(ffgp_predict_small_tree_batch(fk, 0, &pp, &tlk, &pm, &sp) == FFGP_ERR_ARG);
      EXPECT(ffgp_predict_small_tree_batch(fk, FFGP_PREDICT_SMALL_MAX_F + 1, &pp, &tlk, &pm, &sp) == FFGP_ERR_ARG);
      pm.nt = 0;
      EXPECT(ffgp_predict_small_tree_batch(fk, 1, &pp, nullptr, &pm, &sp) == FFGP_ERR_ARG);
      pm.nt = 5; pm.var_dev = nullptr;
      EXPECT(ffgp_predict_small_tree_batch(fk, 1, &pp, nullptr, &pm, &sp) == FFGP_ERR_ARG);
      pm.var_dev = &out[1]; pp.n = FFGP_PREDICT_SMALL_MAX_N + 1;
      EXPECT(ffgp_predict_small_tree_batch(fk, 1, &pp, &tlk, &pm, &sp) == FFGP_ERR_ARG);
      pp.n = 8; pp.D = FFGP_PREDICT_SMALL_MAX_D + 1;
      EXPECT(ffgp_predict_small_tree_batch(fk, 1, &pp, &tlk, &pm, &sp) == FFGP_ERR_ARG);
      pp.D = 2; pp.d = FFGP_PREDICT_SMALL_MAX_d + 1;
      EXPECT(ffgp_predict_small_tree_batch(fk, 1, &pp, &tlk, &pm, &sp) == FFGP_ERR_ARG);
      pp.d = 3; pp.tree = nullptr;
      EXPECT(ffgp_predict_small_tree_batch(fk, 1, &pp, &tlk, &pm, &sp) == FFGP_ERR_ARG);
      pp.tree = &tq; tq.n_leaves = 5;
      EXPECT(ffgp_predict_small_tree_batch(fk, 1, &pp, &tlk, &pm, &sp) == FFGP_ERR_ARG);
      tq.n_leaves = 4; tq.shape = 2;
      EXPECT(ffgp_predict_small_tree_batch(fk, 1, &pp, &tlk, &pm, &sp) == FFGP_ERR_ARG);
      tq.shape = FFGP_TREE_BALANCED; tq.op[1] = 2;
      EXPECT(ffgp_predict_small_tree_batch(fk, 1, &pp, &tlk, &pm, &sp) == FFGP_ERR_ARG);
      tq.op[1] = FFGP_KOP_PRODUCT; lf[3].kfun = FFGP_KFUN_RQ;      // a learnable profile parameter
      EXPECT(ffgp_predict_small_tree_batch(fk, 1, &pp, &tlk, &pm, &sp) == FFGP_ERR_ARG);
      lf[3].kfun = FFGP_KFUN_SE; lf[2].amp_dev = nullptr;
      EXPECT(ffgp_predict_small_tree_batch(fk, 1, &pp, &tlk, &pm, &sp) == FFGP_ERR_ARG);
      lf[2].amp_dev = &x; pp.diag_vec_dev = &x;      // the predict paths drop y_var
      EXPECT(ffgp_predict_small_tree_batch(fk, 1, &pp, &tlk, &pm, &sp) == FFGP_ERR_ARG);
      pp.diag_vec_dev = nullptr; pp.add_all = 0.5;
      EXPECT(ffgp_predict_small_tree_batch(fk, 1, &pp, &tlk, &pm, &sp) == FFGP_ERR_ARG);
      pp.add_all = 0.0; pp.diag_add_dev = nullptr;
      EXPECT(ffgp_predict_small_tree_batch(fk, 1, &pp, &tlk, &pm, &sp) == FFGP_ERR_ARG);
      pp.diag_add_dev = &x; pp.Y_dev = nullptr;
      EXPECT(ffgp_predict_small_tree_batch(fk, 1, &pp, nullptr, &pm, &sp) == FFGP_ERR_ARG);
      EXPECT(sp == 7 && out[0] == 7.0 && out[1] == 7.0);      // (a refused call writes nothing)
    }
    ffgp_kdesc kd[2];
    ffgp_kdesc_grads kg[2];
    std::memset(kd, 0, sizeof kd);
    std::memset(kg, 0, sizeof kg);
    EXPECT(ffgp_assemble_pair(nullptr, &x, 1, &x, 1, 1, kd, FFGP_KOP_SUM, nullptr, nullptr, 0, nullptr, 0, 0.0, 0.0, &x, 2, 0) < 0);
    EXPECT(ffgp_kernel_grad_pair(nullptr, &x, 1, &x, 1, 1, kd, FFGP_KOP_PRODUCT, &x, 2, kg) < 0);
    // the acquisition optimiser on a stack of posteriors: every refusal comes before the handle or a member is dereferenced
    ffgp_acq_member mem[2];
    std::memset(mem, 0, sizeof mem);
    for (ffgp_acq_member& m : mem) {
      m.n = 4; m.D = 1; m.d = 1; m.ldl = 4; m.kfun = FFGP_KFUN_SE; m.kparam = 1.0; m.mean_coef = 1.0; m.var_coef = 1.0;
      m.X_dev = m.L_dev = m.alpha_dev = m.w_dev = m.amp_dev = &x;
    }
    ffgp_acq_stack stk;
    std::memset(&stk, 0, sizeof stk);
    stk.F = 2; stk.members = mem; stk.acq = FFGP_ACQ_UCB_VAR;
    ffgp_handle* fake = reinterpret_cast<ffgp_handle*>(0x1);      // never dereferenced by a refused call
    EXPECT(ffgp_acq_optimize_stack(nullptr, &stk, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    EXPECT(ffgp_acq_optimize_stack(fake, nullptr, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    EXPECT(ffgp_acq_optimize_stack(fake, &stk, nullptr, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    EXPECT(ffgp_acq_optimize_stack(fake, &stk, &x, 0, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    EXPECT(ffgp_acq_optimize_stack(fake, &stk, &x, 1, FFGP_ACQ_MAX_STEPS + 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    EXPECT(ffgp_acq_optimize_stack(fake, &stk, &x, 1, 1, nullptr, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    EXPECT(ffgp_acq_optimize_stack(fake, &stk, &x, 1, 1, &ad, nullptr, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    EXPECT(ffgp_acq_optimize_stack(fake, &stk, &x, 1, 1, &ad, &x, -1, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    EXPECT(ffgp_acq_optimize_stack(fake, &stk, &x, 1, 1, &ad, &x, 0, nullptr, nullptr, nullptr) == FFGP_ERR_ARG);
    stk.F = 0;
    EXPECT(ffgp_acq_optimize_stack(fake, &stk, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    stk.F = FFGP_ACQ_MAX_MEMBERS + 1;      // (the table holds two members: the count is refused before any is read)
    EXPECT(ffgp_acq_optimize_stack(fake, &stk, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    stk.F = 2; stk.members = nullptr;
    EXPECT(ffgp_acq_optimize_stack(fake, &stk, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    stk.members = mem; stk.acq = 3;
    EXPECT(ffgp_acq_optimize_stack(fake, &stk, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    stk.acq = FFGP_ACQ_EI; mem[1].D = 2;      // members whose D differ
    EXPECT(ffgp_acq_optimize_stack(fake, &stk, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    mem[1].D = 1; mem[1].n = FFGP_ACQ_MAX_N + 1; mem[1].ldl = 512;
    EXPECT(ffgp_acq_optimize_stack(fake, &stk, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    mem[1].n = 4; mem[1].ldl = 3;
    EXPECT(ffgp_acq_optimize_stack(fake, &stk, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    mem[1].ldl = 4; mem[1].kfun = FFGP_KFUN_LINEAR;
    EXPECT(ffgp_acq_optimize_stack(fake, &stk, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    mem[1].kfun = FFGP_KFUN_SE; mem[1].d = 2;
    EXPECT(ffgp_acq_optimize_stack(fake, &stk, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    mem[1].d = 1; mem[0].alpha_dev = nullptr;
    EXPECT(ffgp_acq_optimize_stack(fake, &stk, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    // the stack entry for members with composed kernels: the trees are checked before the driver, nothing is dereferenced on refusal
    {
      mem[0].alpha_dev = &x;
      ffgp_kdesc lf[4];
      std::memset(lf, 0, sizeof lf);
      for (ffgp_kdesc& k : lf) { k.kfun = FFGP_KFUN_SE; k.w_dev = &x; k.amp_dev = &x; k.kparam = 1.0; }
      lf[1].kfun = FFGP_KFUN_LINEAR;
      ffgp_ktree tr;
      std::memset(&tr, 0, sizeof tr);
      tr.n_leaves = 2; tr.op[0] = FFGP_KOP_SUM; tr.leaf = lf;
      const ffgp_ktree* trees[2] = {&tr, nullptr};      // member 0 on the tree, member 1 on its own radial kernel
      EXPECT(ffgp_acq_optimize_stack_tree(nullptr, &stk, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_stack_tree(fake, nullptr, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_stack_tree(fake, &stk, nullptr, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_stack_tree(fake, &stk, trees, nullptr, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_stack_tree(fake, &stk, trees, &x, 0, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_stack_tree(fake, &stk, trees, &x, 1, 1, nullptr, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_stack_tree(fake, &stk, trees, &x, 1, 1, &ad, nullptr, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_stack_tree(fake, &stk, trees, &x, 1, 1, &ad, &x, 0, nullptr, nullptr, nullptr) == FFGP_ERR_ARG);
      stk.F = FFGP_ACQ_MAX_MEMBERS + 1;      // (two trees, two members: the count is refused before any is read)
      EXPECT(ffgp_acq_optimize_stack_tree(fake, &stk, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      stk.F = 2; tr.n_leaves = 1;
      EXPECT(ffgp_acq_optimize_stack_tree(fake, &stk, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      tr.n_leaves = 5;
      EXPECT(ffgp_acq_optimize_stack_tree(fake, &stk, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      tr.n_leaves = 4; tr.shape = 2;
      EXPECT(ffgp_acq_optimize_stack_tree(fake, &stk, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      tr.shape = FFGP_TREE_BALANCED; tr.op[2] = 2;
      EXPECT(ffgp_acq_optimize_stack_tree(fake, &stk, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      tr.op[2] = FFGP_KOP_PRODUCT; lf[3].kfun = FFGP_KFUN_LINEAR + 1;
      EXPECT(ffgp_acq_optimize_stack_tree(fake, &stk, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      lf[3].kfun = FFGP_KFUN_RQ; lf[2].w_dev = nullptr;
      EXPECT(ffgp_acq_optimize_stack_tree(fake, &stk, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      lf[2].w_dev = &x; lf[0].amp_dev = nullptr;
      EXPECT(ffgp_acq_optimize_stack_tree(fake, &stk, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      lf[0].amp_dev = &x; tr.leaf = nullptr;
      EXPECT(ffgp_acq_optimize_stack_tree(fake, &stk, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      tr.leaf = lf; mem[1].w_dev = nullptr;      // the member without a tree needs its own kernel ...
      EXPECT(ffgp_acq_optimize_stack_tree(fake, &stk, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      mem[1].w_dev = &x; mem[0].w_dev = nullptr; mem[0].amp_dev = nullptr; mem[0].n = 0;      // ... the one with a tree does not: refused for n
      EXPECT(ffgp_acq_optimize_stack_tree(fake, &stk, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      mem[0].w_dev = mem[0].amp_dev = &x; mem[0].n = 4;
      // the two launch-per-stage entries share one driver (acq_staged_run): its refusals, with the staged rule on n and the one on Q D
      EXPECT(ffgp_acq_optimize_stack_staged(nullptr, &stk, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_stack_staged(fake, &stk, &x, 0, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_stack_staged(fake, &stk, &x, INT_MAX, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_stack_tree_staged(nullptr, &stk, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_stack_tree_staged(fake, nullptr, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_stack_tree_staged(fake, &stk, nullptr, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_stack_tree_staged(fake, &stk, trees, &x, 0, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_stack_tree_staged(fake, &stk, trees, &x, INT_MAX, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_stack_tree_staged(fake, &stk, trees, &x, 1, 1, &ad, &x, 0, nullptr, nullptr, nullptr) == FFGP_ERR_ARG);
      mem[1].n = FFGP_ACQ_STAGED_MAX_N + 1; mem[1].ldl = 4096;
      EXPECT(ffgp_acq_optimize_stack_tree_staged(fake, &stk, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_stack_staged(fake, &stk, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      mem[1].n = 4; mem[1].ldl = 4; tr.n_leaves = 5;
      EXPECT(ffgp_acq_optimize_stack_tree_staged(fake, &stk, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      tr.n_leaves = 4;
    }
    // the chain entry (NAR): the stack entry's driver with the D / D + 1 rule, and its own refusal of a coefficient other than 1
    mem[0].alpha_dev = &x; mem[1].D = 2;
    ffgp_acq_chain chn;
    std::memset(&chn, 0, sizeof chn);
    chn.F = 2; chn.members = mem; chn.acq = FFGP_ACQ_UCB_VAR;
    EXPECT(ffgp_acq_optimize_chain(nullptr, &chn, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    EXPECT(ffgp_acq_optimize_chain(fake, nullptr, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    EXPECT(ffgp_acq_optimize_chain(fake, &chn, &x, 0, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    mem[1].D = 1;                             // the second member must take D + 1 inputs
    EXPECT(ffgp_acq_optimize_chain(fake, &chn, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    mem[1].D = 2; mem[1].mean_coef = 0.8;
    EXPECT(ffgp_acq_optimize_chain(fake, &chn, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    mem[1].mean_coef = 1.0; mem[0].D = FFGP_ACQ_MAX_D; mem[1].D = FFGP_ACQ_MAX_D + 1;
    EXPECT(ffgp_acq_optimize_chain(fake, &chn, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    chn.members = nullptr;
    EXPECT(ffgp_acq_optimize_chain(fake, &chn, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    // the chain entry for members with composed kernels: the coefficients and the trees are checked before the driver, which then
    // applies the chain's D / D + 1 rule and skips the radial checks of the members that have a tree
    {
      chn.members = mem; mem[0].D = 1; mem[1].D = 2;
      ffgp_kdesc lf[4];
      std::memset(lf, 0, sizeof lf);
      for (ffgp_kdesc& k : lf) { k.kfun = FFGP_KFUN_SE; k.w_dev = &x; k.amp_dev = &x; k.kparam = 1.0; }
      lf[0].kfun = FFGP_KFUN_LINEAR;
      ffgp_ktree tr;
      std::memset(&tr, 0, sizeof tr);
      tr.n_leaves = 2; tr.op[0] = FFGP_KOP_SUM; tr.leaf = lf;
      const ffgp_ktree* trees[2] = {nullptr, &tr};      // member 0 on its own radial kernel, member 1 on the tree
      EXPECT(ffgp_acq_optimize_chain_tree(nullptr, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_chain_tree(fake, nullptr, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, nullptr, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, nullptr, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 0, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, nullptr, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, nullptr, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, nullptr, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, -1, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      chn.F = FFGP_ACQ_MAX_MEMBERS + 1;      // (two trees, two members: the count is refused before any is read)
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      chn.F = 0;
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      chn.F = 2; mem[1].var_coef = 0.5;      // a chain member has no weight
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      mem[1].var_coef = 1.0; mem[1].D = 1;   // the second member, tree or not, must take D + 1 inputs
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      mem[0].D = FFGP_ACQ_MAX_D; mem[1].D = FFGP_ACQ_MAX_D + 1;
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      mem[0].D = 1; mem[1].D = 2; tr.n_leaves = 1;
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      tr.n_leaves = 5;
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      tr.n_leaves = 4; tr.shape = 2;
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      tr.shape = FFGP_TREE_BALANCED; tr.op[2] = 2;
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      tr.op[2] = FFGP_KOP_PRODUCT; lf[3].kfun = FFGP_KFUN_LINEAR + 1;
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      lf[3].kfun = FFGP_KFUN_RQ; lf[2].w_dev = nullptr;
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      lf[2].w_dev = &x; lf[0].amp_dev = nullptr;
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      lf[0].amp_dev = &x; tr.leaf = nullptr;
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      tr.leaf = lf; mem[0].w_dev = nullptr;      // the member without a tree needs its own kernel ...
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      mem[0].w_dev = &x; mem[0].kfun = FFGP_KFUN_LINEAR;      // ... a radial one
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      mem[0].kfun = FFGP_KFUN_SE; mem[1].w_dev = nullptr; mem[1].amp_dev = nullptr; mem[1].n = 0;      // the one with a tree does not: refused for n
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      mem[1].w_dev = mem[1].amp_dev = &x; mem[1].n = 4; chn.members = nullptr;
      EXPECT(ffgp_acq_optimize_chain_tree(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      // the launch-per-stage entry for such chains: the coefficients and the trees are checked before the staged prologue, which
      // applies the chain's D / D + 1 rule, the staged rule on n and the one on Q D
      chn.members = mem;
      EXPECT(ffgp_acq_optimize_chain_tree_staged(nullptr, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, nullptr, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, nullptr, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, nullptr, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, &x, 0, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, &x, INT_MAX, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, &x, 1, 1, nullptr, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, &x, 1, 1, &ad, nullptr, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, nullptr, nullptr, nullptr) == FFGP_ERR_ARG);
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, &x, 1, 1, &ad, &x, -1, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      chn.F = FFGP_ACQ_MAX_MEMBERS + 1;
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      chn.F = 0;
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      chn.F = 2; mem[1].mean_coef = 0.8;
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      mem[1].mean_coef = 1.0; mem[1].D = 1;   // the member on the tree must take D + 1 inputs
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      mem[0].D = FFGP_ACQ_MAX_D; mem[1].D = FFGP_ACQ_MAX_D + 1;
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      mem[0].D = 1; mem[1].D = 2; mem[1].n = FFGP_ACQ_STAGED_MAX_N + 1; mem[1].ldl = 4096;
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      mem[1].n = 4; mem[1].ldl = 4; mem[1].d = 2;
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      mem[1].d = 1; tr.n_leaves = 5;
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      tr.n_leaves = 4; lf[3].kfun = FFGP_KFUN_LINEAR + 1;
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      lf[3].kfun = FFGP_KFUN_RQ; mem[0].kfun = FFGP_KFUN_LINEAR;      // the member without a tree needs a radial kernel of its own
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      mem[0].kfun = FFGP_KFUN_SE; chn.acq = 7;
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
      chn.acq = FFGP_ACQ_UCB_VAR; chn.members = nullptr;
      EXPECT(ffgp_acq_optimize_chain_tree_staged(fake, &chn, trees, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    }
    mem[0].D = 1; mem[1].D = 1; mem[0].alpha_dev = nullptr;
    // the single-posterior entry builds its one-member stack on the host and forwards: its refusals, next to the stack entry's
    ffgp_acq_problem ap;
    std::memset(&ap, 0, sizeof ap);
    ap.n = 4; ap.D = 1; ap.d = 1; ap.ldl = 4; ap.kfun = FFGP_KFUN_SE; ap.kparam = 1.0; ap.acq = FFGP_ACQ_UCB;
    ap.X_dev = ap.L_dev = ap.alpha_dev = ap.w_dev = ap.amp_dev = &x;
    EXPECT(ffgp_acq_optimize(nullptr, &ap, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    EXPECT(ffgp_acq_optimize(fake, nullptr, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    EXPECT(ffgp_acq_optimize(fake, &ap, nullptr, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    EXPECT(ffgp_acq_optimize(fake, &ap, &x, 1, 1, &ad, &x, 0, nullptr, nullptr, nullptr) == FFGP_ERR_ARG);
    EXPECT(ffgp_acq_optimize(fake, &ap, &x, 0, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    EXPECT(ffgp_acq_optimize(fake, &ap, &x, 1, 1, &ad, &x, -1, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    ap.n = 0;
    EXPECT(ffgp_acq_optimize(fake, &ap, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    ap.n = 4; ap.D = FFGP_ACQ_MAX_D + 1;
    EXPECT(ffgp_acq_optimize(fake, &ap, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    ap.D = 1; ap.d = 2;
    EXPECT(ffgp_acq_optimize(fake, &ap, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    ap.d = 1; ap.kfun = FFGP_KFUN_LINEAR;
    EXPECT(ffgp_acq_optimize(fake, &ap, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    ap.kfun = FFGP_KFUN_SE; ap.acq = FFGP_ACQ_UCB_VAR;      // the stack entry only
    EXPECT(ffgp_acq_optimize(fake, &ap, &x, 1, 1, &ad, &x, 0, &x, nullptr, nullptr) == FFGP_ERR_ARG);
    // K Adam steps of HOGP blocks: every refusal of ffgp_train_hogp_raw comes before the handle is dereferenced or anything is enqueued
    {
      ffgp_hogp_model hm;
      std::memset(&hm, 0, sizeof hm);
      hm.n = 4; hm.D = 2; hm.nmodes = 2; hm.dims[0] = 3; hm.dims[1] = 2; hm.kfun = FFGP_KFUN_SE; hm.kparam = 1.0;
      hm.X_dev = hm.Y_dev = &x;
      hm.w_dev = hm.amp_dev = hm.noise_dev = &x;
      ffgp_hogp_residual hr;
      std::memset(&hr, 0, sizeof hr);
      const long s0 = 0;
      auto call = [&](ffgp_handle* hh, int F, const ffgp_hogp_residual* r, long stride) {
        return ffgp_train_hogp_raw(hh, F, &hm, &lk, r, 3, &ad, &x, stride, &s0, &x, 3, nullptr, nullptr);
      };
      EXPECT(call(nullptr, 1, nullptr, 8) == FFGP_ERR_ARG);
      EXPECT(call(fake, 0, nullptr, 8) == FFGP_ERR_ARG);
      EXPECT(call(fake, 17, nullptr, 8) == FFGP_ERR_ARG);
      EXPECT(call(fake, 1, nullptr, 7) == FFGP_ERR_ARG);                 // state_stride < 2 (nw + 2), nw = D = 2
      EXPECT(ffgp_train_hogp_raw(fake, 1, &hm, &lk, nullptr, 3, &ad, &x, 8, &s0, &x, 2, nullptr, nullptr) == FFGP_ERR_ARG);   // trace_stride < steps
      EXPECT(ffgp_train_hogp_raw(fake, 1, &hm, &lk, nullptr, 3, &ad, &x, 8, nullptr, &x, 3, nullptr, nullptr) == FFGP_ERR_ARG);
      hm.n = 0;   EXPECT(call(fake, 1, nullptr, 8) == FFGP_ERR_ARG);
      hm.n = FFGP_SYEV_LDS_MAX_N + 1; EXPECT(call(fake, 1, nullptr, 8) == FFGP_ERR_ARG);
      hm.n = 4; hm.nmodes = 0; EXPECT(call(fake, 1, nullptr, 8) == FFGP_ERR_ARG);
      hm.nmodes = 4; EXPECT(call(fake, 1, nullptr, 8) == FFGP_ERR_ARG);
      hm.nmodes = 2; hm.dims[1] = 65; EXPECT(call(fake, 1, nullptr, 8) == FFGP_ERR_ARG);
      hm.dims[1] = 0; EXPECT(call(fake, 1, nullptr, 8) == FFGP_ERR_ARG);
      hm.nmodes = 3; hm.dims[0] = 16; hm.dims[1] = 16; hm.dims[2] = 17;      // every mode <= 64, the product 4352 > FFGP_HOGP_MAX_OUT
      EXPECT(call(fake, 1, nullptr, 8) == FFGP_ERR_ARG);
      hm.dims[0] = hm.dims[1] = hm.dims[2] = 64; EXPECT(call(fake, 1, nullptr, 8) == FFGP_ERR_ARG);
      hm.nmodes = 2; hm.dims[0] = 3; hm.dims[2] = 0;
      hm.dims[1] = 2; hm.noise_dev = nullptr; EXPECT(call(fake, 1, nullptr, 8) == FFGP_ERR_ARG);
      hm.noise_dev = &x; hm.Y_dev = nullptr; EXPECT(call(fake, 1, nullptr, 8) == FFGP_ERR_ARG);      // a plain block needs its targets
      hm.Y_dev = &x; hm.kfun = FFGP_KFUN_RQ; EXPECT(call(fake, 1, nullptr, 8) == FFGP_ERR_ARG);
      hm.kfun = FFGP_KFUN_SE; hm.D = 1; lk.w_broadcast = 1; EXPECT(call(fake, 1, nullptr, 8) == FFGP_ERR_ARG);   // one raw value for ONE column
      lk.w_broadcast = 0; hm.D = 2;
      hr.V_dev = &x; hr.l = 2;                                           // a residual member without its fields, with too small a state
      EXPECT(call(fake, 1, &hr, 64) == FFGP_ERR_ARG);
      hr.y_low_dev = hr.y_high_dev = &x; hr.l = 65; EXPECT(call(fake, 1, &hr, 64) == FFGP_ERR_ARG);
      hr.l = 2; EXPECT(call(fake, 1, &hr, 2 * (2 + 2 + 2 * 2) - 1) == FFGP_ERR_ARG);
      hr.V_row_stride = -1; hr.V_col_stride = 1; EXPECT(call(fake, 1, &hr, 64) == FFGP_ERR_ARG);
    }
    // the two tree trainers share the entry check, the tree-form check and the trainable-leaf check: every refusal of either comes
    // before the handle is dereferenced
    {
      ffgp_kdesc lf[4];
      std::memset(lf, 0, sizeof lf);
      for (ffgp_kdesc& k : lf) { k.kfun = FFGP_KFUN_MATERN32; k.w_dev = &x; k.amp_dev = &x; k.kparam = 1.0; }
      lf[0].kfun = FFGP_KFUN_LINEAR;
      ffgp_ktree tr;
      std::memset(&tr, 0, sizeof tr);
      tr.n_leaves = 2; tr.op[0] = FFGP_KOP_SUM; tr.leaf = lf;
      ffgp_problem tp;
      std::memset(&tp, 0, sizeof tp);
      tp.n = 4; tp.D = 1; tp.d = 1; tp.ll_variant = FFGP_LL_V1; tp.X_dev = tp.Y_dev = tp.diag_add_dev = &x; tp.tree = &tr;
      ffgp_tree_links tl;
      std::memset(&tl, 0, sizeof tl);
      for (auto tt : {ffgp_train_tree_raw, ffgp_train_tree_lds_raw}) {
        auto refused = [&](long stride = 64) { return tt(fake, 1, &tp, &tl, 3, &ad, &x, stride, 0, &x, 3) == FFGP_ERR_ARG; };
        EXPECT(tt(nullptr, 1, &tp, &tl, 3, &ad, &x, 64, 0, &x, 3) == FFGP_ERR_ARG);
        EXPECT(tt(fake, 1, nullptr, &tl, 3, &ad, &x, 64, 0, &x, 3) == FFGP_ERR_ARG);
        EXPECT(tt(fake, 17, &tp, &tl, 3, &ad, &x, 64, 0, &x, 3) == FFGP_ERR_ARG);
        EXPECT(tt(fake, 1, &tp, &tl, 0, &ad, &x, 64, 0, &x, 3) == FFGP_ERR_ARG);
        EXPECT(tt(fake, 1, &tp, &tl, 3, &ad, &x, 64, -1, &x, 3) == FFGP_ERR_ARG);
        EXPECT(tt(fake, 1, &tp, &tl, 3, &ad, &x, 64, 0, &x, 2) == FFGP_ERR_ARG);      // trace_stride < steps
        tr.n_leaves = 1; EXPECT(refused());
        tr.n_leaves = 5; EXPECT(refused());
        tr.n_leaves = 2; tr.leaf = nullptr; EXPECT(refused());
        tr.leaf = lf; lf[1].kfun = FFGP_KFUN_RQ; EXPECT(refused());
        lf[1].kfun = FFGP_KFUN_MATERN32; lf[1].w_dev = nullptr; EXPECT(refused());
        lf[1].w_dev = &x; lf[0].amp_dev = nullptr; EXPECT(refused());
        lf[0].amp_dev = &x; tl.leaf[1].center_train = 1; EXPECT(refused());      // a trained centre on a leaf that is not linear ...
        tl.leaf[1].center_train = 0; tl.leaf[0].center_train = 1; EXPECT(refused());      // ... and on a linear leaf without center_dev
        tl.leaf[0].center_train = 0; EXPECT(refused(2 * (2 + 2 + 1) - 1));      // state_stride < 2 P
        tp.tree = nullptr; EXPECT(refused());
        tp.tree = &tr;
      }
      {   // ffgp_train_tree_res_raw: the residual member's own refusals, and r = NULL is ffgp_train_tree_raw's check
        ffgp_residual rr;
        std::memset(&rr, 0, sizeof rr);
        auto refused = [&](const ffgp_residual* r, long stride = 64) {      // (both forms: launch per stage and one launch)
          return ffgp_train_tree_res_raw(fake, 1, &tp, &tl, r, 3, &ad, &x, stride, 0, &x, 3) == FFGP_ERR_ARG &&
                 ffgp_train_tree_lds_res_raw(fake, 1, &tp, &tl, r, 3, &ad, &x, stride, 0, &x, 3) == FFGP_ERR_ARG;
        };
        EXPECT(ffgp_train_tree_lds_res_raw(nullptr, 1, &tp, &tl, &rr, 3, &ad, &x, 64, 0, &x, 3) == FFGP_ERR_ARG);
        tp.n = 129; EXPECT(ffgp_train_tree_lds_res_raw(fake, 1, &tp, &tl, nullptr, 3, &ad, &x, 64, 0, &x, 3) == FFGP_ERR_ARG);
        tp.n = 4;
        EXPECT(ffgp_train_tree_res_raw(nullptr, 1, &tp, &tl, &rr, 3, &ad, &x, 64, 0, &x, 3) == FFGP_ERR_ARG);
        EXPECT(refused(nullptr, 2 * (2 + 2 + 1) - 1));      // a plain member: state_stride < 2 P
        rr.rho_dev = &x; EXPECT(refused(&rr));              // a residual member without y_low_dev / y_high_dev
        rr.y_low_dev = rr.y_high_dev = &x; EXPECT(refused(&rr, 2 * (2 + 2 + 1)));      // state_stride < 2 (P + 1)
        rr.v_low_dev = &x; EXPECT(refused(&rr));            // v_low_dev without v_high_dev
        rr.v_high_dev = &x; rr.v_high_stride = -1; EXPECT(refused(&rr));
        rr.v_high_stride = 1; lf[1].kfun = FFGP_KFUN_RQ; EXPECT(refused(&rr));
        lf[1].kfun = FFGP_KFUN_MATERN32;
      }
      tr.n_leaves = 4; tr.shape = 2;      // the one-launch form alone (the other leaves the shape to the assembly, behind the handle)
      EXPECT(ffgp_train_tree_lds_raw(fake, 1, &tp, &tl, 3, &ad, &x, 64, 0, &x, 3) == FFGP_ERR_ARG);
    }
    std::printf("asan_host_check: no device -- argument / no-device paths clean\n");
    return 0;
  }
  EXPECT(rc == FFGP_OK && h != nullptr);
  EXPECT(ffgp_set_option(h, "no-such-option", 1.0) < 0);
  EXPECT(ffgp_potrf(h, nullptr, 4, 4) < 0);
  EXPECT(ffgp_destroy(h) == FFGP_OK);
  std::printf("asan_host_check: device present -- create / option / argument / destroy paths clean\n");
  return 0;
}
