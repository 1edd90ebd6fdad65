"""The acquisition optimiser on composed-kernel models past 256 training points: the launch-per-stage loop inside one library call
(ffgp_acq_optimize_stack_tree_staged, csrc/acq_staged_tree.hip on the driver of csrc/acq_staged.hip; `fuse_composed=True` together with
`staged=True` on Posterior / PosteriorStack.optimize_acquisition and acq.optimize_acqf / optimize_acqf_mf) against the references
test_gpu_acq_tree.py and test_gpu_acq_stack_tree.py are written against -- the reference's kernel formulas in plain fp64 torch on the
CPU, the per-step loop on the GPU, the one-launch tree kernels where they still serve, the radial staged entry on an all-radial stack --
and two fixtures of the reference's own loops at its demos' sizes (tests/golden/acq_tree_cigp_n300.npz and mf_acq_ar_sum_n300.npz,
written by tests/golden/gen_acq_staged_tree_goldens.py).

Helpers, recipes and bars are those files' and test_gpu_acq_staged.py's, imported and unchanged.  Evaluate mode (steps = 0): values rel.
1e-10, gradients rel. 1e-8.  Trajectories: (A) the CPU loop and (B) the per-step GPU loop differ by rounding only; d0 = their distance is
the yardstick, max(10 d0, 1e-12) the bound, a case with d0 > 1e-10 fails as ill-conditioned, and a CPU twin started one ulp away must stay
within 1e-11 before anything is compared.  State: a + b steps equal a + b in one call bit for bit.  Cutting Q into two calls can change
the tile shape the fp64 GEMM picks (see test_gpu_acq_staged.py), so that comparison is held to a relative distance of 1e-13.  Every case
runs a handful of steps on shapes just past the one-launch limit (257: a row chunk of one row), at the demo's 300, and at 513 = 4 chunks
of 128 rows + 1 with D = 16."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_acq_stack as S            # noqa: E402
import test_gpu_acq_stack_tree as ST      # noqa: E402
import test_gpu_acq_staged as G           # noqa: E402
import test_gpu_acq_tree as T             # noqa: E402
from test_gpu_acq_stack import ACQ_CODE, DEV, LINEAR, M52, distance, rel, select      # noqa: E402
from test_gpu_acq_staged import is_staged, one_stack, single, stacked, yardstick      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 8
LR = 0.1
BOTH = dict(fuse_composed=True, staged=True)
FORCE = dict(fuse_composed=True, staged="force")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(torch.float32)


# ---- the GPU side --------------------------------------------------------------------------------------------------------------------
def raw(gst, Xq, level, sp, steps=0, lr=0.1, step0=0, Q=None, null=(), F=None, accumulate=0, acq=None, member=0, tree=None, tree_null=None,
        **over):
    """ffgp_acq_optimize_stack_tree_staged through ctypes: test_gpu_acq_stack_tree.raw_call with the staged entry.  `over` overrides
    fields of member `member`, `tree` = (member, keyword arguments of test_gpu_acq_tree._tree_copy), `tree_null` names a member whose
    tree pointer is passed as NULL, `null` names pointers to pass as NULL.  Returns (status, X, state, trace, hist, grad), every buffer
    pre-filled with a sentinel."""
    from fidelityfusion_amd import _lib
    keep = []
    tab = gst._member_table(gst.test_var_adds, keep)
    trees = gst._tree_table()
    for k, v in over.items():
        setattr(tab[member], k, v)
    if tree is not None:
        trees[tree[0]] = T._tree_copy(gst.members[tree[0]], keep, **tree[1])
    if tree_null is not None:
        trees[tree_null] = C.POINTER(_lib.KTree)()
    Qn, D = Xq.shape
    X = Xq.to(DEV).clone().contiguous()
    state = torch.zeros((3, Qn, D), device=DEV)
    trace = torch.full((max(steps, 1), Qn), -7.0, device=DEV)
    hist = torch.full((max(steps, 0) + 1, Qn, D), -7.0, device=DEV)
    grad = torch.full((Qn, D), -7.0, device=DEV)
    lv = None if level is None else level.to(device=DEV, dtype=torch.int32).contiguous()
    s = _lib.AcqStack(F=gst.F if F is None else F, members=None if "members" in null else tab, level_dev=None if lv is None else lv.data_ptr(),
                      var_floor=sp["var_floor"], acq=ACQ_CODE[sp["acq"]] if acq is None else acq, kappa=sp["kappa"], xi=sp["xi"],
                      f_best=sp["f_best"], accumulate_grad=accumulate)
    opt = _lib.Adam(lr, 0.9, 0.999, 1e-8)
    ptr = lambda name, t: None if name in null else C.c_void_p(t.data_ptr())
    rc = _lib.lib.ffgp_acq_optimize_stack_tree_staged(None if "h" in null else gst.members[0]._h(), None if "s" in null else C.byref(s),
                                                      None if "trees" in null else trees, ptr("X", X), Qn if Q is None else Q, steps,
                                                      None if "opt" in null else C.byref(opt), ptr("state", state), step0, ptr("trace", trace),
                                                      ptr("hist", hist), ptr("grad", grad))
    torch.cuda.synchronize()
    return rc, X, state, trace, hist, grad


# ---- 1. values and gradients (steps = 0) against CPU autograd --------------------------------------------------------------------------
#        n    D   Q   tree               257: a row chunk of one row, a ragged column tile; 513: five chunks, the widest DM; Q = 70: two tiles
EVAL = [(257, 2, 37, "sum_lin_m52"),       # the reference's tree: Sum(Linear, Matern-5/2)
        (257, 2, 37, "prod_ard_linc"),     # a product with a centred LinearKernel: k(x, x) depends on x through it
        (300, 1, 16, "se_m32_rq"),         # three leaves, Matern-3/2 with its clamp, RQ
        (513, 16, 21, "chain4"),           # ((Linear + SE) x Matern52) + Matern12
        (513, 16, 21, "balanced4"),        # (SE x Linear) + (Matern32 x RQ)
        (300, 2, 70, "balanced4")]


@functools.lru_cache(maxsize=None)
def eval_case(i):
    n, D, Q, tree = EVAL[i]
    c = T.make_case(n, D, Q, tree, seed=3000 + i)
    return c, one_stack(T.gpu_posterior(c), 0.05)


@pytest.mark.parametrize("acq", ["ucb", "ei"])
@pytest.mark.parametrize("i", range(len(EVAL)))
def test_evaluate_matches_cpu_autograd(i, acq):
    c, gst = eval_case(i)
    sp = T.spec(acq, f_best=0.3, var_add=0.05)
    rc, X, _, trace, _, grad = raw(gst, c["X0"], None, sp)
    assert rc == 0
    assert torch.equal(X.cpu(), c["X0"])      # evaluate mode: nothing moves
    a, g, _, _ = T.cpu_eval(c, c["X0"], sp)
    ev, eg = rel(trace[0], a), rel(grad, g)
    print("staged tree n=%d D=%d Q=%d %s %s: value rel %.2e, gradient rel %.2e" % (EVAL[i] + (acq, ev, eg)))
    assert ev <= 1e-10, ev
    assert eg <= 1e-8, eg


# ---- 2. trajectories against the per-step GPU loop and the CPU loop -------------------------------------------------------------------
#        n    D   Q   tree            acquisition                                 seed
TRAJ = [(257, 2, 37, "sum_lin_m52", T.spec("ucb", var_add=0.05), 11),
        (300, 1, 16, "se_m32_rq", T.spec("ei", f_best=0.3, var_add=0.05), 12),
        (513, 16, 21, "balanced4", T.spec("ucb", var_add=0.05), 13)]


@functools.lru_cache(maxsize=None)
def traj(i, steps=STEPS):
    """case i once: the CPU loop, its twin, loop B, the staged call -- shared by the tests below and left unchanged"""
    n, D, Q, tree, sp, seed = TRAJ[i]
    c = T.make_case(n, D, Q, tree, seed)
    A = T.loop_a(c, c["X0"], sp, steps, LR)
    twin = T.loop_a(c, c["X0"] * (1.0 + 2e-16), sp, steps, LR)
    post = T.gpu_posterior(c)
    B = T.loop_b(post, c["X0"], sp, steps, LR)
    X0d = c["X0"].to(DEV)
    keep = X0d.clone()
    Z = single(post, X0d, sp, steps, LR, **BOTH)
    assert torch.equal(X0d, keep)      # X0 is left untouched
    return c, post, A, twin, B, Z


@pytest.mark.parametrize("i", range(len(TRAJ)))
def test_trajectory_follows_both_references(i):
    c, post, A, twin, B, Z = traj(i)
    d0, bound = yardstick(A, twin, B)
    dA, dB = distance(Z, A), distance(Z, B)
    print("staged tree case %d: d0 %.2e, bound %.2e, staged vs A %.2e, vs B %.2e" % (i, d0, bound, dA, dB))
    n, D, Q = TRAJ[i][:3]
    assert is_staged(Z[3]) and Z[3]["step"] == STEPS
    assert Z[1].shape == (STEPS, Q) and Z[2].shape == (STEPS + 1, Q, D)
    assert torch.equal(Z[0], Z[2][-1]) and torch.equal(Z[2][0].cpu(), c["X0"])
    assert dA <= bound, (dA, bound)
    assert dB <= bound, (dB, bound)


# ---- 3. stacks: radial and tree members mixed -----------------------------------------------------------------------------------------
#          ns               D   members                                     coefs               var_coefs          Q
STACKS = [((300, 300, 250), 2, ("sum_lin_m52", "M32", "prod_ard_linc"), (1.0, 0.8, -1.3), None, 19),      # the demo's sizes; rho != 1, one negative
          ((257, 40, 130), 3, ("chain4", "SE", "se_m32_rq"), (1.0, 0.8, 1.2), (1.0, 0.5, 2.0), 37)]      # a smaller member after a larger one
STACK_ACQ = {"ucb": S.spec("ucb"), "ei": S.spec("ei", f_best=0.3), "ucb_var": S.spec("ucb_var", kappa=0.4)}
STACK_CASES = [(0, "ucb", False), (0, "ei", True), (0, "ucb_var", False), (0, "ucb_var", True), (1, "ucb", True), (1, "ei", False)]


@functools.lru_cache(maxsize=None)
def big_stack(i):
    ns, D, kinds, coefs, var_coefs, Q = STACKS[i]
    st = ST.make_stack(ns, D, kinds, coefs, Q, seed=800 + i, var_coefs=var_coefs)      # var_adds 0.05; levels mixed: (7 q + 2) % 3
    return st, ST.gpu_stack(st)


@pytest.mark.parametrize("i,acq,accumulate", STACK_CASES)
def test_stack_follows_both_references(i, acq, accumulate):
    st, gst = big_stack(i)
    sp, lr = STACK_ACQ[acq], 0.01 if accumulate else 0.1
    A = ST.loop_a(st, st["X0"], st["level"], sp, STEPS, lr, accumulate)
    twin = ST.loop_a(st, st["X0"] * (1.0 + 2e-16), st["level"], sp, STEPS, lr, accumulate)
    B = ST.loop_b(gst, st["X0"], st["level"], sp, STEPS, lr, accumulate)
    d0, bound = yardstick(A, twin, B)
    Z = stacked(gst, st["X0"].to(DEV), st["level"], sp, STEPS, lr, accumulate, **BOTH)
    dA, dB = distance(Z, A), distance(Z, B)
    print("staged tree stack %d %s accumulate=%s: d0 %.2e, bound %.2e, staged vs A %.2e, vs B %.2e" % (i, acq, accumulate, d0, bound, dA, dB))
    assert is_staged(Z[3]) and Z[3]["step"] == STEPS and ("grad_sum" in Z[3]) == accumulate
    assert torch.equal(Z[0], Z[2][-1]) and torch.equal(Z[2][0].cpu(), st["X0"])
    assert dA <= bound, (dA, bound)
    assert dB <= bound, (dB, bound)


@pytest.mark.parametrize("acq", ["ucb", "ei", "ucb_var"])
def test_stack_evaluate_matches_cpu_autograd(acq):
    st, gst = big_stack(1)      # given variance coefficients, D = 3 padded to DM = 8
    sp = STACK_ACQ[acq]
    rc, _, _, trace, _, grad = raw(gst, st["X0"], st["level"], sp)
    assert rc == 0
    a, g, _ = ST.cpu_eval(st, st["X0"], st["level"], sp)
    assert rel(trace[0], a) <= 1e-10 and rel(grad, g) <= 1e-8, (rel(trace[0], a), rel(grad, g))
    rc, _, _, trace, _, grad = raw(gst, st["X0"], None, sp)      # without levels: every member counts
    a, g, _ = ST.cpu_eval(st, st["X0"], None, sp)
    assert rc == 0 and rel(trace[0], a) <= 1e-10 and rel(grad, g) <= 1e-8


@pytest.mark.parametrize("accumulate", [0, 1])
def test_stack_with_a_negative_level_switches_every_member_off_for_that_point(accumulate):
    """the C entry reads a negative level as "no member": mean = var = 0, a zero gradient (the self term included), the point stays"""
    st, gst = big_stack(0)
    sp, lr = STACK_ACQ["ucb"], 0.01 if accumulate else 0.1
    level = st["level"].clone()
    level[3] = -1
    level[17] = -2
    A = ST.loop_a(st, st["X0"], level, sp, STEPS, lr, bool(accumulate))
    twin = ST.loop_a(st, st["X0"] * (1.0 + 2e-16), level, sp, STEPS, lr, bool(accumulate))
    B = ST.loop_b(gst, st["X0"], level, sp, STEPS, lr, bool(accumulate))
    _, bound = yardstick(A, twin, B)
    rc, X, state, trace, hist, _ = raw(gst, st["X0"], level, sp, steps=STEPS, lr=lr, accumulate=accumulate)
    assert rc == 0
    got = (X, trace, hist)
    assert distance(got, B) <= bound and distance(got, A) <= bound
    D = st["D"]
    assert torch.equal(hist[:, 3].cpu(), st["X0"][3].expand(STEPS + 1, D)) and torch.equal(hist[:, 17].cpu(), st["X0"][17].expand(STEPS + 1, D))
    assert bool(state[2].ne(0).any()) == bool(accumulate)


# ---- 4. the forced staged call against the one-launch tree calls -----------------------------------------------------------------------
#          n    D   Q   tree            acquisition                      seed  steps
FORCED = [(40, 2, 37, "sum_lin_m52", T.spec("ucb", var_add=0.05), 21, 10),
          (256, 16, 20, "chain4", T.spec("ucb", var_add=0.05), 22, STEPS)]


@functools.lru_cache(maxsize=None)
def forced(i):
    n, D, Q, tree, sp, seed, steps = FORCED[i]
    c = T.make_case(n, D, Q, tree, seed)
    A = T.loop_a(c, c["X0"], sp, steps, LR)
    twin = T.loop_a(c, c["X0"] * (1.0 + 2e-16), sp, steps, LR)
    post = T.gpu_posterior(c)
    B = T.loop_b(post, c["X0"], sp, steps, LR)
    one = T.fused(post, c["X0"].to(DEV), sp, steps, LR)
    return c, post, A, twin, B, one


@pytest.mark.parametrize("i", range(len(FORCED)))
def test_forced_staged_call_follows_the_one_launch_tree_call(i):
    c, post, A, twin, B, one = forced(i)
    sp, steps = FORCED[i][4], FORCED[i][6]
    d0, bound = yardstick(A, twin, B)
    Z = single(post, c["X0"].to(DEV), sp, steps, LR, **FORCE)
    assert one[3]["fused"] is True and not one[3].get("staged") and is_staged(Z[3])
    dO, dA = distance(Z, one), distance(Z, A)
    print("forced tree n=%d: d0 %.2e, bound %.2e, staged vs one-launch %.2e, vs A %.2e" % (FORCED[i][0], d0, bound, dO, dA))
    assert dO <= bound and dA <= bound, (dO, dA, bound)


def test_forced_staged_call_follows_the_one_launch_stack_tree_call():
    st = ST.make_stack((40, 24, 17), 2, ("sum_lin_m52", "prod_ard_linc", "M32"), (1.0, 0.8, -1.3), 37, seed=810)
    gst = ST.gpu_stack(st)
    sp = S.spec("ucb")
    A = ST.loop_a(st, st["X0"], st["level"], sp, STEPS, LR)
    twin = ST.loop_a(st, st["X0"] * (1.0 + 2e-16), st["level"], sp, STEPS, LR)
    B = ST.loop_b(gst, st["X0"], st["level"], sp, STEPS, LR)
    _, bound = yardstick(A, twin, B)
    one = ST.fused(gst, st["X0"].to(DEV), st["level"], sp, STEPS, LR)
    Z = stacked(gst, st["X0"].to(DEV), st["level"], sp, STEPS, LR, **FORCE)
    assert one[3]["fused"] is True and is_staged(Z[3])
    assert distance(Z, one) <= bound and distance(Z, A) <= bound


@pytest.mark.parametrize("first", ["one-launch", "staged"])
def test_a_state_moves_between_the_one_launch_and_the_staged_call(first):
    c, post, A, twin, B, one = forced(0)      # 10 one-launch steps
    sp = FORCED[0][4]
    _, bound = yardstick(A, twin, B)
    kw1, kw2 = (dict(fuse_composed=True), FORCE) if first == "one-launch" else (FORCE, dict(fuse_composed=True))
    X1, t1, h1, s1 = single(post, c["X0"].to(DEV), sp, 4, LR, **kw1)
    X2, t2, h2, s2 = single(post, X1, sp, 6, LR, state=s1, **kw2)
    assert is_staged(s1) == (first == "staged") and is_staged(s2) == (first != "staged") and s2["step"] == 10
    got = (X2, torch.cat([t1, t2]), torch.cat([h1[:-1], h2]))
    d = distance(got, one)
    print("4 %s steps + 6 of the other call vs 10 one-launch steps: %.2e (bound %.2e)" % (first, d, bound))
    assert d <= bound and rel(X2, one[0]) <= bound


# ---- 5. the neighbouring entries on the models they share ---------------------------------------------------------------------------------
def test_an_all_radial_stack_through_the_new_entry_follows_the_radial_staged_entry():
    """trees[f] = NULL for every member: the model ffgp_acq_optimize_stack_staged serves, each member run as a one-leaf record; the
    leaves are re-evaluated in the gradient pass where that entry keeps a derivative image, so the bound is the trajectory bound"""
    st = S.make_stack((300, 257, 40), 2, (1.0, 0.8, -1.3), 37, seed=820)
    gst = S.gpu_stack(st)
    sp = S.spec("ucb")
    A = S.loop_a(st, st["X0"], st["level"], sp, STEPS, LR)
    twin = S.loop_a(st, st["X0"] * (1.0 + 2e-16), st["level"], sp, STEPS, LR)
    B = S.loop_b(gst, st["X0"], st["level"], sp, STEPS, LR)
    d0, bound = yardstick(A, twin, B)
    rc0, X0_, _, t0, h0, _ = G.raw_staged(gst, st["X0"], st["level"], sp, steps=STEPS)
    rc1, X1_, _, t1, h1, _ = raw(gst, st["X0"], st["level"], sp, steps=STEPS)
    assert rc0 == 0 and rc1 == 0
    new, old = (X1_, t1, h1), (X0_, t0, h0)
    print("all radial: d0 %.2e, new entry vs radial staged entry %.2e, vs A %.2e" % (d0, distance(new, old), distance(new, A)))
    assert distance(new, old) <= bound and distance(new, A) <= bound and distance(new, B) <= bound


def test_one_tree_member_with_coefficient_one_is_the_single_posterior_call():
    c, post, A, twin, B, Z = traj(0)
    sp = TRAJ[0][4]
    _, bound = yardstick(A, twin, B)
    gst = one_stack(post, sp["var_add"])
    r = stacked(gst, c["X0"].to(DEV), None, S.spec(sp["acq"], kappa=sp["kappa"]), STEPS, LR, **BOTH)
    assert is_staged(r[3])
    assert distance(r, Z) <= bound and distance(r, A) <= bound


# ---- 6. determinism ----------------------------------------------------------------------------------------------------------------------
def test_state_continues_the_optimiser_bit_for_bit():
    c, post, _, _, _, _ = traj(0)
    sp, X0 = TRAJ[0][4], c["X0"].to(DEV)
    full = single(post, X0, sp, 10, LR, **BOTH)
    X1, t1, h1, s1 = single(post, X0, sp, 4, LR, **BOTH)
    assert is_staged(s1) and s1["step"] == 4
    X2, t2, h2, s2 = single(post, X1, sp, 6, LR, state=s1, **BOTH)
    assert is_staged(s2) and s2["step"] == 10
    assert torch.equal(X2, full[0])
    assert torch.equal(torch.cat([t1, t2]), full[1])
    assert torch.equal(torch.cat([h1[:-1], h2]), full[2])
    assert torch.equal(s2["exp_avg"], full[3]["exp_avg"]) and torch.equal(s2["exp_avg_sq"], full[3]["exp_avg_sq"])


def test_state_continues_the_stack_with_accumulation_bit_for_bit():
    st, gst = big_stack(0)
    sp, X0, lv = STACK_ACQ["ucb_var"], st["X0"].to(DEV), st["level"]
    full = stacked(gst, X0, lv, sp, 10, 0.01, True, **BOTH)
    X1, t1, h1, s1 = stacked(gst, X0, lv, sp, 4, 0.01, True, **BOTH)
    X2, t2, h2, s2 = stacked(gst, X1, lv, sp, 6, 0.01, True, state=s1, **BOTH)
    assert torch.equal(X2, full[0]) and torch.equal(torch.cat([t1, t2]), full[1]) and torch.equal(torch.cat([h1[:-1], h2]), full[2])
    assert torch.equal(s2["grad_sum"], full[3]["grad_sum"]) and bool(s2["grad_sum"].ne(0).any())


def test_cutting_the_points_into_two_calls_changes_rounding_at_most():
    """Q = 37 in one call against 16 + 21: a tolerance (1e-13, relative), not equality -- the GEMM's tile choice (the module's docstring)"""
    c, post, _, _, _, Z = traj(0)
    sp, X0 = TRAJ[0][4], c["X0"].to(DEV)
    lo = single(post, X0[:16].contiguous(), sp, STEPS, LR, **BOTH)
    hi = single(post, X0[16:].contiguous(), sp, STEPS, LR, **BOTH)
    got = (torch.cat([lo[0], hi[0]]), torch.cat([lo[1], hi[1]], 1), torch.cat([lo[2], hi[2]], 1))
    d = max(distance(got, Z), rel(got[0], Z[0]))
    print("Q = 37 against 16 + 21: %.2e" % d)
    assert d <= 1e-13, d


def test_a_point_does_not_depend_on_its_tile_neighbours_or_their_levels():
    """the same number of points in every call, so the GEMM's tile shape is the same: then a point's trajectory is the same bits wherever
    it stands, whoever stands beside it and whatever their levels"""
    st, gst = big_stack(0)
    sp, X0, lv = STACK_ACQ["ucb"], st["X0"].to(DEV), st["level"]
    Q = X0.shape[0]
    Z = stacked(gst, X0, lv, sp, STEPS, LR, **BOTH)
    idx = torch.arange(Q - 1, -1, -1)      # another column, other neighbours
    r = stacked(gst, X0[idx.to(DEV)].contiguous(), lv[idx], sp, STEPS, LR, **BOTH)
    assert torch.equal(r[1], Z[1][:, idx.to(DEV)]) and torch.equal(r[2], Z[2][:, idx.to(DEV)])
    keep = torch.tensor([0, 7, 18])        # the neighbours moved and given other levels
    X1, lv1 = 2.0 - X0, (lv + 1) % 3
    X1[keep.to(DEV)], lv1[keep] = X0[keep.to(DEV)], lv[keep]
    r = stacked(gst, X1.contiguous(), lv1, sp, STEPS, LR, **BOTH)
    assert torch.equal(r[1][:, keep.to(DEV)], Z[1][:, keep.to(DEV)]) and torch.equal(r[2][:, keep.to(DEV)], Z[2][:, keep.to(DEV)])
    assert not torch.equal(r[1], Z[1])


# ---- 7. memory that must not be read --------------------------------------------------------------------------------------------------------
def test_padding_the_upper_triangle_and_a_tree_members_own_kernel_fields_are_never_read():
    st, gst = big_stack(1)      # member 0: chain4 on 257 points
    sp, post = STACK_ACQ["ucb"], gst.members[0]
    n = post.n
    ldl = (n + 9) // 2 * 2      # > n, even like the library's own leading dimensions
    clean = torch.zeros((n, ldl), device=DEV)
    clean[:, :n] = torch.tril(post.W[:n, :n])
    dirty = clean.clone()
    dirty[:, :n] += torch.triu(torch.full((n, n), float("nan"), device=DEV), diagonal=1)
    dirty[:, n:] = float("nan")
    nan = torch.full((16,), float("nan"), device=DEV)
    assert bool(torch.isnan(dirty).any()) and torch.equal(torch.tril(dirty[:, :n]), clean[:, :n])
    ra = raw(gst, st["X0"], st["level"], sp, steps=STEPS, L_dev=clean.data_ptr(), ldl=ldl)
    rb = raw(gst, st["X0"], st["level"], sp, steps=STEPS, L_dev=dirty.data_ptr(), ldl=ldl, w_dev=nan.data_ptr(), amp_dev=nan.data_ptr(), kfun=99)
    assert ra[0] == 0 and rb[0] == 0
    assert bool(torch.isfinite(ra[3]).all()) and bool(ra[1].ne(st["X0"].to(DEV)).any())
    for x, y in zip(ra[1:], rb[1:]):
        assert torch.equal(x, y)


# ---- 8. the fixtures of the reference's loops at its demos' sizes ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cigp_fixture():
    """test_gpu_acq_tree.fixture on the 300-point file"""
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.cigp_v10 import cigp
    z = np.load(os.path.join(ROOT, "tests", "golden", "acq_tree_cigp_n300.npz"))
    lin, mat = kernel.LinearKernel(1, float(z["lin_length_scale"]), float(z["lin_signal_variance"])), \
        kernel.MaternKernel(1, float(z["matern_length_scale"]), float(z["matern_signal_variance"]))
    with torch.no_grad():
        lin.center.fill_(float(z["lin_center"]))
    m = cigp(kernel.SumKernel(lin, mat), float(z["log_beta"])).double().to(DEV)
    m.requires_grad_(False)
    x, y = torch.tensor(z["x"], device=DEV), torch.tensor(z["y"], device=DEV)
    return z, m, x, y, m._cached_posterior(x, y)[0]


@pytest.mark.parametrize("tag", ["ucb", "ei"])
def test_staged_call_reproduces_the_reference_cigp_fixture(tag):
    from fidelityfusion_amd import acq
    z, m, x, y, post = cigp_fixture()
    assert float(z["twin_distance"]) <= 1e-11 and post.n == 300
    assert post.tree is not None and [int(d["kfun"]) for d in post.tree[0]] == [LINEAR, M52]
    steps, lr = int(z["steps"]), float(z["lr"])
    noise = float(m.log_beta.exp().pow(-1))
    sp = T.spec(tag, kappa=float(z["kappa"]), xi=float(z["xi"]), f_best=float(z["f_best"]), var_add=noise, var_floor=0.0)
    X0 = torch.tensor(z["X0"])
    ref = (None, torch.tensor(z["trace_" + tag]), torch.tensor(z["hist_" + tag]))
    B = T.loop_b(post, X0, sp, steps, lr)
    d0 = distance(B, ref)
    assert d0 <= 1e-10, "ill-conditioned case: d0 = %.2e" % d0
    bound = max(10.0 * d0, 1e-12)
    Z = single(post, X0.to(DEV), sp, steps, lr, **BOTH)
    assert is_staged(Z[3])
    print("fixture cigp n300 %s: d0 %.2e, bound %.2e, staged vs fixture %.2e, vs B %.2e" % (tag, d0, bound, distance(Z, ref), distance(Z, B)))
    assert distance(Z, ref) <= bound and distance(Z, B) <= bound
    assert rel(Z[0], ref[2][-1]) <= bound      # the final points
    # the reference's selected point
    k_ref, best_ref = select(X0, ref[1], ref[2])
    assert k_ref >= 0 and torch.equal(best_ref, torch.tensor(z["best_" + tag]))      # (the restated rule selects what the reference selected)
    best = acq.optimize_acqf(m, x, y, X0.to(DEV), steps=steps, lr=lr, acq=tag, kappa=float(z["kappa"]), xi=float(z["xi"]),
                             f_best=float(z["f_best"]), var_floor=0.0, **BOTH)
    e_best = float((best.cpu() - best_ref).abs().max()) / float(ref[2].abs().max())
    print("fixture cigp n300 %s: selected step %d, best_x %.2e" % (tag, k_ref, e_best))
    assert torch.equal(best, Z[2][k_ref + 1])      # optimize_acqf took the staged call and returned exactly that history entry
    assert e_best <= bound, (e_best, bound)


@functools.lru_cache(maxsize=None)
def ar_fixture():
    """test_gpu_acq_stack_tree.fixture on the (300, 300, 250) file"""
    from fidelityfusion_amd import functional as F, kernel
    from fidelityfusion_amd.cigp_v10 import cigp
    z = np.load(os.path.join(ROOT, "tests", "golden", "mf_acq_ar_sum_n300.npz"))
    models, data, members, noise = [], [], [], []
    for f in range(3):
        lin = kernel.LinearKernel(2, float(z["lin_length_scale"][f]), float(z["lin_signal_variance"][f]))
        mat = kernel.MaternKernel(2, float(z["matern_length_scale"][f]), float(z["matern_signal_variance"][f]))
        with torch.no_grad():
            lin.center.copy_(torch.tensor(z["lin_center"][f]))
        m = cigp(kernel.SumKernel(lin, mat), float(z["log_beta"][f])).double().to(DEV)
        m.requires_grad_(False)
        x, y = torch.tensor(z["x_%d" % f], device=DEV), torch.tensor(z["y_%d" % f], device=DEV)
        models.append(m)
        data.append((x, y))
        members.append(m._cached_posterior(x, y)[0])
        noise.append(math.exp(-float(z["log_beta"][f])))
    coefs = [1.0] + [float(r) for r in z["rho"]]
    gst = F.PosteriorStack(members, coefs)
    gst.test_var_adds = noise
    return z, models, data, gst


@pytest.mark.parametrize("tag", ["zg", "acc"])
def test_staged_call_reproduces_the_reference_ar_fixture_at_every_level(tag):
    z, _, _, gst = ar_fixture()
    assert [p.n for p in gst.members] == [300, 300, 250]
    assert float(z["twin_distance"]) <= 1e-11
    assert all(p.tree is not None and [int(d["kfun"]) for d in p.tree[0]] == [LINEAR, M52] for p in gst.members)
    assert bool(np.any(z["lin_center"] != 0.0))
    steps, lr, acc = int(z["steps"]), float(z["lr"]), tag == "acc"
    sp = S.spec("ucb_var", kappa=float(z["kappa"]))
    X0 = torch.tensor(z["X0"])                           # [3, 6, 2]: six starts per level
    level = torch.arange(3).repeat_interleave(6)
    Z = stacked(gst, X0.reshape(18, 2).to(DEV), level, sp, steps, lr, acc, **BOTH)      # every level from one call
    assert is_staged(Z[3])
    for s in range(3):
        ref = (None, torch.tensor(z["trace_" + tag][s]), torch.tensor(z["hist_" + tag][s]))
        B = ST.loop_b(gst, X0[s], torch.full((6,), s), sp, steps, lr, acc)
        d0 = distance(B, ref)
        assert d0 <= 1e-10, "ill-conditioned case: d0 = %.2e" % d0
        bound = max(10.0 * d0, 1e-12)
        got = (None, Z[1][:, 6 * s:6 * s + 6], Z[2][:, 6 * s:6 * s + 6])
        print("fixture AR n300 %s level %d: d0 %.2e, bound %.2e, staged vs fixture %.2e, vs B %.2e" % (tag, s, d0, bound, distance(got, ref), distance(got, B)))
        assert distance(got, ref) <= bound and distance(got, B) <= bound
        assert rel(Z[0][6 * s:6 * s + 6], ref[2][-1]) <= bound      # the final points


def test_optimize_acqf_mf_selects_as_the_reference_rule_does_on_the_fixture():
    from fidelityfusion_amd import acq
    z, models, data, gst = ar_fixture()
    steps, lr = int(z["steps"]), float(z["lr"])
    sp = S.spec("ucb_var", kappa=float(z["kappa"]))
    rho = [float(r) for r in z["rho"]]
    for s in range(3):
        X0 = torch.tensor(z["X0"][s])
        ref_t, ref_h = torch.tensor(z["trace_zg"][s]), torch.tensor(z["hist_zg"][s])
        k_ref, best_ref = select(X0, ref_t, ref_h)
        B = ST.loop_b(gst, X0, torch.full((6,), s), sp, steps, lr)
        d0 = distance(B, (None, ref_t, ref_h))
        assert d0 <= 1e-10
        bound = max(10.0 * d0, 1e-12)
        kw = dict(rho=rho, level=s, steps=steps, lr=lr, acq="ucb_var", kappa=float(z["kappa"]), **BOTH)
        best = acq.optimize_acqf_mf(models, data, X0.to(DEV), **kw)
        final = acq.optimize_acqf_mf(models, data, X0.to(DEV), return_best_only=False, **kw)
        Z = stacked(gst, X0.to(DEV), torch.full((6,), s), sp, steps, lr, **BOTH)
        assert is_staged(Z[3]) and torch.equal(final, Z[0])      # optimize_acqf_mf took the staged call
        scale = float(ref_h.abs().max())
        e_best, e_final = float((best.cpu() - best_ref).abs().max()) / scale, float((final.cpu() - ref_h[-1]).abs().max()) / scale
        print("optimize_acqf_mf n300 level %d: selected step %d, d0 %.2e, best_x %.2e, final %.2e" % (s, k_ref, d0, e_best, e_final))
        assert k_ref >= 0
        assert e_best <= bound and e_final <= bound, (e_best, e_final, bound)


# ---- 9. routing ---------------------------------------------------------------------------------------------------------------------------
def _per_step_loop(r, B):
    assert r[3]["fused"] is False and "staged" not in r[3]
    assert distance(r, B) <= 1e-12      # the same launches in the same order as loop B


def test_a_composed_model_of_300_points_needs_both_keywords():
    c = T.make_case(300, 2, 19, "sum_lin_m52", seed=31)
    post, sp = T.gpu_posterior(c), T.spec("ucb", var_add=0.05)
    X0 = c["X0"].to(DEV)
    assert post.acq_tree_staged_ok(X0) and not post.acq_tree_fusable(X0) and not post.acq_staged_ok(X0)
    B = T.loop_b(post, X0, sp, 6, LR)
    _per_step_loop(single(post, X0, sp, 6, LR), B)
    _per_step_loop(single(post, X0, sp, 6, LR, fuse_composed=True), B)
    _per_step_loop(single(post, X0, sp, 6, LR, staged=True), B)
    _per_step_loop(single(post, X0, sp, 6, LR, staged="force"), B)
    r = single(post, X0, sp, 6, LR, **BOTH)
    assert is_staged(r[3]) and distance(r, B) <= 1e-10


def test_a_stack_with_a_composed_member_of_300_points_needs_both_keywords():
    st, gst = big_stack(0)
    sp, X0, lv = STACK_ACQ["ucb"], st["X0"].to(DEV), st["level"]
    assert gst.acq_tree_staged_ok(X0) and not gst.acq_tree_fusable(X0) and not gst.acq_staged_ok(X0)
    B = ST.loop_b(gst, X0, lv, sp, 6, LR)
    _per_step_loop(stacked(gst, X0, lv, sp, 6, LR), B)
    _per_step_loop(stacked(gst, X0, lv, sp, 6, LR, fuse_composed=True), B)
    _per_step_loop(stacked(gst, X0, lv, sp, 6, LR, staged=True), B)
    assert is_staged(stacked(gst, X0, lv, sp, 6, LR, **BOTH)[3])


def test_with_both_keywords_a_small_model_keeps_its_one_launch_call_bit_for_bit():
    c, post, _, _, _, one = forced(0)
    sp, steps = FORCED[0][4], FORCED[0][6]
    r = single(post, c["X0"].to(DEV), sp, steps, LR, **BOTH)
    assert r[3]["fused"] is True and not r[3].get("staged")
    assert torch.equal(r[0], one[0]) and torch.equal(r[1], one[1]) and torch.equal(r[2], one[2])
    st = ST.make_stack((40, 24, 17), 2, ("sum_lin_m52", "prod_ard_linc", "M32"), (1.0, 0.8, -1.3), 37, seed=810)
    gst = ST.gpu_stack(st)
    a = ST.fused(gst, st["X0"].to(DEV), st["level"], S.spec("ucb"), STEPS, LR)
    b = stacked(gst, st["X0"].to(DEV), st["level"], S.spec("ucb"), STEPS, LR, **BOTH)
    assert a[3]["fused"] is True and b[3]["fused"] is True and not b[3].get("staged")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_with_both_keywords_a_large_radial_model_takes_the_radial_staged_call():
    """a stack without a composed member: the radial entry, the same bits as with `staged=True` alone"""
    c, post, _, _, _, Z = G.traj(0)
    r = single(post, c["X0"].to(DEV), G.TRAJ[0][4], G.STEPS, G.LR, **BOTH)
    assert is_staged(r[3])
    assert torch.equal(r[0], Z[0]) and torch.equal(r[1], Z[1]) and torch.equal(r[2], Z[2])


@pytest.mark.parametrize("what", ["n", "d", "cpu"])
def test_fallback_outside_the_limits(what):
    sp = T.spec("ucb", var_add=0.05)
    n, d = {"n": (2049, 1), "d": (300, 2), "cpu": (300, 1)}[what]
    c = T.make_case(n, 2, 19, "sum_lin_m52", seed=31)
    if d > 1:
        c["Y"] = torch.cat([c["Y"], torch.cos(3.0 * c["X"].sum(1)).reshape(n, 1)], 1)
    X0 = c["X0"] if what == "cpu" else c["X0"].to(DEV)
    post = T.gpu_posterior(c)
    assert not post.acq_tree_staged_ok(X0)
    keep = X0.clone()
    r = single(post, X0, sp, 4, LR, **BOTH)
    assert torch.equal(X0, keep) and all(t.device == X0.device for t in r[:3])
    _per_step_loop(r, T.loop_b(post, X0, sp, 4, LR))


def test_a_tree_of_five_leaves_is_never_routed_to_the_staged_call():
    """a `Posterior` cannot be built on more than four leaves (`kdesc._tree_spec`), so the predicate and the route are what there is to
    check: a fifth descriptor sends the problem to the per-step loop"""
    from fidelityfusion_amd.posterior import _TreePosterior
    c = T.make_case(300, 2, 9, "chain4", seed=21)
    post = T.gpu_posterior(c)
    X0 = c["X0"].to(DEV)
    assert post.acq_tree_staged_ok(X0)
    assert _TreePosterior([post], [1.0])._acq_route(X0, True, True)[1] is True
    post.tree[0].append(dict(post.tree[0][0]))
    try:
        assert not post.acq_tree_staged_ok(X0)
        assert _TreePosterior([post], [1.0])._acq_route(X0, True, True) == (None, False)
    finally:
        post.tree[0].pop()


# ---- 10. the C ABI -------------------------------------------------------------------------------------------------------------------------
# member 0: chain4 (four leaves), member 1: one radial kernel, member 2: sum_lin_m52.  Everything ffgp_acq_optimize_stack_tree refuses, with
# the staged rule on n in place of its own, and Q D beyond INT_MAX
REFUSALS = [dict(b, n=2049) if b.get("n") == 257 else b for b in ST.REFUSALS] + [dict(Q=1 << 30)]


@pytest.fixture(scope="module")
def abi_stack():
    st = ST.make_stack((40, 24, 17), 2, ("chain4", "M32", "sum_lin_m52"), (1.0, 0.8, -1.3), 21, seed=701)
    return st, ST.gpu_stack(st)


@pytest.mark.parametrize("bad", REFUSALS, ids=lambda b: ",".join("%s=%s" % kv for kv in b.items()))
def test_c_abi_refuses_before_anything_is_enqueued(abi_stack, bad):
    from fidelityfusion_amd import _lib
    st, gst = abi_stack
    assert _lib.FFGP_ACQ_STAGED_MAX_N == 2048 and sum(1 for b in REFUSALS if b.get("n") == 2049) == 2      # the cap + 1
    kw = dict(bad)
    kw.setdefault("steps", 4)
    rc, X, state, trace, hist, grad = raw(gst, st["X0"], st["level"], S.spec("ucb"), accumulate=1, **kw)
    assert rc == _lib.FFGP_ERR_ARG
    assert torch.equal(X.cpu(), st["X0"]) and not bool(state.any()) and bool((trace == -7.0).all())
    assert bool((hist == -7.0).all()) and bool((grad == -7.0).all())


@pytest.mark.parametrize("accumulate", [0, 1])
def test_c_abi_accepted_call_runs(abi_stack, accumulate):
    st, gst = abi_stack
    sp = S.spec("ucb")
    tab = gst._member_table(gst.test_var_adds, [])
    assert not tab[0].w_dev and not tab[0].amp_dev and tab[1].w_dev      # a tree member carries no kernel of its own
    # ... and whatever stands in those fields is not read: an unmodified copy of the tree, a kfun no radial member may have
    rc, X, state, trace, hist, grad = raw(gst, st["X0"], st["level"], sp, steps=4, lr=0.01, accumulate=accumulate, member=0, w_dev=None,
                                          amp_dev=None, kfun=99, tree=(0, {}))
    assert rc == 0
    A = ST.loop_a(st, st["X0"], st["level"], sp, 4, 0.01, bool(accumulate))
    assert rel(trace, A[1]) <= 1e-10 and rel(hist, A[2]) <= 1e-10 and torch.equal(X, hist[-1])
    assert bool(state[1].gt(0).any()) and bool(state[2].ne(0).any()) == bool(accumulate)
    # the gradient output is that of the LAST evaluation alone: the points before the fourth step
    _, g, _ = ST.cpu_eval(st, A[2][3], st["level"], sp)
    assert rel(grad, g) <= 1e-8


def test_c_abi_accepted_call_in_evaluate_mode(abi_stack):
    st, gst = abi_stack
    sp = S.spec("ei", f_best=0.3)
    rc, X, state, trace, hist, grad = raw(gst, st["X0"], st["level"], sp, steps=0, null=("opt", "state"))      # neither is needed
    assert rc == 0
    assert torch.equal(X.cpu(), st["X0"]) and not bool(state.any()) and torch.equal(hist[0].cpu(), st["X0"])
    a, g, _ = ST.cpu_eval(st, st["X0"], st["level"], sp)
    assert rel(trace[0], a) <= 1e-10 and rel(grad, g) <= 1e-8
