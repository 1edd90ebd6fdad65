"""The acquisition optimiser on a NAR chain with COMPOSED-kernel members past 256 training points: the launch-per-stage loop inside one
library call (ffgp_acq_optimize_chain_tree_staged, csrc/acq_staged_chain_tree.hip; `fuse_composed="staged", staged=True` on
PosteriorChain.optimize_acquisition and acq.optimize_acqf_nar) against the references test_gpu_acq_chain_tree.py is written against --
plain fp64 torch on the CPU, the per-step loop on the GPU, the one-launch chain kernel where it still serves -- its sibling entries, and
a fixture of the reference's own loop on its NAR with SumKernel(LinearKernel, MaternKernel) fidelities at its demo's sizes
(tests/golden/mf_acq_nar_sum_n300.npz, written by tests/golden/gen_nar_acq_sum_staged_goldens.py).

Helpers, recipes and bars are test_gpu_acq_chain_tree.py's, test_gpu_acq_chain_staged.py's and test_gpu_acq_staged.py's, imported and
unchanged.  Evaluate mode (steps = 0): values rel. 1e-10, gradients rel. 1e-8 against CPU autograd.  Trajectories: (A) the CPU loop and
(B) the per-step GPU loop differ by rounding only; d0 = their distance is the yardstick, max(10 d0, 1e-12) the bound, a case with
d0 > 1e-10 fails as ill-conditioned, and a CPU twin started one ulp away must stay within 1e-11 before anything is compared
(`yardstick`).  State: 3 + 5 steps equal 8 bit for bit.  level = k for all points is the cut chain bit for bit (the same Q, so the same
GEMM shapes); a point alone is held to 1e-13, since the GEMM's tile choice changes with Q.  Every case runs STEPS = 8 steps on the
smallest shapes that reach a boundary: a first member one row past the one-launch limit (257), a smaller member behind a larger one, a
chunk of 2 rows (130), two column tiles with a ragged second (Q = 70), DM = 16 with 4 chunks + 1 row (513) and a four-leaf tree in the
middle, F = 1 with Q = 1, and the demo's (300, 300, 250)."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_acq_chain as CH                 # noqa: E402
import test_gpu_acq_chain_staged as CS          # noqa: E402
import test_gpu_acq_chain_tree as CT            # noqa: E402
import test_gpu_acq_tree as T                   # noqa: E402
from test_gpu_acq_chain import ACQ_CODE, DEV, LINEAR, M52, distance, rel, select, spec      # noqa: E402
from test_gpu_acq_chain_tree import cpu_eval, gpu_chain, loop_a, loop_b, make_chain, served      # noqa: E402
from test_gpu_acq_staged import STEPS, is_staged, yardstick      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(torch.float32)


# ---- the GPU side --------------------------------------------------------------------------------------------------------------------
def raw_staged(gch, Xq, level, sp, steps=0, lr=0.1, step0=0, Q=None, null=(), F=None, accumulate=0, acq=None, member=0, tree=None,
               tree_null=None, state_in=None, **over):
    """ffgp_acq_optimize_chain_tree_staged through ctypes: test_gpu_acq_chain_tree.raw_call with the staged entry and the same keywords.
    Returns (status, X, state, trace, hist, grad), every buffer pre-filled with a sentinel."""
    from fidelityfusion_amd import _lib
    keep = []
    tab = gch._member_table(gch.test_var_adds, keep)
    trees = gch._tree_table()
    for k, v in over.items():
        setattr(tab[member], k, v)
    if tree is not None:
        trees[tree[0]] = T._tree_copy(gch.members[tree[0]], keep, **tree[1])
    if tree_null is not None:
        trees[tree_null] = C.POINTER(_lib.KTree)()
    Qn, D = Xq.shape
    X = Xq.to(DEV).clone().contiguous()
    state = torch.zeros((3, Qn, D), device=DEV)
    if state_in is not None:
        state[0], state[1] = state_in[0].to(DEV), state_in[1].to(DEV)
    trace = torch.full((max(steps, 1), Qn), -7.0, device=DEV)
    hist = torch.full((max(steps, 0) + 1, Qn, D), -7.0, device=DEV)
    grad = torch.full((Qn, D), -7.0, device=DEV)
    lv = None if level is None else level.to(device=DEV, dtype=torch.int32).contiguous()
    s = _lib.AcqChain(F=gch.F if F is None else F, members=None if "members" in null else tab, level_dev=None if lv is None else lv.data_ptr(),
                      var_floor=sp["var_floor"], acq=ACQ_CODE[sp["acq"]] if acq is None else acq, kappa=sp["kappa"], xi=sp["xi"],
                      f_best=sp["f_best"], accumulate_grad=accumulate)
    opt = _lib.Adam(lr, 0.9, 0.999, 1e-8)
    ptr = lambda name, t: None if name in null else C.c_void_p(t.data_ptr())
    rc = _lib.lib.ffgp_acq_optimize_chain_tree_staged(None if "h" in null else gch.members[0]._h(), None if "s" in null else C.byref(s),
                                                      None if "trees" in null else trees, ptr("X", X), Qn if Q is None else Q, steps,
                                                      None if "opt" in null else C.byref(opt), ptr("state", state), step0,
                                                      ptr("trace", trace), ptr("hist", hist), ptr("grad", grad))
    torch.cuda.synchronize()
    return rc, X, state, trace, hist, grad


def raw_as_result(gch, X0, level, sp, steps, lr, accumulate=False):
    rc, X, _, trace, hist, _ = raw_staged(gch, X0, level, sp, steps=steps, lr=lr, accumulate=1 if accumulate else 0)
    assert rc == 0
    return X, trace, hist


def staged(gch, X0, level, sp, steps, lr, accumulate=False, state=None, fuse_composed="staged", staged=True):
    """the public call with the two opt-in keywords"""
    return CT.fused(gch, X0, level, sp, steps, lr, accumulate, state=state, fuse_composed=fuse_composed, staged=staged)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
#          ns                 D   members                                       Q   gaps      acquisition                 seed
CASES = [((257, 40, 130), 1, ("sum_lin_m52", "sum_linc_m32", "SE"), 37, None, spec("ucb"), 940),
         ((40, 300), 2, ("M32", "prod_linc_se"), 70, None, spec("ei", f_best=0.3), 941),
         ((33, 513, 16), 15, ("SE", "balanced4", "chain3"), 21, (5, 11), spec("ucb_var", kappa=0.4), 942),      # every level and -1 (raw)
         ((300,), 2, ("sum_lin_m52",), 1, None, spec("ucb"), 943),
         ((300, 300, 250), 2, ("sum_lin_m52", "sum_linc_m32", "sum_lin_m52"), 37, None, spec("ucb"), 944)]


@functools.lru_cache(maxsize=None)
def case(i):
    ns, D, kinds, Q, gaps, _, seed = CASES[i]
    level = None if gaps is None else CT._levels_with_gaps(Q, len(ns), gaps)
    ch = make_chain(ns, D, kinds, Q, seed=seed, level=level)
    return ch, gpu_chain(ch)


# ---- 1. values and gradients (steps = 0) against CPU autograd --------------------------------------------------------------------------
@pytest.mark.parametrize("acq", ["ucb", "ei", "ucb_var"])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_evaluate_matches_cpu_autograd(i, acq):
    ch, gch = case(i)
    sp = spec(acq, f_best=0.3, kappa=2.0 if acq != "ucb_var" else 0.4)
    rc, X, _, trace, _, grad = raw_staged(gch, ch["X0"], ch["level"], sp)
    assert rc == 0
    assert torch.equal(X.cpu(), ch["X0"])      # evaluate mode: nothing moves
    on = served(ch)
    off = torch.nonzero(ch["level"] < 0).reshape(-1)
    a, g = cpu_eval(ch, ch["X0"][on], ch["level"][on], sp)
    ev, eg = rel(trace[0][on.to(DEV)], a), rel(grad[on.to(DEV)], g)
    print("staged chain %s %s D=%d %s: value rel %.2e, gradient rel %.2e" % (CASES[i][0], CASES[i][2], CASES[i][1], acq, ev, eg))
    assert ev <= 1e-10, ev
    assert eg <= 1e-8, eg
    assert bool((trace[0][off.to(DEV)] == 0.0).all()) and bool((grad[off.to(DEV)] == 0.0).all())      # a negative level: value 0, gradient 0


@pytest.mark.parametrize("i", [0, 2])
def test_evaluate_without_levels(i):
    ch, gch = case(i)
    sp = spec("ucb")
    rc, _, _, trace, _, grad = raw_staged(gch, ch["X0"], None, sp)
    assert rc == 0
    a, g = cpu_eval(ch, ch["X0"], None, sp)
    assert rel(trace[0], a) <= 1e-10 and rel(grad, g) <= 1e-8


# ---- 2. trajectories against the CPU loop and the per-step GPU loop ------------------------------------------------------------------
TRAJ = [(i, acc) for i in range(len(CASES)) for acc in (False, True)]


@functools.lru_cache(maxsize=None)
def traj(i, accumulate):
    """case i once: the CPU loop and its twin and loop B on the served points, the staged call on all of them -- shared by the tests
    below and left unchanged"""
    ch, gch = case(i)
    sp = CASES[i][5]
    lr = 0.01 if accumulate else 0.1
    on = served(ch)
    X0, lv = ch["X0"][on], ch["level"][on]
    A = loop_a(ch, X0, lv, sp, STEPS, lr, accumulate)
    twin = loop_a(ch, X0 * (1.0 + 2e-16), lv, sp, STEPS, lr, accumulate)
    B = loop_b(gch, X0, lv, sp, STEPS, lr, accumulate)
    if len(on) == ch["X0"].shape[0]:      # every level is one Python accepts: through the public call
        X0d = ch["X0"].to(DEV)
        keep = X0d.clone()
        Z = staged(gch, X0d, ch["level"], sp, STEPS, lr, accumulate)
        assert torch.equal(X0d, keep)      # X0 is left untouched
        assert is_staged(Z[3]) and Z[3]["step"] == STEPS and ("grad_sum" in Z[3]) == accumulate
    else:
        Z = raw_as_result(gch, ch["X0"], ch["level"], sp, STEPS, lr, accumulate) + (None,)
    return ch, gch, A, twin, B, Z, lr


@pytest.mark.parametrize("i,accumulate", TRAJ)
def test_trajectory_follows_both_references(i, accumulate):
    ch, gch, A, twin, B, Z, lr = traj(i, accumulate)
    d0, bound = yardstick(A, twin, B)
    on = served(ch).to(DEV)
    got = (Z[0][on], Z[1][:, on], Z[2][:, on])
    dA, dB = distance(got, A), distance(got, B)
    print("staged chain-tree %d accumulate=%s: d0 %.2e, bound %.2e, staged vs A %.2e, vs B %.2e" % (i, accumulate, d0, bound, dA, dB))
    Q, D = ch["X0"].shape
    assert Z[1].shape == (STEPS, Q) and Z[2].shape == (STEPS + 1, Q, D)
    assert torch.equal(Z[0], Z[2][-1]) and torch.equal(Z[2][0].cpu(), ch["X0"])
    assert dA <= bound, (dA, bound)
    assert dB <= bound, (dB, bound)
    for q in torch.nonzero(ch["level"] < 0).reshape(-1).tolist():      # a negative level: value 0 and the point does not move
        assert bool((Z[1][:, q] == 0.0).all()) and bool((Z[2][:, q].cpu() == ch["X0"][q]).all())


# ---- 3. the sibling entries --------------------------------------------------------------------------------------------------------------
def test_an_all_radial_chain_follows_the_radial_staged_entry():
    """trees[f] = NULL for every member: the model ffgp_acq_optimize_chain_staged serves, each member run as a one-leaf record and both
    self terms exact zeros; the leaves' derivative is combined in another order, so the bound is the trajectory bound"""
    ch = CH.make_chain((257, 40, 130), 1, 37, seed=950)
    gch = CH.gpu_chain(ch)
    sp = spec("ucb")
    A = CH.loop_a(ch, ch["X0"], ch["level"], sp, STEPS, 0.1)
    twin = CH.loop_a(ch, ch["X0"] * (1.0 + 2e-16), ch["level"], sp, STEPS, 0.1)
    B = CH.loop_b(gch, ch["X0"], ch["level"], sp, STEPS, 0.1)
    d0, bound = yardstick(A, twin, B)
    rc0, X0_, _, t0, h0, _ = CS.raw_staged(gch, ch["X0"], ch["level"], sp, steps=STEPS)
    rc1, X1_, _, t1, h1, _ = raw_staged(gch, ch["X0"], ch["level"], sp, steps=STEPS)
    assert rc0 == 0 and rc1 == 0
    new, old = (X1_, t1, h1), (X0_, t0, h0)
    print("all radial: d0 %.2e, new entry vs radial staged entry %.2e, vs A %.2e" % (d0, distance(new, old), distance(new, A)))
    assert distance(new, old) <= bound and distance(new, A) <= bound and distance(new, B) <= bound


def test_a_one_member_chain_follows_the_staged_stack_tree_entry():
    """F = 1 with a tree member of 300 points: the model ffgp_acq_optimize_stack_tree_staged serves as the stack of one"""
    ch, gch, A, twin, B, Z, lr = traj(3, False)
    sp = CASES[3][5]
    _, bound = yardstick(A, twin, B)
    post = gch.members[0]
    assert post.tree is not None and post.n == 300
    one = post.optimize_acquisition(ch["X0"].to(DEV), steps=STEPS, lr=lr, acq=sp["acq"], kappa=sp["kappa"], var_floor=sp["var_floor"],
                                    var_add_all=ch["members"][0]["var_add"], fuse_composed=True, staged=True)
    assert is_staged(one[3]) and is_staged(Z[3])
    print("F = 1: chain call vs staged stack-tree call %.2e (bound %.2e)" % (distance(Z, one), bound))
    assert distance(Z, one) <= bound and distance(one, A) <= bound


@functools.lru_cache(maxsize=None)
def forced():
    """(40, 256): the one-launch limit, where both calls serve"""
    sp = spec("ucb")
    ch = make_chain((40, 256), 2, ("sum_lin_m52", "sum_linc_m32"), 37, seed=951)
    gch = gpu_chain(ch)
    A = loop_a(ch, ch["X0"], ch["level"], sp, STEPS, 0.1)
    twin = loop_a(ch, ch["X0"] * (1.0 + 2e-16), ch["level"], sp, STEPS, 0.1)
    B = loop_b(gch, ch["X0"], ch["level"], sp, STEPS, 0.1)
    one = staged(gch, ch["X0"].to(DEV), ch["level"], sp, STEPS, 0.1, fuse_composed=True, staged=False)
    return ch, gch, sp, A, twin, B, one


def test_forced_staged_call_follows_the_one_launch_call():
    ch, gch, sp, A, twin, B, one = forced()
    d0, bound = yardstick(A, twin, B)
    Z = staged(gch, ch["X0"].to(DEV), ch["level"], sp, STEPS, 0.1, staged="force")
    assert one[3]["fused"] is True and not one[3].get("staged") and is_staged(Z[3])
    dO, dA = distance(Z, one), distance(Z, A)
    print("forced (40, 256): d0 %.2e, bound %.2e, staged vs one-launch %.2e, vs A %.2e" % (d0, bound, dO, dA))
    assert dO <= bound and dA <= bound, (dO, dA, bound)
    # "staged" with staged=True leaves a one-launch chain on its call, bit for bit
    r = staged(gch, ch["X0"].to(DEV), ch["level"], sp, STEPS, 0.1)
    assert r[3]["fused"] is True and not r[3].get("staged")
    assert torch.equal(r[0], one[0]) and torch.equal(r[1], one[1]) and torch.equal(r[2], one[2])


# ---- 4. state ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,accumulate", [(0, False), (0, True), (4, True)])
def test_state_continues_the_optimiser_bit_for_bit(i, accumulate):
    ch, gch, _, _, _, Z, lr = traj(i, accumulate)
    sp = CASES[i][5]
    X1, t1, h1, s1 = staged(gch, ch["X0"].to(DEV), ch["level"], sp, 3, lr, accumulate)
    assert is_staged(s1) and s1["step"] == 3
    X2, t2, h2, s2 = staged(gch, X1, ch["level"], sp, 5, lr, accumulate, state=s1)
    assert is_staged(s2) and s2["step"] == STEPS == 8
    assert torch.equal(X2, Z[0])
    assert torch.equal(torch.cat([t1, t2]), Z[1])
    assert torch.equal(torch.cat([h1[:-1], h2]), Z[2])
    assert torch.equal(s2["exp_avg"], Z[3]["exp_avg"]) and torch.equal(s2["exp_avg_sq"], Z[3]["exp_avg_sq"])
    if accumulate:
        assert torch.equal(s2["grad_sum"], Z[3]["grad_sum"]) and bool(s2["grad_sum"].ne(0).any())


def test_state_moves_to_and_from_the_one_launch_entry():
    ch, gch, sp, A, twin, B, one = forced()
    _, bound = yardstick(A, twin, B)
    # ffgp_acq_optimize_chain_tree, then the staged entry
    X1, t1, h1, s1 = staged(gch, ch["X0"].to(DEV), ch["level"], sp, 3, 0.1, fuse_composed=True, staged=False)
    assert s1["fused"] is True
    X2, t2, h2, s2 = staged(gch, X1, ch["level"], sp, 5, 0.1, state=s1, staged="force")
    assert is_staged(s2) and s2["step"] == 8
    got = (X2, torch.cat([t1, t2]), torch.cat([h1[:-1], h2]))
    assert distance(got, one) <= bound and distance(got, A) <= bound
    # ... and back
    X1, t1, h1, s1 = staged(gch, ch["X0"].to(DEV), ch["level"], sp, 3, 0.1, staged="force")
    assert is_staged(s1)
    X2, t2, h2, s2 = staged(gch, X1, ch["level"], sp, 5, 0.1, state=s1, fuse_composed=True, staged=False)
    assert s2["fused"] is True and s2["step"] == 8
    got = (X2, torch.cat([t1, t2]), torch.cat([h1[:-1], h2]))
    assert distance(got, one) <= bound and distance(got, A) <= bound


# ---- 5. levels and points ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [False, True])
def test_a_level_for_all_points_is_the_cut_chain(accumulate):
    from fidelityfusion_amd import functional as F
    ch, gch = case(0)
    sp, X0 = CASES[0][5], ch["X0"]
    lr = 0.01 if accumulate else 0.1
    top = raw_as_result(gch, X0, None, sp, STEPS, lr, accumulate)
    for k in range(ch["F"]):
        # the same Posterior objects: a member factored again has its alpha solved on other inverted diagonal blocks
        cut_chain = F.PosteriorChain(gch.members[:k + 1])
        cut_chain.test_var_adds = gch.test_var_adds[:k + 1]
        cut = raw_as_result(cut_chain, X0, None, sp, STEPS, lr, accumulate)
        lev = raw_as_result(gch, X0, torch.full((X0.shape[0],), k), sp, STEPS, lr, accumulate)
        assert torch.equal(cut[0], lev[0]) and torch.equal(cut[1], lev[1]) and torch.equal(cut[2], lev[2])
        if k < ch["F"] - 1:
            assert not torch.equal(cut[1], top[1])      # the members above k do change the result
        else:
            assert torch.equal(cut[1], top[1]) and torch.equal(cut[2], top[2])      # level = F - 1 everywhere is level_dev = NULL


def test_a_point_does_not_depend_on_its_neighbours_or_their_levels():
    ch, gch, _, _, _, Z, lr = traj(0, False)
    sp, X0, lv = CASES[0][5], ch["X0"].to(DEV), ch["level"]
    for q in (0, 20, 36):      # alone: only its own member's chains run, and the GEMM sees one column
        r = staged(gch, X0[q:q + 1].contiguous(), lv[q:q + 1], sp, STEPS, lr)
        d = max(rel(r[1][:, 0], Z[1][:, q]), rel(r[2][:, 0], Z[2][:, q]))
        print("point %d (level %d) alone: %.2e" % (q, int(lv[q]), d))
        assert d <= 1e-13, d
    idx = torch.arange(X0.shape[0] - 1, -1, -1)      # in another column, beside other neighbours
    r = staged(gch, X0[idx.to(DEV)].contiguous(), lv[idx], sp, STEPS, lr)
    d = max(rel(r[1], Z[1][:, idx.to(DEV)]), rel(r[2], Z[2][:, idx.to(DEV)]))
    print("all points in reverse order: %.2e" % d)
    assert d <= 1e-13, d


def test_c_abi_reads_a_negative_level_as_no_member():
    """value 0, gradient 0, the point does not move; its neighbours are served bit for bit as without it (the same Q)"""
    ch, gch = case(0)
    sp = spec("ucb")
    lv = ch["level"].clone()
    lv[3] = -1
    lv[36] = -5
    rc, X, _, trace, hist, grad = raw_staged(gch, ch["X0"], lv, sp, steps=3, lr=0.1)
    ref = raw_staged(gch, ch["X0"], ch["level"], sp, steps=3, lr=0.1)
    assert rc == 0 and ref[0] == 0
    for q in (3, 36):
        assert bool((trace[:, q] == 0.0).all()) and bool((grad[q] == 0.0).all()) and torch.equal(X[q].cpu(), ch["X0"][q])
        assert torch.equal(hist[:, q].cpu(), ch["X0"][q].expand(4, ch["D"]))
    others = [q for q in range(ch["X0"].shape[0]) if q not in (3, 36)]
    assert torch.equal(trace[:, others], ref[3][:, others]) and torch.equal(hist[:, others], ref[4][:, others])
    assert torch.equal(grad[others], ref[5][others])
    # every level negative: no member runs at all
    rc, X, _, trace, hist, grad = raw_staged(gch, ch["X0"], torch.full_like(lv, -1), sp, steps=2, lr=0.1)
    assert rc == 0 and not bool(trace.any()) and not bool(grad.any()) and torch.equal(X.cpu(), ch["X0"])


# ---- 6. the term neither staged parent has: the share of k_s(z, z) that depends on the mean below ---------------------------------------
def _edited(w_mean, c_mean, ns=(40, 300), seed=960):
    D = 2

    def edit(leaves):
        leaves[0]["w"][D] = w_mean
        leaves[0]["center"][D] = c_mean
    ch = make_chain(ns, D, ("SE", "sum_linc_m32"), 19, seed=seed, edits={1: edit})
    assert ch["members"][1]["leaves"][0]["kfun"] == LINEAR
    return ch, gpu_chain(ch)


def test_a_linear_leaf_blind_to_the_mean_gives_the_chain_no_self_term():
    """weight 0 on the mean coordinate: k(z, z) does not depend on u, su is gv times an exact 0, and the leaf's centre there is multiplied
    by 0 wherever it is read -- two chains that differ in that centre alone are the same bit for bit"""
    sp = spec("ucb_var", kappa=0.4)
    (ch, g0), (_, g1) = _edited(0.0, 0.3), _edited(0.0, 5.0)
    r0, r1 = raw_as_result(g0, ch["X0"], ch["level"], sp, STEPS, 0.1), raw_as_result(g1, ch["X0"], ch["level"], sp, STEPS, 0.1)
    assert all(torch.equal(x, y) for x, y in zip(r0, r1))
    e0, e1 = raw_staged(g0, ch["X0"], ch["level"], sp), raw_staged(g1, ch["X0"], ch["level"], sp)
    assert torch.equal(e0[5], e1[5])
    a, g = cpu_eval(ch, ch["X0"], ch["level"], sp)
    assert rel(e0[3][0], a) <= 1e-10 and rel(e0[5], g) <= 1e-8


def test_the_self_term_reaches_the_chain_through_the_mean_coordinate():
    """the top member's linear leaf weighs, and is centred on, the mean coordinate; levels mixed.  Without su = dk_s(z, z)/du in gu the
    gradient of the points that stop at the top member misses -gv su dm_0/dx: this comparison then fails (tried on a scratch build
    with that one line removed: gradient rel. 0.17 here, and eight of the ten trajectory cases fail as well)"""
    sp = spec("ucb_var", kappa=0.4)
    ch, gch = _edited(0.9, 0.4)
    assert bool((ch["level"] == 0).any()) and bool((ch["level"] == 1).any())
    rc, _, _, trace, _, grad = raw_staged(gch, ch["X0"], ch["level"], sp)
    assert rc == 0
    a, g = cpu_eval(ch, ch["X0"], ch["level"], sp)
    ev, eg = rel(trace[0], a), rel(grad, g)
    print("self term through u: value rel %.2e, gradient rel %.2e" % (ev, eg))
    assert ev <= 1e-10 and eg <= 1e-8, (ev, eg)
    # and the centre on that coordinate does count
    _, g2 = _edited(0.9, 5.0)
    assert not torch.equal(raw_staged(g2, ch["X0"], ch["level"], sp)[5], grad)


# ---- 7. the fixture of the reference's loop at (300, 300, 250) ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    from fidelityfusion_amd import functional as F, kernel
    from fidelityfusion_amd.cigp_v10 import cigp
    z = np.load(os.path.join(ROOT, "tests", "golden", "mf_acq_nar_sum_n300.npz"))
    models, data, members, noise = [], [], [], []
    for f in range(3):
        Df = 2 + (1 if f else 0)
        lin = kernel.LinearKernel(Df, float(z["lin_length_scale"][f]), float(z["lin_signal_variance"][f]))
        mat = kernel.MaternKernel(Df, float(z["matern_length_scale"][f]), float(z["matern_signal_variance"][f]))
        with torch.no_grad():
            lin.center.copy_(torch.tensor(z["lin_center_%d" % f]))
        m = cigp(kernel.SumKernel(lin, mat), float(z["log_beta"][f])).double().to(DEV)
        m.requires_grad_(False)
        x, y = torch.tensor(z["x_%d" % f], device=DEV), torch.tensor(z["y_%d" % f], device=DEV)
        models.append(m)
        data.append((x, y) if f == 0 else (x, [y, torch.full_like(y, 0.01)]))      # the trainer stores [y, y_var] above fidelity 0
        members.append(m._cached_posterior(x, y)[0])
        noise.append(math.exp(-float(z["log_beta"][f])))
    gch = F.PosteriorChain(members)
    gch.test_var_adds = noise
    return z, models, data, gch


@pytest.mark.parametrize("tag", ["zg", "acc"])
def test_staged_call_reproduces_the_reference_fixture_at_every_level(tag):
    z, _, _, gch = fixture()
    assert [p.n for p in gch.members] == [300, 300, 250]
    assert float(z["twin_distance"]) <= 1e-11
    assert all(p.tree is not None and [int(d["kfun"]) for d in p.tree[0]] == [LINEAR, M52] for p in gch.members)
    steps, lr, acc = int(z["steps"]), float(z["lr"]), tag == "acc"
    sp = spec("ucb_var", kappa=float(z["kappa"]))
    X0 = torch.tensor(z["X0"])                           # [3, 6, 2]: six starts per level
    level = torch.arange(3).repeat_interleave(6)
    Z = staged(gch, X0.reshape(18, 2).to(DEV), level, sp, steps, lr, acc)      # every level from one call
    assert is_staged(Z[3])
    for s in range(3):
        ref = (None, torch.tensor(z["trace_" + tag][s]), torch.tensor(z["hist_" + tag][s]))
        B = loop_b(gch, X0[s], torch.full((6,), s), sp, steps, lr, acc)
        d0 = distance(B, ref)
        assert d0 <= 1e-10, "ill-conditioned case: d0 = %.2e" % d0
        bound = max(10.0 * d0, 1e-12)
        got = (None, Z[1][:, 6 * s:6 * s + 6], Z[2][:, 6 * s:6 * s + 6])
        print("fixture nar sum n300 %s level %d: d0 %.2e, bound %.2e, staged vs fixture %.2e, vs B %.2e" % (tag, s, d0, bound, distance(got, ref),
                                                                                                         distance(got, B)))
        assert distance(got, ref) <= bound and distance(got, B) <= bound
        assert rel(Z[0][6 * s:6 * s + 6], ref[2][-1]) <= bound      # the final points


def test_optimize_acqf_nar_selects_as_the_reference_rule_does_on_the_fixture():
    from fidelityfusion_amd import acq
    z, models, data, gch = fixture()
    steps, lr = int(z["steps"]), float(z["lr"])
    sp = spec("ucb_var", kappa=float(z["kappa"]))
    for s in range(3):
        X0 = torch.tensor(z["X0"][s])
        ref_t, ref_h = torch.tensor(z["trace_zg"][s]), torch.tensor(z["hist_zg"][s])
        k_ref, best_ref = select(X0, ref_t, ref_h)
        B = loop_b(gch, X0, torch.full((6,), s), sp, steps, lr)
        d0 = distance(B, (None, ref_t, ref_h))
        assert d0 <= 1e-10
        bound = max(10.0 * d0, 1e-12)
        kw = dict(level=s, steps=steps, lr=lr, acq="ucb_var", kappa=float(z["kappa"]), fuse_composed="staged", staged=True)
        best = acq.optimize_acqf_nar(models, data, X0.to(DEV), **kw)
        final = acq.optimize_acqf_nar(models, data, X0.to(DEV), return_best_only=False, **kw)
        Z = staged(gch, X0.to(DEV), torch.full((6,), s), sp, steps, lr)
        assert is_staged(Z[3]) and torch.equal(final, Z[0])      # optimize_acqf_nar took the staged call
        scale = float(ref_h.abs().max())
        e_best, e_final = float((best.cpu() - best_ref).abs().max()) / scale, float((final.cpu() - ref_h[-1]).abs().max()) / scale
        print("optimize_acqf_nar staged sum level %d: selected step %d, d0 %.2e, best_x %.2e, final %.2e" % (s, k_ref, d0, e_best, e_final))
        assert k_ref >= 0
        assert e_best <= bound and e_final <= bound, (e_best, e_final, bound)


# ---- 8. routing ---------------------------------------------------------------------------------------------------------------------------
def _keeps_the_loop(gch, X0, level, sp, accumulate=False, **kw):
    r = CT._fallback_equals_loop_b(gch, X0, level, sp, accumulate, steps=4, **kw)
    assert "staged" not in r[3]
    return r


def test_without_the_new_value_a_large_composed_chain_keeps_the_per_step_loop():
    ch, gch = case(1)      # (40, 300)
    X0, sp = ch["X0"].to(DEV), spec("ucb")
    assert gch.acq_chain_tree_staged_ok(X0) and not gch.acq_tree_fusable(X0) and not gch.acq_chain_staged_ok(X0)
    _keeps_the_loop(gch, X0, ch["level"], sp, fuse_composed=False)
    _keeps_the_loop(gch, X0, ch["level"], sp, fuse_composed=True, staged=True)
    _keeps_the_loop(gch, X0, ch["level"], sp, fuse_composed=True, staged="force")
    _keeps_the_loop(gch, X0, ch["level"], spec("ucb_var", kappa=0.4), accumulate=True, fuse_composed="staged", staged=False)
    assert is_staged(staged(gch, X0, ch["level"], sp, 4, 0.1)[3])
    with pytest.raises(ValueError, match="fuse_composed"):
        staged(gch, X0, ch["level"], sp, 4, 0.1, fuse_composed="force")


@pytest.mark.parametrize("what", ["n", "D", "F"])
def test_fallback_outside_the_limits(what):
    """n = 2049, D + 1 = 17, F = 9 with both keywords: the per-step loop"""
    sp = spec("ucb")
    if what == "F":
        ch = make_chain((12,) * 8 + (260,), 2, ("sum_lin_m52", "SE") * 4 + ("sum_lin_m52",), 19, seed=970)
    elif what == "D":
        ch = make_chain((40, 260), 16, ("M32", "sum_lin_m52"), 19, seed=971)
    else:
        ch = make_chain((40, 2049), 2, ("M32", "sum_lin_m52"), 19, seed=972)
    gch = gpu_chain(ch)
    X0 = ch["X0"].to(DEV)
    assert not gch.acq_chain_tree_staged_ok(X0)
    _keeps_the_loop(gch, X0, ch["level"], sp, fuse_composed="staged", staged=True)


def test_a_non_library_leaf_is_never_routed_to_the_staged_call():
    ch, gch = case(1)
    X0 = ch["X0"].to(DEV)
    assert gch._acq_route(X0, "staged", True) == (gch._acq_call_chain_trees_staged, True)
    gch.members[1].tree[0][1]["kfun"] = 6
    try:
        assert not gch.acq_chain_tree_staged_ok(X0) and gch._acq_route(X0, "staged", True) == (None, False)
    finally:
        gch.members[1].tree[0][1]["kfun"] = CT.SE
    assert gch.acq_chain_tree_staged_ok(X0)
    _keeps_the_loop(gch, X0.cpu(), ch["level"], spec("ucb"), fuse_composed="staged", staged=True)      # start points off the GPU


# ---- 9. the C ABI ---------------------------------------------------------------------------------------------------------------------------
# test_gpu_acq_chain_tree.py's list (null pointers, coefficients other than 1, bad trees, a wrong D on an upper member, Q = 0 among
# them) with the staged cap + 1 in place of the one-launch limit + 1
REFUSALS = [dict(b, n=2049) if b.get("n") == 257 else b for b in CT.REFUSALS]


@pytest.fixture(scope="module")
def abi_chain():
    ch = make_chain((40, 24, 17), 2, ("balanced4", "M32", "sum_lin_m52"), 21, seed=701)
    return ch, gpu_chain(ch)


@pytest.mark.parametrize("bad", REFUSALS, ids=lambda b: ",".join("%s=%s" % kv for kv in b.items()))
def test_c_abi_refuses_before_anything_is_enqueued(abi_chain, bad):
    from fidelityfusion_amd import _lib
    ch, gch = abi_chain
    assert _lib.FFGP_ACQ_STAGED_MAX_N == 2048 and sum(1 for b in REFUSALS if b.get("n") == 2049) == 2      # the cap + 1
    assert sum(1 for b in REFUSALS if "mean_coef" in b or "var_coef" in b) == 3 and not any(b.get("n") == 257 for b in REFUSALS)
    assert dict(Q=0) in REFUSALS and dict(null=("trees",)) in REFUSALS and dict(member=2, D=4) in REFUSALS
    kw = dict(bad)
    kw.setdefault("steps", 4)
    rc, X, state, trace, hist, grad = raw_staged(gch, ch["X0"], ch["level"], spec("ucb"), accumulate=1, **kw)
    assert rc == _lib.FFGP_ERR_ARG
    assert torch.equal(X.cpu(), ch["X0"]) and not bool(state.any()) and bool((trace == -7.0).all())
    assert bool((hist == -7.0).all()) and bool((grad == -7.0).all())


@pytest.mark.parametrize("accumulate", [0, 1])
def test_c_abi_accepted_call_runs(abi_chain, accumulate):
    ch, gch = abi_chain
    sp = spec("ucb")
    rc, X, state, trace, hist, grad = raw_staged(gch, ch["X0"], ch["level"], sp, steps=4, lr=0.01, accumulate=accumulate, member=0, w_dev=None,
                                                 amp_dev=None, kfun=99, tree=(0, {}))
    assert rc == 0
    A = loop_a(ch, ch["X0"], ch["level"], sp, 4, 0.01, bool(accumulate))
    assert rel(trace, A[1]) <= 1e-10 and rel(hist, A[2]) <= 1e-10 and torch.equal(X, hist[-1])
    assert bool(state[1].gt(0).any()) and bool(state[2].ne(0).any()) == bool(accumulate)
    _, g = cpu_eval(ch, A[2][3], ch["level"], sp)      # the gradient output is that of the LAST evaluation alone
    assert rel(grad, g) <= 1e-8
