"""The acquisition optimiser's Adam loop on a CHAIN of frozen posteriors whose members may carry COMPOSED kernels, in one launch
(ffgp_acq_optimize_chain_tree, csrc/acq_chain_tree.hip; PosteriorChain.optimize_acquisition(..., fuse_composed=True);
acq.optimize_acqf_nar(..., fuse_composed=True)) against plain fp64 torch on the CPU: test_gpu_acq_tree.py's restatement of the
reference's kernel formulas under test_gpu_acq_chain.py's nesting of the members (member f > 0 is queried at [x, mean of member f - 1],
the model reports the mean and the variance of the member a point stops at), and against the fixture of the reference's own loop on NAR
with SumKernel(LinearKernel, MaternKernel) per fidelity (tests/golden/mf_acq_nar_sum.npz, gen_nar_acq_sum_goldens.py).

Bars and method are test_gpu_acq_chain.py's, restated.  Evaluate mode (steps = 0): values rel. 1e-10, gradients rel. 1e-8 against CPU
autograd.  Trajectories: (A) the CPU loop and (B) the per-step loop on the GPU (`PosteriorChain.predict_diff` + torch.optim.Adam, what
the call runs without the keyword) do not contain the new kernel; d0 = their distance is the yardstick and max(10 d0, 1e-12) the bound;
a case with d0 > 1e-10 is ill-conditioned and fails rather than widening anything.  Before anything is compared, a CPU twin started at
X0 (1 + 2e-16) must stay within 1e-11.  Fall-backs against loop B: 1e-12.

Member recipe: test_gpu_acq_chain.py's data (X = 2 rand(n, D_f), above member 0 the last column in [-1, 1) entering y as + 0.5 u;
y = sin(2 sum x) + 0.1 randn; Sigma = K + (0.05 + 1e-6) I, var_add 0.05) under a kernel named by `kind`: a radial profile (one leaf, amp
1.3, w = 0.6 + rand) or a tree of TREES, whose leaves are test_gpu_acq_tree._leaf's on the member's own D_f inputs -- so a linear leaf
weighs, and is centred on, the mean coordinate as on any other.  A negative level (C only) stops at no member."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_acq_chain as CH      # noqa: E402
import test_gpu_acq_tree as T        # noqa: E402
from test_gpu_acq_chain import ACQ_CODE, DEV, LINEAR, M32, M52, NEG_INF, SE, acq_torch, distance, rel, run_loop, select, spec      # noqa: E402
from test_gpu_acq_tree import BALANCED, CHAIN, PRODUCT, SUM, _leaf      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 30
RADIAL = {"SE": SE, "M32": M32}
TREES = {
    # the reference's tree: SumKernel(LinearKernel, MaternKernel)
    "sum_lin_m52": T.TREES["sum_lin_m52"],
    "sum_linc_m32": lambda g, D: ([_leaf(g, D, LINEAR, 0.6, center=0.3), _leaf(g, D, M32, 1.2, 1.3)], CHAIN, (SUM,)),
    # k(z, z) depends on z, u included, through a product
    "prod_linc_se": lambda g, D: ([_leaf(g, D, LINEAR, 0.7, center=0.4), _leaf(g, D, SE, 1.3)], CHAIN, (PRODUCT,)),
    # (SE x Linear) + (Matern32 x RQ)
    "balanced4": T.TREES["balanced4"],
    # (Linear + SE) x Matern52
    "chain3": lambda g, D: ([_leaf(g, D, LINEAR, 0.5, center=0.2), _leaf(g, D, SE, 1.0), _leaf(g, D, M52, 0.9, 0.8)], CHAIN, (SUM, PRODUCT)),
}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(torch.float32)


# ---- the comparator: plain torch on the CPU ---------------------------------------------------------------------------------------
def kval(c, A, B):
    return T.leaf_value(A, B, c["leaves"][0]) if c["radial"] else T.tree_value(A, B, c)


def finish_member(c):
    n = c["X"].shape[0]
    c["L"] = torch.linalg.cholesky(kval(c, c["X"], c["X"]) + c["dadd"] * torch.eye(n))
    c["alpha"] = torch.cholesky_solve(c["Y"], c["L"])
    return c


def make_member(n, D, f, kind, seed, noise=0.05, edit=None):
    """member f of a chain on x [D]: D inputs for f = 0, D + 1 above (the last one stands for the mean below); `edit(leaves)` changes
    the leaves before the member is factored"""
    g = torch.Generator().manual_seed(seed)
    Df = D + (1 if f else 0)
    X = 2.0 * torch.rand(n, Df, generator=g)
    y = torch.sin(2.0 * X[:, :D].sum(1)) + 0.1 * torch.randn(n, generator=g)
    if f:
        X[:, D] -= 1.0
        y = y + 0.5 * X[:, D]
    c = {"X": X, "Y": y.reshape(n, 1), "dadd": noise + 1e-6, "var_add": noise, "kind": kind, "radial": kind in RADIAL}
    if c["radial"]:
        kfun = RADIAL[kind]
        c.update(w=0.6 + torch.rand(Df, generator=g), amp=1.3, kfun=kfun, kparam=1.3 if kfun == M32 else 1.0,
                 clamp=1e-30 if kfun == M32 else NEG_INF)
        c["leaves"] = [{"kfun": kfun, "amp": c["amp"], "kparam": c["kparam"], "center": None, "clamp": c["clamp"], "w": c["w"]}]
    else:
        c["leaves"], c["shape"], c["ops"] = TREES[kind](g, Df)
    if edit is not None:
        edit(c["leaves"])
    return finish_member(c)


def make_chain(ns, D, kinds, Q, seed, level=None, edits=None):
    g = torch.Generator().manual_seed(seed)
    members = [make_member(n, D, f, kinds[f], 100 * seed + f, edit=(edits or {}).get(f)) for f, n in enumerate(ns)]
    F = len(ns)
    return {"members": members, "F": F, "D": D, "X0": 2.0 * torch.rand(Q, D, generator=g),
            "level": (torch.arange(Q) * 7 + 2) % F if level is None else level}      # levels mixed inside every tile


def cpu_member(c, Z):
    Ks = kval(c, c["X"], Z)
    V = torch.linalg.solve_triangular(c["L"], Ks, upper=False)
    kss = c["amp"] if c["radial"] else kval(c, Z, Z).diagonal()      # phi(0) = 1 for every radial profile
    return Ks.T @ c["alpha"], kss - (V * V).sum(0) + c["var_add"]


def cpu_predict(ch, Xq, level):
    """NAR.forward per point: the chain is followed up to level[q] and the mean and variance of that member are kept"""
    F = ch["F"]
    lv = torch.full((Xq.shape[0],), F - 1) if level is None else level
    mean, var, low = torch.zeros(Xq.shape[0], 1), torch.zeros(Xq.shape[0]), None
    for f, c in enumerate(ch["members"][:int(lv.max()) + 1]):
        z = Xq if f == 0 else torch.cat([Xq, low.reshape(-1, 1)], dim=-1)
        m, v = cpu_member(c, z)
        low = m
        on = lv == f
        mean = torch.where(on.unsqueeze(1), m, mean)
        var = torch.where(on, v, var)
    return mean, var


def cpu_eval(ch, Xq, level, sp):
    X = Xq.clone().requires_grad_(True)
    a = acq_torch(*cpu_predict(ch, X, level), sp)
    (-a.sum()).backward()
    return a.detach().sum(1), X.grad


def loop_a(ch, X0, level, sp, steps, lr, accumulate=False):
    return run_loop(lambda X: cpu_predict(ch, X, level), X0.cpu(), sp, steps, lr, accumulate)


loop_b = CH.loop_b      # the per-step loop on the GPU: PosteriorChain.predict_diff (the members' predict_diff, nested) + torch.optim.Adam


# ---- the GPU side --------------------------------------------------------------------------------------------------------------------
def gpu_posterior(c):
    return CH.gpu_posterior(c) if c["radial"] else T.gpu_posterior(c)


def gpu_chain(ch, upto=None):
    from fidelityfusion_amd import functional as F
    k = ch["F"] if upto is None else upto
    gch = F.PosteriorChain([gpu_posterior(c) for c in ch["members"][:k]])
    gch.test_var_adds = [c["var_add"] for c in ch["members"][:k]]
    return gch


def fused(gch, X0, level, sp, steps, lr, accumulate=False, state=None, fuse_composed=True, **kw):
    return gch.optimize_acquisition(X0, steps=steps, lr=lr, acq=sp["acq"], kappa=sp["kappa"], xi=sp["xi"], f_best=sp["f_best"],
                                    var_floor=sp["var_floor"], level=None if level is None else level.to(DEV), var_adds=gch.test_var_adds,
                                    accumulate_grad=accumulate, state=state, fuse_composed=fuse_composed, **kw)


def raw_call(gch, Xq, level, sp, steps=0, lr=0.1, step0=0, Q=None, null=(), F=None, accumulate=0, acq=None, member=0, tree=None,
             tree_null=None, state_in=None, **over):
    """ffgp_acq_optimize_chain_tree through ctypes on the chain's own buffers; `over` overrides fields of member `member`, `tree` =
    (member, keyword arguments of test_gpu_acq_tree._tree_copy) replaces that member's tree by a modified copy, `tree_null` names a
    member whose tree pointer is passed as NULL, `null` names pointers to pass as NULL, `state_in` = (exp_avg, exp_avg_sq) starts from
    an optimiser's moments.  Returns (status, X, state, trace, hist, grad) -- every buffer pre-filled with a sentinel."""
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
    rc = _lib.lib.ffgp_acq_optimize_chain_tree(None if "h" in null else gch.members[0]._h(), None if "s" in null else C.byref(s),
                                               None if "trees" in null else trees, ptr("X", X), Qn if Q is None else Q, steps,
                                               None if "opt" in null else C.byref(opt), ptr("state", state), step0, ptr("trace", trace),
                                               ptr("hist", hist), ptr("grad", grad))
    torch.cuda.synchronize()
    return rc, X, state, trace, hist, grad


def raw_as_result(gch, X0, level, sp, steps, lr, accumulate=False):
    """(X, trace, hist) of the C entry on a fresh optimiser"""
    rc, X, _, trace, hist, _ = raw_call(gch, X0, level, sp, steps=steps, lr=lr, accumulate=1 if accumulate else 0)
    assert rc == 0
    return X, trace, hist


# ---- the cases: the smallest shapes that reach every path ----------------------------------------------------------------------------------
def _levels_with_gaps(Q, F, gaps):
    lv = (torch.arange(Q) * 7 + 2) % F
    lv[list(gaps)] = -1
    return lv


#          ns                 D   members                                       Q   levels                               acquisition
CASES = [((17, 130, 24), 1, ("sum_lin_m52", "sum_linc_m32", "SE"), 37, None, spec("ucb")),               # DM 2; a member smaller than its
                                                                                                          # predecessor, np crossing 128, a ragged
                                                                                                          # last tile; trees and a one-leaf member
         ((40, 256), 7, ("M32", "prod_linc_se"), 21, None, spec("ei", f_best=0.3)),                       # DM 8 at the n limit; the self term
                                                                                                          # through a product node
         ((33, 20, 16, 9), 15, ("SE", "balanced4", "M32", "chain3"), 16, (5, 11), spec("ucb_var", kappa=0.4))]      # DM 16; four leaves in the middle,
                                                                                                          # three on top; one tile with every level
                                                                                                          # and -1


@functools.lru_cache(maxsize=None)
def case(i):
    ns, D, kinds, Q, gaps, _ = CASES[i]
    level = None if gaps is None else _levels_with_gaps(Q, len(ns), gaps)
    ch = make_chain(ns, D, kinds, Q, seed=300 + i, level=level)
    return ch, gpu_chain(ch)


def served(ch):
    """the points with a level of their own (a negative level is C's way of switching a point off)"""
    return torch.nonzero(ch["level"] >= 0).reshape(-1)


# ---- values and gradients (steps = 0) against CPU autograd ----------------------------------------------------------------------------
@pytest.mark.parametrize("acq", ["ucb", "ei", "ucb_var"])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_evaluate_matches_cpu_autograd(i, acq):
    ch, gch = case(i)
    sp = spec(acq, f_best=0.3, kappa=2.0 if acq != "ucb_var" else 0.4)
    rc, X, _, trace, _, grad = raw_call(gch, ch["X0"], ch["level"], sp)
    assert rc == 0
    assert torch.equal(X.cpu(), ch["X0"])      # evaluate mode: nothing moves
    on = served(ch)
    off = torch.nonzero(ch["level"] < 0).reshape(-1)
    a, g = cpu_eval(ch, ch["X0"][on], ch["level"][on], sp)
    ev, eg = rel(trace[0][on.to(DEV)], a), rel(grad[on.to(DEV)], g)
    print("chain %s %s D=%d %s: value rel %.2e, gradient rel %.2e" % (CASES[i][0], CASES[i][2], CASES[i][1], acq, ev, eg))
    assert ev <= 1e-10, ev
    assert eg <= 1e-8, eg
    assert bool((trace[0][off.to(DEV)] == 0.0).all()) and bool((grad[off.to(DEV)] == 0.0).all())      # a negative level: value 0, gradient 0


def test_evaluate_without_levels_and_predict_diff():
    ch, gch = case(0)
    sp = spec("ucb")
    rc, _, _, trace, _, grad = raw_call(gch, ch["X0"], None, sp)
    assert rc == 0
    a, g = cpu_eval(ch, ch["X0"], None, sp)
    assert rel(trace[0], a) <= 1e-10 and rel(grad, g) <= 1e-8
    # predict_diff, the per-step loop's query, is the same nesting
    Q = ch["X0"].shape[0]
    for level in (ch["level"], None, 1):
        m, v = gch.predict_diff(ch["X0"].to(DEV), level=level, var_adds=gch.test_var_adds)
        mc, vc = cpu_predict(ch, ch["X0"], torch.full((Q,), level) if isinstance(level, int) else level)
        assert rel(m, mc) <= 1e-10 and rel(v, vc) <= 1e-10


# ---- trajectories ------------------------------------------------------------------------------------------------------------------
TRAJ = [(i, acc) for i in range(len(CASES)) for acc in (False, True)]


@functools.lru_cache(maxsize=None)
def traj(i, accumulate):
    """case i once: the CPU loop and its twin and loop B on the served points, the new entry on all of them -- shared by the tests
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
        Fz = fused(gch, X0d, ch["level"], sp, STEPS, lr, accumulate)
        assert torch.equal(X0d, keep)      # X0 is left untouched
        assert Fz[3]["fused"] is True and Fz[3]["step"] == STEPS and ("grad_sum" in Fz[3]) == accumulate
        Fz = Fz[:3]
    else:
        Fz = raw_as_result(gch, ch["X0"], ch["level"], sp, STEPS, lr, accumulate)
    return ch, gch, A, twin, B, Fz, lr


@pytest.mark.parametrize("i,accumulate", TRAJ)
def test_trajectory_follows_both_references(i, accumulate):
    ch, gch, A, twin, B, Fz, lr = traj(i, accumulate)
    dt_x, dt_t = rel(twin[2], A[2]), rel(twin[1], A[1])
    assert dt_x <= 1e-11 and dt_t <= 1e-11, (dt_x, dt_t)      # conditioning of the case, before anything is compared
    d0 = distance(B, A)
    assert d0 <= 1e-10, "ill-conditioned case: d0 = %.2e" % d0
    bound = max(10.0 * d0, 1e-12)
    on = served(ch).to(DEV)
    got = (Fz[0][on], Fz[1][:, on], Fz[2][:, on])
    dA, dB = distance(got, A), distance(got, B)
    print("chain %d accumulate=%s: twin %.2e / %.2e, d0 %.2e, bound %.2e, fused vs A %.2e, vs B %.2e" % (i, accumulate, dt_x, dt_t, d0, bound, dA, dB))
    Q, D = ch["X0"].shape
    assert Fz[1].shape == (STEPS, Q) and Fz[2].shape == (STEPS + 1, Q, D)
    assert torch.equal(Fz[0], Fz[2][-1]) and torch.equal(Fz[2][0].cpu(), ch["X0"])
    assert dA <= bound, (dA, bound)
    assert dB <= bound, (dB, bound)
    off = torch.nonzero(ch["level"] < 0).reshape(-1)
    for q in off.tolist():      # a negative level: value 0 and the point does not move
        assert bool((Fz[1][:, q] == 0.0).all()) and bool((Fz[2][:, q].cpu() == ch["X0"][q]).all())


def test_an_all_radial_chain_through_the_new_entry_follows_the_radial_chain_entry():
    """trees[f] = NULL for every member: the model ffgp_acq_optimize_chain serves, each member run as a one-leaf record and both self
    terms exact zeros; the leaves' derivative is combined in another order, so the bound is the trajectory bound"""
    ch = CH.make_chain((40, 24, 17), 2, 37, seed=400)
    gch = CH.gpu_chain(ch)
    sp = spec("ucb")
    A = CH.loop_a(ch, ch["X0"], ch["level"], sp, STEPS, 0.1)
    B = CH.loop_b(gch, ch["X0"], ch["level"], sp, STEPS, 0.1)
    d0 = distance(B, A)
    assert d0 <= 1e-10, "ill-conditioned case: d0 = %.2e" % d0
    bound = max(10.0 * d0, 1e-12)
    rc0, X0_, _, t0, h0, _ = CH.raw_call(gch, ch["X0"], ch["level"], sp, steps=STEPS)
    rc1, X1_, _, t1, h1, _ = raw_call(gch, ch["X0"], ch["level"], sp, steps=STEPS)
    assert rc0 == 0 and rc1 == 0
    new, old = (X1_, t1, h1), (X0_, t0, h0)
    print("all radial: d0 %.2e, new entry vs chain entry %.2e, vs A %.2e" % (d0, distance(new, old), distance(new, A)))
    assert distance(new, old) <= bound and distance(new, A) <= bound and distance(new, B) <= bound


def test_one_member_chain_is_the_single_posterior_tree_call():
    """F = 1 with a tree member: the same model as ffgp_acq_optimize_tree serves; the summation order of the gradient differs, so the
    bound is the trajectory bound, not bit equality"""
    sp = spec("ucb")
    ch = make_chain((40,), 2, ("sum_lin_m52",), 37, seed=500)
    gch = gpu_chain(ch)
    post = gch.members[0]
    assert post.tree is not None
    A = loop_a(ch, ch["X0"], None, sp, STEPS, 0.1)
    B = loop_b(gch, ch["X0"], None, sp, STEPS, 0.1)
    d0 = distance(B, A)
    assert d0 <= 1e-10, "ill-conditioned case: d0 = %.2e" % d0
    bound = max(10.0 * d0, 1e-12)
    X0d = ch["X0"].to(DEV)
    one = post.optimize_acquisition(X0d, steps=STEPS, lr=0.1, acq=sp["acq"], kappa=sp["kappa"], var_add_all=ch["members"][0]["var_add"],
                                    var_floor=sp["var_floor"], fuse_composed=True)
    Fz = fused(gch, X0d, None, sp, STEPS, 0.1)
    assert one[3]["fused"] is True and Fz[3]["fused"] is True
    print("F = 1: d0 %.2e, chain call vs single tree call %.2e" % (d0, distance(Fz, one)))
    assert distance(Fz, one) <= bound and distance(Fz, A) <= bound


# ---- determinism ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,accumulate", [(0, False), (0, True), (1, True)])
def test_state_continues_the_optimiser_bit_for_bit(i, accumulate):
    ch, gch, _, _, _, Fz, lr = traj(i, accumulate)
    sp = CASES[i][5]
    X1, t1, h1, s1 = fused(gch, ch["X0"].to(DEV), ch["level"], sp, 12, lr, accumulate)
    assert s1["fused"] is True and s1["step"] == 12
    X2, t2, h2, s2 = fused(gch, X1, ch["level"], sp, 18, lr, accumulate, state=s1)
    assert s2["fused"] is True and s2["step"] == 30
    assert torch.equal(X2, Fz[0])
    assert torch.equal(torch.cat([t1, t2]), Fz[1])
    assert torch.equal(torch.cat([h1[:-1], h2]), Fz[2])
    if accumulate:
        assert bool(s2["grad_sum"].ne(0).any())


def test_state_moves_to_and_from_the_radial_chain_entry():
    """an all-radial chain: 12 steps of one entry, 18 of the other, either way round, against 30 steps of the CPU loop"""
    ch = CH.make_chain((40, 24, 17), 2, 37, seed=400)
    gch = CH.gpu_chain(ch)
    sp, lr = spec("ucb"), 0.1
    A = CH.loop_a(ch, ch["X0"], ch["level"], sp, STEPS, lr)
    B = CH.loop_b(gch, ch["X0"], ch["level"], sp, STEPS, lr)
    d0 = distance(B, A)
    assert d0 <= 1e-10
    bound = max(10.0 * d0, 1e-12)
    # ffgp_acq_optimize_chain, then the new entry
    X1, t1, h1, s1 = CH.fused(gch, ch["X0"].to(DEV), ch["level"], sp, 12, lr)
    assert s1["fused"] is True
    rc, X2, _, t2, h2, _ = raw_call(gch, X1, ch["level"], sp, steps=18, lr=lr, step0=12, state_in=(s1["exp_avg"], s1["exp_avg_sq"]))
    assert rc == 0
    assert distance((X2, torch.cat([t1, t2]), torch.cat([h1[:-1], h2])), A) <= bound
    # the new entry, then ffgp_acq_optimize_chain
    rc, X1, st, t1, h1, _ = raw_call(gch, ch["X0"], ch["level"], sp, steps=12, lr=lr)
    assert rc == 0
    X2, t2, h2, s2 = CH.fused(gch, X1, ch["level"], sp, 18, lr, state={"step": 12, "exp_avg": st[0], "exp_avg_sq": st[1]})
    assert s2["fused"] is True and s2["step"] == 30
    assert distance((X2, torch.cat([t1, t2]), torch.cat([h1[:-1], h2])), A) <= bound


def test_a_point_does_not_depend_on_its_tile_neighbours_or_their_levels():
    ch, gch, _, _, _, Fz, lr = traj(0, False)
    sp, X0, lv = CASES[0][5], ch["X0"].to(DEV), ch["level"]
    # alone
    for q in (0, 20, 36):
        r = fused(gch, X0[q:q + 1].contiguous(), lv[q:q + 1], sp, STEPS, lr)
        assert torch.equal(r[1][:, 0], Fz[1][:, q]) and torch.equal(r[2][:, 0], Fz[2][:, q])
    # in another tile and column, beside other neighbours: the points in reverse order
    idx = torch.arange(X0.shape[0] - 1, -1, -1)
    r = fused(gch, X0[idx.to(DEV)].contiguous(), lv[idx], sp, STEPS, lr)
    assert torch.equal(r[1], Fz[1][:, idx.to(DEV)]) and torch.equal(r[2], Fz[2][:, idx.to(DEV)])
    # beside points of their own level only: the tiles then stop after that member and run the chains of that member alone
    for k in range(ch["F"]):
        sel = torch.nonzero(lv == k).reshape(-1)
        r = fused(gch, X0[sel.to(DEV)].contiguous(), lv[sel], sp, STEPS, lr)
        assert torch.equal(r[1], Fz[1][:, sel.to(DEV)]) and torch.equal(r[2], Fz[2][:, sel.to(DEV)])
    # beside a switched-off neighbour (C only)
    lo = lv.clone()
    lo[3] = -1
    r = raw_as_result(gch, ch["X0"], lo, sp, STEPS, lr)
    others = [q for q in range(X0.shape[0]) if q != 3]
    assert torch.equal(r[1][:, others], Fz[1][:, others]) and torch.equal(r[2][:, others], Fz[2][:, others])
    assert bool((r[1][:, 3] == 0.0).all()) and torch.equal(r[0][3].cpu(), ch["X0"][3])


@pytest.mark.parametrize("accumulate", [False, True])
def test_a_level_for_all_points_is_the_cut_chain(accumulate):
    ch, gch = case(2)
    sp, X0 = CASES[2][5], ch["X0"]
    lr = 0.01 if accumulate else 0.1
    from fidelityfusion_amd import functional as F
    top = raw_as_result(gch, X0, None, sp, STEPS, lr, accumulate)
    for k in range(ch["F"]):
        # the same Posterior objects: a member factored again has its alpha solved on other inverted diagonal blocks (see predict_diff)
        cut_chain = F.PosteriorChain(gch.members[:k + 1])
        cut_chain.test_var_adds = gch.test_var_adds[:k + 1]
        # the cut chain through the C entry itself: `optimize_acquisition` hands the all-radial cut after member 0 to ffgp_acq_optimize_chain
        cut = raw_as_result(cut_chain, X0, None, sp, STEPS, lr, accumulate)
        lev = raw_as_result(gch, X0, torch.full((X0.shape[0],), k), sp, STEPS, lr, accumulate)
        assert torch.equal(cut[0], lev[0]) and torch.equal(cut[1], lev[1]) and torch.equal(cut[2], lev[2])
        if k < ch["F"] - 1:
            assert not torch.equal(cut[1], top[1])      # the members above k do change the result


def test_a_linear_leaf_blind_to_the_mean_gives_the_chain_no_self_term():
    """the top member's linear leaf with weight 0 on the mean coordinate: k(z, z) does not depend on u, the self term's share of gu is
    gv times an exact 0, and the leaf's centre on that coordinate is multiplied by 0 wherever it is read -- two chains that differ in
    that centre alone are the same bit for bit.  With a weight on the coordinate the centre does count."""
    D, sp = 2, spec("ucb_var", kappa=0.4)

    def build(w_mean, c_mean):
        def edit(leaves):
            leaves[0]["w"][D] = w_mean
            leaves[0]["center"][D] = c_mean
        ch = make_chain((24, 20), D, ("SE", "sum_linc_m32"), 19, seed=620, edits={1: edit})
        assert ch["members"][1]["leaves"][0]["kfun"] == LINEAR
        return ch, gpu_chain(ch)

    (ch, g0), (_, g1) = build(0.0, 0.3), build(0.0, 5.0)
    r0, r1 = raw_as_result(g0, ch["X0"], ch["level"], sp, 8, 0.1), raw_as_result(g1, ch["X0"], ch["level"], sp, 8, 0.1)
    assert all(torch.equal(x, y) for x, y in zip(r0, r1))
    e0, e1 = raw_call(g0, ch["X0"], ch["level"], sp), raw_call(g1, ch["X0"], ch["level"], sp)
    assert torch.equal(e0[5], e1[5])
    a, g = cpu_eval(ch, ch["X0"], ch["level"], sp)
    assert rel(e0[3][0], a) <= 1e-10 and rel(e0[5], g) <= 1e-8
    (_, g2), (_, g3) = build(0.5, 0.3), build(0.5, 5.0)
    assert not torch.equal(raw_call(g2, ch["X0"], ch["level"], sp)[5], raw_call(g3, ch["X0"], ch["level"], sp)[5])


# ---- the fixture of the reference's loop ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    from fidelityfusion_amd import functional as F, kernel
    from fidelityfusion_amd.cigp_v10 import cigp
    z = np.load(os.path.join(ROOT, "tests", "golden", "mf_acq_nar_sum.npz"))
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
def test_fused_call_reproduces_the_reference_fixture_at_every_level(tag):
    z, _, _, gch = fixture()
    assert float(z["twin_distance"]) <= 1e-11
    assert all(p.tree is not None and [int(d["kfun"]) for d in p.tree[0]] == [LINEAR, M52] for p in gch.members)
    assert float(z["lin_center_1"][2]) != 0.0      # the middle member's linear leaf is centred on the mean coordinate too
    steps, lr, acc = int(z["steps"]), float(z["lr"]), tag == "acc"
    sp = spec("ucb_var", kappa=float(z["kappa"]))
    X0 = torch.tensor(z["X0"])                           # [3, 6, 2]: six starts per level
    level = torch.arange(3).repeat_interleave(6)
    Fz = fused(gch, X0.reshape(18, 2).to(DEV), level, sp, steps, lr, acc)      # every level from one call
    assert Fz[3]["fused"] is True
    for s in range(3):
        ref = (None, torch.tensor(z["trace_" + tag][s]), torch.tensor(z["hist_" + tag][s]))
        B = loop_b(gch, X0[s], torch.full((6,), s), sp, steps, lr, acc)
        d0 = distance(B, ref)
        assert d0 <= 1e-10, "ill-conditioned case: d0 = %.2e" % d0
        bound = max(10.0 * d0, 1e-12)
        got = (None, Fz[1][:, 6 * s:6 * s + 6], Fz[2][:, 6 * s:6 * s + 6])
        print("fixture %s level %d: d0 %.2e, bound %.2e, fused vs fixture %.2e, vs B %.2e" % (tag, s, d0, bound, distance(got, ref), distance(got, B)))
        assert distance(got, ref) <= bound and distance(got, B) <= bound
        assert rel(Fz[0][6 * s:6 * s + 6], ref[2][-1]) <= bound      # the final points


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
        kw = dict(level=s, steps=steps, lr=lr, acq="ucb_var", kappa=float(z["kappa"]), fuse_composed=True)
        best = acq.optimize_acqf_nar(models, data, X0.to(DEV), **kw)
        final = acq.optimize_acqf_nar(models, data, X0.to(DEV), return_best_only=False, **kw)
        Fz = fused(gch, X0.to(DEV), torch.full((6,), s), sp, steps, lr)
        assert Fz[3]["fused"] is True and torch.equal(final, Fz[0])      # optimize_acqf_nar took the fused call
        scale = float(ref_h.abs().max())
        e_best, e_final = float((best.cpu() - best_ref).abs().max()) / scale, float((final.cpu() - ref_h[-1]).abs().max()) / scale
        print("optimize_acqf_nar level %d: selected step %d, d0 %.2e, best_x %.2e, final %.2e" % (s, k_ref, d0, e_best, e_final))
        assert k_ref >= 0
        assert e_best <= bound and e_final <= bound, (e_best, e_final, bound)


# ---- routing ---------------------------------------------------------------------------------------------------------------------------
def _fallback_equals_loop_b(gch, X0, level, sp, accumulate=False, steps=6, **kw):
    keep = X0.clone()
    r = fused(gch, X0, level, sp, steps, 0.1, accumulate, **kw)
    assert r[3]["fused"] is False and ("grad_sum" in r[3]) == accumulate
    assert torch.equal(X0, keep)
    B = loop_b(gch, X0, level, sp, steps, 0.1, accumulate)
    for got, want in zip(r[:3], B):
        assert got.device == X0.device
        assert rel(got, want) <= 1e-12
    return r


def test_the_default_is_untouched_and_the_keyword_opts_in():
    ch = make_chain((40, 24), 2, ("sum_lin_m52", "sum_linc_m32"), 19, seed=601)
    gch = gpu_chain(ch)
    X0 = ch["X0"].to(DEV)
    assert gch.acq_tree_fusable(X0) and not gch.acq_fusable(X0)
    _fallback_equals_loop_b(gch, X0, ch["level"], spec("ucb"), fuse_composed=False)
    _fallback_equals_loop_b(gch, X0, ch["level"], spec("ucb_var", kappa=0.4), accumulate=True, fuse_composed=False)
    assert gch.optimize_acquisition(X0, steps=6, var_adds=gch.test_var_adds)[3]["fused"] is False      # the default
    r = fused(gch, X0, ch["level"], spec("ucb"), 6, 0.1)
    assert r[3]["fused"] is True and "staged" not in r[3]
    B = loop_b(gch, X0, ch["level"], spec("ucb"), 6, 0.1)
    assert distance(r, B) <= 1e-10


def test_the_keyword_changes_nothing_on_an_all_radial_chain():
    ch = CH.make_chain((40, 24, 17), 2, 37, seed=400)
    gch = CH.gpu_chain(ch)
    X0 = ch["X0"].to(DEV)
    assert gch.acq_fusable(X0) and gch.acq_tree_fusable(X0)
    for acc in (False, True):
        a = fused(gch, X0, ch["level"], spec("ucb"), 12, 0.1, acc, fuse_composed=False)
        b = fused(gch, X0, ch["level"], spec("ucb"), 12, 0.1, acc, fuse_composed=True)
        assert a[3]["fused"] is True and b[3]["fused"] is True
        assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
        assert torch.equal(a[3]["exp_avg"], b[3]["exp_avg"]) and torch.equal(a[3]["exp_avg_sq"], b[3]["exp_avg_sq"])


@pytest.mark.parametrize("what", ["n", "D", "F"])
def test_fallback_outside_the_limits(what):
    """n = 257, D + 1 = 17, F = 9 -- with `staged=True` as well, which serves radial chains only: the per-step loop"""
    sp = spec("ucb")
    if what == "F":
        ch = okc = make_chain((12,) * 9, 2, ("sum_lin_m52", "SE") * 4 + ("sum_lin_m52",), 19, seed=603)
        gch, ok, ok_level = gpu_chain(ch), gpu_chain(ch, upto=8), None
        assert gch.F == 9
    elif what == "D":
        ch = make_chain((40, 24), 16, ("M32", "sum_lin_m52"), 19, seed=604)
        okc = make_chain((40, 24), 15, ("M32", "sum_lin_m52"), 19, seed=604)
        gch, ok, ok_level = gpu_chain(ch), gpu_chain(okc), okc["level"]
    else:
        ch = make_chain((40, 257), 2, ("M32", "sum_lin_m52"), 19, seed=602)
        okc = make_chain((40, 256), 2, ("M32", "sum_lin_m52"), 19, seed=602)
        gch, ok, ok_level = gpu_chain(ch), gpu_chain(okc), okc["level"]
    X0 = ch["X0"].to(DEV)
    assert not gch.acq_tree_fusable(X0)
    _fallback_equals_loop_b(gch, X0, ch["level"], sp)
    r = _fallback_equals_loop_b(gch, X0, ch["level"], sp, staged=True)
    assert "staged" not in r[3]
    X0ok = okc["X0"].to(DEV)
    assert ok.acq_tree_fusable(X0ok) and fused(ok, X0ok, ok_level, sp, 6, 0.1)[3]["fused"] is True


def test_a_non_library_leaf_is_never_routed_to_the_fused_call():
    """a `Posterior` cannot be built on a leaf the library does not evaluate, so the predicate is what there is to check (as for the
    single posterior, test_gpu_acq_tree.py); the chain then runs loop B"""
    ch = make_chain((30, 20), 2, ("SE", "sum_lin_m52"), 9, seed=621)
    gch = gpu_chain(ch)
    X0 = ch["X0"].to(DEV)
    assert gch.acq_tree_fusable(X0)
    gch.members[1].tree[0][1]["kfun"] = 6
    assert not gch.acq_tree_fusable(X0)
    gch.members[1].tree[0][1]["kfun"] = M52
    assert gch.acq_tree_fusable(X0)
    _fallback_equals_loop_b(gch, X0.cpu(), ch["level"], spec("ucb"))      # start points off the GPU: the per-step loop as well


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
# member 0: balanced4 (four leaves), member 1: one radial kernel, member 2: sum_lin_m52
REFUSALS = [dict(null=("h",)), dict(null=("s",)), dict(null=("X",)), dict(null=("trace",)), dict(null=("opt",)), dict(null=("state",)),
            dict(null=("members",)), dict(null=("trees",)), dict(F=0), dict(F=9), dict(F=-1),
            dict(X_dev=None), dict(L_dev=None), dict(alpha_dev=None), dict(member=2, X_dev=None),
            dict(member=1, w_dev=None), dict(member=1, amp_dev=None), dict(member=1, kfun=LINEAR), dict(member=1, kfun=6), dict(member=1, kfun=-1),
            dict(tree_null=0), dict(tree_null=2),      # a tree member without its tree is a radial member without w_dev / amp_dev
            dict(n=0), dict(n=257), dict(member=1, n=257), dict(D=0), dict(D=16), dict(D=17), dict(D=3), dict(member=1, D=2), dict(member=2, D=4),
            dict(d=2), dict(member=2, d=2), dict(ldl=39), dict(member=1, ldl=1 << 31),
            dict(mean_coef=0.8), dict(member=1, var_coef=0.5), dict(member=2, mean_coef=-1.0),
            dict(tree=(0, dict(leaf_null=True))), dict(tree=(0, dict(n_leaves=1))), dict(tree=(0, dict(n_leaves=5))), dict(tree=(2, dict(n_leaves=0))),
            dict(tree=(0, dict(shape=2))), dict(tree=(0, dict(shape=-1))), dict(tree=(0, dict(op=(0, 2)))), dict(tree=(0, dict(op=(2, -1)))),
            dict(tree=(2, dict(op=(0, 7)))), dict(tree=(0, dict(leaf=(1, "kfun", 6)))), dict(tree=(0, dict(leaf=(3, "kfun", -1)))),
            dict(tree=(0, dict(leaf=(0, "w_dev", None)))), dict(tree=(0, dict(leaf=(2, "amp_dev", None)))), dict(tree=(2, dict(leaf=(1, "w_dev", None)))),
            dict(acq=3), dict(acq=-1), dict(steps=-1), dict(steps=4097), dict(Q=0), dict(Q=-3), dict(step0=-1)]


@pytest.fixture(scope="module")
def abi_chain():
    ch = make_chain((40, 24, 17), 2, ("balanced4", "M32", "sum_lin_m52"), 21, seed=701)
    return ch, gpu_chain(ch)


@pytest.mark.parametrize("bad", REFUSALS, ids=lambda b: ",".join("%s=%s" % kv for kv in b.items()))
def test_c_abi_refuses_before_anything_is_enqueued(abi_chain, bad):
    from fidelityfusion_amd import _lib
    ch, gch = abi_chain
    kw = dict(bad)
    kw.setdefault("steps", 4)
    rc, X, state, trace, hist, grad = raw_call(gch, ch["X0"], ch["level"], spec("ucb"), accumulate=1, **kw)
    assert rc == _lib.FFGP_ERR_ARG
    assert torch.equal(X.cpu(), ch["X0"]) and not bool(state.any()) and bool((trace == -7.0).all())
    assert bool((hist == -7.0).all()) and bool((grad == -7.0).all())


@pytest.mark.parametrize("accumulate", [0, 1])
def test_c_abi_accepted_call_runs(abi_chain, accumulate):
    ch, gch = abi_chain
    sp = spec("ucb")
    tab = gch._member_table(gch.test_var_adds, [])
    assert not tab[0].w_dev and not tab[0].amp_dev and tab[1].w_dev      # a tree member carries no kernel of its own
    # ... and whatever stands in those fields is not read: an unmodified copy of the tree, a kfun no radial member may have
    rc, X, state, trace, hist, grad = raw_call(gch, ch["X0"], ch["level"], sp, steps=4, lr=0.01, accumulate=accumulate, member=0, w_dev=None,
                                               amp_dev=None, kfun=99, tree=(0, {}))
    assert rc == 0
    A = loop_a(ch, ch["X0"], ch["level"], sp, 4, 0.01, bool(accumulate))
    assert rel(trace, A[1]) <= 1e-10 and rel(hist, A[2]) <= 1e-10 and torch.equal(X, hist[-1])
    assert bool(state[1].gt(0).any()) and bool(state[2].ne(0).any()) == bool(accumulate)
    # the gradient output is that of the LAST evaluation alone: the points before the fourth step
    _, g = cpu_eval(ch, A[2][3], ch["level"], sp)
    assert rel(grad, g) <= 1e-8
