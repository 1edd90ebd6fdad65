"""The acquisition optimiser's Adam loop on a STACK of frozen posteriors whose members may carry COMPOSED kernels, in one launch
(ffgp_acq_optimize_stack_tree, csrc/acq_stack_tree.hip; PosteriorStack.optimize_acquisition(..., fuse_composed=True);
acq.optimize_acqf_mf(..., fuse_composed=True)) against plain fp64 torch on the CPU: test_gpu_acq_tree.py's restatement of the
reference's kernel formulas under test_gpu_acq_stack.py's combination of the members (mean = sum_f c_f mean_f, var = sum_f c'_f var_f
up to `to_fidelity`), and against the fixture of the reference's own loop on AR with SumKernel(LinearKernel, MaternKernel) per fidelity.

Bars and method are those two files', whose helpers are imported as they stand.  Evaluate mode (steps = 0): values rel. 1e-10,
gradients rel. 1e-8.  Trajectories: (A) the CPU loop and (B) the per-step loop on the GPU (the members' `predict_diff` + torch.optim.Adam,
what `fuse_composed=False` runs) do not contain the new kernel; d0 = their distance is the yardstick and max(10 d0, 1e-12) the bound; a
case with d0 > 1e-10 is ill-conditioned and fails rather than widening anything.  Before anything is compared, a CPU twin started at
X0 (1 + 2e-16) must stay within 1e-11.  Fall-backs against loop B: 1e-12.  The fixture tests/golden/mf_acq_ar_sum.npz
(gen_mf_acq_ar_sum_goldens.py) is held to the rule applied to mf_acq_ar.npz: d0 = distance(loop B, fixture) <= 1e-10, bound
max(10 d0, 1e-12).

Member recipe: seed g; X = 2 rand(n, D), y = sin(2 sum X) + 0.1 randn; the leaves from test_gpu_acq_tree.TREES[name](g, D), or for a
radial member ONE leaf: amp 1.3, w = 0.6 + rand(D), SE or Matern-3/2 (kparam 1.3, clamp 1e-30); Sigma = K + (0.05 + 1e-6) I, var_add
0.05.  Member f of a stack with seed s uses seed 100 s + f; X0 = 2 rand(Q, D) from seed s; level = (arange(Q) 7 + 2) % F."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_acq_stack as S      # noqa: E402
import test_gpu_acq_tree as T       # noqa: E402
from test_gpu_acq_stack import ACQ_CODE, DEV, LINEAR, M32, M52, NEG_INF, SE, acq_torch, distance, rel, run_loop, select, spec      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 30
RADIAL = {"SE": SE, "M32": M32}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(torch.float32)


# ---- the comparator: plain torch on the CPU ---------------------------------------------------------------------------------------
def make_member(n, D, kind, seed, noise=0.05):
    """one member: `kind` names a tree of test_gpu_acq_tree.TREES or a radial profile (RADIAL)"""
    g = torch.Generator().manual_seed(seed)
    X = 2.0 * torch.rand(n, D, generator=g)
    y = torch.sin(2.0 * X.sum(1)) + 0.1 * torch.randn(n, generator=g)
    c = {"X": X, "Y": y.reshape(n, 1), "dadd": noise + 1e-6, "var_add": noise, "kind": kind, "radial": kind in RADIAL}
    if c["radial"]:
        kfun = RADIAL[kind]
        c.update(w=0.6 + torch.rand(D, generator=g), amp=1.3, kfun=kfun, kparam=1.3 if kfun == M32 else 1.0,
                 clamp=1e-30 if kfun == M32 else NEG_INF)
        c["leaves"] = [{"kfun": kfun, "amp": c["amp"], "kparam": c["kparam"], "center": None, "clamp": c["clamp"], "w": c["w"]}]
    else:
        c["leaves"], c["shape"], c["ops"] = T.TREES[kind](g, D)
    S_ = kval(c, X, X) + c["dadd"] * torch.eye(n)
    c["L"] = torch.linalg.cholesky(S_)
    c["alpha"] = torch.cholesky_solve(c["Y"], c["L"])
    return c


def kval(c, A, B):
    return T.leaf_value(A, B, c["leaves"][0]) if c["radial"] else T.tree_value(A, B, c)


def make_stack(ns, D, kinds, coefs, Q, seed, var_coefs=None):
    g = torch.Generator().manual_seed(seed)
    members = [make_member(n, D, kinds[f], 100 * seed + f) for f, n in enumerate(ns)]
    F = len(ns)
    return {"members": members, "coefs": list(coefs), "var_coefs": list(var_coefs) if var_coefs else [c * c for c in coefs], "F": F, "D": D,
            "X0": 2.0 * torch.rand(Q, D, generator=g), "level": (torch.arange(Q) * 7 + 2) % F}      # levels mixed inside every tile


def cpu_member(c, Xq):
    Ks = kval(c, c["X"], Xq)
    V = torch.linalg.solve_triangular(c["L"], Ks, upper=False)
    kss = c["amp"] if c["radial"] else kval(c, Xq, Xq).diagonal()      # phi(0) = 1 for every radial profile
    return Ks.T @ c["alpha"], kss - (V * V).sum(0) + c["var_add"]


def cpu_predict(st, Xq, level):
    mean, var = torch.zeros(Xq.shape[0], 1), torch.zeros(Xq.shape[0])
    for f, c in enumerate(st["members"]):
        on = torch.ones(Xq.shape[0]) if level is None else (level >= f).double()
        m, v = cpu_member(c, Xq)
        mean = mean + st["coefs"][f] * on.unsqueeze(1) * m
        var = var + st["var_coefs"][f] * on * v
    return mean, var


def cpu_eval(st, Xq, level, sp):
    X = Xq.clone().requires_grad_(True)
    mean, var = cpu_predict(st, X, level)
    a = acq_torch(mean, var, sp)
    (-a.sum()).backward()
    return a.detach().sum(1), X.grad, var.detach()


def loop_a(st, X0, level, sp, steps, lr, accumulate=False):
    return run_loop(lambda X: cpu_predict(st, X, level), X0.cpu(), sp, steps, lr, accumulate)


# ---- the GPU side --------------------------------------------------------------------------------------------------------------------
def gpu_posterior(c):
    return S.gpu_posterior(c) if c["radial"] else T.gpu_posterior(c)


def gpu_stack(st, upto=None):
    from fidelityfusion_amd import functional as F
    k = st["F"] if upto is None else upto
    gst = F.PosteriorStack([gpu_posterior(c) for c in st["members"][:k]], st["coefs"][:k], st["var_coefs"][:k])
    gst.test_var_adds = [c["var_add"] for c in st["members"][:k]]
    return gst


loop_b = S.loop_b      # the per-step loop on the GPU: every member's Posterior.predict_diff, combined there, + torch.optim.Adam


def fused(gst, X0, level, sp, steps, lr, accumulate=False, state=None, fuse_composed=True):
    return gst.optimize_acquisition(X0, steps=steps, lr=lr, acq=sp["acq"], kappa=sp["kappa"], xi=sp["xi"], f_best=sp["f_best"],
                                    var_floor=sp["var_floor"], level=None if level is None else level.to(DEV), var_adds=gst.test_var_adds,
                                    accumulate_grad=accumulate, state=state, fuse_composed=fuse_composed)


def raw_call(gst, Xq, level, sp, steps=0, lr=0.1, step0=0, Q=None, null=(), F=None, accumulate=0, acq=None, member=0, tree=None,
             tree_null=None, **over):
    """ffgp_acq_optimize_stack_tree through ctypes on the stack's own buffers; `over` overrides fields of member `member`, `tree` =
    (member, keyword arguments of test_gpu_acq_tree._tree_copy) replaces that member's tree by a modified copy, `tree_null` names a
    member whose tree pointer is passed as NULL, `null` names pointers to pass as NULL.  Returns (status, X, state, trace, hist, grad)
    -- every buffer pre-filled with a sentinel."""
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
    rc = _lib.lib.ffgp_acq_optimize_stack_tree(None if "h" in null else gst.members[0]._h(), None if "s" in null else C.byref(s),
                                               None if "trees" in null else trees, ptr("X", X), Qn if Q is None else Q, steps,
                                               None if "opt" in null else C.byref(opt), ptr("state", state), step0, ptr("trace", trace),
                                               ptr("hist", hist), ptr("grad", grad))
    torch.cuda.synchronize()
    return rc, X, state, trace, hist, grad


# ---- values and gradients (steps = 0) against CPU autograd ----------------------------------------------------------------------------
#          ns              D   members                                    coefs              Q
EVAL = [((17, 130, 24), 3, ("balanced4", "sum_lin_m52", "M32"), (1.0, -0.7, 1.1), 20),      # a member shrinks and grows, the leaf count
                                                                                             # shrinks: the stale-row and stale-leaf case
        ((24, 40, 17), 2, ("prod_ard_linc", "SE", "chain4"), (1.0, 0.8, -1.3), 20),          # a radial member right after a centred linear
                                                                                             # leaf: stale centre / self value
        ((1, 16), 2, ("sum_lin_m52", "M32"), (1.0, 0.8), 20),
        ((256, 200), 16, ("chain4", "balanced4"), (1.0, 0.8), 16)]                           # the LDS maximum


@functools.lru_cache(maxsize=None)
def eval_stack(i):
    ns, D, kinds, coefs, Q = EVAL[i]
    st = make_stack(ns, D, kinds, coefs, Q, seed=300 + i)
    return st, gpu_stack(st)


@pytest.mark.parametrize("acq", ["ucb", "ei", "ucb_var"])
@pytest.mark.parametrize("i", range(len(EVAL)))
def test_evaluate_matches_cpu_autograd(i, acq):
    st, gst = eval_stack(i)
    sp = spec(acq, f_best=0.3, kappa=2.0 if acq != "ucb_var" else 0.4)
    rc, X, _, trace, _, grad = raw_call(gst, st["X0"], st["level"], sp)
    assert rc == 0
    assert torch.equal(X.cpu(), st["X0"])      # evaluate mode: nothing moves
    a, g, _ = cpu_eval(st, st["X0"], st["level"], sp)
    ev, eg = rel(trace[0], a), rel(grad, g)
    print("stack %s %s D=%d %s: value rel %.2e, gradient rel %.2e" % (EVAL[i][0], EVAL[i][2], EVAL[i][1], acq, ev, eg))
    assert ev <= 1e-10, ev
    assert eg <= 1e-8, eg


def test_evaluate_without_levels_and_with_given_variance_coefficients():
    st = make_stack((40, 24, 17), 2, ("sum_lin_m52", "M32", "prod_ard_linc"), (1.0, 0.8, -1.3), 20, seed=311, var_coefs=(1.0, 0.5, 2.0))
    gst = gpu_stack(st)
    sp = spec("ucb")
    rc, _, _, trace, _, grad = raw_call(gst, st["X0"], None, sp)
    assert rc == 0
    a, g, _ = cpu_eval(st, st["X0"], None, sp)
    assert rel(trace[0], a) <= 1e-10 and rel(grad, g) <= 1e-8
    # predict_diff, the per-step loop's query, is the same combination
    m, v = gst.predict_diff(st["X0"].to(DEV), level=st["level"], var_adds=gst.test_var_adds)
    mc, vc = cpu_predict(st, st["X0"], st["level"])
    assert rel(m, mc) <= 1e-10 and rel(v, vc) <= 1e-10


def floor_case():
    st = make_stack((40, 24), 3, ("sum_lin_m52", "prod_ard_linc"), (1.0, 0.8), 37, seed=312)
    Xq = st["X0"].clone()
    Xq[18:] = 3.0 + 2.0 * Xq[18:]      # half of the points outside the data's box: their variance is above the floor
    return st, Xq, spec("ucb", var_floor=0.5)


def test_evaluate_with_points_on_and_off_the_variance_floor():
    st, Xq, sp = floor_case()
    gst = gpu_stack(st)
    rc, _, _, trace, _, grad = raw_call(gst, Xq, st["level"], sp)
    assert rc == 0
    a, g, var = cpu_eval(st, Xq, st["level"], sp)
    below = var < 0.5
    assert bool(below.any()) and bool((~below).any()), var      # both kinds occur
    assert rel(trace[0], a) <= 1e-10 and rel(grad, g) <= 1e-8
    assert bool((grad.cpu()[below] != 0).any())                 # the mean's gradient still flows below the floor


# ---- trajectories ------------------------------------------------------------------------------------------------------------------
#          ns                  D   members                                          coefs                   Q   acquisition
STACKS = [((40, 24, 17), 2, ("sum_lin_m52", "prod_ard_linc", "se_m32_rq"), (1.0, 0.8, -1.3), 37, spec("ucb")),
          ((33, 16), 1, ("sum_lin_m52", "sum_lin_m52"), (1.0, 1.2), 20, spec("ei", f_best=0.3)),
          ((64, 48, 31, 20), 5, ("SE", "chain4", "M32", "balanced4"), (1.0, 0.8, 1.2, 0.9), 37, spec("ucb_var", kappa=0.4)),
          ((130, 100), 16, ("se_m32_rq", "prod_ard_linc"), (1.0, 0.8), 20, spec("ucb"))]
TRAJ = [(i, acc) for i in range(len(STACKS)) for acc in (False, True)]


@functools.lru_cache(maxsize=None)
def traj_cpu(i, accumulate):
    """case i on the CPU: the stack, loop A and its twin"""
    ns, D, kinds, coefs, Q, sp = STACKS[i]
    lr = 0.01 if accumulate else 0.1
    st = make_stack(ns, D, kinds, coefs, Q, seed=400 + i)
    A = loop_a(st, st["X0"], st["level"], sp, STEPS, lr, accumulate)
    twin = loop_a(st, st["X0"] * (1.0 + 2e-16), st["level"], sp, STEPS, lr, accumulate)
    return st, A, twin, lr


@functools.lru_cache(maxsize=None)
def traj_stack(i):
    return gpu_stack(traj_cpu(i, False)[0])


@functools.lru_cache(maxsize=None)
def traj(i, accumulate):
    """case i once: the CPU loop, its twin, loop B, the fused call -- shared by the tests below and left unchanged"""
    st, A, twin, lr = traj_cpu(i, accumulate)
    sp = STACKS[i][5]
    gst = traj_stack(i)
    B = loop_b(gst, st["X0"], st["level"], sp, STEPS, lr, accumulate)
    X0d = st["X0"].to(DEV)
    keep = X0d.clone()
    Fz = fused(gst, X0d, st["level"], sp, STEPS, lr, accumulate)
    assert torch.equal(X0d, keep)      # X0 is left untouched
    return st, gst, A, twin, B, Fz, lr


@pytest.mark.parametrize("i,accumulate", TRAJ)
def test_trajectory_follows_both_references(i, accumulate):
    st, gst, A, twin, B, Fz, lr = traj(i, accumulate)
    dt_x, dt_t = rel(twin[2], A[2]), rel(twin[1], A[1])
    assert dt_x <= 1e-11 and dt_t <= 1e-11, (dt_x, dt_t)      # conditioning of the case, before anything is compared
    d0 = distance(B, A)
    assert d0 <= 1e-10, "ill-conditioned case: d0 = %.2e" % d0
    bound = max(10.0 * d0, 1e-12)
    dA, dB = distance(Fz, A), distance(Fz, B)
    print("stack %d accumulate=%s: twin %.2e / %.2e, d0 %.2e, bound %.2e, fused vs A %.2e, vs B %.2e" % (i, accumulate, dt_x, dt_t, d0, bound, dA, dB))
    Q, D = st["X0"].shape
    assert Fz[3]["fused"] is True and Fz[3]["step"] == STEPS and ("grad_sum" in Fz[3]) == accumulate
    assert Fz[1].shape == (STEPS, Q) and Fz[2].shape == (STEPS + 1, Q, D)
    assert torch.equal(Fz[0], Fz[2][-1]) and torch.equal(Fz[2][0].cpu(), st["X0"])
    assert dA <= bound, (dA, bound)
    assert dB <= bound, (dB, bound)


@pytest.mark.parametrize("i", [0, 3])
def test_one_tree_member_with_coefficient_one_is_the_single_posterior_call(i):
    """F = 1 with a tree member, mean_coef = var_coef = 1: the same model as ffgp_acq_optimize_tree serves; the summation order of the
    gradient differs, so the bound is the trajectory bound, not bit equality"""
    ns, D, kinds, _, Q, sp = STACKS[i]
    st = make_stack(ns[:1], D, kinds[:1], (1.0,), Q, seed=500 + i)
    gst = gpu_stack(st)
    post = gst.members[0]
    assert post.tree is not None
    A = loop_a(st, st["X0"], None, sp, STEPS, 0.1)
    B = loop_b(gst, st["X0"], None, sp, STEPS, 0.1)
    d0 = distance(B, A)
    assert d0 <= 1e-10, "ill-conditioned case: d0 = %.2e" % d0
    bound = max(10.0 * d0, 1e-12)
    X0d = st["X0"].to(DEV)
    one = post.optimize_acquisition(X0d, steps=STEPS, lr=0.1, acq=sp["acq"], kappa=sp["kappa"], var_add_all=st["members"][0]["var_add"],
                                    var_floor=sp["var_floor"], fuse_composed=True)
    Fz = fused(gst, X0d, None, sp, STEPS, 0.1)
    assert one[3]["fused"] is True and Fz[3]["fused"] is True
    print("F = 1, stack %d: d0 %.2e, stack call vs single tree call %.2e" % (i, d0, distance(Fz, one)))
    assert distance(Fz, one) <= bound and distance(Fz, A) <= bound


def test_an_all_radial_stack_through_the_new_entry_follows_the_radial_stack_entry():
    """trees[f] = NULL for every member: the model ffgp_acq_optimize_stack serves, each member run as a one-leaf record; the leaves are
    re-evaluated in the gradient pass where that kernel keeps a derivative image, so the bound is the trajectory bound"""
    st = S.make_stack((40, 24, 17), 2, (1.0, 0.8, -1.3), 37, seed=400)
    gst = S.gpu_stack(st)
    sp = spec("ucb")
    A = S.loop_a(st, st["X0"], st["level"], sp, STEPS, 0.1)
    B = S.loop_b(gst, st["X0"], st["level"], sp, STEPS, 0.1)
    d0 = distance(B, A)
    assert d0 <= 1e-10, "ill-conditioned case: d0 = %.2e" % d0
    bound = max(10.0 * d0, 1e-12)
    rc0, X0_, _, t0, h0, _ = S.raw_call(gst, st["X0"], st["level"], sp, steps=STEPS)
    rc1, X1_, _, t1, h1, _ = raw_call(gst, st["X0"], st["level"], sp, steps=STEPS)
    assert rc0 == 0 and rc1 == 0
    new, old = (X1_, t1, h1), (X0_, t0, h0)
    print("all radial: d0 %.2e, new entry vs stack entry %.2e, vs A %.2e" % (d0, distance(new, old), distance(new, A)))
    assert distance(new, old) <= bound and distance(new, A) <= bound and distance(new, B) <= bound


# ---- determinism ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,accumulate", [(0, False), (0, True), (2, True)])
def test_state_continues_the_optimiser_bit_for_bit(i, accumulate):
    st, gst, _, _, _, Fz, lr = traj(i, accumulate)
    sp = STACKS[i][5]
    X1, t1, h1, s1 = fused(gst, st["X0"].to(DEV), st["level"], sp, 12, lr, accumulate)
    assert s1["fused"] is True and s1["step"] == 12
    X2, t2, h2, s2 = fused(gst, X1, st["level"], sp, 18, lr, accumulate, state=s1)
    assert s2["step"] == 30
    assert torch.equal(X2, Fz[0])
    assert torch.equal(torch.cat([t1, t2]), Fz[1])
    assert torch.equal(torch.cat([h1[:-1], h2]), Fz[2])
    assert torch.equal(s2["exp_avg"], Fz[3]["exp_avg"]) and torch.equal(s2["exp_avg_sq"], Fz[3]["exp_avg_sq"])
    if accumulate:
        assert torch.equal(s2["grad_sum"], Fz[3]["grad_sum"]) and bool(s2["grad_sum"].ne(0).any())


def test_a_point_does_not_depend_on_its_tile_neighbours_or_their_levels():
    st, gst, _, _, _, Fz, lr = traj(0, False)
    sp, X0, lv = STACKS[0][5], st["X0"].to(DEV), st["level"]
    # alone
    for q in (0, 20, 36):
        r = fused(gst, X0[q:q + 1].contiguous(), lv[q:q + 1], sp, STEPS, lr)
        assert torch.equal(r[1][:, 0], Fz[1][:, q]) and torch.equal(r[2][:, 0], Fz[2][:, q])
    # in another tile and column, beside other neighbours: the points in reverse order
    idx = torch.arange(X0.shape[0] - 1, -1, -1)
    r = fused(gst, X0[idx.to(DEV)].contiguous(), lv[idx], sp, STEPS, lr)
    assert torch.equal(r[1], Fz[1][:, idx.to(DEV)]) and torch.equal(r[2], Fz[2][:, idx.to(DEV)])
    # beside points of other levels only: the points of level 0 (their tiles then stop after member 0) and of level 1 on their own
    for k in (0, 1):
        sel = torch.nonzero(lv == k).reshape(-1)
        r = fused(gst, X0[sel.to(DEV)].contiguous(), lv[sel], sp, STEPS, lr)
        assert torch.equal(r[1], Fz[1][:, sel.to(DEV)]) and torch.equal(r[2], Fz[2][:, sel.to(DEV)])


@pytest.mark.parametrize("accumulate", [False, True])
def test_a_level_for_all_points_is_the_truncated_stack(accumulate):
    st, gst, _, _, _, _, lr = traj(2, accumulate)
    sp, X0 = STACKS[2][5], st["X0"].to(DEV)
    from fidelityfusion_amd import functional as F
    for k in range(st["F"]):
        # the same Posterior objects: a member factored again has its alpha solved on other inverted diagonal blocks (see predict_diff)
        cut_stack = F.PosteriorStack(gst.members[:k + 1], gst.mean_coefs[:k + 1], gst.var_coefs[:k + 1])
        cut_stack.test_var_adds = gst.test_var_adds[:k + 1]
        # the cut stack through the C entry itself: `optimize_acquisition` hands the all-radial cut after member 0 to ffgp_acq_optimize_stack
        cut = raw_as_result(cut_stack, X0, None, sp, STEPS, lr, accumulate)
        lev = fused(gst, X0, torch.full((X0.shape[0],), k), sp, STEPS, lr, accumulate)
        assert lev[3]["fused"] is True
        assert torch.equal(cut[0], lev[0]) and torch.equal(cut[1], lev[1]) and torch.equal(cut[2], lev[2])
        if k < st["F"] - 1:
            assert not torch.equal(cut[1], fused(gst, X0, None, sp, STEPS, lr, accumulate)[1])      # the members above k do count


def raw_as_result(gst, X0, level, sp, steps, lr, accumulate):
    """(X, trace, hist) of the C entry on a fresh optimiser"""
    rc, X, _, trace, hist, _ = raw_call(gst, X0, level, sp, steps=steps, lr=lr, accumulate=1 if accumulate else 0)
    assert rc == 0
    return X, trace, hist


# ---- the fixture of the reference's loop ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    from fidelityfusion_amd import functional as F, kernel
    from fidelityfusion_amd.cigp_v10 import cigp
    z = np.load(os.path.join(ROOT, "tests", "golden", "mf_acq_ar_sum.npz"))
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
def test_fused_call_reproduces_the_reference_fixture_at_every_level(tag):
    z, _, _, gst = fixture()
    assert float(z["twin_distance"]) <= 1e-11
    assert all(p.tree is not None and [int(d["kfun"]) for d in p.tree[0]] == [LINEAR, M52] for p in gst.members)
    assert bool(np.any(z["lin_center"] != 0.0))
    steps, lr, acc = int(z["steps"]), float(z["lr"]), tag == "acc"
    sp = spec("ucb_var", kappa=float(z["kappa"]))
    X0 = torch.tensor(z["X0"])                           # [3, 6, 2]: six starts per level
    level = torch.arange(3).repeat_interleave(6)
    Fz = fused(gst, X0.reshape(18, 2).to(DEV), level, sp, steps, lr, acc)      # every level from one call
    assert Fz[3]["fused"] is True
    for s in range(3):
        ref = (None, torch.tensor(z["trace_" + tag][s]), torch.tensor(z["hist_" + tag][s]))
        B = loop_b(gst, X0[s], torch.full((6,), s), sp, steps, lr, acc)
        d0 = distance(B, ref)
        assert d0 <= 1e-10, "ill-conditioned case: d0 = %.2e" % d0
        bound = max(10.0 * d0, 1e-12)
        got = (None, Fz[1][:, 6 * s:6 * s + 6], Fz[2][:, 6 * s:6 * s + 6])
        print("fixture %s level %d: d0 %.2e, bound %.2e, fused vs fixture %.2e, vs B %.2e" % (tag, s, d0, bound, distance(got, ref), distance(got, B)))
        assert distance(got, ref) <= bound and distance(got, B) <= bound
        assert rel(Fz[0][6 * s:6 * s + 6], ref[2][-1]) <= bound      # the final points


def test_optimize_acqf_mf_selects_as_the_reference_rule_does_on_the_fixture():
    from fidelityfusion_amd import acq
    z, models, data, gst = fixture()
    steps, lr = int(z["steps"]), float(z["lr"])
    sp = spec("ucb_var", kappa=float(z["kappa"]))
    rho = [float(r) for r in z["rho"]]
    for s in range(3):
        X0 = torch.tensor(z["X0"][s])
        ref_t, ref_h = torch.tensor(z["trace_zg"][s]), torch.tensor(z["hist_zg"][s])
        k_ref, best_ref = select(X0, ref_t, ref_h)
        B = loop_b(gst, X0, torch.full((6,), s), sp, steps, lr)
        d0 = distance(B, (None, ref_t, ref_h))
        assert d0 <= 1e-10
        bound = max(10.0 * d0, 1e-12)
        kw = dict(rho=rho, level=s, steps=steps, lr=lr, acq="ucb_var", kappa=float(z["kappa"]), fuse_composed=True)
        best = acq.optimize_acqf_mf(models, data, X0.to(DEV), **kw)
        final = acq.optimize_acqf_mf(models, data, X0.to(DEV), return_best_only=False, **kw)
        Fz = fused(gst, X0.to(DEV), torch.full((6,), s), sp, steps, lr)
        assert Fz[3]["fused"] is True and torch.equal(final, Fz[0])      # optimize_acqf_mf took the fused call
        scale = float(ref_h.abs().max())
        e_best, e_final = float((best.cpu() - best_ref).abs().max()) / scale, float((final.cpu() - ref_h[-1]).abs().max()) / scale
        print("optimize_acqf_mf level %d: selected step %d, d0 %.2e, best_x %.2e, final %.2e" % (s, k_ref, d0, e_best, e_final))
        assert k_ref >= 0
        assert e_best <= bound and e_final <= bound, (e_best, e_final, bound)


# ---- routing ---------------------------------------------------------------------------------------------------------------------------
def _fallback_equals_loop_b(gst, X0, level, sp, accumulate=False, steps=6, **kw):
    keep = X0.clone()
    r = fused(gst, X0, level, sp, steps, 0.1, accumulate, **kw)
    assert r[3]["fused"] is False and ("grad_sum" in r[3]) == accumulate
    assert torch.equal(X0, keep)
    B = loop_b(gst, X0, level, sp, steps, 0.1, accumulate)
    for got, want in zip(r[:3], B):
        assert got.device == X0.device
        assert rel(got, want) <= 1e-12
    return r


def test_the_default_is_untouched_and_the_keyword_opts_in():
    st = make_stack((40, 24), 2, ("sum_lin_m52", "M32"), (1.0, 0.8), 19, seed=601)
    gst = gpu_stack(st)
    X0 = st["X0"].to(DEV)
    assert gst.acq_tree_fusable(X0) and not gst.acq_fusable(X0)
    _fallback_equals_loop_b(gst, X0, st["level"], spec("ucb"), fuse_composed=False)
    _fallback_equals_loop_b(gst, X0, st["level"], spec("ucb_var", kappa=0.4), accumulate=True, fuse_composed=False)
    assert gst.optimize_acquisition(X0, steps=6, var_adds=gst.test_var_adds)[3]["fused"] is False      # the default
    r = fused(gst, X0, st["level"], spec("ucb"), 6, 0.1)
    assert r[3]["fused"] is True
    B = loop_b(gst, X0, st["level"], spec("ucb"), 6, 0.1)
    assert distance(r, B) <= 1e-10


def test_the_keyword_changes_nothing_on_an_all_radial_stack():
    st = S.make_stack((40, 24, 17), 2, (1.0, 0.8, -1.3), 37, seed=400)
    gst = S.gpu_stack(st)
    X0 = st["X0"].to(DEV)
    assert gst.acq_fusable(X0) and gst.acq_tree_fusable(X0)
    for acc in (False, True):
        a = fused(gst, X0, st["level"], spec("ucb"), 12, 0.1, acc, fuse_composed=False)
        b = fused(gst, X0, st["level"], spec("ucb"), 12, 0.1, acc, fuse_composed=True)
        assert a[3]["fused"] is True and b[3]["fused"] is True
        assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
        assert torch.equal(a[3]["exp_avg"], b[3]["exp_avg"]) and torch.equal(a[3]["exp_avg_sq"], b[3]["exp_avg_sq"])


@pytest.mark.parametrize("what", ["n", "d", "F"])
def test_fallback_outside_the_limits(what):
    sp = spec("ucb")
    if what == "F":
        st = make_stack((12,) * 9, 2, ("sum_lin_m52", "SE") * 4 + ("sum_lin_m52",), (1.0,) + (0.5,) * 8, 19, seed=603)
        gst = gpu_stack(st)
        assert gst.F == 9
        ok = gpu_stack(st, upto=8)
        ok_level = None
    else:
        st = make_stack((40, 257 if what == "n" else 24), 2, ("M32", "sum_lin_m52"), (1.0, 0.8), 19, seed=602)
        if what == "d":
            c = st["members"][1]
            c["Y"] = torch.cat([c["Y"], torch.cos(3.0 * c["X"].sum(1)).reshape(-1, 1)], 1)
        gst = gpu_stack(st)
        ok = gpu_stack(make_stack((40, 256 if what == "n" else 24), 2, ("M32", "sum_lin_m52"), (1.0, 0.8), 19, seed=602))
        ok_level = st["level"]
    X0 = st["X0"].to(DEV)
    assert not gst.acq_tree_fusable(X0)
    _fallback_equals_loop_b(gst, X0, st["level"], sp)
    assert ok.acq_tree_fusable(X0) and fused(ok, X0, ok_level, sp, 6, 0.1)[3]["fused"] is True


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
# member 0: chain4 (four leaves), member 1: one radial kernel, member 2: sum_lin_m52
REFUSALS = [dict(null=("h",)), dict(null=("s",)), dict(null=("X",)), dict(null=("trace",)), dict(null=("opt",)), dict(null=("state",)),
            dict(null=("members",)), dict(null=("trees",)), dict(F=0), dict(F=9), dict(F=-1),
            dict(X_dev=None), dict(L_dev=None), dict(alpha_dev=None), dict(member=2, X_dev=None),
            dict(member=1, w_dev=None), dict(member=1, amp_dev=None), dict(member=1, kfun=LINEAR), dict(member=1, kfun=6), dict(member=1, kfun=-1),
            dict(tree_null=0), dict(tree_null=2),      # a tree member without its tree is a radial member without w_dev / amp_dev
            dict(n=0), dict(n=257), dict(member=1, n=257), dict(D=0), dict(D=17), dict(member=1, D=3), dict(d=2), dict(member=2, d=2),
            dict(ldl=39), dict(member=1, ldl=1 << 31),
            dict(tree=(0, dict(leaf_null=True))), dict(tree=(0, dict(n_leaves=1))), dict(tree=(0, dict(n_leaves=5))), dict(tree=(2, dict(n_leaves=0))),
            dict(tree=(0, dict(shape=2))), dict(tree=(0, dict(shape=-1))), dict(tree=(0, dict(op=(0, 2)))), dict(tree=(0, dict(op=(2, -1)))),
            dict(tree=(2, dict(op=(0, 7)))), dict(tree=(0, dict(leaf=(1, "kfun", 6)))), dict(tree=(0, dict(leaf=(3, "kfun", -1)))),
            dict(tree=(0, dict(leaf=(0, "w_dev", None)))), dict(tree=(0, dict(leaf=(2, "amp_dev", None)))), dict(tree=(2, dict(leaf=(1, "w_dev", None)))),
            dict(acq=3), dict(acq=-1), dict(steps=-1), dict(steps=4097), dict(Q=0), dict(Q=-3), dict(step0=-1)]


@pytest.fixture(scope="module")
def abi_stack():
    st = make_stack((40, 24, 17), 2, ("chain4", "M32", "sum_lin_m52"), (1.0, 0.8, -1.3), 21, seed=701)
    return st, gpu_stack(st)


@pytest.mark.parametrize("bad", REFUSALS, ids=lambda b: ",".join("%s=%s" % kv for kv in b.items()))
def test_c_abi_refuses_before_anything_is_enqueued(abi_stack, bad):
    from fidelityfusion_amd import _lib
    st, gst = abi_stack
    kw = dict(bad)
    kw.setdefault("steps", 4)
    rc, X, state, trace, hist, grad = raw_call(gst, st["X0"], st["level"], spec("ucb"), accumulate=1, **kw)
    assert rc == _lib.FFGP_ERR_ARG
    assert torch.equal(X.cpu(), st["X0"]) and not bool(state.any()) and bool((trace == -7.0).all())
    assert bool((hist == -7.0).all()) and bool((grad == -7.0).all())


@pytest.mark.parametrize("accumulate", [0, 1])
def test_c_abi_accepted_call_runs(abi_stack, accumulate):
    st, gst = abi_stack
    sp = spec("ucb")
    tab = gst._member_table(gst.test_var_adds, [])
    assert not tab[0].w_dev and not tab[0].amp_dev and tab[1].w_dev      # a tree member carries no kernel of its own
    # ... and whatever stands in those fields is not read: an unmodified copy of the tree, a kfun no radial member may have
    rc, X, state, trace, hist, grad = raw_call(gst, st["X0"], st["level"], sp, steps=4, lr=0.01, accumulate=accumulate, member=0, w_dev=None,
                                               amp_dev=None, kfun=99, tree=(0, {}))
    assert rc == 0
    A = loop_a(st, st["X0"], st["level"], sp, 4, 0.01, bool(accumulate))
    assert rel(trace, A[1]) <= 1e-10 and rel(hist, A[2]) <= 1e-10 and torch.equal(X, hist[-1])
    assert bool(state[1].gt(0).any()) and bool(state[2].ne(0).any()) == bool(accumulate)
    # the gradient output is that of the LAST evaluation alone: the points before the fourth step
    _, g, _ = cpu_eval(st, A[2][3], st["level"], sp)
    assert rel(grad, g) <= 1e-8
