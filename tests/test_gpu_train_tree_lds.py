"""train_many(..., tree_one_launch=True): SumKernel / ProductKernel models of at most 128 points trained by ffgp_train_tree_lds_raw --
ONE launch for all their steps, a persistent workgroup per model (csrc/train_tree_lds.hip) -- against the reference's fixtures, the
per-step loop through the drop-in modules, the launch-per-stage call it replaces, and itself (each model as alone, bit for bit).
Every test asserts through state["tree_one_launch"] that the models it meant to send to the new kernel went there.

The trajectory bound is test_gpu_train_tree.py's: max(10 x d0, floor), d0 = the case's loop yardstick (two per-step loops that differ
only in rounding, kernel.FUSE_PAIRS True / False -- code this route does not touch), measured on an MI355X and written into the case
table; the floor is 1e-12, or, where a case needs more, 10 x the distance on that case's data between ffgp_train_raw's LDS trainer and
its launch-per-stage form (option train_persist 1 / 0) for the tree's first radial leaf alone: what an LDS trainer is known to differ
from its launch-per-stage form by.  A case whose bound would exceed 1e-9 is ill-conditioned and is replaced.  The measured d0, floors
and trainer distances: DESIGN.md section 4.8."""
import copy
import ctypes as C

import numpy as np
import pytest

from test_gpu_train_tree import CASES, DEV, FIXTURES, LM, LR, STEPS1, STEPS2, T, build_kernel, distance, make_models, params_of, reference_loop, rel

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(torch.float32)


def build_kernel2(spec, D, rng):
    """test_gpu_train_tree.build_kernel, and the leaf "lin0": a LinearKernel whose centre starts at the origin"""
    from fidelityfusion_amd import kernel
    if isinstance(spec, tuple):
        cls = kernel.SumKernel if spec[0] == "sum" else kernel.ProductKernel
        return cls(build_kernel2(spec[1], D, rng), build_kernel2(spec[2], D, rng))
    if spec == "lin0":
        k = kernel.LinearKernel(D)
        with torch.no_grad():
            k.length_scales.copy_(torch.tensor(rng.uniform(0.7, 1.6, D)))
        return k
    return build_kernel(spec, D, rng)


def make_models2(members, seed):
    """test_gpu_train_tree.make_models with build_kernel2's leaves"""
    from fidelityfusion_amd.cigp_v10 import cigp
    from oracle import gp_oracle as O
    rng = np.random.default_rng(seed)
    models, xs, ys = [], [], []
    for f, (n, D, d, spec, yvar) in enumerate(members):
        models.append(cigp(build_kernel2(spec, D, rng), 0.7 + 0.1 * f).double().to(DEV))
        if n > 1:
            X, Y = O.synthetic_xy(n, D, d, seed=seed + f)
        else:      # (synthetic_xy normalises by the sample deviation: not defined for one point)
            r1 = np.random.default_rng(seed + f)
            X, Y = r1.random((1, D)), r1.standard_normal((1, d))
        xs.append(T(X))
        ys.append([T(Y), torch.diag(T(rng.uniform(0.01, 0.2, n)))] if yvar else T(Y))
    return models, xs, ys


# name -> (members, d0, floor): d0 = loop_yardstick2 on an MI355X (FUSE_PAIRS True against False through the per-step loop, 25 + 15 steps,
# lr = 1e-2); floor = 1e-12, or 10 x persist_distance where the case needs it (none does)
NEW_CASES = {
    "n1": ([(1, 2, 1, LM, False)], 4.72e-16, 1e-12),                                                               # one point
    "n16": ([(16, 3, 1, ("prod", "ard", "m32"), False)], 4.37e-16, 1e-12),                                         # one block exactly
    "n17": ([(17, 2, 2, LM, False)], 3.14e-16, 1e-12),                                                             # a second, almost empty block
    "n113": ([(113, 3, 1, ("sum", ("prod", "lin", "ard"), "m12"), False)], 1.07e-15, 1e-12),                       # eight blocks, the last ragged
    "D1": ([(40, 1, 1, LM, False)], 6.41e-14, 1e-12),
    "D9": ([(50, 9, 1, ("sum", "lin", "m52"), False)], 8.12e-15, 1e-12),                                           # the padded half of the 16-wide unroll
    "D16": ([(64, 16, 1, ("sum", "lin", "ard"), False)], 4.70e-15, 1e-12),
    "d16": ([(48, 2, 16, LM, False)], 5.37e-15, 1e-12),
    "balanced4_se": ([(70, 2, 3, ("prod", ("sum", "lin", "m52"), ("sum", "se", "ard")), False)], 7.26e-15, 1e-12),      # 4-balanced, broadcast SE
    "chain4_two_lin": ([(60, 3, 1, ("sum", ("sum", ("prod", "lin", "m32"), "ard"), "lin0"), False)], 1.28e-14, 1e-12),  # centres off and at the origin
    "yvar": ([(45, 2, 1, LM, True)], 2.31e-15, 1e-12),                                                             # a [y, y_var] member
}
ALL_CASES = {name: (CASES[name][0], CASES[name][1], 1e-12, make_models) for name in ("sum2_n24", "prod2_n128", "three_small")}
ALL_CASES.update({name: (m, d0, fl, make_models2) for name, (m, d0, fl) in NEW_CASES.items()})


def loop_yardstick2(name):
    """d0 of a case (for re-measuring the table above; the tests do not call it)"""
    from fidelityfusion_amd import kernel
    members, _, _, make = ALL_CASES[name]
    runs = []
    for fuse in (True, False):
        kernel.FUSE_PAIRS = fuse
        try:
            models, xs, ys = make(members, 11)
            runs.append((reference_loop(models, xs, ys, STEPS1 + STEPS2, LR), models))
        finally:
            kernel.FUSE_PAIRS = True
    return distance(runs[1][0], runs[1][1], runs[0][0], runs[0][1])


def persist_distance(name):
    """the floor's measurement: the tree's first radial leaf alone on the case's data, ffgp_train_raw's one-launch trainer against its
    launch-per-stage form (for re-measuring; the tests do not call it)"""
    from fidelityfusion_amd import _lib
    from fidelityfusion_amd.cigp_v10 import cigp, train_many
    members, _, _, make = ALL_CASES[name]

    def first_radial(spec):
        if isinstance(spec, tuple):
            return first_radial(spec[1]) or first_radial(spec[2])
        return None if spec in ("lin", "lin0") else spec
    runs = []
    for persist in (1, 0):
        _, xs, ys = make(members, 11)
        rng = np.random.default_rng(11)
        models = [cigp(build_kernel(first_radial(m[3]), m[1], rng), 0.7).double().to(DEV) for m in members]
        _lib.set_option("train_persist", persist)
        try:
            tr, st = train_many(models, xs, ys, STEPS1, lr=LR)
            tr2, st = train_many(models, xs, ys, STEPS2, lr=LR, state=st)
        finally:
            _lib.set_option("train_persist", 1)
        runs.append((torch.cat([tr, tr2], dim=1), models))
    return distance(runs[1][0], runs[1][1], runs[0][0], runs[0][1])


def bound_of(name):
    _, d0, floor, _ = ALL_CASES[name]
    assert d0 is not None and max(10 * d0, floor) <= 1e-9, "the case has no measured yardstick, or is ill-conditioned"
    return max(10 * d0, floor)


def test_sum_kernel_model_takes_the_one_launch_route():
    """fails before ffgp_train_tree_lds_raw: train_many has no keyword tree_one_launch"""
    from fidelityfusion_amd.cigp_v10 import train_many
    models, xs, ys = make_models([(40, 2, 1, LM, False)], 3)
    before = params_of(models[0])
    trace, state = train_many(models, xs, ys, 5, lr=1e-2, tree_one_launch=True)
    assert state["fused"] is True and state["tree_one_launch"] == [0]
    assert all(p.grad is None for p in models[0].parameters())
    assert trace.shape == (1, 5) and trace.is_cuda and bool(torch.isfinite(trace).all())
    assert float(trace[0, -1]) < float(trace[0, 0])
    assert all(np.abs(a - b).max() > 0 for a, b in zip(params_of(models[0]), before))      # every parameter moved, the centre included
    models, xs, ys = make_models([(40, 2, 1, LM, False)], 3)
    trace2, state2 = train_many(models, xs, ys, 5, lr=1e-2)
    assert state2["fused"] is True and state2["tree_one_launch"] == []


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_one_launch_on_the_reference_fixtures(golden, name):
    """the reference's own fp64 loop (n = 16, 32, 100, 128): loss trace and final parameters within 1e-8, the bound the fixtures are
    held to on the launch-per-stage route"""
    from fidelityfusion_amd.cigp_v10 import cigp, train_many
    g = golden(name)
    D, spec = FIXTURES[name]
    m = cigp(build_kernel(spec, D, np.random.default_rng(0)), 1.0).double().to(DEV)
    with torch.no_grad():
        for i, p in enumerate(m.parameters()):
            p.copy_(T(g["init_%d" % i]).reshape(p.shape))
    trace, state = train_many([m], [T(g["x"])], [T(g["y"])], int(g["steps"]), lr=float(g["lr"]), tree_one_launch=True)
    assert state["fused"] is True and state["tree_one_launch"] == [0]
    errs = {"trace": rel(trace[0], g["trace"])}
    for i, p in enumerate(m.parameters()):
        errs["final_%d" % i] = rel(p, g["final_%d" % i])
    print(name, errs)
    assert max(errs.values()) <= 1e-8, errs


def _follows_the_loop(name):
    from fidelityfusion_amd.cigp_v10 import train_many
    members, d0, floor, make = ALL_CASES[name]
    bound = bound_of(name)
    models, xs, ys = make(members, 11)
    twins = [copy.deepcopy(m) for m in models]
    trace, state = train_many(models, xs, ys, STEPS1, lr=LR, tree_one_launch=True)
    assert state["fused"] is True and state["tree_one_launch"] == list(range(len(members)))
    trace2, state = train_many(models, xs, ys, STEPS2, lr=LR, state=state, tree_one_launch=True)      # the optimisers continue
    assert state["tree_one_launch"] == list(range(len(members)))
    ref = reference_loop(twins, xs, ys, STEPS1 + STEPS2, LR)
    dist = distance(torch.cat([trace, trace2], dim=1), models, ref, twins)
    print("%s: d0 %.3g, one-launch trainer %.3g, bound %.3g" % (name, d0, dist, bound))
    assert dist <= bound, (dist, bound)


@pytest.mark.parametrize("name", sorted(n for n in ALL_CASES if n != "three_small"))
def test_one_launch_follows_the_per_step_loop(name):
    _follows_the_loop(name)


@pytest.mark.noisy
def test_one_launch_follows_the_per_step_loop_beside_the_load():
    """three tree models in ONE launch (n = 24, 60 with y_var, 128), beside the background load"""
    _follows_the_loop("three_small")


@pytest.mark.parametrize("first", [True, False])
def test_state_is_portable_between_the_two_routes(first):
    """25 steps on one route, 15 on the other, ONE state: within the case's bound of the 40-step loop"""
    from fidelityfusion_amd.cigp_v10 import train_many
    name = "three_small"
    members, d0, _, make = ALL_CASES[name]
    bound = bound_of(name)
    models, xs, ys = make(members, 11)
    twins = [copy.deepcopy(m) for m in models]
    trace, state = train_many(models, xs, ys, STEPS1, lr=LR, tree_one_launch=first)
    assert state["tree_one_launch"] == ([0, 1, 2] if first else [])
    trace2, state = train_many(models, xs, ys, STEPS2, lr=LR, state=state, tree_one_launch=not first)
    assert state["tree_one_launch"] == ([] if first else [0, 1, 2])
    assert len(state["chunks"]) == 1 and state["chunks"][(0, 1, 2)].step == STEPS1 + STEPS2
    ref = reference_loop(twins, xs, ys, STEPS1 + STEPS2, LR)
    dist = distance(torch.cat([trace, trace2], dim=1), models, ref, twins)
    print("%s, one launch %s: %.3g, bound %.3g" % (name, "first" if first else "second", dist, bound))
    assert dist <= bound, (dist, bound)


SIXTEEN = [(1, 2, 1, LM, False), (16, 3, 1, ("prod", "ard", "m32"), False), (17, 2, 2, LM, False), (33, 9, 1, ("sum", "lin", "m52"), False),
           (40, 1, 1, LM, False), (64, 16, 1, ("sum", "lin", "ard"), False), (48, 2, 16, LM, False), (128, 4, 1, ("prod", "ard", "m32"), False),
           (70, 2, 3, ("prod", ("sum", "lin", "m52"), ("sum", "se", "ard")), False), (60, 3, 1, ("sum", ("sum", ("prod", "lin", "m32"), "ard"), "lin0"), False),
           (45, 2, 1, LM, True), (113, 3, 1, ("sum", ("prod", "lin", "ard"), "m12"), False), (24, 3, 2, LM, False), (90, 5, 1, ("sum", "se", "m12"), True),
           (31, 8, 2, ("prod", "lin", "se"), False), (100, 2, 1, ("sum", ("prod", "lin0", "ard"), "m52"), False)]


def test_sixteen_models_in_one_call_train_each_as_alone():
    """mixed n, D (both instantiations), d and tree shapes: every trajectory bit-identical to the model trained alone"""
    from fidelityfusion_amd.cigp_v10 import train_many
    models, xs, ys = make_models2(SIXTEEN, 21)
    solo = [copy.deepcopy(m) for m in models]
    trace, state = train_many(models, xs, ys, 6, lr=LR, tree_one_launch=True)
    assert state["fused"] is True and state["tree_one_launch"] == list(range(16)) and list(state["chunks"]) == [tuple(range(16))]
    assert bool(torch.isfinite(trace).all())
    for f in range(16):
        tr, st = train_many([solo[f]], [xs[f]], [ys[f]], 6, lr=LR, tree_one_launch=True)
        assert st["tree_one_launch"] == [0]
        assert torch.equal(tr[0], trace[f]), (f, rel(tr[0], trace[f]))
        for a, b in zip(params_of(solo[f]), params_of(models[f])):
            assert np.array_equal(a, b), f


def _on_a_handle_of_its_own(fn):
    """fn() with this thread's library calls on a handle created here and destroyed behind it.  (The raw-parameter path lives on
    slot 0 of its GPU, so the new handle takes that slot for the time being.)"""
    from fidelityfusion_amd import _lib
    with _lib._lock:
        kept = _lib._handles.pop((0, 0), None)
    try:
        h = _lib.handle(0)
        assert kept is None or h.value != kept.value
        return fn()
    finally:
        torch.cuda.synchronize()
        with _lib._lock:
            h = _lib._handles.pop((0, 0), None)
            if kept is not None:
                _lib._handles[(0, 0)] = kept
        if h is not None:
            _lib.check(_lib.lib.ffgp_destroy(h), "ffgp_destroy")


def test_the_two_one_launch_drivers_share_the_handles_block():
    """ffgp_train_persist and ffgp_train_tree_lds_raw keep their tables, status words and scratch in ONE block of the handle.  Four calls
    on one handle -- 2 ARD models (the block is made), 3 tree models (the tree driver grows it), 5 ARD models (the plain driver reuses it,
    smaller), 1 tree model (the tree driver reuses it, smaller) -- against the same four calls each on a handle of its own, the first call
    of that handle: traces, parameters and Adam state bit for bit (one workgroup per model, no atomics: the kernels are deterministic)"""
    from fidelityfusion_amd.cigp_v10 import train_many
    calls = [([(17, 2, 1, "ard", False)] * 2, False), ([(33, 2, 1, LM, False)] * 3, True), ([(80, 9, 3, "ard", False)] * 5, False),
             ([(17, 2, 1, LM, False)], True)]
    made = [make_models(members, 41 + 10 * z) for z, (members, _) in enumerate(calls)]

    def run(z):
        models, xs, ys = made[z]
        models = [copy.deepcopy(m) for m in models]      # every run from the same initial parameters
        trace, state = train_many(models, xs, ys, 6, lr=LR, tree_one_launch=calls[z][1])
        n = len(models)
        assert state["fused"] is True and state["tree_one_launch"] == (list(range(n)) if calls[z][1] else [])
        assert list(state["chunks"]) == [tuple(range(n))] and bool(torch.isfinite(trace).all())
        return trace.clone(), [params_of(m) for m in models], state["chunks"][tuple(range(n))].buf.clone()

    alone = [_on_a_handle_of_its_own(lambda z=z: run(z)) for z in range(4)]
    shared = _on_a_handle_of_its_own(lambda: [run(z) for z in range(4)])
    for z in range(4):
        assert torch.equal(shared[z][0], alone[z][0]), (z, rel(shared[z][0], alone[z][0]))
        assert torch.equal(shared[z][2], alone[z][2]), z
        for pa, pb in zip(shared[z][1], alone[z][1]):
            assert all(np.array_equal(a, b) for a, b in zip(pa, pb)), z
        assert any(np.abs(a - b).max() > 0 for pa, pb in zip(alone[z][1], [params_of(m) for m in made[z][0]]) for a, b in zip(pa, pb)), z


def test_seventeen_models_make_two_chunks():
    from fidelityfusion_amd.cigp_v10 import train_many
    members = [(20 + 3 * f, 2, 1, LM, False) for f in range(17)]
    models, xs, ys = make_models(members, 31)
    solo = [copy.deepcopy(m) for m in models]
    trace, state = train_many(models, xs, ys, 4, lr=LR, tree_one_launch=True)
    assert state["tree_one_launch"] == list(range(17))
    assert sorted(state["chunks"]) == [tuple(range(16)), (16,)]
    for f in (0, 15, 16):      # the right rows of the trace: the first chunk's ends and the second chunk's model
        tr, _ = train_many([solo[f]], [xs[f]], [ys[f]], 4, lr=LR, tree_one_launch=True)
        assert torch.equal(tr[0], trace[f]), f
        for a, b in zip(params_of(solo[f]), params_of(models[f])):
            assert np.array_equal(a, b), f


def test_mixed_call_trains_each_model_as_alone_one_launch():
    """a tree model (one-launch route), a plain model and a residual model in ONE train_many call: each trajectory is the one of training
    that model alone, bit for bit -- test_gpu_train_tree.test_mixed_call_trains_each_model_as_alone under the keyword"""
    from test_gpu_train_residual import make_residual
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.cigp_v10 import cigp, train_many
    from oracle import gp_oracle as O

    def build():
        tree, xs, ys = make_models([(50, 2, 1, LM, False)], 5)
        Xp, Yp = O.synthetic_xy(70, 3, 2, seed=8)
        plain = cigp(kernel.ARDKernel(3), 0.8).double().to(DEV)
        mr, xr, res = make_residual(64, 2, 1, "matern", "subset", 9)
        return [tree[0], plain, mr], [xs[0], T(Xp), xr], [ys[0], T(Yp), None], [None, None, res]
    models, xs, ys, rs = build()
    trace, state = train_many(models, xs, ys, 12, lr=1e-2, residual=rs, tree_one_launch=True)
    assert state["fused"] is True and state["tree_one_launch"] == [0]
    solo, xs2, ys2, rs2 = build()
    for f in range(3):
        tr, st = train_many([solo[f]], [xs2[f]], [ys2[f]], 12, lr=1e-2, residual=[rs2[f]], tree_one_launch=True)
        assert st["fused"] is True and st["tree_one_launch"] == ([0] if f == 0 else [])
        assert torch.equal(tr[0], trace[f]), (f, rel(tr[0], trace[f]))
        for a, b in zip(params_of(solo[f]), params_of(models[f])):
            assert np.array_equal(a, b), f
    assert torch.equal(rs2[2][0].detach(), rs[2][0].detach())


def test_not_positive_definite_stops_that_model_alone():
    """two models in one call, one continued with y_var = -3 I: LinAlgError; the failing model's parameters are bit-identical to before the
    call, the other model has completed its steps as in its solo run (its parameters: train_many returns no trace when it raises), the
    chunk's step count is not advanced, and the next call on the handle works"""
    from fidelityfusion_amd.cigp_v10 import train_many
    members = [(30, 2, 1, LM, False), (50, 3, 1, ("prod", "ard", "m52"), False)]
    models, xs, ys = make_models(members, 7)
    solo, xs_s, ys_s = make_models(members, 7)
    _, state = train_many(models, xs, ys, 2, lr=1e-2, tree_one_launch=True)
    assert state["tree_one_launch"] == [0, 1] and state["chunks"][(0, 1)].step == 2
    tr_s, state_s = train_many([solo[1]], [xs_s[1]], [ys_s[1]], 2, lr=1e-2, tree_one_launch=True)
    mid = params_of(models[0])
    n = xs[0].shape[0]
    with pytest.raises(torch.linalg.LinAlgError):
        train_many(models, xs, [[ys[0], -3.0 * torch.eye(n, device=DEV)], ys[1]], 4, lr=1e-2, state=state, tree_one_launch=True)
    assert state["tree_one_launch"] == [0, 1]
    assert all(np.array_equal(a, b) for a, b in zip(params_of(models[0]), mid))      # bit-identical to before the failing call
    tr_s2, state_s = train_many([solo[1]], [xs_s[1]], [ys_s[1]], 4, lr=1e-2, state=state_s, tree_one_launch=True)
    assert bool(torch.isfinite(tr_s2).all())
    for a, b in zip(params_of(solo[1]), params_of(models[1])):      # the other model trained on, as alone
        assert np.array_equal(a, b)
    assert state["chunks"][(0, 1)].step == 2                         # the optimisers of the failed call were not advanced
    trace, state = train_many(models, xs, ys, 1, lr=1e-2, state=state, tree_one_launch=True)      # ... and the handle is usable again
    assert bool(torch.isfinite(trace).all())


def test_c_abi_refuses_what_the_kernel_does_not_cover():
    """ffgp_train_tree_lds_raw through ctypes: FFGP_ERR_ARG with parameters, state and trace untouched for n = 129, D = 17, d = 17, an RQ
    leaf, one leaf, five leaves and F = 17 -- and the accepted call behind them runs"""
    from fidelityfusion_amd import _lib
    from fidelityfusion_amd._lib import KDesc, KTree, Problem, TreeLinks
    from oracle import gp_oracle as O
    n, D = 20, 2
    X, Y = O.synthetic_xy(n, D, 1, seed=2)
    x, y = T(X), T(Y)
    raw = {k: T(v) for k, v in {"w0": [1.0, 1.2], "a0": [1.0], "c0": [0.1, -0.1], "w1": [0.9, 1.1], "a1": [1.0], "lb": [0.7]}.items()}
    h = _lib.handle(0)
    _lib.bind_stream(h, 0)
    opt = _lib.Adam(1e-2, 0.9, 0.999, 1e-8)
    P = 2 * D + 1 + D + 1 + 1

    def call(nl=2, kfun1=3, np_=n, Dp=D, dp=1, F=1):
        arr = (KDesc * 5)()
        for e in range(5):
            arr[e].kfun, arr[e].clamp_min, arr[e].kparam = (5, float("-inf"), 1.0) if e == 0 else (kfun1, 1e-30, 1.0)
            arr[e].w_dev, arr[e].amp_dev = raw["w0" if e == 0 else "w1"].data_ptr(), raw["a0" if e == 0 else "a1"].data_ptr()
        arr[0].center_dev = raw["c0"].data_ptr()
        t = KTree()
        t.n_leaves, t.shape, t.leaf = nl, 0, arr
        p = Problem()
        p.n, p.D, p.d, p.X_dev, p.Y_dev, p.diag_add_dev = np_, Dp, dp, x.data_ptr(), y.data_ptr(), raw["lb"].data_ptr()
        p.ll_variant, p.pi_const = 1, 3.1415
        p.tree = C.pointer(t)
        L = TreeLinks()
        for e in range(4):
            L.leaf[e].w_link, L.leaf[e].w_c = (_lib.LINK_INV, 0.0) if e == 0 else (_lib.LINK_INV_ABS_EPS, 1e-9)
            L.leaf[e].amp_link = _lib.LINK_ABS
        L.leaf[0].center_train = 1
        L.dadd_link, L.dadd_c, L.out_scale = _lib.LINK_EXP_NEG, 1e-6, 1.0
        state = torch.zeros(2 * 200, device=DEV)
        trace = torch.full((3,), -7.0, device=DEV)
        rc = _lib.lib.ffgp_train_tree_lds_raw(h, F, C.byref(p), C.byref(L), 3, C.byref(opt), state.data_ptr(), 400, 0, trace.data_ptr(), 3)
        torch.cuda.synchronize()
        return rc, state, trace

    before = {k: v.clone() for k, v in raw.items()}
    refused = {"n_129": dict(np_=129), "D_17": dict(Dp=17), "d_17": dict(dp=17), "rq_leaf": dict(kfun1=4), "one_leaf": dict(nl=1),
               "five_leaves": dict(nl=5), "F_17": dict(F=17)}
    for name, kw in refused.items():
        rc, state, trace = call(**kw)
        assert rc == _lib.FFGP_ERR_ARG, (name, rc)
        assert float(state.abs().max()) == 0.0 and bool((trace == -7.0).all()), name
        assert all(torch.equal(raw[k], before[k]) for k in raw), name
    rc, state, trace = call()
    assert rc == 0 and bool(torch.isfinite(trace).all()) and float(state[:2 * P].abs().max()) > 0.0
    assert not torch.equal(raw["c0"], before["c0"])


@pytest.mark.parametrize("centre", ["origin", "given"])
def test_untrained_centres_against_the_launch_per_stage_call(centre):
    """a linear leaf whose centre is NOT a parameter -- center_dev NULL (the origin) or given -- cannot be built from the modules (every
    LinearKernel trains its centre), so the two C entry points are compared on ONE description: Sum(Linear, Matern 5/2), n = 40, D = 2,
    40 steps.  Bound 1e-12, the floor of the cases above: either call is within 8e-14 of the per-step loop on every case of the table
    (DESIGN.md section 4.8), so the two are within 2e-13 of each other where both are right."""
    from fidelityfusion_amd import _lib
    from fidelityfusion_amd._lib import KDesc, KTree, Problem, TreeLinks
    from oracle import gp_oracle as O
    n, D, steps = 40, 2, STEPS1 + STEPS2
    X, Y = O.synthetic_xy(n, D, 1, seed=6)
    x, y = T(X), T(Y)
    h = _lib.handle(0)
    _lib.bind_stream(h, 0)
    opt = _lib.Adam(LR, 0.9, 0.999, 1e-8)
    P = 2 * (D + 1) + 1

    def run(fn):
        raw = {k: T(v) for k, v in {"w0": [1.3, 0.8], "a0": [0.7], "c0": [0.25, -0.15], "w1": [0.9, -1.1], "a1": [1.2], "lb": [0.7]}.items()}
        arr = (KDesc * 2)()
        arr[0].kfun, arr[0].clamp_min, arr[0].kparam = 5, float("-inf"), 1.0
        arr[1].kfun, arr[1].clamp_min, arr[1].kparam = 3, 1e-30, 1.0
        arr[0].w_dev, arr[0].amp_dev = raw["w0"].data_ptr(), raw["a0"].data_ptr()
        arr[1].w_dev, arr[1].amp_dev = raw["w1"].data_ptr(), raw["a1"].data_ptr()
        if centre == "given":
            arr[0].center_dev = raw["c0"].data_ptr()
        t = KTree()
        t.n_leaves, t.shape, t.leaf = 2, 0, arr
        t.op[0] = 0
        p = Problem()
        p.n, p.D, p.d, p.X_dev, p.Y_dev, p.diag_add_dev = n, D, 1, x.data_ptr(), y.data_ptr(), raw["lb"].data_ptr()
        p.ll_variant, p.pi_const = 1, 3.1415
        p.tree = C.pointer(t)
        L = TreeLinks()
        L.leaf[0].w_link, L.leaf[0].w_c, L.leaf[0].amp_link = _lib.LINK_INV, 0.0, _lib.LINK_ABS
        L.leaf[1].w_link, L.leaf[1].w_c, L.leaf[1].amp_link = _lib.LINK_INV_ABS_EPS, 1e-9, _lib.LINK_ABS
        L.dadd_link, L.dadd_c, L.out_scale = _lib.LINK_EXP_NEG, 1e-6, 1.0
        state = torch.zeros(2 * P, device=DEV)
        trace = torch.zeros(steps, device=DEV)
        rc = fn(h, 1, C.byref(p), C.byref(L), steps, C.byref(opt), state.data_ptr(), 2 * P, 0, trace.data_ptr(), steps)
        torch.cuda.synchronize()
        assert rc == 0, rc
        return raw, state, trace

    raw1, state1, trace1 = run(_lib.lib.ffgp_train_tree_lds_raw)
    raw0, state0, trace0 = run(_lib.lib.ffgp_train_tree_raw)
    assert bool(torch.isfinite(trace1).all()) and float(trace1[-1]) < float(trace1[0])
    assert torch.equal(raw1["c0"], T([0.25, -0.15]))                       # not a parameter: untouched
    errs = {"trace": rel(trace1, trace0)}
    for k in ("w0", "a0", "w1", "a1", "lb"):
        assert not torch.equal(raw1[k], T({"w0": [1.3, 0.8], "a0": [0.7], "w1": [0.9, -1.1], "a1": [1.2], "lb": [0.7]}[k])), k      # trained
        errs[k] = rel(raw1[k], raw0[k])
    print(centre, errs)
    assert max(errs.values()) <= 1e-12, errs
