"""train_many for models whose kernel is a SumKernel / ProductKernel tree (cigp_v10.train_many -> ffgp_train_tree_raw): K Adam steps
per library call, the links of every leaf and Adam's update on the device, against the per-step loop through the drop-in modules and
torch.optim.Adam -- what these models ran on before -- and against fixtures of the reference's own loop
(tests/golden/train_tree_*.npz, written by tests/golden/gen_train_tree_goldens.py).

The trajectory bound.  The fused call and the loop run the SAME likelihood launches; they differ in where the links' chain rule is
evaluated (library: exp(-log_beta) + jitter and ffgp_link_der; loop: torch's exp().pow(-1) + jitter and autograd) -- by rounding.  The
yardstick d0 of a case is the distance between two per-step loops that themselves differ only by rounding (kernel.FUSE_PAIRS = True:
one tile pass; False: part by part), measured on an MI355X with this file's own metric; the bound is 10 x d0 (one decade for the
run-to-run spread of a rounding-level quantity), never below the 1e-12 that test_gpu_train.py uses where the arithmetic is identical,
and a case whose 10 x d0 exceeded 1e-9 would be ill-conditioned and would have been replaced.  Measured d0 and the trainer's own
distance per case: DESIGN.md section 4.8."""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(torch.float32)


DEV = "cuda:0"


def T(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)


def rel(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    return float(np.abs(a.reshape(b.shape) - b).max() / max(np.abs(b).max(), 1e-300))


def params_of(m):
    return [p.detach().cpu().numpy().copy() for p in m.parameters()]


def reference_loop(models, xs, ys, steps, lr):
    """the reference's loop: a fresh Adam per model, the loss recorded before the update"""
    trace = np.zeros((len(models), steps))
    for f, (m, x, y) in enumerate(zip(models, xs, ys)):
        opt = torch.optim.Adam(m.parameters(), lr=lr)
        for k in range(steps):
            opt.zero_grad()
            loss = -m.negative_log_likelihood(x, y)
            loss.backward()
            opt.step()
            trace[f, k] = float(loss.detach())
    return trace


def distance(trace, models, ref_trace, ref_models):
    """the metric of every trajectory comparison here: the largest of rel(trace) and rel(parameter tensor) over all models"""
    d = rel(trace, ref_trace)
    for m, t in zip(models, ref_models):
        for a, b in zip(params_of(m), params_of(t)):
            d = max(d, rel(a, b))
    return d


def build_kernel(spec, D, rng):
    """spec: a leaf name -- lin (LinearKernel, its centre off the origin and trained), ard, se (scalar log length scale, broadcast),
    m12 / m32 / m52 (MaternKernel) -- or ("sum" | "prod", spec, spec)"""
    from fidelityfusion_amd import kernel
    if isinstance(spec, tuple):
        cls = kernel.SumKernel if spec[0] == "sum" else kernel.ProductKernel
        return cls(build_kernel(spec[1], D, rng), build_kernel(spec[2], D, rng))
    if spec == "se":
        return kernel.SquaredExponentialKernel(0.3, 0.2)
    k = {"lin": lambda: kernel.LinearKernel(D), "ard": lambda: kernel.ARDKernel(D), "m12": lambda: kernel.MaternKernel(D, nu=0.5),
         "m32": lambda: kernel.MaternKernel(D, nu=1.5), "m52": lambda: kernel.MaternKernel(D, nu=2.5)}[spec]()
    with torch.no_grad():
        k.length_scales.copy_(torch.tensor(rng.uniform(0.7, 1.6, D) * (rng.choice([-1.0, 1.0], D) if spec != "lin" else 1.0)))
        if spec == "lin":
            k.center.copy_(torch.tensor(rng.uniform(-0.3, 0.3, D)))
    return k


def make_models(members, seed):
    """members: [(n, D, d, kernel spec, with y_var)]"""
    from fidelityfusion_amd.cigp_v10 import cigp
    from oracle import gp_oracle as O
    rng = np.random.default_rng(seed)
    models, xs, ys = [], [], []
    for f, (n, D, d, spec, yvar) in enumerate(members):
        models.append(cigp(build_kernel(spec, D, rng), 0.7 + 0.1 * f).double().to(DEV))
        X, Y = O.synthetic_xy(n, D, d, seed=seed + f)
        xs.append(T(X))
        ys.append([T(Y), torch.diag(T(rng.uniform(0.01, 0.2, n)))] if yvar else T(Y))
    return models, xs, ys


LM = ("sum", "lin", "m52")
# name -> (members, d0 measured on an MI355X: FUSE_PAIRS True against False through the per-step loop, 25 + 15 steps, lr = 1e-2)
CASES = {
    "sum2_n24": ([(24, 3, 2, LM, False)], 8.84e-16),                                                              # 2 leaves, d > 1
    "prod2_n128": ([(128, 4, 1, ("prod", "ard", "m32"), False)], 2.84e-16),                                       # one diagonal block exactly
    "nest3_n129": ([(129, 2, 1, ("sum", ("prod", "lin", "ard"), "m12"), False)], 7.40e-15),                       # 3 leaves, two blocks
    "chain4_n300_yvar": ([(300, 16, 2, ("sum", ("sum", ("prod", "ard", "se"), "m52"), "lin"), True)], 2.46e-14),  # 4-chain, D = 16, [y, y_var]
    "balanced4_n700": ([(700, 2, 3, ("prod", ("sum", "lin", "m52"), ("sum", "se", "ard")), False)], 8.17e-14),    # 4-balanced, broadcast SE
    "three_small": ([(24, 3, 1, LM, False), (60, 2, 2, ("prod", "se", "m32"), True), (128, 5, 1, ("sum", ("sum", "ard", "m12"), "lin"), False)],
                    1.63e-14),                                                                                    # several tree models, ONE call
    "three_large": ([(150, 3, 1, LM, False), (260, 2, 2, ("prod", "ard", "m52"), False), (200, 4, 1, ("sum", ("prod", "lin", "se"), "m32"), True)],
                    2.65e-14),                                                                                    # side by side from host threads
}
STEPS1, STEPS2, LR = 25, 15, 1e-2


def loop_yardstick(name):
    """d0 of a case: two per-step loops that differ only in rounding (for re-measuring the table above; the tests do not call it)"""
    from fidelityfusion_amd import kernel
    members = CASES[name][0]
    runs = []
    for fuse in (True, False):
        kernel.FUSE_PAIRS = fuse
        try:
            models, xs, ys = make_models(members, 11)
            runs.append((reference_loop(models, xs, ys, STEPS1 + STEPS2, LR), models))
        finally:
            kernel.FUSE_PAIRS = True
    return distance(runs[1][0], runs[1][1], runs[0][0], runs[0][1])


def test_sum_kernel_model_is_trained_by_the_fused_call():
    """fails before ffgp_train_tree_raw: a SumKernel model fell back to the reference loop (state["fused"] False, .grad populated)"""
    from fidelityfusion_amd.cigp_v10 import train_many
    models, xs, ys = make_models([(40, 2, 1, LM, False)], 3)
    before = params_of(models[0])
    trace, state = train_many(models, xs, ys, 5, lr=1e-2)
    assert state["fused"] is True
    assert all(p.grad is None for p in models[0].parameters())
    assert trace.shape == (1, 5) and trace.is_cuda and bool(torch.isfinite(trace).all())
    assert float(trace[0, -1]) < float(trace[0, 0])
    assert all(np.abs(a - b).max() > 0 for a, b in zip(params_of(models[0]), before))      # every parameter moved, the centre included


@pytest.mark.parametrize("name", sorted(CASES))
def test_train_many_tree_follows_the_per_step_loop(name):
    from fidelityfusion_amd.cigp_v10 import train_many
    members, d0 = CASES[name]
    assert d0 is not None and 10 * d0 <= 1e-9, "the case has no measured yardstick, or is ill-conditioned"
    bound = max(10 * d0, 1e-12)
    models, xs, ys = make_models(members, 11)
    twins = [copy.deepcopy(m) for m in models]
    trace, state = train_many(models, xs, ys, STEPS1, lr=LR)
    assert state["fused"] is True
    trace2, state = train_many(models, xs, ys, STEPS2, lr=LR, state=state)      # the optimisers continue where they stopped
    ref = reference_loop(twins, xs, ys, STEPS1 + STEPS2, LR)
    dist = distance(torch.cat([trace, trace2], dim=1), models, ref, twins)
    print("%s: d0 %.3g, trainer %.3g, bound %.3g" % (name, d0, dist, bound))
    assert dist <= bound, (dist, bound)


FIXTURES = {
    "train_tree_demo1": (1, ("sum", "lin", "m52")),
    "train_tree_demo2": (2, ("sum", "lin", "m52")),
    "train_tree_prod": (3, ("prod", "ard", "m52")),
    "train_tree_nest3": (2, ("sum", ("prod", "lin", "ard"), "m52")),
}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_train_many_tree_on_the_reference_fixtures(golden, name):
    """the reference's own loop in fp64 on the CPU (trajectories shown well-conditioned by the generator: twin distance <= 2e-13):
    loss trace and final parameters within 1e-8, the bound resgp_chain is held to"""
    from fidelityfusion_amd.cigp_v10 import cigp, train_many
    g = golden(name)
    D, spec = FIXTURES[name]
    m = cigp(build_kernel(spec, D, np.random.default_rng(0)), 1.0).double().to(DEV)
    with torch.no_grad():
        for i, p in enumerate(m.parameters()):
            p.copy_(T(g["init_%d" % i]).reshape(p.shape))
    trace, state = train_many([m], [T(g["x"])], [T(g["y"])], int(g["steps"]), lr=float(g["lr"]))
    assert state["fused"] is True
    errs = {"trace": rel(trace[0], g["trace"])}
    for i, p in enumerate(m.parameters()):
        errs["final_%d" % i] = rel(p, g["final_%d" % i])
    print(name, errs)
    assert max(errs.values()) <= 1e-8, errs


def test_mixed_call_trains_each_model_as_alone():
    """a tree model, a plain model and a residual model (all <= 128 points) in ONE train_many call: each trajectory is the one of
    training that model alone, bit for bit (the tree model forms a library call of its own either way; the other two are one
    workgroup each of the one-launch trainer)"""
    from test_gpu_train_residual import clone_residual, make_residual
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
    trace, state = train_many(models, xs, ys, 12, lr=1e-2, residual=rs)
    assert state["fused"] is True
    solo, xs2, ys2, rs2 = build()
    for f in range(3):
        tr, st = train_many([solo[f]], [xs2[f]], [ys2[f]], 12, lr=1e-2, residual=[rs2[f]])
        assert st["fused"] is True
        assert torch.equal(tr[0], trace[f]), (f, rel(tr[0], trace[f]))
        for a, b in zip(params_of(solo[f]), params_of(models[f])):
            assert np.array_equal(a, b), f
    assert torch.equal(rs2[2][0].detach(), rs[2][0].detach())


def test_not_positive_definite_raises_and_leaves_the_parameters():
    from fidelityfusion_amd.cigp_v10 import train_many
    models, xs, ys = make_models([(30, 2, 1, LM, False), (150, 2, 1, LM, False)], 7)
    for f in (0, 1):
        n = xs[f].shape[0]
        before = params_of(models[f])
        ok_trace, state = train_many([models[f]], [xs[f]], [ys[f]], 2, lr=1e-2)
        step = state["chunks"][(0,)].step
        mid = params_of(models[f])
        with pytest.raises(torch.linalg.LinAlgError):
            train_many([models[f]], [xs[f]], [[ys[f], -3.0 * torch.eye(n, device=DEV)]], 4, lr=1e-2, state=state)
        assert all(np.array_equal(a, b) for a, b in zip(params_of(models[f]), mid))      # bit-identical to before the failing call
        assert any(np.abs(a - b).max() > 0 for a, b in zip(mid, before))
        assert state["chunks"][(0,)].step == step == 2                                       # the optimisers were not advanced
        trace, state = train_many([models[f]], [xs[f]], [ys[f]], 1, lr=1e-2, state=state)     # ... and the handle is usable again
        assert bool(torch.isfinite(trace).all())


def _fallback_cases():
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.cigp_v10 import cigp
    from oracle import gp_oracle as O
    X, Y = O.synthetic_xy(40, 2, 1, seed=4)
    x, y = T(X), T(Y)
    mk = lambda k: cigp(k, 0.8).double().to(DEV)
    shared = kernel.ARDKernel(2)
    frozen = mk(kernel.SumKernel(kernel.LinearKernel(2), kernel.MaternKernel(2)))
    frozen.kernel.kernel1.center.requires_grad_(False)
    rho = torch.nn.Parameter(torch.tensor(0.8, dtype=torch.float64, device=DEV))
    plain = lambda: mk(kernel.SumKernel(kernel.LinearKernel(2), kernel.MaternKernel(2)))
    return {
        "rq_leaf": (mk(kernel.SumKernel(kernel.RationalQuadraticKernel(), kernel.MaternKernel(2))), x, y, None, True),
        "frozen_leaf_parameter": (frozen, x, y, None, True),
        "module_used_twice": (mk(kernel.SumKernel(shared, shared)), x, y, None, True),
        "fuse_pairs_off": (plain(), x, y, None, False),
        "residual_link": (plain(), x, None, (rho, 0.5 * y, y), True),
        "cpu_tensors": (cigp(kernel.SumKernel(kernel.LinearKernel(2), kernel.MaternKernel(2)), 0.8).double(), x.cpu(), y.cpu(), None, True),
    }


@pytest.mark.parametrize("case", ["rq_leaf", "frozen_leaf_parameter", "module_used_twice", "fuse_pairs_off", "residual_link", "cpu_tensors"])
def test_fallbacks_stay_fallbacks(case):
    """what ffgp_train_tree_raw does not train keeps the reference loop: state["fused"] False, and the loop's own trajectory"""
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.cigp_v10 import train_many
    m, x, y, res, fuse = _fallback_cases()[case]
    twin = copy.deepcopy(m)
    res_t = (torch.nn.Parameter(res[0].detach().clone()), res[1], res[2]) if res is not None else None
    kernel.FUSE_PAIRS = fuse
    try:
        trace, state = train_many([m], [x], [y], 4, lr=1e-2, residual=None if res is None else [res])
        assert state["fused"] is False
        opt = torch.optim.Adam([p for p in twin.parameters()] + ([res_t[0]] if res_t else []), lr=1e-2)
        ref = []
        for _ in range(4):
            opt.zero_grad()
            loss = -twin.negative_log_likelihood(x, y if res_t is None else res_t[2] - res_t[0] * res_t[1])
            loss.backward()
            opt.step()
            ref.append(float(loss.detach()))
    finally:
        kernel.FUSE_PAIRS = True
    assert rel(trace[0], np.array(ref)) <= 1e-12
    for a, b in zip(params_of(m), params_of(twin)):
        assert rel(a, b) <= 1e-12
    if res is not None:
        assert rel(res[0], res_t[0]) <= 1e-12


def test_parameters_are_updated_in_place_and_the_posterior_is_rebuilt():
    from fidelityfusion_amd.cigp_v10 import train_many
    models, xs, ys = make_models([(90, 2, 1, LM, False)], 13)
    twins = [copy.deepcopy(m) for m in models]
    with torch.no_grad():
        stale, _ = models[0](xs[0], ys[0], xs[0][:5])      # caches the factor of the untrained parameters
    train_many(models, xs, ys, 20, lr=1e-2)
    reference_loop(twins, xs, ys, 20, 1e-2)
    with torch.no_grad():
        mean, _ = models[0](xs[0], ys[0], xs[0][:5])
        mean_t, _ = twins[0](xs[0], ys[0], xs[0][:5])
    assert rel(mean, mean_t) <= 1e-9
    assert rel(mean, stale) > 1e-6


def test_c_abi_refuses_what_it_does_not_train():
    """ffgp_train_tree_raw through ctypes: every refused shape returns FFGP_ERR_ARG before anything is enqueued (state, trace and the
    parameters untouched), and the accepted call behind them still runs"""
    from fidelityfusion_amd import _lib
    from fidelityfusion_amd._lib import KDesc, KTree, Problem, TreeLinks
    n, D = 20, 2
    from oracle import gp_oracle as O
    X, Y = O.synthetic_xy(n, D, 1, seed=2)
    x, y = T(X), T(Y)
    raw = {k: T(v) for k, v in {"w0": [1.0, 1.2], "a0": [1.0], "c0": [0.1, -0.1], "w1": [0.9, 1.1], "a1": [1.0], "lb": [0.7]}.items()}
    h = _lib.handle(0)
    _lib.bind_stream(h, 0)
    opt = _lib.Adam(1e-2, 0.9, 0.999, 1e-8)
    P = 2 * D + 1 + D + 1 + 1

    def call(nl=2, kfun1=3, cov=False, Dp=D, stride=2 * P, F=1, tree=True):
        arr = (KDesc * 4)()
        for e in range(4):
            arr[e].kfun, arr[e].clamp_min, arr[e].kparam = (5, float("-inf"), 1.0) if e == 0 else (kfun1, 1e-30, 1.0)
            arr[e].w_dev, arr[e].amp_dev = raw["w0" if e == 0 else "w1"].data_ptr(), raw["a0" if e == 0 else "a1"].data_ptr()
        arr[0].center_dev = raw["c0"].data_ptr()
        t = KTree()
        t.n_leaves, t.shape, t.leaf = nl, 0, arr
        p = Problem()
        p.n, p.D, p.d, p.X_dev, p.Y_dev, p.diag_add_dev = n, Dp, 1, x.data_ptr(), y.data_ptr(), raw["lb"].data_ptr()
        p.ll_variant, p.pi_const = 1, 3.1415
        if tree:
            p.tree = C.pointer(t)
        if cov:
            p.cov_dev, p.ld_cov = x.data_ptr(), n
        L = TreeLinks()
        for e in range(4):
            L.leaf[e].w_link, L.leaf[e].w_c = (_lib.LINK_INV, 0.0) if e == 0 else (_lib.LINK_INV_ABS_EPS, 1e-9)
            L.leaf[e].amp_link = _lib.LINK_ABS
        L.leaf[0].center_train = 1
        L.dadd_link, L.dadd_c, L.out_scale = _lib.LINK_EXP_NEG, 1e-6, 1.0
        state = torch.zeros(max(stride, 2 * P), device=DEV)
        trace = torch.full((3,), -7.0, device=DEV)
        rc = _lib.lib.ffgp_train_tree_raw(h, F, C.byref(p), C.byref(L), 3, C.byref(opt), state.data_ptr(), stride, 0, trace.data_ptr(), 3)
        torch.cuda.synchronize()
        return rc, state, trace

    before = {k: v.clone() for k, v in raw.items()}
    refused = {"one_leaf": dict(nl=1), "five_leaves": dict(nl=5), "rq_leaf": dict(kfun1=4), "cov_dev": dict(cov=True), "D_129": dict(Dp=129),
               "short_state_stride": dict(stride=2 * P - 1), "no_tree": dict(tree=False), "too_many_models": dict(F=17)}
    for name, kw in refused.items():
        rc, state, trace = call(**kw)
        assert rc == _lib.FFGP_ERR_ARG, (name, rc)
        assert float(state.abs().max()) == 0.0 and bool((trace == -7.0).all()), name
        assert all(torch.equal(raw[k], before[k]) for k in raw), name
    rc, state, trace = call()
    assert rc == 0 and bool(torch.isfinite(trace).all()) and float(state.abs().max()) > 0.0
    assert not torch.equal(raw["c0"], before["c0"])
