"""train_many(..., fuse_composed=True): train_AR's residual fidelities on a composed kernel (a `cigp` over SumKernel / ProductKernel
trees with a `residual=` link -> ffgp_train_tree_res_raw, csrc/train_tree_res.hip) and `GP_basic` blocks over a composed kernel
(noise_variance under the square link, no jitter, FFGP_LL_V2 -> the tree entries), launch per stage -- against fixtures of the
reference's own loops (tests/golden/train_tree_ar_*.npz, train_tree_gpbasic*.npz, written by gen_train_tree_residual_goldens.py), the
per-step loop through the drop-in modules, and itself (each model as alone, bit for bit).  Every test asserts through state["fused"]
(and state["tree_one_launch"]) that the models went where it meant them to go.

The trajectory bound is test_gpu_train_tree.py's: max(10 x d0, 1e-12), d0 = the case's loop yardstick (two per-step loops that differ
only in rounding, kernel.FUSE_PAIRS True / False -- code this route does not touch), measured on an MI355X and written into the case
table.  A case whose bound would exceed 1e-9 is ill-conditioned and is replaced.  Measured d0 and trainer distances: DESIGN.md
section 4.8.  Both routes are run: launch per stage (ffgp_train_tree_res_raw / ffgp_train_tree_raw) and, under `tree_one_launch=True` for
members of at most 128 points, ONE launch per likelihood class (ffgp_train_tree_lds_res_raw, csrc/train_tree_lds_res.hip)."""
import copy
import ctypes as C

import numpy as np
import pytest

from test_gpu_train_residual import clone_residual
from test_gpu_train_tree import DEV, LM, LR, STEPS1, STEPS2, T, make_models, rel
from test_gpu_train_tree_lds import build_kernel2

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(torch.float32)


def params_of(m, rho=None):
    out = [p.detach().cpu().numpy().copy() for p in m.parameters()]
    return out + ([rho.detach().cpu().numpy().copy().reshape(-1)] if rho is not None else [])


def make_member(n, D, d, spec, form, seed, cls="cigp", rho0=0.8):
    """one member: (model, x, y or None, residual link or None).  form: "plain" (targets), "subset" (rho, y_low, y_high) or "full"
    (diagonal [n, n] variances with v_low several times v_high on most points, so that s_i = v_high - rho v_low is negative there and
    the abs backward's sign matters; positive on the others)"""
    from fidelityfusion_amd.cigp_v10 import cigp
    from fidelityfusion_amd.gp_basic import GP_basic
    rng = np.random.default_rng(seed)
    k = build_kernel2(spec, D, rng)
    m = (cigp(k, 0.6) if cls == "cigp" else GP_basic(k, 0.5)).double().to(DEV)
    x = rng.uniform(0, 1, (n, D))
    yl = np.sin(3 * x[:, :1] + np.arange(d)) + 0.1 * rng.standard_normal((n, d))
    yh = 1.3 * yl + 0.2 * np.cos(2 * x[:, :1]) + 0.05 * rng.standard_normal((n, d))
    if form == "plain":
        return m, T(x), T(yh), None
    rho = torch.nn.Parameter(torch.tensor(rho0, dtype=torch.float64, device=DEV))
    if form == "subset":
        return m, T(x), None, (rho, T(yl), T(yh))
    vh = rng.uniform(0.01, 0.03, n)
    vl = vh * rng.uniform(3.0, 6.0, n)                 # s < 0 at rho ~ 0.8
    vl[np.arange(n) % 4 == 1] *= 0.05                  # s > 0
    return m, T(x), None, (rho, [T(yl), torch.diag(T(vl))], [T(yh), torch.diag(T(vh))])


def loss_of(m, x, y):
    if hasattr(m, "negative_log_likelihood"):
        return -m.negative_log_likelihood(x, y)
    return (-m.log_likelihood(x, y)).sum()


def reference_loop(m, x, y, res, steps, lr):
    """the reference's loops through the drop-in modules: train_AR's (AR_autoRegression.py:123-137) for a residual member, the plain one
    otherwise; a `GP_basic` minimises -log_likelihood(...).sum().  Returns (trace, the last step's targets)"""
    opt = torch.optim.Adam(list(m.parameters()) + ([res[0]] if res is not None else []), lr=lr)
    trace, last = [], None
    for _ in range(steps):
        opt.zero_grad()
        if res is not None:
            rho, yl, yh = res
            y = [yh[0] - rho * yl[0], (yh[1] - rho * yl[1]).abs()] if isinstance(yl, list) else yh - rho * yl
        last = y
        loss = loss_of(m, x, y)
        loss.backward()
        opt.step()
        trace.append(float(loss.detach()))
    return np.array(trace), last


def distance(trace, m, rho, ref_trace, twin, trho):
    d = rel(trace, ref_trace)
    for a, b in zip(params_of(m, rho), params_of(twin, trho)):
        d = max(d, rel(a, b))
    return d


NEST3 = ("sum", ("prod", "lin", "ard"), "m12")
BAL4 = ("prod", ("sum", "lin", "m52"), ("sum", "lin0", "ard"))      # a centre off the origin (trained) and one still AT the origin
# name -> ((n, D, d, spec, form, class), d0 measured on an MI355X: FUSE_PAIRS True against False through the per-step loop, 25 + 15 steps)
CASES = {
    "n16_D1": ((16, 1, 2, LM, "subset", "cigp"), 3.23e-16),               # one block
    "n17_D9": ((17, 9, 2, LM, "full", "cigp"), 3.80e-16),                 # a second, almost empty block; the padded half of a 16-wide unroll
    "n113_nest3": ((113, 2, 1, NEST3, "subset", "cigp"), 8.71e-16),       # a ragged last block
    "n128_D16_d16": ((128, 16, 16, LM, "full", "cigp"), 2.68e-15),
    "balanced4": ((60, 2, 2, BAL4, "subset", "cigp"), 1.29e-15),
    "negative_s": ((40, 2, 1, LM, "full", "cigp"), 5.61e-16),             # v_low several times v_high
    "gpbasic_plain": ((32, 2, 1, LM, "plain", "gpbasic"), 3.14e-15),      # V2
    "gpbasic_residual": ((50, 1, 1, LM, "subset", "gpbasic"), 8.21e-14),  # V2 x residual
    "n129": ((129, 2, 1, LM, "full", "cigp"), 3.42e-15),                  # the blocked path
    "n300": ((300, 3, 2, NEST3, "subset", "cigp"), 6.65e-16),
}
SEED = 11


def loop_yardstick(name):
    """d0 of a case (for re-measuring the table above; the tests do not call it)"""
    from fidelityfusion_amd import kernel
    runs = []
    for fuse in (True, False):
        kernel.FUSE_PAIRS = fuse
        try:
            m, x, y, res = make_member(*CASES[name][0][:5], SEED, CASES[name][0][5])
            tr, _ = reference_loop(m, x, y, res, STEPS1 + STEPS2, LR)
            runs.append((tr, m, res[0] if res is not None else None))
        finally:
            kernel.FUSE_PAIRS = True
    return distance(runs[1][0], runs[1][1], runs[1][2], runs[0][0], runs[0][1], runs[0][2])


def bound_of(name):
    d0 = CASES[name][1]
    assert d0 is not None and 10 * d0 <= 1e-9, "the case has no measured yardstick, or is ill-conditioned"
    return max(10 * d0, 1e-12)


def test_tree_model_with_a_residual_link_is_fused_under_the_keyword():
    """fails before ffgp_train_tree_res_raw: train_many has no keyword fuse_composed (TypeError)"""
    from fidelityfusion_amd.cigp_v10 import train_many
    m, x, _, res = make_member(40, 2, 1, LM, "subset", 3)
    before = params_of(m, res[0])
    trace, state = train_many([m], [x], [None], 8, lr=1e-2, residual=[res], fuse_composed=True)
    assert state["fused"] is True and state["tree_one_launch"] == []
    assert all(p.grad is None for p in m.parameters()) and res[0].grad is None
    assert trace.shape == (1, 8) and trace.is_cuda and bool(torch.isfinite(trace).all())
    assert bool((trace[0, 1:] < trace[0, :-1]).all())
    assert all(np.abs(a - b).max() > 0 for a, b in zip(params_of(m, res[0]), before))      # every parameter moved, rho included
    m, x, _, res = make_member(40, 2, 1, LM, "subset", 3)
    _, state = train_many([m], [x], [None], 2, lr=1e-2, residual=[res])
    assert state["fused"] is False                                                           # off by default


ROUTES = ["stage", "lds"]
SMALL = sorted(n for n in CASES if CASES[n][0][0] <= 128)


def _kw(route):
    return dict(fuse_composed=True, tree_one_launch=(route == "lds"))


def _follow(name, route="stage"):
    from fidelityfusion_amd.cigp_v10 import train_many
    (n, D, d, spec, form, cls), d0 = CASES[name]
    bound = bound_of(name)
    went = [0] if route == "lds" and n <= 128 else []
    m, x, y, res = make_member(n, D, d, spec, form, SEED, cls)
    twin, tres = copy.deepcopy(m), (clone_residual(res) if res is not None else None)
    rs = [res] if res is not None else None
    trace, state = train_many([m], [x], [y], STEPS1, lr=LR, residual=rs, **_kw(route))
    assert state["fused"] is True and state["tree_one_launch"] == went
    trace2, state = train_many([m], [x], [y], STEPS2, lr=LR, residual=rs, state=state, **_kw(route))
    assert state["chunks"][(0,)].step == STEPS1 + STEPS2 and state["tree_one_launch"] == went
    ref, last = reference_loop(twin, x, y, tres, STEPS1 + STEPS2, LR)
    assert bool(torch.isfinite(trace).all()) and bool(torch.isfinite(trace2).all())
    dist = distance(torch.cat([trace, trace2], dim=1)[0], m, res[0] if res else None, ref, twin, tres[0] if tres else None)
    print("%s [%s]: d0 %.3g, trainer %.3g, bound %.3g" % (name, route, d0, dist, bound))
    assert dist <= bound, (dist, bound)
    return state, last, res


@pytest.mark.parametrize("name", sorted(CASES))
def test_follows_the_per_step_loop(name):
    _follow(name)


@pytest.mark.parametrize("name", SMALL)
def test_follows_the_per_step_loop_in_one_launch(name):
    _follow(name, "lds")


@pytest.mark.parametrize("name", ["n17_D9", "n300", "gpbasic_residual"])
def test_residual_targets_are_the_torch_expression_at_rho_last(name):
    """state["residual_targets"][f] = [y_high - rho y_low, |v_high - rho v_low| or None] at the rho of the start of the last step: the
    targets of the reference loop's last iteration.  Its rho agrees to the case's bound and the expression is linear in rho:
    |delta r| <= |delta rho| max|y_low|, and max|y_low| / max|r| (likewise for the variances) is below 10 on this data"""
    state, last, res = _follow(name, "stage" if name == "n300" else "lds")
    got = state["residual_targets"][0]
    want = last if isinstance(last, list) else [last, None]
    assert rel(got[0], want[0].detach()) <= 10 * bound_of(name)
    if want[1] is None:
        assert got[1] is None
    else:
        assert rel(got[1], want[1].detach()) <= 10 * bound_of(name)
    # ... and bit for bit the torch expression at a rho one Adam step back from the final one: rho_last is not the final rho
    rho, yl, yh = res
    final = (yh[0] if isinstance(yh, list) else yh) - rho.detach() * (yl[0] if isinstance(yl, list) else yl)
    assert not torch.equal(got[0], final)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("form", ["subset", "full"])
def test_residual_targets_after_one_step_are_the_expression_at_the_initial_rho(form, route):
    """one step: the rho of the start of the last step is the rho given, so the targets are torch's own expression on it, bit for bit"""
    from fidelityfusion_amd.cigp_v10 import train_many
    m, x, _, res = make_member(37, 2, 2, LM, form, 4)
    rho0 = res[0].detach().clone()
    _, state = train_many([m], [x], [None], 1, lr=1e-2, residual=[res], **_kw(route))
    assert state["fused"] is True and not torch.equal(res[0].detach(), rho0) and state["tree_one_launch"] == ([0] if route == "lds" else [])
    got = state["residual_targets"][0]
    if form == "subset":
        assert torch.equal(got[0], res[2] - rho0 * res[1]) and got[1] is None
    else:
        assert torch.equal(got[0], res[2][0] - rho0 * res[1][0]) and torch.equal(got[1], (res[2][1] - rho0 * res[1][1]).abs())


FIXTURES = {
    "train_tree_ar_subset": (1, LM, "cigp"),
    "train_tree_ar_nonsubset": (2, LM, "cigp"),
    "train_tree_gpbasic": (2, LM, "gpbasic"),
    "train_tree_gpbasic_ar": (1, LM, "gpbasic"),
    "train_tree_ar_nest3": (3, ("sum", ("prod", "lin", "ard"), "m52"), "cigp"),
}


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_on_the_reference_fixtures(golden, name, route):
    """the reference's own loops in fp64 on the CPU (each trajectory shown well-conditioned by the generator: a twin started one ulp
    away stays within 1e-11): loss trace, final parameters and final rho within 1e-8, the bound every reference fixture is held to"""
    from fidelityfusion_amd.cigp_v10 import cigp, train_many
    from fidelityfusion_amd.gp_basic import GP_basic
    g = golden(name)
    D, spec, cls = FIXTURES[name]
    k = build_kernel2(spec, D, np.random.default_rng(0))
    m = (cigp(k, 1.0) if cls == "cigp" else GP_basic(k, 1.0)).double().to(DEV)
    with torch.no_grad():
        for i, p in enumerate(m.parameters()):
            p.copy_(T(g["init_%d" % i]).reshape(p.shape))
    x, res, y = T(g["x"]), None, None
    if "y_low" in g:
        rho = torch.nn.Parameter(T(g["rho_init"]).reshape(()))
        if "v_low" in g:
            res = (rho, [T(g["y_low"]), T(g["v_low"])], [T(g["y_high"]), T(g["v_high"])])
        else:
            res = (rho, T(g["y_low"]), T(g["y_high"]))
    else:
        y = T(g["y"])
    trace, state = train_many([m], [x], [y], int(g["steps"]), lr=float(g["lr"]), residual=[res] if res else None, **_kw(route))
    assert state["fused"] is True and state["tree_one_launch"] == ([0] if route == "lds" else [])
    errs = {"trace": rel(trace[0], g["trace"])}
    for i, p in enumerate(m.parameters()):
        errs["final_%d" % i] = rel(p, g["final_%d" % i])
    if res is not None:
        errs["rho"] = rel(res[0], g["rho_final"])
    print(name, route, errs)
    assert max(errs.values()) <= 1e-8, errs


def _companions(seed):
    """a tree-residual member, a plain tree member, a `GP_basic` tree member, a radial plain member and a radial residual member"""
    from test_gpu_train_residual import make_residual
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.cigp_v10 import cigp
    from oracle import gp_oracle as O
    a = make_member(45, 2, 2, LM, "full", seed)
    tree, xs, ys = make_models([(50, 2, 1, ("prod", "ard", "m32"), False)], seed + 1)
    b = make_member(32, 3, 1, LM, "plain", seed + 2, "gpbasic")
    Xp, Yp = O.synthetic_xy(70, 3, 2, seed=seed + 3)
    plain = cigp(kernel.ARDKernel(3), 0.8).double().to(DEV)
    mr, xr, rr = make_residual(64, 2, 1, "matern", "subset", seed + 4)
    return ([a[0], tree[0], b[0], plain, mr], [a[1], xs[0], b[1], T(Xp), xr], [None, ys[0], b[2], T(Yp), None], [a[3], None, None, None, rr])


def _each_as_alone(pick, route, steps=10):
    from fidelityfusion_amd.cigp_v10 import train_many
    sel = lambda t: tuple([v[i] for i in pick] for v in t)
    models, xs, ys, rs = sel(_companions(5))
    trace, state = train_many(models, xs, ys, steps, lr=1e-2, residual=rs, **_kw(route))
    assert state["fused"] is True and state["tree_one_launch"] == ([i for i, q in enumerate(pick) if q < 3] if route == "lds" else [])
    assert bool(torch.isfinite(trace).all())
    solo, xs2, ys2, rs2 = sel(_companions(5))
    for f in range(len(pick)):
        tr, st = train_many([solo[f]], [xs2[f]], [ys2[f]], steps, lr=1e-2, residual=[rs2[f]], **_kw(route))
        assert st["fused"] is True
        assert torch.equal(tr[0], trace[f]), (f, rel(tr[0], trace[f]))
        for a, b in zip(params_of(solo[f], rs2[f][0] if rs2[f] else None), params_of(models[f], rs[f][0] if rs[f] else None)):
            assert np.array_equal(a, b), f


@pytest.mark.parametrize("route", ROUTES)
def test_companions_do_not_matter(route):
    """five kinds of member in ONE train_many call (the three tree members share one ffgp_train_tree_res_raw / ffgp_train_tree_lds_res_raw
    call, the two radial ones the one-launch trainer): each trajectory bit-identical to training that model alone"""
    _each_as_alone([0, 1, 2, 3, 4], route)


@pytest.mark.noisy
def test_companions_do_not_matter_beside_the_load():
    """the three tree members of the call above, beside the background load"""
    _each_as_alone([0, 1, 2], "lds")


@pytest.mark.parametrize("first", ROUTES)
@pytest.mark.parametrize("name", ["n17_D9", "gpbasic_residual"])
def test_state_is_portable_between_the_two_routes(name, first):
    """25 steps on one route, 15 on the other, ONE state, for a residual member (V1 with variances; V2): within the case's bound of the
    40-step loop"""
    from fidelityfusion_amd.cigp_v10 import train_many
    (n, D, d, spec, form, cls), _ = CASES[name]
    second = "stage" if first == "lds" else "lds"
    m, x, y, res = make_member(n, D, d, spec, form, SEED, cls)
    twin, tres = copy.deepcopy(m), clone_residual(res)
    trace, state = train_many([m], [x], [None], STEPS1, lr=LR, residual=[res], **_kw(first))
    assert state["tree_one_launch"] == ([0] if first == "lds" else [])
    trace2, state = train_many([m], [x], [None], STEPS2, lr=LR, residual=[res], state=state, **_kw(second))
    assert state["tree_one_launch"] == ([0] if second == "lds" else [])
    assert len(state["chunks"]) == 1 and state["chunks"][(0,)].step == STEPS1 + STEPS2
    ref, _ = reference_loop(twin, x, None, tres, STEPS1 + STEPS2, LR)
    dist = distance(torch.cat([trace, trace2], dim=1)[0], m, res[0], ref, twin, tres[0])
    print("%s, %s first: %.3g, bound %.3g" % (name, first, dist, bound_of(name)))
    assert dist <= bound_of(name), (dist, bound_of(name))


def test_not_positive_definite_stops_that_member_alone_in_one_launch():
    """one-launch route, three members in one call -- a residual member, a plain tree member, a `GP_basic` tree member -- continued with
    the residual member's first variance not a number: LinAlgError; the failing member's parameters, rho and moments are bit-identical
    to before the call, its companions have completed their steps as in their solo runs, the chunk's step count is not advanced, and
    the next call on the handle works.  (train_many returns no trace when it raises; the NaN trace is checked through the C ABI below.)"""
    from fidelityfusion_amd.cigp_v10 import train_many
    models, xs, ys, rs = (v[:3] for v in _companions(9))
    solo, xs_s, ys_s, rs_s = (v[:3] for v in _companions(9))
    _, state = train_many(models, xs, ys, 2, lr=1e-2, residual=rs, **_kw("lds"))
    assert state["tree_one_launch"] == [0, 1, 2] and state["chunks"][(0, 1, 2)].step == 2
    sst = [train_many([solo[f]], [xs_s[f]], [ys_s[f]], 2, lr=1e-2, residual=[rs_s[f]], **_kw("lds"))[1] for f in (1, 2)]
    mid = params_of(models[0], rs[0][0])
    row = state["chunks"][(0, 1, 2)].buf[0].clone()
    vbad = rs[0][2][1].clone()
    vbad[0, 0] = float("nan")
    bad = [(rs[0][0], rs[0][1], [rs[0][2][0], vbad]), None, None]
    with pytest.raises(torch.linalg.LinAlgError):
        train_many(models, xs, ys, 4, lr=1e-2, residual=bad, state=state, **_kw("lds"))
    assert all(np.array_equal(a, b) for a, b in zip(params_of(models[0], rs[0][0]), mid))
    assert torch.equal(state["chunks"][(0, 1, 2)].buf[0], row) and state["chunks"][(0, 1, 2)].step == 2
    for k, f in enumerate((1, 2)):      # the companions trained on, as alone
        tr, _ = train_many([solo[f]], [xs_s[f]], [ys_s[f]], 4, lr=1e-2, residual=[rs_s[f]], state=sst[k], **_kw("lds"))
        assert bool(torch.isfinite(tr).all())
        for a, b in zip(params_of(solo[f]), params_of(models[f])):
            assert np.array_equal(a, b), f
    trace, state = train_many(models, xs, ys, 1, lr=1e-2, residual=rs, state=state, **_kw("lds"))
    assert bool(torch.isfinite(trace).all())


@pytest.mark.parametrize("n", [30, 150])
def test_not_positive_definite_raises_and_nothing_moves(n):
    """a residual member whose Sigma is not positive definite at step 0 of a continued call: LinAlgError, parameters, rho, moments and
    the step count as before the call, and the handle usable afterwards.  (The diagonal extra of a residual member is |v_high - rho v_low|:
    no finite variance makes it negative, v_high = -3 I included -- so the first pivot is spoilt through a variance that is not a number,
    which the factorisation reports as it reports a negative pivot.  An input the library is specified to survive, not a GPU fault.)"""
    from fidelityfusion_amd.cigp_v10 import train_many
    m, x, _, res = make_member(n, 2, 1, LM, "full", 7)
    _, state = train_many([m], [x], [None], 2, lr=1e-2, residual=[res], fuse_composed=True)
    assert state["fused"] is True and state["chunks"][(0,)].step == 2
    mid = params_of(m, res[0])
    buf = state["chunks"][(0,)].buf.clone()
    vbad = res[2][1].clone()
    vbad[0, 0] = float("nan")
    bad = (res[0], res[1], [res[2][0], vbad])
    with pytest.raises(torch.linalg.LinAlgError):
        train_many([m], [x], [None], 4, lr=1e-2, residual=[bad], state=state, fuse_composed=True)
    assert all(np.array_equal(a, b) for a, b in zip(params_of(m, res[0]), mid))
    assert torch.equal(state["chunks"][(0,)].buf, buf) and state["chunks"][(0,)].step == 2
    trace, state = train_many([m], [x], [None], 1, lr=1e-2, residual=[res], state=state, fuse_composed=True)
    assert bool(torch.isfinite(trace).all()) and state["chunks"][(0,)].step == 3


def test_the_status_is_shared_by_the_call():
    """a residual member and a plain tree member with y_var = -3 I in ONE ffgp_train_tree_res_raw call: LinAlgError, and neither member
    moves -- rho and its moments included (ffgp_train_tree_raw's failure semantics)"""
    from fidelityfusion_amd.cigp_v10 import train_many
    m, x, _, res = make_member(30, 2, 1, LM, "subset", 7)
    tree, xs, ys = make_models([(40, 2, 1, LM, False)], 8)
    models, xs, rs = [m, tree[0]], [x, xs[0]], [res, None]
    _, state = train_many(models, xs, [None, ys[0]], 2, lr=1e-2, residual=rs, fuse_composed=True)
    assert state["fused"] is True and list(state["chunks"]) == [(0, 1)]
    mid = [params_of(m, res[0]), params_of(tree[0])]
    buf = state["chunks"][(0, 1)].buf.clone()
    with pytest.raises(torch.linalg.LinAlgError):
        train_many(models, xs, [None, [ys[0], -3.0 * torch.eye(40, device=DEV)]], 4, lr=1e-2, residual=rs, state=state, fuse_composed=True)
    assert all(np.array_equal(a, b) for a, b in zip(params_of(m, res[0]), mid[0]))
    assert all(np.array_equal(a, b) for a, b in zip(params_of(tree[0]), mid[1]))
    assert torch.equal(state["chunks"][(0, 1)].buf, buf) and state["chunks"][(0, 1)].step == 2
    trace, state = train_many(models, xs, [None, ys[0]], 1, lr=1e-2, residual=rs, state=state, fuse_composed=True)
    assert bool(torch.isfinite(trace).all())


def _abi_case(D):
    """one member through the C entries by ctypes: n = 20 (two 16-row strips, the second padded), d = 1, Sum(Linear with a trained centre,
    leaf 1: Matern 5/2 unless `kfun1` says otherwise), the residual link with variances unless `resid` is off (None: r = NULL).
    -> (call, raw, P): call(**kw) runs 3 Adam steps from zero moments and returns (rc, state, trace); raw: the parameters it moves"""
    from fidelityfusion_amd import _lib
    from fidelityfusion_amd._lib import KDesc, KTree, Problem, Residual, TreeLinks
    n = 20
    rng = np.random.default_rng(2)
    x = T(rng.uniform(0, 1, (n, D)))
    yl = T(np.sin(3 * x.cpu().numpy()[:, :1]))
    yh = 1.2 * yl + 0.1 * T(rng.standard_normal((n, 1)))
    vl, vh = T(rng.uniform(0.01, 0.1, n)), T(rng.uniform(0.01, 0.1, n))
    vnan_t = vh.clone()
    vnan_t[0] = float("nan")
    raw = {k: T(v) for k, v in {"w0": np.linspace(1.0, 1.2, D), "a0": [1.0], "c0": np.linspace(0.1, -0.1, D), "w1": np.linspace(0.9, 1.1, D),
                                "a1": [1.0], "lb": [0.7], "rho": [0.8]}.items()}
    h = _lib.handle(0)
    _lib.bind_stream(h, 0)
    opt = _lib.Adam(1e-2, 0.9, 0.999, 1e-8)
    P = 2 * D + 1 + D + 1 + 1

    def call(kfun1=3, stride=2 * (P + 1), v_high=True, y_low=True, resid=True, variant=1, fn="ffgp_train_tree_res_raw", np_=n, vnan=False):
        arr = (KDesc * 2)()
        for e in range(2):
            arr[e].kfun, arr[e].clamp_min, arr[e].kparam = (5, float("-inf"), 1.0) if e == 0 else (kfun1, 1e-30, 1.0)
            arr[e].w_dev, arr[e].amp_dev = raw["w0" if e == 0 else "w1"].data_ptr(), raw["a0" if e == 0 else "a1"].data_ptr()
        arr[0].center_dev = raw["c0"].data_ptr()
        t = KTree()
        t.n_leaves, t.shape, t.leaf = 2, 0, arr
        p = Problem()
        p.n, p.D, p.d, p.X_dev, p.diag_add_dev = np_, D, 1, x.data_ptr(), raw["lb"].data_ptr()
        p.Y_dev = None if resid else yh.data_ptr()
        p.ll_variant, p.pi_const = variant, 3.1415
        p.tree = C.pointer(t)
        L = TreeLinks()
        for e in range(2):
            L.leaf[e].w_link, L.leaf[e].w_c = (_lib.LINK_INV, 0.0) if e == 0 else (_lib.LINK_INV_ABS_EPS, 1e-9)
            L.leaf[e].amp_link = _lib.LINK_ABS
        L.leaf[0].center_train = 1
        L.dadd_link, L.dadd_c, L.out_scale = _lib.LINK_EXP_NEG, 1e-6, 1.0
        r = Residual()
        if resid:
            r.rho_dev, r.y_high_dev = raw["rho"].data_ptr(), yh.data_ptr()
            r.y_low_dev = yl.data_ptr() if y_low else None
            r.v_low_dev, r.v_low_stride = vl.data_ptr(), 1
            if v_high:
                r.v_high_dev, r.v_high_stride = (vnan_t if vnan else vh).data_ptr(), 1
        state = torch.zeros(2 * (P + 1), device=DEV)
        trace = torch.full((3,), -7.0, device=DEV)
        args = (state.data_ptr(), stride, 0, trace.data_ptr(), 3)
        if fn.endswith("res_raw"):
            rc = getattr(_lib.lib, fn)(h, 1, C.byref(p), C.byref(L), C.byref(r) if resid is not None else None, 3, C.byref(opt), *args)
        else:
            rc = getattr(_lib.lib, fn)(h, 1, C.byref(p), C.byref(L), 3, C.byref(opt), *args)
        torch.cuda.synchronize()
        return rc, state, trace

    return call, raw, P


def test_c_abi_refuses_and_accepts():
    """ffgp_train_tree_res_raw through ctypes: FFGP_ERR_ARG with parameters, rho, state and trace untouched for state_stride = 2 P on a
    residual member, v_low_dev without v_high_dev, an RQ leaf and a residual member without y_low_dev; the accepted call behind them
    runs (P + 1 parameters move), with r = NULL it is ffgp_train_tree_raw, and ffgp_train_tree_lds_raw still refuses V2"""
    from fidelityfusion_amd import _lib
    call, raw, P = _abi_case(2)
    before = {k: v.clone() for k, v in raw.items()}
    LDS = "ffgp_train_tree_lds_res_raw"
    refused = {"lds_short_state_stride": dict(stride=2 * P, fn=LDS), "lds_v_low_without_v_high": dict(v_high=False, fn=LDS),
               "lds_rq_leaf": dict(kfun1=4, fn=LDS), "lds_n_129": dict(np_=129, fn=LDS), "lds_no_y_low": dict(y_low=False, fn=LDS),
               "short_state_stride": dict(stride=2 * P), "v_low_without_v_high": dict(v_high=False), "rq_leaf": dict(kfun1=4),
               "no_y_low": dict(y_low=False), "lds_entry_refuses_v2": dict(resid=False, variant=2, fn="ffgp_train_tree_lds_raw")}
    for name, kw in refused.items():
        rc, state, trace = call(**kw)
        assert rc == _lib.FFGP_ERR_ARG, (name, rc)
        assert float(state.abs().max()) == 0.0 and bool((trace == -7.0).all()), name
        assert all(torch.equal(raw[k], before[k]) for k in raw), name
    for fn in ("ffgp_train_tree_res_raw", LDS):
        for k in raw:
            raw[k].copy_(before[k])
        rc, state, trace = call(fn=fn)
        assert rc == 0 and bool(torch.isfinite(trace).all()), fn
        assert float(state[P].abs()) > 0.0 and float(state[2 * P + 1].abs()) > 0.0, fn      # rho's two moments, at [P] and [2 P + 1]
        assert all(not torch.equal(raw[k], before[k]) for k in raw), fn
    # the one-launch entry on a member that is not positive definite at step 0: its status, NaN in the whole trace, nothing moved
    for k in raw:
        raw[k].copy_(before[k])
    rc, state, trace = call(fn=LDS, vnan=True)
    assert rc > 0 and bool(torch.isnan(trace).all()) and float(state.abs().max()) == 0.0
    assert all(torch.equal(raw[k], before[k]) for k in raw)
    # ... and with r = NULL-like plain members it trains V2, which ffgp_train_tree_lds_raw refuses
    rc, state, trace = call(fn=LDS, resid=False, variant=2)
    assert rc == 0 and bool(torch.isfinite(trace).all()) and float(state.abs().max()) > 0.0
    # a plain member through the new entry (rho_dev NULL) is ffgp_train_tree_raw's member, bit for bit -- V2 too
    for variant in (1, 2):
        outs = []
        for fn in ("ffgp_train_tree_res_raw", "ffgp_train_tree_raw"):
            for k in raw:
                raw[k].copy_(before[k])
            rc, state, trace = call(resid=False, variant=variant, fn=fn)
            assert rc == 0
            outs.append((state.clone(), trace.clone(), {k: v.clone() for k, v in raw.items()}))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        assert all(torch.equal(outs[0][2][k], outs[1][2][k]) for k in raw)
        assert torch.equal(raw["rho"], before["rho"])


@pytest.mark.parametrize("D", [2, 9])
def test_plain_member_through_the_lds_res_entry_is_the_lds_entry_bit_for_bit(D):
    """one step loop (csrc/train_tree_lds.h's ttl_body), two units: a plain V1 member through ffgp_train_tree_lds_res_raw with r = NULL gives
    the state, trace and raw parameters of ffgp_train_tree_lds_raw, bit for bit -- Sum(Linear with a trained centre, Matern 3/2), n = 20,
    d = 1, three Adam steps; D = 2 runs the <8> instantiations, D = 9 the <16> ones"""
    call, raw, P = _abi_case(D)
    before = {k: v.clone() for k, v in raw.items()}
    outs = []
    for fn in ("ffgp_train_tree_lds_res_raw", "ffgp_train_tree_lds_raw"):
        for k in raw:
            raw[k].copy_(before[k])
        rc, state, trace = call(kfun1=2, resid=None, fn=fn)
        assert rc == 0 and bool(torch.isfinite(trace).all()), fn
        outs.append((state.clone(), trace.clone(), {k: v.clone() for k, v in raw.items()}))
    assert all(not torch.equal(outs[1][2][k], before[k]) for k in raw if k != "rho") and float(outs[1][0][:2 * P].abs().max()) > 0.0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert all(torch.equal(outs[0][2][k], outs[1][2][k]) for k in raw)
    assert torch.equal(raw["rho"], before["rho"])
