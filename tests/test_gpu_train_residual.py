"""train_many(..., residual=): train_AR's residual fidelities (FidelityFusion_Models/AR_autoRegression.py:123-137) -- targets
y_high - rho * y_low and, in the non-subset form, the y_var |v_high - rho * v_low| re-formed at every step, rho a fourth Adam parameter --
against the reference's own loop (drop-in modules, torch.optim.Adam over the GP parameters and rho, the residual recomputed every step)
and against the reference-generated fixture tests/golden/ar_chain.npz.  n <= 128 trains in ONE launch (csrc/train.hip, tr_body<DM, true,
true>), larger models or option train_persist = 0 on the launch-per-stage loop of ffgp_train_residual_raw."""
import copy

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


def params_of(m, rho=None):
    out = [p.detach().cpu().numpy().copy() for p in m.parameters()]
    return out + ([rho.detach().cpu().numpy().copy()] if rho is not None else [])


def make_kernel(kind, D, rng):
    from fidelityfusion_amd import kernel
    if kind == "ard":
        k = kernel.ARDKernel(D)
        with torch.no_grad():
            k.length_scales.copy_(torch.tensor(rng.uniform(0.6, 1.6, D) * rng.choice([-1.0, 1.0], D)))
        return k
    if kind == "se":
        return kernel.SquaredExponentialKernel(0.3, 0.2)
    return kernel.MaternKernel(D, nu=2.5)


def make_residual(n, D, d, kind, form, seed, rho0=0.8):
    """one residual fidelity: model, x, (rho, y_low, y_high).  Non-subset form: diagonal variances with s_i = v_high - rho v_low
    positive, negative and exactly zero (v_high = rho0 * v_low, v_low an exact power of two: zero at the first step's rho)"""
    from fidelityfusion_amd.cigp_v10 import cigp
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (n, D))
    yl = np.sin(3 * x[:, :1] + np.arange(d)) + 0.1 * rng.standard_normal((n, d))
    yh = 1.3 * yl + 0.2 * np.cos(2 * x[:, :1]) + 0.05 * rng.standard_normal((n, d))
    m = cigp(make_kernel(kind, D, rng), 0.6).double().to(DEV)
    rho = torch.nn.Parameter(torch.tensor(rho0, dtype=torch.float64, device=DEV))
    if form == "subset":
        return m, T(x), (rho, T(yl), T(yh))
    vl = rng.uniform(0.01, 0.2, n)
    vh = rng.uniform(0.01, 0.3, n)
    k = np.arange(n)
    vh[k % 3 == 1] = 0.0                                # s < 0
    vl[k % 5 == 2] = 0.0                                # no rho dependence: sgn term vanishes
    vl[k % 7 == 3], vh[k % 7 == 3] = 0.125, rho0 * 0.125   # s == 0 at the first step (sgn(0) = 0)
    return m, T(x), (rho, [T(yl), torch.diag(T(vl))], [T(yh), torch.diag(T(vh))])


def clone_residual(res):
    rho, yl, yh = res
    r2 = torch.nn.Parameter(rho.detach().clone())
    return (r2, yl, yh)


def reference_ar_loop(m, x, res, steps, lr, opt=None):
    """train_AR's loop (AR_autoRegression.py:123-137) through the drop-in modules: Adam over the GP parameters and rho"""
    rho, yl, yh = res
    opt = opt or torch.optim.Adam(list(m.parameters()) + [rho], lr=lr)
    trace, last = [], None
    for k in range(steps):
        opt.zero_grad()
        if isinstance(yl, list):
            y = [yh[0] - rho * yl[0], (yh[1] - rho * yl[1]).abs()]
        else:
            y = yh - rho * yl
        last = y
        loss = -m.negative_log_likelihood(x, y)
        loss.backward()
        opt.step()
        trace.append(float(loss.detach()))
    return np.array(trace), opt, last


def test_train_many_residual_on_the_reference_fixture(golden):
    """tests/golden/ar_chain.npz (the reference's train_AR, non-subset, N = 45, 5 steps per fidelity): fidelity 0 plain, fidelity 1 with
    residual= -- the losses, parameters (rho included) and AR.forward on state["residual_targets"] at test_ar_nar_chain_golden's bars"""
    import mf_harness as H
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.cigp_v10 import train_many
    g = golden("ar_chain")
    model = H.AR(2, [kernel.SquaredExponentialKernel() for _ in range(2)], rho_init=1.0).double().to(DEV)
    x0, y0 = T(g["x0n"]), T(g["y0n"])
    tr0, _ = train_many([model.gpr_list[0]], [x0], [y0], 5, lr=1e-2)
    xf = T(g["fill_x"])
    res = (model.rho_list[0], [T(g["fill_ylow_mean"]), T(g["fill_ylow_var"])], [T(g["fill_yhigh_mean"]), T(g["fill_yhigh_var"])])
    tr1, st = train_many([model.gpr_list[1]], [xf], [None], 5, lr=1e-2, residual=[res])
    assert rel(-torch.cat([tr0[0], tr1[0]]), g["ll_trace"]) < 1e-8
    for name, p in model.state_dict().items():
        assert rel(p, g[name.replace(".", "__")]) < 1e-7, name
    data = [(x0, y0), (xf, st["residual_targets"][0])]
    with torch.no_grad():
        yp, vp = model(data, T(g["xtn"]))
    assert rel(yp, g["ypred"]) < 1e-7 and rel(vp, g["var_pred"]) < 1e-7


CASES = [
    (1, 1, 1, "ard", "full"), (4, 2, 1, "ard", "subset"), (17, 9, 3, "se", "full"), (32, 2, 1, "ard", "full"),
    (100, 16, 16, "matern", "subset"), (128, 16, 3, "ard", "full"), (128, 2, 1, "matern", "full"),
    (129, 2, 1, "ard", "full"), (300, 9, 3, "se", "subset"), (300, 1, 1, "matern", "full"),
]


@pytest.mark.parametrize("n,D,d,kind,form", CASES)
def test_train_many_residual_follows_the_reference_loop(n, D, d, kind, form):
    from fidelityfusion_amd.cigp_v10 import train_many
    lr = 1e-2
    m, x, res = make_residual(n, D, d, kind, form, 100 * n + D)
    twin, tres = copy.deepcopy(m), clone_residual(res)
    trace, state = train_many([m], [x], [None], 25, lr=lr, residual=[res])
    trace2, state = train_many([m], [x], [None], 15, lr=lr, state=state, residual=[res])
    ref, _, last = reference_ar_loop(twin, x, tres, 40, lr)
    assert torch.isfinite(trace).all() and torch.isfinite(trace2).all()
    assert rel(torch.cat([trace, trace2], dim=1), ref) < 1e-11, rel(torch.cat([trace, trace2], dim=1), ref)
    for a, b in zip(params_of(m, res[0]), params_of(twin, tres[0])):
        assert rel(a, b) < 1e-10, (a, b)
    got = state["residual_targets"][0]
    want = last if isinstance(last, list) else [last, None]
    assert rel(got[0], want[0]) < 1e-12
    if want[1] is None:
        assert got[1] is None
    else:
        assert rel(got[1], want[1]) < 1e-12


@pytest.mark.parametrize("n,D,d,kind,form", [(32, 2, 1, "ard", "full"), (100, 9, 3, "matern", "subset"), (128, 16, 16, "ard", "full")])
def test_one_launch_residual_trainer_is_the_launch_per_stage_trainer(n, D, d, kind, form):
    from fidelityfusion_amd import _lib
    from fidelityfusion_amd.cigp_v10 import train_many
    runs = {}
    for persist in (1, 0):
        m, x, res = make_residual(n, D, d, kind, form, 7 * n + d)
        _lib.set_option("train_persist", persist, 0)
        try:
            tr1, state = train_many([m], [x], [None], 30, lr=2e-2, residual=[res])
            tr2, _ = train_many([m], [x], [None], 7, lr=2e-2, state=state, residual=[res])
        finally:
            _lib.set_option("train_persist", 1, 0)
        runs[persist] = (torch.cat([tr1, tr2], dim=1).clone(), params_of(m, res[0]))
    assert rel(runs[1][0], runs[0][0]) < 1e-11, rel(runs[1][0], runs[0][0])
    for a, b in zip(runs[1][1], runs[0][1]):
        assert rel(a, b) < 1e-10, (a, b)


def _mixed(seed):
    """plain and residual models of several sizes: three small ones share a launch, two larger ones get calls of their own"""
    from fidelityfusion_amd.cigp_v10 import cigp
    from oracle import gp_oracle as O
    rng = np.random.default_rng(seed)
    models, xs, ys, res = [], [], [], []
    for f, (n, D, d, kind, form) in enumerate([(60, 3, 1, "ard", None), (45, 2, 1, "se", "full"), (128, 5, 2, "matern", "subset"),
                                                (180, 2, 1, "ard", "full"), (200, 3, 1, "ard", None)]):
        if form is None:
            X, Y = O.synthetic_xy(n, D, d, seed=seed + f)
            models.append(cigp(make_kernel(kind, D, rng), 0.7).double().to(DEV))
            xs.append(T(X))
            ys.append(T(Y))
            res.append(None)
        else:
            m, x, r = make_residual(n, D, d, kind, form, seed + f)
            models.append(m)
            xs.append(x)
            ys.append(None)
            res.append(r)
    return models, xs, ys, res


def test_train_many_mixes_plain_and_residual_models():
    from fidelityfusion_amd.cigp_v10 import train_many
    models, xs, ys, res = _mixed(5)
    trace, _ = train_many(models, xs, ys, 12, residual=res)
    solo_m, solo_x, solo_y, solo_r = _mixed(5)
    for f in range(len(models)):
        tf, _ = train_many([solo_m[f]], [solo_x[f]], [solo_y[f]], 12, residual=[solo_r[f]])
        assert rel(trace[f], tf[0]) < 1e-12
        rho_a = res[f][0] if res[f] is not None else None
        rho_b = solo_r[f][0] if solo_r[f] is not None else None
        for a, b in zip(params_of(models[f], rho_a), params_of(solo_m[f], rho_b)):
            assert rel(a, b) < 1e-12


def test_train_many_residual_exp_aligned_sweep_in_one_call():
    """Experiments/GAR_Aligned/exp_aligned.py:56-102's AR fidelity 1: N_high 4/8/16/32, D = 2, d = 1, 5 seeds -- 20 models, two chunks of
    one launch each -- against each model's reference loop"""
    from fidelityfusion_amd.cigp_v10 import train_many
    items = [make_residual(nh, 2, 1, "se", "full", 1000 * seed + nh) for seed in range(5) for nh in (4, 8, 16, 32)]
    twins = [(copy.deepcopy(m), x, clone_residual(r)) for m, x, r in items]
    trace, _ = train_many([m for m, _, _ in items], [x for _, x, _ in items], [None] * 20, 30, residual=[r for _, _, r in items])
    for f, (m, x, r) in enumerate(twins):
        ref, _, _ = reference_ar_loop(m, x, r, 30, 1e-2)
        assert rel(trace[f], ref) < 1e-11, f
        for a, b in zip(params_of(items[f][0], items[f][2][0]), params_of(m, r[0])):
            assert rel(a, b) < 1e-10


def test_train_many_residual_members_survive_a_failing_plain_model():
    from fidelityfusion_amd.cigp_v10 import train_many
    models, xs, ys, res = _mixed(9)
    before = params_of(models[0])
    bad = [ys[0], -3.0 * torch.eye(xs[0].shape[0], device=DEV, dtype=torch.float64)]
    with pytest.raises(torch.linalg.LinAlgError):
        train_many(models, xs, [bad] + ys[1:], 6, residual=res)
    for a, b in zip(params_of(models[0]), before):
        assert np.array_equal(a, b)
    solo_m, solo_x, solo_y, solo_r = _mixed(9)
    for f in (1, 2, 3):
        train_many([solo_m[f]], [solo_x[f]], [None], 6, residual=[solo_r[f]])
        for a, b in zip(params_of(models[f], res[f][0]), params_of(solo_m[f], solo_r[f][0])):
            assert rel(a, b) < 1e-12


def test_train_many_residual_runs_the_reference_loop_when_it_cannot_fuse():
    """a CPU-resident residual model is not eligible: train_many is then train_AR's loop itself, residual_targets included"""
    from fidelityfusion_amd.cigp_v10 import train_many
    m, x, res = make_residual(20, 2, 1, "ard", "full", 3)
    m = m.cpu()
    x = x.cpu()
    rho = torch.nn.Parameter(res[0].detach().cpu())
    res = (rho, [t.cpu() for t in res[1]], [t.cpu() for t in res[2]])
    twin, tres = copy.deepcopy(m), clone_residual(res)
    trace, state = train_many([m], [x], [None], 6, residual=[res])
    ref, _, last = reference_ar_loop(twin, x, tres, 6, 1e-2)
    assert state["fused"] is False and rel(trace, ref) < 1e-12
    assert rel(rho, tres[0]) < 1e-12
    assert rel(state["residual_targets"][0][0], last[0]) == 0.0 and rel(state["residual_targets"][0][1], last[1]) == 0.0
