"""train_many(..., car=): train_CAR's fidelities above 0 (FidelityFusion_Models/CAR_ContinuousAutoRegression.py:116-142) -- a `GP_basic`
over `kernel.FidelityKernelMCMC`, targets y_high - exp(b) * y_low and the Monte-Carlo scalar s(b, l_z, sigma_z) re-formed at every step,
six groups of parameters under Adam -- against the reference-generated fixture tests/golden/car_chain.npz and against the per-step loop
(drop-in modules, autograd through the module's torch `scale()`, torch.optim.Adam).  n <= 128 trains in ONE launch (csrc/train.hip,
ffgp_train_car_kernel), larger models or option train_persist = 0 on the launch-per-stage loop of ffgp_train_car_raw.

Bars.  The fixture: test_car_chain_golden's (LL trace 1e-8, parameters 1e-7).  Against the per-step loop the bar is measured: the
reference evaluates -b * (z - hf) in binary32 (its samples are fp32 draws under torch's default dtype), and the noise that step injects
is the distance d0 between the per-step loop as it stands and the same loop with the samples widened to fp64 first; the fused trajectory
must lie within max(10 d0, 1e-12) of the per-step loop.  These cases run under the default dtype float32 (fp32 draws, as the reference's
demo has them) with every tensor explicitly fp64; the fixture was generated under default float64, where torch.rand draws fp64 numbers
(ffgp_car_link.z1d_dev / z2d_dev).  The two fused routes against each other: 1e-11 trace, 1e-10 parameters; a member of a batch
against its solo run: 1e-12 (the residual tests' bars)."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield


@pytest.fixture()
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


DEV = "cuda:0"


def T(a, dev=DEV):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device=dev)


def rel(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    return float(np.abs(a.reshape(b.shape) - b).max() / max(np.abs(b).max(), 1e-300))


def params_of(m):
    return [p.detach().cpu().numpy().copy() for p in m.parameters()]


def distance(a, b):
    return max([rel(a[0], b[0])] + [rel(p, q) for p, q in zip(a[1], b[1])])


def make_car(n, D, d, kind, seed, neg=False, b0=1.0, dev=DEV):
    """one CAR fidelity: model (GP_basic over FidelityKernelMCMC(input_dim = 1) over an ARD / Matern base kernel on D inputs), x,
    (b, y_low, y_high).  neg: raw l_z and sigma_z negative (the sgn branches)"""
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.gp_basic import GP_basic
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (n, D))
    yl = np.sin(3 * x[:, :1] + np.arange(d)) + 0.1 * rng.standard_normal((n, d))
    yh = 1.3 * yl + 0.2 * np.cos(2 * x[:, :1]) + 0.05 * rng.standard_normal((n, d))
    if kind == "ard":
        base = kernel.ARDKernel(D)
        with torch.no_grad():
            base.length_scales.copy_(torch.tensor(rng.uniform(0.6, 1.6, D) * rng.choice([-1.0, 1.0], D)))
    else:
        base = kernel.MaternKernel(D, nu=2.5)
    b = torch.nn.Parameter(torch.tensor(b0, dtype=torch.float64))
    k = kernel.FidelityKernelMCMC(1, base, 0, 1, b, initial_length_scale=-0.8 if neg else 0.9, initial_signal_variance=-1.2 if neg else 1.1)
    m = GP_basic(k, 0.6).double().to(dev)
    assert m.kernel.b is b and b.dtype == torch.float64
    return m, T(x, dev), (b, T(yl, dev), T(yh, dev))


def car_loop(m, x, car, steps, lr, widen=False):
    """train_CAR's loop (CAR_ContinuousAutoRegression.py:130-139) through the drop-in modules: Adam over the model's parameters (b is one
    of them), the residual re-formed with its graph at every step.  widen: the samples widened to fp64 before anything is computed from
    them (then nothing in `scale()` is binary32)"""
    b, yl, yh = car
    if widen:
        draw = m.kernel.samples
        m.kernel.samples = lambda: tuple(z.double() for z in draw())
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    trace, last = [], None
    for _ in range(steps):
        opt.zero_grad()
        last = yh - b.exp() * yl
        loss = (-m.log_likelihood(x, last)).sum()
        loss.backward()
        opt.step()
        trace.append(float(loss.detach()))
    return np.array(trace), params_of(m), last.detach()


class _Chain(torch.nn.Module):
    """ContinuousAutoRegression's parameters under the reference's names (b, cigp_list.f. ...), on the library's own fidelity kernel"""

    def __init__(self, fidelity_num):
        super().__init__()
        from fidelityfusion_amd import kernel
        from fidelityfusion_amd.gp_basic import GP_basic
        self.b = torch.nn.Parameter(torch.tensor(1.0))
        blocks = [GP_basic(kernel.ARDKernel(1), 1.0)]
        for f in range(fidelity_num - 1):
            blocks.append(GP_basic(kernel.FidelityKernelMCMC(1, kernel.ARDKernel(1), f, f + 1, self.b), 1.0))
        self.cigp_list = torch.nn.ModuleList(blocks)


def test_train_many_car_on_the_reference_fixture(golden, f64):
    """tests/golden/car_chain.npz (the reference's train_CAR, 3 fidelities x 4 steps, lr 1e-2): fidelity 0 plain, fidelities 1 and 2 with
    car=, a fresh state each -- LL trace and parameters at test_car_chain_golden's bars"""
    from fidelityfusion_amd.gp_basic import train_many
    g = golden("car_chain")
    model = _Chain(3).double().to(DEV)
    tr0, st = train_many([model.cigp_list[0]], [T(g["x0"])], [T(g["y0"])], 4, lr=1e-2)
    assert st["fused"] is True
    traces = [tr0[0]]
    for i in (1, 2):
        car = (model.b, T(g[f"ov{i}_ylow"]), T(g[f"ov{i}_yhigh"]))
        tr, st = train_many([model.cigp_list[i]], [T(g[f"ov{i}_x"])], [None], 4, lr=1e-2, car=[car])
        assert st["fused"] is True
        traces.append(tr[0])
    print("car_chain: LL trace %.2e" % rel(-torch.cat(traces), g["ll_trace"]))
    assert rel(-torch.cat(traces), g["ll_trace"]) < 1e-8
    for name, p in model.state_dict().items():
        print("car_chain: %s %.2e" % (name, rel(p, g[name.replace(".", "__")])))
        assert rel(p, g[name.replace(".", "__")]) < 1e-7, name


CASES = [(4, 1, 1, "ard", False, 1.0), (17, 1, 3, "matern", True, -0.4), (32, 1, 1, "ard", True, 1.0), (33, 3, 1, "matern", False, -0.4),
         (128, 1, 16, "ard", False, -0.4), (129, 1, 1, "matern", True, 1.0), (300, 1, 1, "ard", True, -0.4), (250, 1, 2, "matern", False, 1.0)]


@pytest.mark.parametrize("n,D,d,kind,neg,b0", CASES)
def test_train_many_car_follows_the_per_step_loop(n, D, d, kind, neg, b0):
    from fidelityfusion_amd.gp_basic import train_many
    lr = 1e-2
    m, x, car = make_car(n, D, d, kind, 100 * n + D, neg, b0)
    twin, wide = copy.deepcopy(m), copy.deepcopy(m)
    tcar, wcar = (twin.kernel.b, car[1], car[2]), (wide.kernel.b, car[1], car[2])
    trace, state = train_many([m], [x], [None], 25, lr=lr, car=[car])
    assert state["fused"] is True
    trace2, state = train_many([m], [x], [None], 15, lr=lr, state=state, car=[car])
    B = car_loop(twin, x, tcar, 40, lr)
    W = car_loop(wide, x, wcar, 40, lr, widen=True)
    Fz = (torch.cat([trace, trace2], dim=1).cpu().numpy()[0], params_of(m))
    assert np.isfinite(Fz[0]).all()
    d0 = distance(B, W)
    bound = max(10.0 * d0, 1e-12)
    print("car n=%d D=%d d=%d %s neg=%s b=%.1f: d0 %.2e, bound %.2e, fused vs loop %.2e, vs widened loop %.2e" % (
        n, D, d, kind, neg, b0, d0, bound, distance(Fz, B), distance(Fz, W)))
    assert d0 <= 1e-6, "the two reference loops disagree beyond rounding: d0 = %.2e" % d0      # (binary32 against fp64: 6e-8 per operation)
    assert distance(Fz, B) <= bound, (distance(Fz, B), bound)
    # the fidelity's data, y_high - exp(b) y_low at the b of the start of the last step: b lies within `bound` of the loop's, and the
    # residual's largest entry is no smaller than a tenth of exp(b) |y_low| here, so ten times the bound
    assert rel(state["residual_targets"][0][0], B[2]) <= 10.0 * bound and state["residual_targets"][0][1] is None


@pytest.mark.parametrize("n,D,d,kind,neg,b0", [(32, 1, 1, "ard", True, 1.0), (100, 3, 3, "matern", False, -0.4), (128, 1, 16, "ard", False, -0.4)])
def test_one_launch_car_trainer_is_the_launch_per_stage_trainer(n, D, d, kind, neg, b0):
    from fidelityfusion_amd import _lib
    from fidelityfusion_amd.gp_basic import train_many
    runs = {}
    for persist in (1, 0):
        m, x, car = make_car(n, D, d, kind, 7 * n + d, neg, b0)
        _lib.set_option("train_persist", persist, 0)
        try:
            tr1, state = train_many([m], [x], [None], 25, lr=2e-2, car=[car])
            tr2, _ = train_many([m], [x], [None], 15, lr=2e-2, state=state, car=[car])
        finally:
            _lib.set_option("train_persist", 1, 0)
        runs[persist] = (torch.cat([tr1, tr2], dim=1).clone(), params_of(m))
    print("car one launch vs per stage n=%d: trace %.2e, parameters %.2e" % (
        n, rel(runs[1][0], runs[0][0]), max(rel(a, b) for a, b in zip(runs[1][1], runs[0][1]))))
    assert rel(runs[1][0], runs[0][0]) < 1e-11, rel(runs[1][0], runs[0][0])
    for a, b in zip(runs[1][1], runs[0][1]):
        assert rel(a, b) < 1e-10, (a, b)


def _sixteen():
    return [make_car(24, 1 + f % 3, 1 + f % 2, "ard" if f % 2 else "matern", 500 + f, f % 4 >= 2, 1.0 if f % 3 else -0.4) for f in range(16)]


def test_sixteen_car_members_in_one_call():
    from fidelityfusion_amd.gp_basic import train_many
    items, solo = _sixteen(), _sixteen()
    trace, state = train_many([m for m, _, _ in items], [x for _, x, _ in items], [None] * 16, 40, car=[c for _, _, c in items])
    assert state["fused"] is True
    for f, (m, x, c) in enumerate(solo):
        tf, _ = train_many([m], [x], [None], 40, car=[c])
        assert rel(trace[f], tf[0]) < 1e-12, f
        for a, b in zip(params_of(items[f][0]), params_of(m)):
            assert rel(a, b) < 1e-12, f


def _beside(seed):
    """two small CAR members, a small plain GP_basic, a larger CAR member"""
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.gp_basic import GP_basic
    rng = np.random.default_rng(seed)
    cars = [make_car(40, 2, 1, "ard", seed + 1), make_car(64, 1, 2, "matern", seed + 2, True, -0.4), make_car(150, 1, 1, "ard", seed + 3)]
    xp = rng.uniform(0, 1, (30, 2))
    plain = GP_basic(kernel.ARDKernel(2), 0.5).double().to(DEV)
    models = [cars[0][0], plain, cars[1][0], cars[2][0]]
    xs = [cars[0][1], T(xp), cars[1][1], cars[2][1]]
    ys = [None, T(np.sin(xp.sum(1, keepdims=True))), None, None]
    return models, xs, ys, [cars[0][2], None, cars[1][2], cars[2][2]]


def test_car_members_survive_a_failing_plain_model():
    """signal_variance = 0 and noise_variance = 0 make the plain model's Sigma exactly zero: its first pivot is not positive"""
    from fidelityfusion_amd.gp_basic import train_many
    models, xs, ys, car = _beside(9)
    with torch.no_grad():
        models[1].kernel.signal_variance.zero_()
        models[1].noise_variance.zero_()
    before = params_of(models[1])
    with pytest.raises(torch.linalg.LinAlgError):
        train_many(models, xs, ys, 6, car=car)
    for a, b in zip(params_of(models[1]), before):
        assert np.array_equal(a, b)
    solo_m, solo_x, solo_y, solo_c = _beside(9)
    for f in (0, 2, 3):
        train_many([solo_m[f]], [solo_x[f]], [None], 6, car=[solo_c[f]])
        for a, b in zip(params_of(models[f]), params_of(solo_m[f])):
            assert rel(a, b) < 1e-12, f


def test_train_many_car_runs_the_reference_loop_when_it_cannot_fuse():
    """a CPU-resident CAR model is not eligible: train_many is then train_CAR's loop itself, residual_targets included"""
    from fidelityfusion_amd.gp_basic import train_many
    m, x, car = make_car(20, 1, 1, "ard", 3, dev="cpu")
    twin = copy.deepcopy(m)
    trace, state = train_many([m], [x], [None], 6, car=[car])
    ref = car_loop(twin, x, (twin.kernel.b, car[1], car[2]), 6, 1e-2)
    assert state["fused"] is False and rel(trace, ref[0]) < 1e-12
    for a, b in zip(params_of(m), ref[1]):
        assert rel(a, b) < 1e-12
    assert rel(state["residual_targets"][0][0], ref[2]) == 0.0 and state["residual_targets"][0][1] is None
