"""train_many on `GP_basic` models (GaussianProcess/gp_basic.py: Sigma = K + noise_variance^2 I without jitter, the FFGP_LL_V2 likelihood
1/2 (|Sigma^-1 Y|^2 + 2 d sum log L_ii + N d log 2 pi)) -- CAR's blocks.  n <= 128 trains in ONE launch (csrc/train.hip,
tr_body<DM, true, false, true>: ffgp_train_v2_kernel), larger models or option train_persist = 0 on the launch-per-stage loop.

Bars.  V2 squares the condition number, so the bar against the per-step loop is measured, not fixed: two references that do not contain
the fused trainer -- (A) the loop in plain torch on the CPU in fp64, (B) the per-step loop on the GPU through the drop-in module
(`GP_basic.log_likelihood`, autograd, torch.optim.Adam) -- differ by rounding only; d0 = their distance is the yardstick and the fused
trajectory must lie within max(10 d0, 1e-12) of B (the rule of the acquisition tests).  The two fused routes against each other: 1e-11
trace, 1e-10 parameters; a member of a batch against its solo run: 1e-12 (the residual tests' bars)."""
import copy
import math

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


def make_model(n, D, d, kind, seed, noise=0.6):
    from fidelityfusion_amd.gp_basic import GP_basic
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (n, D))
    y = np.sin(3 * x[:, :1] + np.arange(d)) + 0.2 * np.cos(2 * x.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((n, d))
    m = GP_basic(make_kernel(kind, D, rng), noise).double().to(DEV)
    return m, T(x), T(y)


def gpu_loop(m, x, y, steps, lr):
    """(B) train_CAR's fidelity-0 loop (CAR_ContinuousAutoRegression.py:116-125) through the drop-in module"""
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    trace = []
    for _ in range(steps):
        opt.zero_grad()
        loss = (-m.log_likelihood(x, y)).sum()
        loss.backward()
        opt.step()
        trace.append(float(loss.detach()))
    return np.array(trace), params_of(m)


def cpu_loop(m, kind, x, y, steps, lr):
    """(A) the same loop in plain torch on the CPU: kernel, Cholesky, likelihood and autograd in fp64.  The parameters start from
    m's; they are returned in the module's order (noise variance, length scale(s), signal variance)"""
    k = m.kernel
    ls, sv, nv = [torch.nn.Parameter(p.detach().cpu().clone())
                  for p in (k.length_scale if kind == "se" else k.length_scales, k.signal_variance, m.noise_variance)]
    x, y = x.cpu(), y.cpu()
    n, d = y.shape
    opt = torch.optim.Adam([ls, sv, nv], lr=lr)
    trace = []
    for _ in range(steps):
        opt.zero_grad()
        if kind == "se":
            w, amp = torch.exp(-ls), sv.exp().pow(2)
        else:
            w, amp = 1.0 / (ls.abs() + m.kernel.eps), sv.abs()
        df = (x[:, None, :] - x[None, :, :]) * w
        sq = (df * df).sum(-1)
        if kind != "se":
            sq = sq.clamp_min(1e-30)
        if kind == "matern":
            r5 = (5.0 * sq).sqrt()
            K = amp * (1.0 + r5 + 5.0 / 3.0 * sq) * torch.exp(-r5)
        else:
            K = amp * torch.exp(-0.5 * sq)
        L = torch.linalg.cholesky(K + nv.pow(2) * torch.eye(n))
        A = torch.cholesky_solve(y, L)
        loss = 0.5 * ((A * A).sum() + 2.0 * d * L.diagonal().log().sum() + n * d * math.log(2.0 * math.pi))
        loss.backward()
        opt.step()
        trace.append(float(loss.detach()))
    return np.array(trace), [p.detach().numpy().copy() for p in (nv, ls, sv)]


def distance(a, b):
    """largest relative difference of two runs (trace, parameters)"""
    return max([rel(a[0], b[0])] + [rel(p, q) for p, q in zip(a[1], b[1])])


CASES = [(1, 1, 1, "ard"), (16, 1, 1, "ard"), (17, 9, 3, "se"), (33, 2, 1, "matern"), (100, 16, 16, "matern"), (128, 16, 3, "ard"),
         (129, 2, 1, "ard"), (300, 1, 1, "ard")]


@pytest.mark.parametrize("n,D,d,kind", CASES)
def test_train_many_gp_basic_follows_the_per_step_loop(n, D, d, kind):
    from fidelityfusion_amd.gp_basic import train_many
    lr = 1e-2
    m, x, y = make_model(n, D, d, kind, 100 * n + D)
    twin = copy.deepcopy(m)
    A = cpu_loop(m, kind, x, y, 40, lr)
    trace, state = train_many([m], [x], [y], 25, lr=lr)
    assert state["fused"] is True
    trace2, state = train_many([m], [x], [y], 15, lr=lr, state=state)
    B = gpu_loop(twin, x, y, 40, lr)
    Fz = (torch.cat([trace, trace2], dim=1).cpu().numpy()[0], params_of(m))
    assert np.isfinite(Fz[0]).all()
    d0 = distance(B, A)
    bound = max(10.0 * d0, 1e-12)
    print("gp_basic n=%d D=%d d=%d %s: d0 %.2e, bound %.2e, fused vs B %.2e, vs A %.2e" % (n, D, d, kind, d0, bound, distance(Fz, B),
                                                                                         distance(Fz, A)))
    assert d0 <= 1e-8, "the two reference loops disagree beyond rounding: d0 = %.2e" % d0      # (both are fp64: a yardstick, not a licence)
    assert distance(Fz, B) <= bound, (distance(Fz, B), bound)


@pytest.mark.parametrize("n,D,d,kind", [(33, 2, 1, "matern"), (100, 16, 16, "matern"), (128, 16, 3, "ard")])
def test_one_launch_v2_trainer_is_the_launch_per_stage_trainer(n, D, d, kind):
    from fidelityfusion_amd import _lib
    from fidelityfusion_amd.gp_basic import train_many
    runs = {}
    for persist in (1, 0):
        m, x, y = make_model(n, D, d, kind, 7 * n + d)
        _lib.set_option("train_persist", persist, 0)
        try:
            tr1, state = train_many([m], [x], [y], 25, lr=2e-2)
            tr2, _ = train_many([m], [x], [y], 15, lr=2e-2, state=state)
        finally:
            _lib.set_option("train_persist", 1, 0)
        runs[persist] = (torch.cat([tr1, tr2], dim=1).clone(), params_of(m))
    print("v2 one launch vs per stage n=%d: trace %.2e, parameters %.2e" % (
        n, rel(runs[1][0], runs[0][0]), max(rel(a, b) for a, b in zip(runs[1][1], runs[0][1]))))
    assert rel(runs[1][0], runs[0][0]) < 1e-11, rel(runs[1][0], runs[0][0])
    for a, b in zip(runs[1][1], runs[0][1]):
        assert rel(a, b) < 1e-10, (a, b)


def _mixed(seed):
    """cigp (V1) and GP_basic (V2) models in one list: the four small ones share a call (two launches: one per likelihood), the two
    larger ones get calls of their own"""
    from fidelityfusion_amd.cigp_v10 import cigp
    rng = np.random.default_rng(seed)
    models, xs, ys = [], [], []
    for f, (n, D, d, kind, v2) in enumerate([(60, 3, 1, "ard", True), (45, 2, 1, "se", False), (128, 5, 2, "matern", True),
                                             (24, 9, 3, "matern", False), (180, 2, 1, "ard", True), (200, 3, 1, "ard", False)]):
        m, x, y = make_model(n, D, d, kind, seed + f)
        if not v2:
            m = cigp(make_kernel(kind, D, rng), 0.7).double().to(DEV)
        models.append(m)
        xs.append(x)
        ys.append(y)
    return models, xs, ys


def test_train_many_mixes_v1_and_v2_models():
    from fidelityfusion_amd.gp_basic import train_many
    models, xs, ys = _mixed(5)
    trace, state = train_many(models, xs, ys, 12)
    assert state["fused"] is True
    solo_m, solo_x, solo_y = _mixed(5)
    for f in range(len(models)):
        tf, _ = train_many([solo_m[f]], [solo_x[f]], [solo_y[f]], 12)
        assert rel(trace[f], tf[0]) < 1e-12, f
        for a, b in zip(params_of(models[f]), params_of(solo_m[f])):
            assert rel(a, b) < 1e-12, f


def test_train_many_gp_basic_members_survive_a_failing_one():
    """signal_variance = 0 and noise_variance = 0: Sigma is exactly zero, its first pivot is not positive"""
    from fidelityfusion_amd.gp_basic import train_many
    models, xs, ys = _mixed(9)
    with torch.no_grad():
        models[0].kernel.signal_variance.zero_()
        models[0].noise_variance.zero_()
    before = params_of(models[0])
    with pytest.raises(torch.linalg.LinAlgError):
        train_many(models, xs, ys, 6)
    for a, b in zip(params_of(models[0]), before):
        assert np.array_equal(a, b)
    solo_m, solo_x, solo_y = _mixed(9)
    for f in range(1, len(models)):
        train_many([solo_m[f]], [solo_x[f]], [solo_y[f]], 6)
        for a, b in zip(params_of(models[f]), params_of(solo_m[f])):
            assert rel(a, b) < 1e-12, f
