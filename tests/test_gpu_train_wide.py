"""train_many(..., wide_one_launch=True): single-kernel `cigp` models of at most 128 points with MORE than 16 target columns trained
by ffgp_train_wide_raw -- ONE launch for all their steps, a persistent workgroup per model that streams 16-column blocks of the
COMPRESSED targets (train.compress_targets) through the step (csrc/train_wide.hip) -- against the per-step loop through the drop-in
modules with torch.optim.Adam, the launch-per-stage call these models take without the keyword, a fixture of the reference's own
loop, and itself (each model as alone, bit for bit).  Every test asserts through state["wide_one_launch"] that the models it meant to
send to the new kernel went there.

The trajectory bound is this project's rule (head of test_gpu_train_tree.py): max(10 x d0, 1e-12), d0 = the distance between two
per-step loops that differ only by rounding -- here the per-step loop on the FULL targets against the per-step loop on the
COMPRESSED ones (`loop_yardstick`: the compressed loop adds the likelihood of d - r zero columns, which is exactly the
(d - r) (sum log L_ii + n / 2 log 2 pi) the compressed columns lack) -- measured on an MI355X with this file's metric and written
into the case table.  A case whose 10 x d0 exceeded 1e-9 would be ill-conditioned and would be replaced, not loosened.  Measured d0
and the trainer's own distance per case: DESIGN.md section 4.8."""
import copy
import ctypes as C

import numpy as np
import pytest

from test_gpu_train_residual import clone_residual, make_kernel, make_residual, reference_ar_loop
from test_gpu_train_tree import DEV, T, params_of, rel

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

STEPS, LR = 25, 1e-2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(torch.float32)


# name -> ((n, D, d, kernel, with y_var | residual form), r = the compressed columns, d0 measured on an MI355X by loop_yardstick)
PLAIN = {
    "n4_d17": ((4, 1, 17, "ard", False), 4, 1.43e-16),            # one partial column block; the true d differs from the columns passed
    "n17_d40": ((17, 2, 40, "se", False), 17, 1.60e-15),          # two factor stages; the second column block holds one column
    "n33_d1024": ((33, 3, 1024, "ard", False), 33, 4.88e-16),     # ARD, three column blocks
    "n128_d300": ((128, 16, 300, "matern", False), 128, 2.58e-16),   # Matern 5/2, the <16> instantiation, 8 full blocks, all 36 tiles
    "n128_d24": ((128, 5, 24, "ard", False), 24, 0.0),        # pass-through: r = d, two blocks (the two loops are one: d0 = 0)
    "n20_d64_yvar": ((20, 2, 64, "ard", True), 20, 3.63e-16),     # a [y, y_var] member: diag_vec
}
RESIDUAL = {
    "res_n20_d64": ((20, 2, 64, "ard", "subset"), 40, 3.33e-16),
    "res_n20_d64_var": ((20, 2, 64, "matern", "full"), 40, 6.23e-16),       # [n, n] variances
    "res_n128_d600": ((128, 8, 600, "ard", "subset"), 256, 3.41e-16),       # 16 column blocks
}


def make_plain(case, seed=11):
    from fidelityfusion_amd.cigp_v10 import cigp
    from oracle import gp_oracle as O
    n, D, d, kind, yvar = case
    rng = np.random.default_rng(seed)
    m = cigp(make_kernel(kind, D, rng), 0.7).double().to(DEV)
    X, Y = O.synthetic_xy(n, D, d, seed=seed)
    y = [T(Y), torch.diag(T(rng.uniform(0.01, 0.2, n)))] if yvar else T(Y)
    return m, T(X), y


def plain_loop(m, x, y, steps, lr, d_true=None):
    """the reference's loop; with d_true the targets are compressed ones and the missing columns' part of the likelihood is added"""
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    y0, yv = (y[0], y[1]) if isinstance(y, list) else (y, None)
    zeros = None
    if d_true is not None and d_true > y0.shape[1]:
        zeros = torch.zeros((y0.shape[0], d_true - y0.shape[1]), dtype=torch.float64, device=DEV)
    trace = np.zeros(steps)
    for k in range(steps):
        opt.zero_grad()
        loss = -m.negative_log_likelihood(x, y)
        if zeros is not None:
            loss = loss - m.negative_log_likelihood(x, [zeros, yv] if yv is not None else zeros)
        loss.backward()
        opt.step()
        trace[k] = float(loss.detach())
    return trace


def residual_loop_compressed(m, x, res, steps, lr, d_true):
    """train_AR's loop on compressed [y_high; y_low], the missing columns' part of the likelihood added"""
    rho, yl, yh = res
    vl, vh = (yl[1], yh[1]) if isinstance(yl, list) else (None, None)
    yl, yh = (yl[0], yh[0]) if vl is not None else (yl, yh)
    opt = torch.optim.Adam(list(m.parameters()) + [rho], lr=lr)
    zeros = torch.zeros((yh.shape[0], d_true - yh.shape[1]), dtype=torch.float64, device=DEV) if d_true > yh.shape[1] else None
    trace = np.zeros(steps)
    for k in range(steps):
        opt.zero_grad()
        yv = (vh - rho * vl).abs() if vl is not None else None
        r = yh - rho * yl
        loss = -m.negative_log_likelihood(x, [r, yv] if yv is not None else r)
        if zeros is not None:
            loss = loss - m.negative_log_likelihood(x, [zeros, yv] if yv is not None else zeros)
        loss.backward()
        opt.step()
        trace[k] = float(loss.detach())
    return trace


def distance(trace, params, ref_trace, ref_params):
    """the metric of every trajectory comparison here: the largest of rel(trace) and rel(parameter tensor), rho included"""
    d = rel(trace, ref_trace)
    for a, b in zip(params, ref_params):
        d = max(d, rel(a, b))
    return d


def loop_yardstick(name):
    """d0 of a case (for re-measuring the tables above; the tests do not call it): the per-step loop on the full targets against the
    per-step loop on the compressed ones"""
    from fidelityfusion_amd.train import compress_targets
    if name in PLAIN:
        case = PLAIN[name][0]
        m, x, y = make_plain(case)
        twin = copy.deepcopy(m)
        full = plain_loop(m, x, y, STEPS, LR)
        y0 = y[0] if isinstance(y, list) else y
        yc, = compress_targets(y0)
        comp = plain_loop(twin, x, [yc, y[1]] if isinstance(y, list) else yc, STEPS, LR, d_true=case[2])
        return distance(comp, params_of(twin), full, params_of(m))
    n, D, d, kind, form = RESIDUAL[name][0]
    m, x, res = make_residual(n, D, d, kind, form, 100 * n + D)
    twin, tres = copy.deepcopy(m), clone_residual(res)
    full, _, _ = reference_ar_loop(m, x, res, STEPS, LR)
    rho, yl, yh = tres
    if form == "subset":
        yhc, ylc = compress_targets(yh, yl)
        cres = (rho, ylc, yhc)
    else:
        yhc, ylc = compress_targets(yh[0], yl[0])
        cres = (rho, [ylc, yl[1]], [yhc, yh[1]])
    comp = residual_loop_compressed(twin, x, cres, STEPS, LR, d)
    return distance(comp, params_of(twin) + [rho.detach().cpu().numpy()], full, params_of(m) + [res[0].detach().cpu().numpy()])


def bound_of(d0):
    assert d0 is not None and 10 * d0 <= 1e-9, "the case has no measured yardstick, or is ill-conditioned"
    return max(10 * d0, 1e-12)


def test_wide_model_takes_the_one_launch_route():
    """fails before ffgp_train_wide_raw: train_many has no keyword wide_one_launch"""
    from fidelityfusion_amd.cigp_v10 import train_many
    m, x, y = make_plain((40, 2, 100, "ard", False), 3)
    before = params_of(m)
    trace, state = train_many([m], [x], [y], 5, lr=LR, wide_one_launch=True)
    assert state["fused"] is True and state["wide_one_launch"] == [0] and state["wide_status"] == {0: 0}
    assert all(p.grad is None for p in m.parameters())
    assert trace.shape == (1, 5) and trace.is_cuda and bool(torch.isfinite(trace).all())
    assert float(trace[0, -1]) < float(trace[0, 0])
    assert all(np.abs(a - b).max() > 0 for a, b in zip(params_of(m), before))
    m, x, y = make_plain((40, 2, 100, "ard", False), 3)
    _, state2 = train_many([m], [x], [y], 5, lr=LR)
    assert state2["fused"] is True and "wide_one_launch" not in state2


def _low_rank(rng, n, d, k):
    return rng.standard_normal((n, k)) @ rng.standard_normal((k, d))


# name -> the matrices handed to compress_targets, by (rows, columns, rank or None = full) -- m = the rows in all
COMPRESS = {
    "m20": [(20, 64, None)],                              # the one-workgroup LDS eigensolver
    "m128": [(128, 300, None)],                           # ... at its largest size
    "m80_unequal": [(30, 200, None), (50, 200, None)],    # a row split into unequal blocks
    "m256": [(128, 600, None), (128, 600, None)],         # a residual member at n = 128: the two-stage eigensolver
    "m40_rank5": [(40, 100, 5)],                          # a rank-deficient Gram: 35 eigenvalues are rounding, of either sign
    "m40_dependent": [(20, 64, None), "half"],            # y_low = y_high / 2: rank 20 of 40, across the row split
}


@pytest.mark.parametrize("name", sorted(COMPRESS))
def test_compress_targets_keeps_the_gram(name):
    """train.compress_targets itself: its row blocks Z_eff [n_i, m] have Z_eff Z_eff^T = Z Z^T, finite entries although a
    rank-deficient Gram has eigenvalues that are rounding of either sign (clamped before the square root).

    The bound, in the Frobenius norm and relative to |G|_F, is no measurement.  With eps = 2^-52 and E the error of the decomposition
    the helper clamps (as a matrix: U Lambda U^T - Z Z^T):
      |E|_F <= rec + gemm,  rec = 1e-13 max(1, sqrt(m) / 8) |G|_F   the bar this project holds both of its eigensolvers to
                                                                    (test_syev_lds_vs_lapack, test_syevd_vs_lapack)
                            gemm = d eps sqrt(m) |G|_F              the Gram's rounding: d eps |z_i| |z_j| per entry, the entries'
                                                                    squares sum to at most trace(G)^2 <= m |G|_F^2
      the clamp removes at most |E|_F: Z Z^T has no negative eigenvalue, so each clamped one is no larger than its distance from the
      true one, and those distances' squares sum to at most |E|_F^2 (Hoffman-Wielandt)
      the test's own two products (Z Z^T and Z_eff Z_eff^T in numpy's fp64): gemm + m eps sqrt(m) |G|_F, and the rounding of the
      square root and of the scaling of U's columns: 4 eps sqrt(m) |G|_F
    so |Z_eff Z_eff^T - Z Z^T|_F <= 2 rec + 3 gemm + (m + 4) eps sqrt(m) |G|_F."""
    from fidelityfusion_amd.train import compress_targets
    rng = np.random.default_rng(sum(map(ord, name)))
    mats = []
    for spec in COMPRESS[name]:
        if spec == "half":
            mats.append(0.5 * mats[0])
        else:
            n, d, k = spec
            mats.append(rng.standard_normal((n, d)) if k is None else _low_rank(rng, n, d, k))
    out = compress_targets(*[T(a) for a in mats])
    m, d = sum(a.shape[0] for a in mats), mats[0].shape[1]
    assert d > m and len(out) == len(mats)
    for a, z in zip(mats, out):
        assert z.shape == (a.shape[0], m) and z.is_contiguous() and z.dtype == torch.float64 and bool(torch.isfinite(z).all())
    Z, Ze = np.concatenate(mats, 0), np.concatenate([z.cpu().numpy() for z in out], 0)
    G = Z @ Z.T
    eps, gn = 2.0 ** -52, np.linalg.norm(G)
    bound = (2 * 1e-13 * max(1.0, np.sqrt(m) / 8) + 3 * d * eps * np.sqrt(m) + (m + 4) * eps * np.sqrt(m)) * gn
    err = np.linalg.norm(Ze @ Ze.T - G)
    print("%s: m %d, d %d, |Z_eff Z_eff^T - Z Z^T|_F %.3g, bound %.3g (|G|_F %.3g)" % (name, m, d, err, bound, gn))
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_plain_wide_model_follows_the_per_step_loop(name):
    """three ways: the fused call, train_many without the keyword (launch per stage), the per-step loop on the full targets"""
    from fidelityfusion_amd.cigp_v10 import train_many
    case, r, d0 = PLAIN[name]
    m, x, y = make_plain(case)
    old, twin = copy.deepcopy(m), copy.deepcopy(m)
    trace, state = train_many([m], [x], [y], STEPS, lr=LR, wide_one_launch=True)
    assert state["fused"] is True and state["wide_one_launch"] == [0]
    trace_old, state_old = train_many([old], [x], [y], STEPS, lr=LR)
    assert state_old["fused"] is True
    ref = plain_loop(twin, x, y, STEPS, LR)
    dist = distance(trace, params_of(m), ref, params_of(twin))
    dist_old = distance(trace_old, params_of(old), ref, params_of(twin))
    print("%s: r %d, d0 %s, one-launch trainer %.3g, launch-per-stage trainer %.3g" % (name, r, d0, dist, dist_old))
    bound = bound_of(d0)
    assert dist <= bound, (dist, bound)
    assert dist_old <= bound, (dist_old, bound)


@pytest.mark.parametrize("name", sorted(RESIDUAL))
def test_residual_wide_model_follows_the_per_step_loop(name):
    from fidelityfusion_amd.cigp_v10 import train_many
    (n, D, d, kind, form), r, d0 = RESIDUAL[name]
    m, x, res = make_residual(n, D, d, kind, form, 100 * n + D)
    old, ores = copy.deepcopy(m), clone_residual(res)
    twin, tres = copy.deepcopy(m), clone_residual(res)
    trace, state = train_many([m], [x], [None], STEPS, lr=LR, residual=[res], wide_one_launch=True)
    assert state["fused"] is True and state["wide_one_launch"] == [0]
    trace_old, state_old = train_many([old], [x], [None], STEPS, lr=LR, residual=[ores])
    ref, _, last = reference_ar_loop(twin, x, tres, STEPS, LR)
    want = params_of(twin) + [tres[0].detach().cpu().numpy()]
    dist = distance(trace, params_of(m) + [res[0].detach().cpu().numpy()], ref, want)
    dist_old = distance(trace_old, params_of(old) + [ores[0].detach().cpu().numpy()], ref, want)
    print("%s: r %d, d0 %s, one-launch trainer %.3g, launch-per-stage trainer %.3g" % (name, r, d0, dist, dist_old))
    bound = bound_of(d0)
    assert dist <= bound, (dist, bound)
    assert dist_old <= bound, (dist_old, bound)
    # train_AR's data for the fidelity: the residual at the rho of the start of the last step, on the FULL targets
    got = state["residual_targets"][0]
    lastl = last if isinstance(last, list) else [last, None]
    assert got[0].shape == (n, d) and rel(got[0], lastl[0]) <= bound
    assert (got[1] is None) == (lastl[1] is None) and (got[1] is None or rel(got[1], lastl[1]) <= bound)


def _mixed():
    """three plain models of different (n, r) and one residual member"""
    items = [make_plain((9, 1, 20, "ard", False), 21) + (None,), make_plain((40, 9, 70, "matern", False), 22) + (None,),
             make_plain((100, 3, 129, "se", True), 23) + (None,)]
    m, x, res = make_residual(30, 2, 90, "ard", "full", 24)
    items.append((m, x, None, res))
    return [list(t) for t in zip(*items)]


def test_mixed_call_trains_each_model_as_alone():
    """bit for bit: one workgroup per model, no atomics"""
    from fidelityfusion_amd.cigp_v10 import train_many
    models, xs, ys, rs = _mixed()
    trace, state = train_many(models, xs, ys, 8, lr=LR, residual=rs, wide_one_launch=True)
    assert state["fused"] is True and state["wide_one_launch"] == [0, 1, 2, 3] and bool(torch.isfinite(trace).all())
    solo, xs2, ys2, rs2 = _mixed()
    for f in range(4):
        tr, st = train_many([solo[f]], [xs2[f]], [ys2[f]], 8, lr=LR, residual=[rs2[f]], wide_one_launch=True)
        assert st["wide_one_launch"] == [0]
        assert torch.equal(tr[0], trace[f]), (f, rel(tr[0], trace[f]))
        for a, b in zip(params_of(solo[f]), params_of(models[f])):
            assert np.array_equal(a, b), f
    assert torch.equal(rs2[3][0].detach(), rs[3][0].detach())


def test_not_positive_definite_stops_that_model_alone():
    """the recipe of the one-launch tests: one model of a mixed call continued with y_var = -3 I.  LinAlgError; its status word is set,
    its trace NaN from the failing (first) step, its parameters bit-identical to before the call; the others trained on as alone"""
    from fidelityfusion_amd.cigp_v10 import train_many
    models, xs, ys, rs = _mixed()
    solo, xs2, ys2, rs2 = _mixed()
    _, state = train_many(models, xs, ys, 2, lr=LR, residual=rs, wide_one_launch=True)
    states2 = [train_many([solo[f]], [xs2[f]], [ys2[f]], 2, lr=LR, residual=[rs2[f]], wide_one_launch=True)[1] for f in range(4)]
    mid = params_of(models[1])
    bad = [ys[1], -3.0 * torch.eye(xs[1].shape[0], device=DEV)]
    with pytest.raises(torch.linalg.LinAlgError):
        train_many(models, xs, [ys[0], bad, ys[2], ys[3]], 4, lr=LR, residual=rs, state=state, wide_one_launch=True)
    assert state["wide_one_launch"] == [0, 1, 2, 3]
    assert state["wide_status"][1] > 0 and all(state["wide_status"][f] == 0 for f in (0, 2, 3))
    assert bool(torch.isnan(state["wide_trace"][1]).all())
    assert all(np.array_equal(a, b) for a, b in zip(params_of(models[1]), mid))
    assert all(state["chunks"][(f,)].step == 2 for f in range(4))      # the optimisers of the failed call were not advanced
    for f in (0, 2, 3):
        tr, _ = train_many([solo[f]], [xs2[f]], [ys2[f]], 4, lr=LR, residual=[rs2[f]], state=states2[f], wide_one_launch=True)
        assert torch.equal(tr[0], state["wide_trace"][f]), f
        for a, b in zip(params_of(solo[f]), params_of(models[f])):
            assert np.array_equal(a, b), f


@pytest.mark.parametrize("first", [True, False])
def test_adam_state_moves_between_the_routes(first):
    """10 steps on one route, 10 on the other, ONE state: within the case's bound of the 20-step loop"""
    from fidelityfusion_amd.cigp_v10 import train_many
    case, r, d0 = PLAIN["n33_d1024"]
    m, x, y = make_plain(case)
    twin = copy.deepcopy(m)
    tr1, state = train_many([m], [x], [y], 10, lr=LR, wide_one_launch=first)
    assert state.get("wide_one_launch", []) == ([0] if first else [])
    tr2, state = train_many([m], [x], [y], 10, lr=LR, state=state, wide_one_launch=not first)
    assert state.get("wide_one_launch", []) == ([] if first else [0])
    assert list(state["chunks"]) == [(0,)] and state["chunks"][(0,)].step == 20
    ref = plain_loop(twin, x, y, 20, LR)
    dist = distance(torch.cat([tr1, tr2], dim=1), params_of(m), ref, params_of(twin))
    print("one launch %s: %.3g, bound %.3g" % ("first" if first else "second", dist, bound_of(d0)))
    assert dist <= bound_of(d0), (dist, bound_of(d0))


def test_unchanged_routing():
    """d <= 16, n > 128, a composed kernel, a GP_basic (the V2 likelihood), a CAR member (d > 16, n <= 128: a GP_basic over
    FidelityKernelMCMC with car=(b, y_low, y_high)), an fp32 model: the keyword changes nothing for them"""
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.cigp_v10 import cigp, train_many
    from fidelityfusion_amd.gp_basic import GP_basic
    from oracle import gp_oracle as O
    from test_gpu_train_car import make_car

    def models():
        out = []
        for f, (n, D, d) in enumerate([(40, 2, 16), (129, 2, 40)]):
            out.append(make_plain((n, D, d, "ard", False), 31 + f) + (None,))
        X, Y = O.synthetic_xy(30, 2, 40, seed=33)
        out.append((cigp(kernel.SumKernel(kernel.LinearKernel(2), kernel.MaternKernel(2)), 0.7).double().to(DEV), T(X), T(Y), None))
        out.append((GP_basic(kernel.ARDKernel(2), 0.5).double().to(DEV), T(X), T(Y), None))
        m, x, c = make_car(30, 2, 40, "ard", 36)
        out.append((m, x, None, c))
        return [list(t) for t in zip(*out)]
    CAR = 4
    ms, xs, ys, cars = models()
    tr, state = train_many(ms, xs, ys, 4, lr=LR, car=cars, wide_one_launch=True)
    assert state["fused"] is True and state["wide_one_launch"] == [] and CAR not in state["wide_status"]
    ms2, xs2, ys2, cars2 = models()
    tr2, state2 = train_many(ms2, xs2, ys2, 4, lr=LR, car=cars2)
    # (the same code on the same inputs: two runs can differ at most by the order of a kernel's atomic adds)
    assert bool(torch.isfinite(tr).all()) and rel(tr, tr2) <= 1e-12 and rel(tr[CAR], tr2[CAR]) <= 1e-12
    assert sorted(state["chunks"]) == sorted(state2["chunks"]) and (CAR,) in state["chunks"]
    assert state["chunks"][(CAR,)].stride == state2["chunks"][(CAR,)].stride      # (the CAR layout: six groups of parameters)
    for a, b in zip(ms, ms2):
        assert all(rel(p, q) <= 1e-12 for p, q in zip(params_of(a), params_of(b)))
    # the CAR member's data for its fidelity is train_CAR's, formed on its own targets
    assert rel(state["residual_targets"][CAR][0], state2["residual_targets"][CAR][0]) <= 1e-12
    # fp32: not eligible for the library's training calls at all -- the reference's loop, with or without the keyword
    X, Y = O.synthetic_xy(20, 2, 40, seed=34)
    m32 = cigp(kernel.ARDKernel(2), 0.7).float().to(DEV)
    _, st32 = train_many([m32], [T(X).float()], [T(Y).float()], 2, lr=LR, wide_one_launch=True)
    assert st32["fused"] is False and st32["wide_one_launch"] == []
    # ... and a wide model is left alone without the keyword (checked with the state: no per-route entries appear)
    m, x, y = make_plain((20, 2, 40, "ard", False), 35)
    _, st = train_many([m], [x], [y], 2, lr=LR)
    assert "wide_one_launch" not in st and "wide_status" not in st


def _handle():
    from fidelityfusion_amd import _lib
    h = _lib.handle(0)
    _lib.bind_stream(h, 0)
    return h


def _raw_call(h, m, x, y, steps=3, d_true=None, **over):
    """ffgp_train_wide_raw through ctypes on model m (an ARD `cigp`), the problem's fields overridden by `over`:
    (status, Adam state, trace, info word)"""
    from fidelityfusion_amd import _lib
    from fidelityfusion_amd._lib import Links, Problem
    from fidelityfusion_amd.cigp_v10 import JITTER, PI
    lk = m.kernel.links()
    n, D = x.shape
    p = Problem()
    p.n, p.D, p.d = n, D, y.shape[1]
    p.X_dev, p.Y_dev, p.w_dev, p.amp_dev, p.diag_add_dev = x.data_ptr(), y.data_ptr(), lk["w"].data_ptr(), lk["amp"].data_ptr(), m.log_beta.data_ptr()
    p.clamp_min, p.ll_variant, p.pi_const, p.kfun, p.kparam = lk["clamp"], 1, PI, lk["kfun"], 1.0
    for k, v in over.items():
        setattr(p, k, v)
    L = Links()
    L.w_link, L.w_c, L.w_broadcast = lk["w_link"], lk["w_c"], 0
    L.amp_link, L.dadd_link, L.dadd_c, L.out_scale = lk["amp_link"], _lib.LINK_EXP_NEG, JITTER, 1.0
    opt = _lib.Adam(LR, 0.9, 0.999, 1e-8)
    state = torch.zeros(64, device=DEV)
    trace = torch.full((steps,), -7.0, device=DEV)
    dt = (C.c_int * 1)(y.shape[1] if d_true is None else d_true)
    info = (C.c_int * 1)(-9)
    rc = _lib.lib.ffgp_train_wide_raw(h, 1, C.byref(p), C.byref(L), None, dt, steps, C.byref(opt), state.data_ptr(), 64, 0, trace.data_ptr(),
                                      steps, info)
    torch.cuda.synchronize()
    return rc, state, trace, info[0]


def test_c_abi_refuses_what_the_kernel_does_not_cover():
    """FFGP_ERR_ARG with parameters, state, trace and info untouched for d_true <= 16, n > 128, D > 16, a tree, the V2 likelihood,
    an RQ kernel, more than 128 columns passed -- and the accepted call behind them runs"""
    from fidelityfusion_amd import _lib
    m, x, y = make_plain((20, 2, 40, "ard", False), 41)
    h = _handle()
    before = params_of(m)
    tree = _lib.KTree()
    refused = {"d_true_16": dict(d_true=16), "n_129": dict(n=129), "D_17": dict(D=17), "tree": dict(tree=C.pointer(tree)),
               "v2": dict(ll_variant=_lib.FFGP_LL_V2), "rq": dict(kfun=4), "cols_129": dict(d=129, d_true=400), "cols_above_d": dict(d=41)}
    for name, kw in refused.items():
        kw = dict(kw)
        dt = kw.pop("d_true", None)
        rc, state, trace, info = _raw_call(h, m, x, y, d_true=dt, **kw)
        assert rc == _lib.FFGP_ERR_ARG, (name, rc)
        assert float(state.abs().max()) == 0.0 and bool((trace == -7.0).all()) and info == -9, name
        assert all(np.array_equal(a, b) for a, b in zip(params_of(m), before)), name
    rc, state, trace, info = _raw_call(h, m, x, y)
    assert rc == 0 and info == 0 and bool(torch.isfinite(trace).all()) and float(state.abs().max()) > 0.0
    assert all(np.abs(a - b).max() > 0 for a, b in zip(params_of(m), before))


def test_the_reference_fixture(golden):
    """tests/golden/train_wide_cigp.npz: the reference's `cigp` under its own Adam loop on the CPU, n = 12, d = 40, 20 steps -- loss
    trace and final parameters within 1e-8, the bound test_train_many_tree_on_the_reference_fixtures holds its fixtures to"""
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.cigp_v10 import cigp, train_many
    g = golden("train_wide_cigp")
    m = cigp(kernel.ARDKernel(2), 1.0).double().to(DEV)
    with torch.no_grad():
        for i, p in enumerate(m.parameters()):
            p.copy_(T(g["init_%d" % i]).reshape(p.shape))
    trace, state = train_many([m], [T(g["x"])], [T(g["y"])], int(g["steps"]), lr=float(g["lr"]), wide_one_launch=True)
    assert state["fused"] is True and state["wide_one_launch"] == [0]
    errs = {"trace": rel(trace[0], g["trace"])}
    for i, p in enumerate(m.parameters()):
        errs["final_%d" % i] = rel(p, g["final_%d" % i])
    print(errs)
    assert max(errs.values()) <= 1e-8, errs
