"""GPU: `hogp_simple.train_many` -- K Adam steps of HOGP blocks and GAR's residual fidelities per library call
(ffgp_train_hogp_raw, csrc/train_hogp.hip) -- against the reference's run (the gar_chain fixture), against the per-step loop on
the drop-in modules, and its contract: companions do not matter, continuation, a failing model stops alone, the fallback route.

Tolerance of the comparison with the per-step loop (not fixed in advance): for every case small enough (n prod(d) <= 1600) a
YARDSTICK is measured first, one PER QUANTITY -- the distance of the per-step GPU loop's loss trace, final parameters, cached A,
cached g and `forward` mean at 5 test points from a CPU float64 loop that evaluates the same loss as a dense Cholesky likelihood
of kron(K_0, ...) + tau I with torch autograd and torch.optim.Adam (its g is the solve S^-1 y of the last step, its A the outer
product of torch.linalg.eigvalsh's eigenvalues + tau, its mean g x_0 K_* x_m K_m) -- and the fused route must lie within 10 x
the quantity's own yardstick of the per-step GPU loop (the larger cases take the largest one measured for that quantity).
One rounding is the floor: a measured yardstick below eps = 2.2e-16 -- the per-step loop agreeing with the CPU to the last bit
of the quantity's largest entry, often exactly -- is read as eps, because two correct fp64 evaluations cannot be asked to agree
more closely than one rounding of the result; which quantities of which case needed that is printed.  On the MI355X: the
parameters of eight of the nine cases the CPU loop covers (Adam's first steps move a parameter by about lr * sign(gradient), and the per-step loop
ends on the CPU loop's very bits), the trace of n = 1, 5 and 17, and every quantity of the 1 x 1 problem n = 1, where all three
routes agree exactly; no A, g or `forward` mean of any other case.  Measured there: yardsticks of g 6e-16 ... 2.5e-11, of the
mean 1e-15 ... 1.2e-13, of A 5e-16 ... 1.5e-14, of the trace up to 2.2e-15; fused against per-step: g <= 1.1e-15, mean <=
3.5e-15, A <= 2.3e-18, trace <= 3.4e-16, parameters <= 2.0e-16.  Every figure is printed before it is asserted.
"""
import copy
import math
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EPS = 2.220446049250313e-16      # one rounding: the floor of a measured yardstick (module docstring)
QUANTITIES = ("trace", "params", "A", "g", "mean")
STEPS, LR = 6, 1e-2

#        name           n   shape       D  kernel
CASES = [("n1", 1, (2,), 1, "SE"),
         ("n5", 5, (3,), 1, "SE"),
         ("n17", 17, (5, 4), 2, "ARD"),
         ("n64", 64, (4, 3), 2, "SE"),
         ("n65", 65, (4, 3), 2, "SE"),
         ("n100", 100, (8, 8), 2, "ARD"),
         ("n128", 128, (16, 5), 3, "ARD"),
         ("n33", 33, (3, 2, 4), 2, "M52"),
         ("n40", 40, (64,), 1, "SE"),
         ("n20", 20, (1, 3), 2, "SE"),
         ("res_l4h8", 20, (3, 8), 2, "ARD"),      # residual, the last mode finer in y_high (l = 4, h = 8: the bilinear initialisation)
         ("res_leqh", 28, (4, 3), 2, "SE")]       # residual, l = h
RES_L = {"res_l4h8": 4, "res_leqh": 3}
CASE = {c[0]: c for c in CASES}


def rel(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    return float(np.abs(a.reshape(b.shape) - b).max() / max(np.abs(b).max(), 1e-300))


def make_kernel(kind, D):
    from fidelityfusion_amd import kernel
    if kind == "SE":
        k = kernel.SquaredExponentialKernel(0.3, 0.2)
    elif kind == "ARD":
        k = kernel.ARDKernel(D)
    else:
        k = kernel.MaternKernel(D, nu=2.5)
    if kind != "SE":
        with torch.no_grad():
            k.length_scales.copy_(torch.tensor([0.8, -1.1, 0.9][:D]))
            k.signal_variance.fill_(1.3)
    return k


def make_case(name):
    """(model, x, y or None, residual or None, x_test) on the GPU; the same numbers on every call"""
    from fidelityfusion_amd.gp_computation_pack import Tensor_linear
    from fidelityfusion_amd.hogp_simple import HOGP_simple
    _, n, shape, D, kind = CASE[name]
    g = torch.Generator().manual_seed(1000 + n + 7 * len(shape) + sum(shape))
    x = torch.rand((n, D), generator=g, dtype=torch.float64)
    xt = torch.rand((5, D), generator=g, dtype=torch.float64)
    phase = x.sum(1)

    def field(shp, amp):
        t = torch.sin(3.0 * phase).reshape((n,) + (1,) * len(shp)) * amp
        for ax, d in enumerate(shp):
            v = torch.cos(0.4 * torch.arange(d, dtype=torch.float64) + 0.3 * ax)
            t = t * v.reshape((1,) * (ax + 1) + (d,) + (1,) * (len(shp) - ax - 1))
        return t + 0.05 * torch.randn((n,) + tuple(shp), generator=g, dtype=torch.float64)

    m = HOGP_simple(make_kernel(kind, D), 0.5, shape).double().to(DEV)
    if name in RES_L:
        l = RES_L[name]
        lshape = shape[:-1] + (l,)
        tl = Tensor_linear(lshape, shape).double().to(DEV)
        yl, yh = field(lshape, 1.0).to(DEV), field(shape, 1.4).to(DEV)
        return m, x.to(DEV), None, (tl, yl, yh), xt.to(DEV)
    return m, x.to(DEV), field(shape, 1.0).to(DEV), None, xt.to(DEV)


def params_of(m, res):
    k = m.kernel_list[0]
    ps = [p for _, p in sorted(k.named_parameters())] + [m.noise_variance]
    if res is not None:
        ps.append(res[0].vectors[-1])
    return [p.detach().clone() for p in ps]


def per_step_loop(m, x, y, res, steps, lr=LR):
    """train_GAR's loop on the drop-in modules (tests/mf_harness.train_gar), one fidelity"""
    pars = list(m.parameters()) + (list(res[0].parameters()) if res is not None else [])
    opt = torch.optim.Adam(pars, lr=lr)
    trace = []
    for _ in range(steps):
        opt.zero_grad()
        yy = y if res is None else res[2] - res[0](res[1])
        loss = m.log_likelihood(x, yy)
        trace.append(float(loss.detach()))
        loss.backward()
        opt.step()
    return np.array(trace)


def cpu_dense_loop(name, m, x, y, res, steps, xt, lr=LR):
    """the same loss as a dense Cholesky likelihood of kron(K_0, K_1, ...) + tau I in float64 on the CPU, torch autograd, torch.optim.Adam;
    returns the trace, the final parameters and the counterparts of the block's caches after the loop: g = S^-1 y and A = outer(eigenvalues)
    + tau of the LAST step (the parameters that step began with), and `forward`'s mean g x_0 K(x_test, x; final parameters) x_m K_m"""
    _, n, shape, D, kind = CASE[name]
    k = m.kernel_list[0]
    names = [nm for nm, _ in sorted(k.named_parameters())]
    raw = {nm: p.detach().cpu().clone().requires_grad_(True) for nm, p in sorted(k.named_parameters())}
    noise = m.noise_variance.detach().cpu().clone().requires_grad_(True)
    xc = x.cpu()
    V = res[0].vectors[-1].detach().cpu().clone().requires_grad_(True) if res is not None else None
    rho = float(getattr(k, "rho", 1.0))

    def kmat(a, b=None):
        b = a if b is None else b
        if kind == "SE":
            w, amp = torch.exp(-raw["length_scale"]), raw["signal_variance"].exp().pow(2)
            d = (a.unsqueeze(1) - b.unsqueeze(0)) * w
            return amp * torch.exp(-0.5 * (d * d).sum(-1))
        w, amp = 1.0 / (raw["length_scales"].abs() + k.eps), raw["signal_variance"].abs()
        if a.shape[1] == 1 and w.numel() > 1:
            a, b = a.expand(-1, w.numel()), b.expand(-1, w.numel())
        d = (a.unsqueeze(1) - b.unsqueeze(0)) * w
        s = (d * d).sum(-1).clamp_min(1e-30)
        if kind == "ARD":
            return amp * torch.exp(-0.5 * s)
        r = torch.sqrt(5.0 * s) / rho
        return amp * (1.0 + r + (5.0 / 3.0) * s / rho ** 2) * torch.exp(-r)

    grids = [torch.arange(d, dtype=torch.float64).reshape(-1, 1) for d in shape]
    opt = torch.optim.Adam(list(raw.values()) + [noise] + ([V] if V is not None else []), lr=lr)
    trace, last = [], {}
    for it in range(steps):
        opt.zero_grad()
        Ks = [kmat(xc)] + [kmat(gr) for gr in grids]
        S = Ks[0]
        for Km in Ks[1:]:
            S = torch.kron(S, Km)
        nd = S.shape[0]
        S = S + torch.eye(nd, dtype=torch.float64) / noise
        yy = y.cpu() if res is None else res[2].cpu() - torch.matmul(res[1].cpu(), V.T)
        L = torch.linalg.cholesky(S)
        a = torch.cholesky_solve(yy.reshape(-1, 1), L)
        loss = (0.5 * nd * math.log(2 * math.pi) + torch.log(L.diagonal()).sum() + 0.5 * (yy.reshape(-1, 1) * a).sum()) / nd
        trace.append(float(loss.detach()))
        if it == steps - 1:
            with torch.no_grad():
                A = torch.linalg.eigvalsh(Ks[0])
                for Km in Ks[1:]:
                    A = A.unsqueeze(-1) * torch.linalg.eigvalsh(Km).reshape((1,) * A.dim() + (-1,))
                last = {"A": A + 1.0 / noise.detach(), "g": a.detach().reshape((n,) + tuple(shape)), "Ks": [Km.detach() for Km in Ks]}
        loss.backward()
        opt.step()
    with torch.no_grad():
        mean = last["g"]
        for ax, Mx in enumerate([kmat(xt.cpu(), xc)] + last["Ks"][1:]):
            mean = torch.tensordot(Mx, mean, dims=([1], [ax])).movedim(0, ax)
    ps = [raw[nm].detach() for nm in names] + [noise.detach()] + ([V.detach()] if V is not None else [])
    return {"trace": np.array(trace), "params": ps, "A": last["A"], "g": last["g"], "mean": mean}


_results = {}


def run_case(name):
    """per-step GPU loop, fused route and (small cases) the CPU loop from identical copies; cached for the module"""
    if name in _results:
        return _results[name]
    from fidelityfusion_amd import hogp_simple as H
    _, n, shape, D, kind = CASE[name]
    m0, x, y, res, xt = make_case(name)
    out = {}
    # per-step loop
    m1, r1 = copy.deepcopy(m0), copy.deepcopy(res)
    out["step_trace"] = per_step_loop(m1, x, y, r1, STEPS)
    out["step_params"] = params_of(m1, r1)
    with torch.no_grad():
        out["step_A"], out["step_g"] = m1.A.detach().clone(), m1.g.detach().clone()
        out["step_mean"] = m1.forward(x, xt)[0].detach().clone()
    # fused
    m2, r2 = copy.deepcopy(m0), copy.deepcopy(res)
    tr, st = H.train_many([m2], [x], [y], STEPS, lr=LR, residual=None if res is None else [r2])
    out["fused"] = st.fused
    out["fused_trace"] = tr[0].cpu().numpy()
    out["fused_params"] = params_of(m2, r2)
    with torch.no_grad():
        out["fused_A"], out["fused_g"] = m2.A.detach().clone(), m2.g.detach().clone()
        out["fused_mean"] = m2.forward(x, xt)[0].detach().clone()
    out["yard"] = None
    if n * math.prod(shape) <= 1600:
        c = cpu_dense_loop(name, m0, x, y, res, STEPS, xt)
        out["yard"] = {"trace": rel(out["step_trace"], c["trace"]),
                       "params": max(rel(a, b) for a, b in zip(out["step_params"], c["params"])),
                       "A": rel(out["step_A"], c["A"]), "g": rel(out["step_g"], c["g"]), "mean": rel(out["step_mean"], c["mean"])}
    _results[name] = out
    return out


def yardsticks(name):
    """({quantity: yardstick}, the quantities whose MEASURED yardstick lay below one rounding and is read as eps): the case's own where it
    is small enough for the CPU loop, else the largest measured one of each quantity"""
    r = run_case(name)
    if r["yard"] is not None:
        raw = r["yard"]
    else:
        small = [run_case(c[0])["yard"] for c in CASES]
        raw = {q: max(y[q] for y in small if y is not None) for q in QUANTITIES}
    return {q: max(raw[q], EPS) for q in QUANTITIES}, [q for q in QUANTITIES if raw[q] < EPS]


def test_gar_chain_golden_through_train_many(golden):
    """the reference's run: train_GAR on the gar_chain fixture (2 fidelities x 3 Adam steps, SE kernels, [4, 3] outputs, the residual
    behind a two-mode Tensor_linear) with both fidelities trained by train_many, held to test_gar_chain_golden's bounds"""
    from fidelityfusion_amd import hogp_simple as H
    from fidelityfusion_amd import kernel
    from mf_harness import GAR
    g = golden("gar_chain")
    tt = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)
    model = GAR(2, [kernel.SquaredExponentialKernel() for _ in range(2)], [(4, 3), (4, 3)]).double().to(DEV)
    v0 = model.Tensor_linear_list[0].vectors[0].detach().clone()
    tr0, st0 = H.train_many([model.hogp_list[0]], [tt(g["x0n"])], [tt(g["y0n"])], 3, lr=1e-2)
    fx = tt(g["fill_x"])
    res = (model.Tensor_linear_list[0], [tt(g["fill_ylow_mean"]), tt(g["fill_ylow_var"])], [tt(g["fill_yhigh_mean"]), tt(g["fill_yhigh_var"])])
    tr1, st1 = H.train_many([model.hogp_list[1]], [fx], [None], 3, lr=1e-2, residual=[res])
    assert st0.fused and st1.fused
    trace = np.concatenate([tr0[0].cpu().numpy(), tr1[0].cpu().numpy()])
    print("loss_trace rel", rel(trace, g["loss_trace"]))
    assert rel(trace, g["loss_trace"]) < 1e-8
    for name, p in model.state_dict().items():
        print(name, rel(p, g[name.replace(".", "__")]))
        assert rel(p, g[name.replace(".", "__")]) < 1e-7, name
    assert torch.equal(model.Tensor_linear_list[0].vectors[0].detach(), v0)
    with torch.no_grad():
        yp, _ = model([tt(g["x0n"]), fx], tt(g["xtn"]))
    print("forward mean rel", rel(yp, g["ypred"]))
    assert rel(yp, g["ypred"]) < 1e-6


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_fused_against_per_step_loop(name):
    r = run_case(name)
    y, floored = yardsticks(name)
    assert r["fused"]
    d = {"trace": rel(r["fused_trace"], r["step_trace"]),
         "params": max(rel(a, b) for a, b in zip(r["fused_params"], r["step_params"])),
         "A": rel(r["fused_A"], r["step_A"]), "g": rel(r["fused_g"], r["step_g"]), "mean": rel(r["fused_mean"], r["step_mean"])}
    print("%s (%s yardsticks): " % (name, "own" if r["yard"] is not None else "largest measured")
          + "  ".join("%s %.2e / %.2e" % (q, d[q], y[q]) for q in QUANTITIES) + "   [fused vs per-step / yardstick; read as eps: %s]" % (floored or "none"))
    assert np.all(np.isfinite(r["step_trace"])) and np.all(np.isfinite(r["fused_trace"]))
    for q in QUANTITIES:
        assert d[q] <= 10 * y[q], (q, d[q], y[q])


def _snapshot(m, res, st, f):
    ea, es = st.moments(f)
    return [p.clone() for p in params_of(m, res)] + [ea.clone(), es.clone()]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


def test_companions_do_not_matter():
    """three models of different n (17, 65, 28 as a residual block) in one call: each model's trace, parameters and moments equal its
    own single-model call bit for bit"""
    from fidelityfusion_amd import hogp_simple as H
    names = ["n17", "n65", "res_leqh"]
    built = [make_case(nm) for nm in names]
    ms = [copy.deepcopy(b[0]) for b in built]
    rs = [copy.deepcopy(b[3]) for b in built]
    tr, st = H.train_many(ms, [b[1] for b in built], [b[2] for b in built], 4, lr=LR, residual=rs)
    assert st.fused and not st.failed
    for f, b in enumerate(built):
        m1, r1 = copy.deepcopy(b[0]), copy.deepcopy(b[3])
        tr1, st1 = H.train_many([m1], [b[1]], [b[2]], 4, lr=LR, residual=None if r1 is None else [r1])
        assert torch.equal(tr[f], tr1[0]), names[f]
        assert _same(_snapshot(ms[f], rs[f], st, f), _snapshot(m1, r1, st1, 0)), names[f]


def test_continuation():
    """3 + 3 steps with the returned state equal 6 steps bit for bit"""
    from fidelityfusion_amd import hogp_simple as H
    for nm in ("n17", "res_l4h8"):
        m0, x, y, res, _ = make_case(nm)
        ma, ra, mb, rb = copy.deepcopy(m0), copy.deepcopy(res), copy.deepcopy(m0), copy.deepcopy(res)
        wrap = lambda r: None if r is None else [r]
        t6, s6 = H.train_many([ma], [x], [y], 6, lr=LR, residual=wrap(ra))
        t3a, s3 = H.train_many([mb], [x], [y], 3, lr=LR, residual=wrap(rb))
        t3b, s3 = H.train_many([mb], [x], [y], 3, lr=LR, residual=wrap(rb), state=s3)
        assert s3.steps == [6] and s6.steps == [6]
        assert torch.equal(t6[0], torch.cat([t3a[0], t3b[0]])), nm
        assert _same(_snapshot(ma, ra, s6, 0), _snapshot(mb, rb, s3, 0)), nm


def test_a_failing_model_stops_alone():
    from fidelityfusion_amd import hogp_simple as H
    good, x, y, _, _ = make_case("n17")
    bad, xb, yb, _, _ = make_case("n5")
    with torch.no_grad():
        bad.noise_variance.fill_(-0.5)
    before = params_of(bad, None)
    g1, b1 = copy.deepcopy(good), copy.deepcopy(bad)
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        tr, st = H.train_many([g1, b1], [x, xb], [y, yb], 4, lr=LR)
    assert any(issubclass(w.category, RuntimeWarning) for w in wlist)       # the documented signal: a warning and state.failed
    assert st.fused and st.failed == {1: 0} and st.steps == [4, 0]
    assert bool(torch.isnan(tr[1]).all()) and bool(torch.isfinite(tr[0]).all())
    assert _same(params_of(b1, None), before)
    ea, es = st.moments(1)
    assert not bool(ea.any()) and not bool(es.any())
    # the survivor: its single call, bit for bit
    g2 = copy.deepcopy(good)
    tr2, st2 = H.train_many([g2], [x], [y], 4, lr=LR)
    assert torch.equal(tr[0], tr2[0]) and _same(_snapshot(g1, None, st, 0), _snapshot(g2, None, st2, 0))
    # ... and continued with the returned state it follows an uninterrupted run
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tr3, st = H.train_many([g1, b1], [x, xb], [y, yb], 2, lr=LR, state=st)
    g3 = copy.deepcopy(good)
    tr6, st6 = H.train_many([g3], [x], [y], 6, lr=LR)
    assert st.steps == [6, 0]
    assert torch.equal(torch.cat([tr[0], tr3[0]]), tr6[0]) and _same(_snapshot(g1, None, st, 0), _snapshot(g3, None, st6, 0))


def test_fallback_route():
    """a learnable_map=True model and an n = 129 model: the reference loop's values, state.fused false"""
    from fidelityfusion_amd import hogp_simple as H
    from fidelityfusion_amd.hogp_simple import HOGP_simple
    g = torch.Generator().manual_seed(5)
    for n, kw in ((12, {"learnable_map": True}), (129, {})):
        x = torch.rand((n, 2), generator=g, dtype=torch.float64).to(DEV)
        y = (torch.sin(3 * x.sum(1)).reshape(n, 1, 1) * torch.ones((1, 3, 2), dtype=torch.float64, device=DEV)
             + 0.05 * torch.randn((n, 3, 2), generator=g, dtype=torch.float64).to(DEV))
        m0 = HOGP_simple(make_kernel("ARD", 2), 0.5, (3, 2), **kw).double().to(DEV)
        ma, mb = copy.deepcopy(m0), copy.deepcopy(m0)
        want = per_step_loop(ma, x, y, None, 3)
        tr, st = H.train_many([mb], [x], [y], 3, lr=LR)
        assert st.fused is False and st.steps == [3]
        # (the same code on the same numbers; 1e-10 leaves room only for a reduction whose order is not fixed from run to run)
        print("fallback n = %d: trace rel %.3e" % (n, rel(tr[0], want)))
        assert rel(tr[0], want) <= 1e-10
        for (na, pa), (_, pb) in zip(ma.state_dict().items(), mb.state_dict().items()):
            assert rel(pb, pa) <= 1e-10, na
