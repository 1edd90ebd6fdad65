"""train_many(..., residual=[(tensor_linear, y_low, y_high)]): train_CIGAR's fidelities above 0 (FidelityFusion_Models/CIGAR.py:110-134) --
a cigp on y_high - Tensor_linear(y_low), the map's matrix V under the same Adam as the three GP parameters -- through ffgp_train_tlin_raw,
against the reference-generated fixture tests/golden/cigar_chain.npz, against the reference's own loop (drop-in modules, torch.optim.Adam
over the GP parameters and the map, the residual recomputed every step) and, for the bound of that comparison, against the same steps in
plain torch on the CPU.

The bound of the loop comparison is measured: delta = the distance between the per-step GPU loop and the CPU loop (two independent fp64
evaluations of one trajectory); the fused route must lie within max(10 delta, 1e-12) of the GPU loop, and within the rho route's bars
(1e-11 trace, 1e-10 parameters) unless delta itself exceeds them.  Measured on an MI355X (profiles/train_tlin_parity.txt holds every
case): delta 1.6e-16 ... 5.9e-16 (trace) and 1.2e-16 ... 5.5e-16 (parameters), so the bound is its floor of 1e-12 at every case; fused distances
0 ... 3.7e-16 (trace) and 0 ... 3.7e-16 (parameters), the largest at (300, 9, 40, 64) and (128, 2, 16, 17)."""
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
BAR_TRACE, BAR_PAR, FLOOR = 1e-11, 1e-10, 1e-12


def T(a, dev=DEV):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device=dev)


def rel(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    return float(np.abs(a.reshape(b.shape) - b).max() / max(np.abs(b).max(), 1e-300))


def params_of(m, tl=None):
    """the GP parameters, then the map's matrix in logical (row-major) order"""
    out = [p.detach().cpu().numpy().copy() for p in m.parameters()]
    return out + ([tl.vectors[0].detach().cpu().numpy().copy()] if tl is not None else [])


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


def make_link(n, D, l, h, kind, form, seed, dev=DEV):
    """one CIGAR fidelity above 0: model, x, (tensor_linear, y_low, y_high).  Generic data: every column of y_low is non-zero and V is the
    initialisation (identity, or for l < h the bilinear interpolation -- a transposed view) plus noise, so that no entry of dV is
    structurally zero.  Full form: symmetric [n, n] variances of which only the diagonals act, their difference of either sign."""
    from fidelityfusion_amd.cigp_v10 import cigp
    from fidelityfusion_amd.gp_computation_pack import Tensor_linear
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (n, D))
    yl = np.sin(3 * x[:, :1] + np.arange(l)) + 0.1 * rng.standard_normal((n, l)) + 0.3
    W = rng.uniform(0.5, 1.5, (h, l)) / l
    yh = 1.3 * yl @ W.T + 0.2 * np.cos(2 * x[:, :1] + np.arange(h)) + 0.05 * rng.standard_normal((n, h))
    m = cigp(make_kernel(kind, D, rng), 0.6).double().to(dev)
    tl = Tensor_linear((l,), (h,)).double().to(dev)
    with torch.no_grad():
        tl.vectors[0].add_(torch.tensor(0.05 * rng.standard_normal((h, l)), device=dev))
    if form == "subset":
        return m, T(x, dev), (tl, T(yl, dev), T(yh, dev))
    a, b = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    vl, vh = 0.02 * (a + a.T), 0.02 * (b + b.T)
    vl[np.diag_indices(n)] = rng.uniform(0.01, 0.2, n)
    vh[np.diag_indices(n)] = rng.uniform(0.01, 0.3, n)
    return m, T(x, dev), (tl, [T(yl, dev), T(vl, dev)], [T(yh, dev), T(vh, dev)])


def clone_link(res):
    return (copy.deepcopy(res[0]), res[1], res[2])


def reference_cigar_loop(m, x, res, steps, lr, opt=None):
    """train_CIGAR's loop (CIGAR.py:116-133) through the drop-in modules: Adam over the GP parameters and the map"""
    tl, yl, yh = res
    opt = opt or torch.optim.Adam(list(m.parameters()) + list(tl.parameters()), lr=lr)
    trace, last = [], None
    for _ in range(steps):
        opt.zero_grad()
        if isinstance(yl, list):
            y = [yh[0] - tl(yl[0]), (yh[1] - yl[1]).abs()]
        else:
            y = yh - tl(yl)
        last = y
        loss = -m.negative_log_likelihood(x, y)
        loss.backward()
        opt.step()
        trace.append(float(loss.detach()))
    return np.array(trace), opt, last


def cpu_torch_loop(kind, m, x, res, steps, lr):
    """the same steps in plain torch on the CPU: oracle/torch_cpu_ref.py's operator sequence (kernel, Sigma = K + (exp(log_beta)^-1 +
    1e-6) I + diag(y_var), Cholesky, triangular solve, the value with the reference's pi) with the kernel of `kind` written out
    (GaussianProcess/kernel.py), autograd and torch.optim.Adam.  Returns the loss trace and the parameters in `params_of`'s order."""
    from oracle import torch_cpu_ref as R
    tl, yl, yh = res
    X = x.detach().cpu()
    pars = [p.detach().cpu().clone().requires_grad_(True) for p in m.parameters()]
    names = [k for k, _ in m.named_parameters()]
    P = dict(zip(names, pars))
    V = tl.vectors[0].detach().cpu().clone().contiguous().requires_grad_(True)
    full = isinstance(yl, list)
    YL, YH = (yl[0] if full else yl).cpu(), (yh[0] if full else yh).cpu()
    dv = (yh[1].cpu() - yl[1].cpu()).abs().diagonal() if full else None
    n, h = YH.shape
    eye = torch.eye(n)
    opt = torch.optim.Adam(pars + [V], lr=lr)
    trace = []
    for _ in range(steps):
        opt.zero_grad()
        if kind == "se":
            sq = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
            K = P["kernel.signal_variance"].exp() ** 2 * torch.exp(-0.5 * sq / P["kernel.length_scale"].exp() ** 2)
        else:
            Xs = X / (P["kernel.length_scales"].abs() + R.EPS)
            sq = ((Xs[:, None, :] - Xs[None, :, :]) ** 2).sum(-1)
            if kind == "ard":
                K = P["kernel.signal_variance"].abs() * torch.exp(-0.5 * sq)
            else:
                a = (5.0 * sq.clamp_min(1e-30)).sqrt()
                K = P["kernel.signal_variance"].abs() * (1 + a + 5.0 / 3.0 * sq) * torch.exp(-a)
        Sigma = K + P["log_beta"].exp().pow(-1) * eye + R.JITTER * eye
        if dv is not None:
            Sigma = Sigma + torch.diag(dv)
        L = torch.linalg.cholesky(Sigma)
        Gamma = torch.linalg.solve_triangular(L, YH - YL @ V.T, upper=False)
        loss = 0.5 * (Gamma ** 2).sum() + L.diag().log().sum() * h + 0.5 * n * h * torch.log(2 * torch.tensor(R.PI_TRUNC))
        loss.backward()
        opt.step()
        trace.append(float(loss.detach()))
    order = [P[k].detach().numpy() for k in names]
    return np.array(trace), order + [V.detach().numpy()]


def bound(delta, bar):
    """10 x the measured distance of two independent fp64 evaluations, floor 1e-12; never beyond the rho route's bar unless delta is"""
    b = max(10.0 * delta, FLOOR)
    return min(b, bar) if delta <= bar else b


# ---------------------------------------------------------------------------------------------------------- 1. the reference fixture
@pytest.mark.parametrize("persist", [1, 0])
def test_train_many_cigar_on_the_reference_fixture(golden, persist):
    """tests/golden/cigar_chain.npz (the reference's train_CIGAR, non-subset, n = 60 / 40 / 30, d = 12, 4 steps per fidelity): fidelity 0
    plain, fidelities 1 and 2 with the Tensor_linear link -- the LL trace, every parameter (both maps included), the res-i sets and
    CIGAR.forward at test_cigar_chain_golden's bars"""
    import mf_harness as H
    from fidelityfusion_amd import _lib, kernel
    from fidelityfusion_amd.cigp_v10 import train_many
    g = golden("cigar_chain")
    model = H.CIGAR(3, [kernel.SquaredExponentialKernel() for _ in range(3)], [(12,)] * 3).double().to(DEV)
    x0, y0 = T(g["x0n"]), T(g["y0n"])
    _lib.set_option("train_persist", persist, 0)
    try:
        tr, st = train_many([model.gpr_list[0]], [x0], [y0], 4, lr=1e-2)
        assert st["fused"]
        traces, data = [tr[0]], [(x0, y0)]
        for i in (1, 2):
            xf = T(g[f"fill{i}_x"])
            res = (model.Tensor_linear_list[i - 1], [T(g[f"fill{i}_ylow_mean"]), T(g[f"fill{i}_ylow_var"])],
                   [T(g[f"fill{i}_yhigh_mean"]), T(g[f"fill{i}_yhigh_var"])])
            tr, st = train_many([model.gpr_list[i]], [xf], [None], 4, lr=1e-2, residual=[res])
            assert st["fused"]
            traces.append(tr[0])
            data.append((xf, st["residual_targets"][0]))
    finally:
        _lib.set_option("train_persist", 1, 0)
    assert rel(-torch.cat(traces), g["ll_trace"]) < 1e-8
    for name, p in model.state_dict().items():
        assert rel(p, g[name.replace(".", "__")]) < 1e-7, name
    for i in (1, 2):
        assert rel(data[i][0], g[f"res{i}_x"]) < 1e-13
        assert rel(data[i][1][0], g[f"res{i}_mean"]) < 1e-8
        assert rel(data[i][1][1], g[f"res{i}_var"]) < 1e-13 or np.abs(g[f"res{i}_var"]).max() == 0.0
    with torch.no_grad():
        yp, vp = model(data, T(g["xtn"]))
    assert rel(yp, g["ypred"]) < 1e-7
    assert rel(vp, g["var_pred"]) < 1e-7


# ------------------------------------------------------------------------------------------------------ 2. against the per-step loop
CASES = [
    (1, 1, 1, 1, "ard", "full", None), (4, 2, 1, 1, "ard", "subset", None), (17, 9, 6, 9, "se", "full", None),
    (32, 2, 1, 1, "ard", "full", None), (100, 16, 12, 12, "matern", "subset", None), (128, 16, 16, 16, "ard", "full", None),
    (128, 2, 4, 16, "matern", "subset", None), (128, 2, 16, 17, "ard", "subset", None), (129, 2, 3, 3, "ard", "full", None),
    (300, 9, 40, 64, "se", "subset", None),
    (300, 9, 40, 64, "se", "subset", 1),      # ... with both products on the fp64 GEMM whatever the switch's default is
    (17, 9, 6, 9, "se", "full", 1),           # ... and the GEMM's MN-major read of the strided bilinear V
]


@pytest.mark.parametrize("n,D,l,h,kind,form,gemm_min", CASES)
def test_train_many_cigar_follows_the_reference_loop(n, D, l, h, kind, form, gemm_min):
    from fidelityfusion_amd import _lib
    from fidelityfusion_amd.cigp_v10 import train_many
    lr = 1e-2
    m, x, res = make_link(n, D, l, h, kind, form, 100 * n + 7 * D + l + h)
    assert (l == h) == res[0].vectors[0].is_contiguous()      # (l < h: the bilinear initialisation's transposed view)
    twin, tres = copy.deepcopy(m), clone_link(res)
    cpu_trace, cpu_pars = cpu_torch_loop(kind, m, x, res, 40, lr)
    if gemm_min is not None:
        _lib.set_option("tlin_gemm_min", gemm_min, 0)
    try:
        trace, state = train_many([m], [x], [None], 25, lr=lr, residual=[res])
        trace2, state = train_many([m], [x], [None], 15, lr=lr, state=state, residual=[res])
    finally:
        if gemm_min is not None:
            _lib.set_option("tlin_gemm_min", 8192, 0)      # (the default: csrc/handle.hip)
    assert state["fused"]
    ref, _, last = reference_cigar_loop(twin, x, tres, 40, lr)
    got_tr = torch.cat([trace, trace2], dim=1)
    assert torch.isfinite(got_tr).all()
    d_tr, e_tr = rel(ref, cpu_trace), rel(got_tr, ref)
    pa, pb = params_of(m, res[0]), params_of(twin, tres[0])
    d_par = [rel(b, c) for b, c in zip(pb, cpu_pars)]
    e_par = [rel(a, b) for a, b in zip(pa, pb)]
    print("TLIN_PARITY case=(%d,%d,%d,%d) %s %s gemm_min=%s delta_trace=%.3e fused_trace=%.3e delta_par=%.3e fused_par=%.3e"
          % (n, D, l, h, kind, form, gemm_min, d_tr, e_tr, max(d_par), max(e_par)))
    assert e_tr <= bound(d_tr, BAR_TRACE), (e_tr, d_tr)
    for e, d in zip(e_par, d_par):
        assert e <= bound(d, BAR_PAR), (e, d)
    got = state["residual_targets"][0]
    want = last if isinstance(last, list) else [last, None]
    assert rel(got[0], want[0]) < 1e-12
    if want[1] is None:
        assert got[1] is None
    else:
        assert rel(got[1], want[1]) < 1e-12
    assert res[0].vectors[0]._version > 0      # (cached posteriors key on the version counters)


# ------------------------------------------------------------------------------------------- 3. one launch = launch per stage
@pytest.mark.parametrize("n,D,l,h,kind,form", [(32, 2, 1, 1, "ard", "full"), (100, 9, 12, 12, "matern", "subset"),
                                               (128, 16, 16, 16, "ard", "full")])
def test_cigar_train_persist_settings_agree(n, D, l, h, kind, form):
    """option train_persist 1 and 0, the Adam state moving between the two in both directions: the same bound rule"""
    from fidelityfusion_amd import _lib
    from fidelityfusion_amd.cigp_v10 import train_many
    runs = {}
    for order in ((1, 0), (0, 1), (0, 0)):
        m, x, res = make_link(n, D, l, h, kind, form, 7 * n + h)
        try:
            _lib.set_option("train_persist", order[0], 0)
            tr1, state = train_many([m], [x], [None], 30, lr=2e-2, residual=[res])
            _lib.set_option("train_persist", order[1], 0)
            tr2, _ = train_many([m], [x], [None], 7, lr=2e-2, state=state, residual=[res])
        finally:
            _lib.set_option("train_persist", 1, 0)
        runs[order] = (torch.cat([tr1, tr2], dim=1).clone(), params_of(m, res[0]))
    twin_m, twin_x, twin_res = make_link(n, D, l, h, kind, form, 7 * n + h)
    cpu_trace, cpu_pars = cpu_torch_loop(kind, twin_m, twin_x, twin_res, 37, 2e-2)
    base = runs[(0, 0)]
    d_tr = rel(base[0], cpu_trace)
    d_par = [rel(a, b) for a, b in zip(base[1], cpu_pars)]
    for order in ((1, 0), (0, 1)):
        assert rel(runs[order][0], base[0]) <= bound(d_tr, BAR_TRACE)
        for a, b, d in zip(runs[order][1], base[1], d_par):
            assert rel(a, b) <= bound(d, BAR_PAR)


# ------------------------------------------------------------------------------------------------------------------- 4. mixed call
def _mixed(seed):
    """one plain model, one rho member and two link members of different (l, h)"""
    from fidelityfusion_amd.cigp_v10 import cigp
    from oracle import gp_oracle as O
    import test_gpu_train_residual as TR
    rng = np.random.default_rng(seed)
    X, Y = O.synthetic_xy(60, 3, 2, seed=seed)
    items = [(cigp(make_kernel("ard", 3, rng), 0.7).double().to(DEV), T(X), T(Y), None)]
    m, x, r = TR.make_residual(45, 2, 1, "se", "full", seed + 1)
    items.append((m, x, None, r))
    for k, (n, D, l, h, kind, form) in enumerate([(50, 3, 2, 5, "matern", "full"), (140, 2, 7, 7, "ard", "subset")]):
        m, x, r = make_link(n, D, l, h, kind, form, seed + 2 + k)
        items.append((m, x, None, r))
    return items


def _all_params(item):
    m, _, _, r = item
    if r is None:
        return params_of(m)
    return params_of(m, r[0]) if isinstance(r[0], torch.nn.Module) else params_of(m) + [r[0].detach().cpu().numpy().copy()]


def test_train_many_mixes_plain_rho_and_link_members():
    from fidelityfusion_amd.cigp_v10 import train_many
    items, solo = _mixed(5), _mixed(5)
    trace, st = train_many([i[0] for i in items], [i[1] for i in items], [i[2] for i in items], 12, residual=[i[3] for i in items])
    assert st["fused"]
    for f, it in enumerate(solo):
        tf, _ = train_many([it[0]], [it[1]], [it[2]], 12, residual=[it[3]])
        assert rel(trace[f], tf[0]) < 1e-12
        for a, b in zip(_all_params(items[f]), _all_params(it)):
            assert rel(a, b) < 1e-12


# --------------------------------------------------------------------------------------------------------------------- 5. failure
@pytest.mark.parametrize("persist", [1, 0])
def test_a_link_member_that_is_not_positive_definite_raises_and_keeps_its_values(persist):
    """A link member's diagonal extra is |diag(v_high) - diag(v_low)|: no finite y_var makes it negative, so through train_many the
    member is made indefinite by a NaN y_var diagonal entry (the factorisation's pivot test is !(pivot > 0)), after three good steps
    that left non-zero moments: LinAlgError naming the member's call; its V, moments and parameters are bit-equal to their values
    before the failing step.  In one-launch form the other member of the call has completed its steps; launch per stage nothing of
    the call has moved.  (The negative entry itself goes through the C entry point, which takes diag_vec from its caller: the next
    test.)  A status path, not a GPU fault: the factorisation reports the pivot and the loop goes on without moving anything."""
    from fidelityfusion_amd import _lib
    from fidelityfusion_amd.cigp_v10 import train_many
    ok_m, ok_x, ok_res = make_link(30, 2, 2, 2, "se", "subset", 12)
    m, x, res = make_link(40, 2, 3, 5, "ard", "full", 11)
    solo_m, solo_x, solo_res = make_link(30, 2, 2, 2, "se", "subset", 12)
    _lib.set_option("train_persist", persist, 0)
    try:
        _, state = train_many([ok_m, m], [ok_x, x], [None, None], 3, residual=[ok_res, res])
        vh = res[2][1].clone()
        vh[5, 5] = float("nan")
        before_ok, before = params_of(ok_m, ok_res[0]), params_of(m, res[0])
        (key, st), = state["chunks"].items()
        assert key == (0, 1)
        moments = st.buf.clone()
        assert bool(moments[0].any()) and bool(moments[1].any())
        with pytest.raises(torch.linalg.LinAlgError, match=r"model.* 1\b"):
            train_many([ok_m, m], [ok_x, x], [None, None], 4, state=state, residual=[ok_res, (res[0], res[1], [res[2][0], vh])])
        _, solo_state = train_many([solo_m], [solo_x], [None], 3, residual=[solo_res])
        if persist:
            train_many([solo_m], [solo_x], [None], 4, state=solo_state, residual=[solo_res])
    finally:
        _lib.set_option("train_persist", 1, 0)
    for a, b in zip(params_of(m, res[0]), before):
        assert np.array_equal(a, b)
    assert torch.equal(st.buf[1], moments[1])
    if persist:      # the other member went on alone: its own 3 + 4 steps
        for a, b in zip(params_of(ok_m, ok_res[0]), params_of(solo_m, solo_res[0])):
            assert rel(a, b) < 1e-12
        assert not torch.equal(st.buf[0], moments[0])
    else:            # the call's members share the status
        for a, b in zip(params_of(ok_m, ok_res[0]), before_ok):
            assert np.array_equal(a, b)
        assert torch.equal(st.buf[0], moments[0])


def test_a_negative_diag_vec_entry_stops_the_c_entry_point_with_nothing_moved():
    """ffgp_train_tlin_raw on a member whose diag_vec has a negative entry large enough to make Sigma indefinite: the pivot status comes
    back, the trace holds NaN, and V, the moments and the three parameters keep their bits"""
    from fidelityfusion_amd import _lib
    rng = np.random.default_rng(3)
    n, D, l, h, steps = 24, 2, 2, 3, 3
    a = _c_member(rng, n, D, l, h)
    a["dvec"][7] = -50.0
    keep = {k: a[k].clone() for k in ("w", "amp", "lb", "V", "st")}
    keep["st"].normal_()
    a["st"].copy_(keep["st"])
    rc = _c_call(a, steps)
    assert rc > 0
    assert torch.isnan(a["trace"]).all()
    for k, v in keep.items():
        assert torch.equal(a[k], v), k


def _c_member(rng, n, D, l, h):
    x, yl, yh = T(rng.uniform(0, 1, (n, D))), T(rng.standard_normal((n, l))), T(rng.standard_normal((n, h)))
    P_ = D + 2 + h * l
    return dict(n=n, D=D, l=l, h=h, x=x, yl=yl, yh=yh, w=T(np.ones(D)), amp=T([1.0]), lb=T([0.6]), V=T(rng.standard_normal((h, l))),
                dvec=T(rng.uniform(0.01, 0.1, n)), st=torch.zeros(2 * P_, dtype=torch.float64, device=DEV), P=P_)


def _c_call(a, steps, l_=None, yl_ptr=None, variant=None, stride=None, sentinel=None):
    from fidelityfusion_amd import _lib
    a["trace"] = torch.full((steps,), -7.0 if sentinel is None else sentinel, dtype=torch.float64, device=DEV)
    p = _lib.Problem()
    p.n, p.D, p.d = a["n"], a["D"], a["h"]
    p.X_dev, p.w_dev, p.amp_dev, p.diag_add_dev = a["x"].data_ptr(), a["w"].data_ptr(), a["amp"].data_ptr(), a["lb"].data_ptr()
    p.diag_vec_dev, p.diag_stride = a["dvec"].data_ptr(), 1
    p.clamp_min, p.ll_variant, p.pi_const, p.kfun, p.kparam = 1e-30, (_lib.FFGP_LL_V1 if variant is None else variant), 3.1415, 0, 1.0
    lk = _lib.Links()
    lk.w_link, lk.w_c, lk.amp_link, lk.dadd_link, lk.dadd_c, lk.out_scale = _lib.LINK_INV_ABS_EPS, 1e-9, _lib.LINK_ABS, _lib.LINK_EXP_NEG, 1e-6, 1.0
    t = _lib.TlinLink()
    t.V_dev, t.l, t.y_high_dev = a["V"].data_ptr(), (a["l"] if l_ is None else l_), a["yh"].data_ptr()
    t.y_low_dev = a["yl"].data_ptr() if yl_ptr is None else yl_ptr
    opt = _lib.Adam(1e-2, 0.9, 0.999, 1e-8)
    rc = _lib.lib.ffgp_train_tlin_raw(_lib.handle(0), 1, C.byref(p), C.byref(lk), C.byref(t), steps, C.byref(opt), a["st"].data_ptr(),
                                      2 * a["P"] if stride is None else stride, 0, a["trace"].data_ptr(), steps)
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------------------------------------------------------- 6. fallbacks
def _hand_loop(m, x, res, steps, lr):
    tr, _, last = reference_cigar_loop(m, x, res, steps, lr)
    return tr, last


@pytest.mark.parametrize("why", ["two_mode", "cpu", "sum_kernel"])
def test_train_many_cigar_runs_the_reference_loop_when_it_cannot_fuse(why):
    """a two-mode Tensor_linear, a CPU model and a SumKernel model: train_many is train_CIGAR's loop itself, same return values"""
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.cigp_v10 import cigp, train_many
    from fidelityfusion_amd.gp_computation_pack import Tensor_linear
    dev = "cpu" if why == "cpu" else DEV
    m, x, res = make_link(20, 2, 4, 4, "ard", "full", 3, dev=dev)
    if why == "sum_kernel":
        m = cigp(kernel.SumKernel(kernel.LinearKernel(2), kernel.MaternKernel(2)), 0.6).double().to(DEV)
    if why == "two_mode":      # (only the last mode's matrix acts: y_low [n, 2, 2] -> [n, 2, 2], flattened by the caller's model shape)
        class Flat(Tensor_linear):
            def forward(self, y):
                return super().forward(y.reshape(-1, 2, 2)).reshape(y.shape[0], -1)
        tl = Flat((2, 2), (2, 2)).double().to(DEV)
        res = (tl, res[1], res[2])
    twin, tres = copy.deepcopy(m), clone_link(res)
    trace, state = train_many([m], [x], [None], 6, residual=[res])
    ref, last = _hand_loop(twin, x, tres, 6, 1e-2)
    assert state["fused"] is False and tuple(trace.shape) == (1, 6) and rel(trace, ref) < 1e-12
    for a, b in zip([p.detach() for p in list(m.parameters()) + list(res[0].parameters())],
                    [p.detach() for p in list(twin.parameters()) + list(tres[0].parameters())]):
        assert rel(a, b) < 1e-12
    got = state["residual_targets"][0]
    assert rel(got[0], last[0]) < 1e-12 and rel(got[1], last[1]) < 1e-12


def test_train_many_refuses_contradicting_arguments():
    from fidelityfusion_amd.cigp_v10 import train_many
    m, x, res = make_link(10, 2, 2, 2, "ard", "subset", 4)
    with pytest.raises(ValueError):
        train_many([m], [x], [res[2]], 2, residual=[res])                                  # a link together with ys[f]
    with pytest.raises(ValueError):
        train_many([m], [x], [None], 2, residual=[res], car=[(res[0], res[1], res[2])])   # car= together with a link


# -------------------------------------------------------------------------------------------------- 7. refusals of the C entry point
def test_refusals_of_the_c_entry_point():
    """l > h, a null y_low_dev, the V2 likelihood on a link member, state_stride one short: FFGP_ERR_ARG, the trace buffer (filled with a
    sentinel) untouched, as are V and the state"""
    from fidelityfusion_amd import _lib
    a = _c_member(np.random.default_rng(0), 20, 2, 2, 3)
    V0 = a["V"].clone()
    for kw in (dict(l_=4), dict(yl_ptr=0), dict(variant=_lib.FFGP_LL_V2), dict(stride=2 * a["P"] - 1)):
        assert _c_call(a, 3, **kw) == -1, kw      # FFGP_ERR_ARG
        assert torch.equal(a["trace"], torch.full_like(a["trace"], -7.0)) and torch.equal(a["V"], V0) and not a["st"].any()
    assert _c_call(a, 3) == 0                      # ... and the accepted call trains
    assert torch.isfinite(a["trace"]).all() and not torch.equal(a["V"], V0)


@pytest.mark.parametrize("persist", [1, 0])
def test_plain_and_link_members_share_a_call_of_the_c_entry_point(persist):
    """t[f].V_dev = NULL is a plain member, trained exactly as ffgp_train_raw trains it: a call of one plain and one link member against
    the two single-member calls (one launch: a workgroup per member, launch per stage: a member's launches do not see its companion)"""
    from fidelityfusion_amd import _lib
    n, D, l, h, steps = 24, 2, 2, 3, 5

    def members():
        rng = np.random.default_rng(8)
        a, b = _c_member(rng, n, D, l, h), _c_member(rng, n, D, l, h)
        b["Y"] = T(rng.standard_normal((n, h)))
        return a, b

    def call(ms):
        F = len(ms)
        P, L, K = (_lib.Problem * F)(), (_lib.Links * F)(), (_lib.TlinLink * F)()
        stride = 2 * ms[0]["P"]
        st = torch.zeros((F, stride), dtype=torch.float64, device=DEV)
        trace = torch.zeros((F, steps), dtype=torch.float64, device=DEV)
        for j, a in enumerate(ms):
            p = P[j]
            p.n, p.D, p.d = n, D, h
            p.X_dev, p.w_dev, p.amp_dev, p.diag_add_dev = a["x"].data_ptr(), a["w"].data_ptr(), a["amp"].data_ptr(), a["lb"].data_ptr()
            p.diag_vec_dev, p.diag_stride = a["dvec"].data_ptr(), 1
            p.clamp_min, p.ll_variant, p.pi_const, p.kfun, p.kparam = 1e-30, _lib.FFGP_LL_V1, 3.1415, 0, 1.0
            lk = L[j]
            lk.w_link, lk.w_c, lk.amp_link, lk.dadd_link, lk.dadd_c, lk.out_scale = _lib.LINK_INV_ABS_EPS, 1e-9, _lib.LINK_ABS, _lib.LINK_EXP_NEG, 1e-6, 1.0
            if "Y" in a:
                p.Y_dev = a["Y"].data_ptr()
            else:
                K[j].V_dev, K[j].l, K[j].y_low_dev, K[j].y_high_dev = a["V"].data_ptr(), l, a["yl"].data_ptr(), a["yh"].data_ptr()
        opt = _lib.Adam(1e-2, 0.9, 0.999, 1e-8)
        rc = _lib.lib.ffgp_train_tlin_raw(_lib.handle(0), F, P, L, K, steps, C.byref(opt), st.data_ptr(), stride, 0, trace.data_ptr(), steps)
        torch.cuda.synchronize()
        assert rc == 0
        return trace, st

    _lib.set_option("train_persist", persist, 0)
    try:
        both = members()
        tr, st = call(list(both))
        solo = members()
        outs = [call([m]) for m in solo]
    finally:
        _lib.set_option("train_persist", 1, 0)
    for j in range(2):
        assert rel(tr[j], outs[j][0][0]) < 1e-12 and rel(st[j], outs[j][1][0]) < 1e-12
        for k in ("w", "amp", "lb", "V"):
            assert rel(both[j][k], solo[j][k]) < 1e-12, (j, k)
    assert torch.equal(both[1]["V"], members()[1]["V"]) and bool(st[1, 2 * (D + 2):].eq(0).all())      # (nothing of a plain member's link is touched; no further moments)
