"""GPU: `cigp_v10.forward_many` / `gp_basic.forward_many` (ffgp_predict_small_batch, csrc/predict_small.hip) -- the posteriors of sets
of small trained models in one launch -- against the torch-CPU restatement of the reference's `cigp.forward`
(oracle.torch_cpu_ref.cigp_forward) and against the per-model path (`m.forward`, covariance diagonal).

THE BAR.  For inputs (x uniform in [0, 1]^D, length scales about 1, noise 1e-2: well conditioned, so that the comparator itself is
stable) the distance d0 of the per-model path from the fp64 CPU comparator is measured, relative to max |value|, for mean and variance
separately; `forward_many` must be within max(10 d0, 1e-12) of the comparator -- and, where a test compares with `m.forward`, within
that of `m.forward`.  For the kernels the oracle does not restate (SE, Matern, GP_basic's noise convention) the comparator is the
same posterior written out in torch on the CPU, cpu_posterior() below.  Every figure is printed before it is asserted.
Bit-for-bit claims (a member alone against the same member in a batch; a point alone against the same point in a longer query; one
split of the tiles against another) are asserted with np.array_equal."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
FLOOR = 1e-12
NOISE = 1e-2
EDGE_SHAPES = [(1, 1, 1, 1), (15, 2, 2, 16), (16, 16, 16, 17), (17, 1, 3, 33), (33, 9, 5, 5), (127, 16, 16, 40), (128, 8, 1, 100)]      # (n, D, d, nt)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(torch.float32)


def T(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)


def rel(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    return float(np.abs(a.reshape(b.shape) - b).max() / max(np.abs(b).max(), 1e-300))


def bits(pairs):
    return [(m.cpu().numpy().copy(), v.cpu().numpy().copy()) for m, v in pairs]


def same_bits(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


def close(a, b, tol=1e-10):
    """the same per-model path run twice (a fresh factor, then the cached one) agrees to rounding, not to the bit"""
    return rel(a[0], b[0]) < tol and rel(a[1], b[1]) < tol


def data(n, D, d, nt, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, D))
    W = rng.uniform(0.5, 2.0, (D, d))
    Y = np.sin(2.0 * X @ W) + 0.05 * rng.standard_normal((n, d))
    return X, Y, rng.uniform(0, 1, (nt, D)), rng


def ard_member(n, D, d, nt, seed):
    """(model on the GPU, x, y, x_test, the oracle's arguments on the CPU)"""
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.cigp_v10 import cigp
    X, Y, Xs, rng = data(n, D, d, nt, seed)
    ls = rng.uniform(0.7, 1.4, D) * rng.choice([-1.0, 1.0], D)
    sv, lb = [-0.9], [float(np.log(1.0 / NOISE))]
    k = kernel.ARDKernel(D)
    with torch.no_grad():
        k.length_scales.copy_(torch.tensor(ls))
        k.signal_variance.copy_(torch.tensor(sv))
    m = cigp(k, lb[0]).double().to(DEV)
    cpu = tuple(torch.tensor(np.asarray(a), dtype=torch.float64) for a in (X, Y, Xs, ls, sv, lb))
    return m, T(X), T(Y), T(Xs), cpu


def oracle_diag(cpu):
    from oracle import torch_cpu_ref as R
    mean, var = R.cigp_forward(*cpu)
    return mean.numpy(), var.diagonal().numpy().reshape(-1, 1)


def loop_diag(m, x, y, xt):
    """the existing per-model path: `m.forward` under no_grad, the covariance reduced to its diagonal"""
    with torch.no_grad():
        mean, cov = m(x, y, xt)
    return mean.reshape(xt.shape[0], -1), cov.diagonal().reshape(-1, 1)


def within_bar(what, got, loop, ref, against_loop=False):
    """prints the figures, then asserts: got within max(10 d0, FLOOR) of the comparator (and of the per-model path), d0 = the per-model
    path's own distance from the comparator; mean and variance separately.  Returns the figures."""
    out = []
    for name, g, l, r in (("mean", got[0], loop[0], ref[0]), ("var", got[1], loop[1], ref[1])):
        d0, d1, dl = rel(l, r), rel(g, r), rel(g, l)
        bar = max(10.0 * d0, FLOOR)
        print("%s %s: per-model path vs comparator %.3e, forward_many vs comparator %.3e, vs per-model path %.3e, bar %.3e" % (what, name, d0, d1, dl, bar))
        out.append((name, d0, d1, dl, bar))
    for name, d0, d1, dl, bar in out:
        assert d1 <= bar, (what, name, d1, bar)
        if against_loop:
            assert dl <= bar, (what, name, dl, bar)
    return out


@pytest.fixture(scope="module")
def edge():
    """the seven edge-shape members, their comparator values and the per-model path's results: computed once, never modified"""
    members = [ard_member(n, D, d, nt, 7000 + 100 * n + D) for (n, D, d, nt) in EDGE_SHAPES]
    refs = [oracle_diag(mb[4]) for mb in members]
    loops = [bits([loop_diag(*mb[:4])])[0] for mb in members]
    return members, refs, loops


def edge_shape_figures(members, refs, loops):
    """the edge-shape check, shared with the child process that repeats it under forced helper-wave placements
    (tests/forward_many_roles_child.py): all seven in one call, each alone, bit-identical either way, every member fused, the bar"""
    from fidelityfusion_amd.cigp_v10 import forward_many
    ms, xs, ys, xts = ([mb[i] for mb in members] for i in range(4))
    st = {}
    batch = bits(forward_many(ms, xs, ys, xts, st))
    assert st["fused"] == list(range(len(members))) and st["status"] == [0] * len(members), st
    figures = []
    for f, (n, D, d, nt) in enumerate(EDGE_SHAPES):
        st1 = {}
        alone = bits(forward_many([ms[f]], [xs[f]], [ys[f]], [xts[f]], st1))[0]
        assert st1["fused"] == [0], (EDGE_SHAPES[f], st1)
        assert batch[f][0].shape == (nt, d) and batch[f][1].shape == (nt, 1)
        assert same_bits(alone, batch[f]), "member %s differs between the batch and a call of its own" % (EDGE_SHAPES[f],)
        figures.append(within_bar("n=%d D=%d d=%d nt=%d" % (n, D, d, nt), batch[f], loops[f], refs[f]))
    return batch, figures


def test_edge_shapes_in_one_call_and_alone(edge):
    edge_shape_figures(*edge)


def test_results_are_views_of_one_allocation(edge):
    from fidelityfusion_amd.cigp_v10 import forward_many
    members = edge[0]
    out = forward_many(*([mb[i] for mb in members] for i in range(4)))
    base = out[0][0].untyped_storage().data_ptr()
    assert all(t.untyped_storage().data_ptr() == base for pair in out for t in pair)


def test_a_point_does_not_depend_on_its_tile_or_on_the_split(edge, monkeypatch):
    """the first 16 points of an nt = 40 query, and points 16..39 as a query of their own (other tiles, other columns), bit for bit; the
    tiles of every member dealt to ONE workgroup and to as many as there are tiles (FFGP_PREDICT_SPLIT, read at every call)"""
    from fidelityfusion_amd.cigp_v10 import forward_many
    m, x, y, xt, _ = edge[0][5]      # n = 127, nt = 40
    assert xt.shape[0] == 40
    full = bits(forward_many([m], [x], [y], [xt]))[0]
    head = bits(forward_many([m], [x], [y], [xt[:16].contiguous()]))[0]
    tail = bits(forward_many([m], [x], [y], [xt[16:].contiguous()]))[0]
    one = bits(forward_many([m], [x], [y], [xt[21:22].contiguous()]))[0]
    assert same_bits(head, (full[0][:16], full[1][:16]))
    assert same_bits(tail, (full[0][16:], full[1][16:]))
    assert same_bits(one, (full[0][21:22], full[1][21:22]))
    args = [[mb[i] for mb in edge[0]] for i in range(4)]
    auto = bits(forward_many(*args))
    for split in ("1", "2", "1000"):      # (the library caps it at the largest member's tiles: 7)
        monkeypatch.setenv("FFGP_PREDICT_SPLIT", split)
        forced = bits(forward_many(*args))
        for f in range(len(auto)):
            assert same_bits(forced[f], auto[f]), (split, EDGE_SHAPES[f])
    monkeypatch.delenv("FFGP_PREDICT_SPLIT")


# ---- the posterior written out in torch on the CPU, for the kernels the oracle does not restate
PHI = {
    "se": lambda s, rho: torch.exp(-0.5 * s),
    "m12": lambda s, rho: torch.exp(-torch.sqrt(s) / rho),
    "m32": lambda s, rho: (1.0 + torch.sqrt(3.0 * s) / rho) * torch.exp(-torch.sqrt(3.0 * s) / rho),
    "m52": lambda s, rho: (1.0 + torch.sqrt(5.0 * s) / rho + (5.0 / 3.0) * s / rho ** 2) * torch.exp(-torch.sqrt(5.0 * s) / rho),
}


def cpu_posterior(phi, rho, X, Y, Xs, w, amp, diag_add, var_add):
    """mean and variance diagonal of the GP with K = amp phi(|w (x - x')|^2), Sigma = K + diag_add I (cigp_v10.py:24-48, gp_basic.py:78-84)"""
    X, Y, Xs, w = (torch.as_tensor(a, dtype=torch.float64).cpu() for a in (X, Y, Xs, w))
    # (the squared distance from the differences themselves: cdist's matrix-product form loses it to cancellation between near
    #  points, and Matern 1/2 takes its square root)
    K = lambda a, b: amp * phi((((a[:, None, :] - b[None, :, :]) * w) ** 2).sum(-1), rho)
    L = torch.linalg.cholesky(K(X, X) + diag_add * torch.eye(X.shape[0]))
    ks = K(X, Xs)
    V = torch.linalg.solve_triangular(L, ks, upper=False)
    mean = ks.t() @ torch.cholesky_solve(Y, L)
    var = K(Xs, Xs).diagonal() - (V * V).sum(0) + var_add
    return mean.numpy(), var.numpy().reshape(-1, 1)


def kernel_member(kind, n, D, d, nt, seed):
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.cigp_v10 import JITTER, cigp
    X, Y, Xs, rng = data(n, D, d, nt, seed)
    lb = float(np.log(1.0 / NOISE))
    if kind == "se":
        k = kernel.SquaredExponentialKernel(0.1, -0.2)
        w, amp, phi, rho = np.exp(-0.1), np.exp(-0.2) ** 2, PHI["se"], 1.0
    elif kind == "rq":
        k = kernel.RationalQuadraticKernel(1.1, 0.9, 1.5)
        w, amp, phi, rho = None, None, None, None
    else:
        ls = rng.uniform(0.7, 1.4, D)
        if kind == "ard":
            k, phi, rho = kernel.ARDKernel(D), PHI["se"], 1.0
        else:
            nu, rho = {"m12": 0.5, "m32": 1.5, "m52": 2.5}[kind], 1.3
            k, phi = kernel.MaternKernel(D, nu=nu, rho=rho), PHI[kind]
        with torch.no_grad():
            k.length_scales.copy_(torch.tensor(ls))
            k.signal_variance.copy_(torch.tensor([0.8]))
        w, amp = 1.0 / (np.abs(ls) + k.eps), 0.8
    m = cigp(k, lb).double().to(DEV)
    ref = None if phi is None else cpu_posterior(phi, rho, X, Y, Xs, w, amp, NOISE + JITTER, NOISE)
    return m, T(X), T(Y), T(Xs), ref


def test_one_member_per_kernel():
    """SE (scalar log parameters, no clamp), ARD, Matern 1/2, 3/2 and 5/2 with rho = 1.3 in ONE call, each against `m.forward` at the bar.
    A RationalQuadraticKernel's alpha is an nn.Parameter -- the trainer's assembly takes a profile parameter as a constant only -- so
    its member runs its own forward, in the caller's order"""
    from fidelityfusion_amd.cigp_v10 import forward_many
    kinds = ["se", "ard", "rq", "m12", "m32", "m52"]
    members = [kernel_member(k, 50 + 9 * i, 3, 2, 37, 8100 + i) for i, k in enumerate(kinds)]
    st = {}
    got = bits(forward_many(*([mb[i] for mb in members] for i in range(4)), st))
    assert st["fused"] == [0, 1, 3, 4, 5] and st["status"] == [0] * 6, st
    for f, kind in enumerate(kinds):
        loop = bits([loop_diag(*members[f][:4])])[0]
        if kind == "rq":
            assert close(got[f], loop)          # the very same path
        else:
            within_bar(kind, got[f], loop, members[f][4], against_loop=True)


def params_and_caches(models):
    return [[p.detach().cpu().numpy().copy() for p in m.parameters()] + [id(m._pcache.posterior)] for m in models]


def test_after_train_many_sixteen_models():
    """the sweep's shape: sixteen N = 64 models trained 20 steps in one launch, predicted in one launch; against the per-model forward
    at the bar, with the models' parameters and posterior caches as the call found them"""
    from fidelityfusion_amd.cigp_v10 import forward_many, train_many
    members = [ard_member(64, 3, 1 + f % 2, 100, 8300 + f) for f in range(16)]
    ms, xs, ys, xts = ([mb[i] for mb in members] for i in range(4))
    train_many(ms, xs, ys, 20, lr=1e-2)
    before = params_and_caches(ms)
    st = {}
    got = bits(forward_many(ms, xs, ys, xts, st))
    assert st["fused"] == list(range(16)) and st["status"] == [0] * 16
    after = params_and_caches(ms)
    for a, b in zip(before, after):
        assert a[-1] == b[-1] and all(np.array_equal(p, q) for p, q in zip(a[:-1], b[:-1]))
    worst = 0.0
    for f, (m, x, y, xt, cpu) in enumerate(members):
        trained = cpu[:3] + tuple(p.detach().cpu() for p in (m.kernel.length_scales, m.kernel.signal_variance, m.log_beta))
        fig = within_bar("trained model %d" % f, got[f], bits([loop_diag(m, x, y, xt)])[0], oracle_diag(trained), against_loop=True)
        worst = max(worst, max(r[3] for r in fig))
    print("sixteen trained models: largest distance from the per-model path %.3e" % worst)


def test_gp_basic_members():
    """GP_basic: Sigma = K + noise_variance^2 I, nothing added to the variance; a FidelityKernelMCMC block has no links of its own, so
    its member runs GP_basic.forward; the mean comes back as [nt, d]"""
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.gp_basic import GP_basic, forward_many
    X, Y, Xs, rng = data(70, 2, 2, 45, 8500)
    ls = rng.uniform(0.7, 1.4, 2)
    k = kernel.ARDKernel(2)
    with torch.no_grad():
        k.length_scales.copy_(torch.tensor(ls))
        k.signal_variance.copy_(torch.tensor([0.8]))
    plain = GP_basic(k, 0.1).double().to(DEV)
    X2, Y2, Xs2, _ = data(40, 2, 1, 20, 8501)
    fk = kernel.FidelityKernelMCMC(1, kernel.ARDKernel(2), 0.0, 1.0, torch.tensor(1.0))
    car = GP_basic(fk, 0.1).double().to(DEV)
    st = {}
    got = bits(forward_many([plain, car], [T(X), T(X2)], [T(Y), T(Y2)], [T(Xs), T(Xs2)], st))
    assert st["fused"] == [0], st
    assert got[0][0].shape == (45, 2) and got[0][1].shape == (45, 1) and got[1][0].shape == (20, 1) and got[1][1].shape == (20, 1)
    with torch.no_grad():
        mu, cov = plain(T(X), T(Y), T(Xs))
        mu2, cov2 = car(T(X2), T(Y2), T(Xs2))
    loop = bits([(mu.reshape(45, 2), cov.diagonal().reshape(-1, 1))])[0]
    ref = cpu_posterior(PHI["se"], 1.0, X, Y, Xs, 1.0 / (np.abs(ls) + k.eps), 0.8, 0.1 ** 2, 0.0)
    within_bar("GP_basic", got[0], loop, ref, against_loop=True)
    assert close(got[1], bits([(mu2.reshape(20, 1), cov2.diagonal().reshape(-1, 1))])[0])


def test_a_member_that_is_not_positive_definite_stops_alone():
    """One member of three whose Sigma is not positive definite.  tests/test_gpu_train.py::test_one_launch_trainer_stops_only_the_model_
    that_failed makes its failing model with a y_var of -3 I; the predict paths drop y_var (cigp_v10.py:31-32), so no `cigp` reaches a
    Sigma that is not positive definite this way, and the same -3 goes in as the member's diag_add through the C entry (effective
    parameters, links == NULL).  That member: its status the failing pivot, NaN everywhere; the other two: bit for bit a call without it."""
    from fidelityfusion_amd import _lib
    h = _lib.handle(0, 0)
    _lib.bind_stream(h, 0)
    shapes = [(50, 2, 1, 30), (90, 3, 2, 40), (128, 2, 2, 25)]
    keep, rows = [], []
    for f, (n, D, d, nt) in enumerate(shapes):
        X, Y, Xs, _ = data(n, D, d, nt, 8700 + f)
        t = [T(X), T(Y), T(Xs), T(np.full(D, 1.1)), T([0.8]), T([-3.0 if f == 1 else NOISE]), torch.zeros(nt * d, device=DEV), torch.zeros(nt, device=DEV)]
        keep.append(t)
        rows.append((n, D, d, nt))

    def call(idx):
        F_ = len(idx)
        P, M = (_lib.Problem * F_)(), (_lib.PredictMember * F_)()
        for k, f in enumerate(idx):
            n, D, d, nt = rows[f]
            X, Y, Xs, w, amp, dadd, mean, var = keep[f]
            mean.fill_(7.0)
            var.fill_(7.0)
            P[k].n, P[k].D, P[k].d = n, D, d
            P[k].X_dev, P[k].Y_dev, P[k].w_dev, P[k].amp_dev, P[k].diag_add_dev = (t.data_ptr() for t in (X, Y, w, amp, dadd))
            P[k].clamp_min, P[k].kfun, P[k].kparam = 1e-30, 0, 1.0
            M[k].Xs_dev, M[k].nt, M[k].mean_dev, M[k].var_dev, M[k].var_add_noise = Xs.data_ptr(), nt, mean.data_ptr(), var.data_ptr(), 1
        torch.cuda.synchronize()
        status = (C.c_int * F_)()
        rc = _lib.lib.ffgp_predict_small_batch(h, F_, P, None, M, status)
        return rc, list(status), [(keep[f][6].cpu().numpy().copy(), keep[f][7].cpu().numpy().copy()) for f in idx]

    rc, status, out = call([0, 1, 2])
    assert status[0] == 0 and status[2] == 0 and 1 <= status[1] <= 90 and rc == status[1], (rc, status)
    assert np.isnan(out[1][0]).all() and np.isnan(out[1][1]).all()
    rc2, status2, out2 = call([0, 2])
    assert rc2 == 0 and status2 == [0, 0]
    assert same_bits(out[0], out2[0]) and same_bits(out[2], out2[1])
    assert np.isfinite(out[0][0]).all() and np.isfinite(out[2][1]).all() and (out[0][1] > 0).all()
    # argument errors: nothing is written
    n, D, d, nt = rows[0]
    rc3, _, out3 = call([0])
    assert rc3 == 0
    for bad in ("n", "nt", "F", "null"):
        P, M = (_lib.Problem * 1)(), (_lib.PredictMember * 1)()
        X, Y, Xs, w, amp, dadd, mean, var = keep[0]
        mean.fill_(7.0)
        P[0].n, P[0].D, P[0].d = (129 if bad == "n" else n), D, d
        P[0].X_dev, P[0].Y_dev, P[0].w_dev, P[0].amp_dev, P[0].diag_add_dev = (t.data_ptr() for t in (X, Y, w, amp, dadd))
        P[0].clamp_min, P[0].kfun, P[0].kparam = 1e-30, 0, 1.0
        M[0].Xs_dev, M[0].nt, M[0].mean_dev, M[0].var_dev = Xs.data_ptr(), (0 if bad == "nt" else nt), (None if bad == "null" else mean.data_ptr()), var.data_ptr()
        assert _lib.lib.ffgp_predict_small_batch(h, 0 if bad == "F" else 1, P, None, M, None) == _lib.FFGP_ERR_ARG, bad
        torch.cuda.synchronize()
        assert (mean == 7.0).all(), bad


def test_a_cigp_that_is_not_positive_definite_raises_or_reports():
    """through the module: a NaN noise parameter makes every pivot fail.  With a state dict the member comes back NaN with its status;
    without one the call raises what the per-model loop raises"""
    from fidelityfusion_amd.cigp_v10 import forward_many
    members = [ard_member(30, 2, 1, 20, 8800 + f) for f in range(3)]
    with torch.no_grad():
        members[1][0].log_beta.fill_(float("nan"))
    args = [[mb[i] for mb in members] for i in range(4)]
    st = {}
    got = bits(forward_many(*args, st))
    assert st["status"][0] == 0 and st["status"][2] == 0 and st["status"][1] > 0
    assert np.isnan(got[1][0]).all() and np.isnan(got[1][1]).all()
    rest = bits(forward_many(*[[a[0], a[2]] for a in args]))
    assert same_bits(got[0], rest[0]) and same_bits(got[2], rest[1])
    with pytest.raises(torch.linalg.LinAlgError):
        forward_many(*args)


def test_mixed_routing():
    """a 129-point model and a SumKernel model among fused ones: theirs are the per-model results, the others' the fused ones (those of
    a call without the two), and state["fused"] says which"""
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.cigp_v10 import cigp, forward_many
    a, b, c = ard_member(60, 2, 1, 33, 8900), ard_member(129, 2, 1, 20, 8901), ard_member(128, 4, 3, 50, 8902)
    X, Y, Xs, _ = data(40, 2, 1, 18, 8903)
    comp = cigp(kernel.SumKernel(kernel.ARDKernel(2), kernel.MaternKernel(2)), float(np.log(1.0 / NOISE))).double().to(DEV)
    s = (comp, T(X), T(Y), T(Xs))
    members = [b, a, s, c]
    args = [[mb[i] for mb in members] for i in range(4)]
    st = {}
    got = bits(forward_many(*args, st))
    assert st["fused"] == [1, 3] and st["status"] == [0, 0, 0, 0]
    only = bits(forward_many(*[[x[1], x[3]] for x in args]))
    assert same_bits(got[1], only[0]) and same_bits(got[3], only[1])
    for f in (0, 2):
        assert close(got[f], bits([loop_diag(*members[f][:4])])[0])


def test_the_reference_resgp_prediction(golden):
    """tests/golden/forward_many_resgp.npz (gen_forward_many_goldens.py): the reference's train_ResGP at exp_aligned.py's sizes -- 100
    low- and 16 high-fidelity points, 100 test points, D = 2 -- and its ResGP.forward.  The trained parameters go into two `cigp`s, both
    fidelities are predicted by ONE forward_many call and summed as ResGP.forward sums them (ResGP.py:48-63); mean and covariance
    diagonal to 1e-8, the bound test_gpu_parity.py::test_resgp_chain_golden holds the per-step modules to"""
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.cigp_v10 import cigp, forward_many
    g = golden("forward_many_resgp")
    gprs = [cigp(kernel.SquaredExponentialKernel(), 1.0).double().to(DEV) for _ in range(2)]
    with torch.no_grad():
        for f, m in enumerate(gprs):
            m.log_beta.copy_(T(g["gpr_list__%d__log_beta" % f]))
            m.kernel.length_scale.copy_(T(g["gpr_list__%d__kernel__length_scale" % f]))
            m.kernel.signal_variance.copy_(T(g["gpr_list__%d__kernel__signal_variance" % f]))
    xt = T(g["xtn"])
    st = {}
    (m0, v0), (m1, v1) = forward_many(gprs, [T(g["x0n"]), T(g["x_res"])], [T(g["y0n"]), T(g["y_res_mean"])], [xt, xt], st)
    assert st["fused"] == [0, 1]
    e_mean, e_var = rel(m0 + m1, g["ypred"]), rel((v0 + v1).reshape(-1), g["var_pred_diag"])
    print("ResGP fixture: mean %.3e, covariance diagonal %.3e (bound 1e-8)" % (e_mean, e_var))
    assert e_mean < 1e-8 and e_var < 1e-8
