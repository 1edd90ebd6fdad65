"""The acquisition optimiser's Adam loop on a frozen posterior in one launch (ffgp_acq_optimize, csrc/acq.hip;
Posterior.optimize_acquisition; acq.optimize_acqf) against plain fp64 torch on the CPU written here from the reference's formulas
(Bayesian_optimization/acq.py:48-68,132-144,161-181): kernel, Cholesky, solve_triangular, autograd, torch.optim.Adam.

Bars.  Evaluate mode (steps = 0): values rel. 1e-10, gradients rel. 1e-8 -- the project's bars for likelihood values and gradients
(`rel` = largest absolute difference over the largest absolute reference entry, the metric of the other GPU suites).
Trajectories: two references that do not contain the new code -- (A) the CPU loop, (B) the per-step loop on the GPU, `predict_diff`
plus torch.optim.Adam -- differ by rounding only; d0 = their distance, computed here, is the yardstick and max(10 d0, 1e-12) the bound
(the decade test_gpu_train_tree.py grants a different summation order).  A case with d0 > 1e-10 is ill-conditioned: the test fails
rather than widening anything.  Before anything is compared, a CPU twin started one ulp away (X0 (1 + 2e-16)) must stay within 1e-11.
Where a fall-back is compared with loop B (the same launches in the same order) the bar is 1e-12; where a selected point is compared
across the fused call and loop B, the same d0 rule holds, with the CPU loop run on that model's own effective parameters."""
import ctypes as C
import functools
import math

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
SE, M12, M32, M52, RQ, LINEAR = 0, 1, 2, 3, 4, 5
NEG_INF = float("-inf")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(torch.float32)


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a.reshape(b.shape) - b).abs().max() / max(float(b.abs().max()), 1e-300))


# ---- the comparator: plain torch on the CPU ---------------------------------------------------------------------------------------
def profile(kfun, kparam, s):
    if kfun == SE:
        return torch.exp(-0.5 * s)
    if kfun == M12:
        return torch.exp(-torch.sqrt(s) / kparam)
    if kfun == M32:
        a = torch.sqrt(3.0 * s) / kparam
        return (1.0 + a) * torch.exp(-a)
    if kfun == M52:
        a = torch.sqrt(5.0 * s) / kparam
        return (1.0 + a + a * a / 3.0) * torch.exp(-a)
    return (1.0 + s / (2.0 * kparam)) ** (-kparam)


def kern(A, B, c):
    d = (A * c["w"]).unsqueeze(1) - (B * c["w"]).unsqueeze(0)
    s = (d * d).sum(-1)
    if c["clamp"] != NEG_INF:
        s = torch.clamp_min(s, c["clamp"])
    return c["amp"] * profile(c["kfun"], c["kparam"], s)


def acq_torch(mean, var, sp):
    """mean [Q, d], var [Q]: the acquisition per point and output (d = 1 everywhere but in the fall-back of several outputs)"""
    var = var.reshape(-1, 1)
    if sp["acq"] == "ucb":
        return mean + sp["kappa"] * torch.sqrt(torch.clamp_min(var, sp["var_floor"]))
    s = torch.clamp(torch.sqrt(var), min=1e-9)
    u = mean - sp["f_best"] - sp["xi"]
    Z = (u / s).detach()
    return u * (0.5 * torch.erfc(-Z / math.sqrt(2.0))) + s * (torch.exp(-0.5 * Z * Z) / math.sqrt(2.0 * math.pi))


def spec(acq="ucb", kappa=2.0, xi=0.01, f_best=0.0, var_add=0.0, var_floor=1e-12):
    return {"acq": acq, "kappa": kappa, "xi": xi, "f_best": f_best, "var_add": var_add, "var_floor": var_floor}


def make_case(n, D, Q, kfun, noise, seed, ard=True, kparam=1.0, clamp=NEG_INF, d=1):
    """the issue's recipe: X = 2 rand, y = sin(2 sum X) + 0.1 randn, w = 0.6 + rand, amp = 1.3, Sigma = K + (noise + 1e-6) I, X0 = 2 rand"""
    g = torch.Generator().manual_seed(seed)
    X = 2.0 * torch.rand(n, D, generator=g)
    y = torch.sin(2.0 * X.sum(1)) + 0.1 * torch.randn(n, generator=g)
    w = 0.6 + torch.rand(D, generator=g)
    if not ard:
        w = w[:1].expand(D).clone()
    X0 = 2.0 * torch.rand(Q, D, generator=g)
    Y = y.reshape(n, 1)
    if d > 1:
        Y = torch.cat([Y] + [torch.cos((j + 2.0) * X.sum(1)).reshape(n, 1) for j in range(d - 1)], 1)
    c = {"X": X, "Y": Y, "w": w, "ard": ard, "amp": 1.3, "kfun": kfun, "kparam": kparam, "clamp": clamp, "dadd": noise + 1e-6, "X0": X0}
    return c


def cpu_factor(c):
    if "L" not in c:
        S = kern(c["X"], c["X"], c) + c["dadd"] * torch.eye(c["X"].shape[0])
        c["L"] = torch.linalg.cholesky(S)
        c["alpha"] = torch.cholesky_solve(c["Y"], c["L"])
    return c


def cpu_predict(c, Xq, var_add):
    cpu_factor(c)
    Ks = kern(c["X"], Xq, c)
    mean = Ks.T @ c["alpha"]
    V = torch.linalg.solve_triangular(c["L"], Ks, upper=False)
    return mean, c["amp"] - (V * V).sum(0) + var_add


def cpu_eval(c, Xq, sp):
    X = Xq.clone().requires_grad_(True)
    mean, var = cpu_predict(c, X, sp["var_add"])
    a = acq_torch(mean, var, sp)
    (-a.sum()).backward()
    return a.detach().sum(1), X.grad, mean.detach(), var.detach()


def run_loop(predict, X0, sp, steps, lr):
    """the reference's loop (acq.py:51-61) on `predict`; trace[k] = the values before step k's update, hist[k] = X before step k"""
    X = X0.clone().requires_grad_(True)
    opt = torch.optim.Adam([X], lr=lr)
    trace, hist = [], []
    for _ in range(steps):
        opt.zero_grad()
        mean, var = predict(X)
        a = acq_torch(mean, var, sp)
        (-a.sum()).backward()
        hist.append(X.detach().clone())
        trace.append(a.detach().sum(1))
        opt.step()
    hist.append(X.detach().clone())
    return X.detach().clone(), torch.stack(trace), torch.stack(hist)


def loop_a(c, X0, sp, steps, lr):
    return run_loop(lambda X: cpu_predict(c, X, sp["var_add"]), X0.cpu(), sp, steps, lr)


def loop_b(post, X0, sp, steps, lr):
    """today's per-step loop on the GPU: Posterior.predict_diff + torch.optim.Adam"""
    return run_loop(lambda X: post.predict_diff(X, full_cov=False, var_add_all=sp["var_add"]), X0.to(DEV), sp, steps, lr)


def distance(r, ref):
    """the metric of every trajectory comparison here: the largest of rel(trace) and rel(hist) (the final X is hist[-1])"""
    return max(rel(r[1], ref[1]), rel(r[2], ref[2]))


def select(X0, trace, hist):
    """acq.py:52-66, restated: the index whose updated X is kept (-1: X0) and that X"""
    losses = [-float(t.sum()) for t in trace]
    best, kbest = losses[0], -1
    for k, v in enumerate(losses):
        if v < best:
            best, kbest = v, k
    return kbest, (X0 if kbest < 0 else hist[kbest + 1])


# ---- the GPU side --------------------------------------------------------------------------------------------------------------------
def gpu_posterior(c, n=None):
    from fidelityfusion_amd import functional as F
    n = n or c["X"].shape[0]
    w = c["w"] if c["ard"] else c["w"][:1]
    return F.Posterior(c["X"][:n].to(DEV), c["Y"][:n].to(DEV), w.to(DEV), torch.tensor([c["amp"]], device=DEV),
                       torch.tensor([c["dadd"]], device=DEV), clamp=c["clamp"], kfun=(c["kfun"], c["kparam"]))


def raw_call(post, Xq, sp, steps=0, lr=0.1, step0=0, Q=None, null=(), **over):
    """ffgp_acq_optimize through ctypes on the posterior's own buffers; `over` overrides fields of the problem, `null` names
    pointers to pass as NULL.  Returns (status, X, state, trace, hist, grad) -- every buffer pre-filled with a sentinel."""
    from fidelityfusion_amd import _lib
    if post.alpha is None:
        post._solve_alpha()
    alpha = post.alpha.reshape(-1).contiguous()
    Qn, D = Xq.shape
    X = Xq.to(DEV).clone().contiguous()
    state = torch.zeros((2, Qn, D), device=DEV)
    trace = torch.full((max(steps, 1), Qn), -7.0, device=DEV)
    hist = torch.full((max(steps, 0) + 1, Qn, D), -7.0, device=DEV)
    grad = torch.full((Qn, D), -7.0, device=DEV)
    f = dict(n=post.n, D=post.D, d=1, X_dev=post.X.data_ptr(), L_dev=post.W.data_ptr(), ldl=post.ld, alpha_dev=alpha.data_ptr(),
             w_dev=post.w.data_ptr(), amp_dev=post.amp.data_ptr(), clamp_min=float(post.clamp), kfun=int(post.kfun[0]),
             kparam=float(post.kfun[1]), var_add_all=sp["var_add"], var_floor=sp["var_floor"],
             acq=_lib.FFGP_ACQ_UCB if sp["acq"] == "ucb" else _lib.FFGP_ACQ_EI, kappa=sp["kappa"], xi=sp["xi"], f_best=sp["f_best"])
    f.update(over)
    p = _lib.AcqProblem(**f)
    opt = _lib.Adam(lr, 0.9, 0.999, 1e-8)
    ptr = lambda name, t: None if name in null else C.c_void_p(t.data_ptr())
    rc = _lib.lib.ffgp_acq_optimize(None if "h" in null else post._h(), None if "p" in null else C.byref(p), ptr("X", X),
                                    Qn if Q is None else Q, steps, None if "opt" in null else C.byref(opt), ptr("state", state), step0,
                                    ptr("trace", trace), ptr("hist", hist), ptr("grad", grad))
    torch.cuda.synchronize()
    return rc, X, state, trace, hist, grad


# ---- values and gradients (steps = 0) against CPU autograd ----------------------------------------------------------------------------
KF = {SE: 1.0, M12: 1.3, M32: 1.3, M52: 0.8, RQ: 1.7}      # kfun -> kparam
NS = [1, 15, 16, 17, 128, 129, 255, 256]
QS = [1, 15, 16, 17, 37]
DS = [1, 3, 16]


def eval_cases():
    cases = []
    # every n, with Q / D / profile / length-scale form / acquisition rotating through all their values
    for i, n in enumerate(NS):
        cases.append((n, QS[i % 5], DS[i % 3], i % 5, bool(i % 2), "ucb" if i % 2 == 0 else "ei"))
        cases.append((n, QS[(i + 2) % 5], DS[(i + 1) % 3], (i + 3) % 5, bool((i + 1) % 2), "ei" if i % 2 == 0 else "ucb"))
    # every profile x scalar / ARD length scale x UCB / EI
    for kfun in (SE, M12, M32, M52, RQ):
        for ard in (False, True):
            for acq in ("ucb", "ei"):
                cases.append((129, 37, 3, kfun, ard, acq))
    # every Q x D
    for Q in QS:
        for D in DS:
            cases.append((17, Q, D, (Q + D) % 5, bool(Q % 2), "ucb" if D != 3 else "ei"))
    return cases


def check_eval(c, sp, Xq):
    post = gpu_posterior(c)
    rc, X, _, trace, _, grad = raw_call(post, Xq, sp)
    assert rc == 0
    assert torch.equal(X.cpu(), Xq)      # evaluate mode: nothing moves
    a, g, mean, var = cpu_eval(c, Xq, sp)
    ev, eg = rel(trace[0], a), rel(grad, g)
    print("n=%d Q=%d D=%d kfun=%d acq=%s: value rel %.2e, gradient rel %.2e" % (c["X"].shape[0], Xq.shape[0], Xq.shape[1], c["kfun"],
                                                                               sp["acq"], ev, eg))
    assert ev <= 1e-10, ev
    assert eg <= 1e-8, eg
    return a, g, mean, var


@pytest.mark.parametrize("n,Q,D,kfun,ard,acq", eval_cases())
def test_evaluate_matches_cpu_autograd(n, Q, D, kfun, ard, acq):
    c = make_case(n, D, Q, kfun, 0.05, seed=1000 + 7 * n + Q + D, ard=ard, kparam=KF[kfun], clamp=1e-30 if kfun in (M12, M32, M52) else NEG_INF)
    check_eval(c, spec(acq, f_best=0.3, var_add=0.05), c["X0"])


def test_evaluate_with_points_on_and_off_the_variance_floor():
    c = make_case(129, 3, 37, SE, 0.05, seed=77)
    sp = spec("ucb", var_floor=0.5, var_add=0.05)
    Xq = c["X0"].clone()
    Xq[18:] = 3.0 + 2.0 * Xq[18:]      # half of the points outside the data's box: their variance is near amp, above the floor
    _, g, _, var = check_eval(c, sp, Xq)
    below = var < 0.5
    assert bool(below.any()) and bool((~below).any()), var      # both kinds occur


def test_evaluate_ei_far_below_the_incumbent():
    c = make_case(128, 3, 37, M52, 0.05, seed=78, kparam=1.0)
    sp = spec("ei", f_best=6.0, var_add=0.05)
    a, _, mean, var = check_eval(c, sp, c["X0"])
    Z = (mean.reshape(-1) - 6.0 - 0.01) / var.sqrt()
    assert float(mean.max()) < 3.0 and float(Z.max()) < -4.0 and float(Z.min()) < -8.0, (mean.max(), Z.max(), Z.min())
    assert float(a.max()) < 1e-5      # Phi is tiny everywhere


# ---- trajectories ------------------------------------------------------------------------------------------------------------------
#        n    D   Q    kernel  acquisition            noise  lr    seed
TRAJ = [(40, 2, 37, SE, spec("ucb"), 0.05, 0.1, 1),
        (128, 3, 50, M52, spec("ei", f_best=0.3), 0.05, 0.1, 2),
        (129, 5, 33, SE, spec("ucb"), 0.02, 0.05, 3),
        (256, 16, 70, M52, spec("ucb"), 0.05, 0.1, 4),
        (17, 1, 16, SE, spec("ei", f_best=0.3), 0.05, 0.1, 5),
        (200, 4, 500, SE, spec("ucb"), 0.05, 0.1, 6)]
STEPS = 30


@functools.lru_cache(maxsize=None)
def traj(i):
    """case i once: the CPU loop, its twin, loop B, the fused call -- shared by the tests below and left unchanged"""
    n, D, Q, kfun, sp, noise, lr, seed = TRAJ[i]
    c = make_case(n, D, Q, kfun, noise, seed)
    A = loop_a(c, c["X0"], sp, STEPS, lr)
    twin = loop_a(c, c["X0"] * (1.0 + 2e-16), sp, STEPS, lr)
    post = gpu_posterior(c)
    B = loop_b(post, c["X0"], sp, STEPS, lr)
    X0d = c["X0"].to(DEV)
    keep = X0d.clone()
    Fz = post.optimize_acquisition(X0d, steps=STEPS, lr=lr, acq=sp["acq"], kappa=sp["kappa"], xi=sp["xi"], f_best=sp["f_best"],
                                   var_add_all=sp["var_add"], var_floor=sp["var_floor"])
    assert torch.equal(X0d, keep)      # X0 is left untouched
    return c, post, A, twin, B, Fz


@pytest.mark.parametrize("i", range(len(TRAJ)))
def test_trajectory_follows_both_references(i):
    c, post, A, twin, B, Fz = traj(i)
    dt_x, dt_t = rel(twin[2], A[2]), rel(twin[1], A[1])
    assert dt_x <= 1e-11 and dt_t <= 1e-11, (dt_x, dt_t)      # conditioning of the case, before anything is compared
    d0 = distance(B, A)
    assert d0 <= 1e-10, "ill-conditioned case: d0 = %.2e" % d0
    bound = max(10.0 * d0, 1e-12)
    dA, dB = distance(Fz, A), distance(Fz, B)
    print("case %d: twin %.2e / %.2e, d0 %.2e, bound %.2e, fused vs A %.2e, vs B %.2e" % (i, dt_x, dt_t, d0, bound, dA, dB))
    assert Fz[3]["fused"] is True and Fz[3]["step"] == STEPS
    assert Fz[1].shape == (STEPS, TRAJ[i][2]) and Fz[2].shape == (STEPS + 1, TRAJ[i][2], TRAJ[i][1])
    assert torch.equal(Fz[0], Fz[2][-1]) and torch.equal(Fz[2][0].cpu(), c["X0"])
    assert dA <= bound, (dA, bound)
    assert dB <= bound, (dB, bound)


def _fused(post, X0, sp, steps, lr, state=None):
    return post.optimize_acquisition(X0, steps=steps, lr=lr, acq=sp["acq"], kappa=sp["kappa"], xi=sp["xi"], f_best=sp["f_best"],
                                     var_add_all=sp["var_add"], var_floor=sp["var_floor"], state=state)


@pytest.mark.parametrize("i", [1, 5])
def test_state_continues_the_optimiser_bit_for_bit(i):
    c, post, _, _, _, Fz = traj(i)
    sp, lr = TRAJ[i][4], TRAJ[i][6]
    X1, t1, h1, st = _fused(post, c["X0"].to(DEV), sp, 12, lr)
    assert st["fused"] is True and st["step"] == 12
    X2, t2, h2, st2 = _fused(post, X1, sp, 18, lr, state=st)
    assert st2["step"] == 30
    assert torch.equal(X2, Fz[0])
    assert torch.equal(torch.cat([t1, t2]), Fz[1])
    assert torch.equal(torch.cat([h1[:-1], h2]), Fz[2])
    assert torch.equal(st2["exp_avg"], Fz[3]["exp_avg"]) and torch.equal(st2["exp_avg_sq"], Fz[3]["exp_avg_sq"])


def test_a_point_does_not_depend_on_its_tile_or_neighbours():
    c, post, _, _, _, Fz = traj(5)
    sp, lr = TRAJ[5][4], TRAJ[5][6]
    X0 = c["X0"].to(DEV)
    lo = _fused(post, X0[:250].contiguous(), sp, STEPS, lr)
    hi = _fused(post, X0[250:].contiguous(), sp, STEPS, lr)
    assert torch.equal(torch.cat([lo[0], hi[0]]), Fz[0])
    assert torch.equal(torch.cat([lo[1], hi[1]], 1), Fz[1])
    assert torch.equal(torch.cat([lo[2], hi[2]], 1), Fz[2])


# ---- optimize_acqf -------------------------------------------------------------------------------------------------------------------
def frozen_model(kernel_module, n=60, D=2, seed=11):
    from fidelityfusion_amd.cigp_v10 import cigp
    g = torch.Generator().manual_seed(seed)
    X = 2.0 * torch.rand(n, D, generator=g)
    y = (torch.sin(2.0 * X.sum(1)) + 0.1 * torch.randn(n, generator=g)).reshape(n, 1)
    m = cigp(kernel_module, log_beta=3.0).double().to(DEV)
    m.requires_grad_(False)
    return m, X.to(DEV), y.to(DEV), 2.0 * torch.rand(23, D, generator=g)


def ard_kernel(D, seed=5):
    from fidelityfusion_amd import kernel
    k = kernel.ARDKernel(D)
    with torch.no_grad():
        k.length_scales.copy_(0.7 + torch.rand(D, generator=torch.Generator().manual_seed(seed)))
        k.signal_variance.fill_(1.3)
    return k


@pytest.mark.parametrize("acq_name", ["ucb", "ei"])
def test_optimize_acqf_selects_as_the_reference_does(acq_name):
    from fidelityfusion_amd import acq
    m, x, y, X0 = frozen_model(ard_kernel(2))
    X0d = X0.to(DEV)
    keep = X0d.clone()
    noise = float(m.log_beta.exp().pow(-1))
    sp = spec(acq_name, f_best=0.3, var_add=noise)
    post = m._cached_posterior(x, y)[0]
    XB, tB, hB = loop_b(post, X0d, sp, STEPS, 0.1)
    kB, bestB = select(X0d, tB, hB)
    best = acq.optimize_acqf(m, x, y, X0d, steps=STEPS, lr=0.1, acq=acq_name, f_best=0.3)
    assert torch.equal(X0d, keep)
    Xf, tf, hf, st = post.optimize_acquisition(X0d, steps=STEPS, lr=0.1, acq=acq_name, f_best=0.3, var_add_all=noise)
    assert st["fused"] is True
    kF, _ = select(X0d, tf, hf)
    # the yardstick of the trajectory tests, on THIS model: the CPU loop on the posterior's own effective parameters, its twin, d0
    c = {"X": x.cpu(), "Y": y.cpu(), "w": post.w.cpu(), "amp": float(post.amp), "kfun": int(post.kfun[0]), "kparam": float(post.kfun[1]),
         "clamp": float(post.clamp), "dadd": float(post.dadd), "X0": X0}
    A = loop_a(c, X0, sp, STEPS, 0.1)
    twin = loop_a(c, X0 * (1.0 + 2e-16), sp, STEPS, 0.1)
    assert rel(twin[2], A[2]) <= 1e-11 and rel(twin[1], A[1]) <= 1e-11
    d0 = distance((XB, tB, hB), A)
    assert d0 <= 1e-10, "ill-conditioned case: d0 = %.2e" % d0
    bound = max(10.0 * d0, 1e-12)
    scale = float(hB.abs().max())      # the normaliser of `distance` on the history, of which best_x and the final X are entries
    e_best, e_final = float((best - bestB).abs().max()) / scale, float((Xf - XB).abs().max()) / scale
    print("%s: selected step %d (loop B: %d), d0 %.2e, bound %.2e, best_x %.2e, final X %.2e, fused vs B %.2e"
          % (acq_name, kF, kB, d0, bound, e_best, e_final, distance((Xf, tf, hf), (XB, tB, hB))))
    assert kF == kB and kB >= 0
    assert torch.equal(best, hf[kF + 1])      # the fused call is deterministic: optimize_acqf returned exactly that history entry
    assert e_best <= bound, (e_best, bound)
    final = acq.optimize_acqf(m, x, y, X0d, steps=STEPS, lr=0.1, acq=acq_name, f_best=0.3, return_best_only=False)
    assert torch.equal(final, Xf) and e_final <= bound, (e_final, bound)


@pytest.mark.parametrize("steps,lr", [(1, 0.1), (5, 0.0)])
def test_optimize_acqf_returns_x0_when_no_step_improves(steps, lr):
    """the first step's loss IS the loss at X0, so one step can never be selected; with lr = 0 nothing ever moves"""
    from fidelityfusion_amd import acq
    m, x, y, X0 = frozen_model(ard_kernel(2))
    X0d = X0.to(DEV)
    post = m._cached_posterior(x, y)[0]
    sp = spec("ucb", var_add=float(m.log_beta.exp().pow(-1)))
    _, tB, hB = loop_b(post, X0d, sp, steps, lr)
    assert select(X0d, tB, hB)[0] == -1
    best = acq.optimize_acqf(m, x, y, X0d, steps=steps, lr=lr)
    assert torch.equal(best, X0d) and best.data_ptr() != X0d.data_ptr()


# ---- fall-backs stay fall-backs -------------------------------------------------------------------------------------------------------
def _fallback_equals_loop_b(post, X0, sp, steps=6):
    keep = X0.clone()
    r = _fused(post, X0, sp, steps, 0.1)
    assert r[3]["fused"] is False
    assert torch.equal(X0, keep)
    B = loop_b(post, X0, sp, steps, 0.1)
    for got, want in zip(r[:3], B):
        assert got.device == X0.device
        assert rel(got, want) <= 1e-12
    return r


def _accepted(post, X0, sp, steps=6):
    assert _fused(post, X0, sp, steps, 0.1)[3]["fused"] is True


def test_fallback_composed_kernels():
    from fidelityfusion_amd import kernel
    D = 2
    for comp in (kernel.SumKernel(ard_kernel(D), kernel.MaternKernel(D)), kernel.SumKernel(kernel.LinearKernel(D), kernel.MaternKernel(D))):
        m, x, y, X0 = frozen_model(comp.double())
        post = m._cached_posterior(x, y)[0]
        assert post.tree is not None
        _fallback_equals_loop_b(post, X0.to(DEV), spec("ucb", var_add=0.05))
    m, x, y, X0 = frozen_model(ard_kernel(D))
    _accepted(m._cached_posterior(x, y)[0], X0.to(DEV), spec("ucb", var_add=0.05))


def test_fallback_linear_profile_is_never_routed_to_the_fused_call():
    c = make_case(30, 2, 9, SE, 0.05, seed=21)
    post = gpu_posterior(c)
    X0 = c["X0"].to(DEV)
    assert post.acq_fusable(X0)
    post.kfun = (LINEAR, 1.0)
    assert not post.acq_fusable(X0)


@pytest.mark.parametrize("what", ["n", "D", "d", "cpu"])
def test_fallback_outside_the_limits(what):
    from fidelityfusion_amd import _lib
    assert (_lib.FFGP_ACQ_MAX_N, _lib.FFGP_ACQ_MAX_D) == (256, 16)
    sp = spec("ucb", var_add=0.05)
    n, D, d = {"n": (257, 2, 1), "D": (40, 17, 1), "d": (40, 2, 2), "cpu": (40, 2, 1)}[what]
    c = make_case(n, D, 19, SE, 0.05, seed=31, d=d)
    X0 = c["X0"] if what == "cpu" else c["X0"].to(DEV)
    _fallback_equals_loop_b(gpu_posterior(c), X0, sp)
    n2, D2, d2 = {"n": (256, 2, 1), "D": (40, 16, 1), "d": (40, 2, 1), "cpu": (40, 2, 1)}[what]
    c2 = make_case(n2, D2, 19, SE, 0.05, seed=31, d=d2)
    _accepted(gpu_posterior(c2), c2["X0"].to(DEV), sp)


# ---- after Posterior.append ------------------------------------------------------------------------------------------------------------
def test_fused_call_uses_the_grown_factor_after_append():
    c = make_case(129, 3, 37, SE, 0.05, seed=41)
    sp, lr = spec("ucb", var_add=0.05), 0.1
    post = gpu_posterior(c, n=120)
    X0 = c["X0"].to(DEV)
    before = _fused(post, X0, sp, STEPS, lr)      # (keys the handle's cached inverses on the 120-point factor)
    post.append(c["X"][120:].to(DEV), c["Y"][120:].to(DEV))
    assert post.n == 129
    A = loop_a(c, c["X0"], sp, STEPS, lr)         # the CPU loop on all 129 points
    B = loop_b(post, X0, sp, STEPS, lr)
    Fz = _fused(post, X0, sp, STEPS, lr)
    d0 = distance(B, A)
    assert d0 <= 1e-10, d0
    bound = max(10.0 * d0, 1e-12)
    print("append: d0 %.2e, fused vs A %.2e, vs B %.2e, vs the 120-point run %.2e" % (d0, distance(Fz, A), distance(Fz, B), distance(Fz, before)))
    assert Fz[3]["fused"] is True
    assert distance(Fz, A) <= bound and distance(Fz, B) <= bound
    assert distance(Fz, before) > 1e-6      # the nine new points do change the answer


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
REFUSALS = [dict(null=("h",)), dict(null=("p",)), dict(null=("X",)), dict(null=("trace",)), dict(null=("opt",)), dict(null=("state",)),
            dict(X_dev=None), dict(L_dev=None), dict(alpha_dev=None), dict(w_dev=None), dict(amp_dev=None),
            dict(n=0), dict(n=257), dict(D=0), dict(D=17), dict(steps=-1), dict(steps=4097), dict(d=2), dict(kfun=LINEAR), dict(kfun=6),
            dict(kfun=-1), dict(acq=2), dict(acq=-1), dict(Q=0), dict(Q=-3), dict(step0=-1)]


@pytest.fixture(scope="module")
def abi_post():
    c = make_case(40, 2, 21, SE, 0.05, seed=51)
    return c, gpu_posterior(c)


@pytest.mark.parametrize("bad", REFUSALS, ids=lambda b: ",".join("%s=%s" % kv for kv in b.items()))
def test_c_abi_refuses_before_anything_is_enqueued(abi_post, bad):
    from fidelityfusion_amd import _lib
    c, post = abi_post
    bad = dict(bad)
    kw = {k: bad.pop(k) for k in ("null", "steps", "Q", "step0") if k in bad}
    kw.setdefault("steps", 4)
    rc, X, state, trace, hist, grad = raw_call(post, c["X0"], spec("ucb"), **kw, **bad)
    assert rc == _lib.FFGP_ERR_ARG
    assert torch.equal(X.cpu(), c["X0"]) and not bool(state.any()) and bool((trace == -7.0).all())
    assert bool((hist == -7.0).all()) and bool((grad == -7.0).all())


def test_c_abi_accepted_call_runs(abi_post):
    c, post = abi_post
    sp = spec("ucb")
    rc, X, state, trace, hist, grad = raw_call(post, c["X0"], sp, steps=4)
    assert rc == 0
    A = loop_a(c, c["X0"], sp, 4, 0.1)
    assert rel(trace, A[1]) <= 1e-10 and rel(hist, A[2]) <= 1e-10 and torch.equal(X, hist[-1])
    assert bool(state[1].gt(0).any())
    # the gradient output is that of the LAST evaluation: the points before the fourth step
    _, g, _, _ = cpu_eval(c, A[2][3], sp)
    assert rel(grad, g) <= 1e-8
