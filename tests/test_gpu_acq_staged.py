"""The acquisition optimiser past 256 training points: the launch-per-stage loop inside one library call
(ffgp_acq_optimize_stack_staged, csrc/acq_staged.hip; `staged=True` on Posterior / PosteriorStack.optimize_acquisition and
acq.optimize_acqf / optimize_acqf_mf) against the references test_gpu_acq.py and test_gpu_acq_stack.py are written against -- plain
fp64 torch on the CPU, the per-step loop on the GPU, the one-launch kernels where they still serve, and a fixture of the reference's own
loop at its demo's sizes (tests/golden/mf_acq_ar_n300.npz, written by tests/golden/gen_acq_staged_goldens.py).

Helpers, recipes and bars are those two files', imported and unchanged.  Evaluate mode (steps = 0): values rel. 1e-10, gradients rel.
1e-8.  Trajectories: (A) the CPU loop and (B) the per-step GPU loop differ by rounding only; d0 = their distance is the yardstick,
max(10 d0, 1e-12) the bound, a case with d0 > 1e-10 fails as ill-conditioned, and a CPU twin started one ulp away must stay within 1e-11
before anything is compared.  State: 12 + 18 steps equal 30 bit for bit.  Cutting Q into two calls can change the tile shape the fp64
GEMM picks for V = L^-1 K_s and B = L^-T V -- a column's accumulation order within one shape is fixed, across shapes it is not -- so
that comparison is held to a relative distance of 1e-13, not to equality.  Every case runs a handful of steps on shapes just past the
one-launch limit (257), at the demo's 300, and at 513 = 4 chunks of 128 rows + 1 with D = 16."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_acq as A1            # noqa: E402
import test_gpu_acq_stack as S       # noqa: E402
from test_gpu_acq_stack import ACQ_CODE, DEV, LINEAR, M12, M32, M52, NEG_INF, RQ, SE, distance, rel      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 8


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(torch.float32)


# ---- the GPU side --------------------------------------------------------------------------------------------------------------------
def raw_staged(gst, Xq, level, sp, steps=0, lr=0.1, step0=0, Q=None, null=(), F=None, accumulate=0, acq=None, member=0, **over):
    """ffgp_acq_optimize_stack_staged through ctypes: test_gpu_acq_stack.raw_call with the staged entry.  `over` overrides fields of
    member `member`, `null` names pointers to pass as NULL.  Returns (status, X, state, trace, hist, grad), every buffer pre-filled."""
    from fidelityfusion_amd import _lib
    keep = []
    tab = gst._member_table(gst.test_var_adds, keep)
    for k, v in over.items():
        setattr(tab[member], k, v)
    Qn, D = Xq.shape
    X = Xq.to(DEV).clone().contiguous()
    state = torch.zeros((3, Qn, D), device=DEV)
    trace = torch.full((max(steps, 1), Qn), -7.0, device=DEV)
    hist = torch.full((max(steps, 0) + 1, Qn, D), -7.0, device=DEV)
    grad = torch.full((Qn, D), -7.0, device=DEV)
    lv = None if level is None else level.to(device=DEV, dtype=torch.int32).contiguous()
    s = _lib.AcqStack(F=gst.F if F is None else F, members=None if "members" in null else tab, level_dev=None if lv is None else lv.data_ptr(),
                      var_floor=sp["var_floor"], acq=ACQ_CODE[sp["acq"]] if acq is None else acq, kappa=sp["kappa"], xi=sp["xi"],
                      f_best=sp["f_best"], accumulate_grad=accumulate)
    opt = _lib.Adam(lr, 0.9, 0.999, 1e-8)
    ptr = lambda name, t: None if name in null else C.c_void_p(t.data_ptr())
    rc = _lib.lib.ffgp_acq_optimize_stack_staged(None if "h" in null else gst.members[0]._h(), None if "s" in null else C.byref(s), ptr("X", X),
                                                 Qn if Q is None else Q, steps, None if "opt" in null else C.byref(opt), ptr("state", state),
                                                 step0, ptr("trace", trace), ptr("hist", hist), ptr("grad", grad))
    torch.cuda.synchronize()
    return rc, X, state, trace, hist, grad


def one_stack(post, var_add):
    """a single posterior as the staged entry takes it: the stack of one member with both coefficients 1"""
    from fidelityfusion_amd import functional as F
    gst = F.PosteriorStack([post], [1.0])
    gst.test_var_adds = [var_add]
    return gst


def single(post, X0, sp, steps, lr, state=None, **kw):
    return post.optimize_acquisition(X0, steps=steps, lr=lr, acq=sp["acq"], kappa=sp["kappa"], xi=sp["xi"], f_best=sp["f_best"],
                                     var_add_all=sp["var_add"], var_floor=sp["var_floor"], state=state, **kw)


def stacked(gst, X0, level, sp, steps, lr, accumulate=False, state=None, **kw):
    return gst.optimize_acquisition(X0, steps=steps, lr=lr, acq=sp["acq"], kappa=sp["kappa"], xi=sp["xi"], f_best=sp["f_best"],
                                    var_floor=sp["var_floor"], level=None if level is None else level.to(DEV), var_adds=gst.test_var_adds,
                                    accumulate_grad=accumulate, state=state, **kw)


def is_staged(st):
    return st["fused"] is False and st.get("staged") is True


def single_case(n, D, Q, kfun, seed):
    return A1.make_case(n, D, Q, kfun, 0.05, seed=seed, kparam=A1.KF[kfun], clamp=1e-30 if kfun in (M12, M32, M52) else NEG_INF)


# ---- 1. values and gradients (steps = 0) against CPU autograd --------------------------------------------------------------------------
#        n    D   Q   profile      every radial profile the one-launch call accepts, at one of the issue's three shapes
EVAL = [(257, 2, 37, SE), (257, 2, 37, M12), (300, 1, 16, M32), (300, 1, 16, RQ), (513, 16, 21, M52)]


@functools.lru_cache(maxsize=None)
def eval_case(i):
    n, D, Q, kfun = EVAL[i]
    c = single_case(n, D, Q, kfun, 2000 + i)
    return c, one_stack(A1.gpu_posterior(c), 0.05)


@pytest.mark.parametrize("acq", ["ucb", "ei"])
@pytest.mark.parametrize("i", range(len(EVAL)))
def test_evaluate_matches_cpu_autograd(i, acq):
    c, gst = eval_case(i)
    sp = A1.spec(acq, f_best=0.3, var_add=0.05)
    rc, X, _, trace, _, grad = raw_staged(gst, c["X0"], None, sp)
    assert rc == 0
    assert torch.equal(X.cpu(), c["X0"])      # evaluate mode: nothing moves
    a, g, _, _ = A1.cpu_eval(c, c["X0"], sp)
    ev, eg = rel(trace[0], a), rel(grad, g)
    print("staged n=%d D=%d Q=%d kfun=%d %s: value rel %.2e, gradient rel %.2e" % (EVAL[i] + (acq, ev, eg)))
    assert ev <= 1e-10, ev
    assert eg <= 1e-8, eg


# ---- 2. trajectories against the per-step GPU loop and the CPU loop -------------------------------------------------------------------
#        n    D   Q   kernel  acquisition                     seed
TRAJ = [(257, 2, 37, SE, A1.spec("ucb", var_add=0.05), 11),
        (300, 1, 16, SE, A1.spec("ei", f_best=0.3, var_add=0.05), 12)]
LR = 0.1


@functools.lru_cache(maxsize=None)
def traj(i, steps=STEPS):
    """case i once: the CPU loop, its twin, loop B, the staged call -- shared by the tests below and left unchanged"""
    n, D, Q, kfun, sp, seed = TRAJ[i]
    c = single_case(n, D, Q, kfun, seed)
    A = A1.loop_a(c, c["X0"], sp, steps, LR)
    twin = A1.loop_a(c, c["X0"] * (1.0 + 2e-16), sp, steps, LR)
    post = A1.gpu_posterior(c)
    B = A1.loop_b(post, c["X0"], sp, steps, LR)
    X0d = c["X0"].to(DEV)
    keep = X0d.clone()
    Z = single(post, X0d, sp, steps, LR, staged=True)
    assert torch.equal(X0d, keep)      # X0 is left untouched
    return c, post, A, twin, B, Z


def yardstick(A, twin, B):
    """the existing rule: the twin within 1e-11, d0 = |B - A| <= 1e-10, the bound max(10 d0, 1e-12)"""
    dt_x, dt_t = rel(twin[2], A[2]), rel(twin[1], A[1])
    assert dt_x <= 1e-11 and dt_t <= 1e-11, (dt_x, dt_t)
    d0 = distance(B, A)
    assert d0 <= 1e-10, "ill-conditioned case: d0 = %.2e" % d0
    return d0, max(10.0 * d0, 1e-12)


@pytest.mark.parametrize("i", range(len(TRAJ)))
def test_trajectory_follows_both_references(i):
    c, post, A, twin, B, Z = traj(i)
    d0, bound = yardstick(A, twin, B)
    dA, dB = distance(Z, A), distance(Z, B)
    print("staged case %d: d0 %.2e, bound %.2e, staged vs A %.2e, vs B %.2e" % (i, d0, bound, dA, dB))
    n, D, Q = TRAJ[i][:3]
    assert is_staged(Z[3]) and Z[3]["step"] == STEPS
    assert Z[1].shape == (STEPS, Q) and Z[2].shape == (STEPS + 1, Q, D)
    assert torch.equal(Z[0], Z[2][-1]) and torch.equal(Z[2][0].cpu(), c["X0"])
    assert dA <= bound, (dA, bound)
    assert dB <= bound, (dB, bound)


# ---- 3. the forced staged call against the one-launch call -----------------------------------------------------------------------------
#          n    D   Q   kernel  acquisition                seed  steps
FORCED = [(40, 2, 37, SE, A1.spec("ucb", var_add=0.05), 21, 30),
          (256, 16, 20, M52, A1.spec("ucb", var_add=0.05), 22, STEPS)]


@functools.lru_cache(maxsize=None)
def forced(i):
    n, D, Q, kfun, sp, seed, steps = FORCED[i]
    c = single_case(n, D, Q, kfun, seed)
    A = A1.loop_a(c, c["X0"], sp, steps, LR)
    twin = A1.loop_a(c, c["X0"] * (1.0 + 2e-16), sp, steps, LR)
    post = A1.gpu_posterior(c)
    B = A1.loop_b(post, c["X0"], sp, steps, LR)
    one = single(post, c["X0"].to(DEV), sp, steps, LR)
    return c, post, A, twin, B, one


@pytest.mark.parametrize("i", range(len(FORCED)))
def test_forced_staged_call_follows_the_one_launch_call(i):
    c, post, A, twin, B, one = forced(i)
    sp, steps = FORCED[i][4], FORCED[i][6]
    d0, bound = yardstick(A, twin, B)
    Z = single(post, c["X0"].to(DEV), sp, steps, LR, staged="force")
    assert one[3]["fused"] is True and not one[3].get("staged") and is_staged(Z[3])
    dO, dA = distance(Z, one), distance(Z, A)
    print("forced n=%d: d0 %.2e, bound %.2e, staged vs one-launch %.2e, vs A %.2e" % (FORCED[i][0], d0, bound, dO, dA))
    assert dO <= bound and dA <= bound, (dO, dA, bound)


def test_one_launch_state_is_continued_by_the_staged_call():
    c, post, A, twin, B, one = forced(0)      # 30 one-launch steps
    sp = FORCED[0][4]
    _, bound = yardstick(A, twin, B)
    X1, t1, h1, s1 = single(post, c["X0"].to(DEV), sp, 12, LR)
    assert s1["fused"] is True
    X2, t2, h2, s2 = single(post, X1, sp, 18, LR, state=s1, staged="force")
    assert is_staged(s2) and s2["step"] == 30
    got = (X2, torch.cat([t1, t2]), torch.cat([h1[:-1], h2]))
    d = distance(got, one)
    print("12 one-launch + 18 staged steps vs 30 one-launch steps: %.2e (bound %.2e)" % (d, bound))
    assert d <= bound and rel(X2, one[0]) <= bound


# ---- 4. the stack at the demo's sizes --------------------------------------------------------------------------------------------------
NS, SD, SQ, COEFS = (300, 300, 250), 2, 19, (1.0, 0.8, -1.3)
STACK_ACQ = {"ucb": S.spec("ucb"), "ei": S.spec("ei", f_best=0.3), "ucb_var": S.spec("ucb_var", kappa=0.4)}


@functools.lru_cache(maxsize=None)
def big_stack():
    st = S.make_stack(NS, SD, COEFS, SQ, seed=800)      # rho != 1, one of them negative; var_adds 0.05; levels mixed: (7 q + 2) % 3
    return st, S.gpu_stack(st)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("acq", ["ucb", "ei", "ucb_var"])
def test_stack_follows_both_references(acq, accumulate):
    st, gst = big_stack()
    sp, lr = STACK_ACQ[acq], 0.01 if accumulate else 0.1
    A = S.loop_a(st, st["X0"], st["level"], sp, STEPS, lr, accumulate)
    twin = S.loop_a(st, st["X0"] * (1.0 + 2e-16), st["level"], sp, STEPS, lr, accumulate)
    B = S.loop_b(gst, st["X0"], st["level"], sp, STEPS, lr, accumulate)
    d0, bound = yardstick(A, twin, B)
    Z = stacked(gst, st["X0"].to(DEV), st["level"], sp, STEPS, lr, accumulate, staged=True)
    dA, dB = distance(Z, A), distance(Z, B)
    print("staged stack %s accumulate=%s: d0 %.2e, bound %.2e, staged vs A %.2e, vs B %.2e" % (acq, accumulate, d0, bound, dA, dB))
    assert is_staged(Z[3]) and Z[3]["step"] == STEPS and ("grad_sum" in Z[3]) == accumulate
    assert torch.equal(Z[0], Z[2][-1]) and torch.equal(Z[2][0].cpu(), st["X0"])
    assert dA <= bound, (dA, bound)
    assert dB <= bound, (dB, bound)


@pytest.mark.parametrize("accumulate", [0, 1])
def test_stack_with_a_negative_level_switches_every_member_off_for_that_point(accumulate):
    """the C entry reads a negative level as "no member": mean = var = 0, a zero gradient, the point stays where it is"""
    st, gst = big_stack()
    sp, lr = STACK_ACQ["ucb"], 0.01 if accumulate else 0.1
    level = st["level"].clone()
    level[3] = -1
    level[17] = -2
    A = S.loop_a(st, st["X0"], level, sp, STEPS, lr, bool(accumulate))
    twin = S.loop_a(st, st["X0"] * (1.0 + 2e-16), level, sp, STEPS, lr, bool(accumulate))
    B = S.loop_b(gst, st["X0"], level, sp, STEPS, lr, bool(accumulate))
    _, bound = yardstick(A, twin, B)
    rc, X, state, trace, hist, _ = raw_staged(gst, st["X0"], level, sp, steps=STEPS, lr=lr, accumulate=accumulate)
    assert rc == 0
    got = (X, trace, hist)
    assert distance(got, B) <= bound and distance(got, A) <= bound
    assert torch.equal(hist[:, 3].cpu(), st["X0"][3].expand(STEPS + 1, SD)) and torch.equal(hist[:, 17].cpu(), st["X0"][17].expand(STEPS + 1, SD))
    assert bool(state[2].ne(0).any()) == bool(accumulate)


# ---- 5. the fixture of the reference's loop at (300, 300, 250) ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "mf_acq_ar_n300.npz"))
    t = lambda k: torch.tensor(z[k])
    members = []
    for f in range(3):
        noise = math.exp(-float(z["log_beta"][f]))
        members.append({"X": t("x_%d" % f), "Y": t("y_%d" % f), "w": torch.full((2,), math.exp(-float(z["log_length_scale"][f]))),
                        "amp": math.exp(float(z["log_signal_variance"][f])) ** 2, "kfun": SE, "kparam": 1.0, "clamp": NEG_INF,
                        "dadd": noise + 1e-6, "var_add": noise})
    coefs = [1.0] + [float(r) for r in z["rho"]]
    st = {"members": members, "coefs": coefs, "var_coefs": [c * c for c in coefs], "F": 3, "D": 2}
    return z, st, S.gpu_stack(st)


@pytest.mark.parametrize("tag", ["zg", "acc"])
def test_staged_call_reproduces_the_reference_fixture_at_every_level(tag):
    """the bars of test_gpu_acq_stack.py's fixture test, on the fixture of the demo's sizes: both gradient modes, all three levels in one call"""
    z, st, gst = fixture()
    assert [m["X"].shape[0] for m in st["members"]] == [300, 300, 250]
    assert float(z["twin_distance"]) <= 1e-11
    steps, lr, acc = int(z["steps"]), float(z["lr"]), tag == "acc"
    sp = S.spec("ucb_var", kappa=float(z["kappa"]))
    X0 = torch.tensor(z["X0"])                           # [3, 6, 2]: six starts per level
    level = torch.arange(3).repeat_interleave(6)
    Z = stacked(gst, X0.reshape(18, 2).to(DEV), level, sp, steps, lr, acc, staged=True)      # every level from one call
    assert is_staged(Z[3])
    for s in range(3):
        ref = (None, torch.tensor(z["trace_" + tag][s]), torch.tensor(z["hist_" + tag][s]))
        B = S.loop_b(gst, X0[s], torch.full((6,), s), sp, steps, lr, acc)
        d0 = distance(B, ref)
        assert d0 <= 1e-10, "ill-conditioned case: d0 = %.2e" % d0
        bound = max(10.0 * d0, 1e-12)
        got = (None, Z[1][:, 6 * s:6 * s + 6], Z[2][:, 6 * s:6 * s + 6])
        print("fixture n300 %s level %d: d0 %.2e, bound %.2e, staged vs fixture %.2e, vs B %.2e" % (tag, s, d0, bound, distance(got, ref), distance(got, B)))
        assert distance(got, ref) <= bound and distance(got, B) <= bound
        assert rel(Z[0][6 * s:6 * s + 6], ref[2][-1]) <= bound      # the final points


# ---- 6. state and splitting ------------------------------------------------------------------------------------------------------------
def test_state_continues_the_optimiser_bit_for_bit():
    c, post, _, _, _, _ = traj(0)
    sp, X0 = TRAJ[0][4], c["X0"].to(DEV)
    full = single(post, X0, sp, 30, LR, staged=True)
    X1, t1, h1, s1 = single(post, X0, sp, 12, LR, staged=True)
    assert is_staged(s1) and s1["step"] == 12
    X2, t2, h2, s2 = single(post, X1, sp, 18, LR, state=s1, staged=True)
    assert is_staged(s2) and s2["step"] == 30
    assert torch.equal(X2, full[0])
    assert torch.equal(torch.cat([t1, t2]), full[1])
    assert torch.equal(torch.cat([h1[:-1], h2]), full[2])
    assert torch.equal(s2["exp_avg"], full[3]["exp_avg"]) and torch.equal(s2["exp_avg_sq"], full[3]["exp_avg_sq"])


def test_state_continues_the_stack_with_accumulation_bit_for_bit():
    st, gst = big_stack()
    sp, X0, lv = STACK_ACQ["ucb_var"], st["X0"].to(DEV), st["level"]
    full = stacked(gst, X0, lv, sp, 30, 0.01, True, staged=True)
    X1, t1, h1, s1 = stacked(gst, X0, lv, sp, 12, 0.01, True, staged=True)
    X2, t2, h2, s2 = stacked(gst, X1, lv, sp, 18, 0.01, True, state=s1, staged=True)
    assert torch.equal(X2, full[0]) and torch.equal(torch.cat([t1, t2]), full[1]) and torch.equal(torch.cat([h1[:-1], h2]), full[2])
    assert torch.equal(s2["grad_sum"], full[3]["grad_sum"]) and bool(s2["grad_sum"].ne(0).any())


def test_cutting_the_points_into_two_calls_changes_rounding_at_most():
    """Q = 37 in one call against 16 + 21: the GEMM may pick another tile shape for 16 or 21 columns than for 37, so this is a
    tolerance (1e-13, relative), not equality -- see the module's docstring"""
    c, post, _, _, _, Z = traj(0)
    sp, X0 = TRAJ[0][4], c["X0"].to(DEV)
    lo = single(post, X0[:16].contiguous(), sp, STEPS, LR, staged=True)
    hi = single(post, X0[16:].contiguous(), sp, STEPS, LR, staged=True)
    got = (torch.cat([lo[0], hi[0]]), torch.cat([lo[1], hi[1]], 1), torch.cat([lo[2], hi[2]], 1))
    d = max(distance(got, Z), rel(got[0], Z[0]))
    print("Q = 37 against 16 + 21: %.2e" % d)
    assert d <= 1e-13, d


# ---- 7. only L's lower triangle within n columns is read ---------------------------------------------------------------------------------
def test_padding_and_the_upper_triangle_of_the_factor_are_never_read():
    c, post, _, _, _, _ = traj(0)
    sp, n = TRAJ[0][4], post.n
    gst = one_stack(post, 0.05)
    ldl = (n + 9) // 2 * 2      # > n, even like the library's own leading dimensions
    clean = torch.zeros((n, ldl), device=DEV)
    clean[:, :n] = torch.tril(post.W[:n, :n])
    dirty = clean.clone()
    dirty[:, :n] += torch.triu(torch.full((n, n), float("nan"), device=DEV), diagonal=1)
    dirty[:, n:] = float("nan")
    assert bool(torch.isnan(dirty).any()) and torch.equal(torch.tril(dirty[:, :n]), clean[:, :n])
    ra = raw_staged(gst, c["X0"], None, sp, steps=STEPS, L_dev=clean.data_ptr(), ldl=ldl)
    rb = raw_staged(gst, c["X0"], None, sp, steps=STEPS, L_dev=dirty.data_ptr(), ldl=ldl)
    assert ra[0] == 0 and rb[0] == 0
    assert bool(torch.isfinite(ra[3]).all()) and bool(ra[1].ne(c["X0"].to(DEV)).any())
    for x, y in zip(ra[1:], rb[1:]):
        assert torch.equal(x, y)


# ---- 8. the C ABI ---------------------------------------------------------------------------------------------------------------------
REFUSALS = [dict(null=("h",)), dict(null=("s",)), dict(null=("X",)), dict(null=("trace",)), dict(null=("opt",)), dict(null=("state",)),
            dict(null=("members",)), dict(F=0), dict(F=9),
            dict(X_dev=None), dict(L_dev=None), dict(alpha_dev=None), dict(w_dev=None), dict(amp_dev=None), dict(member=2, X_dev=None),
            dict(n=0), dict(n=2049), dict(member=1, n=2049), dict(D=0), dict(D=17), dict(member=1, D=3), dict(d=2), dict(member=2, d=2),
            dict(ldl=39), dict(kfun=LINEAR), dict(kfun=6), dict(member=2, kfun=-1),
            dict(acq=3), dict(acq=-1), dict(steps=-1), dict(steps=4097), dict(Q=0), dict(Q=-3), dict(step0=-1)]


@pytest.fixture(scope="module")
def abi_stack():
    st = S.make_stack((40, 24, 17), 2, (1.0, 0.8, -1.3), 21, seed=701)
    return st, S.gpu_stack(st)


@pytest.mark.parametrize("bad", REFUSALS, ids=lambda b: ",".join("%s=%s" % kv for kv in b.items()))
def test_c_abi_refuses_before_anything_is_enqueued(abi_stack, bad):
    from fidelityfusion_amd import _lib
    st, gst = abi_stack
    assert _lib.FFGP_ACQ_STAGED_MAX_N == 2048      # REFUSALS' n = 2049 is the cap + 1
    kw = dict(bad)
    kw.setdefault("steps", 4)
    rc, X, state, trace, hist, grad = raw_staged(gst, st["X0"], st["level"], S.spec("ucb"), accumulate=1, **kw)
    assert rc == _lib.FFGP_ERR_ARG
    assert torch.equal(X.cpu(), st["X0"]) and not bool(state.any()) and bool((trace == -7.0).all())
    assert bool((hist == -7.0).all()) and bool((grad == -7.0).all())


@pytest.mark.parametrize("accumulate", [0, 1])
def test_c_abi_accepted_call_runs(abi_stack, accumulate):
    st, gst = abi_stack
    sp = S.spec("ucb")
    rc, X, state, trace, hist, grad = raw_staged(gst, st["X0"], st["level"], sp, steps=4, lr=0.01, accumulate=accumulate)
    assert rc == 0
    A = S.loop_a(st, st["X0"], st["level"], sp, 4, 0.01, bool(accumulate))
    assert rel(trace, A[1]) <= 1e-10 and rel(hist, A[2]) <= 1e-10 and torch.equal(X, hist[-1])
    assert bool(state[1].gt(0).any()) and bool(state[2].ne(0).any()) == bool(accumulate)
    _, g = S.cpu_eval(st, A[2][3], st["level"], sp)      # the gradient output is that of the LAST evaluation alone
    assert rel(grad, g) <= 1e-8


# ---- 9. nothing else moved ----------------------------------------------------------------------------------------------------------------
def test_without_the_keyword_a_large_model_keeps_the_per_step_loop():
    c, post, _, _, B, _ = traj(0)
    r = single(post, c["X0"].to(DEV), TRAJ[0][4], STEPS, LR)
    assert r[3]["fused"] is False and not r[3].get("staged")
    assert distance(r, B) <= 1e-12      # the same launches in the same order as loop B
    assert post.acq_staged_ok(c["X0"].to(DEV)) and not post.acq_fusable(c["X0"].to(DEV))


def test_with_the_keyword_a_small_model_keeps_the_one_launch_call_bit_for_bit():
    c, post, _, _, _, one = forced(0)
    sp, steps = FORCED[0][4], FORCED[0][6]
    r = single(post, c["X0"].to(DEV), sp, steps, LR, staged=True)
    assert r[3]["fused"] is True and not r[3].get("staged")
    assert torch.equal(r[0], one[0]) and torch.equal(r[1], one[1]) and torch.equal(r[2], one[2])
    st = S.make_stack((40, 24, 17), 2, (1.0, 0.8, -1.3), 21, seed=701)
    gst = S.gpu_stack(st)
    a = stacked(gst, st["X0"].to(DEV), st["level"], S.spec("ucb"), STEPS, LR)
    b = stacked(gst, st["X0"].to(DEV), st["level"], S.spec("ucb"), STEPS, LR, staged=True)
    assert a[3]["fused"] is True and b[3]["fused"] is True and not b[3].get("staged")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_optimize_acqf_takes_the_keyword():
    """acq.optimize_acqf on a Posterior of 257 points: the final points and the selection rule's point from the staged call against
    the same entry's per-step loop, within the trajectory bound"""
    from fidelityfusion_amd import acq
    c, post0, A, twin, B, _ = traj(0)
    _, bound = yardstick(A, twin, B)
    X0 = c["X0"].to(DEV)
    # a Posterior enters as it stands (no noise added): compare the two routes of the same entry
    slow = acq.optimize_acqf(post0, X0=X0, steps=STEPS, lr=LR, acq="ucb", return_best_only=False)
    fast = acq.optimize_acqf(post0, X0=X0, steps=STEPS, lr=LR, acq="ucb", return_best_only=False, staged=True)
    assert rel(fast, slow) <= bound
    best_s = acq.optimize_acqf(post0, X0=X0, steps=STEPS, lr=LR, acq="ucb")
    best_f = acq.optimize_acqf(post0, X0=X0, steps=STEPS, lr=LR, acq="ucb", staged=True)
    assert rel(best_f, best_s) <= bound
