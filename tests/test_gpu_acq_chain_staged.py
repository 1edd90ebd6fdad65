"""The acquisition optimiser on a NAR chain past 256 training points: the launch-per-stage loop inside one library call
(ffgp_acq_optimize_chain_staged, csrc/acq_staged_chain.hip; `staged=True` on PosteriorChain.optimize_acquisition and
acq.optimize_acqf_nar) against the references test_gpu_acq_chain.py is written against -- plain fp64 torch on the CPU, the per-step
loop on the GPU, the one-launch chain kernel where it still serves -- and a fixture of the reference's own loop on its NAR at its
demo's sizes (tests/golden/mf_acq_nar_n300.npz, written by tests/golden/gen_nar_acq_staged_goldens.py).

Helpers, recipes and bars are test_gpu_acq_chain.py's and test_gpu_acq_staged.py's, imported and unchanged.  Evaluate mode (steps = 0):
values rel. 1e-10, gradients rel. 1e-8.  Trajectories: (A) the CPU loop and (B) the per-step GPU loop differ by rounding only; d0 =
their distance is the yardstick, max(10 d0, 1e-12) the bound, a case with d0 > 1e-10 fails as ill-conditioned, and a CPU twin started
one ulp away must stay within 1e-11 before anything is compared (`yardstick`).  State: 3 + 5 steps equal 8 bit for bit.  level = k for
all points is the cut chain bit for bit (the same Q, so the same GEMM shapes); cutting Q can change the tile shape the fp64 GEMM picks
for V = L^-1 K_s and B = L^-T V, so a point alone is held to a relative distance of 1e-13, not to equality, as test_gpu_acq_staged.py
explains.  Every case runs a few steps on the smallest shapes that reach a boundary: a first member one row past the one-launch limit
(257), a smaller member behind a larger one, a chunk of 2 rows (130), two column tiles with a ragged second (Q = 70), DM = 16 with
4 chunks + 1 row (513), F = 1 with Q = 1, and the demo's (300, 300, 250)."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_acq_chain as CH                                  # noqa: E402
from test_gpu_acq_chain import ACQ_CODE, DEV, LINEAR, NEG_INF, SE, distance, rel, spec      # noqa: E402
from test_gpu_acq_staged import STEPS, is_staged, yardstick      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(torch.float32)


# ---- the GPU side --------------------------------------------------------------------------------------------------------------------
def raw_staged(gch, Xq, level, sp, steps=0, lr=0.1, step0=0, Q=None, null=(), F=None, accumulate=0, acq=None, member=0, **over):
    """ffgp_acq_optimize_chain_staged through ctypes: test_gpu_acq_chain.raw_call with the staged entry.  `over` overrides fields of
    member `member`, `null` names pointers to pass as NULL.  Returns (status, X, state, trace, hist, grad), every buffer pre-filled."""
    from fidelityfusion_amd import _lib
    keep = []
    tab = gch._member_table(gch.test_var_adds, keep)
    for k, v in over.items():
        setattr(tab[member], k, v)
    Qn, D = Xq.shape
    X = Xq.to(DEV).clone().contiguous()
    state = torch.zeros((3, Qn, D), device=DEV)
    trace = torch.full((max(steps, 1), Qn), -7.0, device=DEV)
    hist = torch.full((max(steps, 0) + 1, Qn, D), -7.0, device=DEV)
    grad = torch.full((Qn, D), -7.0, device=DEV)
    lv = None if level is None else level.to(device=DEV, dtype=torch.int32).contiguous()
    s = _lib.AcqChain(F=gch.F if F is None else F, members=None if "members" in null else tab, level_dev=None if lv is None else lv.data_ptr(),
                      var_floor=sp["var_floor"], acq=ACQ_CODE[sp["acq"]] if acq is None else acq, kappa=sp["kappa"], xi=sp["xi"],
                      f_best=sp["f_best"], accumulate_grad=accumulate)
    opt = _lib.Adam(lr, 0.9, 0.999, 1e-8)
    ptr = lambda name, t: None if name in null else C.c_void_p(t.data_ptr())
    rc = _lib.lib.ffgp_acq_optimize_chain_staged(None if "h" in null else gch.members[0]._h(), None if "s" in null else C.byref(s), ptr("X", X),
                                                 Qn if Q is None else Q, steps, None if "opt" in null else C.byref(opt), ptr("state", state),
                                                 step0, ptr("trace", trace), ptr("hist", hist), ptr("grad", grad))
    torch.cuda.synchronize()
    return rc, X, state, trace, hist, grad


def chained(gch, X0, level, sp, steps, lr, accumulate=False, state=None, **kw):
    """test_gpu_acq_chain.fused with further keywords (`staged`)"""
    return gch.optimize_acquisition(X0, steps=steps, lr=lr, acq=sp["acq"], kappa=sp["kappa"], xi=sp["xi"], f_best=sp["f_best"],
                                    var_floor=sp["var_floor"], level=None if level is None else level.to(DEV), var_adds=gch.test_var_adds,
                                    accumulate_grad=accumulate, state=state, **kw)


# ---- 1. values and gradients (steps = 0) against CPU autograd --------------------------------------------------------------------------
#          ns              D   Q
EVAL = [((257, 40, 130), 1, 37),      # the first member one row past the limit; a smaller member behind a larger one; a chunk of 2 rows
        ((40, 300), 2, 70),           # two column tiles, the second ragged
        ((129, 513), 15, 21),         # DM = 16; 4 chunks + 1 row
        ((300,), 2, 1)]               # F = 1, Q = 1


@functools.lru_cache(maxsize=None)
def eval_chain(i):
    ns, D, Q = EVAL[i]
    ch = CH.make_chain(ns, D, Q, seed=900 + i)
    return ch, CH.gpu_chain(ch)


@pytest.mark.parametrize("acq", ["ucb", "ei", "ucb_var"])
@pytest.mark.parametrize("i", range(len(EVAL)))
def test_evaluate_matches_cpu_autograd(i, acq):
    ch, gch = eval_chain(i)
    sp = spec(acq, f_best=0.3, kappa=2.0 if acq != "ucb_var" else 0.4)
    rc, X, _, trace, _, grad = raw_staged(gch, ch["X0"], ch["level"], sp)
    assert rc == 0
    assert torch.equal(X.cpu(), ch["X0"])      # evaluate mode: nothing moves
    a, g = CH.cpu_eval(ch, ch["X0"], ch["level"], sp)
    ev, eg = rel(trace[0], a), rel(grad, g)
    print("staged chain %s D=%d Q=%d %s: value rel %.2e, gradient rel %.2e" % (EVAL[i] + (acq, ev, eg)))
    assert ev <= 1e-10, ev
    assert eg <= 1e-8, eg


def test_evaluate_without_levels():
    ch, gch = eval_chain(0)
    sp = spec("ucb")
    rc, _, _, trace, _, grad = raw_staged(gch, ch["X0"], None, sp)
    assert rc == 0
    a, g = CH.cpu_eval(ch, ch["X0"], None, sp)
    assert rel(trace[0], a) <= 1e-10 and rel(grad, g) <= 1e-8


# ---- 2. trajectories against the per-step GPU loop and the CPU loop -------------------------------------------------------------------
#          ns               D   Q   acquisition                  seed
CHAINS = [((257, 40, 130), 1, 37, spec("ucb"), 910),
          ((40, 300), 2, 70, spec("ei", f_best=0.3), 911),
          ((129, 513), 15, 21, spec("ucb_var", kappa=0.4), 912),
          ((300, 300, 250), 2, 37, spec("ucb"), 913)]
TRAJ = [(i, acc) for i in range(len(CHAINS)) for acc in (False, True)]


def traj_case(i, accumulate, steps=STEPS):
    """the CPU side of case i: the chain, loop A and its twin"""
    ns, D, Q, sp, seed = CHAINS[i]
    lr = 0.01 if accumulate else 0.1
    ch = CH.make_chain(ns, D, Q, seed=seed)
    A = CH.loop_a(ch, ch["X0"], ch["level"], sp, steps, lr, accumulate)
    twin = CH.loop_a(ch, ch["X0"] * (1.0 + 2e-16), ch["level"], sp, steps, lr, accumulate)
    return ch, A, twin, lr


@functools.lru_cache(maxsize=None)
def traj(i, accumulate):
    """case i once: the CPU loop, its twin, loop B, the staged call -- shared by the tests below and left unchanged"""
    ch, A, twin, lr = traj_case(i, accumulate)
    sp = CHAINS[i][3]
    gch = CH.gpu_chain(ch)
    B = CH.loop_b(gch, ch["X0"], ch["level"], sp, STEPS, lr, accumulate)
    X0d = ch["X0"].to(DEV)
    keep = X0d.clone()
    Z = chained(gch, X0d, ch["level"], sp, STEPS, lr, accumulate, staged=True)
    assert torch.equal(X0d, keep)      # X0 is left untouched
    return ch, gch, A, twin, B, Z, lr


@pytest.mark.parametrize("i,accumulate", TRAJ)
def test_trajectory_follows_both_references(i, accumulate):
    ch, gch, A, twin, B, Z, lr = traj(i, accumulate)
    d0, bound = yardstick(A, twin, B)
    dA, dB = distance(Z, A), distance(Z, B)
    print("staged chain %d accumulate=%s: d0 %.2e, bound %.2e, staged vs A %.2e, vs B %.2e" % (i, accumulate, d0, bound, dA, dB))
    Q, D = ch["X0"].shape
    assert is_staged(Z[3]) and Z[3]["step"] == STEPS and ("grad_sum" in Z[3]) == accumulate
    assert Z[1].shape == (STEPS, Q) and Z[2].shape == (STEPS + 1, Q, D)
    assert torch.equal(Z[0], Z[2][-1]) and torch.equal(Z[2][0].cpu(), ch["X0"])
    assert dA <= bound, (dA, bound)
    assert dB <= bound, (dB, bound)


# ---- 3. the forced staged call against the one-launch chain call -------------------------------------------------------------------------
#          ns             D   Q   acquisition   seed  steps
FORCED = [((40, 24, 17), 2, 37, spec("ucb"), 920, 30),
          ((256, 200), 15, 20, spec("ucb"), 921, STEPS)]


@functools.lru_cache(maxsize=None)
def forced(i):
    ns, D, Q, sp, seed, steps = FORCED[i]
    ch = CH.make_chain(ns, D, Q, seed=seed)
    A = CH.loop_a(ch, ch["X0"], ch["level"], sp, steps, 0.1)
    twin = CH.loop_a(ch, ch["X0"] * (1.0 + 2e-16), ch["level"], sp, steps, 0.1)
    gch = CH.gpu_chain(ch)
    B = CH.loop_b(gch, ch["X0"], ch["level"], sp, steps, 0.1)
    one = chained(gch, ch["X0"].to(DEV), ch["level"], sp, steps, 0.1)
    return ch, gch, A, twin, B, one


@pytest.mark.parametrize("i", range(len(FORCED)))
def test_forced_staged_call_follows_the_one_launch_call(i):
    ch, gch, A, twin, B, one = forced(i)
    sp, steps = FORCED[i][3], FORCED[i][5]
    d0, bound = yardstick(A, twin, B)
    Z = chained(gch, ch["X0"].to(DEV), ch["level"], sp, steps, 0.1, staged="force")
    assert one[3]["fused"] is True and not one[3].get("staged") and is_staged(Z[3])
    dO, dA = distance(Z, one), distance(Z, A)
    print("forced chain %s: d0 %.2e, bound %.2e, staged vs one-launch %.2e, vs A %.2e" % (FORCED[i][0], d0, bound, dO, dA))
    assert dO <= bound and dA <= bound, (dO, dA, bound)
    # staged=True alone leaves a fusable chain on the one-launch call, bit for bit
    r = chained(gch, ch["X0"].to(DEV), ch["level"], sp, steps, 0.1, staged=True)
    assert r[3]["fused"] is True and not r[3].get("staged")
    assert torch.equal(r[0], one[0]) and torch.equal(r[1], one[1]) and torch.equal(r[2], one[2])


# ---- 4. state ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,accumulate", [(0, False), (0, True), (3, True)])
def test_state_continues_the_optimiser_bit_for_bit(i, accumulate):
    ch, gch, _, _, _, Z, lr = traj(i, accumulate)
    sp = CHAINS[i][3]
    X1, t1, h1, s1 = chained(gch, ch["X0"].to(DEV), ch["level"], sp, 3, lr, accumulate, staged=True)
    assert is_staged(s1) and s1["step"] == 3
    X2, t2, h2, s2 = chained(gch, X1, ch["level"], sp, 5, lr, accumulate, state=s1, staged=True)
    assert is_staged(s2) and s2["step"] == STEPS == 8
    assert torch.equal(X2, Z[0])
    assert torch.equal(torch.cat([t1, t2]), Z[1])
    assert torch.equal(torch.cat([h1[:-1], h2]), Z[2])
    assert torch.equal(s2["exp_avg"], Z[3]["exp_avg"]) and torch.equal(s2["exp_avg_sq"], Z[3]["exp_avg_sq"])
    if accumulate:
        assert torch.equal(s2["grad_sum"], Z[3]["grad_sum"]) and bool(s2["grad_sum"].ne(0).any())


def test_one_launch_state_is_continued_by_the_staged_call():
    ch, gch, A, twin, B, one = forced(0)      # 30 one-launch steps
    sp = FORCED[0][3]
    _, bound = yardstick(A, twin, B)
    X1, t1, h1, s1 = chained(gch, ch["X0"].to(DEV), ch["level"], sp, 12, 0.1)
    assert s1["fused"] is True
    X2, t2, h2, s2 = chained(gch, X1, ch["level"], sp, 18, 0.1, state=s1, staged="force")
    assert is_staged(s2) and s2["step"] == 30
    got = (X2, torch.cat([t1, t2]), torch.cat([h1[:-1], h2]))
    d, dA = distance(got, one), distance(got, A)
    print("12 one-launch + 18 staged steps vs 30 one-launch steps: %.2e, vs A %.2e (bound %.2e)" % (d, dA, bound))
    assert d <= bound and dA <= bound and rel(X2, one[0]) <= bound


# ---- 5. levels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [False, True])
def test_a_level_for_all_points_is_the_cut_chain(accumulate):
    from fidelityfusion_amd import functional as F
    ch, gch, _, _, _, _, lr = traj(0, accumulate)
    sp, X0 = CHAINS[0][3], ch["X0"].to(DEV)
    top = chained(gch, X0, None, sp, STEPS, lr, accumulate, staged=True)
    assert is_staged(top[3])
    for k in range(ch["F"]):
        # the same Posterior objects: a member factored again has its alpha solved on other inverted diagonal blocks
        cut_chain = F.PosteriorChain(gch.members[:k + 1])
        cut_chain.test_var_adds = gch.test_var_adds[:k + 1]
        cut = chained(cut_chain, X0, None, sp, STEPS, lr, accumulate, staged=True)
        lev = chained(gch, X0, torch.full((X0.shape[0],), k), sp, STEPS, lr, accumulate, staged=True)
        assert is_staged(cut[3]) and is_staged(lev[3])
        assert torch.equal(cut[0], lev[0]) and torch.equal(cut[1], lev[1]) and torch.equal(cut[2], lev[2])
        assert torch.equal(cut[3]["exp_avg"], lev[3]["exp_avg"]) and torch.equal(cut[3]["exp_avg_sq"], lev[3]["exp_avg_sq"])
        if k < ch["F"] - 1:
            assert not torch.equal(cut[1], top[1])      # the members above k do change the result
        else:
            assert torch.equal(cut[1], top[1]) and torch.equal(cut[2], top[2])      # level = F - 1 everywhere is level_dev = NULL


def test_a_point_does_not_depend_on_its_neighbours_or_their_levels():
    ch, gch, _, _, _, Z, lr = traj(0, False)
    sp, X0, lv = CHAINS[0][3], ch["X0"].to(DEV), ch["level"]
    # alone: only its own member's chains run, and the GEMM sees one column
    for q in (0, 20, 36):
        r = chained(gch, X0[q:q + 1].contiguous(), lv[q:q + 1], sp, STEPS, lr, staged=True)
        d = max(rel(r[1][:, 0], Z[1][:, q]), rel(r[2][:, 0], Z[2][:, q]))
        print("point %d (level %d) alone: %.2e" % (q, int(lv[q]), d))
        assert d <= 1e-13, d
    # in another column, beside other neighbours: the points in reverse order
    idx = torch.arange(X0.shape[0] - 1, -1, -1)
    r = chained(gch, X0[idx.to(DEV)].contiguous(), lv[idx], sp, STEPS, lr, staged=True)
    d = max(rel(r[1], Z[1][:, idx.to(DEV)]), rel(r[2], Z[2][:, idx.to(DEV)]))
    print("all points in reverse order: %.2e" % d)
    assert d <= 1e-13, d


def test_c_abi_reads_a_negative_level_as_no_member():
    """in C a negative level matches no member (Python refuses it): value 0, gradient 0, the point does not move; its neighbours are
    served bit for bit as without it (the same Q: the same GEMM shapes)"""
    ch, gch = eval_chain(0)
    sp = spec("ucb")
    lv = ch["level"].clone()
    lv[3] = -1
    lv[36] = -5
    rc, X, _, trace, hist, grad = raw_staged(gch, ch["X0"], lv, sp, steps=3, lr=0.1)
    ref = raw_staged(gch, ch["X0"], ch["level"], sp, steps=3, lr=0.1)
    assert rc == 0 and ref[0] == 0
    for q in (3, 36):
        assert bool((trace[:, q] == 0.0).all()) and bool((grad[q] == 0.0).all()) and torch.equal(X[q].cpu(), ch["X0"][q])
        assert torch.equal(hist[:, q].cpu(), ch["X0"][q].expand(4, ch["D"]))
    others = [q for q in range(ch["X0"].shape[0]) if q not in (3, 36)]
    assert torch.equal(trace[:, others], ref[3][:, others]) and torch.equal(hist[:, others], ref[4][:, others])
    assert torch.equal(grad[others], ref[5][others])
    # every level negative: no member runs at all
    rc, X, _, trace, hist, grad = raw_staged(gch, ch["X0"], torch.full_like(lv, -1), sp, steps=2, lr=0.1)
    assert rc == 0 and not bool(trace.any()) and not bool(grad.any()) and torch.equal(X.cpu(), ch["X0"])


# ---- 6. the fixture of the reference's loop at (300, 300, 250) ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "mf_acq_nar_n300.npz"))
    t = lambda k: torch.tensor(z[k])
    members = []
    for f in range(3):
        x, y = t("x_%d" % f), t("y_%d" % f)
        noise = math.exp(-float(z["log_beta"][f]))
        members.append({"X": x, "Y": y, "w": torch.full((x.shape[1],), math.exp(-float(z["log_length_scale"][f]))),
                        "amp": math.exp(float(z["log_signal_variance"][f])) ** 2, "kfun": SE, "kparam": 1.0, "clamp": NEG_INF,
                        "dadd": noise + 1e-6, "var_add": noise})
    ch = {"members": members, "F": 3, "D": 2}
    return z, ch, CH.gpu_chain(ch)


@pytest.mark.parametrize("tag", ["zg", "acc"])
def test_staged_call_reproduces_the_reference_fixture_at_every_level(tag):
    """the procedure and bars of test_gpu_acq_chain.py's fixture test, on the fixture of the demo's sizes"""
    z, ch, gch = fixture()
    assert [m["X"].shape[0] for m in ch["members"]] == [300, 300, 250]
    assert float(z["twin_distance"]) <= 1e-11
    steps, lr, acc = int(z["steps"]), float(z["lr"]), tag == "acc"
    sp = spec("ucb_var", kappa=float(z["kappa"]))
    X0 = torch.tensor(z["X0"])                           # [3, 6, 2]: six starts per level
    level = torch.arange(3).repeat_interleave(6)
    Z = chained(gch, X0.reshape(18, 2).to(DEV), level, sp, steps, lr, acc, staged=True)      # every level from one call
    assert is_staged(Z[3])
    for s in range(3):
        ref = (None, torch.tensor(z["trace_" + tag][s]), torch.tensor(z["hist_" + tag][s]))
        B = CH.loop_b(gch, X0[s], torch.full((6,), s), sp, steps, lr, acc)
        d0 = distance(B, ref)
        assert d0 <= 1e-10, "ill-conditioned case: d0 = %.2e" % d0
        bound = max(10.0 * d0, 1e-12)
        got = (None, Z[1][:, 6 * s:6 * s + 6], Z[2][:, 6 * s:6 * s + 6])
        print("fixture nar n300 %s level %d: d0 %.2e, bound %.2e, staged vs fixture %.2e, vs B %.2e" % (tag, s, d0, bound, distance(got, ref),
                                                                                                     distance(got, B)))
        assert distance(got, ref) <= bound and distance(got, B) <= bound
        assert rel(Z[0][6 * s:6 * s + 6], ref[2][-1]) <= bound      # the final points


def test_optimize_acqf_nar_selects_as_the_reference_rule_does_on_the_fixture():
    from fidelityfusion_amd import acq, kernel
    from fidelityfusion_amd.cigp_v10 import cigp
    z, ch, gch = fixture()
    steps, lr = int(z["steps"]), float(z["lr"])
    models, data = [], []
    for f in range(3):
        m = cigp(kernel.SquaredExponentialKernel(float(z["log_length_scale"][f]), float(z["log_signal_variance"][f])), float(z["log_beta"][f]))
        m = m.double().to(DEV)
        m.requires_grad_(False)
        models.append(m)
        x, y = torch.tensor(z["x_%d" % f], device=DEV), torch.tensor(z["y_%d" % f], device=DEV)
        data.append((x, y) if f == 0 else (x, [y, torch.full_like(y, 0.01)]))      # the trainer stores [y, y_var] above fidelity 0
    sp = spec("ucb_var", kappa=float(z["kappa"]))
    for s in range(3):
        X0 = torch.tensor(z["X0"][s])
        ref_t, ref_h = torch.tensor(z["trace_zg"][s]), torch.tensor(z["hist_zg"][s])
        k_ref, best_ref = CH.select(X0, ref_t, ref_h)
        B = CH.loop_b(gch, X0, torch.full((6,), s), sp, steps, lr)
        d0 = distance(B, (None, ref_t, ref_h))
        assert d0 <= 1e-10
        bound = max(10.0 * d0, 1e-12)
        kw = dict(level=s, steps=steps, lr=lr, acq="ucb_var", kappa=float(z["kappa"]), staged=True)
        best = acq.optimize_acqf_nar(models, data, X0.to(DEV), **kw)
        final = acq.optimize_acqf_nar(models, data, X0.to(DEV), return_best_only=False, **kw)
        scale = float(ref_h.abs().max())
        e_best, e_final = float((best.cpu() - best_ref).abs().max()) / scale, float((final.cpu() - ref_h[-1]).abs().max()) / scale
        print("optimize_acqf_nar staged level %d: selected step %d, d0 %.2e, best_x %.2e, final %.2e" % (s, k_ref, d0, e_best, e_final))
        assert k_ref >= 0
        assert e_best <= bound and e_final <= bound, (e_best, e_final, bound)


# ---- 7. fall-backs and refusals -----------------------------------------------------------------------------------------------------------
def _keeps_the_loop(gch, X0, level, sp, accumulate=False, steps=4, **kw):
    keep = X0.clone()
    r = chained(gch, X0, level, sp, steps, 0.1, accumulate, **kw)
    assert r[3]["fused"] is False and "staged" not in r[3] and ("grad_sum" in r[3]) == accumulate
    assert torch.equal(X0, keep)
    B = CH.loop_b(gch, X0, level, sp, steps, 0.1, accumulate)
    for got, want in zip(r[:3], B):
        assert got.device == X0.device
        assert rel(got, want) <= 1e-12
    return r


def test_without_the_keyword_a_large_chain_keeps_the_per_step_loop():
    ch = CH.make_chain((40, 260), 2, 19, seed=602)
    gch = CH.gpu_chain(ch)
    X0 = ch["X0"].to(DEV)
    assert gch.acq_chain_staged_ok(X0) and not gch.acq_fusable(X0)
    _keeps_the_loop(gch, X0, ch["level"], spec("ucb"))
    assert is_staged(chained(gch, X0, ch["level"], spec("ucb"), 4, 0.1, staged=True)[3])


def test_with_the_keyword_a_composed_member_keeps_the_per_step_loop():
    from fidelityfusion_amd import functional as F, kernel
    from fidelityfusion_amd.cigp_v10 import cigp
    D = 2
    ch = CH.make_chain((40, 260), D, 19, seed=930)
    c = ch["members"][1]
    m = cigp(kernel.SumKernel(kernel.ARDKernel(D + 1), kernel.MaternKernel(D + 1)).double(), log_beta=3.0).double().to(DEV)
    m.requires_grad_(False)
    odd = m._cached_posterior(c["X"].to(DEV), c["Y"].to(DEV))[0]
    assert odd.tree is not None
    gch = F.PosteriorChain([CH.gpu_posterior(ch["members"][0]), odd])
    gch.test_var_adds = [0.05, 0.05]
    X0 = ch["X0"].to(DEV)
    assert not gch.acq_chain_staged_ok(X0)
    _keeps_the_loop(gch, X0, ch["level"], spec("ucb"), staged=True)
    _keeps_the_loop(gch, X0, ch["level"], spec("ucb_var", kappa=0.4), accumulate=True, staged="force")


def test_with_the_keyword_a_member_beyond_the_cap_keeps_the_per_step_loop():
    ch = CH.make_chain((40, 2049), 2, 19, seed=931)
    gch = CH.gpu_chain(ch)
    assert not gch.acq_chain_staged_ok(ch["X0"].to(DEV))
    _keeps_the_loop(gch, ch["X0"].to(DEV), ch["level"], spec("ucb"), staged=True)


# the chain test's list with the staged cap + 1 in place of the one-launch limit + 1 (coefficients other than 1 are in it)
REFUSALS = [dict(b, n=2049) if b.get("n") == 257 else b for b in CH.REFUSALS]


@pytest.fixture(scope="module")
def abi_chain():
    ch = CH.make_chain((40, 24, 17), 2, 21, seed=701)
    return ch, CH.gpu_chain(ch)


@pytest.mark.parametrize("bad", REFUSALS, ids=lambda b: ",".join("%s=%s" % kv for kv in b.items()))
def test_c_abi_refuses_before_anything_is_enqueued(abi_chain, bad):
    from fidelityfusion_amd import _lib
    ch, gch = abi_chain
    assert _lib.FFGP_ACQ_STAGED_MAX_N == 2048 and sum(1 for b in REFUSALS if b.get("n") == 2049) == 2      # the cap + 1
    assert sum(1 for b in REFUSALS if "mean_coef" in b or "var_coef" in b) == 3 and not any(b.get("n") == 257 for b in REFUSALS)
    kw = dict(bad)
    kw.setdefault("steps", 4)
    rc, X, state, trace, hist, grad = raw_staged(gch, ch["X0"], ch["level"], spec("ucb"), accumulate=1, **kw)
    assert rc == _lib.FFGP_ERR_ARG
    assert torch.equal(X.cpu(), ch["X0"]) and not bool(state.any()) and bool((trace == -7.0).all())
    assert bool((hist == -7.0).all()) and bool((grad == -7.0).all())


@pytest.mark.parametrize("accumulate", [0, 1])
def test_c_abi_accepted_call_runs(abi_chain, accumulate):
    ch, gch = abi_chain
    sp = spec("ucb")
    rc, X, state, trace, hist, grad = raw_staged(gch, ch["X0"], ch["level"], sp, steps=4, lr=0.01, accumulate=accumulate)
    assert rc == 0
    A = CH.loop_a(ch, ch["X0"], ch["level"], sp, 4, 0.01, bool(accumulate))
    assert rel(trace, A[1]) <= 1e-10 and rel(hist, A[2]) <= 1e-10 and torch.equal(X, hist[-1])
    assert bool(state[1].gt(0).any()) and bool(state[2].ne(0).any()) == bool(accumulate)
    _, g = CH.cpu_eval(ch, A[2][3], ch["level"], sp)      # the gradient output is that of the LAST evaluation alone
    assert rel(grad, g) <= 1e-8
