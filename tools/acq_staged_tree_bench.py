"""The acquisition optimiser's Adam loop on COMPOSED-kernel models past 256 training points: the staged call
(`optimize_acquisition(..., fuse_composed=True, staged=True)` -> ffgp_acq_optimize_stack_tree_staged, csrc/acq_staged_tree.hip: launch
per stage, every step enqueued by one library call) against the per-step loop a caller runs there today (predict_diff +
torch.optim.Adam, Bayesian_optimization/acq.py:48-62; on a stack MF_BayesianOptimization/Discrete/DMF_acq.py:226-262).  The models are
the reference's: SumKernel(LinearKernel, MaternKernel) (Bayesian_optimization/cigp.py:119; AR / ResGP on every fidelity), and one
four-leaf tree.  tools/acq_staged_bench.py's method: both in this process, alternating, median [min .. max] of three rounds each after
a warm-up of either; every timing ends in a device synchronise.  The tool asserts that the staged call's slowest round beats the loop's
fastest at every size above 256.  The last row -- n = 256 forced onto the staged call beside the one-launch tree call that serves it --
is informative only.
    python tools/acq_staged_tree_bench.py [out file, default profiles/acq_staged_tree_bench.txt]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from fidelityfusion_amd import functional as F

dev = torch.device("cuda", 0)
torch.set_default_dtype(torch.float64)
Q, STEPS, LR, KAPPA, NOISE = 500, 30, 0.1, 2.0, 0.05
SE, M12, M52, LINEAR = 0, 1, 3, 5                # FFGP_KFUN_*
SUM, PRODUCT, CHAIN = 0, 1, 0                    # FFGP_KOP_*, FFGP_TREE_CHAIN
SINGLES = ((300, 2), (1024, 8), (2048, 8))       # (n, D) on Sum(Linear, Matern-5/2)
STACK = ((300, 300, 250), 2, (1.0, 0.8, 1.2))    # the reference demo's sizes, D, AR's (1, rho_0, rho_1)
FOUR = (1024, 16)                                # ((Linear + SE) x Matern-5/2) + Matern-1/2
INFORMATIVE = (256, 8)


def leaf(g, D, kfun, amp, kparam=1.0, center=None):
    w = 0.6 + torch.rand(D, generator=g)
    if kfun == LINEAR:
        w = w / D ** 0.5      # k_lin stays O(1) over the box at every D
    return {"kfun": kfun, "w": w.to(dev), "amp": torch.tensor([amp], device=dev), "kparam": kparam,
            "clamp": 1e-30 if kfun in (M12, M52) else float("-inf"), "center": None if center is None else torch.full((D,), center, device=dev)}


def make(n, D, seed=0, four=False):
    g = torch.Generator().manual_seed(seed)
    X = 2.0 * torch.rand(n, D, generator=g)
    y = (torch.sin(2.0 * X.sum(1)) + 0.1 * torch.randn(n, generator=g)).reshape(n, 1)
    if four:
        descs = [leaf(g, D, LINEAR, 0.5, center=0.2), leaf(g, D, SE, 1.0), leaf(g, D, M52, 0.9, 0.8), leaf(g, D, M12, 0.4, 1.3)]
        op = (CHAIN, (SUM, PRODUCT, SUM))
    else:
        descs, op = [leaf(g, D, LINEAR, 0.6), leaf(g, D, M52, 1.2, 0.8)], SUM
    return F.Posterior(X.to(dev), y.to(dev), None, None, torch.tensor([NOISE + 1e-6], device=dev), tree=(descs, op))


def starts(D, seed=99):
    return (2.0 * torch.rand(Q, D, generator=torch.Generator().manual_seed(seed))).to(dev)


def loop(predict, X0, steps):
    X = X0.clone().requires_grad_(True)
    opt = torch.optim.Adam([X], lr=LR)
    for _ in range(steps):
        opt.zero_grad()
        mean, var = predict(X)
        loss = -(mean + KAPPA * torch.sqrt(torch.clamp_min(var.reshape(-1, 1), 1e-12))).sum()
        loss.backward()
        opt.step()
    return X.detach()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def rounds(a, b):
    """three alternating rounds of a and b after a warm-up of either: their sorted times"""
    ta, tb = [], []
    for _ in range(3):
        ta.append(timed(a))
        tb.append(timed(b))
    return sorted(ta), sorted(tb)


def row(what, name_b, ta, tb):
    return ("%-38s staged %8.3f [%8.3f .. %8.3f] (%.4f ms/step)   %s %8.3f [%8.3f .. %8.3f] (%.4f ms/step)   x%.2f"
            % (what, ta[1], ta[0], ta[2], ta[1] / STEPS, name_b, tb[1], tb[0], tb[2], tb[1] / STEPS, tb[1] / ta[1]))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "acq_staged_tree_bench.txt")
    lines = ["UCB (kappa = 2) on frozen Sum(Linear, Matern-5/2) posteriors, Q = %d, %d steps, lr = %g; ms per call: median [min .. max] of 3 alternating rounds"
             % (Q, STEPS, LR)]
    print(lines[0], flush=True)
    lost = []

    def single(what, n, D, four):
        post, X0 = make(n, D, four=four), starts(D)
        staged = lambda k=STEPS: post.optimize_acquisition(X0, steps=k, lr=LR, acq="ucb", kappa=KAPPA, var_add_all=NOISE, fuse_composed=True,
                                                           staged=True)
        st = staged(3)[3]
        assert st["fused"] is False and st.get("staged") is True, "the call did not take the staged path"
        per_step = lambda k=STEPS: loop(lambda X: post.predict_diff(X, full_cov=False, var_add_all=NOISE), X0, k)
        per_step(3)
        ta, tb = rounds(staged, per_step)
        lines.append(row(what % (n, D), "per-step loop", ta, tb))
        print(lines[-1], flush=True)
        if not ta[2] < tb[0]:
            lost.append((n, D))

    for n, D in SINGLES:
        single("n=%4d D=%2d", n, D, False)
    ns, D, coefs = STACK
    stack = F.PosteriorStack([make(n, D, seed=10 + f) for f, n in enumerate(ns)], coefs)
    X0, va = starts(D), [NOISE] * len(ns)
    staged = lambda k=STEPS: stack.optimize_acquisition(X0, steps=k, lr=LR, acq="ucb", kappa=KAPPA, var_adds=va, fuse_composed=True, staged=True)
    st = staged(3)[3]
    assert st["fused"] is False and st.get("staged") is True, "the stack call did not take the staged path"
    per_step = lambda k=STEPS: loop(lambda X: stack.predict_diff(X, var_adds=va), X0, k)
    per_step(3)
    ta, tb = rounds(staged, per_step)
    lines.append(row("stack n=%s D=%d" % (ns, D), "per-step loop", ta, tb))
    print(lines[-1], flush=True)
    if not ta[2] < tb[0]:
        lost.append((ns, D))
    single("four leaves n=%4d D=%2d", FOUR[0], FOUR[1], True)
    # informative: the one-launch tree call's own size, forced onto the staged call
    n, D = INFORMATIVE
    post, X0 = make(n, D), starts(D)
    kw = dict(lr=LR, acq="ucb", kappa=KAPPA, var_add_all=NOISE, fuse_composed=True)
    forced = lambda k=STEPS: post.optimize_acquisition(X0, steps=k, staged="force", **kw)
    one = lambda k=STEPS: post.optimize_acquisition(X0, steps=k, **kw)
    assert forced(3)[3].get("staged") is True and one(3)[3]["fused"] is True
    ta, tb = rounds(forced, one)
    lines.append(row("n=%4d D=%2d forced (informative)" % (n, D), "one-launch call", ta, tb))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert not lost, "the staged call is not ahead of the per-step loop at (n, D) = %s" % lost


if __name__ == "__main__":
    main()
