"""The acquisition optimiser's Adam loop on a NAR chain with COMPOSED kernels (Sum(Linear, Matern-5/2) per fidelity, the reference's
two_fidelity_models/NAR_NonlinearAR.py:23-26) past 256 training points: the staged call
(`PosteriorChain.optimize_acquisition(..., fuse_composed="staged", staged=True)` -> ffgp_acq_optimize_chain_tree_staged,
csrc/acq_staged_chain_tree.hip: launch per stage, every step enqueued by one library call) against the per-step loop such a chain ran
before (`PosteriorChain.predict_diff` + torch.optim.Adam; MF_BayesianOptimization/Discrete/DMF_acq.py:226-262 on
FidelityFusion_Models/NAR.py).  tools/acq_chain_staged_bench.py's shape: the routes alternate in this process, every shape is warmed
up, median [min .. max] of five rounds, every timing ends in a device synchronise.  Every chain is timed with all points at the top
level and with the levels mixed inside every tile ((7 q + 2) mod F).
Gated (fixed before the first run): the staged call's slowest round beats the loop's fastest at every size.  Reported only: the ratio
to ffgp_acq_optimize_chain_staged on squared-exponential members of the same sizes, measured in the same run -- what the leaves'
re-evaluation and the tree's reverse sweep per row cost --, and the forced staged call beside the one-launch call
(ffgp_acq_optimize_chain_tree) at (256, 256), which stays the route at n <= 256 whatever that row says.
    python tools/acq_chain_staged_tree_bench.py [out file, default profiles/acq_chain_staged_tree_bench.txt]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from fidelityfusion_amd import functional as F

dev = torch.device("cuda", 0)
torch.set_default_dtype(torch.float64)
D, Q, STEPS, LR, KAPPA, NOISE, ROUNDS = 8, 500, 30, 0.1, 2.0, 0.05, 5
CHAINS = ((300, 300, 250), (1024, 1024), (2048,))
INFORMATIVE = (256, 256)
LINEAR, M52 = 5, 3


def data(n, seed, extra):
    """tools/acq_chain_tree_bench.py's recipe: inputs on D columns, or (extra) on D + 1, the last standing for the mean below"""
    g = torch.Generator().manual_seed(seed)
    Df = D + (1 if extra else 0)
    X = 2.0 * torch.rand(n, Df, generator=g)
    y = torch.sin(2.0 * X[:, :D].sum(1)) + 0.1 * torch.randn(n, generator=g)
    if extra:
        X[:, D] -= 1.0
        y = y + 0.5 * X[:, D]
    return g, Df, X.to(dev), y.reshape(n, 1).to(dev)


def member(n, seed, extra=False):
    g, Df, X, y = data(n, seed, extra)
    w = 0.6 + torch.rand(Df, generator=g)
    return F.Posterior(X, y, w.to(dev), torch.tensor([1.3], device=dev), torch.tensor([NOISE + 1e-6], device=dev))


def sum_member(n, seed, extra=False):
    g, Df, X, y = data(n, seed, extra)
    wl, wm = (0.6 + torch.rand(Df, generator=g)) / Df ** 0.5, 0.6 + torch.rand(Df, generator=g)
    descs = [{"kfun": LINEAR, "w": wl.to(dev), "amp": torch.tensor([0.6], device=dev), "clamp": float("-inf"), "kparam": 1.0, "center": None},
             {"kfun": M52, "w": wm.to(dev), "amp": torch.tensor([1.2], device=dev), "clamp": 1e-30, "kparam": 0.8, "center": None}]
    return F.Posterior(X, y, None, None, torch.tensor([NOISE + 1e-6], device=dev), tree=(descs, 0))


def make(ns):
    tree = F.PosteriorChain([sum_member(n, 10 + f, extra=f > 0) for f, n in enumerate(ns)])
    radial = F.PosteriorChain([member(n, 10 + f, extra=f > 0) for f, n in enumerate(ns)])
    return tree, radial, (2.0 * torch.rand(Q, D, generator=torch.Generator().manual_seed(1))).to(dev)


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


def rounds(*fns):
    """sorted times of ROUNDS alternating rounds of every function, after a warm-up of each"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(ROUNDS):
        for t, fn in zip(ts, fns):
            t.append(timed(fn))
    return [sorted(t) for t in ts]


def levels(F_):
    out = [("top level   ", None)]
    if F_ > 1:
        out.append(("levels mixed", ((torch.arange(Q) * 7 + 2) % F_).to(dev)))
    return out


def is_staged(st):
    return st["fused"] is False and st.get("staged") is True


FMT = "%8.3f [%8.3f .. %8.3f]"


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "acq_chain_staged_tree_bench.txt")
    mid = ROUNDS // 2
    lines = ["UCB (kappa = 2) on NAR chains of frozen Sum(Linear, Matern-5/2) posteriors (member f > 0 on [x, mean below]), D = %d, Q = %d, %d steps, "
             "lr = %g; ms per call: median [min .. max] of %d alternating rounds; radial staged = ffgp_acq_optimize_chain_staged on "
             "squared-exponential members of the same sizes, in the same run" % (D, Q, STEPS, LR, ROUNDS)]
    print(lines[0], flush=True)
    lost = []
    for ns in CHAINS:
        tree, radial, X0 = make(ns)
        va = [NOISE] * tree.F
        assert tree.acq_chain_tree_staged_ok(X0) and not tree.acq_tree_fusable(X0) and radial.acq_chain_staged_ok(X0)
        for name, level in levels(tree.F):
            kw = dict(steps=STEPS, lr=LR, acq="ucb", kappa=KAPPA, var_adds=va, level=level)
            new = lambda: tree.optimize_acquisition(X0, fuse_composed="staged", staged=True, **kw)
            rad = lambda: radial.optimize_acquisition(X0, staged=True, **kw)
            assert is_staged(new()[3]) and is_staged(rad()[3]), "a call did not take its staged path"
            assert tree.optimize_acquisition(X0, fuse_composed=True, staged=True, **dict(kw, steps=2))[3]["fused"] is False      # the route before
            tn, tl, tr = rounds(new, lambda: loop(lambda X: tree.predict_diff(X, level=level, var_adds=va), X0, STEPS), rad)
            lines.append(("chain n=%-16s %s  staged " + FMT + " (%.4f ms/step)   per-step loop " + FMT + "   x%.2f   radial staged " + FMT
                          + "   tree / radial %.2f")
                         % (ns, name, tn[mid], tn[0], tn[-1], tn[mid] / STEPS, tl[mid], tl[0], tl[-1], tl[mid] / tn[mid], tr[mid], tr[0], tr[-1],
                            tn[mid] / tr[mid]))
            print(lines[-1], flush=True)
            if not tn[-1] < tl[0]:
                lost.append((ns, name.strip()))
    lines.append("gated: the staged call's slowest round beats the per-step loop's fastest at every size: %s" % ("NOT met at %s" % lost if lost else "met"))
    print(lines[-1], flush=True)
    # reported only: the forced staged call beside the one-launch call where both serve
    tree, _, X0 = make(INFORMATIVE)
    va = [NOISE] * tree.F
    for name, level in levels(tree.F):
        kw = dict(steps=STEPS, lr=LR, acq="ucb", kappa=KAPPA, var_adds=va, level=level)
        forced = lambda: tree.optimize_acquisition(X0, fuse_composed="staged", staged="force", **kw)
        one = lambda: tree.optimize_acquisition(X0, fuse_composed="staged", staged=True, **kw)
        assert is_staged(forced()[3]) and one()[3]["fused"] is True
        tf, to = rounds(forced, one)
        lines.append(("chain n=%-16s %s  forced staged " + FMT + "   one-launch call " + FMT + "   staged / one-launch %.2f (reported only)")
                     % (INFORMATIVE, name, tf[mid], tf[0], tf[-1], to[mid], to[0], to[-1], tf[mid] / to[mid]))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert not lost, "the staged call is not ahead of the per-step loop at %s" % lost


if __name__ == "__main__":
    main()
