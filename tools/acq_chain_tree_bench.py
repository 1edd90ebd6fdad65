"""The acquisition optimiser's Adam loop on a CHAIN of frozen posteriors with COMPOSED kernels (NAR on SumKernel(LinearKernel,
MaternKernel) fidelities): the one-launch call (PosteriorChain.optimize_acquisition(..., fuse_composed=True) ->
ffgp_acq_optimize_chain_tree, csrc/acq_chain_tree.hip) against the per-step loop it replaces (PosteriorChain.predict_diff +
torch.optim.Adam, what the same call runs without the keyword).  Both in this process, alternating, median [min .. max] of five rounds
each after a warm-up of either; every timing ends in a device synchronise.  The radial chain call (ffgp_acq_optimize_chain) on a chain
of squared-exponential members of the same sizes is measured in the same run: the ratio to it is what the leaves' re-evaluation and the
tree's reverse sweep per row cost.  Every size runs with all points at the top level and with the points dealt to the levels in turn
(mixed inside every tile).  The tool asserts only that the fused call's slowest round beats the loop's fastest.
      python tools/acq_chain_tree_bench.py [out file, default profiles/acq_chain_tree_bench.txt]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from fidelityfusion_amd import functional as F

dev = torch.device("cuda", 0)
torch.set_default_dtype(torch.float64)
CHAINS = (((32, 32, 32), 8, 500, 30), ((128, 128, 96), 8, 500, 30), ((256, 256), 8, 500, 30))      # (ns, D, Q, steps)
KAPPA, NOISE, ROUNDS = 2.0, 0.05, 5
LINEAR, M52 = 5, 3


def data(n, D, seed, extra):
    """inputs on D columns, or (extra) on D + 1: the last column stands for the mean of the member below"""
    g = torch.Generator().manual_seed(seed)
    Df = D + (1 if extra else 0)
    X = 2.0 * torch.rand(n, Df, generator=g)
    y = torch.sin(2.0 * X[:, :D].sum(1)) + 0.1 * torch.randn(n, generator=g)
    if extra:
        X[:, D] -= 1.0
        y = y + 0.5 * X[:, D]
    return g, Df, X.to(dev), y.reshape(n, 1).to(dev)


def member(n, D, seed, extra=False):
    """a posterior on one squared-exponential kernel"""
    g, Df, X, y = data(n, D, seed, extra)
    w = 0.6 + torch.rand(Df, generator=g)
    return F.Posterior(X, y, w.to(dev), torch.tensor([1.3], device=dev), torch.tensor([NOISE + 1e-6], device=dev))


def sum_member(n, D, seed, extra=False):
    """the same data under Sum(Linear, Matern-5/2), the reference's NAR kernel"""
    g, Df, X, y = data(n, D, seed, extra)
    wl, wm = (0.6 + torch.rand(Df, generator=g)) / Df ** 0.5, 0.6 + torch.rand(Df, generator=g)
    descs = [{"kfun": LINEAR, "w": wl.to(dev), "amp": torch.tensor([0.6], device=dev), "clamp": float("-inf"), "kparam": 1.0, "center": None},
             {"kfun": M52, "w": wm.to(dev), "amp": torch.tensor([1.2], device=dev), "clamp": 1e-30, "kparam": 0.8, "center": None}]
    return F.Posterior(X, y, None, None, torch.tensor([NOISE + 1e-6], device=dev), tree=(descs, 0))


def make(ns, D, Q):
    tree = F.PosteriorChain([sum_member(n, D, 10 + f, extra=f > 0) for f, n in enumerate(ns)])
    radial = F.PosteriorChain([member(n, D, 10 + f, extra=f > 0) for f, n in enumerate(ns)])
    return tree, radial, (2.0 * torch.rand(Q, D, generator=torch.Generator().manual_seed(1))).to(dev)


def loop(predict, X0, steps, lr=0.1):
    X = X0.clone().requires_grad_(True)
    opt = torch.optim.Adam([X], lr=lr)
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


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "acq_chain_tree_bench.txt")
    lines = ["UCB (kappa = 2) on chains of frozen Sum(Linear, Matern-5/2) posteriors (NAR: member f > 0 on [x, mean below]), lr = 0.1; "
             "ms per call: median [min .. max] of %d alternating rounds; radial = ffgp_acq_optimize_chain on squared-exponential members "
             "of the same sizes" % ROUNDS]
    print(lines[0], flush=True)
    lost = []
    fmt = "%8.3f [%8.3f .. %8.3f]"
    mid = ROUNDS // 2
    for ns, D, Q, steps in CHAINS:
        tree, radial, X0 = make(ns, D, Q)
        va = [NOISE] * tree.F
        assert tree.acq_tree_fusable(X0) and not tree.acq_fusable(X0) and radial.acq_fusable(X0)
        for name, level in (("top level ", None), ("levels mix", (torch.arange(Q) % tree.F).to(torch.int32).to(dev))):
            kw = dict(steps=steps, lr=0.1, acq="ucb", kappa=KAPPA, var_adds=va, level=level)
            fused = lambda: tree.optimize_acquisition(X0, fuse_composed=True, **kw)
            rad = lambda: radial.optimize_acquisition(X0, **kw)
            assert fused()[3]["fused"] is True and rad()[3]["fused"] is True, "a call did not take the fused path"
            assert tree.optimize_acquisition(X0, **kw)[3]["fused"] is False, "the default is not the per-step loop"
            tf, tl, tr = rounds(fused, lambda: loop(lambda X: tree.predict_diff(X, level=level, var_adds=va), X0, steps), rad)
            lines.append(("%s n=%-15s D=%2d Q=%4d steps=%3d   fused " + fmt + "   per-step loop %8.2f [%8.2f .. %8.2f]   x%.1f   radial chain call " + fmt
                          + "   tree / radial %.2f")
                         % (name, ns, D, Q, steps, tf[mid], tf[0], tf[-1], tl[mid], tl[0], tl[-1], tl[mid] / tf[mid], tr[mid], tr[0], tr[-1],
                            tf[mid] / tr[mid]))
            print(lines[-1], flush=True)
            if not tf[-1] < tl[0]:
                lost.append((name.strip(), ns, D, Q, steps))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert not lost, "the fused call is not ahead of the per-step loop at %s" % lost


if __name__ == "__main__":
    main()
