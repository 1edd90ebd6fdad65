"""The acquisition optimiser's Adam loop on a CHAIN of frozen posteriors (NAR): the one-launch call
(PosteriorChain.optimize_acquisition -> ffgp_acq_optimize_chain, csrc/acq_chain.hip) against the per-step loop it replaces
(PosteriorChain.predict_diff + torch.optim.Adam).  Both in this process, alternating, median [min .. max] of three rounds each after a
warm-up of either; every timing ends in a device synchronise.  The stack call (ffgp_acq_optimize_stack) on members of the same sizes
is measured in the same run for comparison: it runs the triangular chains of EVERY member per point, the chain call those of one.  One
row deals the points to the levels in turn (each point its own level, mixed inside every tile), and one runs the same points sorted by
level, so that tiles are level-homogeneous: the measurement behind the decision not to sort inside the library.  The tool asserts only
that the fused call's slowest round beats the loop's fastest.
      python tools/acq_chain_bench.py [out file, default profiles/acq_chain_bench.txt]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from fidelityfusion_amd import functional as F

dev = torch.device("cuda", 0)
torch.set_default_dtype(torch.float64)
CHAINS = (((32, 32, 32), 2, 500, 30), ((128, 128, 96), 2, 500, 30), ((256, 256), 8, 500, 30))      # (ns, D, Q, steps)
KAPPA, NOISE = 2.0, 0.05


def member(n, D, seed, extra=False):
    """a posterior on D inputs, or (extra) on D + 1: the last column stands for the mean of the member below"""
    g = torch.Generator().manual_seed(seed)
    Df = D + (1 if extra else 0)
    X = 2.0 * torch.rand(n, Df, generator=g)
    y = torch.sin(2.0 * X[:, :D].sum(1)) + 0.1 * torch.randn(n, generator=g)
    if extra:
        X[:, D] -= 1.0
        y = y + 0.5 * X[:, D]
    w = 0.6 + torch.rand(Df, generator=g)
    return F.Posterior(X.to(dev), y.reshape(n, 1).to(dev), w.to(dev), torch.tensor([1.3], device=dev), torch.tensor([NOISE + 1e-6], device=dev))


def make(ns, D, Q):
    ch = F.PosteriorChain([member(n, D, 10 + f, extra=f > 0) for f, n in enumerate(ns)])
    st = F.PosteriorStack([member(n, D, 10 + f) for f, n in enumerate(ns)], [1.0] * len(ns))
    return ch, st, (2.0 * torch.rand(Q, D, generator=torch.Generator().manual_seed(1))).to(dev)


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
    """sorted times of three alternating rounds of every function, after a warm-up of each"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(3):
        for t, fn in zip(ts, fns):
            t.append(timed(fn))
    return [sorted(t) for t in ts]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "acq_chain_bench.txt")
    lines = ["UCB (kappa = 2) on chains of frozen squared-exponential posteriors (NAR: member f > 0 on [x, mean below]), lr = 0.1; "
             "ms per call: median [min .. max] of 3 alternating rounds"]
    print(lines[0], flush=True)
    lost = []
    fmt = "%8.3f [%8.3f .. %8.3f]"
    for ns, D, Q, steps in CHAINS:
        ch, st, X0 = make(ns, D, Q)
        va = [NOISE] * ch.F
        fused = lambda: ch.optimize_acquisition(X0, steps=steps, lr=0.1, acq="ucb", kappa=KAPPA, var_adds=va)
        stack = lambda: st.optimize_acquisition(X0, steps=steps, lr=0.1, acq="ucb", kappa=KAPPA, var_adds=va)
        assert fused()[3]["fused"] is True and stack()[3]["fused"] is True, "a call did not take the fused path"
        tf, tl, ts = rounds(fused, lambda: loop(lambda X: ch.predict_diff(X, var_adds=va), X0, steps), stack)
        lines.append(("chain   n=%-15s D=%2d Q=%4d steps=%3d   fused " + fmt + "   per-step loop %8.2f [%8.2f .. %8.2f]   x%.1f   stack call, same sizes " + fmt)
                     % (ns, D, Q, steps, tf[1], tf[0], tf[2], tl[1], tl[0], tl[2], tl[1] / tf[1], ts[1], ts[0], ts[2]))
        print(lines[-1], flush=True)
        if not tf[2] < tl[0]:
            lost.append((ns, D, Q, steps))
    # every level in one call: the points dealt to the levels in turn, and the same points sorted by level (level-homogeneous tiles)
    ns, D, Q, steps = CHAINS[1]
    ch, st, X0 = make(ns, D, Q)
    va = [NOISE] * ch.F
    level = (torch.arange(Q) % ch.F).to(torch.int32).to(dev)
    order = torch.argsort(level, stable=True)
    Xs, ls = X0[order].contiguous(), level[order].contiguous()
    one = lambda: ch.optimize_acquisition(X0, steps=steps, lr=0.1, acq="ucb", kappa=KAPPA, var_adds=va, level=level)
    srt = lambda: ch.optimize_acquisition(Xs, steps=steps, lr=0.1, acq="ucb", kappa=KAPPA, var_adds=va, level=ls)
    stack = lambda: st.optimize_acquisition(X0, steps=steps, lr=0.1, acq="ucb", kappa=KAPPA, var_adds=va, level=level)
    a, b = one(), srt()
    assert torch.equal(a[0][order], b[0]) and torch.equal(a[1][:, order], b[1]), "sorting by level changed a trajectory"
    t1, tsrt, tl, ts = rounds(one, srt, lambda: loop(lambda X: ch.predict_diff(X, level=level, var_adds=va), X0, steps), stack)
    lines.append(("levels  n=%-15s D=%2d Q=%4d steps=%3d   levels in turn " + fmt + "   sorted by level " + fmt
                  + "   per-step loop %8.2f [%8.2f .. %8.2f]   stack call, levels in turn " + fmt)
                 % (ns, D, Q, steps, t1[1], t1[0], t1[2], tsrt[1], tsrt[0], tsrt[2], tl[1], tl[0], tl[2], ts[1], ts[0], ts[2]))
    print(lines[-1], flush=True)
    if not t1[2] < tl[0]:
        lost.append(("levels",) + (ns, D, Q, steps))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert not lost, "the fused call is not ahead of the per-step loop at %s" % lost


if __name__ == "__main__":
    main()
