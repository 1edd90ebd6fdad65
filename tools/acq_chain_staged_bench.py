"""The acquisition optimiser's Adam loop on a NAR chain past 256 training points: the staged call
(`PosteriorChain.optimize_acquisition(..., staged=True)` -> ffgp_acq_optimize_chain_staged, csrc/acq_staged_chain.hip: launch per
stage, every step enqueued by one library call) against the per-step loop such a chain runs without the keyword
(`PosteriorChain.predict_diff` + torch.optim.Adam; MF_BayesianOptimization/Discrete/DMF_acq.py:226-262 on FidelityFusion_Models/NAR.py).
tools/acq_staged_bench.py's method: both in this process, alternating, median [min .. max] of three rounds each after a warm-up of
either; every timing ends in a device synchronise.  Every chain is timed twice: all points at the top level (the drivers' call, one
level at a time: 3 F + 4 launches per step) and the levels mixed inside every tile ((7 q + 2) mod F: every member's triangular products
run, 5 F + 2 launches per step).  The last case -- (256, 256) forced onto the staged call beside the one-launch chain call that serves
it -- is informative.  The matching rows of profiles/acq_staged_bench.txt (the stack of the same sizes) are quoted beside the chain's.
Nothing is asserted on the ratios: the two expectations are written out as met or NOT met.
    python tools/acq_chain_staged_bench.py [out file, default profiles/acq_chain_staged_bench.txt]"""
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
CHAINS = (((300, 300, 250), 2), ((1024, 1024), 8), ((2048,), 8))      # (ns, D): NAR's demo sizes; the staged stack bench's larger sizes
INFORMATIVE = ((256, 256), 8)
STACK_ROWS = ("stack n=(300, 300, 250)", "n=1024", "n=2048", "n= 256")    # of profiles/acq_staged_bench.txt


def make_chain(ns, D, seed=0):
    """tests/test_gpu_acq_chain.py's member recipe on squared-exponential kernels: above member 0 one more input in [-1, 1)"""
    members = []
    for f, n in enumerate(ns):
        g = torch.Generator().manual_seed(seed + f)
        Df = D + (1 if f else 0)
        X = 2.0 * torch.rand(n, Df, generator=g)
        y = torch.sin(2.0 * X[:, :D].sum(1)) + 0.1 * torch.randn(n, generator=g)
        if f:
            X[:, D] -= 1.0
            y = y + 0.5 * X[:, D]
        w = 0.6 + torch.rand(Df, generator=g)
        members.append(F.Posterior(X.to(dev), y.reshape(n, 1).to(dev), w.to(dev), torch.tensor([1.3], device=dev),
                                   torch.tensor([NOISE + 1e-6], device=dev)))
    return F.PosteriorChain(members)


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
    return ("%-42s staged %8.3f [%8.3f .. %8.3f] (%.4f ms/step)   %s %8.3f [%8.3f .. %8.3f] (%.4f ms/step)   x%.2f"
            % (what, ta[1], ta[0], ta[2], ta[1] / STEPS, name_b, tb[1], tb[0], tb[2], tb[1] / STEPS, tb[1] / ta[1]))


def case(chain, D, level, staged_kw, other):
    """(staged times, the other route's times); `other`: "loop" or "one" (the one-launch call)"""
    X0, va = starts(D), [NOISE] * chain.F
    kw = dict(lr=LR, acq="ucb", kappa=KAPPA, var_adds=va, level=level)
    staged = lambda k=STEPS: chain.optimize_acquisition(X0, steps=k, staged=staged_kw, **kw)
    st = staged(3)[3]
    assert st["fused"] is False and st.get("staged") is True, "the call did not take the staged path"
    if other == "one":
        b = lambda k=STEPS: chain.optimize_acquisition(X0, steps=k, **kw)
        assert b(3)[3]["fused"] is True
    else:
        b = lambda k=STEPS: loop(lambda X: chain.predict_diff(X, level=level, var_adds=va), X0, k)
        assert chain.optimize_acquisition(X0, steps=3, **kw)[3]["fused"] is False      # what the chain takes without the keyword
        b(3)
    return rounds(staged, b)


def levels(chain):
    """(label, level) pairs: the top level for all points; levels mixed inside every tile when there is more than one member"""
    out = [("top level", None)]
    if chain.F > 1:
        out.append(("levels mixed", ((torch.arange(Q) * 7 + 2) % chain.F).to(dev)))
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "acq_chain_staged_bench.txt")
    lines = ["UCB (kappa = 2) on NAR chains of frozen squared-exponential posteriors, Q = %d, %d steps, lr = %g; ms per call: median [min .. max] "
             "of 3 alternating rounds" % (Q, STEPS, LR)]
    print(lines[0], flush=True)
    results = {}
    for ns, D in CHAINS:
        chain = make_chain(ns, D)
        for label, lv in levels(chain):
            ta, tb = case(chain, D, lv, True, "loop")
            results[(ns, label)] = (ta, tb)
            lines.append(row("chain n=%s D=%d, %s" % (ns, D, label), "per-step loop", ta, tb))
            print(lines[-1], flush=True)
    ns, D = INFORMATIVE
    chain = make_chain(ns, D)
    for label, lv in levels(chain):
        ta, tb = case(chain, D, lv, "force", "one")
        results[(ns, label)] = (ta, tb)
        lines.append(row("chain n=%s D=%d forced, %s" % (ns, D, label), "one-launch call", ta, tb))
        print(lines[-1], flush=True)
    # the two expectations, stated and not asserted: no route depends on them
    ahead = all(results[(CHAINS[0][0], label)][0][2] < results[(CHAINS[0][0], label)][1][0] for label in ("top level", "levels mixed"))
    behind = all(results[(ns, label)][1][2] < results[(ns, label)][0][0] for label in ("top level", "levels mixed"))
    lines.append("expectation: at %s the staged call's slowest round beats the per-step loop's fastest: %s" % (CHAINS[0][0], "met" if ahead else "NOT met"))
    lines.append("expectation: at %s the one-launch call's slowest round beats the forced staged call's fastest: %s" % (ns, "met" if behind else "NOT met"))
    ref = os.path.join(ROOT, "profiles", "acq_staged_bench.txt")
    if os.path.exists(ref):
        lines.append("for comparison, the stack's staged call at the same sizes (profiles/acq_staged_bench.txt, an earlier run):")
        lines += ["    " + l.rstrip() for l in open(ref) if l.startswith(STACK_ROWS)]
    print("\n".join(lines[-7:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
