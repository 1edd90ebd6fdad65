"""The acquisition optimiser's Adam loop on a STACK of frozen posteriors with COMPOSED kernels (AR / ResGP on
SumKernel(LinearKernel, MaternKernel) per fidelity): the one-launch call (PosteriorStack.optimize_acquisition(..., fuse_composed=True)
-> ffgp_acq_optimize_stack_tree, csrc/acq_stack_tree.hip) against the per-step loop it replaces (the same call without the keyword: the
members' predict_diff + torch.optim.Adam).  Both in this process, alternating, median [min .. max] of five rounds each after a warm-up
of either; a round times several back-to-back calls between two device synchronises and reports ms per call.  Beside each composed
stack stands the radial stack call (ffgp_acq_optimize_stack on squared-exponential members of the same sizes) for orientation.  One
row runs a mixed radial / four-leaf stack at D = 16, one runs every level in ONE call against the per-step loop per level.  Each row
also prints the distance between the two paths' final points (the largest absolute difference over the largest coordinate).
The tool asserts only that the fused call's slowest round beats the loop's fastest at every size.
      python tools/acq_stack_tree_bench.py [out file, default profiles/acq_stack_tree_bench.txt]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from fidelityfusion_amd import functional as F

dev = torch.device("cuda", 0)
torch.set_default_dtype(torch.float64)
SE, M12, M32, M52, RQ, LINEAR = 0, 1, 2, 3, 4, 5
SUM, PRODUCT, CHAIN = 0, 1, 0
STACKS = (((32, 32, 32), 2), ((128, 128, 96), 2), ((256, 256), 8))      # (ns, D)
Q, STEPS, ROUNDS = 500, 30, 5
COEFS = (1.0, 0.8, 1.2)
KAPPA, NOISE = 2.0, 0.05
FUSED_CALLS, LOOP_CALLS = 40, 3      # per round: a timed window of roughly 0.1 s or more for either path


def leaf(g, D, kfun, amp, kparam=1.0, center=None):
    w = 0.6 + torch.rand(D, generator=g)
    if kfun == LINEAR:
        w = w / D ** 0.5      # the linear part stays O(1) over the box at every D
    return {"kfun": kfun, "w": w.to(dev), "amp": torch.tensor([amp], device=dev), "clamp": 1e-30 if kfun in (M12, M32, M52) else float("-inf"),
            "kparam": kparam, "center": None if center is None else torch.full((D,), center).to(dev)}


def data(n, D, seed):
    g = torch.Generator().manual_seed(seed)
    X = 2.0 * torch.rand(n, D, generator=g)
    y = (torch.sin(2.0 * X.sum(1)) + 0.1 * torch.randn(n, generator=g)).reshape(n, 1)
    return g, X.to(dev), y.to(dev)


def member(n, D, seed, kind):
    g, X, y = data(n, D, seed)
    dadd = torch.tensor([NOISE + 1e-6], device=dev)
    if kind == "radial":
        return F.Posterior(X, y, (0.6 + torch.rand(D, generator=g)).to(dev), torch.tensor([1.3], device=dev), dadd)
    if kind == "sum":       # the reference's SumKernel(LinearKernel, MaternKernel)
        return F.Posterior(X, y, None, None, dadd, tree=([leaf(g, D, LINEAR, 0.6), leaf(g, D, M52, 1.2, 0.8)], SUM))
    # four leaves: ((Linear + SE) x Matern52) + Matern12
    leaves = [leaf(g, D, LINEAR, 0.5, center=0.2), leaf(g, D, SE, 1.0), leaf(g, D, M52, 0.9, 0.8), leaf(g, D, M12, 0.4, 1.3)]
    return F.Posterior(X, y, None, None, dadd, tree=(leaves, (CHAIN, (SUM, PRODUCT, SUM))))


def make(ns, D, kinds):
    st = F.PosteriorStack([member(n, D, 10 + f, kinds[f]) for f, n in enumerate(ns)], COEFS[:len(ns)])
    return st, (2.0 * torch.rand(Q, D, generator=torch.Generator().manual_seed(1))).to(dev)


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def rounds(fused, slow):
    fused(), slow()      # warm-up of either
    tf, tl = [], []
    for _ in range(ROUNDS):
        tf.append(timed(fused, FUSED_CALLS))
        tl.append(timed(slow, LOOP_CALLS))
    return sorted(tf), sorted(tl)


def fmt(t):
    return "%8.3f [%8.3f .. %8.3f]" % (t[ROUNDS // 2], t[0], t[-1])


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "acq_stack_tree_bench.txt")
    lines = ["UCB (kappa = 2) on stacks of frozen posteriors, coefficients (1, 0.8, 1.2), Q = %d, %d steps, lr = 0.1; ms per call: median "
             "[min .. max] of %d alternating rounds (%d fused calls / %d per-step loops per round)" % (Q, STEPS, ROUNDS, FUSED_CALLS, LOOP_CALLS)]
    print(lines[0], flush=True)
    lost = []

    def row(tag, ns, D, kinds, level=None):
        st, X0 = make(ns, D, kinds)
        va = [NOISE] * st.F
        call = lambda fc: st.optimize_acquisition(X0, steps=STEPS, lr=0.1, acq="ucb", kappa=KAPPA, var_adds=va, level=level, fuse_composed=fc)
        a, b = call(True), call(False)
        composed = any(m.tree is not None for m in st.members)
        assert a[3]["fused"] is True and b[3]["fused"] is (not composed), "the calls did not take the paths they are timed as"
        if not composed:      # the radial stack call, for orientation: fused whatever the keyword says
            t = sorted(timed(lambda: call(False), FUSED_CALLS) for _ in range(ROUNDS))
            lines.append("%-7s n=%-15s D=%2d   radial stack call %s" % (tag, ns, D, fmt(t)))
            print(lines[-1], flush=True)
            return
        dist = float((a[0] - b[0]).abs().max() / b[0].abs().max())
        tf, tl = rounds(lambda: call(True), lambda: call(False))
        lines.append("%-7s n=%-15s D=%2d   fused %s   per-step loop %s   x%.1f   final points differ by %.1e"
                     % (tag, ns, D, fmt(tf), fmt(tl), tl[ROUNDS // 2] / tf[ROUNDS // 2], dist))
        print(lines[-1], flush=True)
        if not tf[-1] < tl[0]:
            lost.append((tag, ns, D))

    for ns, D in STACKS:
        row("sum", ns, D, ("sum",) * len(ns))
        row("radial", ns, D, ("radial",) * len(ns))
    ns, D = (128, 128, 96), 16
    row("mixed", ns, D, ("radial", "four", "radial"))
    row("radial", ns, D, ("radial",) * 3)
    ns, D = STACKS[1]
    row("levels", ns, D, ("sum",) * 3, level=(torch.arange(Q) % 3).to(torch.int32).to(dev))      # every level in ONE call, either path
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert not lost, "the fused call is not ahead of the per-step loop at %s" % lost


if __name__ == "__main__":
    main()
