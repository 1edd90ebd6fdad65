"""The acquisition optimiser's Adam loop on a STACK of frozen posteriors (AR / ResGP): the one-launch call
(PosteriorStack.optimize_acquisition -> ffgp_acq_optimize_stack, csrc/acq_stack.hip) against the per-step loop it replaces (the members'
predict_diff + torch.optim.Adam).  Both in this process, alternating, median [min .. max] of three rounds each after a warm-up of
either; every timing ends in a device synchronise.  One row runs every level in ONE call (each point its own level) against one
call per level; and the single-posterior call (ffgp_acq_optimize, tools/acq_bench.py's sizes) is measured in the same run as the
per-member yardstick.  The tool asserts only that the fused call's slowest round beats the loop's fastest.
      python tools/acq_stack_bench.py [out file, default profiles/acq_stack_bench.txt]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from fidelityfusion_amd import functional as F

dev = torch.device("cuda", 0)
torch.set_default_dtype(torch.float64)
STACKS = (((32, 32, 32), 2, 500, 30), ((128, 128, 96), 2, 500, 30), ((256, 256), 8, 500, 30))      # (ns, D, Q, steps)
COEFS = (1.0, 0.8, 1.2)
KAPPA, NOISE = 2.0, 0.05


def member(n, D, seed):
    g = torch.Generator().manual_seed(seed)
    X = 2.0 * torch.rand(n, D, generator=g)
    y = (torch.sin(2.0 * X.sum(1)) + 0.1 * torch.randn(n, generator=g)).reshape(n, 1)
    w = 0.6 + torch.rand(D, generator=g)
    return F.Posterior(X.to(dev), y.to(dev), w.to(dev), torch.tensor([1.3], device=dev), torch.tensor([NOISE + 1e-6], device=dev))


def make(ns, D, Q):
    st = F.PosteriorStack([member(n, D, 10 + f) for f, n in enumerate(ns)], COEFS[:len(ns)])
    return st, (2.0 * torch.rand(Q, D, generator=torch.Generator().manual_seed(1))).to(dev)


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


def rounds(fused, slow):
    fused(), slow()      # warm-up of either
    tf, tl = [], []
    for _ in range(3):
        tf.append(timed(fused))
        tl.append(timed(slow))
    return sorted(tf), sorted(tl)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "acq_stack_bench.txt")
    lines = ["UCB (kappa = 2) on stacks of frozen squared-exponential posteriors, coefficients (1, 0.8, 1.2), lr = 0.1; "
             "ms per call: median [min .. max] of 3 alternating rounds"]
    print(lines[0], flush=True)
    lost, single, stack_ms = [], {}, {}
    # the single-posterior call on one member of each stack size: the per-member yardstick
    for n, D, Q, steps in ((32, 2, 500, 30), (128, 2, 500, 30), (256, 8, 500, 30)):
        post = member(n, D, 10)
        X0 = (2.0 * torch.rand(Q, D, generator=torch.Generator().manual_seed(1))).to(dev)
        fused = lambda: post.optimize_acquisition(X0, steps=steps, lr=0.1, acq="ucb", kappa=KAPPA, var_add_all=NOISE)
        assert fused()[3]["fused"] is True
        tf, tl = rounds(fused, lambda: loop(lambda X: post.predict_diff(X, full_cov=False, var_add_all=NOISE), X0, steps))
        single[(n, D)] = tf[1]
        lines.append("single  n=%4d           D=%2d Q=%4d steps=%3d   fused %8.3f [%8.3f .. %8.3f]   per-step loop %8.2f [%8.2f .. %8.2f]   x%.1f"
                     % (n, D, Q, steps, tf[1], tf[0], tf[2], tl[1], tl[0], tl[2], tl[1] / tf[1]))
        print(lines[-1], flush=True)
    for ns, D, Q, steps in STACKS:
        st, X0 = make(ns, D, Q)
        va = [NOISE] * st.F
        fused = lambda: st.optimize_acquisition(X0, steps=steps, lr=0.1, acq="ucb", kappa=KAPPA, var_adds=va)
        assert fused()[3]["fused"] is True, "the call did not take the fused path"
        tf, tl = rounds(fused, lambda: loop(lambda X: st.predict_diff(X, var_adds=va), X0, steps))
        stack_ms[ns] = tf[1]
        lines.append("stack   n=%-15s D=%2d Q=%4d steps=%3d   fused %8.3f [%8.3f .. %8.3f]   per-step loop %8.2f [%8.2f .. %8.2f]   x%.1f"
                     % (ns, D, Q, steps, tf[1], tf[0], tf[2], tl[1], tl[0], tl[2], tl[1] / tf[1]))
        print(lines[-1], flush=True)
        if not tf[2] < tl[0]:
            lost.append((ns, D, Q, steps))
    # every level in one call (the points dealt to the levels in turn) against one fused call per level on that level's points
    ns, D, Q, steps = STACKS[1]
    st, X0 = make(ns, D, Q)
    va = [NOISE] * st.F
    level = (torch.arange(Q) % st.F).to(torch.int32).to(dev)
    groups = [(k, X0[level == k].contiguous()) for k in range(st.F)]
    one = lambda: st.optimize_acquisition(X0, steps=steps, lr=0.1, acq="ucb", kappa=KAPPA, var_adds=va, level=level)
    per = lambda: [st.optimize_acquisition(Xk, steps=steps, lr=0.1, acq="ucb", kappa=KAPPA, var_adds=va, level=k) for k, Xk in groups]
    slow = lambda: [loop(lambda X, k=k: st.predict_diff(X, level=k, var_adds=va), Xk, steps) for k, Xk in groups]
    t1, tp = rounds(one, per)
    _, tl = rounds(one, slow)
    lines.append("levels  n=%-15s D=%2d Q=%4d steps=%3d   all levels in one call %8.3f [%8.3f .. %8.3f]   one fused call per level %8.3f [%8.3f .. %8.3f]"
                 "   per-step loop per level %8.2f [%8.2f .. %8.2f]" % (ns, D, Q, steps, t1[1], t1[0], t1[2], tp[1], tp[0], tp[2], tl[1], tl[0], tl[2]))
    print(lines[-1], flush=True)
    if not t1[2] < tl[0]:
        lost.append(("levels",) + (ns, D, Q, steps))
    # what a member costs in the stack against the single kernel on a posterior of that size
    for ns, D, Q, steps in STACKS:
        base = sum(single[(n, D)] for n in ns if (n, D) in single)
        known = [n for n in ns if (n, D) in single]
        if len(known) == len(ns):
            lines.append("per member: stack n=%s %.3f ms = %.2f x the sum of its members' single calls (%.3f ms)" % (ns, stack_ms[ns], stack_ms[ns] / base, base))
        else:
            lines.append("per member: stack n=%s %.3f ms = %.3f ms per member; the single call at n=%d: %.3f ms"
                         % (ns, stack_ms[ns], stack_ms[ns] / len(ns), known[0], single[(known[0], D)]))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert not lost, "the fused call is not ahead of the per-step loop at %s" % lost


if __name__ == "__main__":
    main()
