"""The acquisition optimiser's Adam loop on a frozen posterior: the one-launch call (Posterior.optimize_acquisition -> ffgp_acq_optimize,
csrc/acq.hip) against the per-step loop it replaces (Posterior.predict_diff + torch.optim.Adam, Bayesian_optimization/acq.py:48-62).
Both in this process, alternating, median [min .. max] of three rounds each after a warm-up of either; every timing ends in a device
synchronise.  The tool asserts that the fused call's slowest round beats the loop's fastest at every size (the rule of
`tools/train_bench.py tree`).      python tools/acq_bench.py [out file, default profiles/acq_bench.txt]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from fidelityfusion_amd import functional as F

dev = torch.device("cuda", 0)
torch.set_default_dtype(torch.float64)
SIZES = ((32, 1, 500, 30), (128, 2, 500, 30), (256, 8, 500, 30), (256, 16, 64, 200))      # (n, D, Q, steps)


def make(n, D, Q, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = 2.0 * torch.rand(n, D, generator=g)
    y = (torch.sin(2.0 * X.sum(1)) + 0.1 * torch.randn(n, generator=g)).reshape(n, 1)
    w = 0.6 + torch.rand(D, generator=g)
    post = F.Posterior(X.to(dev), y.to(dev), w.to(dev), torch.tensor([1.3], device=dev), torch.tensor([0.05 + 1e-6], device=dev))
    return post, (2.0 * torch.rand(Q, D, generator=g)).to(dev)


def loop(post, X0, steps, lr=0.1, kappa=2.0, var_add=0.05):
    X = X0.clone().requires_grad_(True)
    opt = torch.optim.Adam([X], lr=lr)
    for _ in range(steps):
        opt.zero_grad()
        mean, var = post.predict_diff(X, full_cov=False, var_add_all=var_add)
        loss = -(mean + kappa * torch.sqrt(torch.clamp_min(var.reshape(-1, 1), 1e-12))).sum()
        loss.backward()
        opt.step()
    return X.detach()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "acq_bench.txt")
    lines = ["UCB (kappa = 2) on a frozen squared-exponential posterior, lr = 0.1; ms per call: median [min .. max] of 3 alternating rounds"]
    print(lines[0], flush=True)
    lost = []
    for n, D, Q, steps in SIZES:
        post, X0 = make(n, D, Q)
        fused = lambda k=steps: post.optimize_acquisition(X0, steps=k, lr=0.1, acq="ucb", var_add_all=0.05)
        assert fused(3)[3]["fused"] is True, "the call did not take the fused path"
        loop(post, X0, 3)
        tf, tl = [], []
        for _ in range(3):
            tf.append(timed(fused))
            tl.append(timed(lambda: loop(post, X0, steps)))
        tf.sort(), tl.sort()
        lines.append("n=%4d D=%2d Q=%4d steps=%4d   fused %8.3f [%8.3f .. %8.3f] (%.4f ms/step)   per-step loop %8.2f [%8.2f .. %8.2f] (%.3f ms/step)   x%.1f"
                     % (n, D, Q, steps, tf[1], tf[0], tf[2], tf[1] / steps, tl[1], tl[0], tl[2], tl[1] / steps, tl[1] / tf[1]))
        print(lines[-1], flush=True)
        if not tf[2] < tl[0]:
            lost.append((n, D, Q, steps))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert not lost, "the fused call is not ahead of the per-step loop at (n, D, Q, steps) = %s" % lost


if __name__ == "__main__":
    main()
