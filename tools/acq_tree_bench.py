"""The acquisition optimiser's Adam loop on a frozen posterior with a COMPOSED kernel: the one-launch call
(Posterior.optimize_acquisition(..., fuse_composed=True) -> ffgp_acq_optimize_tree, csrc/acq_tree.hip) against the per-step loop it
replaces (Posterior.predict_diff + torch.optim.Adam, Bayesian_optimization/acq.py:48-62), in the method of tools/acq_bench.py: both in
this process, alternating, median [min .. max] of three rounds each after a warm-up of either; every timing ends in a device
synchronise.  A third column is the single-kernel call (ffgp_acq_optimize on a squared-exponential posterior) at the same sizes, so the
cost of the tree shows.  Cases: the reference's SumKernel(LinearKernel, MaternKernel) at three sizes, and the four-leaf tree
(SE x Linear) + (Matern32 x RQ) at the kernel's limits.  The tool asserts what its predecessors assert: the fused call's slowest round
beats the loop's fastest at every size.      python tools/acq_tree_bench.py [out file, default profiles/acq_tree_bench.txt] [commit label, default: git's HEAD]"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from fidelityfusion_amd import functional as F

dev = torch.device("cuda", 0)
torch.set_default_dtype(torch.float64)
SE, M32, M52, RQ, LINEAR = 0, 2, 3, 4, 5
SUM, PRODUCT, BALANCED = 0, 1, 1
NEG_INF = float("-inf")
CASES = (("sum(linear, matern52)", 32, 1, 500, 30), ("sum(linear, matern52)", 128, 2, 500, 30), ("sum(linear, matern52)", 256, 8, 500, 30),
         ("(se x linear) + (matern32 x rq)", 256, 16, 64, 200))      # (tree, n, D, Q, steps)


def leaf(g, D, kfun, amp, kparam=1.0):
    w = 0.6 + torch.rand(D, generator=g)
    if kfun == LINEAR:
        w = w / D ** 0.5
    return {"kfun": kfun, "w": w.to(dev), "amp": torch.tensor([amp], device=dev), "clamp": 1e-30 if kfun in (M32, M52) else NEG_INF,
            "kparam": kparam, "center": None}


def make(tree, n, D, Q, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = 2.0 * torch.rand(n, D, generator=g)
    y = (torch.sin(2.0 * X.sum(1)) + 0.1 * torch.randn(n, generator=g)).reshape(n, 1)
    w = 0.6 + torch.rand(D, generator=g)
    if tree.startswith("sum"):
        spec = ([leaf(g, D, LINEAR, 0.6), leaf(g, D, M52, 1.2, 0.8)], SUM)
    else:
        spec = ([leaf(g, D, SE, 1.1), leaf(g, D, LINEAR, 0.6), leaf(g, D, M32, 0.8, 1.3), leaf(g, D, RQ, 1.2, 1.7)], (BALANCED, (PRODUCT, PRODUCT, SUM)))
    dadd = torch.tensor([0.05 + 1e-6], device=dev)
    post = F.Posterior(X.to(dev), y.to(dev), None, None, dadd, tree=spec)
    single = F.Posterior(X.to(dev), y.to(dev), w.to(dev), torch.tensor([1.3], device=dev), dadd)
    return post, single, (2.0 * torch.rand(Q, D, generator=g)).to(dev)


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
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "acq_tree_bench.txt")
    try:
        commit = sys.argv[2] if len(sys.argv) > 2 else subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"
    lines = ["UCB (kappa = 2) on a frozen posterior with a composed kernel, lr = 0.1; ms per call: median [min .. max] of 3 alternating rounds "
             "after a warm-up of each; every timing ends in a device synchronise",
             "%s on parent commit %s + this change; `single` = ffgp_acq_optimize on a squared-exponential posterior of the same n, D, Q, steps"
             % (torch.cuda.get_device_name(0), commit)]
    print("\n".join(lines), flush=True)
    lost = []
    for tree, n, D, Q, steps in CASES:
        post, single, X0 = make(tree, n, D, Q)
        fused = lambda k=steps: post.optimize_acquisition(X0, steps=k, lr=0.1, acq="ucb", var_add_all=0.05, fuse_composed=True)
        plain = lambda k=steps: single.optimize_acquisition(X0, steps=k, lr=0.1, acq="ucb", var_add_all=0.05)
        assert fused(3)[3]["fused"] is True and plain(3)[3]["fused"] is True, "a call did not take the fused path"
        loop(post, X0, 3)
        tf, tl, ts = [], [], []
        for _ in range(3):
            tf.append(timed(fused))
            tl.append(timed(lambda: loop(post, X0, steps)))
            ts.append(timed(plain))
        tf.sort(), tl.sort(), ts.sort()
        lines.append("%-32s n=%4d D=%2d Q=%4d steps=%4d   fused tree %8.3f [%8.3f .. %8.3f] (%.4f ms/step)   per-step loop %8.2f [%8.2f .. %8.2f] "
                     "(%.3f ms/step)   x%.1f   single %8.3f [%8.3f .. %8.3f]   tree / single %.2f"
                     % (tree, n, D, Q, steps, tf[1], tf[0], tf[2], tf[1] / steps, tl[1], tl[0], tl[2], tl[1] / steps, tl[1] / tf[1],
                        ts[1], ts[0], ts[2], tf[1] / ts[1]))
        print(lines[-1], flush=True)
        if not tf[2] < tl[0]:
            lost.append((tree, n, D, Q, steps))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert not lost, "the fused call is not ahead of the per-step loop at (tree, n, D, Q, steps) = %s" % lost


if __name__ == "__main__":
    main()
