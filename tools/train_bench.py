"""K Adam steps per call (cigp_v10.train_many -> ffgp_train_raw) against the per-step loop through the drop-in modules
(gate: 200 steps at N = 128 in <= 20 ms).  python tools/train_bench.py [steps]

python tools/train_bench.py tree [steps]: the same for the reference's demo kernel SumKernel(LinearKernel, MaternKernel) -- train_many
(ffgp_train_tree_raw) against the per-step loop these models ran on before, both in this process, alternating, three rounds each
after a warm-up of either; and, for information, the single-kernel Matern model of the same size through the launch-per-stage trainer
(option train_persist = 0): what the tree pass costs per step.  At N <= train.TREE_ONE_LAUNCH_MAX_N a further column: the same models
through train_many(..., tree_one_launch=True) (ffgp_train_tree_lds_raw: one launch for all the steps), which has to beat the
launch-per-stage call by more than the spread of either over the run's three rounds."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench import synthetic_xy
from fidelityfusion_amd import kernel
from fidelityfusion_amd.cigp_v10 import cigp, train_many

mode = "tree" if len(sys.argv) > 1 and sys.argv[1] == "tree" else "plain"
args = sys.argv[2:] if mode == "tree" else sys.argv[1:]
steps = int(args[0]) if args else 200
for kv in os.environ.get("FFGP_OPTS", "").split(","):      # library options for A/B runs: FFGP_OPTS=small_finish=1
    if kv:
        from fidelityfusion_amd import _lib
        _lib.set_option(kv.split("=")[0], float(kv.split("=")[1]), 0)
        print("option", kv)
dev = torch.device("cuda", 0)
torch.set_default_dtype(torch.float64)


def make(n, D, d, F=1, kind="ard"):
    ms, xs, ys = [], [], []
    for f in range(F):
        X, Y = synthetic_xy(n, D, d, seed=f)
        k = {"ard": lambda: kernel.ARDKernel(D), "matern": lambda: kernel.MaternKernel(D),
             "tree": lambda: kernel.SumKernel(kernel.LinearKernel(D), kernel.MaternKernel(D))}[kind]()
        ms.append(cigp(k, 1.0).to(dev))
        xs.append(torch.tensor(X, device=dev))
        ys.append(torch.tensor(Y, device=dev))
    return ms, xs, ys


def loop(ms, xs, ys, k):
    for m, x, y in zip(ms, xs, ys):
        opt = torch.optim.Adam(m.parameters(), lr=1e-2)
        for _ in range(k):
            opt.zero_grad()
            loss = -m.negative_log_likelihood(x, y)
            loss.backward()
            opt.step()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def tree_mode():
    from fidelityfusion_amd import _lib, train
    print("SumKernel(LinearKernel(2), MaternKernel(2, nu = 2.5)), d = 1, %d Adam steps; ms per call: median [min .. max] of 3 alternating rounds" % steps)
    for n, F in ((16, 1), (32, 1), (64, 1), (128, 1), (300, 1), (1024, 1), (64, 16)):
        fused, looped, lds = make(n, 2, 1, F, "tree"), make(n, 2, 1, F, "tree"), make(n, 2, 1, F, "tree")
        one = n <= train.TREE_ONE_LAUNCH_MAX_N
        _, st = train_many(*fused, 5)
        assert st["fused"] is True, "the tree model was not trained by the library call"
        loop(*looped, 5)
        if one:
            _, st = train_many(*lds, 5, tree_one_launch=True)
            assert st["tree_one_launch"] == list(range(F)), "the tree models did not take the one-launch route"
        t_many, t_loop, t_lds = [], [], []
        for _ in range(3):
            t_many.append(timed(lambda: train_many(*fused, steps)))
            if one:
                t_lds.append(timed(lambda: train_many(*lds, steps, tree_one_launch=True)))
            t_loop.append(timed(lambda: loop(*looped, steps)))
        _lib.set_option("train_persist", 0, 0)
        try:
            single = make(n, 2, 1, F, "matern")
            train_many(*single, 5)
            t_single = sorted(timed(lambda: train_many(*single, steps)) for _ in range(3))
        finally:
            _lib.set_option("train_persist", 1, 0)
        t_many.sort(), t_loop.sort(), t_lds.sort()
        print("N=%5d F=%2d  train_many %8.2f [%8.2f .. %8.2f] (%.3f ms/step/model)   per-step loop %8.2f [%8.2f .. %8.2f] (%.3f)   x%.1f"
              "   | single Matern, launch per stage: %8.2f (%.3f ms/step/model)"
              % (n, F, t_many[1], t_many[0], t_many[2], t_many[1] / steps / F, t_loop[1], t_loop[0], t_loop[2], t_loop[1] / steps / F,
                 t_loop[1] / t_many[1], t_single[1], t_single[1] / steps / F), flush=True)
        assert t_many[2] < t_loop[0], "train_many is not ahead of the per-step loop at N = %d, F = %d" % (n, F)
        if one:
            spread = max(t_many[2] - t_many[0], t_lds[2] - t_lds[0])
            print("              one launch %8.2f [%8.2f .. %8.2f] (%.4f ms/step/model)   x%.1f against launch per stage (spread %.2f)"
                  % (t_lds[1], t_lds[0], t_lds[2], t_lds[1] / steps / F, t_many[1] / t_lds[1], spread), flush=True)
            assert t_many[1] - t_lds[1] > spread, "the one-launch route is not ahead of launch per stage at N = %d, F = %d" % (n, F)


if mode == "tree":
    tree_mode()
    sys.exit(0)

for n, D, d, F in ((32, 5, 1, 1), (128, 5, 1, 1), (256, 5, 1, 1), (512, 5, 1, 1), (1024, 8, 1, 1), (128, 5, 1, 8), (64, 5, 1, 16), (300, 5, 1, 3), (512, 5, 1, 4), (1024, 8, 1, 4)):
    ms, xs, ys = make(n, D, d, F)
    train_many(ms, xs, ys, 5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    train_many(ms, xs, ys, steps)
    torch.cuda.synchronize()
    t_many = time.perf_counter() - t0
    ms2, _, _ = make(n, D, d, F)
    k_loop = max(10, steps // 4)
    loop(ms2, xs, ys, 3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop(ms2, xs, ys, k_loop)
    torch.cuda.synchronize()
    t_loop = (time.perf_counter() - t0) * steps / k_loop
    print("N=%5d D=%d d=%d F=%2d  %d steps: train_many %8.2f ms (%.3f ms/step/model)   per-step loop %8.2f ms (%.3f)   x%.1f"
          % (n, D, d, F, steps, t_many * 1e3, t_many * 1e3 / steps / F, t_loop * 1e3, t_loop * 1e3 / steps / F, t_loop / t_many), flush=True)
