"""train_CIGAR's fidelities above 0 through train_many (residual=[(tensor_linear, y_low, y_high)] -> ffgp_train_tlin_raw) against the
per-step loop through the drop-in modules -- the only route such a model had before -- both in this process, alternating, three rounds
each after a warm-up of either; every figure is the median, the spread (max - min of the three) beside it.
python tools/train_tlin_bench.py [steps] > profiles/train_tlin_bench.txt

  one launch         (n, l = h) = (4, 1), (32, 1), (100, 12), (128, 16): the persistent-workgroup class of csrc/train.hip, beside the
                     launch-per-stage form of the same call (option train_persist = 0) and the loop
  launch per stage   (128, 64), (300, 64), (1024, 256), (8192, 1024): the default route, the plain fixed-order kernels alone (option
                     tlin_gemm_min = 0), the fp64 GEMM alone (tlin_gemm_min = 1) and the loop; fewer steps at the two large shapes (stated)
  the GEMM switch    ms per step of the two product routes at shapes around the switch: what the default of tlin_gemm_min was chosen from
  sixteen members    sixteen (32, 1) members in one call: Experiments/GAR_Aligned/exp_aligned.py's sweep"""
import copy
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from fidelityfusion_amd import _lib, kernel
from fidelityfusion_amd.cigp_v10 import cigp, train_many
from fidelityfusion_amd.gp_computation_pack import Tensor_linear

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
dev = torch.device("cuda", 0)
torch.set_default_dtype(torch.float64)
GEMM_MIN_DEFAULT = 8192      # (csrc/handle.hip)


def make(n, l, h, seed, D=2):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (n, D))
    yl = np.sin(3 * x[:, :1] + 0.01 * np.arange(l)) + 0.1 * rng.standard_normal((n, l)) + 0.3
    W = rng.uniform(0.5, 1.5, (h, l)) / l
    yh = 1.3 * yl @ W.T + 0.2 * np.cos(2 * x[:, :1] + 0.01 * np.arange(h)) + 0.05 * rng.standard_normal((n, h))
    m = cigp(kernel.ARDKernel(D), 0.6).double().to(dev)
    tl = Tensor_linear((l,), (h,)).double().to(dev)
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)
    return m, t(x), (tl, t(yl), t(yh))


def loop(items, k):
    for m, x, (tl, yl, yh) in items:
        opt = torch.optim.Adam(list(m.parameters()) + list(tl.parameters()), lr=1e-2)
        for _ in range(k):
            opt.zero_grad()
            loss = -m.negative_log_likelihood(x, yh - tl(yl))
            loss.backward()
            opt.step()


def fused(items, k):
    train_many([i[0] for i in items], [i[1] for i in items], [None] * len(items), k, lr=1e-2, residual=[i[2] for i in items])


def timed(fn, items, k):
    items = copy.deepcopy(items)      # (every timing starts from the same parameters)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(items, k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def with_opts(opts, fn):
    def run(items, k):
        for key, v in opts.items():
            _lib.set_option(key, v, 0)
        try:
            fn(items, k)
        finally:
            _lib.set_option("train_persist", 1, 0)
            _lib.set_option("tlin_gemm_min", GEMM_MIN_DEFAULT, 0)
    return run


def legs(items, k, routes, rounds=3):
    """{name: (median ms, spread ms)} of the routes, alternating, after a warm-up of each"""
    for fn in routes.values():
        timed(fn, items, min(k, 3))
    ts = {name: [] for name in routes}
    for _ in range(rounds):
        for name, fn in routes.items():
            ts[name].append(timed(fn, items, k))
    return {name: (statistics.median(v), max(v) - min(v)) for name, v in ts.items()}


def row(label, res, k):
    cells = "  ".join("%s %9.3f (+-%7.3f)" % (name, med, spread) for name, (med, spread) in res.items())
    print("%-34s steps %4d  %s" % (label, k, cells))


print("train_CIGAR's residual fidelities through train_many against the per-step loop: ms per call of `steps` Adam steps, lr 1e-2, "
      "median of 3 alternating rounds (spread = max - min), ARD kernel, D = 2, subset form (%s)" % torch.cuda.get_device_name(0))
print()
print("one launch (csrc/train.hip, the tensor-linear class) | the same call launch per stage (train_persist = 0) | the per-step loop")
for n, c in ((4, 1), (32, 1), (100, 12), (128, 16)):
    items = [make(n, c, c, 10 * n + c)]
    row("n = %d, l = h = %d" % (n, c), legs(items, steps, {"one_launch": fused, "per_stage": with_opts({"train_persist": 0}, fused),
                                                            "loop": loop}), steps)
items = [make(32, 1, 1, 500 + f) for f in range(16)]
row("sixteen members n = 32, l = h = 1", legs(items, steps, {"one_launch": fused, "per_stage": with_opts({"train_persist": 0}, fused),
                                                              "loop": loop}), steps)
print()
print("launch per stage (csrc/train_loop.hip): default switch | plain kernels (tlin_gemm_min = 0) | fp64 GEMM (tlin_gemm_min = 1) | the per-step loop")
for n, c, k in ((128, 64, steps), (300, 64, steps), (1024, 256, max(steps // 5, 1)), (8192, 1024, max(steps // 20, 1))):
    try:
        items = [make(n, c, c, 10 * n + c)]
        row("n = %d, l = h = %d" % (n, c), legs(items, k, {"default": fused, "plain": with_opts({"tlin_gemm_min": 0}, fused),
                                                            "gemm": with_opts({"tlin_gemm_min": 1}, fused), "loop": loop},
                                                 rounds=3 if n < 8192 else 2), k)
    except torch.cuda.OutOfMemoryError:
        print("n = %d, l = h = %d: out of memory, not measured" % (n, c))
print()
print("the GEMM switch: ms per step launch per stage (train_persist = 0 throughout, so that the small shapes take this route too), "
      "plain kernels | fp64 GEMM, by n l h (the default of tlin_gemm_min = %d)" % GEMM_MIN_DEFAULT)
for n, l, h in ((4, 1, 1), (32, 1, 1), (32, 8, 8), (100, 12, 12), (128, 16, 16), (128, 16, 17), (129, 17, 17), (129, 32, 32), (200, 40, 40),
                (300, 40, 64), (300, 64, 64), (512, 64, 64), (1024, 64, 64), (2048, 32, 32)):
    items = [make(n, l, h, n + l + h)]
    res = legs(items, 50, {"plain": with_opts({"tlin_gemm_min": 0, "train_persist": 0}, fused),
                           "gemm": with_opts({"tlin_gemm_min": 1, "train_persist": 0}, fused)})
    print("n = %5d l = %3d h = %3d  n l h = %9d  plain %8.4f (+-%7.4f)  gemm %8.4f (+-%7.4f)"
          % (n, l, h, n * l * h, res["plain"][0] / 50, res["plain"][1] / 50, res["gemm"][0] / 50, res["gemm"][1] / 50))
