"""The reference's own `cigp` demo recipes (GaussianProcess/cigp_v10.py:74-125: noisy points of sin(x) + 10 at D = 1 and of
sin(x1 + x2) + 10 at D = 2, SumKernel(LinearKernel, MaternKernel), log_beta = 1, Adam with lr = 0.1) as a sweep of eight seeds each:
all sixteen models trained by ONE launch (`train_many(..., tree_one_launch=True)`), then predicted in two ways on the MI355X -- the
per-model loop `m.forward(x, y, x_test)`, which is what `forward_many` runs for a composed kernel, and `forward_many_composed`, ONE
launch for all sixteen (ffgp_predict_small_tree_batch).  Same means, same variances.
(The D = 2 recipe uses LinearKernel(2) / MaternKernel(2): the one-launch calls take a linear leaf's centre with D entries; the
reference's LinearKernel(1) at D = 2 broadcasts a one-entry centre and runs the per-model paths.)

python examples/sum_kernel_forward_many.py        (needs an MI355X: the fused calls have no CPU path)
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fidelityfusion_amd import kernel
from fidelityfusion_amd.cigp_v10 import cigp, forward_many_composed, train_many

torch.set_default_dtype(torch.float64)
dev = torch.device("cuda", 0)
gen = torch.Generator().manual_seed(16)

models, xs, ys, xts = [], [], [], []
for seed in range(8):      # recipe 1: 16 points, D = 1, tested on a grid of 100
    xtr = torch.rand(16, 1, generator=gen) * 6
    ys.append((torch.sin(xtr) + torch.randn(16, 1, generator=gen) * 0.5 + 10).to(dev))
    xs.append(xtr.to(dev))
    xts.append(torch.linspace(0, 6, 100).view(-1, 1).to(dev))
    models.append(cigp(kernel.SumKernel(kernel.LinearKernel(1), kernel.MaternKernel(1)), log_beta=1.0).to(dev))
for seed in range(8):      # recipe 2: 32 points, D = 2, tested at 128 random points
    xtr = torch.rand(32, 2, generator=gen) * 2
    ys.append((torch.sin(xtr.sum(1)).view(-1, 1) + torch.randn(32, 1, generator=gen) * 0.5 + 10).to(dev))
    xs.append(xtr.to(dev))
    xts.append((torch.rand(128, 2, generator=gen) * 2).to(dev))
    models.append(cigp(kernel.SumKernel(kernel.LinearKernel(2), kernel.MaternKernel(2)), log_beta=1.0).to(dev))

trace, state = train_many(models, xs, ys, 100, lr=1e-1, tree_one_launch=True)
assert state["tree_one_launch"] == list(range(16)), "a model did not take the one-launch trainer"
print("trained sixteen models, 100 steps in one launch: loss %.4f -> %.4f (model 0), %.4f -> %.4f (model 8)"
      % (trace[0, 0].item(), trace[0, -1].item(), trace[8, 0].item(), trace[8, -1].item()))
for m in models:
    m.cache_posterior = False      # a sweep predicts every model once: the loop factors on every call, as the reference does


def loop():
    with torch.no_grad():
        return [(mean, cov.diagonal().reshape(-1, 1)) for mean, cov in (m(x, y, xt) for m, x, y, xt in zip(models, xs, ys, xts))]


def clock(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) / reps * 1e3


st = {}
forward_many_composed(models, xs, ys, xts, st)
assert st["fused_composed"] == list(range(16)) and st["status"] == [0] * 16, st
per_model, t_loop = clock(loop)
fused, t_fused = clock(lambda: forward_many_composed(models, xs, ys, xts))
worst_mean = max(((a[0] - b[0]).abs().max() / b[0].abs().max()).item() for a, b in zip(fused, per_model))
worst_var = max(((a[1] - b[1]).abs().max() / b[1].abs().max()).item() for a, b in zip(fused, per_model))
print("largest relative difference from the per-model path: mean %.2e, variance %.2e" % (worst_mean, worst_var))
print("sixteen posteriors: per-model loop %.3f ms, forward_many_composed %.3f ms" % (t_loop, t_fused))
mean, var = fused[0]
print("model 0 at x = 0, 3, 6: mean %s, std %s" % (mean[[0, 50, 99], 0].cpu().numpy().round(4), var[[0, 50, 99], 0].sqrt().cpu().numpy().round(4)))
