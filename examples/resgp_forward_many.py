"""A three-fidelity residual GP of our own making at the sizes of the reference's experiment sweeps (100 low- against a few dozen
high-fidelity points, Experiments/GAR_Aligned/exp_aligned.py:66-74), from training to prediction in two library calls: the three `cigp`s
train side by side in `cigp_v10.train_many` (every Adam iteration inside one launch), `cigp_v10.forward_many` predicts all three at the
test points in ONE launch, and the means and variances are summed as ResGP.forward sums them (FidelityFusion_Models/ResGP.py:48-63).
Printed against the reference's way: one `gpr(x_train, y_train, x_test)` per fidelity, the covariance's diagonal taken.

python examples/resgp_forward_many.py        (needs an MI355X: the fused calls have no CPU path)
"""
import copy
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fidelityfusion_amd import kernel
from fidelityfusion_amd.cigp_v10 import cigp, forward_many, train_many

torch.set_default_dtype(torch.float64)
dev = torch.device("cuda", 0)
gen = torch.Generator().manual_seed(11)


def truth(x, level):                              # three levels of one 2-D function: each adds finer structure to the one below
    base = torch.sin(3.0 * x[:, :1]) * torch.cos(2.0 * x[:, 1:2])
    mid = 0.4 * torch.sin(9.0 * x[:, :1] + 1.0)
    fine = 0.15 * torch.cos(17.0 * x[:, 1:2]) * x[:, :1]
    return base + (mid if level >= 1 else 0.0) + (fine if level >= 2 else 0.0)


sizes = (100, 60, 32)                             # ragged: fewer points at every higher fidelity
xs = [torch.rand(n, 2, generator=gen) for n in sizes]
# residual targets of a subset design: fidelity f learns what fidelity f - 1 leaves over (here: against the known lower level)
ys = [truth(xs[0], 0)] + [truth(xs[f], f) - truth(xs[f], f - 1) for f in (1, 2)]
ys = [y + 0.02 * torch.randn(y.shape, generator=gen) for y in ys]
xs, ys = [x.to(dev) for x in xs], [y.to(dev) for y in ys]
x_test = torch.rand(100, 2, generator=gen).to(dev)
models = [cigp(kernel.ARDKernel(2), 1.0).to(dev) for _ in sizes]

train_many([copy.deepcopy(m) for m in models], xs, ys, 3, lr=1e-2)      # (warm-up: workspaces, streams)
train_many(models, xs, ys, 200, lr=1e-2)


def predict_many():
    state = {}
    parts = forward_many(models, xs, ys, [x_test] * len(models), state)
    return sum(p[0] for p in parts), sum(p[1] for p in parts), state["fused"]


def predict_loop():                               # the reference's loop, fidelity after fidelity, each on a fresh factor
    mean = var = 0.0
    with torch.no_grad():
        for m, x, y in zip(models, xs, ys):
            m.clear_posterior_cache()
            mu, cov = m(x, y, x_test)
            mean, var = mean + mu, var + cov.diagonal().reshape(-1, 1)
    return mean, var


def timed(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) / 20 * 1e3


(mean, var, fused), t_many = timed(predict_many)
(mean_l, var_l), t_loop = timed(predict_loop)
y_true = truth(x_test.cpu(), 2)
print("3 fidelities (%s points) trained 200 steps by train_many, predicted at %d points" % (" / ".join(map(str, sizes)), x_test.shape[0]))
print("  forward_many (members fused: %s)  %7.3f ms per call" % (fused, t_many))
print("  per-model loop                        %7.3f ms per call" % t_loop)
print("  largest relative difference: mean %.1e, variance %.1e"
      % (float((mean - mean_l).abs().max() / mean_l.abs().max()), float((var - var_l).abs().max() / var_l.abs().max())))
print("  rmse against the top fidelity's truth %.4f, mean predictive sd %.4f" % (float((mean.cpu() - y_true).pow(2).mean().sqrt()), float(var.sqrt().mean())))
