"""The acquisition optimiser past 256 training points on the reference's own models, both ways: UCB from 500 start points on a frozen
`cigp` on SumKernel(LinearKernel, MaternKernel) of n = 300 -- the reference's Bayesian-optimisation model
(Bayesian_optimization/cigp.py:119 under Bayesian_optimization/acq.py:48-68) -- and on an autoregressive stack with that kernel on every
fidelity, trained on (300, 300, 250) points, the sizes of the reference's multi-fidelity demo
(MF_BayesianOptimization/Discrete/DMF_acq.py:226-262 on AR; two_fidelity_models/AR_autoRegression.py:31-34 for the kernel).
The one-launch tree kernels stop at 256 points, so without keywords both run the per-step loop (`predict_diff` + torch.optim.Adam, a
Python round trip per step); `fuse_composed=True` with `staged=True` keeps the loop in the library: launch per stage, every step
enqueued by one call (ffgp_acq_optimize_stack_tree_staged).

python examples/acq_optimize_large_n_sum_kernel.py        (needs an MI355X: the library has no CPU path)
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fidelityfusion_amd import acq, kernel
from fidelityfusion_amd.cigp_v10 import cigp, train_many

torch.set_default_dtype(torch.float64)
dev = torch.device("cuda", 0)
gen = torch.Generator().manual_seed(7)
D, NS, RHO, Q, STEPS, LR = 2, (300, 300, 250), (0.8, 1.2), 500, 30, 0.05

# y_0 = f_0, y_s = rho_{s-1} y_{s-1} + residual_s: model s > 0 is trained on its residual set
f0 = lambda x: torch.sin(2.0 * x.sum(1, keepdim=True)) + 0.3 * x.sum(1, keepdim=True)
res = [None, lambda x: 0.3 * torch.cos(3.0 * x.sum(1, keepdim=True)), lambda x: 0.2 * x[:, :1] - 0.1]
data = []
for s, n in enumerate(NS):
    x = 2.0 * torch.rand(n, D, generator=gen)
    y = (f0(x) if s == 0 else res[s](x)) + 0.05 * torch.randn(n, 1, generator=gen)
    data.append((x.to(dev), y.to(dev)))
models = [cigp(kernel.SumKernel(kernel.LinearKernel(D), kernel.MaternKernel(D)), log_beta=1.0).to(dev) for _ in NS]
trace, _ = train_many(models, [x for x, _ in data], [y for _, y in data], 60, lr=5e-2)
for m in models:
    m.requires_grad_(False)                                   # frozen: from here on only the query points move
print("trained %d fidelities of %s points on Sum(Linear, Matern): losses %s -> %s"
      % (len(NS), NS, [round(v, 2) for v in trace[:, 0].tolist()], [round(v, 2) for v in trace[:, -1].tolist()]))
X0 = (2.0 * torch.rand(Q, D, generator=gen)).to(dev)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def compare(what, fn):
    fn(True), fn(False)                                       # warm-up: code objects, workspaces, the cached factors
    Xs, t_s = timed(lambda: fn(True))
    Xl, t_l = timed(lambda: fn(False))
    print("%s, %d start points, %d Adam iterations: staged call %.2f ms, per-step loop %.2f ms; largest difference of the answers %.2e"
          % (what, Q, STEPS, t_s, t_l, (Xs - Xl).abs().max().item()))
    return Xs


# both keywords select the staged call for composed kernels; without them the same entry runs the per-step loop
route = lambda staged: dict(fuse_composed=True, staged=True) if staged else {}

# the reference's BO model at 300 points: UCB = mean + 2 sqrt(var)
x0, y0 = data[0]
Xs = compare("single n = %d" % NS[0], lambda staged: acq.optimize_acqf(models[0], x0, y0, X0, steps=STEPS, lr=LR, acq="ucb", kappa=2.0,
                                                                         return_best_only=False, **route(staged)))
with torch.no_grad():
    mean, var = models[0](x0, y0, Xs)
    u = (mean + 2.0 * var.diag().reshape(-1, 1).sqrt())[:, 0]
    print("  best candidate x = (%.4f, %.4f), UCB there %.5f" % (Xs[int(u.argmax()), 0].item(), Xs[int(u.argmax()), 1].item(), u.max().item()))

# the AR stack at its top fidelity
compare("AR stack n = %s" % (NS,), lambda staged: acq.optimize_acqf_mf(models, data, X0, rho=RHO, steps=STEPS, lr=LR, acq="ucb", kappa=2.0,
                                                                        return_best_only=False, **route(staged)))
