"""The acquisition optimiser on the reference's own Bayesian-optimisation model -- a `cigp` on SumKernel(LinearKernel, MaternKernel)
(Bayesian_optimization/cigp.py:119, cigp_v10.py:81) -- on the MI355X, both ways: a 1-D surface with a trend, the model trained by
`cigp_v10.train_many`, frozen, and UCB maximised from 500 start points by 30 Adam iterations -- once by the per-step loop
(`acq.optimize_acqf` as it routes a composed kernel by default: `predict_diff` + torch.optim.Adam), once with `fuse_composed=True`,
which runs the whole loop in ONE kernel launch (ffgp_acq_optimize_tree, csrc/acq_tree.hip).  Same selection rule, same answer.

python examples/acq_optimize_sum_kernel.py        (needs an MI355X: the library has no CPU path)
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

xtr = torch.rand(40, 1, generator=gen) * 6
ytr = 0.4 * xtr + torch.sin(xtr) + 0.3 * torch.sin(3.1 * xtr) + torch.randn(40, 1, generator=gen) * 0.1
xtr, ytr = xtr.to(dev), ytr.to(dev)

model = cigp(kernel.SumKernel(kernel.LinearKernel(1), kernel.MaternKernel(1)), log_beta=1.0).to(dev)
trace, state = train_many([model], [xtr], [ytr], 200, lr=5e-2)
model.requires_grad_(False)                                   # frozen: from here on only the query points move
print("trained (one launch: %s): loss %.4f -> %.4f" % (state["fused"], trace[0, 0].item(), trace[0, -1].item()))

X0 = (torch.rand(500, 1, generator=gen) * 6).to(dev)
steps, lr, kappa = 30, 0.1, 2.0


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


fused = lambda: acq.optimize_acqf(model, xtr, ytr, X0, steps=steps, lr=lr, acq="ucb", kappa=kappa, var_floor=0.0, fuse_composed=True)
per_step = lambda: acq.optimize_acqf(model, xtr, ytr, X0, steps=steps, lr=lr, acq="ucb", kappa=kappa, var_floor=0.0)
fused(), per_step()                                           # warm-up: code objects, workspaces, the cached factor
best_f, t_f = timed(fused)
best_l, t_l = timed(per_step)

with torch.no_grad():
    mean, var = model(xtr, ytr, best_f)
    u = (mean[:, 0] + kappa * var.diag().sqrt())
top = int(u.argmax())
print("%d start points, %d Adam iterations: one launch %.2f ms, per-step loop %.2f ms" % (X0.shape[0], steps, t_f, t_l))
print("largest difference of the two answers: %.2e" % (best_f - best_l).abs().max().item())
print("best candidate: x = %.6f (one launch), %.6f (loop); UCB there %.6f" % (best_f[top, 0].item(), best_l[top, 0].item(), u[top].item()))
