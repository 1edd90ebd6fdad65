"""The acquisition optimiser of the reference's Bayesian-optimisation drivers (Bayesian_optimization/acq.py:48-68, acq_demo.py:51-68)
on the MI355X, both ways: a 1-D surface, a `cigp` trained by `cigp_v10.train_many`, frozen, and UCB maximised from 500 start points
by 30 Adam iterations -- once step by step through `cigp.forward` under autograd (what the reference's loop does on the drop-in
modules), once by `acq.optimize_acqf`, which runs the whole loop in ONE kernel launch (ffgp_acq_optimize).  Same selection rule,
same answer.

python examples/acq_optimize.py        (needs an MI355X: the library has no CPU path)
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
ytr = torch.sin(xtr) + 0.3 * torch.sin(3.1 * xtr) + torch.randn(40, 1, generator=gen) * 0.1
xtr, ytr = xtr.to(dev), ytr.to(dev)

model = cigp(kernel.ARDKernel(1), log_beta=1.0).to(dev)
trace, state = train_many([model], [xtr], [ytr], 200, lr=5e-2)
assert state["fused"]
model.requires_grad_(False)                                   # frozen: from here on only the query points move
print("trained: loss %.4f -> %.4f" % (trace[0, 0].item(), trace[0, -1].item()))

X0 = (torch.rand(500, 1, generator=gen) * 6).to(dev)
steps, lr, kappa = 30, 0.1, 2.0


def reference_loop():
    """acq.py:48-68 with UCB (acq.py:132-144) on the model's posterior, from X0"""
    ucb = acq.UCB(lambda X: model(xtr, ytr, X)[0], lambda X: model(xtr, ytr, X)[1].diag().reshape(-1, 1), kappa)
    X = X0.clone().requires_grad_(True)
    opt = torch.optim.Adam([X], lr=lr)
    with torch.no_grad():
        best_x, best_value = X0.clone(), float(-ucb.forward(X0).sum())
    for _ in range(steps):
        opt.zero_grad()
        loss = -ucb.forward(X).sum()
        loss.backward()
        opt.step()
        if loss.item() < best_value:
            best_value, best_x = loss.item(), X.detach().clone()
    return best_x


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


fused = lambda: acq.optimize_acqf(model, xtr, ytr, X0, steps=steps, lr=lr, acq="ucb", kappa=kappa, var_floor=0.0)
fused(), reference_loop()                                     # warm-up: code objects, workspaces, the cached factor
best_f, t_f = timed(fused)
best_l, t_l = timed(reference_loop)

with torch.no_grad():
    mean, var = model(xtr, ytr, best_f)
    u = (mean[:, 0] + kappa * var.diag().sqrt())
top = int(u.argmax())
print("%d start points, %d Adam iterations: one launch %.2f ms, per-step loop %.2f ms" % (X0.shape[0], steps, t_f, t_l))
print("largest difference of the two answers: %.2e" % (best_f - best_l).abs().max().item())
print("best candidate: x = %.6f (one launch), %.6f (loop); UCB there %.6f" % (best_f[top, 0].item(), best_l[top, 0].item(), u[top].item()))
