"""The acquisition optimiser of the reference's multi-fidelity drivers (MF_BayesianOptimization/Discrete/DMF_acq.py:226-262) on a
nonlinear autoregressive chain (FidelityFusion_Models/NAR.py:30-61) whose fidelities run on the reference's own composed kernel,
SumKernel(LinearKernel, MaternKernel) (FidelityFusion_Models/two_fidelity_models/NAR_NonlinearAR.py:23-26), on the MI355X, both ways:
three fidelities with ragged training sets (60, 35, 20 points), one `cigp` per fidelity -- fidelity s > 0 trained on
[x, mean of fidelity s - 1 at x], the 'concat-s' set of the NAR trainer, so its linear leaf weighs the mean below like any other input --
frozen, and UCB_MF(x, s) = mean_s(x) + 0.2 D var_s(x) maximised for EVERY fidelity s: once as the drivers do it, a loop over s of
per-step Adam loops through the models' forward under autograd, once by `acq.optimize_acqf_nar(..., fuse_composed=True)`, where each
start point carries its own level and all of them run in ONE kernel launch (ffgp_acq_optimize_chain_tree).  Without the keyword the
same call runs the per-step loop.

python examples/nar_acq_optimize_sum_kernel.py        (needs an MI355X: the library has no CPU path)
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
gen = torch.Generator().manual_seed(11)
D, NS = 2, (60, 35, 20)

# y_s = g_s(x, y_{s-1}(x)): fidelity s > 0 is a nonlinear function of the fidelity below
f0 = lambda x: torch.sin(2.0 * x.sum(1, keepdim=True))
up = [None, lambda x, u: u * u + 0.3 * torch.cos(3.0 * x.sum(1, keepdim=True)), lambda x, u: 1.5 * u + 0.2 * x[:, :1] - 0.1]
models, data = [], []
for s, n in enumerate(NS):
    x = (2.0 * torch.rand(n, D, generator=gen)).to(dev)
    noise = (0.05 * torch.randn(n, 1, generator=gen)).to(dev)
    truth = f0(x)
    for f in range(1, s + 1):
        truth = up[f](x, truth)
    if s > 0:                                                 # the trainer's concat set: [x, the chain's own mean below], [y, y_var]
        with torch.no_grad():
            low = None
            for f in range(s):
                z = x if f == 0 else torch.cat([x, low], dim=-1)
                low = models[f](data[f][0], data[f][1], z)[0]
        x = torch.cat([x, low], dim=-1)
    m = cigp(kernel.SumKernel(kernel.LinearKernel(x.shape[1]), kernel.MaternKernel(x.shape[1])), log_beta=1.0).to(dev)
    trace, _ = train_many([m], [x], [truth + noise], 150, lr=5e-2)
    m.requires_grad_(False)                                   # frozen: from here on only the query points move
    models.append(m)
    data.append((x, truth + noise) if s == 0 else (x, [truth + noise, torch.zeros_like(noise)]))
    print("fidelity %d trained on %d points with %d inputs: loss %.3f -> %.3f" % (s, n, x.shape[1], trace[0, 0].item(), trace[0, -1].item()))

Q, steps, lr, kappa = 200, 30, 0.05, 0.2 * D
X0 = (2.0 * torch.rand(len(NS), Q, D, generator=gen)).to(dev)   # Q start points per level


def posterior(X, s):
    """NAR.forward(..., to_fidelity=s): mean and diagonal variance of fidelity s, fed the means below"""
    low = var = None
    for f in range(s + 1):
        z = X if f == 0 else torch.cat([X, low.reshape(-1, 1)], dim=-1)
        low, var = models[f](data[f][0], data[f][1], z)
    return low, var.diag().reshape(-1, 1)


def drivers_loop():
    out = []
    for s in range(len(NS)):
        X = X0[s].clone().requires_grad_(True)
        opt = torch.optim.Adam([X], lr=lr)
        for _ in range(steps):
            opt.zero_grad()
            mean, var = posterior(X, s)
            (-(mean + kappa * var).sum()).backward()
            opt.step()
        out.append(X.detach())
    return torch.stack(out)


level = torch.arange(len(NS)).repeat_interleave(Q)
one_launch = lambda: acq.optimize_acqf_nar(models, data, X0.reshape(-1, D), level=level, steps=steps, lr=lr, acq="ucb_var", kappa=kappa,
                                           return_best_only=False, fuse_composed=True).reshape(len(NS), Q, D)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


one_launch(), drivers_loop()                                  # warm-up: code objects, workspaces, the cached factors
Xf, t_f = timed(one_launch)
Xl, t_l = timed(drivers_loop)
print("%d levels x %d start points, %d Adam iterations: one launch %.2f ms, a per-step loop per level %.2f ms" % (len(NS), Q, steps, t_f, t_l))
print("largest difference of the two answers: %.2e" % (Xf - Xl).abs().max().item())
with torch.no_grad():
    for s in range(len(NS)):
        mean, var = posterior(Xf[s], s)
        u = (mean + kappa * var)[:, 0]
        top = int(u.argmax())
        print("level %d: best candidate x = (%.4f, %.4f), UCB_MF there %.5f" % (s, Xf[s, top, 0].item(), Xf[s, top, 1].item(), u[top].item()))
