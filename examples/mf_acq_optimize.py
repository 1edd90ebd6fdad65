"""The acquisition optimiser of the reference's multi-fidelity drivers (MF_BayesianOptimization/Discrete/DMF_acq.py:226-262) on an
autoregressive stack (FidelityFusion_Models/AR_autoRegression.py:56-89) on the MI355X, both ways: three fidelities with ragged
training sets (60, 35, 20 points), one `cigp` per fidelity trained by `cigp_v10.train_many` on the data / the residuals, frozen, and
UCB_MF(x, s) = mean_s(x) + 0.2 D var_s(x) maximised for EVERY fidelity s -- once as the drivers do it, a loop over s of per-step
Adam loops through the models' forward under autograd, once by `acq.optimize_acqf_mf`, where each start point carries its own level
and all of them run in ONE kernel launch (ffgp_acq_optimize_stack).

python examples/mf_acq_optimize.py        (needs an MI355X: the library has no CPU path)
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
D, NS, RHO = 2, (60, 35, 20), (0.8, 1.2)

# y_0 = f_0, y_s = rho_{s-1} y_{s-1} + residual_s: model s > 0 is trained on its residual set
f0 = lambda x: torch.sin(2.0 * x.sum(1, keepdim=True))
res = [None, lambda x: 0.3 * torch.cos(3.0 * x.sum(1, keepdim=True)), lambda x: 0.2 * x[:, :1] - 0.1]
data = []
for s, n in enumerate(NS):
    x = 2.0 * torch.rand(n, D, generator=gen)
    y = (f0(x) if s == 0 else res[s](x)) + 0.05 * torch.randn(n, 1, generator=gen)
    data.append((x.to(dev), y.to(dev)))
models = [cigp(kernel.ARDKernel(D), log_beta=1.0).to(dev) for _ in NS]
trace, state = train_many(models, [x for x, _ in data], [y for _, y in data], 150, lr=5e-2)
for m in models:
    m.requires_grad_(False)                                   # frozen: from here on only the query points move
print("trained %d fidelities: losses %s -> %s" % (len(NS), [round(v, 3) for v in trace[:, 0].tolist()], [round(v, 3) for v in trace[:, -1].tolist()]))

Q, steps, lr, kappa = 200, 30, 0.05, 0.2 * D
X0 = (2.0 * torch.rand(len(NS), Q, D, generator=gen)).to(dev)   # Q start points per level
coefs = (1.0,) + RHO


def posterior(X, s):
    """AR.forward(..., to_fidelity=s): mean and diagonal variance"""
    mean = var = 0.0
    for f in range(s + 1):
        m, v = models[f](data[f][0], data[f][1], X)
        mean, var = mean + coefs[f] * m, var + coefs[f] ** 2 * v.diag().reshape(-1, 1)
    return mean, var


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
one_launch = lambda: acq.optimize_acqf_mf(models, data, X0.reshape(-1, D), rho=RHO, level=level, steps=steps, lr=lr, acq="ucb_var", kappa=kappa,
                                          return_best_only=False).reshape(len(NS), Q, D)


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
