"""The acquisition optimiser of the reference's multi-fidelity drivers (MF_BayesianOptimization/Discrete/DMF_acq.py:226-262) on an
autoregressive stack whose fidelities run on the reference's own composed kernel, SumKernel(LinearKernel, MaternKernel)
(two_fidelity_models/AR_autoRegression.py:31-34), on the MI355X: three fidelities with ragged training sets (60, 35, 20 points), one
`cigp` per fidelity trained by `cigp_v10.train_many` on the data / the residuals, frozen, and UCB_MF(x, s) = mean_s(x) + 0.2 D var_s(x)
maximised for EVERY fidelity s by `acq.optimize_acqf_mf`, each start point carrying its own level -- once as it runs by default on
such a stack, step by step (the members' `predict_diff` + torch.optim.Adam), once with `fuse_composed=True`, where all the iterations
of all the points are ONE kernel launch (ffgp_acq_optimize_stack_tree).

python examples/mf_acq_optimize_sum_kernel.py        (needs an MI355X: the library has no CPU path)
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
f0 = lambda x: torch.sin(2.0 * x.sum(1, keepdim=True)) + 0.3 * x.sum(1, keepdim=True)
res = [None, lambda x: 0.3 * torch.cos(3.0 * x.sum(1, keepdim=True)), lambda x: 0.2 * x[:, :1] - 0.1]
data = []
for s, n in enumerate(NS):
    x = 2.0 * torch.rand(n, D, generator=gen)
    y = (f0(x) if s == 0 else res[s](x)) + 0.05 * torch.randn(n, 1, generator=gen)
    data.append((x.to(dev), y.to(dev)))
models = [cigp(kernel.SumKernel(kernel.LinearKernel(D), kernel.MaternKernel(D)), log_beta=1.0).to(dev) for _ in NS]
trace, state = train_many(models, [x for x, _ in data], [y for _, y in data], 150, lr=5e-2)
for m in models:
    m.requires_grad_(False)                                   # frozen: from here on only the query points move
print("trained %d fidelities: losses %s -> %s" % (len(NS), [round(v, 3) for v in trace[:, 0].tolist()], [round(v, 3) for v in trace[:, -1].tolist()]))

Q, steps, lr, kappa = 200, 30, 0.05, 0.2 * D
X0 = (2.0 * torch.rand(len(NS) * Q, D, generator=gen)).to(dev)   # Q start points per level
level = torch.arange(len(NS)).repeat_interleave(Q)
run = lambda fuse: acq.optimize_acqf_mf(models, data, X0, rho=RHO, level=level, steps=steps, lr=lr, acq="ucb_var", kappa=kappa,
                                        return_best_only=False, fuse_composed=fuse)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


run(True), run(False)                                         # warm-up: code objects, workspaces, the cached factors
Xf, t_f = timed(lambda: run(True))
Xl, t_l = timed(lambda: run(False))
print("%d levels x %d start points, %d Adam iterations: one launch %.2f ms, the per-step loop %.2f ms" % (len(NS), Q, steps, t_f, t_l))
print("largest difference of the two answers: %.2e" % (Xf - Xl).abs().max().item())
best = acq.optimize_acqf_mf(models, data, X0, rho=RHO, level=level, steps=steps, lr=lr, acq="ucb_var", kappa=kappa, fuse_composed=True)
print("the reference's selection rule (select_best) keeps the final points: %s" % bool(torch.equal(best, Xf)))
