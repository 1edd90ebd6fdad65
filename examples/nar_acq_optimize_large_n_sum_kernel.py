"""The acquisition optimiser on a nonlinear autoregressive chain (FidelityFusion_Models/NAR.py:30-61) whose fidelities run on the
reference's own composed kernel, SumKernel(LinearKernel, MaternKernel) (two_fidelity_models/NAR_NonlinearAR.py:23-26), past 256
training points on the MI355X, both ways: three fidelities trained on (300, 300, 250) points -- the sizes of NAR's own demo
(NAR.py:119-128) --, one `cigp` per fidelity, fidelity s > 0 trained on [x, mean of fidelity s - 1 at x], so its linear leaf weighs the
mean below like any other input, frozen, and UCB_MF(x, s) = mean_s(x) + 0.2 D var_s(x)
(MF_BayesianOptimization/Discrete/DMF_acq.py:226-262) maximised for EVERY fidelity s from one call of `acq.optimize_acqf_nar`, each
start point carrying its own level.  The one-launch kernel for composed chains stops at 256 points, so with `fuse_composed=True` that
call runs the per-step loop (`PosteriorChain.predict_diff` + torch.optim.Adam, a Python round trip per step);
`fuse_composed="staged", staged=True` keeps the loop in the library: launch per stage, every step enqueued by one call
(ffgp_acq_optimize_chain_tree_staged).

python examples/nar_acq_optimize_large_n_sum_kernel.py        (needs an MI355X: the library has no CPU path)
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
D, NS, Q, STEPS, LR = 2, (300, 300, 250), 200, 30, 0.05
KAPPA = 0.2 * D

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
    trace, _ = train_many([m], [x], [truth + noise], 60, lr=5e-2)
    m.requires_grad_(False)                                   # frozen: from here on only the query points move
    models.append(m)
    data.append((x, truth + noise) if s == 0 else (x, [truth + noise, torch.zeros_like(noise)]))
    print("fidelity %d trained on %d points with %d inputs: loss %.3f -> %.3f" % (s, n, x.shape[1], trace[0, 0].item(), trace[0, -1].item()))

X0 = (2.0 * torch.rand(len(NS), Q, D, generator=gen)).to(dev)   # Q start points per level
level = torch.arange(len(NS)).repeat_interleave(Q)
run = lambda **kw: acq.optimize_acqf_nar(models, data, X0.reshape(-1, D), level=level, steps=STEPS, lr=LR, acq="ucb_var", kappa=KAPPA,
                                         return_best_only=False, **kw).reshape(len(NS), Q, D)
staged = lambda: run(fuse_composed="staged", staged=True)
per_step = lambda: run(fuse_composed=True, staged=True)      # past 256 points these two keywords leave a composed chain on the loop


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


staged(), per_step()                                          # warm-up: code objects, workspaces, the cached factors
Xs, t_s = timed(staged)
Xl, t_l = timed(per_step)
print("NAR chain on Sum(Linear, Matern) n = %s, %d levels x %d start points, %d Adam iterations: staged call %.2f ms, per-step loop %.2f ms"
      % (NS, len(NS), Q, STEPS, t_s, t_l))
print("largest difference of the two answers: %.2e" % (Xs - Xl).abs().max().item())
with torch.no_grad():
    for s in range(len(NS)):
        low = var = None
        for f in range(s + 1):                                # NAR.forward(..., to_fidelity=s)
            z = Xs[s] if f == 0 else torch.cat([Xs[s], low.reshape(-1, 1)], dim=-1)
            low, var = models[f](data[f][0], data[f][1], z)
        u = (low + KAPPA * var.diag().reshape(-1, 1))[:, 0]
        top = int(u.argmax())
        print("level %d: best candidate x = (%.4f, %.4f), UCB_MF there %.5f" % (s, Xs[s, top, 0].item(), Xs[s, top, 1].item(), u[top].item()))
