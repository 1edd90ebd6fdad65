"""A two-fidelity AR on the reference's own kernel -- SumKernel(LinearKernel, MaternKernel) per fidelity, as
two_fidelity_models/AR_autoRegression.py:31-37 builds it -- trained in two ways on the MI355X: train_AR's per-iteration loops
(FidelityFusion_Models/AR_autoRegression.py:103-137) through the drop-in modules, and `cigp_v10.train_many`: fidelity 0 in one
ffgp_train_tree_raw call, fidelity 1 -- the residual y_high - rho * y_low, rho trained with the GP -- in one ffgp_train_tree_res_raw call
under `fuse_composed=True`.  Same losses, same parameters, same rho; the two trajectories' distance is printed.

python examples/ar_sum_kernel_train_many.py        (needs an MI355X: the fused training call has no CPU path)
"""
import copy
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fidelityfusion_amd import kernel
from fidelityfusion_amd.cigp_v10 import cigp, train_many

torch.set_default_dtype(torch.float64)
dev = torch.device("cuda", 0)
gen = torch.Generator().manual_seed(7)

n, steps, lr = 60, 100, 1e-2
x = (torch.rand(n, 1, generator=gen) * 6).to(dev)
y_low = (torch.sin(x.cpu()) - 0.5 * torch.sin(2 * x.cpu()) + torch.rand(n, 1, generator=gen) * 0.1 - 0.05).to(dev)
y_high = (torch.sin(x.cpu()) - 0.3 * torch.sin(2 * x.cpu()) + torch.rand(n, 1, generator=gen) * 0.1 - 0.05).to(dev)

demo = lambda: cigp(kernel.SumKernel(kernel.LinearKernel(1), kernel.MaternKernel(1)), log_beta=1.0).to(dev)
gps = [demo(), demo()]
rho = torch.nn.Parameter(torch.tensor(1.0, device=dev))
twins, trho = copy.deepcopy(gps), torch.nn.Parameter(rho.detach().clone())


def fused(models, r, k):
    tr0, _ = train_many([models[0]], [x], [y_low], k, lr=lr)
    tr1, st = train_many([models[1]], [x], [None], k, lr=lr, residual=[(r, y_low, y_high)], fuse_composed=True)
    assert st["fused"], "the residual fidelity was trained by the reference loop, not by the library call"
    return torch.cat([tr0[0], tr1[0]]), st


fused(copy.deepcopy(gps), torch.nn.Parameter(rho.detach().clone()), 2)      # warm-up: code objects, workspaces
torch.cuda.synchronize()
t0 = time.perf_counter()
trace, state = fused(gps, rho, steps)
torch.cuda.synchronize()
t_many = time.perf_counter() - t0

(-copy.deepcopy(twins[0]).negative_log_likelihood(x, y_low)).backward()      # warm-up of the per-step route
torch.cuda.synchronize()
losses = []
t0 = time.perf_counter()
for f in range(2):      # train_AR: one Adam over the whole model per fidelity; only this fidelity's parameters (and rho) have gradients
    opt = torch.optim.Adam(list(twins[f].parameters()) + ([trho] if f else []), lr=lr)
    for i in range(steps):
        opt.zero_grad()
        loss = -twins[f].negative_log_likelihood(x, y_low if f == 0 else y_high - trho * y_low)
        loss.backward()
        opt.step()
        losses.append(loss.item())
torch.cuda.synchronize()
t_loop = time.perf_counter() - t0

print("fidelity iter   train_many        per-step loop")
for i in list(range(0, 2 * steps, 20)) + [2 * steps - 1]:
    print("%8d %4d   %.10f   %.10f" % (i // steps, i % steps, trace[i].item(), losses[i]))
# (each fidelity's losses against that fidelity's largest loss: the second trace crosses zero, where a ratio per step says nothing)
dist = max(max(abs(trace[i].item() - losses[i]) for i in range(f * steps, (f + 1) * steps)) / max(abs(v) for v in losses[f * steps:(f + 1) * steps])
           for f in range(2))
for f in range(2):
    for p, q in zip(gps[f].parameters(), twins[f].parameters()):
        # (against max(|parameter|, 1): the linear leaf's centre passes through zero near iteration 95, where a relative
        #  distance measures nothing -- two runs of the per-step loop one ulp apart are 1e-10 apart by it there)
        dist = max(dist, ((p - q).abs().max() / max(q.abs().max().item(), 1.0)).item())
dist = max(dist, ((rho - trho).abs() / trho.abs()).item())
print("rho: train_many %.10f, loop %.10f" % (rho.item(), trho.item()))
print("distance of the two trajectories (losses, parameters, rho): %.2e" % dist)
print("2 x %d iterations: train_many %.2f ms, per-step loop %.2f ms" % (steps, t_many * 1e3, t_loop * 1e3))
res_mean, _ = state["residual_targets"][0]      # what train_AR hands to add_data: the residual at the rho of the start of the last step
with torch.no_grad():
    m0, _ = gps[0](x, y_low, x[:3])
    m1, _ = gps[1](x, res_mean, x[:3])
print("AR mean at the first three points: %s   (y_high there: %s)" % ((rho.detach() * m0 + m1).flatten().cpu().numpy().round(4),
                                                                      y_high[:3].flatten().cpu().numpy().round(4)))
