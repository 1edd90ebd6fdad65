"""The reference's own `cigp` demo (GaussianProcess/cigp_v10.py:75-91: 16 noisy points of sin(x) + 10, SumKernel(LinearKernel(1),
MaternKernel(1)), log_beta = 1, Adam with lr = 0.1, 100 iterations) trained in two ways on the MI355X: the demo's per-iteration loop
through the drop-in modules, and `cigp_v10.train_many`, which runs the same iterations in ONE library call (ffgp_train_tree_raw: the
links of both leaves, the likelihood, its closed-form gradients and Adam's update on the device).  Same losses, same parameters.
With `tree_one_launch=True` the call is ONE kernel launch for all the iterations (ffgp_train_tree_lds_raw, models of at most 128
points): the third column.

python examples/sum_kernel_train_many.py        (needs an MI355X: the fused training call has no CPU path)
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
gen = torch.Generator().manual_seed(16)

xtr = torch.rand(16, 1, generator=gen) * 6
ytr = torch.sin(xtr) + torch.randn(16, 1, generator=gen) * 0.5 + 10       # (the +10 matters: it keeps the trajectory well-conditioned)
xte = torch.linspace(0, 6, 100).view(-1, 1)
xtr, ytr, xte = xtr.to(dev), ytr.to(dev), xte.to(dev)

model = cigp(kernel.SumKernel(kernel.LinearKernel(1), kernel.MaternKernel(1)), log_beta=1.0).to(dev)
twin, one = copy.deepcopy(model), copy.deepcopy(model)
steps, lr = 100, 1e-1

train_many([copy.deepcopy(model)], [xtr], [ytr], 2, lr=lr)                # warm-up: code objects, workspaces
torch.cuda.synchronize()
t0 = time.perf_counter()
trace, state = train_many([model], [xtr], [ytr], steps, lr=lr)
torch.cuda.synchronize()
t_many = time.perf_counter() - t0
assert state["fused"], "the model was trained by the reference loop, not by the library call"

train_many([copy.deepcopy(one)], [xtr], [ytr], 2, lr=lr, tree_one_launch=True)
torch.cuda.synchronize()
t0 = time.perf_counter()
trace_one, state_one = train_many([one], [xtr], [ytr], steps, lr=lr, tree_one_launch=True)
torch.cuda.synchronize()
t_one = time.perf_counter() - t0
assert state_one["tree_one_launch"] == [0], "the model did not take the one-launch route"

optimizer = torch.optim.Adam(twin.parameters(), lr=lr)
losses = []
t0 = time.perf_counter()
for i in range(steps):
    optimizer.zero_grad()
    loss = -twin.negative_log_likelihood(xtr, ytr)
    loss.backward()
    optimizer.step()
    losses.append(loss.item())
torch.cuda.synchronize()
t_loop = time.perf_counter() - t0

print("iter   train_many        per-step loop     tree_one_launch=True")
for i in list(range(0, steps, 10)) + [steps - 1]:
    print("%4d   %.10f   %.10f     %.10f" % (i, trace[0, i].item(), losses[i], trace_one[0, i].item()))
worst = max(abs(trace[0, i].item() - losses[i]) / abs(losses[i]) for i in range(steps))
worst_one = max(abs(trace_one[0, i].item() - losses[i]) / abs(losses[i]) for i in range(steps))
print("largest relative difference from the loop's loss trace: %.2e, one launch %.2e" % (worst, worst_one))
for (name, p), q in zip(model.named_parameters(), twin.parameters()):
    print("%-32s %s   |difference| %.1e" % (name, p.detach().cpu().numpy().round(6), (p - q).abs().max().item()))
print("%d iterations: train_many %.2f ms, in one launch %.2f ms, per-step loop %.2f ms" % (steps, t_many * 1e3, t_one * 1e3, t_loop * 1e3))
with torch.no_grad():
    mean, var = model(xtr, ytr, xte)
print("posterior at x = 0, 3, 6: mean %s, std %s" % (mean[[0, 50, 99], 0].cpu().numpy().round(4), var.diag()[[0, 50, 99]].sqrt().cpu().numpy().round(4)))
