"""A three-fidelity continuous auto-regression (CAR) model of our own making, trained the way
FidelityFusion_Models/CAR_ContinuousAutoRegression.py:116-142 trains one -- fidelity 0 a `GP_basic` on its data, every fidelity above it a
`GP_basic` over `kernel.FidelityKernelMCMC` on the residual y_high - exp(b) * y_low, b shared by all fidelities, 200 Adam iterations each
-- in two ways on the MI355X: the reference's per-iteration loop through the drop-in modules (the fidelity integral formed by torch on
the host at every step), and `gp_basic.train_many(..., car=)`, which runs all iterations of a fidelity in one library call (targets,
fidelity integral, likelihood, the six gradients and Adam's update on the device).  Same losses, same parameters, to the rounding of the
reference's binary32 step.

python examples/car_train_many.py        (needs an MI355X: the fused training call has no CPU path)
"""
import copy
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fidelityfusion_amd import kernel
from fidelityfusion_amd.gp_basic import GP_basic, train_many

dev = torch.device("cuda", 0)
gen = torch.Generator().manual_seed(7)
f64 = dict(dtype=torch.float64)


class CAR(torch.nn.Module):
    """ContinuousAutoRegression's blocks (:69-92): one b, a plain block, and a fidelity-kernel block per step up"""

    def __init__(self, fidelity_num):
        super().__init__()
        self.b = torch.nn.Parameter(torch.tensor(1.0))
        blocks = [GP_basic(kernel.ARDKernel(1), 1.0)]
        for f in range(fidelity_num - 1):
            blocks.append(GP_basic(kernel.FidelityKernelMCMC(1, kernel.ARDKernel(1), f, f + 1, self.b), 1.0))
        self.cigp_list = torch.nn.ModuleList(blocks)


def truth(x, level):                              # three levels of one function: each adds finer structure to the one below
    y = torch.sin(x) - 0.5 * torch.sin(2.0 * x)
    return y + (0.2 * torch.sin(2.0 * x) if level >= 1 else 0.0) + (0.3 * torch.sin(2.0 * x) if level >= 2 else 0.0)


sizes = (300, 300, 250)                           # as in the reference's own demo
x0 = torch.rand(sizes[0], 1, generator=gen, **f64) * 10
y0 = truth(x0, 0) + 0.05 * torch.rand(sizes[0], 1, generator=gen, **f64)
overlaps = []                                     # (x, y_low, y_high) on the inputs fidelities f - 1 and f share
for f in (1, 2):
    x = torch.rand(sizes[f], 1, generator=gen, **f64) * 10
    overlaps.append(tuple(t.to(dev) for t in (x, truth(x, f - 1), truth(x, f) + 0.05 * torch.rand(sizes[f], 1, generator=gen, **f64))))
x0, y0 = x0.to(dev), y0.to(dev)
steps, lr = 200, 1e-2


def fused(model):
    trace, _ = train_many([model.cigp_list[0]], [x0], [y0], steps, lr=lr)
    traces = [trace[0]]
    for f, (x, yl, yh) in enumerate(overlaps, start=1):       # a fresh optimiser per fidelity, as train_CAR has it
        trace, state = train_many([model.cigp_list[f]], [x], [None], steps, lr=lr, car=[(model.b, yl, yh)])
        traces.append(trace[0])                               # (state["residual_targets"][0][0]: the fidelity's data for forward)
    return torch.stack(traces).cpu()


def loop(model):
    out = torch.zeros(3, steps, **f64)
    for f in range(3):
        opt = torch.optim.Adam(model.parameters(), lr=lr)
        for i in range(steps):
            opt.zero_grad()
            if f == 0:
                loss = -model.cigp_list[0].log_likelihood(x0, y0)
            else:
                x, yl, yh = overlaps[f - 1]
                loss = -model.cigp_list[f].log_likelihood(x, yh - model.b.exp() * yl)
            loss.sum().backward()
            opt.step()
            out[f, i] = float(loss.detach())
    return out


model = CAR(3).double().to(dev)
twin = copy.deepcopy(model)
fused(copy.deepcopy(model))                       # (warm-up: workspaces, streams)
torch.cuda.synchronize()
t0 = time.perf_counter()
trace = fused(model)
torch.cuda.synchronize()
t_many = time.perf_counter() - t0
t0 = time.perf_counter()
ref = loop(twin)
torch.cuda.synchronize()
t_loop = time.perf_counter() - t0

print("3 fidelities (%s points), %d Adam steps each" % (" / ".join(map(str, sizes)), steps))
print("  train_many          %7.1f ms    final losses %s" % (t_many * 1e3, ["%.4f" % v for v in trace[:, -1].tolist()]))
print("  per-iteration loop  %7.1f ms    final losses %s" % (t_loop * 1e3, ["%.4f" % v for v in ref[:, -1].tolist()]))
print("  largest relative difference of the loss traces: %.1e" % float(((trace - ref).abs() / ref.abs().clamp_min(1e-300)).max()))
print("  b = %.6f (loop: %.6f)" % (float(model.b.detach()), float(twin.b.detach())))
for (name, p), q in zip(model.named_parameters(), twin.parameters()):
    print("  %-44s %10.6f   difference %.1e" % (name, float(p.detach().reshape(-1)[0]), float((p.detach() - q.detach()).abs().max())))
