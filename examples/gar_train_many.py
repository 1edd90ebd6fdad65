"""A two-fidelity GAR model of our own making on synthetic 8 x 8 fields, trained the way FidelityFusion_Models/GAR.py:76-126 trains one
-- fidelity 0 a `HOGP_simple` block on the low-fidelity fields, fidelity 1 a `HOGP_simple` block on the residual
y_high - Tensor_linear(y_low) over the points both fidelities share, the Tensor_linear's last matrix learned along -- in two ways on
the MI355X: the reference's per-iteration loop through the drop-in modules, and `hogp_simple.train_many`, which runs all iterations
of a fidelity in one library call (targets, assembly, eigensolvers, the Kronecker likelihood and its closed-form backward, Adam's
update, all on the device).  Same losses, same parameters, to rounding.

python examples/gar_train_many.py        (needs an MI355X: the fused training call has no CPU path)
"""
import copy
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fidelityfusion_amd import kernel
from fidelityfusion_amd.gp_computation_pack import Tensor_linear
from fidelityfusion_amd.hogp_simple import HOGP_simple, train_many

dev = torch.device("cuda", 0)
gen = torch.Generator().manual_seed(11)
f64 = dict(dtype=torch.float64)
shape = (8, 8)
n_low, n_high = 100, 32                           # as in Experiments/GAR_Aligned/exp_aligned.py: 100 low- against 4..32 high-fidelity points
steps, lr = 200, 1e-2


class GAR(torch.nn.Module):
    """GAR's blocks (GAR.py:14-31): a HOGP block per fidelity and the map between consecutive output shapes"""

    def __init__(self):
        super().__init__()
        self.hogp_list = torch.nn.ModuleList([HOGP_simple(kernel.ARDKernel(2), 1.0, shape) for _ in range(2)])
        self.Tensor_linear_list = torch.nn.ModuleList([Tensor_linear(shape, shape)])


def field(x, level):                              # an 8 x 8 field per input point; the high fidelity adds finer structure
    u = torch.linspace(0, 1, shape[0], **f64).reshape(1, -1, 1)
    v = torch.linspace(0, 1, shape[1], **f64).reshape(1, 1, -1)
    a, b = x[:, 0].reshape(-1, 1, 1), x[:, 1].reshape(-1, 1, 1)
    y = torch.sin(3 * a + 2 * u) * torch.cos(2 * b + v)
    return y + (0.3 * torch.sin(5 * a * u + 3 * b * v) if level else 0.0)


x0 = torch.rand(n_low, 2, generator=gen, **f64)
y0 = field(x0, 0) + 0.02 * torch.randn(n_low, *shape, generator=gen, **f64)
x1 = x0[:n_high].clone()                          # the points both fidelities share
y_low = y0[:n_high].clone()
y_high = field(x1, 1) + 0.02 * torch.randn(n_high, *shape, generator=gen, **f64)
x0, y0, x1, y_low, y_high = (t.to(dev) for t in (x0, y0, x1, y_low, y_high))


def fused(model):
    t0, _ = train_many([model.hogp_list[0]], [x0], [y0], steps, lr=lr)
    t1, _ = train_many([model.hogp_list[1]], [x1], [None], steps, lr=lr, residual=[(model.Tensor_linear_list[0], y_low, y_high)])
    return torch.stack([t0[0], t1[0]]).cpu()


def loop(model):
    out = torch.zeros(2, steps, **f64)
    for f in range(2):
        opt = torch.optim.Adam(model.parameters(), lr=lr)     # a fresh optimiser per fidelity, as train_GAR has it
        for i in range(steps):
            opt.zero_grad()
            if f == 0:
                loss = model.hogp_list[0].log_likelihood(x0, y0)
            else:
                loss = model.hogp_list[1].log_likelihood(x1, y_high - model.Tensor_linear_list[0](y_low))
            loss.backward()
            opt.step()
            out[f, i] = float(loss.detach())
    return out


model = GAR().double().to(dev)
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

print("2 fidelities (%d / %d points, %s fields), %d Adam steps each" % (n_low, n_high, "x".join(map(str, shape)), steps))
for f in range(2):
    print("  fidelity %d loss trace  train_many %s ... %.6f    loop %s ... %.6f" % (
        f, ["%.6f" % v for v in trace[f, :3].tolist()], float(trace[f, -1]), ["%.6f" % v for v in ref[f, :3].tolist()], float(ref[f, -1])))
print("  train_many          %8.1f ms" % (t_many * 1e3))
print("  per-iteration loop  %8.1f ms" % (t_loop * 1e3))
print("  largest relative difference of the loss traces: %.1e" % float(((trace - ref).abs() / ref.abs().clamp_min(1e-300)).max()))
for (name, p), q in zip(model.named_parameters(), twin.parameters()):
    if p.requires_grad:
        print("  %-44s difference %.1e" % (name, float((p.detach() - q.detach()).abs().max())))
with torch.no_grad():                             # forward runs straight after training: the blocks' caches are those of the last step
    xt = torch.rand(5, 2, generator=gen, **f64).to(dev)
    mean = model.hogp_list[0].forward(x0, xt)[0]
    mean_ref = twin.hogp_list[0].forward(x0, xt)[0]
print("  fidelity-0 posterior mean at 5 points: largest difference %.1e" % float((mean - mean_ref).abs().max()))
