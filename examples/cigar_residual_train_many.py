"""A three-fidelity CIGAR of our own making on 12 output columns, trained the way the reference trains it
(FidelityFusion_Models/CIGAR.py:84-134, subset form): fidelity 0 a plain `cigp`, every fidelity above it a `cigp` on
y_high - Tensor_linear(y_low) whose map sits under the same Adam as the three GP parameters -- 100 Adam iterations per fidelity, in two
ways on the MI355X: the reference's loop through the drop-in modules (one Python round trip, one autograd graph and one optimiser step
per iteration) and `train_many(..., residual=[(tensor_linear, y_low, y_high)])`, which runs all steps of a fidelity in ONE kernel launch
(csrc/train.hip, the tensor-linear class: the map's matrix, its moments and its gradient stay in LDS).  Same losses, same parameters,
same maps, to rounding.  (Much further on this data's trajectory amplifies rounding: at 200 steps two fp64 evaluations of the reference's
own loop, the drop-in modules on the GPU and plain torch on the CPU, are 5e-3 apart in the loss, and the fused call lies as close to either.)

python examples/cigar_residual_train_many.py        (needs an MI355X: the fused training call has no CPU path)
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fidelityfusion_amd import kernel
from fidelityfusion_amd.cigp_v10 import cigp, train_many
from fidelityfusion_amd.gp_computation_pack import Tensor_linear

torch.set_default_dtype(torch.float64)
dev = torch.device("cuda", 0)
gen = torch.Generator().manual_seed(5)
cols = torch.linspace(0, 1, 12)


def level(x, f):                                  # 12 columns per input point; every level adds finer structure and a gain
    a, b = x[:, :1], x[:, 1:2]
    y = torch.sin(3.0 * a + 2.0 * cols) * torch.cos(2.0 * b)
    for k in range(1, f + 1):
        y = (1.0 + 0.1 * k) * y + 0.2 / k * torch.sin((4.0 + 3.0 * k) * a * cols + 5.0 * b)
    return y


ns = (60, 40, 30)                                 # nested designs: the first n_f points of one sample carry fidelity f
x_all = torch.rand(ns[0], 2, generator=gen)
noise = lambda y: y + 0.02 * torch.randn(y.shape, generator=gen)
xs = [x_all[:n].to(dev) for n in ns]
ys = [noise(level(x_all[:n], f)).to(dev) for f, n in enumerate(ns)]
steps, lr = 100, 1e-2


def build():
    gps = [cigp(kernel.ARDKernel(2), 1.0).to(dev) for _ in ns]
    maps = [Tensor_linear((12,), (12,)).double().to(dev) for _ in ns[1:]]
    return gps, maps


def links(maps):                                  # fidelity f trains on y_f - map(y_{f-1}) at its own points (the subset form)
    return [None] + [(maps[f - 1], ys[f - 1][:ns[f]].contiguous(), ys[f]) for f in range(1, len(ns))]


def reference_loop(gps, maps, k):
    trace = []
    for f, (m, x) in enumerate(zip(gps, xs)):
        opt = torch.optim.Adam(list(m.parameters()) + (list(maps[f - 1].parameters()) if f else []), lr=lr)
        for _ in range(k):
            opt.zero_grad()
            y = ys[0] if f == 0 else ys[f] - maps[f - 1](ys[f - 1][:ns[f]])
            loss = -m.negative_log_likelihood(x, y)
            loss.backward()
            opt.step()
            trace.append(float(loss.detach()))
    return torch.tensor(trace).reshape(len(ns), k)


def fused(gps, maps, k):
    res = links(maps)
    rows = []
    for f in range(len(ns)):                      # (fidelity after fidelity, as train_CIGAR goes: one call each)
        tr, state = train_many([gps[f]], [xs[f]], [ys[0] if f == 0 else None], k, lr=lr, residual=[res[f]])
        assert state["fused"]
        rows.append(tr[0])
    return torch.stack(rows).cpu()


def timed(fn, k):
    gps, maps = build()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trace = fn(gps, maps, k)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, trace, gps, maps


timed(reference_loop, 3), timed(fused, 3)         # (warm-up: workspaces, streams, code objects)
t_ref, tr_ref, g_ref, m_ref = timed(reference_loop, steps)
t_new, tr_new, g_new, m_new = timed(fused, steps)
print("CIGAR, %d / %d / %d points, 12 columns, %d Adam steps per fidelity" % (*ns, steps))
print("  the reference's loop (drop-in modules)   %7.1f ms    final losses %s" % (t_ref * 1e3, ["%.4f" % v for v in tr_ref[:, -1].tolist()]))
print("  train_many with the Tensor_linear link   %7.1f ms    final losses %s" % (t_new * 1e3, ["%.4f" % v for v in tr_new[:, -1].tolist()]))
print("  largest relative difference of the loss traces: %.1e" % float(((tr_new - tr_ref).abs() / tr_ref.abs().clamp_min(1e-300)).max()))
for f, (a, b) in enumerate(zip(g_new, g_ref)):
    d = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(a.parameters(), b.parameters()))
    print("  fidelity %d: length scales %s, largest parameter difference %.1e" % (f, ["%.3f" % abs(float(v)) for v in a.kernel.length_scales.detach()], d))
for f, (a, b) in enumerate(zip(m_new, m_ref)):
    print("  map %d -> %d: diagonal %.4f ... %.4f, largest difference %.1e"
          % (f, f + 1, float(a.vectors[0].detach().diagonal().min()), float(a.vectors[0].detach().diagonal().max()),
             float((a.vectors[0].detach() - b.vectors[0].detach()).abs().max())))
