"""Two field-valued fidelities of our own making -- an 8 x 8 field per input point, 64 output columns -- trained the way the reference
trains them: CIGAR's fidelity 0 (FidelityFusion_Models/CIGAR.py:149-176: a plain `cigp` on the flattened field) and a ResGP-style
residual fidelity (a `cigp` on y_high - rho * y_low, rho learned: `residual=`), 200 Adam iterations each, in two ways on the MI355X:
`train_many` as it stands (launch per stage for such wide outputs: 13 dependent launches per step) and
`train_many(..., wide_one_launch=True)`, which compresses the 64 columns to at most n (the residual member: 2 n) columns that carry
the same likelihood and gradients and runs ALL steps of both models in ONE kernel launch (csrc/train_wide.hip).  Same losses, same
parameters, to rounding.

python examples/cigar_train_many.py        (needs an MI355X: the fused training call has no CPU path)
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fidelityfusion_amd import kernel
from fidelityfusion_amd.cigp_v10 import cigp, train_many

torch.set_default_dtype(torch.float64)
dev = torch.device("cuda", 0)
gen = torch.Generator().manual_seed(11)
side = 8
gy, gx = torch.meshgrid(torch.linspace(0, 1, side), torch.linspace(0, 1, side), indexing="ij")


def field(x, level):                              # an 8 x 8 field per input point, flattened; the high level adds finer structure
    a, b = x[:, :1, None], x[:, 1:2, None]
    low = torch.sin(3.0 * a + 2.0 * gx) * torch.cos(2.0 * b + gy)
    fine = 0.3 * torch.sin(7.0 * a * gx + 5.0 * b * gy)
    return (low + (fine if level else 0.0)).reshape(x.shape[0], side * side)


n0, n1 = 48, 20                                   # many low-fidelity points, few high-fidelity ones
x0, x1 = torch.rand(n0, 2, generator=gen), torch.rand(n1, 2, generator=gen)
noise = lambda y: y + 0.02 * torch.randn(y.shape, generator=gen)
y0 = noise(field(x0, 0)).to(dev)
y_low, y_high = noise(field(x1, 0)).to(dev), noise(field(x1, 1)).to(dev)
x0, x1 = x0.to(dev), x1.to(dev)
steps, lr = 200, 1e-2


def build():
    models = [cigp(kernel.ARDKernel(2), 1.0).to(dev), cigp(kernel.ARDKernel(2), 1.0).to(dev)]
    rho = torch.nn.Parameter(torch.tensor(1.0, device=dev))
    return models, [None, (rho, y_low, y_high)]


def run(wide):
    models, res = build()
    warm, wres = build()
    train_many(warm, [x0, x1], [y0, None], 3, lr=lr, residual=wres, wide_one_launch=wide)      # (warm-up: workspaces, streams)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trace, state = train_many(models, [x0, x1], [y0, None], steps, lr=lr, residual=res, wide_one_launch=wide)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, trace, models, res[1][0], state


t_old, tr_old, m_old, rho_old, _ = run(False)
t_new, tr_new, m_new, rho_new, st = run(True)
assert st["wide_one_launch"] == [0, 1]
print("fidelity 0: %d points, residual fidelity: %d points, %d x %d field (%d columns), %d Adam steps each" % (n0, n1, side, side, side * side, steps))
print("  train_many, launch per stage     %7.1f ms    final losses %s" % (t_old * 1e3, ["%.4f" % v for v in tr_old[:, -1].tolist()]))
print("  train_many, wide_one_launch      %7.1f ms    final losses %s" % (t_new * 1e3, ["%.4f" % v for v in tr_new[:, -1].tolist()]))
print("  largest relative difference of the loss traces: %.1e" % float(((tr_new - tr_old).abs() / tr_old.abs().clamp_min(1e-300)).max()))
for f, (a, b) in enumerate(zip(m_new, m_old)):
    d = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(a.parameters(), b.parameters()))
    print("  fidelity %d: length scales %s, largest parameter difference %.1e" % (f, ["%.3f" % abs(float(v)) for v in a.kernel.length_scales.detach()], d))
print("  rho %.6f (launch per stage %.6f)" % (float(rho_new.detach()), float(rho_old.detach())))
