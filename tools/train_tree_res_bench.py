"""train_many(..., fuse_composed=True) -- residual and `GP_basic` members on the reference's demo kernel SumKernel(LinearKernel,
MaternKernel) on both routes, launch per stage (ffgp_train_tree_res_raw / ffgp_train_tree_raw) and, up to 128 points, one launch for all
steps (tree_one_launch=True: ffgp_train_tree_lds_res_raw) -- against the per-step loop these models ran on before, with
tools/train_bench.py tree's protocol: all in this process, alternating, three rounds each after a warm-up of each; ms per call as
median [min .. max].  Each fused call's SLOWEST round is asserted against the loop's FASTEST.

python tools/train_tree_res_bench.py [steps]        (default 200; the table of DESIGN.md section 4.8: profiles/train_tree_res_bench.txt)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench import synthetic_xy
from fidelityfusion_amd import kernel
from fidelityfusion_amd.cigp_v10 import cigp, train_many
from fidelityfusion_amd.gp_basic import GP_basic

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
dev = torch.device("cuda", 0)
torch.set_default_dtype(torch.float64)


def make(n, F, kind):
    """kind: "residual" (cigp, subset form), "residual_var" (cigp, [n, n] variances), "gpbasic" (plain targets)"""
    ms, xs, ys, rs = [], [], [], []
    for f in range(F):
        X, Y = synthetic_xy(n, 2, 1, seed=f)
        x, yl = torch.tensor(X, device=dev), torch.tensor(Y, device=dev)
        yh = 1.3 * yl + 0.2 * torch.cos(2 * x[:, :1])
        k = kernel.SumKernel(kernel.LinearKernel(2), kernel.MaternKernel(2))
        ms.append((GP_basic(k, 1.0) if kind == "gpbasic" else cigp(k, 1.0)).to(dev))
        xs.append(x)
        if kind == "gpbasic":
            ys.append(yh), rs.append(None)
            continue
        rho = torch.nn.Parameter(torch.tensor(1.0, device=dev))
        ys.append(None)
        if kind == "residual":
            rs.append((rho, yl, yh))
        else:
            g = torch.Generator().manual_seed(f)
            vl, vh = (torch.diag(0.005 + 0.02 * torch.rand(n, generator=g)).to(dev) for _ in range(2))
            rs.append((rho, [yl, vl], [yh, vh]))
    return ms, xs, ys, rs


def fused(case, k, one=False):
    ms, xs, ys, rs = case
    return train_many(ms, xs, ys, k, residual=rs, fuse_composed=True, tree_one_launch=one)


def loop(case, k):
    for m, x, y, res in zip(*case):
        opt = torch.optim.Adam(list(m.parameters()) + ([res[0]] if res is not None else []), lr=1e-2)
        for _ in range(k):
            opt.zero_grad()
            if res is not None:
                rho, yl, yh = res
                y = [yh[0] - rho * yl[0], (yh[1] - rho * yl[1]).abs()] if isinstance(yl, list) else yh - rho * yl
            loss = -m.negative_log_likelihood(x, y) if hasattr(m, "negative_log_likelihood") else (-m.log_likelihood(x, y)).sum()
            loss.backward()
            opt.step()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


print("SumKernel(LinearKernel(2), MaternKernel(2, nu = 2.5)), d = 1, %d Adam steps; ms per call: median [min .. max] of 3 alternating rounds" % steps)
for n, F, kind in ((32, 1, "residual"), (128, 1, "residual"), (128, 1, "residual_var"), (300, 1, "residual"), (64, 16, "residual"), (128, 1, "gpbasic")):
    a, b, c = make(n, F, kind), make(n, F, kind), make(n, F, kind)
    one = n <= 128
    _, st = fused(a, 5)
    assert st["fused"] is True and st["tree_one_launch"] == [], "the models were not trained by the launch-per-stage call"
    loop(b, 5)
    if one:
        _, st = fused(c, 5, True)
        assert st["tree_one_launch"] == list(range(F)), "the models did not take the one-launch route"
    t_many, t_loop, t_lds = [], [], []
    for _ in range(3):
        t_many.append(timed(lambda: fused(a, steps)))
        if one:
            t_lds.append(timed(lambda: fused(c, steps, True)))
        t_loop.append(timed(lambda: loop(b, steps)))
    t_many.sort(), t_loop.sort(), t_lds.sort()
    print("N=%4d F=%2d %-12s  train_many %8.2f [%8.2f .. %8.2f] (%.3f ms/step/model)   per-step loop %8.2f [%8.2f .. %8.2f] (%.3f)   x%.1f"
          % (n, F, kind, t_many[1], t_many[0], t_many[2], t_many[1] / steps / F, t_loop[1], t_loop[0], t_loop[2], t_loop[1] / steps / F,
             t_loop[1] / t_many[1]), flush=True)
    assert t_many[2] < t_loop[0], "train_many is not ahead of the per-step loop at N = %d, F = %d, %s" % (n, F, kind)
    if one:
        print("              one launch %8.2f [%8.2f .. %8.2f] (%.4f ms/step/model)   x%.1f against launch per stage, x%.1f against the loop"
              % (t_lds[1], t_lds[0], t_lds[2], t_lds[1] / steps / F, t_many[1] / t_lds[1], t_loop[1] / t_lds[1]), flush=True)
        assert t_lds[2] < t_loop[0], "the one-launch route is not ahead of the per-step loop at N = %d, F = %d, %s" % (n, F, kind)
