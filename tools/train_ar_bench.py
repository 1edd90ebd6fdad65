"""train_AR's residual fidelities through train_many(..., residual=) against the reference's loop (AR_autoRegression.py:123-137).

Legs (fp64, cuda:0; wall time per call after one warm-up call, median of --reps):
  * exp_aligned's AR fidelity 1 (Experiments/GAR_Aligned/exp_aligned.py:56-102: D = 2, d = 1, N_high 4/8/16/32, 300 steps, lr 1e-2):
    one model per call, and all 20 (5 seeds x 4 sizes) in ONE call;
  * N = 45 (the ar_chain fixture's size) and N = 180 (the demo's larger overlaps: the launch-per-stage loop);
  * a plain model of the same shape per residual leg (the residual overhead per step);
  * the reference loop: drop-in modules + torch.optim.Adam over the GP parameters and rho, the residual recomputed every step.
Usage: python tools/train_ar_bench.py [--steps 300] [--reps 5] [--ref-steps 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def residual_problem(n, D, seed, dev):
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.cigp_v10 import cigp
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (n, D))
    yl = np.sin(3 * x[:, :1]) + 0.1 * rng.standard_normal((n, 1))
    yh = 1.3 * yl + 0.2 * np.cos(2 * x[:, :1]) + 0.05 * rng.standard_normal((n, 1))
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)
    m = cigp(kernel.SquaredExponentialKernel(), 1.0).double().to(dev)
    rho = torch.nn.Parameter(torch.tensor(1.0, dtype=torch.float64, device=dev))
    vl, vh = rng.uniform(0.0, 0.05, n), rng.uniform(0.0, 0.05, n)
    return m, t(x), (rho, [t(yl), torch.diag(t(vl))], [t(yh), torch.diag(t(vh))])


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-steps", type=int, default=50)
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    from fidelityfusion_amd.cigp_v10 import train_many
    dev = torch.device("cuda:0")
    K = a.steps
    out = []

    def leg(name, **kw):
        kw["name"] = name
        print(json.dumps(kw), flush=True)
        out.append(kw)

    for n in (4, 8, 16, 32, 45, 180):
        D = 2
        m, x, res = residual_problem(n, D, 10 + n, dev)
        ms_res = timed(lambda: train_many([m], [x], [None], K, lr=1e-2, residual=[res]), a.reps) * 1e3
        mp, xp, resp = residual_problem(n, D, 10 + n, dev)
        yp = [resp[2][0] - 1.0 * resp[1][0], (resp[2][1] - resp[1][1]).abs()]
        ms_plain = timed(lambda: train_many([mp], [xp], [yp], K, lr=1e-2), a.reps) * 1e3
        leg("residual_one_model", n=n, D=D, d=1, steps=K, ms_per_call=round(ms_res, 4), us_per_step=round(ms_res * 1e3 / K, 3),
            plain_us_per_step=round(ms_plain * 1e3 / K, 3), residual_over_plain=round(ms_res / ms_plain, 4),
            path="one launch" if n <= 128 else "launch per stage")
    items = [residual_problem(nh, 2, 1000 * s + nh, dev) for s in range(5) for nh in (4, 8, 16, 32)]
    ms20 = timed(lambda: train_many([i[0] for i in items], [i[1] for i in items], [None] * 20, K, lr=1e-2,
                                    residual=[i[2] for i in items]), a.reps) * 1e3
    leg("exp_aligned_20_models_one_call", models=20, steps=K, ms_per_call=round(ms20, 4), us_per_step=round(ms20 * 1e3 / K, 3))
    # the reference loop: drop-in modules, torch.optim.Adam over the GP parameters and rho, residual recomputed every step
    for n in (32, 45, 180):
        m, x, res = residual_problem(n, 2, 10 + n, dev)
        rho, yl, yh = res
        opt = torch.optim.Adam(list(m.parameters()) + [rho], lr=1e-2)

        def ref_loop():
            for _ in range(a.ref_steps):
                opt.zero_grad()
                y = [yh[0] - rho * yl[0], (yh[1] - rho * yl[1]).abs()]
                loss = -m.negative_log_likelihood(x, y)
                loss.backward()
                opt.step()
        ms = timed(ref_loop, max(1, a.reps // 2)) * 1e3
        leg("reference_loop", n=n, D=2, d=1, steps=a.ref_steps, ms_per_call=round(ms, 4), us_per_step=round(ms * 1e3 / a.ref_steps, 3),
            ms_per_300_steps=round(ms * 300 / a.ref_steps, 3))


if __name__ == "__main__":
    main()
