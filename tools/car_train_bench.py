"""train_CAR's fidelities through train_many (GP_basic blocks, car=) against the per-step loop (CAR_ContinuousAutoRegression.py:116-142:
drop-in modules, the fidelity integral formed by torch on the host, autograd, torch.optim.Adam), and the yardsticks of the tests.

Legs (every tensor fp64, default dtype float32 -- fp32 Monte-Carlo draws, as the reference's demo has them; cuda:0; wall time per call
after one warm-up call, median of --reps; reported, not asserted):
  * one CAR fidelity at n = 32 and n = 128 (ONE launch for all steps) and the demo's three fidelities 300 / 300 / 250 (fidelity 0 a plain
    GP_basic, launch per stage), --steps Adam steps each, fused call against per-step loop;
  * sixteen n = 64 CAR models in one call against sixteen per-step loops;
  * the yardsticks of tests/test_gpu_train_gp_basic.py and tests/test_gpu_train_car.py, case by case: d0 = the distance of the two reference
    loops (GP_basic: per-step GPU loop against plain torch on the CPU; CAR: the per-step loop against the same loop with the samples widened
    to fp64) and the distance of the fused trajectory from the per-step loop, 40 steps.
Usage: python tools/car_train_bench.py [--steps 200] [--reps 3] [--out profiles/car_train_bench.txt]
"""
import argparse
import copy
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(make, run, reps):
    """median wall time of run(make()): every repetition trains fresh models"""
    ts = []
    for k in range(reps + 1):
        args = make()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(*args)
        torch.cuda.synchronize()
        if k:
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "car_train_bench.txt"))
    a = ap.parse_args()
    import test_gpu_train_car as TC
    import test_gpu_train_gp_basic as TB
    from fidelityfusion_amd.gp_basic import train_many
    K = a.steps
    lines = ["train_CAR through train_many against the per-step loop: %d Adam steps, lr 1e-2, median of %d calls (%s)" % (
        K, a.reps, torch.cuda.get_device_name(0)), ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def car_leg(name, shapes):
        """shapes: [(n, D, d)] CAR fidelities trained one call (fused) / one loop (per step) each, summed"""
        fused = loop = 0.0
        for j, (n, D, d) in enumerate(shapes):
            mk = lambda: TC.make_car(n, D, d, "ard", 40 + j)
            fused += timed(mk, lambda m, x, c: train_many([m], [x], [None], K, lr=1e-2, car=[c]), a.reps)
            loop += timed(mk, lambda m, x, c: TC.car_loop(m, x, c, K, 1e-2), a.reps)
        return name, fused, loop

    say("%-44s %12s %12s %8s" % ("leg", "fused ms", "per-step ms", "ratio"))
    rows = [car_leg("CAR fidelity n = 32 (one launch)", [(32, 1, 1)]), car_leg("CAR fidelity n = 128 (one launch)", [(128, 1, 1)])]
    # the demo: fidelity 0 plain on 300 points, fidelities 1 and 2 CAR on 300 / 250
    mk0 = lambda: TB.make_model(300, 1, 1, "ard", 7)
    f0 = timed(mk0, lambda m, x, y: train_many([m], [x], [y], K, lr=1e-2), a.reps)
    l0 = timed(mk0, lambda m, x, y: TB.gpu_loop(m, x, y, K, 1e-2), a.reps)
    _, f12, l12 = car_leg("", [(300, 1, 1), (250, 1, 1)])
    rows.append(("CAR demo 300 / 300 / 250 (launch per stage)", f0 + f12, l0 + l12))
    mk16 = lambda: ([TC.make_car(64, 1, 1, "ard", 900 + f) for f in range(16)],)
    f16 = timed(mk16, lambda it: train_many([i[0] for i in it], [i[1] for i in it], [None] * 16, K, lr=1e-2, car=[i[2] for i in it]), a.reps)
    l16 = timed(mk16, lambda it: [TC.car_loop(m, x, c, K, 1e-2) for m, x, c in it], max(1, a.reps // 2))
    rows.append(("sixteen CAR models n = 64 (one launch)", f16, l16))
    for name, f, l in rows:
        say("%-44s %12.3f %12.3f %8.1f" % (name, f * 1e3, l * 1e3, l / f))

    say("")
    say("yardsticks, 40 steps (25 + 15 continued): d0 = distance of the two reference loops, fused = fused trajectory against the per-step loop")
    torch.set_default_dtype(torch.float64)      # (the GP_basic tests' dtype)
    for n, D, d, kind in TB.CASES:
        m, x, y = TB.make_model(n, D, d, kind, 100 * n + D)
        twin = copy.deepcopy(m)
        A = TB.cpu_loop(m, kind, x, y, 40, 1e-2)
        t1, st = train_many([m], [x], [y], 25, lr=1e-2)
        t2, _ = train_many([m], [x], [y], 15, lr=1e-2, state=st)
        B = TB.gpu_loop(twin, x, y, 40, 1e-2)
        Fz = (torch.cat([t1, t2], dim=1).cpu().numpy()[0], TB.params_of(m))
        say("GP_basic n=%-4d D=%-3d d=%-3d %-7s d0 %.2e  fused %.2e" % (n, D, d, kind, TB.distance(B, A), TB.distance(Fz, B)))
    torch.set_default_dtype(torch.float32)
    for n, D, d, kind, neg, b0 in TC.CASES:
        m, x, car = TC.make_car(n, D, d, kind, 100 * n + D, neg, b0)
        twin, wide = copy.deepcopy(m), copy.deepcopy(m)
        t1, st = train_many([m], [x], [None], 25, lr=1e-2, car=[car])
        t2, _ = train_many([m], [x], [None], 15, lr=1e-2, state=st, car=[car])
        B = TC.car_loop(twin, x, (twin.kernel.b, car[1], car[2]), 40, 1e-2)
        W = TC.car_loop(wide, x, (wide.kernel.b, car[1], car[2]), 40, 1e-2, widen=True)
        Fz = (torch.cat([t1, t2], dim=1).cpu().numpy()[0], TC.params_of(m))
        say("CAR      n=%-4d D=%-3d d=%-3d %-7s neg=%-5s b=%-4.1f d0 %.2e  fused %.2e" % (n, D, d, kind, neg, b0, TC.distance(B, W),
                                                                                          TC.distance(Fz, B)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
