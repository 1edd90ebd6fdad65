"""Wide-output models (d > 16, n <= 128) through train_many three ways, in one run: the fused call (wide_one_launch=True:
ffgp_train_wide_raw, ONE launch for all steps; the time INCLUDES the compression of the targets -- Gram, eigendecomposition, the
factor's row blocks -- which runs once per call), the same train_many call without the keyword (ffgp_train_raw's launch-per-stage
form, what these models ran before), and the per-step loop through the drop-in modules with torch.optim.Adam.

Legs: plain models at (n, d) = (32, 1024), (100, 4096), (128, 1024); a residual member at (32, 1024) and, the kernel's largest case
(r = 256: sixteen column blocks, the two-stage eigensolver in the compression), at (128, 1024); sixteen (64, 256) models in one call.
Every tensor fp64 on cuda:0; wall time per call around a device synchronise, fresh models per repetition, one warm-up round, then
--reps rounds in which the three ways ALTERNATE (the host is shared: a drift hits them alike).  Reported per way: the median and
the spread (min .. max) of the rounds, and the number of rounds behind them (n).  The fused and the launch-per-stage call are timed in
every round.  The per-step loop is a 0.1 to 1 s window that no verdict rests on, so it is timed in the first two rounds only, and in
the sixteen-model leg in ONE: there its column is a single time (n = 1) and its "min .. max" carries no spread.
The rule (the one LDS_EIGH_MAX_N was set by): the fused call wins a shape when its SLOWEST round beats the launch-per-stage call's
FASTEST round -- a difference larger than the measured spread; the verdict is printed per leg.
Usage: python tools/train_wide_bench.py [--steps 200] [--reps 7] [--out profiles/train_wide_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def once(make, run):
    args = make()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(*args)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_wide_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_wide_bench: needs the GPU (a CPU run gives no time)")
    torch.set_default_dtype(torch.float64)
    import test_gpu_train_residual as TR
    import test_gpu_train_wide as TW
    from fidelityfusion_amd.cigp_v10 import train_many
    K = a.steps
    lines = ["wide-output models through train_many: %d Adam steps, lr 1e-2, %d alternating rounds after one warm-up round (%s)" % (
        K, a.reps, torch.cuda.get_device_name(0)),
        "ms per call: median (min .. max) n = rounds timed; fused = wide_one_launch=True, compression of the targets included", ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def plain(n, d, seed):
        return lambda: TW.make_plain((n, 3, d, "ard", False), seed)

    def leg(name, make, fused, staged, loop, loop_reps):
        ways = {"fused": fused, "staged": staged, "loop": loop}
        ts = {k: [] for k in ways}
        for rnd in range(a.reps + 1):
            for k, run in ways.items():
                if k == "loop" and rnd > loop_reps:
                    continue
                t = once(make, run)
                if rnd:
                    ts[k].append(t * 1e3)
        fmt = lambda v: "%9.3f (%8.3f .. %8.3f) n=%d" % (float(np.median(v)), min(v), max(v), len(v))
        win = max(ts["fused"]) < min(ts["staged"])
        say("%-34s %s  %s  %s  %5.1fx  %s" % (name, fmt(ts["fused"]), fmt(ts["staged"]), fmt(ts["loop"]),
                                              float(np.median(ts["staged"]) / np.median(ts["fused"])),
                                              "fused wins beyond the spread" if win else "NOT beyond the spread"))

    say("%-34s %-35s  %-35s  %-35s  %6s" % ("leg", "fused", "launch per stage", "per-step loop", "ratio"))
    one = lambda kw: (lambda m, x, y: train_many([m], [x], [y], K, lr=1e-2, **kw))
    for n, d in ((32, 1024), (100, 4096), (128, 1024)):
        leg("plain n = %d, d = %d" % (n, d), plain(n, d, 50 + n), one({"wide_one_launch": True}), one({}),
            lambda m, x, y: TW.plain_loop(m, x, y, K, 1e-2), 2)
    mkr = lambda: TR.make_residual(32, 2, 1024, "ard", "subset", 77)
    leg("residual n = 32, d = 1024", mkr, lambda m, x, r: train_many([m], [x], [None], K, lr=1e-2, residual=[r], wide_one_launch=True),
        lambda m, x, r: train_many([m], [x], [None], K, lr=1e-2, residual=[r]), lambda m, x, r: TR.reference_ar_loop(m, x, r, K, 1e-2), 2)
    # (not one of the shapes the rule is applied to: the kernel's largest case, r = 256 -- 16 column blocks -- after the two-stage eigensolver)
    mkr2 = lambda: TR.make_residual(128, 2, 1024, "ard", "subset", 78)
    leg("residual n = 128, d = 1024", mkr2, lambda m, x, r: train_many([m], [x], [None], K, lr=1e-2, residual=[r], wide_one_launch=True),
        lambda m, x, r: train_many([m], [x], [None], K, lr=1e-2, residual=[r]), lambda m, x, r: TR.reference_ar_loop(m, x, r, K, 1e-2), 2)
    mk16 = lambda: ([TW.make_plain((64, 3, 256, "ard", False), 900 + f) for f in range(16)],)
    many = lambda kw: (lambda it: train_many([i[0] for i in it], [i[1] for i in it], [i[2] for i in it], K, lr=1e-2, **kw))
    leg("sixteen models n = 64, d = 256", mk16, many({"wide_one_launch": True}), many({}),
        lambda it: [TW.plain_loop(m, x, y, K, 1e-2) for m, x, y in it], 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
