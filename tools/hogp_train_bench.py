"""HOGP blocks through hogp_simple.train_many (ffgp_train_hogp_raw: K Adam steps per library call) against the per-step loop of
train_GAR (GAR.py:76-126 on the drop-in modules: log_likelihood, the closed-form backward of _KronNLL, autograd through the kernel,
torch.optim.Adam, one Python round trip per step) -- the parent path, timed in the same process.

Legs (fp64, cuda:0; wall time per call after one warm-up call, every repetition on fresh models; median and spread = (max - min) of
--reps repetitions; reported, and the verdict "faster by more than the spread" printed per leg):
  * one block at (n, shape) = (32, 8x8), (100, 8x8), (128, 16x16), (16, 8x8), --steps Adam steps;
  * four n = 32 blocks in one call against four per-step loops;
  * the per-stage split of ONE fused step (assembly + links, eigensolver, forward, backward, chain rule + Adam) from the handle's stage
    events (option "timing"), per size -- what a warm-started Jacobi or a persistent kernel would have to beat.
Usage: python tools/hogp_train_bench.py [--steps 200] [--reps 5] [--out profiles/hogp_train_bench.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = torch.device("cuda", 0)
STAGES = ("assembly + links", "eigensolver", "forward", "backward", "chain rule + Adam")


def make(n, shape, seed):
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.hogp_simple import HOGP_simple
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((n, 2), generator=g, dtype=torch.float64)
    y = torch.sin(3.0 * x.sum(1)).reshape((n,) + (1,) * len(shape)) * torch.ones(shape, dtype=torch.float64)
    for ax, d in enumerate(shape):
        y = y * torch.cos(0.4 * torch.arange(d, dtype=torch.float64)).reshape((1,) * (ax + 1) + (d,) + (1,) * (len(shape) - ax - 1))
    y = y + 0.05 * torch.randn((n,) + tuple(shape), generator=g, dtype=torch.float64)
    m = HOGP_simple(kernel.ARDKernel(2), 0.5, shape).double().to(DEV)
    return m, x.to(DEV), y.to(DEV)


def per_step(m, x, y, steps, lr):
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    for _ in range(steps):
        opt.zero_grad()
        loss = m.log_likelihood(x, y)
        float(loss.detach())                     # (train_GAR prints / records the loss of every step)
        loss.backward()
        opt.step()


def timed(mk, run, reps):
    ts = []
    for k in range(reps + 1):
        args = mk()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(*args)
        torch.cuda.synchronize()
        if k:
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(max(ts) - min(ts))


def stage_split(n, shape):
    """milliseconds per stage of the last step of a 3-step fused call, from the handle's events"""
    from fidelityfusion_amd import _lib
    from fidelityfusion_amd.hogp_simple import train_many
    m, x, y = make(n, shape, 5)
    train_many([m], [x], [y], 3)                 # warm-up
    _lib.set_option("timing", 1, DEV.index)
    try:
        train_many([m], [x], [y], 3)
        ms, cnt = (C.c_float * 16)(), C.c_int(0)
        _lib.check(_lib.lib.ffgp_last_timings(_lib.handle(DEV.index), ms, None, 16, C.byref(cnt)), "ffgp_last_timings")
    finally:
        _lib.set_option("timing", 0, DEV.index)
    return [float(ms[i]) for i in range(min(cnt.value, len(STAGES)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hogp_train_bench.txt"))
    a = ap.parse_args()
    from fidelityfusion_amd.hogp_simple import train_many
    K, lr = a.steps, 1e-2
    lines = ["HOGP blocks through hogp_simple.train_many against the per-step loop: %d Adam steps, lr 1e-2, median (spread = max - min) of "
             "%d calls (%s)" % (K, a.reps, torch.cuda.get_device_name(0)), ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("%-34s %12s %10s %13s %10s %7s  %s" % ("leg", "fused ms", "spread", "per-step ms", "spread", "ratio", "faster by more than the spread"))
    sizes = [(32, (8, 8)), (100, (8, 8)), (128, (16, 16)), (16, (8, 8))]
    for n, shape in sizes:
        mk = lambda: make(n, shape, 11 + n)
        f, fs = timed(mk, lambda m, x, y: train_many([m], [x], [y], K, lr=lr), a.reps)
        l, ls = timed(mk, lambda m, x, y: per_step(m, x, y, K, lr), a.reps)
        say("%-34s %12.3f %10.3f %13.3f %10.3f %7.1f  %s" % ("n = %d, %s" % (n, "x".join(map(str, shape))), f * 1e3, fs * 1e3, l * 1e3, ls * 1e3,
                                                           l / f, "yes" if l - f > fs + ls else "NO"))
    mk4 = lambda: ([make(32, (8, 8), 300 + j) for j in range(4)],)
    f, fs = timed(mk4, lambda it: train_many([i[0] for i in it], [i[1] for i in it], [i[2] for i in it], K, lr=lr), a.reps)
    l, ls = timed(mk4, lambda it: [per_step(m, x, y, K, lr) for m, x, y in it], a.reps)
    say("%-34s %12.3f %10.3f %13.3f %10.3f %7.1f  %s" % ("four n = 32, 8x8 in one call", f * 1e3, fs * 1e3, l * 1e3, ls * 1e3, l / f,
                                                       "yes" if l - f > fs + ls else "NO"))
    say("")
    say("one fused step by stage, microseconds (events on the stream around the stages of the last step of a 3-step call)")
    say("%-20s " % "size" + " ".join("%18s" % s for s in STAGES) + " %10s" % "sum")
    for n, shape in sizes:
        ms = stage_split(n, shape)
        say("%-20s " % ("n = %d, %s" % (n, "x".join(map(str, shape)))) + " ".join("%18.1f" % (v * 1e3) for v in ms) + " %10.1f" % (sum(ms) * 1e3))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
