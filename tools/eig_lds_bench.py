"""The one-workgroup LDS eigensolver (ffgp_syev_lds, csrc/eig_lds.hip) against the routes it can replace, both in this process,
alternating, after a warm-up of either; every timing ends in a device synchronise.  Per row: median [min .. max] and the
interquartile range (the "spread") over REPS repetitions.

  (i)  functional._syev_lds on a batch of SE kernel matrices (D = 3, ls 0.7) against eigh.eigh (the two-stage ffgp_syevd, called
       once per matrix: it has no batch) at n = 65, 100, 128, batch 1 and 16
  (ii) HOGP_simple.log_likelihood + backward() at N = 32 and N = 100, modes 8 x 8, D = 2, with hogp_simple.LDS_EIGH_MAX_N = 128
       against 64 (64 is the routing without the LDS solver: every n > 64 goes to ffgp_syevd).  N = 32 takes neither route
       (ffgp_syevj_small serves it): the row shows what the harness itself resolves.

The last line states what the default of LDS_EIGH_MAX_N should be by the rule in README.md: 128 only if the N = 100 step is faster
with it by more than the larger of the two spreads.
      python tools/eig_lds_bench.py [out file, default profiles/eig_lds_bench.txt]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from fidelityfusion_amd import eigh as E
from fidelityfusion_amd import functional as F
from fidelityfusion_amd import hogp_simple, kernel

dev = torch.device("cuda", 0)
torch.set_default_dtype(torch.float64)
REPS, WARM = 25, 5


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(fns):
    """REPS timings [ms] of every callable, taken in turn after WARM untimed rounds of all of them"""
    for _ in range(WARM):
        for fn in fns:
            timed(fn)
    ts = [[] for _ in fns]
    for _ in range(REPS):
        for i, fn in enumerate(fns):
            ts[i].append(timed(fn))
    return ts


def stats(t):
    q = statistics.quantiles(t, n=4)
    return statistics.median(t), min(t), max(t), q[2] - q[0]


def fmt(t):
    return "%8.3f [%8.3f .. %8.3f] iqr %6.3f" % stats(t)


def kernel_matrices(n, batch):
    g = torch.Generator().manual_seed(n)
    X = torch.rand(batch, n, 3, generator=g)
    d = torch.cdist(X / 0.7, X / 0.7)
    return torch.exp(-0.5 * d * d).to(dev)


def main(out_path):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# %s, %d repetitions per row after %d warm-up rounds, alternating; times in ms: median [min .. max] iqr" %
        (torch.cuda.get_device_name(0), REPS, WARM))
    say("# (i) eigendecomposition of SE kernel matrices: ffgp_syev_lds (one launch per batch) | eigh.eigh = ffgp_syevd (one call per matrix)")
    for n in (65, 100, 128):
        for batch in (1, 16):
            M = kernel_matrices(n, batch)
            ev, Q, info = F._syev_lds(M, info=True)
            assert int(info.abs().max()) == 0
            t_new, t_old = alternate([lambda: F._syev_lds(M), lambda: [E.eigh(M[b]) for b in range(batch)]])
            say("n %3d batch %2d   syev_lds %s   | syevd %s   | ratio of medians %.2f" %
                (n, batch, fmt(t_new), fmt(t_old), stats(t_old)[0] / stats(t_new)[0]))
    say("# (ii) HOGP_simple.log_likelihood + backward, modes 8 x 8, D = 2: LDS_EIGH_MAX_N = 128 | = 64")
    verdict = None
    own = hogp_simple.LDS_EIGH_MAX_N
    try:
        for N in (32, 100):
            g = torch.Generator().manual_seed(N)
            X = torch.rand(N, 2, generator=g).to(dev)
            Y = torch.randn(N, 8, 8, generator=g).to(dev)
            m = hogp_simple.HOGP_simple(kernel.ARDKernel(2), 0.7, [8, 8]).double().to(dev)

            def step(cap):
                hogp_simple.LDS_EIGH_MAX_N = cap
                m.zero_grad(set_to_none=True)
                m.log_likelihood(X, Y).backward()
            t_new, t_old = alternate([lambda: step(128), lambda: step(64)])
            s_new, s_old = stats(t_new), stats(t_old)
            say("N %3d   128: %s   | 64: %s   | ratio of medians %.2f" % (N, fmt(t_new), fmt(t_old), s_old[0] / s_new[0]))
            if N == 100:
                verdict = (s_old[0] - s_new[0], max(s_new[3], s_old[3]))
    finally:
        hogp_simple.LDS_EIGH_MAX_N = own
    gain, spread = verdict
    say("# N = 100 step: the LDS route is %.3f ms %s per step; larger spread %.3f ms -> default LDS_EIGH_MAX_N = %d" %
        (abs(gain), "faster" if gain > 0 else "slower", spread, 128 if gain > spread else 64))
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "eig_lds_bench.txt"))
