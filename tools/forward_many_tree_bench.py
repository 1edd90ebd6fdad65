"""`cigp_v10.forward_many_composed` (ffgp_predict_small_tree_batch: every Sum / Product-kernel model factored in LDS and predicted in ONE
launch) against the per-model loop `[m.forward(x, y, x_test) for m ...]` with the covariance's diagonal taken -- what `forward_many`
runs for such members.  A sweep predicts every trained model ONCE, so the loop's models refactorise on every call
(`cache_posterior = False`, what the reference does, cigp_v10.py:31-35).  Beside it, reported only: `forward_many` on SE (ARD) members of
the same sizes in the same run, and the ratio of the two one-launch calls.

Cases (fp64, cuda:0, Sum(Linear, Matern-5/2), D = 2, d = 1): sixteen (n = 64, nt = 100); sixteen (n = 128, nt = 100); two (n = 100 and
32, nt = 100: exp_aligned's pair of fidelities); one (n = 128, nt = 1000).
Method: one process; after a warm-up of each leg, --rounds rounds in which the legs ALTERNATE; a round times --inner consecutive calls of
a leg between two device synchronisations (a host clock around work that ends in a synchronise) and reports the time per call;
median [min .. max] over the rounds.  Gated statement (asserted, multi-model cases): forward_many_composed's slowest round beats the
loop's fastest.  The single-model case is reported only.
Usage: python tools/forward_many_tree_bench.py [--rounds 7] [--inner 20] [--out profiles/forward_many_tree_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("sixteen models n = 64, nt = 100", [64] * 16, 100, True),
         ("sixteen models n = 128, nt = 100", [128] * 16, 100, True),
         ("two models n = 100 / 32, nt = 100 (exp_aligned)", [100, 32], 100, True),
         ("one model n = 128, nt = 1000", [128], 1000, False)]


def make(ns, nt, seed, dev, composed):
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.cigp_v10 import cigp
    g = torch.Generator().manual_seed(seed)
    ms, xs, ys, xts = [], [], [], []
    for n in ns:
        x = torch.rand(n, 2, generator=g, dtype=torch.float64)
        y = torch.sin(3.0 * x.sum(1, keepdim=True)) + 0.05 * torch.randn(n, 1, generator=g, dtype=torch.float64)
        k = kernel.SumKernel(kernel.LinearKernel(2), kernel.MaternKernel(2)) if composed else kernel.ARDKernel(2)
        ms.append(cigp(k, 3.0).double().to(dev))
        xs.append(x.to(dev))
        ys.append(y.to(dev))
        xts.append(torch.rand(nt, 2, generator=g, dtype=torch.float64).to(dev))
    return ms, xs, ys, xts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forward_many_tree_bench.txt"))
    a = ap.parse_args()
    assert a.rounds >= 5
    from fidelityfusion_amd.cigp_v10 import forward_many, forward_many_composed
    torch.set_default_dtype(torch.float64)
    dev = torch.device("cuda", 0)
    lines = ["forward_many_composed on Sum(Linear, Matern-5/2) against the per-model loop: ms per call, median [min .. max] of %d alternating "
             "rounds of %d calls each, after a warm-up of each leg (%s)" % (a.rounds, a.inner, torch.cuda.get_device_name(0)), ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def loop(ms, xs, ys, xts):
        with torch.no_grad():
            out = []
            for m, x, y, xt in zip(ms, xs, ys, xts):
                mean, cov = m(x, y, xt)
                out.append((mean, cov.diagonal().reshape(-1, 1)))
            return out

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.inner):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.inner * 1e3

    fmt = lambda ts: "%8.3f [%8.3f .. %8.3f]" % (float(np.median(ts)), min(ts), max(ts))
    say("%-50s %-32s %-32s %-32s %-20s %s" % ("case", "forward_many_composed", "loop, fresh factor per call", "forward_many, SE members",
                                              "loop / composed", "composed / SE (reported only)"))
    failed = []
    for k, (name, ns, nt, gated) in enumerate(CASES):
        fresh = make(ns, nt, 100 + k, dev, True)
        radial = make(ns, nt, 100 + k, dev, False)
        for m in fresh[0]:
            m.cache_posterior = False
        st = {}
        forward_many_composed(*fresh, st)
        assert st["fused_composed"] == list(range(len(ns))), st      # (the leg measures the one launch, not a fall-back)
        legs = {"composed": lambda: forward_many_composed(*fresh), "fresh": lambda: loop(*fresh), "se": lambda: forward_many(*radial)}
        # the two routes agree on these very inputs (the tests hold them to a measured bar; here: a plain sanity bound)
        got, want = legs["composed"](), legs["fresh"]()
        err = max(float((g[j] - w[j]).abs().max() / w[j].abs().max()) for g, w in zip(got, want) for j in (0, 1))
        assert err < 1e-9, (name, err)
        for fn in legs.values():      # warm-up of each leg
            clock(fn)
        ts = {key: [] for key in legs}
        for _ in range(a.rounds):
            for key, fn in legs.items():
                ts[key].append(clock(fn))
        ok = max(ts["composed"]) < min(ts["fresh"])
        med = {key: float(np.median(v)) for key, v in ts.items()}
        say("%-50s %-32s %-32s %-32s %-20s %6.2f x" % (name, fmt(ts["composed"]), fmt(ts["fresh"]), fmt(ts["se"]),
                                                       "%6.1f x%s" % (med["fresh"] / med["composed"], "" if gated else " (reported)"),
                                                       med["composed"] / med["se"]))
        if gated and not ok:
            failed.append(name)
    say("")
    say("gated: at the multi-model cases forward_many_composed's slowest round beats the fresh-factor loop's fastest: %s"
        % ("FAILED for %s" % failed if failed else "holds"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert not failed, failed


if __name__ == "__main__":
    main()
