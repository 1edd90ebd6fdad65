#!/usr/bin/env python3
"""Fixtures of the reference's acquisition loops on its composed-kernel models at the sizes of its own demos, past the 256 training
points the one-launch acquisition kernels take, where the staged call for composed kernels (ffgp_acq_optimize_stack_tree_staged) serves:

    gen_acq_tree_goldens.py's recipe, unchanged, with N = 300 in place of 24: the reference's `cigp` on
        SumKernel(LinearKernel(1), MaternKernel(1)) under its `UCB` / `EI` and its loop   -> tests/golden/acq_tree_cigp_n300.npz
    gen_mf_acq_ar_sum_goldens.py's recipe, unchanged, with NS = (300, 300, 250) in place of (24, 17, 12): the reference's `AR` on
        Sum(Linear, Matern) fidelities under `UCB_MF` and the drivers' loop               -> tests/golden/mf_acq_ar_sum_n300.npz

The models, the acquisition classes, the loops, the seeds, the parameters, the start points' recipes and the twin checks at 1e-11 are those
generators' own code, run from here; only data is written.  Run:

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg FFGP_REFERENCE=<reference checkout> python tests/golden/gen_acq_staged_tree_goldens.py
"""
import os
import shutil
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_acq_tree_goldens as G1            # noqa: E402
import gen_mf_acq_ar_sum_goldens as G2       # noqa: E402

N = 300
NS = (300, 300, 250)


def run(G, written, name):
    """G.main() into a temporary directory (gen_goldens, which the generators import, is found through HERE), its file moved here"""
    with tempfile.TemporaryDirectory() as tmp:
        G.OUT = tmp
        G.main()
        path = os.path.join(HERE, name)
        shutil.move(os.path.join(tmp, written), path)
    print("moved to %s (%d bytes)" % (path, os.path.getsize(path)))


def main():
    G1.N = N
    run(G1, "acq_tree_cigp.npz", "acq_tree_cigp_n300.npz")
    G2.NS = NS
    run(G2, "mf_acq_ar_sum.npz", "mf_acq_ar_sum_n300.npz")


if __name__ == "__main__":
    main()
