#!/usr/bin/env python3
"""Fixture of the reference's multi-fidelity acquisition loop on its NAR model at the sizes of NAR's own demo
(FidelityFusion_Models/NAR.py:119-128): gen_nar_acq_goldens.py's recipe, unchanged, with NS = (300, 300, 250) training points per
fidelity in place of (24, 17, 12) -- past the 256 points the one-launch chain kernel takes, where the staged call
(ffgp_acq_optimize_chain_staged) serves.  The reference's `NAR` and `DiscreteAcquisitionFunction.UCB_MF`, the drivers' loop with and
without zero_grad(), the seed, the parameters, the start points' recipe and the twin check at 1e-11 are that generator's own code, run
from here; only data is written, as tests/golden/mf_acq_nar_n300.npz.  Run:

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg FFGP_REFERENCE=<reference checkout> python tests/golden/gen_nar_acq_staged_goldens.py
"""
import os
import shutil
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_nar_acq_goldens as G      # noqa: E402

NS = (300, 300, 250)


def main():
    G.NS = NS      # (the generator holds its own name for the AR fixture's sizes)
    with tempfile.TemporaryDirectory() as tmp:
        G.OUT = tmp      # where G.main() writes mf_acq_nar.npz; gen_goldens, which it imports, is found through HERE
        G.main()
        path = os.path.join(HERE, "mf_acq_nar_n300.npz")
        shutil.move(os.path.join(tmp, "mf_acq_nar.npz"), path)
    print("moved to %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
