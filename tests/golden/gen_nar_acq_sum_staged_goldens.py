#!/usr/bin/env python3
"""Fixture of the reference's multi-fidelity acquisition loop on its NAR model with SumKernel(LinearKernel, MaternKernel) per fidelity
(FidelityFusion_Models/two_fidelity_models/NAR_NonlinearAR.py:23-26) at the sizes of NAR's own demo (FidelityFusion_Models/NAR.py:119-128):
gen_nar_acq_sum_goldens.py's recipe with NS = (300, 300, 250) training points per fidelity in place of (24, 17, 12) -- past the 256
points the one-launch chain kernel takes, where the staged call for composed-kernel chains (ffgp_acq_optimize_chain_tree_staged)
serves.  That generator asserts its own sizes, so this one has a main of its own, built from the same imported pieces: the data
manager, the loop, the seed, LOG_BETA, the kernels' parameters, the linear leaves' centres, the acquisition (UCB_MF = mean + 0.2 D var),
10 Adam steps at lr 0.01 from six start points per level with and without zero_grad(), and the twin check at 1e-11.  The reference is
imported read-only, in fp64 on the CPU; only data is written, as tests/golden/mf_acq_nar_sum_n300.npz, with the keys and layouts of
mf_acq_nar_sum.npz.  Run:

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg FFGP_REFERENCE=<reference checkout> python tests/golden/gen_nar_acq_sum_staged_goldens.py
"""
import os
import sys

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from gen_mf_acq_goldens import D, LOG_BETA, LR, Q, STEPS, TWIN_BOUND, TWIN_SCALE, rel      # noqa: E402  the radial fixtures' parameters
from gen_mf_acq_ar_sum_goldens import LIN_LS, LIN_SV, MAT_LS, MAT_SV                        # noqa: E402  the AR sum fixture's kernels
from gen_nar_acq_goldens import REF, DataManager, loop                                      # noqa: E402
from gen_nar_acq_sum_goldens import LIN_CENTER                                              # noqa: E402

NS = (300, 300, 250)


def main():
    if not REF or not os.path.isdir(os.path.join(REF, "FidelityFusion_Models")):
        sys.exit("set FFGP_REFERENCE to a checkout of the reference (the directory that holds FidelityFusion_Models/)")
    assert D == 2 and Q == 6
    from gen_goldens import _install_tensorly_stub      # the package's __init__ imports modules that import tensorly; NAR never calls it
    _install_tensorly_stub()
    sys.path.insert(0, REF)
    os.chdir("/tmp")      # keep any stray relative output away from the reference and the repository
    torch.set_default_dtype(torch.float64)
    import GaussianProcess.kernel as rk
    from FidelityFusion_Models.NAR import NAR
    # by file: the package's __init__ imports a module the reference does not ship
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_DMF_acq", os.path.join(REF, "MF_BayesianOptimization", "Discrete", "DMF_acq.py"))
    dmf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dmf)

    dims = [D + (1 if f else 0) for f in range(len(NS))]
    kernels = [rk.SumKernel(rk.LinearKernel(dims[f], LIN_LS[f], LIN_SV[f]), rk.MaternKernel(dims[f], MAT_LS[f], MAT_SV[f])) for f in range(len(NS))]
    model = NAR(len(NS), kernels)
    with torch.no_grad():
        for f in range(len(NS)):
            model.gpr_list[f].log_beta.fill_(LOG_BETA[f])
            model.gpr_list[f].kernel.kernel1.center.copy_(torch.tensor(LIN_CENTER[f]))
    model.requires_grad_(False)
    assert all(p.dtype == torch.float64 for p in model.parameters())
    assert all(model.gpr_list[f].kernel is kernels[f] and kernels[f].kernel2.nu == 2.5 and kernels[f].kernel2.rho == 1 for f in range(len(NS)))

    g = torch.Generator().manual_seed(20261019)
    rand = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    sets = []
    dm = DataManager(sets)
    for f, n in enumerate(NS):
        x = 2.0 * rand(n, D)
        if f == 0:
            sets.append((x, (torch.sin(2.0 * x.sum(1)) + 0.1 * randn(n)).reshape(n, 1)))
            continue
        # the set the trainer would have stored as 'concat-f': [x, the model's own mean of fidelity f - 1 at x], [y, y_var]
        with torch.no_grad():
            low = model(dm, x, f - 1)[0].reshape(n, 1)
        y = torch.sin(2.0 * x.sum(1)) + 0.3 * torch.cos((f + 2.0) * x.sum(1)) + 0.2 * x[:, 0] + 0.05 * randn(n)
        sets.append((torch.cat([x, low], dim=-1), [y.reshape(n, 1), 0.01 * rand(n, 1)]))
    starts = 2.0 * rand(len(NS), Q, D)

    mean_f = lambda x, s: model(dm, x, s)[0]
    var_f = lambda x, s: model(dm, x, s)[1].diag().reshape(-1, 1)
    acq = dmf.DiscreteAcquisitionFunction(mean_f, var_f, len(NS), D, None)

    out = {"lin_length_scale": LIN_LS, "lin_signal_variance": LIN_SV, "matern_length_scale": MAT_LS, "matern_signal_variance": MAT_SV,
           "matern_eps": [float(k.kernel2.eps) for k in kernels], "log_beta": LOG_BETA, "kappa": 0.2 * D, "lr": LR, "steps": STEPS, "X0": starts}
    for f, (x, y) in enumerate(sets):
        out["x_%d" % f], out["y_%d" % f] = x, (y[0] if isinstance(y, list) else y)
        out["lin_center_%d" % f] = LIN_CENTER[f]
    dist = 0.0
    for tag, zg in (("zg", True), ("acc", False)):
        traces, hists = [], []
        for s in range(len(NS)):
            t, h = loop(acq, s, starts[s], zg)
            tt, ht = loop(acq, s, starts[s] * TWIN_SCALE, zg)
            assert torch.isfinite(t).all() and torch.isfinite(h).all()
            dist = max(dist, rel(tt, t), rel(ht, h))
            traces.append(t)
            hists.append(h)
            print("%s level %d: acquisition sum %.6f -> %.6f, moved %.3e" % (tag, s, float(t[0].sum()), float(t[-1].sum()),
                                                                            float((h[-1] - h[0]).abs().max())))
        out["trace_" + tag], out["hist_" + tag] = torch.stack(traces), torch.stack(hists)
    assert abs(float(acq.beta) - 0.2 * D) < 1e-15
    assert dist <= TWIN_BOUND, "ill-conditioned trajectories (twin distance %.3g > %.0e)" % (dist, TWIN_BOUND)
    out["twin_distance"] = dist
    path = os.path.join(OUT, "mf_acq_nar_sum_n300.npz")
    np.savez_compressed(path, **{k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float64)
                                 for k, v in out.items()})
    print("wrote %s (%d bytes), twin distance %.2e" % (path, os.path.getsize(path), dist))


if __name__ == "__main__":
    main()
