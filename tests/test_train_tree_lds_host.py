"""The one-launch trainer for SumKernel / ProductKernel models (ffgp_train_tree_lds_raw, train_many(..., tree_one_launch=True)) as far
as it can be checked without a GPU: the keyword, the export, and the fallback of models the fused calls cannot train."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

torch = pytest.importorskip("torch")


def test_tree_one_launch_is_a_keyword_of_train_many_and_off_by_default():
    from fidelityfusion_amd import train
    from fidelityfusion_amd.cigp_v10 import train_many
    par = inspect.signature(train_many).parameters
    assert "tree_one_launch" in par and par["tree_one_launch"].default is False
    assert train.TREE_ONE_LAUNCH_MAX_N <= 128


def test_export_is_declared_defined_and_bound():
    from fidelityfusion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ffgp.h")).read()
    assert re.search(r"\bint ffgp_train_tree_lds_raw\s*\(", hdr)
    assert "ffgp_train_tree_lds_raw" in _lib.EXPORTS
    assert _lib.EXPORTS["ffgp_train_tree_lds_raw"] == _lib.EXPORTS["ffgp_train_tree_raw"]      # exactly its parameter list
    so = os.path.join(ROOT, "fidelityfusion_amd", "libffgp.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT ffgp_train_tree_lds_raw\b", syms)


class _TorchGP(torch.nn.Module):
    """a CPU model in plain torch (the package's own modules evaluate on the GPU only): Sum(Linear, SE) + noise, the reference's loss sign"""

    def __init__(self):
        super().__init__()
        self.log_ls = torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))
        self.lin = torch.nn.Parameter(torch.tensor(0.5, dtype=torch.float64))
        self.log_beta = torch.nn.Parameter(torch.tensor(0.8, dtype=torch.float64))

    def negative_log_likelihood(self, x, y):
        z = x * torch.exp(-self.log_ls)
        K = torch.exp(-0.5 * torch.cdist(z, z) ** 2) + self.lin ** 2 * (x @ x.T) + (torch.exp(-self.log_beta) + 1e-6) * torch.eye(x.shape[0])
        L = torch.linalg.cholesky(K)
        a = torch.cholesky_solve(y, L)
        return -(0.5 * (y * a).sum() + torch.log(torch.diagonal(L)).sum() + 0.5 * x.shape[0] * np.log(2 * np.pi))


def test_cpu_models_keep_the_reference_loop_under_the_keyword():
    """no GPU needed: a model the fused calls cannot train runs the reference's loop, with or without the keyword, and reports no
    model on the one-launch route"""
    from fidelityfusion_amd.cigp_v10 import train_many
    rng = np.random.default_rng(0)
    x = torch.tensor(rng.uniform(-1.0, 1.0, (12, 2)))
    y = torch.sin(x.sum(1, keepdim=True))
    m, twin, plain = _TorchGP(), _TorchGP(), _TorchGP()
    trace, state = train_many([m], [x], [y], 3, lr=1e-2, tree_one_launch=True)
    assert state["fused"] is False and state["tree_one_launch"] == []
    trace_p, state_p = train_many([plain], [x], [y], 3, lr=1e-2)
    assert state_p["fused"] is False and state_p["tree_one_launch"] == [] and torch.equal(trace, trace_p)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-2)
    ref = []
    for _ in range(3):
        opt.zero_grad()
        loss = -twin.negative_log_likelihood(x, y)
        loss.backward()
        opt.step()
        ref.append(float(loss.detach()))
    assert np.array_equal(trace[0].numpy(), np.array(ref))
    for a, b in zip(m.parameters(), twin.parameters()):
        assert torch.equal(a, b)
