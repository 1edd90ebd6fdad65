"""Residual and `GP_basic` members on composed kernels in train_many (ffgp_train_tree_res_raw, train_many(..., fuse_composed=True)) as
far as they can be checked without a GPU: the keyword, the export, the eligibility rules and the fallback to the reference's loop."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_train_tree_lds_host import _TorchGP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

torch = pytest.importorskip("torch")


def test_fuse_composed_is_a_keyword_of_train_many_and_off_by_default():
    from fidelityfusion_amd import gp_basic
    from fidelityfusion_amd.cigp_v10 import train_many
    par = inspect.signature(train_many).parameters
    assert "fuse_composed" in par and par["fuse_composed"].default is False
    assert gp_basic.train_many is train_many      # a GP_basic's train_many takes the keyword too


def test_export_is_declared_defined_and_bound():
    from fidelityfusion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ffgp.h")).read()
    assert re.search(r"\bint ffgp_train_tree_res_raw\s*\(", hdr)
    # ffgp_train_tree_raw's parameter list with the residual members behind the links, as ffgp_train_residual_raw has them
    tree, res = _lib.EXPORTS["ffgp_train_tree_raw"], _lib.EXPORTS["ffgp_train_tree_res_raw"]
    assert res[0] is tree[0] and res[1][:4] == tree[1][:4] and res[1][5:] == tree[1][4:]
    assert res[1][4] is _lib.EXPORTS["ffgp_train_residual_raw"][1][4]
    so = os.path.join(ROOT, "fidelityfusion_amd", "libffgp.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT ffgp_train_tree_res_raw\b", syms)
    exports = open(os.path.join(ROOT, "fidelityfusion_amd", "csrc", "exports.map")).read()
    assert "ffgp_train_tree_res_raw;" in exports
    # ... and the one-launch form: the same parameter list
    assert re.search(r"\bint ffgp_train_tree_lds_res_raw\s*\(", hdr) and _lib.EXPORTS["ffgp_train_tree_lds_res_raw"] == res
    assert re.search(r"\bT ffgp_train_tree_lds_res_raw\b", syms) and "ffgp_train_tree_lds_res_raw;" in exports


def test_cpu_models_keep_the_reference_loop_under_the_keyword():
    """a residual model the fused calls cannot train runs the reference's loop with or without the keyword: the same trace, rho and
    parameters, bit for bit, and train_AR's loop restated here"""
    from fidelityfusion_amd.cigp_v10 import train_many
    rng = np.random.default_rng(0)
    x = torch.tensor(rng.uniform(-1.0, 1.0, (12, 2)))
    yl = torch.sin(x.sum(1, keepdim=True))
    yh = 1.2 * yl + 0.1 * torch.cos(x[:, :1])
    runs = []
    for kw in (dict(fuse_composed=True), dict()):
        m = _TorchGP()
        rho = torch.nn.Parameter(torch.tensor(1.0, dtype=torch.float64))
        trace, state = train_many([m], [x], [None], 3, lr=1e-2, residual=[(rho, yl, yh)], **kw)
        assert state["fused"] is False and state["tree_one_launch"] == []
        assert torch.equal(state["residual_targets"][0][0], yh - runs[0][3] * yl) if runs else True
        runs.append((trace, [p.detach().clone() for p in m.parameters()], rho.detach().clone(), None))
        if len(runs) == 1:      # the rho of the start of the last step: from the restated loop below
            twin, trho = _TorchGP(), torch.nn.Parameter(torch.tensor(1.0, dtype=torch.float64))
            opt = torch.optim.Adam(list(twin.parameters()) + [trho], lr=1e-2)
            ref, last = [], None
            for _ in range(3):
                opt.zero_grad()
                last = trho.detach().clone()
                loss = -twin.negative_log_likelihood(x, yh - trho * yl)
                loss.backward()
                opt.step()
                ref.append(float(loss.detach()))
            assert np.array_equal(trace[0].numpy(), np.array(ref)) and torch.equal(rho.detach(), trho.detach())
            assert torch.equal(state["residual_targets"][0][0], yh - last * yl)
            runs[0] = runs[0][:3] + (last,)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def _gp_basic_sum(D):
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.gp_basic import GP_basic
    return GP_basic(kernel.SumKernel(kernel.LinearKernel(D), kernel.MaternKernel(D)), 1.0).double()


def test_gp_basic_over_a_composed_kernel_is_eligible_only_under_the_keyword_and_never_with_a_list_y(monkeypatch):
    """the eligibility rules on the module structure alone (the device test of functional.raw_ok is stubbed out: no GPU here): a
    `GP_basic` over Sum(Linear, Matern) is a tree member under the keyword -- noise_variance under the square link, c = 0, FFGP_LL_V2,
    pi = math.pi -- and the reference's loop without it, or with y = [y, y_var] (the FULL matrix enters Sigma)"""
    import math
    from fidelityfusion_amd import _lib, functional as F, train
    monkeypatch.setattr(F, "raw_ok", lambda *a: True)
    m = _gp_basic_sum(2)
    x, y = torch.rand(9, 2, dtype=torch.float64), torch.rand(9, 1, dtype=torch.float64)
    assert train._eligible(m, x, y) is None
    e = train._eligible(m, x, y, True)
    assert e is not None and train._is_tree(e)
    assert e[0]["diag"][0] is m.noise_variance and e[0]["diag"][1:] == (_lib.LINK_SQUARE, 0.0)
    assert e[0]["ll"] == (_lib.FFGP_LL_V2, math.pi)
    assert train._eligible(m, x, [y, torch.eye(9, dtype=torch.float64)], True) is None
    m.kernel.kernel1.center.requires_grad_(False)      # `_eligible_tree`'s rules: every leaf parameter trainable
    assert train._eligible(m, x, y, True) is None


def test_gp_basic_with_a_list_y_stays_on_the_loop(monkeypatch):
    """train_many itself: state["fused"] False for a `GP_basic` given [y, y_var], keyword or not (the loop body is stubbed: the drop-in
    modules evaluate on the GPU only)"""
    from fidelityfusion_amd import functional as F, train
    monkeypatch.setattr(F, "raw_ok", lambda *a: True)
    seen = []
    monkeypatch.setattr(train, "_reference_loop", lambda models, xs, ys, steps, *a, **k: seen.append(ys) or torch.zeros(len(models), steps, dtype=torch.float64))
    m = _gp_basic_sum(2)
    x, y = torch.rand(9, 2, dtype=torch.float64), torch.rand(9, 1, dtype=torch.float64)
    for kw in (dict(fuse_composed=True), dict()):
        _, state = train.train_many([m], [x], [[y, torch.eye(9, dtype=torch.float64)]], 2, **kw)
        assert state["fused"] is False
    assert len(seen) == 2


def test_gp_basic_with_residual_variances_stays_on_the_loop(monkeypatch):
    """a `GP_basic` over a tree with a NON-subset link: |v_high - rho v_low| is a full matrix in its Sigma, so the reference's loop keeps
    it under the keyword too (a `cigp` takes the matrix's diagonal and is fused: tests/test_gpu_train_tree_residual.py)"""
    from fidelityfusion_amd import functional as F, train
    monkeypatch.setattr(F, "raw_ok", lambda *a: True)
    monkeypatch.setattr(train, "_reference_loop", lambda models, xs, ys, steps, *a, **k: torch.zeros(len(models), steps, dtype=torch.float64))
    m = _gp_basic_sum(2)
    x, yl, yh = (torch.rand(9, k, dtype=torch.float64) for k in (2, 1, 1))
    v = torch.eye(9, dtype=torch.float64)
    rho = torch.nn.Parameter(torch.tensor(1.0, dtype=torch.float64))
    _, state = train.train_many([m], [x], [None], 2, residual=[(rho, [yl, 0.1 * v], [yh, 0.2 * v])], fuse_composed=True)
    assert state["fused"] is False
