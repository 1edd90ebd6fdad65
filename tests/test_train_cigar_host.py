"""Build-time and closed-form checks of the tensor-linear trainer (no GPU needed): the gradient ffgp_train_tlin_raw forms for the map's
matrix against autograd on the torch-CPU restatement of the likelihood, the C surface, and the register file of the new one-launch
instantiations of csrc/train.hip."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,l,h", [(4, 1, 1), (17, 6, 9), (32, 16, 16), (40, 40, 64)])
def test_dloss_dV_is_minus_A_transposed_y_low(n, l, h):
    """loss = -cigp_ll(X, y_high - y_low V^T + diag extra): dloss/dV = -A^T y_low with A = Sigma^-1 R, and the diagonal extra
    |diag(v_high) - diag(v_low)| has no V dependence.  1e-12 relative: both sides are fp64 evaluations of one function, and a wrong sign
    or a transposed V is O(1)."""
    from oracle import torch_cpu_ref as R
    rng = np.random.default_rng(1000 * n + l)
    D = 3
    tt = lambda a: torch.tensor(a, dtype=torch.float64)
    X, yl, yh = tt(rng.uniform(0, 1, (n, D))), tt(rng.standard_normal((n, l))), tt(rng.standard_normal((n, h)))
    ls, sv, lb = tt(rng.uniform(0.6, 1.6, D)), tt([1.3]), tt([0.6])
    dvec = (tt(rng.uniform(0, 0.3, n)) - tt(rng.uniform(0, 0.3, n))).abs()
    V = tt(rng.standard_normal((h, l))).requires_grad_(True)

    def loss_of(V_):
        # oracle.torch_cpu_ref.cigp_ll's operator sequence, with the diagonal extra in Sigma (cigp_v10.py:59-60)
        ell = ls.abs() + R.EPS
        K = sv.abs() * torch.exp(-0.5 * torch.cdist(X / ell, X / ell, p=2) ** 2)
        Sigma = K + (lb.exp().pow(-1) + R.JITTER) * torch.eye(n, dtype=torch.float64) + torch.diag(dvec)
        L = torch.linalg.cholesky(Sigma)
        Rm = yh - yl @ V_.T
        Gamma = torch.linalg.solve_triangular(L, Rm, upper=False)
        nll = 0.5 * (Gamma ** 2).sum() + L.diag().log().sum() * h + 0.5 * n * h * torch.log(2 * torch.tensor(R.PI_TRUNC, dtype=torch.float64))
        return nll, Sigma, Rm

    loss, Sigma, Rm = loss_of(V)
    loss.backward()
    with torch.no_grad():
        A = torch.linalg.solve(Sigma, Rm)
        closed = -(A.T @ yl)
    assert float((V.grad - closed).abs().max() / closed.abs().max()) < 1e-12
    # the value is the oracle's own when there is no extra: -cigp_ll on the residual
    with torch.no_grad():
        dvec0 = dvec.clone()
        dvec.zero_()
        assert abs(float(loss_of(V)[0]) + float(R.cigp_ll(X, yh - yl @ V.T, ls, sv, lb))) < 1e-10 * abs(float(loss))
        dvec.copy_(dvec0)


def test_tlin_export_is_declared_exported_and_bound():
    from fidelityfusion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ffgp.h")).read()
    assert re.search(r"\bint ffgp_train_tlin_raw\s*\(", hdr)
    assert "CIGAR.py:116-133" in hdr
    assert "ffgp_train_tlin_raw" in _lib.EXPORTS
    so = os.path.join(ROOT, "fidelityfusion_amd", "libffgp.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT ffgp_train_tlin_raw\b", syms)
    assert _lib.lib.ffgp_train_tlin_raw is not None


def test_train_many_signature_is_unchanged():
    from fidelityfusion_amd.cigp_v10 import train_many
    assert list(inspect.signature(train_many).parameters) == ["models", "xs", "ys", "steps", "lr", "betas", "eps", "state", "residual",
                                                              "tree_one_launch", "car", "fuse_composed", "wide_one_launch"]


def test_tlin_one_launch_instantiations_spill_no_more_than_the_residual_ones():
    """kernel metadata of csrc/train.hip (private_segment_fixed_size only): the new <8> instantiation has no scratch, the new <16> no
    more than ffgp_train_resid_kernel<16>"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from check_isa import device_asm
    from test_train_residual_isa import _meta
    asm = device_asm("train.hip")
    assert _meta(asm, "ffgp_train_tlin_kernelILi8E")["private_segment_fixed_size"] == 0
    lin16, res16 = _meta(asm, "ffgp_train_tlin_kernelILi16E"), _meta(asm, "ffgp_train_resid_kernelILi16E")
    assert lin16["private_segment_fixed_size"] <= res16["private_segment_fixed_size"], (lin16, res16)
