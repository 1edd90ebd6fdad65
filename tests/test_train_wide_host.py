"""CPU: what ffgp_train_wide_raw (csrc/train_wide.hip) and train_many(..., wide_one_launch=True) rest on, and their surface.

The identity.  The V1 likelihood and its gradients see the targets only through inner products of their rows, so training on the row
blocks of Z_eff = U sqrt(max(Lambda, 0)), U Lambda U^T = Z Z^T (Z = Y, or [y_high; y_low] of a residual member), with the TRUE d in
d sum log L_ii + n d / 2 log(2 pi), gives the loss and every gradient of the full targets -- dloss/drho included.  Checked here in fp64
on the operator sequence of oracle/torch_cpu_ref.py (`wide_ll` with the full targets IS `cigp_ll`, asserted bit for bit), with
torch.linalg.eigh standing in for the package's device solver (`compress_cpu` restates the compression: these tests check the
mathematics; train.compress_targets itself -- its eigensolver routes, clamp and row split -- is held to Z_eff Z_eff^T = Z Z^T on
the GPU, test_gpu_train_wide.py::test_compress_targets_keeps_the_gram).

The bound: both sides are fp64 evaluations of one function on data that differ by the rounding of an m x m eigendecomposition and of
the Gram (a d-term sum: up to ~sqrt(d) u relative); the loss is dominated by terms of relative size 1, the gradients by sums of n^2
terms.  The issue's own measurement of these shapes is 1.4e-15 (plain) and 1.7e-14 (rho); 1e-12 leaves two decades and is four
decades below anything a wrong d, a dropped block or a missing clamp would give (those are O(1))."""
import inspect
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(4, 40), (17, 33), (32, 1024), (128, 300), (100, 4096)]
D = 3
BOUND = 1e-12


def compress_cpu(*mats):
    """train.compress_targets with torch's CPU eigensolver in place of the device's"""
    Z = torch.cat(mats, 0)
    lam, U = torch.linalg.eigh(Z @ Z.T)
    Zeff = U * lam.clamp_min(0.0).sqrt()
    out, r0 = [], 0
    for t in mats:
        out.append(Zeff[r0:r0 + t.shape[0]].contiguous())
        r0 += t.shape[0]
    return out


def wide_ll(X, Y, ls, sv, lb, d_true):
    """oracle/torch_cpu_ref.cigp_ll, its d given apart from the columns of Y"""
    from oracle import torch_cpu_ref as R
    n = X.shape[0]
    eye = torch.eye(n, dtype=X.dtype)
    Sigma = R.ard_kernel(X, X, ls, sv) + lb.exp().pow(-1) * eye + R.JITTER * eye
    L = torch.linalg.cholesky(Sigma)
    Gamma = torch.linalg.solve_triangular(L, Y, upper=False)
    nll = 0.5 * (Gamma ** 2).sum() + L.diag().log().sum() * d_true + 0.5 * n * torch.log(2 * torch.tensor(R.PI_TRUNC, dtype=X.dtype)) * d_true
    return -nll


def problem(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, D, generator=g, dtype=torch.float64) * 2
    W = torch.randn(D, d, generator=g, dtype=torch.float64)
    Y = torch.sin(X @ W) + 0.1 * torch.randn(n, d, generator=g, dtype=torch.float64)
    Yl = torch.cos(X @ W) + 0.1 * torch.randn(n, d, generator=g, dtype=torch.float64)
    ls = torch.tensor([0.8, -1.1, 1.3], dtype=torch.float64)
    return X, Y, Yl, ls, torch.tensor([1.2], dtype=torch.float64), torch.tensor([0.7], dtype=torch.float64)


def grads(fn, params):
    ps = [p.clone().requires_grad_(True) for p in params]
    v = fn(*ps)
    v.backward()
    return [v.detach()] + [p.grad for p in ps]


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("n,d", SHAPES)
def test_compressed_targets_give_the_loss_and_gradients_of_the_full_ones(n, d):
    from oracle import torch_cpu_ref as R
    X, Y, _, ls, sv, lb = problem(n, d, 100 + n)
    assert torch.equal(wide_ll(X, Y, ls, sv, lb, d), R.cigp_ll(X, Y, ls, sv, lb))      # the same operator sequence
    Yc, = compress_cpu(Y)
    assert Yc.shape == (n, n)
    full = grads(lambda a, b, c: wide_ll(X, Y, a, b, c, d), [ls, sv, lb])
    comp = grads(lambda a, b, c: wide_ll(X, Yc, a, b, c, d), [ls, sv, lb])
    errs = [rel(c, f) for c, f in zip(comp, full)]
    print((n, d), errs)
    assert max(errs) <= BOUND, errs
    # ... and the d of the log-determinant term is the true one: with the compressed column count the value is another
    assert rel(wide_ll(X, Yc, ls, sv, lb, n), full[0]) > 1e-3


@pytest.mark.parametrize("n,d", SHAPES)
def test_compressed_residual_targets_give_the_gradient_of_rho_too(n, d):
    X, Yh, Yl, ls, sv, lb = problem(n, d, 200 + n)
    rho = torch.tensor([0.9], dtype=torch.float64)
    yhc, ylc = compress_cpu(Yh, Yl)
    assert yhc.shape == ylc.shape == (n, 2 * n)
    full = grads(lambda a, b, c, r: wide_ll(X, Yh - r * Yl, a, b, c, d), [ls, sv, lb, rho])
    comp = grads(lambda a, b, c, r: wide_ll(X, yhc - r * ylc, a, b, c, d), [ls, sv, lb, rho])
    errs = [rel(c, f) for c, f in zip(comp, full)]
    print((n, d), errs)
    assert max(errs) <= BOUND, errs


def test_negative_eigenvalues_are_clamped():
    """a Gram of rank 2 among 6 rows: rounding leaves eigenvalues of either sign at 1e-16 of the largest; the factor stays real"""
    g = torch.Generator().manual_seed(5)
    Y = torch.randn(6, 2, generator=g, dtype=torch.float64) @ torch.randn(2, 50, generator=g, dtype=torch.float64)
    Yc, = compress_cpu(Y)
    assert bool(torch.isfinite(Yc).all())
    assert rel(Yc @ Yc.T, Y @ Y.T) <= 1e-13


def test_no_more_columns_than_rows_pass_through():
    """d <= m: nothing to gain, the very tensors come back (no device is touched)"""
    from fidelityfusion_amd.train import compress_targets
    y = torch.randn(30, 24, dtype=torch.float64)
    out = compress_targets(y)
    assert len(out) == 1 and out[0] is y
    yh, yl = torch.randn(20, 40, dtype=torch.float64), torch.randn(20, 40, dtype=torch.float64)
    out = compress_targets(yh, yl)
    assert out[0] is yh and out[1] is yl


def test_the_symbol_is_declared_exported_and_bound():
    """fails before this route: include/ffgp.h has no ffgp_train_wide_raw"""
    import ctypes
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ffgp.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ffgp_train_wide_raw\s*\(", src)
    from fidelityfusion_amd import _lib
    assert "ffgp_train_wide_raw" in _lib.EXPORTS
    res, args = _lib.EXPORTS["ffgp_train_wide_raw"]
    assert res is ctypes.c_int and len(args) == 14
    assert _lib.lib.ffgp_train_wide_raw.argtypes == args
    # a NULL handle is refused before anything is read
    assert _lib.lib.ffgp_train_wide_raw(None, 1, None, None, None, None, 1, None, None, 8, 0, None, 1, None) == _lib.FFGP_ERR_ARG


def test_the_keyword_is_off_by_default():
    from fidelityfusion_amd.cigp_v10 import train_many
    assert inspect.signature(train_many).parameters["wide_one_launch"].default is False


def test_without_a_gpu_the_keyword_raises_and_does_not_fall_back():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from fidelityfusion_amd import _lib, kernel
    from fidelityfusion_amd.cigp_v10 import cigp, train_many
    m = cigp(kernel.ARDKernel(2), 0.7).double()
    x, y = torch.rand(8, 2, dtype=torch.float64), torch.randn(8, 20, dtype=torch.float64)
    before = [p.detach().clone() for p in m.parameters()]
    with pytest.raises(_lib.FFGPError):
        train_many([m], [x], [y], 2, wide_one_launch=True)
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, m.parameters()))      # the reference's loop did not run in its place
