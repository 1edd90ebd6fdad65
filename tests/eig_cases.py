"""Inputs, references and bounds of the eigensolver's scale and hard-case tests, shared by the device tests (test_gpu_syevd.py) and
their CPU twins on the numpy restatement (test_eigh_model.py), so that the kernel and the model are held to the same checks.

Every comparison is made in O(1) units: inputs and results are divided by the scale the test applied before numpy sees them (at 1e-160
and 1e150 numpy's own squares under- or overflow)."""
import numpy as np
import torch

STAGE3_SCALES = (1e-160, 1e-20, 1e-6, 1e150)
SYEVD_SCALES = (1e-160, 1e-6, 1e150)
STAGE3_POW2 = (-200, -40, 40, 200)
SYEVD_POW2 = (-200, 200)
SYEVD_SIZES = (40, 64, 100, 130, 256)      # Jacobi path, the no-padding boundary, two padded sizes, two merge levels
HARD_CASES = ("wilkinson", "glued_wilkinson", "zero_e_on_leaf_boundaries", "negative_zero_e", "zero", "identity", "identity_e1e-9",
              "zero_d_unit_e", "random320")
CONSTANT_CASES = {"zero": 0.0, "identity": 1.0}   # every eigenvalue exactly this


def kernel_matrix(n, D, ls, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    X = torch.rand((n, D), generator=g, dtype=torch.float64)
    d = torch.cdist(X / ls, X / ls)
    return torch.exp(-0.5 * d * d)


def random_sym(n, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    M = torch.randn((n, n), generator=g, dtype=torch.float64)
    return M + M.T


def syevd_matrix(kind, n):
    return (random_sym(n, n) if kind == "rand" else kernel_matrix(n, 3, 0.7, n)).numpy()


def random_tridiagonal(n, seed=0):
    """d, e ~ N(0, 1); e has n entries, the last one unused (the device's convention)"""
    g = np.random.default_rng(seed)
    return g.standard_normal(n), g.standard_normal(n)


def hard_case(name):
    """(d [n], e [n]) of the classic hard inputs of the tridiagonal divide and conquer"""
    n = 256
    if name == "wilkinson":                      # W_n^+: pairs of eigenvalues that agree to working precision at the top of the spectrum
        return np.abs(np.arange(n) - (n - 1) / 2.0), np.ones(n)
    if name == "glued_wilkinson":                # W_21^+ blocks glued by 1e-8: clusters of ~13 eigenvalues within 1e-8 (LAPACK's stress case)
        i = np.arange(n)
        e = np.ones(n)
        e[i % 21 == 20] = 1e-8
        return np.abs(i % 21 - 10.0), e
    if name in ("zero_e_on_leaf_boundaries", "negative_zero_e"):   # rho = 0 in a merge
        d, e = random_tridiagonal(n)
        e[63] = 0.0
        e[127] = -0.0 if name == "negative_zero_e" else 0.0
        return d, e
    if name == "zero":
        return np.zeros(n), np.zeros(n)
    if name == "identity":
        return np.ones(n), np.zeros(n)
    if name == "identity_e1e-9":
        return np.ones(n), 1e-9 * np.ones(n)
    if name == "zero_d_unit_e":
        return np.zeros(n), np.ones(n)
    if name == "random320":                      # five leaves: a merge with an empty second half on two levels, a ragged last GEMM
        return random_tridiagonal(320, 320)
    raise KeyError(name)


def check_stage3(d, e, W, Z, unit=1.0, label=""):
    """the bounds of test_stage3_divide_and_conquer, relative to the matrix scale: (d, e, W) / unit against LAPACK"""
    d, e, W = np.asarray(d) / unit, np.asarray(e) / unit, np.asarray(W) / unit
    n = d.size
    T = np.diag(d) + np.diag(e[:n - 1], 1) + np.diag(e[:n - 1], -1)
    ref = np.linalg.eigvalsh(T)
    scale = np.abs(ref).max()
    e_val = np.abs(W - ref).max()
    e_orth = np.abs(Z.T @ Z - np.eye(n)).max()
    e_rec = np.abs((Z * W) @ Z.T - T).max()
    b_val = 1e-14 * scale * max(1.0, np.sqrt(n) / 8)
    print("%s unit %g: values %.2e (bound %.2e) orth %.2e (2e-13) rec %.2e (bound %.2e)" % (label, unit, e_val, b_val, e_orth, e_rec, 1e-13 * scale))
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(Z))
    assert np.all(np.diff(W) >= 0)
    assert e_val <= b_val, (e_val, b_val)
    assert e_orth <= 2e-13, e_orth
    assert e_rec <= 1e-13 * scale, (e_rec, 1e-13 * scale)


def check_syevd(A, W, Z, unit=1.0, label=""):
    """the bounds of test_syevd_vs_lapack, relative to the matrix scale: (A, W) / unit against LAPACK"""
    A, W = np.asarray(A) / unit, np.asarray(W) / unit
    n = A.shape[0]
    ref = np.linalg.eigvalsh(A)
    e_val = np.abs(W - ref).max() / np.abs(ref).max()
    e_orth = np.abs(Z.T @ Z - np.eye(n)).max()
    e_rec = np.linalg.norm((Z * W) @ Z.T - A)
    b_rec = 1e-13 * np.linalg.norm(A) * max(1.0, np.sqrt(n) / 8)
    print("%s n %d unit %g: values %.2e (1e-13) orth %.2e (5e-13) rec %.2e (bound %.2e)" % (label, n, unit, e_val, e_orth, e_rec, b_rec))
    assert W.shape == (n,) and Z.shape == (n, n)
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(Z))
    assert np.all(np.diff(W) >= 0)
    assert e_val <= 1e-13, e_val
    assert e_orth <= 5e-13, e_orth
    assert e_rec <= b_rec, (e_rec, b_rec)
