"""The one-workgroup LDS eigensolver for n <= 128 (ffgp_syev_lds, csrc/eig_lds.hip: one-sided Jacobi on one LDS image of the
shifted matrix) through the C ABI and its Python callers: against LAPACK at the bounds of test_syevd_vs_lapack, its layout
contract, batch independence, argument errors, `eigh_small` above 64 rows and the HOGP block at GAR's size (N = 100; reference:
two_fidelity_models/hogp_simple.py:15-19,97-100)."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.noisy]   # (noisy: beside a background load by default, tests/conftest.py)
DEV = "cuda:0"
SENTINEL = -777.25


def ptr(t):
    return C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def ff():
    from fidelityfusion_amd import _lib
    h = _lib.handle(0)
    _lib.bind_stream(h, 0)
    return _lib, h


def _se(rng, n, D, ls):
    X = rng.random((n, D))
    return np.exp(-0.5 * ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1) / ls ** 2)


def _seven_kinds(n):
    rng = np.random.default_rng(1000 + n)
    R = rng.standard_normal((n, n))
    Qo, _ = np.linalg.qr(rng.standard_normal((n, n)))
    k = np.arange(n)
    d = np.where(k % 2 == 0, 1.0, -1.0) * 10.0 ** (-16.0 * k / max(n - 1, 1))
    G = (Qo * d) @ Qo.T
    return np.stack([_se(rng, n, 3, 0.7), _se(rng, n, 1, 0.5), R + R.T, np.eye(n) + np.ones((n, n)) / n,
                     np.diag(rng.standard_normal(n)), 0.5 * (G + G.T), np.zeros((n, n))])


@pytest.mark.parametrize("n", [1, 2, 64, 65, 66, 100, 127, 128])
def test_syev_lds_vs_lapack(n):
    """seven kinds of matrix in one call -- SE kernel matrices (D = 3, ls 0.7; D = 1, ls 0.5), R + R^T, I + 11^T / n, a diagonal
    matrix, a graded indefinite spectrum +-10^(-16 k / (n - 1)) and the zero matrix -- at the bounds of test_syevd_vs_lapack"""
    from fidelityfusion_amd import functional as F
    M = _seven_kinds(n)
    ev, Q, info = F._syev_lds(torch.tensor(M, device=DEV), info=True)
    evd, Qd, infod = F._syev_lds(torch.tensor(M, device=DEV), descending=True, info=True)
    assert info.dtype == torch.int32 and info.cpu().tolist() == [0] * 7 and infod.cpu().tolist() == [0] * 7
    ev, Q, evd, Qd = ev.cpu().numpy(), Q.cpu().numpy(), evd.cpu().numpy(), Qd.cpu().numpy()
    assert ev.shape == (7, n) and Q.shape == (7, n, n)
    for b in range(7):
        ref = np.linalg.eigvalsh(M[b])
        scale = max(np.abs(ref).max(), 1e-300)
        e_val = np.abs(ev[b] - ref).max() / scale
        e_orth = np.abs(Q[b].T @ Q[b] - np.eye(n)).max()
        e_rec = np.linalg.norm((Q[b] * ev[b]) @ Q[b].T - M[b])
        bound = 1e-13 * np.linalg.norm(M[b]) * max(1.0, np.sqrt(n) / 8)
        print("n=%d kind=%d values %.2e orth %.2e rec %.2e (bound %.2e)" % (n, b, e_val, e_orth, e_rec, bound))
        assert np.all(np.diff(ev[b]) >= 0), b
        assert e_val <= 1e-13, (b, e_val)
        assert e_orth <= 5e-13, (b, e_orth)
        assert e_rec <= bound, (b, e_rec, bound)
        assert np.array_equal(evd[b], ev[b][::-1]), b
        if len(np.unique(ev[b])) == n:                  # (equal eigenvalues keep their index order in both directions)
            assert np.array_equal(Qd[b], Q[b][:, ::-1]), b
        else:
            assert np.abs(Qd[b].T @ Qd[b] - np.eye(n)).max() <= 5e-13, b
            assert np.linalg.norm((Qd[b] * evd[b]) @ Qd[b].T - M[b]) <= bound, b
    assert np.array_equal(ev[6], np.zeros(n)) and np.array_equal(Q[6], np.eye(n))      # the zero matrix: zeros and the identity


def test_syev_lds_layout_lower_triangle_and_padding(ff):
    """ldm = n + 3, ldq = n + 5, strideE = n + 2, the strict upper triangle filled with 7.0: the values are the clean call's bit for
    bit, the input is unchanged and every padding element of the outputs still holds the sentinel"""
    from fidelityfusion_amd import functional as F
    _lib, h = ff
    n, B = 77, 3
    rng = np.random.default_rng(7)
    R = rng.standard_normal((B, n, n))
    A = torch.tensor(R + R.transpose(0, 2, 1), device=DEV)
    ev0, Q0 = F._syev_lds(A)
    ldm, ldq, sE = n + 3, n + 5, n + 2
    sM, sQ = n * ldm + 11, n * ldq + 13
    Mbuf = torch.full((B * sM,), SENTINEL, dtype=torch.float64, device=DEV)
    iu = torch.triu_indices(n, n, 1, device=DEV)
    junk = A.clone()
    junk[:, iu[0], iu[1]] = 7.0
    Mview = torch.as_strided(Mbuf, (B, n, n), (sM, ldm, 1))
    Mview.copy_(junk)
    keep = Mbuf.clone()
    Qbuf = torch.full((B * sQ,), SENTINEL, dtype=torch.float64, device=DEV)
    Ebuf = torch.full((B * sE,), SENTINEL, dtype=torch.float64, device=DEV)
    info = torch.full((B,), 99, dtype=torch.int32, device=DEV)
    assert _lib.lib.ffgp_syev_lds(h, ptr(Mbuf), n, ldm, B, sM, ptr(Qbuf), ldq, sQ, ptr(Ebuf), sE, 0, ptr(info)) == 0
    torch.cuda.synchronize()
    assert torch.equal(Mbuf, keep)
    assert info.cpu().tolist() == [0] * B
    Qv = torch.as_strided(Qbuf, (B, n, n), (sQ, ldq, 1))
    Ev = torch.as_strided(Ebuf, (B, n), (sE, 1))
    assert torch.equal(Qv, Q0) and torch.equal(Ev, ev0)
    Qpad, Epad = torch.ones_like(Qbuf, dtype=torch.bool), torch.ones_like(Ebuf, dtype=torch.bool)
    torch.as_strided(Qpad, (B, n, n), (sQ, ldq, 1)).fill_(False)
    torch.as_strided(Epad, (B, n), (sE, 1)).fill_(False)
    assert bool((Qbuf[Qpad] == SENTINEL).all()) and bool((Ebuf[Epad] == SENTINEL).all())
    # a NULL info is allowed
    Qbuf2 = torch.full_like(Qbuf, SENTINEL)
    assert _lib.lib.ffgp_syev_lds(h, ptr(Mbuf), n, ldm, B, sM, ptr(Qbuf2), ldq, sQ, ptr(Ebuf), sE, 0, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(Qbuf2, Qbuf)


def test_syev_lds_batch_members_do_not_interact():
    """one matrix at positions 0, 4 and 8 of a batch of 9 (n = 100) between different ones: three bit-identical results"""
    from fidelityfusion_amd import functional as F
    n = 100
    rng = np.random.default_rng(3)
    mats = []
    for b in range(9):
        mats.append(_se(rng, n, 2, 0.6) if b % 2 else rng.standard_normal((n, n)))
    same = _se(rng, n, 3, 0.7)
    for b in (0, 4, 8):
        mats[b] = same
    M = np.stack(mats)
    M = M + M.transpose(0, 2, 1)
    ev, Q, info = F._syev_lds(torch.tensor(M, device=DEV), info=True)
    assert info.cpu().tolist() == [0] * 9
    for b in (4, 8):
        assert torch.equal(ev[b], ev[0]) and torch.equal(Q[b], Q[0])
    assert not torch.equal(ev[1], ev[0])


def test_syev_lds_argument_errors_leave_the_outputs_alone(ff):
    _lib, h = ff
    assert _lib.lib.ffgp_syev_lds.argtypes is not None
    for n, ldm, ldq in ((129, 129, 129), (100, 100, 99), (100, 99, 100), (0, 4, 4)):
        nn = max(n, 1)
        M = torch.eye(nn, dtype=torch.float64, device=DEV).repeat(2, 1, 1)
        Q = torch.full((2, nn, nn), SENTINEL, dtype=torch.float64, device=DEV)
        ev = torch.full((2, nn), SENTINEL, dtype=torch.float64, device=DEV)
        info = torch.full((2,), 99, dtype=torch.int32, device=DEV)
        rc = _lib.lib.ffgp_syev_lds(h, ptr(M), n, ldm, 2, nn * nn, ptr(Q), ldq, nn * nn, ptr(ev), nn, 0, ptr(info))
        torch.cuda.synchronize()
        assert rc == _lib.FFGP_ERR_ARG, (n, ldm, ldq, rc)
        assert bool((Q == SENTINEL).all()) and bool((ev == SENTINEL).all()) and info.cpu().tolist() == [99, 99]
    M = torch.eye(4, dtype=torch.float64, device=DEV)
    Q = torch.full((4, 4), SENTINEL, dtype=torch.float64, device=DEV)
    ev = torch.full((4,), SENTINEL, dtype=torch.float64, device=DEV)
    assert _lib.lib.ffgp_syev_lds(h, None, 4, 4, 1, 16, ptr(Q), 4, 16, ptr(ev), 4, 0, None) == _lib.FFGP_ERR_ARG
    assert _lib.lib.ffgp_syev_lds(h, ptr(M), 4, 4, 1, 16, None, 4, 16, ptr(ev), 4, 0, None) == _lib.FFGP_ERR_ARG
    assert _lib.lib.ffgp_syev_lds(h, ptr(M), 4, 4, 1, 16, ptr(Q), 4, 16, None, 4, 0, None) == _lib.FFGP_ERR_ARG
    assert _lib.lib.ffgp_syev_lds(h, ptr(M), 4, 4, 0, 16, ptr(Q), 4, 16, ptr(ev), 4, 0, None) == 0      # an empty batch is not an error
    torch.cuda.synchronize()
    assert bool((Q == SENTINEL).all()) and bool((ev == SENTINEL).all())


def test_eigh_small_at_100_rows_matches_torch():
    """`eigh_small` above 64 rows (it raised there before ffgp_syev_lds): value and gradient of the sign-invariant loss of
    test_eigh_small_backward_matches_torch, sized to n = 100, against torch.linalg.eigh.  K = Q diag((1..n) / n) Q^T: the
    backward divides by the eigenvalue gaps, which are 1 / n here."""
    from fidelityfusion_amd import functional as F
    n = 100
    rng = np.random.default_rng(4)
    Qo, _ = np.linalg.qr(rng.standard_normal((n, n)))
    K0 = (Qo * (np.arange(1, n + 1) / n)) @ Qo.T
    K0 = 0.5 * (K0 + K0.T)
    W = torch.tensor(rng.standard_normal((n, n)), device=DEV)
    outs = []
    for fn in (F.eigh_small, lambda K: torch.linalg.eigh(K, UPLO="U")):
        K = torch.tensor(K0, device=DEV, requires_grad=True)
        lam, U = fn(K)
        loss = (lam ** 2 * torch.arange(1, n + 1, device=DEV)).sum() + ((U * lam.sqrt()) @ (U * lam.sqrt()).T * W).sum() \
            + (U @ torch.diag(1.0 / (1.0 + lam)) @ U.T * W.T).sum()
        loss.backward()
        outs.append((float(loss.detach()), K.grad.cpu().numpy()))
    print("loss rel %.2e" % (abs(outs[0][0] - outs[1][0]) / abs(outs[1][0])))
    assert abs(outs[0][0] - outs[1][0]) <= 1e-11 * abs(outs[1][0])
    g0, g1 = outs[0][1], outs[1][1]
    print("grad rel %.2e" % (np.abs(g0 - 0.5 * (g1 + g1.T)).max() / np.abs(g1).max()))
    assert np.abs(g0 - 0.5 * (g1 + g1.T)).max() <= 1e-9 * np.abs(g1).max()


def test_hogp_block_at_100_points_on_the_lds_solver():
    """HOGP_simple at N = 100, D = 3, modes (6, 5), variance_mode="eigen": loss, the Y, noise and length-scale gradients, the cached
    g and the posterior mean with LDS_EIGH_MAX_N = 128 (one-launch LDS solver), = 64 (two-stage solver) and a torch.linalg.eigh
    comparator, at the tolerances of test_hogp_block_same_with_both_eigensolvers.  With 128 the input kernel must not reach
    `eigh.eigh` (patched to raise); at N = 129 it must."""
    from fidelityfusion_amd import eigh as E
    from fidelityfusion_amd import hogp_simple, kernel
    n, d1, d2 = 100, 6, 5
    g = torch.Generator(device=DEV).manual_seed(5)
    X = torch.rand((n, 3), generator=g, device=DEV, dtype=torch.float64)
    Y = torch.randn((n, d1, d2), generator=g, device=DEV, dtype=torch.float64)
    Xt = torch.rand((9, 3), generator=g, device=DEV, dtype=torch.float64)

    class _VendorPairs:                               # the comparator: torch.linalg.eigh = rocSOLVER
        def __init__(self, matrix):
            self.value, self.vector = torch.linalg.eigh(matrix.detach(), UPLO="U")

    me = threading.get_ident()       # (the background load of the noisy tests calls eigh.eigh from its own thread: let it)

    def _raise(A, *a, **k):
        if threading.get_ident() == me:
            raise AssertionError("the two-stage solver was called")
        return real_eigh(A, *a, **k)

    real_eigh = E.eigh
    own_pairs, own_max = hogp_simple.eigen_pairs, hogp_simple.LDS_EIGH_MAX_N
    res = {}
    try:
        for route in ("lds", "twostage", "rocsolver"):
            hogp_simple.eigen_pairs = _VendorPairs if route == "rocsolver" else own_pairs
            hogp_simple.LDS_EIGH_MAX_N = 128 if route == "lds" else 64
            E.eigh = _raise if route == "lds" else real_eigh
            m = hogp_simple.HOGP_simple(kernel.ARDKernel(3), 0.7, [d1, d2], variance_mode="eigen").double().to(DEV)
            Yr = Y.clone().requires_grad_(True)
            loss = m.log_likelihood(X, Yr)
            loss.backward()
            with torch.no_grad():
                mu, _ = m.forward(X, Xt)
            if route == "lds":
                assert not m.K_eigen[0].value.requires_grad and m.K_eigen[0].vector.grad_fn is None
            res[route] = (float(loss.detach()), Yr.grad.clone(), m.noise_variance.grad.clone(), m.kernel_list[0].length_scales.grad.clone(),
                          m.g.clone(), mu.clone())
        # one row past the LDS solver's range: the two-stage solver serves the input kernel
        calls = []

        def _spy(A, *a, **k):
            if threading.get_ident() == me:
                calls.append(A.shape[0])
            return real_eigh(A, *a, **k)
        hogp_simple.eigen_pairs, hogp_simple.LDS_EIGH_MAX_N, E.eigh = own_pairs, 128, _spy
        X2 = torch.rand((129, 3), generator=g, device=DEV, dtype=torch.float64)
        Y2 = torch.randn((129, d1, d2), generator=g, device=DEV, dtype=torch.float64)
        m = hogp_simple.HOGP_simple(kernel.ARDKernel(3), 0.7, [d1, d2], variance_mode="eigen").double().to(DEV)
        with torch.no_grad():
            m.log_likelihood(X2, Y2)
        assert calls == [129]
    finally:
        hogp_simple.eigen_pairs, hogp_simple.LDS_EIGH_MAX_N, E.eigh = own_pairs, own_max, real_eigh
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
    b = res["rocsolver"]
    for own in ("lds", "twostage"):
        a = res[own]
        print(own, "loss %.2e" % (abs(a[0] - b[0]) / abs(b[0])), " ".join("%.2e" % rel(a[i], b[i]) for i in range(1, 6)))
        assert abs(a[0] - b[0]) <= 1e-10 * abs(b[0]), own
        assert rel(a[1], b[1]) < 1e-8 and rel(a[2], b[2]) < 1e-8 and rel(a[3], b[3]) < 1e-7, own
        assert rel(a[4], b[4]) < 1e-8 and rel(a[5], b[5]) < 1e-8, own


def test_syev_lds_non_finite_input_gives_nan_and_a_status():
    """a NaN row and column (what one NaN row of X makes of a kernel matrix), an all-NaN matrix, one Inf and one NaN in the strict
    upper triangle (never read) beside a clean matrix: NaN in every output and info = n for the first three, the others untouched by
    their neighbours; the Python callers that do not read the status get NaN eigenvalues"""
    from fidelityfusion_amd import functional as F
    from fidelityfusion_amd import hogp_simple
    n = 100
    rng = np.random.default_rng(11)
    clean = _se(rng, n, 3, 0.7)
    nan_cross, all_nan, one_inf, upper_nan = clean.copy(), np.full((n, n), np.nan), clean.copy(), clean.copy()
    nan_cross[17, :] = np.nan
    nan_cross[:, 17] = np.nan
    one_inf[60, 3] = np.inf
    upper_nan[3, 60] = np.nan
    M = torch.tensor(np.stack([nan_cross, clean, all_nan, one_inf, upper_nan]), device=DEV)
    ev, Q, info = F._syev_lds(M, info=True)
    assert info.cpu().tolist() == [n, 0, n, n, 0]
    for b in (0, 2, 3):
        assert bool(ev[b].isnan().all()) and bool(Q[b].isnan().all()), b
    ev1, Q1 = F._syev_lds(M[1:2])
    for b in (1, 4):
        assert torch.equal(ev[b], ev1[0]) and torch.equal(Q[b], Q1[0]), b
    evc, _ = F._syev_lds_checked(M)
    assert bool(evc[0].isnan().all()) and torch.equal(evc[1], ev[1])
    assert hogp_simple.LDS_EIGH_MAX_N >= n
    assert bool(hogp_simple.eigen_pairs(M[0]).value.isnan().all())
    lam, _ = F.eigh_small(M[0])
    assert bool(lam.isnan().all())


def test_syev_lds_checked_poisons_an_unconverged_member(monkeypatch):
    """the status is honoured without a host wait: a member whose info is not 0 comes back with NaN eigenvalues"""
    from fidelityfusion_amd import linalg
    ev = torch.arange(6, dtype=torch.float64, device=DEV).reshape(2, 3)
    Q = torch.eye(3, dtype=torch.float64, device=DEV).repeat(2, 1, 1)
    monkeypatch.setattr(linalg, "_syev_lds", lambda M, descending=False, info=False: (ev, Q, torch.tensor([0, 5], dtype=torch.int32, device=DEV)))
    got, _ = linalg._syev_lds_checked(Q)
    assert torch.equal(got[0], ev[0]) and bool(got[1].isnan().all())


@pytest.mark.parametrize("scale", [1e-160, 1e150])
def test_syev_lds_at_extreme_scales(scale):
    """entries whose squares are denormal (or overflow): the norms are taken of the scaled image, so the shift still bounds the
    spectrum and the bounds of test_syev_lds_vs_lapack hold relative to the matrix"""
    from fidelityfusion_amd import functional as F
    n = 100
    rng = np.random.default_rng(12)
    R = rng.standard_normal((n, n))
    M = np.stack([(R + R.T) * scale, _se(rng, n, 3, 0.7) * scale])
    ev, Q, info = F._syev_lds(torch.tensor(M, device=DEV), info=True)
    assert info.cpu().tolist() == [0, 0]
    ev, Q = ev.cpu().numpy(), Q.cpu().numpy()
    for b in range(2):
        A = M[b] / scale                                   # (compare in O(1) units: numpy's own squares would under/overflow too)
        lam = ev[b] / scale
        ref = np.linalg.eigvalsh(A)
        e_val = np.abs(lam - ref).max() / np.abs(ref).max()
        e_orth = np.abs(Q[b].T @ Q[b] - np.eye(n)).max()
        e_rec = np.linalg.norm((Q[b] * lam) @ Q[b].T - A)
        bound = 1e-13 * np.linalg.norm(A) * max(1.0, np.sqrt(n) / 8)
        print("scale %g kind=%d values %.2e orth %.2e rec %.2e (bound %.2e)" % (scale, b, e_val, e_orth, e_rec, bound))
        assert e_val <= 1e-13 and e_orth <= 5e-13 and e_rec <= bound, (b, e_val, e_orth, e_rec, bound)
