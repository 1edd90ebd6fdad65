"""GPU: the rotated k loop of the 128 x 128 fast GEMM tile (gemm_tile_fast128, csrc/gemm.hip).

The loop keeps one barrier per k-tile but places it between the MFMAs of kq = 2 and kq = 3, stores k-tile t+1 into the other LDS stage
under the MFMAs of k-tile t and reads the first operands of k-tile t+1 behind the barrier.  What can go wrong is stage parity, the loop
ends (the prologue preload, the peeled last k-tile) and a stage being overwritten while another wave still reads it; the arithmetic
itself must be the unrotated loop's bit for bit, which the 64-row tiles (an untouched loop with the same accumulation order) witness.
All calls go through ffgp_gemm with the tile forced by the `gemm_tile` option, even leading dimensions, alpha = -1 / beta = 1 (or
+1 / 0), so the 128-tile launches take the fast form."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ff():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fidelityfusion_amd import _lib
    h = _lib.handle(0)
    _lib.bind_stream(h, 0)
    return _lib, h


def relerr(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def gemm(ff, tile, opa, opb, lower, A, B, C0, alpha, beta, launches=1):
    """op(A) [m,k], op(B) [k,n] stored as the op flags say (0: k contiguous, 1: m / n contiguous), unpadded; the results of
    `launches` launches from the same inputs."""
    _lib, h = ff
    m, k = A.shape
    n = B.shape[1]
    As = np.ascontiguousarray(A if opa == 0 else A.T)
    Bs = np.ascontiguousarray(B.T if opb == 0 else B)
    assert As.shape[1] % 2 == 0 and Bs.shape[1] % 2 == 0 and n % 2 == 0, "even leading dimensions: the fast form"
    Ad = torch.tensor(As, dtype=torch.float64, device="cuda:0")
    Bd = torch.tensor(Bs, dtype=torch.float64, device="cuda:0")
    C0d = torch.tensor(np.ascontiguousarray(C0), dtype=torch.float64, device="cuda:0")
    outs = []
    assert _lib.lib.ffgp_set_option(h, b"gemm_tile", float(tile)) == 0
    try:
        for _ in range(launches):
            Cd = C0d.clone()
            rc = _lib.lib.ffgp_gemm(h, opa, opb, lower, 0, C.c_void_p(Ad.data_ptr()), As.shape[1], C.c_void_p(Bd.data_ptr()), Bs.shape[1],
                                    C.c_void_p(Cd.data_ptr()), n, m, n, k, alpha, beta)
            assert rc == 0, rc
            torch.cuda.synchronize()
            outs.append(Cd.cpu().numpy())
    finally:
        _lib.lib.ffgp_set_option(h, b"gemm_tile", 0.0)
    return outs if launches > 1 else outs[0]


def operands(m, n, k, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((m, k)), rng.standard_normal((k, n)), rng.standard_normal((m, n))


@pytest.mark.parametrize("k", [16, 32, 48, 64, 80, 512])
def test_one_tile_stage_parity_and_loop_ends(ff, k):
    """nkt = 1, 2, 3, 4, 5, 32: the prologue preload alone, both stage parities, a last k-tile with and without a predecessor"""
    A, B, C0 = operands(128, 128, k, 100 + k)
    out = gemm(ff, 128, 0, 0, 0, A, B, C0, -1.0, 1.0)
    err = relerr(out, C0 - A @ B)
    print("k = %d: relerr %.3e" % (k, err))
    assert err < 1e-13
    assert np.array_equal(out, gemm(ff, 64, 0, 0, 0, A, B, C0, -1.0, 1.0)), "the rotated loop changed the arithmetic"


@pytest.mark.parametrize("k", [32, 48])
def test_one_tile_beta_zero_does_not_read_c(ff, k):
    A, B, _ = operands(128, 128, k, 200 + k)
    nan = np.full((128, 128), np.nan)
    out = gemm(ff, 128, 0, 0, 0, A, B, nan, 1.0, 0.0)
    err = relerr(out, A @ B)
    print("k = %d: relerr %.3e" % (k, err))
    assert err < 1e-13, "beta == 0 must not read C"
    assert np.array_equal(out, gemm(ff, 64, 0, 0, 0, A, B, nan, 1.0, 0.0))


@pytest.mark.parametrize("opa,opb", [(0, 1), (1, 0), (1, 1)])
def test_one_tile_other_layouts(ff, opa, opb):
    """the rotated loop serves every operand layout of the 128-tile (the MN-major LDS image has another stage size)"""
    A, B, C0 = operands(128, 128, 48, 300 + 2 * opa + opb)
    out = gemm(ff, 128, opa, opb, 0, A, B, C0, -1.0, 1.0)
    assert relerr(out, C0 - A @ B) < 1e-13
    assert np.array_equal(out, gemm(ff, 64, opa, opb, 0, A, B, C0, -1.0, 1.0))


def test_full_mode_same_bits_as_the_64_tile(ff):
    A, B, C0 = operands(384, 256, 48, 7)
    out = gemm(ff, 128, 0, 0, 0, A, B, C0, -1.0, 1.0)
    assert relerr(out, C0 - A @ B) < 1e-13
    assert np.array_equal(out, gemm(ff, 64, 0, 0, 0, A, B, C0, -1.0, 1.0))


@pytest.mark.parametrize("k", [48, 512])
def test_lower_mode(ff, k):
    """the strictly-lower tiles take the rotated loop, the diagonal tiles the general form; the upper part is not written"""
    A, B, C0 = operands(384, 384, k, 400 + k)
    out = gemm(ff, 128, 0, 0, 1, A, B, C0, -1.0, 1.0)
    full = C0 - A @ B
    mask = np.tril(np.ones((384, 384), dtype=bool))
    err = relerr(out[mask], full[mask])
    print("k = %d: relerr %.3e" % (k, err))
    assert err < 1e-13
    assert np.array_equal(out[~mask], C0[~mask]), "strictly-upper part must not be written"


def test_stage_reuse_under_contention(ff):
    """1024 tiles (two per CU and then some), five launches from the same inputs: a stage overwritten under a slow wave's reads shows
    as a launch that differs from the 64-tile result"""
    A, B, C0 = operands(4096, 4096, 256, 11)
    ref = gemm(ff, 64, 0, 0, 0, A, B, C0, -1.0, 1.0)
    for i, out in enumerate(gemm(ff, 128, 0, 0, 0, A, B, C0, -1.0, 1.0, launches=5)):
        assert np.array_equal(out, ref), "launch %d differs from the 64-tile result" % i
