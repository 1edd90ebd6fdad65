"""GPU: direct-to-LDS operand staging of the 128 x 128 fast GEMM tile (gemm_tile_fast128, csrc/gemm.hip, K-major x K-major).

The pieces of k-tile kt + 2 are issued behind the barrier of k-tile kt into the stage that barrier freed, with a per-lane SOURCE
address that carries the LDS image's swizzle.  What can go wrong: the swizzle on the wrong chunk or a stride taken from k instead of
the leading dimension (operands that are sub-blocks of a wider array), the loop's ends (no k-tile 1, no k-tile kt + 2, the peeled
tail), a stage refilled under a slow wave's reads or read before every wave's pieces landed, the wave that issues no MFMA in a
diagonal tile, another LDS base.  The arithmetic must be the 64-row tiles' bit for bit (an untouched loop, same accumulation order).
Tolerance against numpy: 1e-13 relative, the bound of test_gpu_gemm_pipeline.py (k <= 80 here)."""
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


def opt(ff, key, value):
    _lib, h = ff
    assert _lib.lib.ffgp_set_option(h, key.encode(), C.c_double(value)) == 0, key


def relerr(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))      # (NaN-filled regions compare too)


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


def ptr(t, row, col, ld):
    return C.c_void_p(t.data_ptr() + 8 * (row * ld + col))


def gemm_sub(ff, tile, lower, Aw, a0, Bw, b0, Cw, c0, m, n, k, alpha=-1.0, beta=1.0, launches=1):
    """C[c0 + (m, n)] = alpha A[a0 + (m, k)] B[b0 + (n, k)]^T + beta C on sub-blocks of the wider host arrays Aw, Bw, Cw (K-major
    operands; origins (row, column)).  Returns the whole C buffer of every launch."""
    _lib, h = ff
    Ad, Bd, C0d = dev(Aw), dev(Bw), dev(Cw)
    outs = []
    opt(ff, "gemm_tile", float(tile))
    try:
        for _ in range(launches):
            Cd = C0d.clone()
            rc = _lib.lib.ffgp_gemm(h, 0, 0, lower, 0, ptr(Ad, *a0, Aw.shape[1]), Aw.shape[1], ptr(Bd, *b0, Bw.shape[1]), Bw.shape[1],
                                    ptr(Cd, *c0, Cw.shape[1]), Cw.shape[1], m, n, k, alpha, beta)
            assert rc == 0, rc
            torch.cuda.synchronize()
            outs.append(Cd.cpu().numpy())
    finally:
        opt(ff, "gemm_tile", 0.0)
    return outs if launches > 1 else outs[0]


def lower_quadrants(n):
    """The strictly-lower 64 x 64 quadrant of every diagonal 128-block.  A lower-mode launch gives its diagonal 128-tiles the general
    form's arithmetic (zero accumulators, alpha * acc + beta * C once); the 64-tile launch runs this quadrant as a tile of its own in
    the fast form, which accumulates onto C and rounds differently -- the one place where the two launches never had the same bits."""
    r, c = np.indices((n, n))
    return (r // 128 == c // 128) & (r % 128 >= 64) & (c % 128 < 64)


def lower_mode_bits(ff, out, Aw, a0, Cw, c0, n, k):
    """a lower-mode 128-tile result against the 64-tile launch (everywhere but lower_quadrants) and against the 128-tile launch with
    the diagonal tiles on the general loop (syrk_light_tiles = 0: everywhere)"""
    ref64 = gemm_sub(ff, 64, 1, Aw, a0, Aw, a0, Cw, c0, n, n, k)
    q = np.zeros(Cw.shape, dtype=bool)
    q[c0[0]:c0[0] + n, c0[1]:c0[1] + n] = lower_quadrants(n)
    assert same_bits(out[~q], ref64[~q]), "not the 64-tile's bits"
    opt(ff, "syrk_light_tiles", 0.0)
    try:
        general = gemm_sub(ff, 128, 1, Aw, a0, Aw, a0, Cw, c0, n, n, k)
    finally:
        opt(ff, "syrk_light_tiles", 1.0)
    assert same_bits(out, general), "not the general diagonal tile's bits"


def wide(rng, rows, ld):
    return rng.standard_normal((rows, ld))


@pytest.mark.parametrize("acol,bcol", [(2, 6), (18, 34)])
def test_operands_inside_wider_arrays(ff, acol, bcol):
    """lda = 272, ldb = 1040, ldc = 400; row origins 3 / 5 / 7, column origins multiples of 2 (16-byte loads) but not of 16 -- what the
    factorisation passes: panel and trailing matrix are blocks of one array"""
    rng = np.random.default_rng(acol)
    m, n, k = 256, 128, 48
    Aw, Bw, Cw = wide(rng, m + 8, 272), wide(rng, n + 8, 1040), wide(rng, m + 8, 400)
    a0, b0, c0 = (3, acol), (5, bcol), (7, 10)
    out = gemm_sub(ff, 128, 0, Aw, a0, Bw, b0, Cw, c0, m, n, k)
    ref = Cw.copy()
    ref[7:7 + m, 10:10 + n] -= Aw[3:3 + m, acol:acol + k] @ Bw[5:5 + n, bcol:bcol + k].T
    err = relerr(out, ref)
    print("relerr %.3e" % err)
    assert err < 1e-13
    assert same_bits(out, gemm_sub(ff, 64, 0, Aw, a0, Bw, b0, Cw, c0, m, n, k)), "not the 64-tile's bits"


@pytest.mark.parametrize("k", [16, 32, 48, 64, 80])
def test_one_tile_loop_ends(ff, k):
    """nkt = 1 ... 5: the prologue's k-tile alone; k-tile 1 and no loop; the first pieces issued behind a loop barrier; both stage
    parities; the k-tile that has a barrier and nothing left to fetch.  Padded leading dimensions."""
    rng = np.random.default_rng(500 + k)
    Aw, Bw, Cw = wide(rng, 128, k + 6), wide(rng, 128, k + 18), wide(rng, 128, 130)
    out = gemm_sub(ff, 128, 0, Aw, (0, 2), Bw, (0, 2), Cw, (0, 2), 128, 128, k)
    ref = Cw.copy()
    ref[:, 2:] -= Aw[:, 2:2 + k] @ Bw[:, 2:2 + k].T
    err = relerr(out, ref)
    print("k = %d: relerr %.3e" % (k, err))
    assert err < 1e-13
    assert same_bits(out, gemm_sub(ff, 64, 0, Aw, (0, 2), Bw, (0, 2), Cw, (0, 2), 128, 128, k))


def test_lower_mode_diagonal_tiles_stage_with_every_wave(ff):
    """384 x 384, k = 48, lda = 54, light tiles on: the diagonal tiles run the rotated loop, their upper-quadrant wave issues no MFMA
    and must still stage its share of every k-tile; the strictly-upper part is not touched"""
    rng = np.random.default_rng(384)
    n, k = 384, 48
    Aw = wide(rng, n, k + 6)
    Cw = rng.standard_normal((n, n))
    Cw[np.triu_indices(n, 1)] = np.nan
    opt(ff, "syrk_light_tiles", 1.0)
    out = gemm_sub(ff, 128, 1, Aw, (0, 4), Aw, (0, 4), Cw, (0, 0), n, n, k)
    low = np.tril(np.ones((n, n), dtype=bool))
    ref = Cw - Aw[:, 4:4 + k] @ Aw[:, 4:4 + k].T
    err = relerr(out[low], ref[low])
    print("relerr %.3e" % err)
    assert err < 1e-13
    assert same_bits(out[~low], Cw[~low]), "strictly-upper part was written"
    lower_mode_bits(ff, out, Aw, (0, 4), Cw, (0, 0), n, k)


def test_syrk_of_a_panel_beside_its_trailing_matrix(ff):
    """B = A = the panel W[:, 2:50]; C = W[:, 50:306], in the same allocation to the right of it (lower mode, as the factorisation
    issues its trailing update)"""
    rng = np.random.default_rng(306)
    n, k = 256, 48
    W = wide(rng, n, 2 + k + n + 4)
    out = gemm_sub(ff, 128, 1, W, (0, 2), W, (0, 2), W, (0, 2 + k), n, n, k)
    ref = W.copy()
    low = np.tril(np.ones((n, n), dtype=bool))
    ref[:, 2 + k:2 + k + n][low] -= (W[:, 2:2 + k] @ W[:, 2:2 + k].T)[low]
    err = relerr(out, ref)
    print("relerr %.3e" % err)
    assert err < 1e-13
    assert same_bits(out[:, :2 + k], W[:, :2 + k]) and same_bits(out[:, 2 + k + n:], W[:, 2 + k + n:])
    lower_mode_bits(ff, out, W, (0, 2), W, (0, 2 + k), n, k)


def test_polite_launch(ff):
    """The trailing updates of a factorisation of N = 1408 (panels of 512: the last update is 3 x 3 tiles) are launched with padded
    dynamic LDS, one workgroup per CU, below `polite_m` rows -- only the factorisation tags a launch as its trailing update, so this
    case goes through it.  Same bits with the padding off, and LAPACK's factor."""
    _lib, h = ff
    n, ld = 1408, 1410
    rng = np.random.default_rng(n)
    B = rng.standard_normal((n, 56))
    S = B @ B.T + np.diag(rng.random(n) + 0.5)
    W = np.full((n, ld), np.nan)
    W[:, :n] = np.tril(S) + np.triu(np.full((n, n), 777.0), 1)
    outs = {}
    opt(ff, "gemm_tile", 128.0)
    try:
        for polite_m in (8192, 0):
            opt(ff, "polite_m", float(polite_m))
            Wd = dev(W)
            assert _lib.lib.ffgp_potrf_rows(h, C.c_void_p(Wd.data_ptr()), n, n, ld) == 0
            torch.cuda.synchronize()
            outs[polite_m] = Wd.cpu().numpy()
    finally:
        opt(ff, "polite_m", 8192.0)
        opt(ff, "gemm_tile", 0.0)
    assert same_bits(outs[8192], outs[0])
    assert relerr(np.tril(outs[8192][:, :n]), np.linalg.cholesky(S)) < 1e-11      # (the factorisation's bound in test_gpu_gemm_light_tiles.py)


def test_batched_launch_against_single_calls(ff):
    _lib, h = ff
    rng = np.random.default_rng(2)
    m, n, k = 256, 128, 48
    A, B, C0 = rng.standard_normal((2, m, k)), rng.standard_normal((2, n, k)), rng.standard_normal((2, m, n))
    Ad, Bd, Cd = dev(A), dev(B), dev(C0)
    opt(ff, "gemm_tile", 128.0)
    try:
        rc = _lib.lib.ffgp_gemm_batched(h, 0, 0, 0, C.c_void_p(Ad.data_ptr()), k, m * k, C.c_void_p(Bd.data_ptr()), k, n * k,
                                        C.c_void_p(Cd.data_ptr()), n, m * n, m, n, k, -1.0, 1.0, 2)
        assert rc == 0, rc
        torch.cuda.synchronize()
    finally:
        opt(ff, "gemm_tile", 0.0)
    out = Cd.cpu().numpy()
    for f in range(2):
        single = gemm_sub(ff, 128, 0, A[f], (0, 0), B[f], (0, 0), C0[f], (0, 0), m, n, k)
        assert same_bits(out[f], single), f
        assert same_bits(out[f], gemm_sub(ff, 64, 0, A[f], (0, 0), B[f], (0, 0), C0[f], (0, 0), m, n, k)), f
        assert relerr(out[f], C0[f] - A[f] @ B[f].T) < 1e-13


def test_ragged_launch_against_single_calls(ff):
    """nlml_many of two d = 1 blocks of 640 and 768 points: after the 512-column panel their trailing updates (128 and 256 rows + the
    passenger row) share one ragged launch; each member's likelihood is its single call's bit for bit"""
    from fidelityfusion_amd import functional as F
    D, sizes = 4, (640, 768)
    gen = torch.Generator(device="cuda:0").manual_seed(sum(sizes))
    Xs, Ys, ws, amps, dadds = [], [], [], [], []
    for f, n in enumerate(sizes):
        X = torch.rand((n, D), generator=gen, device="cuda:0", dtype=torch.float64)
        Y = torch.sin(2.0 * np.pi * X.sum(1, keepdim=True)) + 0.1 * torch.randn((n, 1), generator=gen, device="cuda:0", dtype=torch.float64)
        Xs.append(X)
        Ys.append(Y.contiguous())
        ws.append(dev(np.full(D, 0.9 + 0.05 * f)))
        amps.append(dev([1.0 + 0.1 * f]))
        dadds.append(dev([np.exp(-1.0) + 1e-6]))
    opt(ff, "gemm_tile", 128.0)
    try:
        with torch.no_grad():
            many = F.nlml_many(Xs, Ys, ws, amps, dadds, clamp=1e-30).clone()
            single = [F.nlml(Xs[f], Ys[f], ws[f], amps[f], diag_add=dadds[f], clamp=1e-30) for f in range(2)]
    finally:
        opt(ff, "gemm_tile", 0.0)
    assert torch.isfinite(many).all()
    for f in range(2):
        assert torch.equal(many[f], single[f].reshape(())), (f, float(many[f]), float(single[f]))


def test_stage_reuse_under_contention(ff):
    """1024 tiles (more than two per CU), k = 80 (the k-tile without pieces and the peeled tail under load), five launches from the
    same inputs: a stage refilled under a slow wave's reads, or read before every wave's pieces landed, shows as a launch that differs
    from the 64-tile result"""
    rng = np.random.default_rng(80)
    n, k = 4096, 80
    A, B, C0 = rng.standard_normal((n, k)), rng.standard_normal((n, k)), rng.standard_normal((n, n))
    ref = gemm_sub(ff, 64, 0, A, (0, 0), B, (0, 0), C0, (0, 0), n, n, k)
    assert relerr(ref, C0 - A @ B.T) < 1e-13
    for i, out in enumerate(gemm_sub(ff, 128, 0, A, (0, 0), B, (0, 0), C0, (0, 0), n, n, k, launches=5)):
        assert same_bits(out, ref), "launch %d differs from the 64-tile result" % i
