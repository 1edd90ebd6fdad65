"""Light tiles of the 128-tile symmetric update (csrc/gemm.hip, option syrk_light_tiles): a last tile row of at most 32 rows -- the
passenger rows of a likelihood's factorisation, m = n + d -- runs as 16-row slabs at the end of the grid (gemm_slab16), and the
diagonal tiles run on the fast tile's rotated k loop without their strictly-upper quadrant (gemm_tile_fast128<.., DIAG>).  Both keep
the general tile's arithmetic, so everything here is compared bit for bit with syrk_light_tiles = 0, the path the library had before.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


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


@pytest.fixture
def tile128(ff):
    """small shapes reach the 128-tile (the launcher would give them the 64-tile)"""
    opt(ff, "gemm_tile", 128.0)
    yield
    opt(ff, "gemm_tile", 0.0)
    opt(ff, "syrk_light_tiles", 1.0)


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


def relerr(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


GUARD = 4          # rows below row m of C: a slab that stored its clamped rows would hit them
SENTINEL = -12345.678


def syrk(ff, light, A, Bt, C0, m, n, k, alpha=-1.0, beta=1.0, opa=0, opb=0, tri=0, lda=None, ldb=None):
    """C[:m] = alpha op(A) op(B) + beta C[:m] on the lower tiles; A [m, k] and Bt [n, k] K-major (or as opa / opb say); C0 carries
    GUARD more rows than m.  Returns the whole buffer."""
    _lib, h = ff
    opt(ff, "syrk_light_tiles", float(light))
    Ad, Bd, Cd = dev(A), dev(Bt), dev(C0)
    rc = _lib.lib.ffgp_gemm(h, opa, opb, 1, tri, C.c_void_p(Ad.data_ptr()), lda or A.shape[1], C.c_void_p(Bd.data_ptr()), ldb or Bt.shape[1],
                            C.c_void_p(Cd.data_ptr()), C0.shape[1], m, n, k, alpha, beta)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return Cd.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))      # (NaN-filled regions compare too)


_OPERANDS = {}


def operands(n, r, k):
    """one set of operands and its float64 reference per shape, shared by the tests"""
    key = (n, r, k)
    if key not in _OPERANDS:
        rng = np.random.default_rng(1000 * r + k + n)
        m = n + r
        A = rng.standard_normal((m, k))
        C0 = np.full((m + GUARD, n), SENTINEL)
        C0[:m] = rng.standard_normal((m, n))
        C0[:n][np.triu_indices(n, 1)] = np.nan
        ref = (torch.tensor(C0[:m]) - torch.tensor(A) @ torch.tensor(A[:n]).T).numpy()
        _OPERANDS[key] = (A, C0, ref)
    return _OPERANDS[key]


@pytest.mark.parametrize("k", [16, 32, 512])
@pytest.mark.parametrize("r", [0, 1, 2, 15, 16, 17, 32, 33, 64, 65, 127])
def test_edge_and_diagonal_tiles(ff, tile128, r, k):
    """n = 384 (three tile rows: diagonal tiles and interior tiles), m = 384 + r, alpha = -1, beta = 1; r on both sides of every slab
    count and of the cut-off (32 | 33; 64, 65 and 127 stay on the edge tile); k = 16 is the peeled last k-tile alone, 32 and 512 run the loops"""
    n, m = 384, 384 + r
    A, C0, ref = operands(n, r, k)
    on = syrk(ff, 1, A, A[:n], C0, m, n, k)
    off = syrk(ff, 0, A, A[:n], C0, m, n, k)
    assert same_bits(on, off), "light tiles changed the arithmetic"
    up = np.triu_indices(n, 1)
    assert np.isnan(on[:n][up]).all() and same_bits(on[:n][up], C0[:n][up]), "strictly-upper triangle was written"
    assert same_bits(on[m:], C0[m:]), "rows at or beyond m were written"
    low = np.tril(np.ones((m, n), dtype=bool))
    err = relerr(on[:m][low], ref[low])
    print("r = %d k = %d: relerr %.3e" % (r, k, err))
    assert err < 1e-13


@pytest.mark.parametrize("form", ["alpha_beta_half", "odd_lda", "triangular_k", "mn_major"])
def test_forms_that_keep_the_general_tiles(ff, tile128, form):
    """launches gemm_plan leaves alone give the same bits with the option on and off.  (An in-place product, C in A's buffer, exists
    only inside the factorisation -- full-rectangle launches, which the option never touches: the end-to-end test below runs them.)"""
    n, r, k = 384, 1, 48
    m = n + r
    rng = np.random.default_rng(7)
    A = rng.standard_normal((m, k))
    C0 = np.full((m + GUARD, n), SENTINEL)
    C0[:m] = rng.standard_normal((m, n))
    kw, Aop, Bop = {}, A, A[:n]
    if form == "alpha_beta_half":
        kw = dict(alpha=0.5, beta=0.5)
    elif form == "odd_lda":
        Aop = np.concatenate([A, np.full((m, 1), np.nan)], axis=1)      # lda = ldb = k + 1: 8-byte operand loads
        Bop = Aop[:n]
        kw = dict(lda=k + 1, ldb=k + 1)
    elif form == "triangular_k":      # the LAUUM's shape: X^T X of a lower-triangular X, both MN-major, k ranges cut per tile
        X = np.tril(rng.standard_normal((n, n)))
        m, k = n, n
        Aop, Bop = X, X
        C0 = np.full((m + GUARD, n), SENTINEL)
        C0[:m] = rng.standard_normal((m, n))
        kw = dict(opa=1, opb=1, tri=1)
    elif form == "mn_major":
        Aop, Bop = np.ascontiguousarray(A.T), np.ascontiguousarray(A[:n].T)
        kw = dict(opa=1, opb=1, lda=m, ldb=n)
    on = syrk(ff, 1, Aop, Bop, C0, m, n, k, **kw)
    off = syrk(ff, 0, Aop, Bop, C0, m, n, k, **kw)
    assert same_bits(on, off), form
    assert same_bits(on[m:], C0[m:])
    if form in ("alpha_beta_half", "odd_lda", "mn_major"):
        a, b = kw.get("alpha", -1.0), kw.get("beta", 1.0)
        low = np.tril(np.ones((m, n), dtype=bool))
        assert relerr(on[:m][low], (b * C0[:m] + a * A @ A[:n].T)[low]) < 1e-13


@pytest.mark.parametrize("r,k", [(1, 16), (0, 48)])
def test_split_tail_with_slabs(ff, r, k):
    """n = 2944, m = 2945: 276 whole tiles, 20 over a round of 256, so the tail splits into quarters -- and one row of slabs behind
    them.  Same bits as the general tiles, and as the unsplit launch.  (The quartered tiles include diagonal tiles: their
    strictly-lower quadrant must keep the general form's rounding.  m = 2944: the same without slabs.)"""
    n, m = 2944, 2944 + r
    rng = np.random.default_rng(2945)
    A = rng.standard_normal((m, k))
    C0 = np.full((m + GUARD, n), SENTINEL)
    C0[:m] = rng.standard_normal((m, n))
    opt(ff, "small_tile_threshold", 0.0)      # (299 tiles: the 128-tile without forcing it -- a forced tile never splits)
    try:
        on = syrk(ff, 1, A, A[:n], C0, m, n, k)
        off = syrk(ff, 0, A, A[:n], C0, m, n, k)
        opt(ff, "split_rem_max", 0.0)
        unsplit = syrk(ff, 1, A, A[:n], C0, m, n, k)
    finally:
        opt(ff, "split_rem_max", 180.0)
        opt(ff, "small_tile_threshold", 640.0)
        opt(ff, "syrk_light_tiles", 1.0)
    assert same_bits(on, off)
    assert same_bits(on, unsplit)
    assert same_bits(on[m:], C0[m:])
    low = np.tril(np.ones((m, n), dtype=bool))
    assert relerr(on[:m][low], (C0[:m] - A @ A[:n].T)[low]) < 1e-13
    assert same_bits(on[:m][~low], C0[:m][~low])


@pytest.mark.parametrize("d", [1, 3])
def test_potrf_with_passenger_rows(ff, tile128, d):
    """the factorisation of [Sigma; Y^T] (N = 1536, d passenger rows) with every GEMM on the 128-tile: factor and Gamma bit for bit
    those of the general tiles, and LAPACK's to the tolerances of test_gpu_kernels.py"""
    import scipy.linalg as sla
    _lib, h = ff
    n = 1536
    rng = np.random.default_rng(n + d)
    B = rng.standard_normal((n, 56))
    S = B @ B.T + np.diag(rng.random(n) + 0.5)
    R = rng.standard_normal((d, n))
    ld = n + 2
    W = np.full((n + d, ld), np.nan)
    W[:n, :n] = np.tril(S) + np.triu(np.full((n, n), 777.0), 1)
    W[n:, :n] = R
    outs = {}
    for on in (1, 0):
        opt(ff, "syrk_light_tiles", float(on))
        Wd = dev(W)
        assert _lib.lib.ffgp_potrf_rows(h, C.c_void_p(Wd.data_ptr()), n, n + d, ld) == 0
        outs[on] = Wd.cpu().numpy()
    assert same_bits(outs[1], outs[0])
    L = np.linalg.cholesky(S)
    assert relerr(np.tril(outs[1][:n, :n]), L) < 1e-11
    assert relerr(outs[1][n:, :n], sla.solve_triangular(L, R.T, lower=True).T) < 1e-10
    assert (outs[1][:n, :n][np.triu_indices(n, 1)] == 777.0).all(), "strictly-upper triangle was written"


@pytest.mark.parametrize("sizes", [(640, 640), (640, 896)])
def test_two_members_in_one_call(ff, tile128, sizes):
    """nlml_many of two d = 1 blocks (one shape: the batched chain; two shapes: the ragged chain) against the two single calls: every
    member's launches are planned as its own single call plans them"""
    from fidelityfusion_amd import functional as F
    D = 4
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
    with torch.no_grad():
        many = F.nlml_many(Xs, Ys, ws, amps, dadds, clamp=1e-30).clone()
        single = [F.nlml(Xs[f], Ys[f], ws[f], amps[f], diag_add=dadds[f], clamp=1e-30) for f in range(2)]
        opt(ff, "syrk_light_tiles", 0.0)
        general = [F.nlml(Xs[f], Ys[f], ws[f], amps[f], diag_add=dadds[f], clamp=1e-30) for f in range(2)]
    assert torch.isfinite(many).all()
    for f in range(2):
        assert torch.equal(many[f], single[f].reshape(())), (f, float(many[f]), float(single[f]))
        assert torch.equal(single[f], general[f]), f
