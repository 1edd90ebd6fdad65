"""GPU: the handle's two stores of pre-inverted blocks (`dinv`: 128 x 128 diagonal blocks, `sinv`: S x S super-blocks) across buffers,
handles and refills.  Every triangular solve reads them, and they are keyed on (address, n, ld) alone: a key that matches while the
buffer holds another factor gives a solve that is wrong by O(1) without any error.  The contract is in include/ffgp.h
(ffgp_trtri_diag / ffgp_invalidate); these tests drive it from the C ABI at FIXED addresses (one arena, two slots P and Q: whether an
address is reused is decided here, not by an allocator), from a small model of the key bookkeeping over random legal sequences, and
from the Python layer (conditional_gaussian's backward, a Posterior queried from another handle slot).  The last part tests
ffgp_gemm_batched -- the launch form that builds the super-block levels -- beyond the one shape the eigensolver gives it.

References: scipy / numpy in fp64 on the CPU.  Tolerance of the solves and of ffgp_potri: relerr < 1e-9, the one
test_trsm_super_block_sweeps and test_potri (test_gpu_kernels.py) apply to the same operations on the same cond-1e3 generator; a
stale store is wrong by O(1)."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NMAX = 1100                    # largest factor of this file
LD = 1104                      # default leading dimension at both slots: even, different from every n used
SLOT = NMAX * (LD + 2)         # doubles per arena slot (room for ld = LD + 2); even, so slot Q is 16-byte aligned like P
P, Q = 0, 1
TOL = 1e-9
DEVICE = "cuda:0"
NRHS = (1, 5, 70)              # matrix-vector, skinny and tile kernels
SOLVES = ("trsm", "trsm_t", "potrs")


@pytest.fixture(scope="module")
def ff():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fidelityfusion_amd import _lib
    return _lib


def handles(_lib):
    """(H0, H1): handle slots 0 and 1 of cuda:0, both bound to the current torch stream"""
    hs = []
    for slot in (0, 1):
        h = _lib.handle(0, slot=slot)
        _lib.bind_stream(h, 0)
        hs.append(h)
    return hs


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEVICE)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def relerr(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def spd(n, rng, cond=1e3):
    Q_, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.logspace(0, np.log10(cond), n)
    return (Q_ * ev) @ Q_.T


# ------------------------------------------------------------------------------------------------ factors and their numpy twins
@functools.lru_cache(maxsize=None)
def family(seed, N):
    """(A, chol(A)) for A = spd(N, rng(seed)), computed once per (seed, N) and never modified.  The leading n x n block of A is SPD with
    cond <= cond(A), and its Cholesky factor is the leading block of chol(A): one family serves a factor and every legal growth of it."""
    A = spd(N, np.random.default_rng(7000 + 13 * seed + N))
    L = np.linalg.cholesky(A)
    A.setflags(write=False)
    L.setflags(write=False)
    return A, L


@functools.lru_cache(maxsize=None)
def _inv_tril(seed, N, n):
    return np.tril(np.linalg.inv(family(seed, N)[0][:n, :n]))


class Fac:
    """the numpy twin of a factor: the leading n rows of family (seed, N)"""

    def __init__(self, seed, n, N=None):
        self.seed, self.n, self.N = seed, n, N or n
        A, L = family(seed, self.N)
        self.A, self.L = A[:n, :n], L[:n, :n]

    def grown(self, n1):
        return Fac(self.seed, n1, self.N)

    def inv_tril(self):
        return _inv_tril(self.seed, self.N, self.n)

    def __repr__(self):
        return "fac(seed=%d, n=%d of %d)" % (self.seed, self.n, self.N)


class Arena:
    """one device allocation with two fixed slots; a factor lives at a slot's first byte with an explicit leading dimension"""

    def __init__(self):
        self.buf = torch.empty(2 * SLOT, dtype=torch.float64, device=DEVICE)
        assert self.buf.data_ptr() % 16 == 0 and (SLOT * 8) % 16 == 0

    def addr(self, s):
        return C.c_void_p(self.buf.data_ptr() + 8 * s * SLOT)

    def view(self, s, rows, ld):
        assert rows * ld <= SLOT and ld % 2 == 0
        return self.buf[s * SLOT:s * SLOT + rows * ld].view(rows, ld)

    def upload(self, s, f, ld):
        """a factor the handles have never seen: np.linalg.cholesky(A), zeros above the diagonal and in the padding"""
        W = np.zeros((f.n, ld))
        W[:, :f.n] = f.L
        self.view(s, f.n, ld).copy_(dev(W))
        torch.cuda.synchronize()

    def grow(self, s, f0, f1, ld):
        """rows f0.n .. f1.n - 1 of the larger factor below the untouched leading rows"""
        assert f1.seed == f0.seed and f1.N == f0.N and f1.n > f0.n
        W = np.zeros((f1.n - f0.n, ld))
        W[:, :f1.n] = f1.L[f0.n:, :]
        self.view(s, f1.n, ld)[f0.n:] = dev(W)
        torch.cuda.synchronize()

    def potrf(self, _lib, h, s, f, ld):
        W = np.zeros((f.n, ld))
        W[:, :f.n] = np.tril(f.A)
        self.view(s, f.n, ld).copy_(dev(W))
        assert _lib.lib.ffgp_potrf(h, self.addr(s), f.n, ld) == 0
        torch.cuda.synchronize()

    def tril(self, s, n, ld):
        return np.tril(self.view(s, n, ld)[:, :n].cpu().numpy())


def solve_fn(_lib, which):
    return {"trsm": _lib.lib.ffgp_trsm_lower, "trsm_t": _lib.lib.ffgp_trsm_lower_t, "potrs": _lib.lib.ffgp_potrs}[which]


def solve_ref(which, L, B):
    import scipy.linalg as sla
    if which == "trsm":
        return sla.solve_triangular(L, B, lower=True)
    if which == "trsm_t":
        return sla.solve_triangular(L.T, B, lower=False)
    return sla.cho_solve((L, True), B)


def run_solve(_lib, h, which, addr, n, ld, B):
    """one solve on a NaN-padded right-hand side (ldb = nrhs + 3): nothing may land in the padding"""
    nrhs = B.shape[1]
    Bp = np.full((n, nrhs + 3), np.nan)
    Bp[:, :nrhs] = B
    Bd = dev(Bp)
    assert solve_fn(_lib, which)(h, addr, n, ld, ptr(Bd), nrhs, nrhs + 3) == 0
    torch.cuda.synchronize()
    got = Bd.cpu().numpy()
    assert np.isnan(got[:, nrhs:]).all(), "solve wrote into the ldb padding"
    return got[:, :nrhs]


def check_solve(_lib, h, arena, s, f, ld, which, nrhs, rng, tag=""):
    B = rng.standard_normal((f.n, nrhs))
    err = relerr(run_solve(_lib, h, which, arena.addr(s), f.n, ld, B), solve_ref(which, f.L, B))
    assert err < TOL, "%s: %s nrhs=%d at slot %d, %r ld=%d: relerr %.3e" % (tag, which, nrhs, s, f, ld, err)


def check_solves(_lib, h, arena, s, f, ld, rng, tag=""):
    for which in SOLVES:
        for nrhs in NRHS:
            check_solve(_lib, h, arena, s, f, ld, which, nrhs, rng, tag)


def check_potri(_lib, h, arena, s, f, ld, tag=""):
    assert _lib.lib.ffgp_potri(h, arena.addr(s), f.n, ld) == 0
    torch.cuda.synchronize()
    err = relerr(arena.tril(s, f.n, ld), f.inv_tril())
    assert err < TOL, "%s: potri at slot %d, %r ld=%d: relerr %.3e" % (tag, s, f, ld, err)


def set_opt(_lib, h, key, val):
    assert _lib.lib.ffgp_set_option(h, key.encode(), float(val)) == 0, key


@contextlib.contextmanager
def solve_path(_lib, path):
    """path "blk": the library's defaults (128-block sweeps at these sizes); "sup": super-block sweeps with S = 256 from n = 1 on.
    The defaults come back in the `finally`, on both handles."""
    hs = handles(_lib)
    try:
        if path == "sup":
            for h in hs:
                set_opt(_lib, h, "super_block", 256)
                set_opt(_lib, h, "super_min_n", 1)
        yield hs
    finally:
        for h in hs:
            _lib.lib.ffgp_set_option(h, b"super_block", 1024.0)
            _lib.lib.ffgp_set_option(h, b"super_min_n", 2048.0)
            _lib.lib.ffgp_set_option(h, b"naive", 0.0)


def announce(_lib, h, via, arena, s, n, ld):
    """the two legal ways to tell a handle that a keyed buffer changed behind its back"""
    if via == "trtri_diag":
        assert _lib.lib.ffgp_trtri_diag(h, arena.addr(s), n, ld) == 0
    else:
        assert _lib.lib.ffgp_invalidate(h) == 0


PATHS = ("blk", "sup")
VIAS = ("trtri_diag", "invalidate")


# ------------------------------------------------------------------------------------------------ A. directed tests
@pytest.mark.parametrize("path,cases", [("blk", [(100, 100), (130, 132), (129, 130), (300, 306), (301, 302), (384, 384), (500, LD), (700, 700)]),
                                        ("sup", [(300, 300), (301, 306), (700, LD), (1100, 1100), (1099, LD)])])
def test_foreign_factor_never_seen_by_the_handle(ff, path, cases):
    """A.1: np.linalg.cholesky output uploaded at a slot, no ffgp_potrf / ffgp_trtri_diag before: each of trsm_lower, trsm_lower_t,
    potrs and potri is in turn the FIRST call that meets the factor (a new factor at the other slot each time, so the handle's key
    names another address: legal without a call), with ld == n, ld != n and odd n"""
    arena = Arena()
    rng = np.random.default_rng(1)
    with solve_path(ff, path) as (h0, _):
        for n, ld in cases:
            for i, first in enumerate(SOLVES + ("potri",)):
                s = i % 2
                f = Fac(10 + i, n)
                arena.upload(s, f, ld)
                tag = "A.1 %s first=%s" % (path, first)
                if first == "potri":
                    check_potri(ff, h0, arena, s, f, ld, tag)
                else:
                    check_solve(ff, h0, arena, s, f, ld, first, 5, rng, tag)
                    check_solves(ff, h0, arena, s, f, ld, rng, tag)


@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("path,sizes", [("blk", (100, 130, 300, 384, 500, 700)), ("sup", (300, 700, 1100))])
def test_same_address_same_n_new_contents(ff, path, sizes, via):
    """A.2: a solve keys the store at (P, n, ld); P is refilled with another factor of the same n; after ffgp_trtri_diag (or
    ffgp_invalidate) the solves follow the new factor"""
    arena = Arena()
    rng = np.random.default_rng(2)
    with solve_path(ff, path) as (h0, _):
        for n in sizes:
            f = Fac(20, n)
            arena.upload(P, f, LD)
            announce(ff, h0, "invalidate", arena, P, n, LD)      # (whatever an earlier size left behind at P)
            check_solves(ff, h0, arena, P, f, LD, rng, "A.2 %s keying" % path)
            g = Fac(21, n)
            arena.upload(P, g, LD)
            announce(ff, h0, via, arena, P, n, LD)
            check_solves(ff, h0, arena, P, g, LD, rng, "A.2 %s after refill + %s" % (path, via))


@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("keyed_by", ["potrf", "solve"])
@pytest.mark.parametrize("path,n0,n1", [("blk", 300, 500), ("sup", 700, 1100)])
def test_same_address_more_rows_unrelated_contents(ff, path, n0, n1, keyed_by, via):
    """A.3: the store is keyed at (P, n0, ld) -- by ffgp_potrf, or by a solve on an uploaded factor -- then P is refilled with an
    UNRELATED factor of n1 > n0 rows at the same ld.  After ffgp_trtri_diag(P, n1, ld) (or ffgp_invalidate) the solves follow the new
    factor.  Before ffgp_trtri_diag dropped the keys first, it took the "factor only grew" route here and kept the old factor's
    leading n0 / 128 diagonal-block inverses (and leading super-blocks): on that library the four ffgp_trtri_diag cases failed at
    their first solve with relerr 1.357e+00 (blk, 300 -> 500) and 2.197e+00 (sup, 700 -> 1100); the ffgp_invalidate cases passed."""
    arena = Arena()
    rng = np.random.default_rng(3)
    with solve_path(ff, path) as (h0, _):
        f = Fac(30, n0)
        assert ff.lib.ffgp_invalidate(h0) == 0
        if keyed_by == "potrf":
            arena.potrf(ff, h0, P, f, LD)
        else:
            arena.upload(P, f, LD)
        check_solves(ff, h0, arena, P, f, LD, rng, "A.3 %s keyed by %s" % (path, keyed_by))
        g = Fac(31, n1)
        arena.upload(P, g, LD)
        announce(ff, h0, via, arena, P, n1, LD)
        check_solves(ff, h0, arena, P, g, LD, rng, "A.3 %s %d -> %d after %s" % (path, n0, n1, via))


@pytest.mark.parametrize("path,big,small", [("blk", 500, 300), ("sup", 1100, 700)])
def test_fewer_rows_and_another_ld_at_the_same_address(ff, path, big, small):
    """A.4: `big` rows then `small` rows at the same ld; `small` rows at ld and then at ld + 2: refill, ffgp_trtri_diag, solves"""
    arena = Arena()
    rng = np.random.default_rng(4)
    with solve_path(ff, path) as (h0, _):
        f = Fac(40, big)
        arena.upload(P, f, LD)
        assert ff.lib.ffgp_invalidate(h0) == 0
        check_solves(ff, h0, arena, P, f, LD, rng, "A.4 %s keying at %d" % (path, big))
        g = Fac(41, small)
        arena.upload(P, g, LD)
        announce(ff, h0, "trtri_diag", arena, P, small, LD)
        check_solves(ff, h0, arena, P, g, LD, rng, "A.4 %s %d -> %d" % (path, big, small))
        k = Fac(42, small)
        arena.upload(P, k, LD + 2)
        announce(ff, h0, "trtri_diag", arena, P, small, LD + 2)
        check_solves(ff, h0, arena, P, k, LD + 2, rng, "A.4 %s ld -> ld + 2" % path)


@pytest.mark.parametrize("keyed_by", ["potrf", "solve"])
@pytest.mark.parametrize("path,n0,n1,n2", [("blk", 130, 300, 500), ("blk", 256, 384, 700), ("blk", 300, 500, 700),
                                           ("sup", 300, 700, 1100), ("sup", 512, 700, 1100)])
def test_legal_growth_without_a_call(ff, path, n0, n1, n2, keyed_by):
    """A.5 (what Posterior.append does): the store is keyed at (P, n0); the rows n0 .. n1 - 1 of the Cholesky factor of a larger SPD
    matrix with the same leading block (computed on the CPU) are written below the untouched leading rows; the solves at (P, n1) need
    no call -- the incremental rebuild of both stores.  Twice in a row."""
    arena = Arena()
    rng = np.random.default_rng(5)
    with solve_path(ff, path) as (h0, _):
        f0 = Fac(50, n0, n2)
        assert ff.lib.ffgp_invalidate(h0) == 0
        if keyed_by == "potrf":
            arena.potrf(ff, h0, P, f0, LD)
            assert relerr(arena.tril(P, n0, LD), f0.L) < 1e-11
        else:
            arena.upload(P, f0, LD)
            check_solves(ff, h0, arena, P, f0, LD, rng, "A.5 %s keying at %d" % (path, n0))
        f1 = f0.grown(n1)
        arena.grow(P, f0, f1, LD)
        check_solves(ff, h0, arena, P, f1, LD, rng, "A.5 %s grown %d -> %d" % (path, n0, n1))
        f2 = f1.grown(n2)
        arena.grow(P, f1, f2, LD)
        check_solves(ff, h0, arena, P, f2, LD, rng, "A.5 %s grown %d -> %d" % (path, n1, n2))


@pytest.mark.parametrize("path,n", [("blk", 300), ("blk", 500), ("sup", 700)])
def test_potri_consumes_the_factor(ff, path, n):
    """A.6: ffgp_potrf at P, ffgp_potri (the inverse is checked), then a new factor of the same n uploaded at P: ffgp_potri cleared the
    keys, so the solves follow the new factor without any call"""
    arena = Arena()
    rng = np.random.default_rng(6)
    with solve_path(ff, path) as (h0, _):
        f = Fac(60, n)
        arena.potrf(ff, h0, P, f, LD)
        check_solve(ff, h0, arena, P, f, LD, "potrs", 5, rng, "A.6 %s before potri" % path)     # (both stores exist and name P)
        check_potri(ff, h0, arena, P, f, LD, "A.6 %s" % path)
        g = Fac(61, n)
        arena.upload(P, g, LD)
        check_solves(ff, h0, arena, P, g, LD, rng, "A.6 %s new factor after potri, no call" % path)


@pytest.mark.parametrize("refill", [False, True])
@pytest.mark.parametrize("kind", ["super_block", "super_min_n", "naive"])
def test_options_between_solves(ff, kind, refill):
    """A.7: an option changes between two solves at (P, 700): super_block 256 -> 512; super_min_n so that n leaves the super path,
    and back; naive 1 and back to 0.  Every step once on the unchanged factor, once after a refill + ffgp_trtri_diag."""
    arena = Arena()
    rng = np.random.default_rng(7)
    n = 700
    steps = {"super_block": [("super_block", 512)], "super_min_n": [("super_min_n", 2048), ("super_min_n", 1)],
             "naive": [("naive", 1), ("naive", 0)]}[kind]
    with solve_path(ff, "sup") as (h0, _):
        f = Fac(70, n)
        arena.upload(P, f, LD)
        assert ff.lib.ffgp_invalidate(h0) == 0
        check_solves(ff, h0, arena, P, f, LD, rng, "A.7 %s on the super path" % kind)
        for i, (key, val) in enumerate(steps):
            set_opt(ff, h0, key, val)
            if refill:
                f = Fac(71 + i, n)
                arena.upload(P, f, LD)
                announce(ff, h0, "trtri_diag", arena, P, n, LD)
            check_solves(ff, h0, arena, P, f, LD, rng, "A.7 after %s = %d%s" % (key, val, ", refill + trtri_diag" if refill else ""))


def _fused_call(_lib, kind, slot):
    """one small fused call on handle `slot`: it factors in the handle's own workspace and re-keys the store to it"""
    from fidelityfusion_amd import functional as F
    g = torch.Generator(device=DEVICE).manual_seed(8)
    if kind == "train":
        from fidelityfusion_amd import kernel
        from fidelityfusion_amd.cigp_v10 import cigp, train_many
        X = torch.rand((64, 2), generator=g, device=DEVICE, dtype=torch.float64)
        Y = torch.randn((64, 1), generator=g, device=DEVICE, dtype=torch.float64)
        m = cigp(kernel.ARDKernel(2), 0.6).double().to("cuda:0")
        with _lib.thread_slot(slot):
            trace, _ = train_many([m], [X], [Y], 3, lr=1e-2)
        assert torch.isfinite(trace).all()
        return
    X = torch.rand((200, 2), generator=g, device=DEVICE, dtype=torch.float64)
    Y = torch.randn((200, 1), generator=g, device=DEVICE, dtype=torch.float64)
    w = torch.full((2,), 1.3, device=DEVICE, dtype=torch.float64, requires_grad=(kind == "nlml"))
    amp = torch.tensor([0.9], device=DEVICE, dtype=torch.float64)
    dadd = torch.tensor([0.05], device=DEVICE, dtype=torch.float64)
    if kind == "nlml":
        v = F.nlml(X, Y, w, amp, diag_add=dadd, clamp=1e-30, slot=slot)
        v.backward()
        assert torch.isfinite(v) and torch.isfinite(w.grad).all()
    else:
        with _lib.thread_slot(slot):
            mean, var = F.predict(X, Y, X[:7], w, amp, diag_add=dadd, clamp=1e-30)
        assert torch.isfinite(mean).all() and torch.isfinite(var).all()
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["nlml", "predict", "train"])
@pytest.mark.parametrize("path,n", [("blk", 300), ("sup", 700)])
def test_fused_call_between_two_solves(ff, path, n, kind):
    """A.8: solve at P; one small fused call on the same handle (ffgp_nlml_fused n = 200, D = 2, d = 1 / ffgp_predict / three steps of
    ffgp_train_raw on one n = 64 model); solve at P again"""
    arena = Arena()
    rng = np.random.default_rng(8)
    with solve_path(ff, path) as (h0, _):
        f = Fac(80, n)
        arena.upload(P, f, LD)
        assert ff.lib.ffgp_invalidate(h0) == 0
        check_solves(ff, h0, arena, P, f, LD, rng, "A.8 %s before %s" % (path, kind))
        _fused_call(ff, kind, 0)
        h0, _ = handles(ff)
        check_solves(ff, h0, arena, P, f, LD, rng, "A.8 %s after %s" % (path, kind))


@pytest.mark.parametrize("path,n", [("blk", 300), ("blk", 384), ("sup", 700)])
def test_two_buffers_alternating(ff, path, n):
    """A.9: factors of equal n and ld at P and Q, solved P, Q, P, Q: each solve gives its own reference"""
    arena = Arena()
    rng = np.random.default_rng(9)
    with solve_path(ff, path) as (h0, _):
        fs = {P: Fac(90, n), Q: Fac(91, n)}
        for s, f in fs.items():
            arena.upload(s, f, LD)
        assert ff.lib.ffgp_invalidate(h0) == 0
        for which in SOLVES:
            for nrhs in NRHS:
                for s in (P, Q, P, Q):
                    check_solve(ff, h0, arena, s, fs[s], LD, which, nrhs, rng, "A.9 %s" % path)


@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("path,n", [("blk", 300), ("sup", 700)])
def test_two_handles_one_buffer(ff, path, n, via):
    """A.10: H1 factors at P; H0 solves there (legal: H0's key is elsewhere); H1 factors a new matrix of the same n at P; H0 calls
    ffgp_trtri_diag (or ffgp_invalidate) and solves.  The device is synchronised between the handles' calls: this is about keys."""
    arena = Arena()
    rng = np.random.default_rng(10)
    with solve_path(ff, path) as (h0, h1):
        assert ff.lib.ffgp_invalidate(h0) == 0
        f = Fac(100, n)
        arena.potrf(ff, h1, P, f, LD)
        assert relerr(arena.tril(P, n, LD), f.L) < 1e-11
        check_solves(ff, h0, arena, P, f, LD, rng, "A.10 %s H0 on H1's factor" % path)
        g = Fac(101, n)
        arena.potrf(ff, h1, P, g, LD)
        announce(ff, h0, via, arena, P, n, LD)
        check_solves(ff, h0, arena, P, g, LD, rng, "A.10 %s H0 after H1 re-factored + %s" % (path, via))
        check_solves(ff, h1, arena, P, g, LD, rng, "A.10 %s H1 on its own factor" % path)


# ------------------------------------------------------------------------------------------------ B. model-based sequences
KINDS = ("F", "U", "G", "TD", "INV", "S", "PI", "OPT", "X")
_WEIGHTS = (0.11, 0.15, 0.12, 0.06, 0.06, 0.30, 0.06, 0.08, 0.06)
SEQ_SIZES = (100, 130, 300, 384, 500, 700, 1100)
SEQ_LDS = (LD, LD + 2)
SEQ_FAMILIES = 4               # families (seed, NMAX): every factor of the sequences is a leading block of one of them
SEQ_SEEDS = (57, 143, 161, 203, 252, 285, 324, 373)      # chosen on the CPU: test_sequence_generator_meets_the_coverage_floors
SEQ_OPS = 40
FLOORS = {"after_TD": 5, "after_INV": 5, "after_G": 5, "more_rows": 3, "h0_on_h1": 5}


def gen_sequence(seed, nops=SEQ_OPS):
    """A random sequence of operations that the contract of include/ffgp.h allows, from a model of (a) what each arena slot holds and
    (b) what each handle's store is keyed on:
        F(h, s, fam, n, ld)  ffgp_potrf of a fresh matrix         U(s, fam, n, ld)  upload of a CPU factor
        G(s, k)              legal growth by k rows               TD(h, s) / INV(h) ffgp_trtri_diag / ffgp_invalidate
        S(h, s, which, nrhs) a solve                              PI(h, s)          ffgp_potri (the slot then holds no factor)
        OPT(h, key, value)   super path on / off, S = 256 / 512   X(h)              a small ffgp_nlml_fused on that handle
    Model of the keys: F, TD and every solve leave handle h keyed on (s, n); PI, INV and X leave it keyed on nothing that the arena
    holds.  After a U, or an F / PI by the OTHER handle, onto a slot that a handle's key names, that handle is `stale`: before its
    next consumer (S, PI) at that slot the generator inserts TD or INV on it, picked at random.  Nothing is inserted after G.
    Returns (ops, coverage counts)."""
    rng = np.random.default_rng(seed)
    slots = [None, None]        # {"fam", "n", "ld", "writer"}
    key = [None, None]          # per handle: {"s", "n"}
    stale = [False, False]
    last = [None, None]         # per handle: ("TD", s) / ("INV",) right after such a call, else None
    sup = [{"on": False, "S": 256}, {"on": False, "S": 256}]
    ops = []
    cov = {k: 0 for k in FLOORS}
    cov["kinds"] = set()

    def emit(op):
        ops.append(op)
        cov["kinds"].add(op[0])

    def written(s, n, by):
        for g in (0, 1):
            if g != by and key[g] is not None and key[g]["s"] == s:
                stale[g] = True
                if n is not None and n > key[g]["n"]:
                    cov["more_rows"] += 1

    def consumer(h, s):
        if key[h] is not None and key[h]["s"] == s and stale[h]:
            if rng.random() < 0.5:
                emit(("TD", h, s))
                key[h], last[h] = {"s": s, "n": slots[s]["n"]}, ("TD", s)
            else:
                emit(("INV", h))
                key[h], last[h] = None, ("INV",)
            stale[h] = False
        if last[h] == ("TD", s):
            cov["after_TD"] += 1
        elif last[h] == ("INV",):
            cov["after_INV"] += 1
        if key[h] is not None and key[h]["s"] == s and key[h]["n"] < slots[s]["n"]:
            cov["after_G"] += 1
        if h == 0 and slots[s]["writer"] == 1:
            cov["h0_on_h1"] += 1
        last[h] = None

    while len(ops) < nops:
        kind = KINDS[int(rng.choice(len(KINDS), p=_WEIGHTS))]
        h, s = int(rng.integers(2)), int(rng.integers(2))
        if kind in ("F", "U"):
            n = int(rng.choice(SEQ_SIZES))
            keyed = [key[g]["n"] for g in (0, 1) if key[g] is not None and key[g]["s"] == s]
            if keyed and rng.random() < 0.5:        # bias: more rows than a key at this address names
                larger = [m for m in SEQ_SIZES if m > min(keyed)]
                if larger:
                    n = int(rng.choice(larger))
            fam, ld = int(rng.integers(SEQ_FAMILIES)), int(rng.choice(SEQ_LDS))
            if kind == "F":
                emit(("F", h, s, fam, n, ld))
                written(s, n, h)
                key[h], stale[h], last[h] = {"s": s, "n": n}, False, None
                slots[s] = {"fam": fam, "n": n, "ld": ld, "writer": h}
            else:
                emit(("U", s, fam, n, ld))
                written(s, n, None)
                slots[s] = {"fam": fam, "n": n, "ld": ld, "writer": None}
        elif kind == "G":
            named = [key[g]["s"] for g in (0, 1) if key[g] is not None and not stale[g] and slots[key[g]["s"]] is not None]
            if named and rng.random() < 0.7:        # bias: a factor that a handle's key names
                s = named[int(rng.integers(len(named)))]
            if slots[s] is None or slots[s]["n"] >= NMAX:
                continue
            room = NMAX - slots[s]["n"]
            k = int(min(room, rng.choice([1, 60, 128, 200, 400])))
            emit(("G", s, k))
            slots[s]["n"] += k
        elif kind == "TD":
            if slots[s] is None:
                continue
            emit(("TD", h, s))
            key[h], stale[h], last[h] = {"s": s, "n": slots[s]["n"]}, False, ("TD", s)
        elif kind == "INV":
            emit(("INV", h))
            key[h], stale[h], last[h] = None, False, ("INV",)
        elif kind == "S":
            if slots[s] is None:
                continue
            # bias: the consumers the bookkeeping has to get right -- a handle on a factor that grew since it keyed it, right after its
            # TD / INV, on a refilled slot its key names (a TD / INV gets inserted), and the first handle on what the second one wrote
            cands = []
            for hh in (0, 1):
                for ss in (0, 1):
                    if slots[ss] is None:
                        continue
                    here = key[hh] is not None and key[hh]["s"] == ss
                    if here and (stale[hh] or key[hh]["n"] < slots[ss]["n"]):
                        cands.append((hh, ss))
                    if last[hh] in (("TD", ss), ("INV",)):
                        cands.append((hh, ss))
                    if hh == 0 and slots[ss]["writer"] == 1:
                        cands.append((hh, ss))
            if cands and rng.random() < 0.6:
                h, s = cands[int(rng.integers(len(cands)))]
            consumer(h, s)
            emit(("S", h, s, SOLVES[int(rng.integers(3))], int(rng.choice(NRHS))))
            key[h] = {"s": s, "n": slots[s]["n"]}
        elif kind == "PI":
            if slots[s] is None:
                continue
            consumer(h, s)
            emit(("PI", h, s))
            key[h] = None
            written(s, None, h)
            slots[s] = None
        elif kind == "OPT":
            if rng.random() < 0.6:
                sup[h]["on"] = not sup[h]["on"]
                emit(("OPT", h, "super_min_n", 1 if sup[h]["on"] else 2048))
            else:
                sup[h]["S"] = 768 - sup[h]["S"]
                emit(("OPT", h, "super_block", sup[h]["S"]))
            last[h] = None
        else:
            emit(("X", h))
            key[h], stale[h], last[h] = None, False, None
    return ops, cov


def fmt_op(op):
    return "%s(%s)" % (op[0], ", ".join(str(a) for a in op[1:]))


def test_sequence_generator_meets_the_coverage_floors():
    """B (no launch): the eight seeds were chosen on the CPU (the best of seeds 1 .. 399) so that the generated sequences exercise the
    state machine.  A sequence of 40 operations cannot hold all the floors by itself, so they are asserted over the eight sequences
    together: at least 5 consumers right after a TD, 5 right after an INV, 5 on a factor that grew since the handle keyed it, 3
    refills that put MORE rows at a keyed address, 5 consumers of H0 on a slot that H1 wrote last (the eight give 21 / 22 / 14 / 32 /
    43).  Every single sequence has every operation kind, at least one of each of the five, and at least 40 operations."""
    total = {k: 0 for k in FLOORS}
    for seed in SEQ_SEEDS:
        ops, cov = gen_sequence(seed)
        assert len(ops) >= SEQ_OPS
        assert cov["kinds"] == set(KINDS), (seed, sorted(set(KINDS) - cov["kinds"]))
        for k in FLOORS:
            assert cov[k] >= 1, (seed, k)
            total[k] += cov[k]
    for k, floor in FLOORS.items():
        assert total[k] >= floor, (k, total)


@pytest.mark.parametrize("seed", SEQ_SEEDS)
def test_random_legal_sequences_against_the_model(ff, seed):
    """B: the library and the numpy model go through the same generated sequence; after every consumer the result is compared with
    the reference of what the model says the slot holds.  On a failure the operation log up to the failing step is printed."""
    ops, cov = gen_sequence(seed)
    assert cov["kinds"] == set(KINDS)
    arena = Arena()
    rng = np.random.default_rng(100 + seed)
    held = [None, None]          # (Fac, ld)
    log = []
    with solve_path(ff, "blk") as hs:
        for h in hs:
            assert ff.lib.ffgp_invalidate(h) == 0
            set_opt(ff, h, "super_block", 256)       # (the super path itself is off until an OPT lowers super_min_n)
            set_opt(ff, h, "super_min_n", 2048)
        try:
            for step, op in enumerate(ops):
                log.append("%2d %s" % (step, fmt_op(op)))
                kind = op[0]
                if kind == "F":
                    _, h, s, fam, n, ld = op
                    held[s] = (Fac(fam, n, NMAX), ld)
                    arena.potrf(ff, hs[h], s, held[s][0], ld)
                elif kind == "U":
                    _, s, fam, n, ld = op
                    held[s] = (Fac(fam, n, NMAX), ld)
                    arena.upload(s, held[s][0], ld)
                elif kind == "G":
                    _, s, k = op
                    f0, ld = held[s]
                    held[s] = (f0.grown(f0.n + k), ld)
                    arena.grow(s, f0, held[s][0], ld)
                elif kind == "TD":
                    _, h, s = op
                    assert ff.lib.ffgp_trtri_diag(hs[h], arena.addr(s), held[s][0].n, held[s][1]) == 0
                elif kind == "INV":
                    assert ff.lib.ffgp_invalidate(hs[op[1]]) == 0
                elif kind == "S":
                    _, h, s, which, nrhs = op
                    check_solve(ff, hs[h], arena, s, held[s][0], held[s][1], which, nrhs, rng, "step %d" % step)
                elif kind == "PI":
                    _, h, s = op
                    check_potri(ff, hs[h], arena, s, held[s][0], held[s][1], "step %d" % step)
                    held[s] = None
                elif kind == "OPT":
                    set_opt(ff, hs[op[1]], op[2], op[3])
                else:
                    _fused_call(ff, "nlml", op[1])
                    hs = handles(ff)
                torch.cuda.synchronize()
        except AssertionError as e:
            raise AssertionError("seed %d failed at step %d: %s\noperations so far:\n%s" % (seed, len(log) - 1, e, "\n".join(log))) from None


# ------------------------------------------------------------------------------------------------ C. the Python layer
def _same_key_as_round_before(keys):
    return [i for i in range(1, len(keys)) if keys[i] == keys[i - 1]]


def test_conditional_gaussian_backward_after_a_forward_on_another_slot(ff):
    """C.1: conditional_gaussian with the forward under thread_slot(1) (the documented threaded_blocks order) and the backward from
    the caller, which solves on slot 0 with L = tril(W[:n, :n]) -- a copy at its own address with ld = n that no handle factored.
    Four rounds, a new Sigma each (exp kernel of random points + 0.3 I), n = 300, d = 2, nt = 5; gradients w.r.t. y, Sigma, K_s, K_ss
    against torch CPU autograd of  mu = K_s^T Sigma^-1 y,  cov = K_ss - K_s^T Sigma^-1 K_s  (Sigma entering through its symmetric
    part: the library returns the symmetric gradient, as torch's cholesky backward does).  Bound: rel < 1e-8, the one
    test_gp_basic_forward_autograd_cached_factor (test_gpu_parity.py) applies to the gradients of the same function.

    The test means something only if slot 0 is handed a recycled address: a recording shim on ffgp_trsm_lower_t asserts that from
    round 2 on at least one round passed the same (pointer, n, ldl) as the round before.  Observed on the MI355X (every run so far):
    round 2 gets another address than round 1 (the first round meets the allocator in another state), rounds 3 and 4 get round 2's,
    because each round frees its tensors before the next one allocates the same sizes in the same order.  Slot 0 sees no
    factorisation between two backward solves, so before the backward announced its factor (ffgp_trtri_diag) rounds 3 and 4 were
    solved with round 2's inverted blocks: gradient errors 1.9e-14, 1.6e-14, 1.47, 1.69 in the four rounds."""
    from fidelityfusion_amd import functional as F
    n, d, nt, D = 300, 2, 5, 3
    rng = np.random.default_rng(11)
    rounds = []
    for r in range(4):
        X = rng.uniform(size=(n, D))
        Sig = np.exp(-0.5 * ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)) + 0.3 * np.eye(n)
        rounds.append((Sig, rng.standard_normal((n, d)), rng.standard_normal((n, nt)), spd(nt, rng, 10.0),
                       rng.standard_normal((nt, d)), rng.standard_normal((nt, nt))))
    keys = []
    real = F._lib.lib.ffgp_trsm_lower_t

    class _Spy:
        def __getattr__(self, name):
            return getattr(F._lib.lib, name)

        def ffgp_trsm_lower_t(self, h, L, n_, ldl, *rest):
            keys.append((L.value, n_, ldl))
            return real(h, L, n_, ldl, *rest)

    worst = []
    with F.patched_lib(_Spy()):
        for r, (Sig, y, Ks, Kss, R1, R2) in enumerate(rounds):
            cpu = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (y, Sig, Ks, Kss)]
            yc, Sc, Ksc, Kssc = cpu
            sol = torch.linalg.solve(0.5 * (Sc + Sc.T), torch.cat([yc, Ksc], 1))
            mu_c, cov_c = Ksc.T @ sol[:, :d], Kssc - Ksc.T @ sol[:, d:]
            ((mu_c * torch.tensor(R1)).sum() + (cov_c * torch.tensor(R2)).sum()).backward()
            gpu = [torch.tensor(a, dtype=torch.float64, device=DEVICE, requires_grad=True) for a in (y, Sig, Ks, Kss)]
            with ff.thread_slot(1):
                mu, cov = F.conditional_gaussian(*gpu)
            assert relerr(mu.detach().cpu().numpy(), mu_c.detach().numpy()) < 1e-9
            assert relerr(cov.detach().cpu().numpy(), cov_c.detach().numpy()) < 1e-9
            before = len(keys)
            ((mu * dev(R1)).sum() + (cov * dev(R2)).sum()).backward()
            assert len(keys) == before + 1, "the backward pass is expected to make one ffgp_trsm_lower_t call"
            errs = [relerr(g.grad.cpu().numpy(), c.grad.numpy()) for g, c in zip(gpu, cpu)]
            print("C.1 round %d: key %s, gradient errors (y, Sigma, K_s, K_ss) %s" % (r + 1, keys[-1], errs))
            worst.append(max(errs))
            del gpu, mu, cov
    reused = _same_key_as_round_before(keys)
    print("C.1 reused in rounds", [i + 1 for i in reused])
    assert reused, "no round handed slot 0 the (pointer, n, ldl) of the round before: the test did not test anything (%s)" % (keys,)
    assert max(worst) < 1e-8, "gradient errors per round %s; rounds with the key of the round before: %s" % (worst, [i + 1 for i in reused])


def test_posterior_rebuilt_and_queried_from_another_slot(ff):
    """C.2: a Posterior (slot 0, n = 300, capacity 320 so that ld repeats) queried from thread_slot(1), dropped, and rebuilt with other
    hyper-parameters and the same shapes; the next one is queried from thread_slot(1) again.  Mean and covariance against the fused
    ffgp_predict path on the same model, rel < 1e-9 (the tolerance of test_posterior_reuse_and_append).  A rebuilt W must land on
    the address of the one before (asserted): slot 1 then holds a store keyed on (W, 300, 320) that belongs to the factor before.
    Every round runs in its own scope and frees all it allocated, so each round meets the allocator in the same state; observed on
    the MI355X (every run so far): all four W at one address.  Before a Posterior told a slot that had not factored its buffer
    (ffgp_trtri_diag), posteriors 2-4 came out with mean errors of 35 .. 206 and covariance errors of 2e3 .. 2.7e5."""
    from fidelityfusion_amd import functional as F
    n, D, d, nt = 300, 3, 2, 9
    g = torch.Generator(device=DEVICE).manual_seed(12)
    X = torch.rand((n, D), generator=g, device=DEVICE, dtype=torch.float64)
    Y = torch.randn((n, d), generator=g, device=DEVICE, dtype=torch.float64)
    Xs = torch.rand((nt, D), generator=g, device=DEVICE, dtype=torch.float64)

    def one_round(w0, a0, d0):
        w = torch.full((D,), w0, device=DEVICE, dtype=torch.float64)
        amp = torch.tensor([a0], device=DEVICE, dtype=torch.float64)
        dadd = torch.tensor([d0], device=DEVICE, dtype=torch.float64)
        with torch.no_grad():
            m_ref, v_ref = F.predict(X, Y, Xs, w, amp, diag_add=dadd, clamp=1e-30, full_cov=True)
            post = F.Posterior(X, Y, w, amp, dadd, clamp=1e-30, capacity=320)
            assert post.ld == 320
            with ff.thread_slot(1):
                mean, var = post.predict(Xs)
        return ((post.W.data_ptr(), post.n, post.ld),
                (relerr(mean.cpu().numpy(), m_ref.cpu().numpy()), relerr(var.cpu().numpy(), v_ref.cpu().numpy())))

    ptrs, errs = [], []
    for params in ((1.7, 0.9, 0.05), (0.8, 1.6, 0.2), (2.4, 0.5, 0.1), (1.1, 1.2, 0.07)):
        key, err = one_round(*params)
        ptrs.append(key)
        errs.append(err)
        print("C.2 posterior %d: W key %s, (mean, covariance) errors %s" % (len(ptrs), key, err))
    reused = _same_key_as_round_before(ptrs)
    print("C.2 rebuilt on the address of the one before:", [i + 1 for i in reused])
    assert reused, "no rebuilt posterior landed on the address of the one before: the test did not test anything (%s)" % (ptrs,)
    assert max(max(e) for e in errs) < 1e-9, "errors per posterior %s; rebuilt on the previous address: %s" % (errs, [i + 1 for i in reused])


# ------------------------------------------------------------------------------------------------ D. ffgp_gemm_batched
GEMM_SHAPES = [(64, 64, 64), (1, 1, 1), (37, 50, 21), (130, 129, 48), (128, 128, 80)]
GEMM_BATCHES = (1, 2, 5, 33)
GEMM_COEFS = ((1.0, 0.0), (0.5, -2.0), (-1.0, 1.0))      # beta = 0 on a NaN-filled C; the general form; the fast form
STRIDE_MODES = ("tight", "even", "odd", "shared_a", "moat")


def _layout(mode, rows, cols, which):
    """(ld, member stride) of a [rows, cols] operand under a stride mode"""
    if mode == "tight" or (mode == "shared_a" and which != "A") or (mode == "moat" and which != "C") or (mode == "odd" and which == "C"):
        return cols, rows * cols
    if mode == "even":
        ld = cols + {"A": 2, "B": 4, "C": 6}[which]
        return ld, rows * ld + 6
    if mode == "odd":                  # odd strides switch the 16-byte operand loads off for the later members
        st = rows * cols + 3
        return cols, st + (1 - st % 2)
    if mode == "shared_a":
        return cols, 0
    return cols + 3, rows * (cols + 3) + 5         # "moat": NaN between the rows and between the members of C


def _pack(mats, rows, cols, ld, stride, batch):
    """the members, each [rows, cols] at leading dimension ld, `stride` apart in a NaN-filled buffer"""
    buf = np.full(((batch - 1) * stride + rows * ld,), np.nan)
    for b in range(batch if stride else 1):
        v = buf[b * stride:b * stride + rows * ld].reshape(rows, ld)
        v[:, :cols] = mats[b]
    return buf


def run_gemm_batched(_lib, h, opa, opb, lower, A, B, C0, alpha, beta, mode):
    """A [batch, m, k] = op(A_b), B [batch, k, n] = op(B_b), C0 [batch, m, n] (NaN where beta = 0) -> (C [batch, m, n], whole buffer
    before, whole buffer after, mask of the elements the call may write)"""
    batch, m, k = A.shape
    n = B.shape[2]
    As = A if opa == 0 else A.transpose(0, 2, 1)
    Bs = B.transpose(0, 2, 1) if opb == 0 else B
    (lda, sA), (ldb, sB), (ldc, sC) = (_layout(mode, As.shape[1], As.shape[2], "A"), _layout(mode, Bs.shape[1], Bs.shape[2], "B"),
                                       _layout(mode, m, n, "C"))
    Ab = _pack(As, As.shape[1], As.shape[2], lda, sA, batch)
    Bb = _pack(Bs, Bs.shape[1], Bs.shape[2], ldb, sB, batch)
    Cb = _pack(C0, m, n, ldc, sC, batch)
    may = np.zeros(Cb.shape, dtype=bool)
    tri = np.tril(np.ones((m, n), dtype=bool)) if lower else np.ones((m, n), dtype=bool)
    for b in range(batch):
        may[b * sC:b * sC + m * ldc].reshape(m, ldc)[:, :n] = tri
    Ad, Bd, Cd = dev(Ab), dev(Bb), dev(Cb)
    rc = _lib.lib.ffgp_gemm_batched(h, opa, opb, lower, ptr(Ad), lda, sA, ptr(Bd), ldb, sB, ptr(Cd), ldc, sC, m, n, k, alpha, beta, batch)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = Cd.cpu().numpy()
    got = np.stack([out[b * sC:b * sC + m * ldc].reshape(m, ldc)[:, :n] for b in range(batch)])
    return got, Cb, out, may


def _gemm_case(_lib, h, opa, opb, lower, m, n, k, batch, mode, alpha, beta, rng):
    A = rng.standard_normal((1 if mode == "shared_a" else batch, m, k))
    if mode == "shared_a":
        A = np.repeat(A, batch, axis=0)
    B = rng.standard_normal((batch, k, n))
    C0 = np.full((batch, m, n), np.nan) if beta == 0.0 else rng.standard_normal((batch, m, n))
    got, before, after, may = run_gemm_batched(_lib, h, opa, opb, lower, A, B, C0, alpha, beta, mode)
    what = (opa, opb, lower, m, n, k, batch, mode, alpha, beta)
    # everything the call may not write -- ldc padding, the moat between members, the strictly-upper part of a lower launch -- is
    # bit for bit what it was (NaN stays NaN)
    assert np.array_equal(before[~may], after[~may], equal_nan=True), what
    tri = np.tril(np.ones((m, n), dtype=bool)) if lower else np.ones((m, n), dtype=bool)
    for b in range(batch):
        ref = alpha * (A[b] @ B[b]) + (0.0 if beta == 0.0 else beta * C0[b])
        assert relerr(got[b][tri], ref[tri]) < 1e-13, what + (b,)


@pytest.mark.parametrize("opa,opb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
def test_gemm_batched_layouts_strides_and_coefficients(ff, opa, opb, m, n, k):
    """D: C_b = alpha op(A_b) op(B_b) + beta C_b against numpy per member, relerr < 1e-13 as test_gemm_layouts: all four layouts;
    batch 1, 2, 5, 33; tight, even-padded, ODD (vector loads off) and zero (one shared A) strides, a NaN moat around every member of
    C that must stay NaN; beta = 0 on a NaN-filled C, the general and the fast coefficient forms"""
    h0, _ = handles(ff)
    rng = np.random.default_rng(1000 * m + 10 * k + 2 * opa + opb)
    for batch in GEMM_BATCHES:
        for mode in STRIDE_MODES:
            for alpha, beta in GEMM_COEFS:
                _gemm_case(ff, h0, opa, opb, 0, m, n, k, batch, mode, alpha, beta, rng)


@pytest.mark.parametrize("opa,opb", [(0, 0), (1, 1)])
@pytest.mark.parametrize("m,n,k", [s for s in GEMM_SHAPES if s[0] >= s[1]])
def test_gemm_batched_lower_tiles(ff, opa, opb, m, n, k):
    """D: lower_tiles = 1 (the supported (0, 0) and (1, 1) layouts): only col <= row is computed, the strictly-upper part of every
    member of C is left as it was"""
    h0, _ = handles(ff)
    rng = np.random.default_rng(2000 * m + 10 * k + opa)
    for batch in GEMM_BATCHES:
        for mode in STRIDE_MODES:
            for alpha, beta in GEMM_COEFS:
                _gemm_case(ff, h0, opa, opb, 1, m, n, k, batch, mode, alpha, beta, rng)


@pytest.mark.parametrize("opa,opb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_batched_members_do_not_interact(ff, opa, opb):
    """D: NaN in member 3's operands leaves every other member's result bit-identical to the unpoisoned run"""
    h0, _ = handles(ff)
    rng = np.random.default_rng(3000 + 2 * opa + opb)
    for m, n, k in GEMM_SHAPES:
        for mode in ("tight", "even", "odd"):
            A, B = rng.standard_normal((5, m, k)), rng.standard_normal((5, k, n))
            C0 = rng.standard_normal((5, m, n))
            clean, _, _, _ = run_gemm_batched(ff, h0, opa, opb, 0, A, B, C0, 0.5, -2.0, mode)
            Ap, Bp = A.copy(), B.copy()
            Ap[3], Bp[3] = np.nan, np.nan
            dirty, _, _, _ = run_gemm_batched(ff, h0, opa, opb, 0, Ap, Bp, C0, 0.5, -2.0, mode)
            assert np.isnan(dirty[3]).all()
            for b in (0, 1, 2, 4):
                assert np.array_equal(clean[b], dirty[b]), (opa, opb, m, n, k, mode, b)
