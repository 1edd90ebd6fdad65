"""The kept factor of a trained model: `Posterior` (factor once, query / differentiate / append afterwards) and the modules' cache of
it.  Reference: `cigp.forward` re-factorises on every call (GaussianProcess/cigp_v10.py:24-48); the acquisition loops of
Bayesian_optimization/acq.py:10-80 query a frozen model again and again.
"""
import ctypes as C
import math
import weakref

import torch

from . import _lib
from ._common import NEG_INF, _check_same_D, _check_xy, _dev, _device_of, _ptr, _raise_not_pd, _split_kfun, _weights
from ._lib import FFGP_LL_V1, FFGP_LL_V2, FFGP_VAR_DIAG, FFGP_VAR_FULL, PI_TRUNC, Grads, KDesc, KDescGrads, Problem, check, lib
from .kdesc import FFGP_KFUN_LINEAR, FFGP_KOP_PRODUCT, FFGP_KOP_SUM, FFGP_TREE_BALANCED, FFGP_TREE_CHAIN, _PAIR_KEYS, _pair_descs, _pair_grad_buffers, _pair_grads_out, _pair_split, _tree_spec
from .linalg import _gemm, _pad_ld, kernel_matrix, kernel_pair


class _PosteriorQuery(torch.autograd.Function):
    """mean = K_s^T alpha, var = K_ss - V^T V (V = L^-1 K_s) on a CACHED factor, differentiable w.r.t. K_s and K_ss only
    (the factor, alpha and the hyper-parameters are constants of a `Posterior`): what an acquisition optimiser needs to
    move its query points (Bayesian_optimization/acq.py:50-62) -- one TRSM sweep forward, one backward, no
    refactorisation.   dK_s = alpha Gm^T - Sigma^-1 K_s (Gv + Gv^T)   [diag mode: - 2 Sigma^-1 K_s diag(gv)],  dK_ss = Gv."""

    @staticmethod
    def forward(ctx, post, Ks, Kss, full_cov):
        dev, n = post.dev, post.n
        nt = Ks.shape[1]
        if post.alpha is None:
            post._solve_alpha()
        Ksd = _dev(Ks, dev)
        mean = _gemm(dev, 1, 1, Ksd, post.alpha, nt, post.d, n, 1.0)
        V = Ksd.clone()
        check(lib.ffgp_trsm_lower(post._h_factor(), _ptr(post.W), n, post.ld, _ptr(V), nt, nt), "ffgp_trsm_lower")
        if full_cov:
            var = _dev(Kss, dev) - _gemm(dev, 1, 1, V, V, nt, nt, n, 1.0)
        else:
            var = _dev(Kss, dev) - (V * V).sum(0)
        ctx.pack = (post, V, n, full_cov, post.alpha)
        return mean, var

    @staticmethod
    def backward(ctx, Gm, Gv):
        post, V, n, full_cov, alpha = ctx.pack
        if post.n != n:
            raise RuntimeError("Posterior.append() was called between a differentiable query and its backward()")
        dev = post.dev
        nt = V.shape[1]
        dKs = torch.zeros_like(V)
        if Gm is not None:
            dKs = _gemm(dev, 0, 0, alpha, _dev(Gm, dev), n, nt, post.d, 1.0)          # alpha Gm^T
        dKss = None
        if Gv is not None:
            B = V.clone()
            check(lib.ffgp_trsm_lower_t(post._h_factor(), _ptr(post.W), n, post.ld, _ptr(B), nt, nt), "ffgp_trsm_lower_t")   # Sigma^-1 K_s
            g = _dev(Gv, dev)
            if full_cov:
                dKs = dKs - _gemm(dev, 0, 0, B, (g + g.T).contiguous(), n, nt, nt, 1.0)
            else:
                dKs = dKs - 2.0 * B * g.unsqueeze(0)
            dKss = g
        return None, dKs, dKss, None


class Posterior:
    """A factored GP block kept on the device: factor once, query many times, append points without refactorising
    (the reference's `cigp.forward` re-runs `torch.linalg.cholesky` on every call,
    cigp_v10.py:31-35 -- inside an acquisition loop or when serving predictions that is N^3/3 per query for a factor
    that has not changed).

        predict(Xs)      assembly of K_s, one TRSM sweep on the cached factor (N^2 nt), two thin GEMMs
        append(X, Y)     L21 = (L^-1 K_nk)^T, L22 = chol(S_kk - L21 L21^T): O(N^2 k) instead of O(N^3 / 3)

    Parameters are the library's effective ones (w, amp, diag_add, clamp, kfun), frozen at construction -- or, for a composed
    kernel (SumKernel / ProductKernel over library kernels, `kernel._Pair.pair()`), `tree = (descriptors, operator spec)`."""

    def __init__(self, X, Y, w, amp, diag_add, clamp=NEG_INF, kfun=(0, 1.0), capacity=None, first_query=None,
                 var_add_all=0.0, tree=None):
        """first_query (optional [nt, D]): its K_s^T rides, with Y^T, as passenger rows of the factorisation itself, so
        the first answer (`self.first` = (mean, covariance)) costs what the fused one-shot posterior costs; the rows
        below the factor are scratch afterwards (later appends overwrite them)."""
        dev = _device_of(X, Y, w if tree is None else tree[0][0]["w"])
        self.dev = dev
        self.kfun, _ = _split_kfun(kfun)
        self.clamp = clamp
        Xd, Yd = _dev(X, dev), _dev(Y, dev)
        _check_xy(Xd, Yd)
        n, D = Xd.shape
        d = Yd.shape[1]
        self.tree = None
        if tree is not None:
            # frozen copies of the leaves' effective quantities on the device; the ctypes tree lives as long as this object
            descs = [{k: (_dev(v.detach(), dev).clone() if isinstance(v, torch.Tensor) else v) for k, v in dsc.items()} for dsc in tree[0]]
            meta, tensors = _pair_split(descs)
            self._tree_keep = []
            self.tree = (descs, tree[1], _pair_descs(dev, D, meta, tensors, self._tree_keep, tree[1]))
            self.w = self.amp = None
        else:
            self.w = _weights(w, D, dev)
            self.amp = _dev(amp.reshape(-1)[:1], dev)
        self.dadd = _dev(diag_add.reshape(-1)[:1], dev)
        Xq = _dev(first_query, dev) if first_query is not None else None
        if Xq is not None:
            _check_same_D(Xd, Xq)
        nt = Xq.shape[0] if Xq is not None else 0
        self.cap = max(int(capacity or 0), n)
        self.ld = _pad_ld(self.cap)
        rows = max(self.cap, n + d + nt)                      # room for the passenger rows of the first factorisation
        self.W = torch.zeros((rows, self.ld), dtype=torch.float64, device=dev)
        self.X = torch.empty((self.cap, D), dtype=torch.float64, device=dev)
        self.X[:n] = Xd
        self.n, self.D, self.d = n, D, d
        self._keyed = (_lib.current_slot(), self.W.data_ptr())   # the handle slot whose cached inverses follow this buffer (`_h_factor`)
        h = self._h()
        self._assemble(Xd, Xd, self.W, self.ld, lower=1, diag=True)
        self.W[n:n + d, :n] = Yd.T
        if nt:
            self._assemble(Xq, Xd, self.W[n + d:], self.ld, lower=0, diag=False)          # K_s^T [nt, n]
        rc = check(lib.ffgp_potrf_rows(h, _ptr(self.W), n, n + d + nt, self.ld), "ffgp_potrf_rows")
        if rc > 0:
            _raise_not_pd(rc, "linalg.cholesky")
        Gt = self.W[n:n + d, :n].contiguous()                 # Gamma^T
        self.Gamma = Gt.T.contiguous()
        self.alpha = None                                     # Sigma^-1 Y: solved when a later query needs it
        self.first = None
        if nt:
            Vt = self.W[n + d:n + d + nt, :n].contiguous()    # V^T = (L^-1 K_s)^T
            mean = _gemm(dev, 0, 0, Vt, Gt, nt, d, n, 1.0)
            var = torch.empty((nt, nt), dtype=torch.float64, device=dev)
            self._assemble(Xq, Xq, var, nt, lower=0, diag=False)
            self.first = (mean, var - _gemm(dev, 0, 0, Vt, Vt, nt, nt, n, 1.0) + var_add_all)

    def _h(self):
        h = _lib.handle(self.dev.index)
        _lib.bind_stream(h, self.dev.index)
        return h

    def _h_factor(self):
        """the calling thread's handle for a call that reads the factor through the handle's cached inverses (the triangular solves).
        Those are keyed on (address, n, ld) alone and follow the factor only on the slot that factored this buffer or was last told
        about it; any other slot has never seen the factor, and its key may well name this very address -- the W of a dropped
        Posterior of the same shapes, recycled by the caching allocator.  Such a slot is told first (ffgp_trtri_diag, the contract in
        include/ffgp.h: the rebuild a key mismatch pays anyway) and becomes the slot that is followed; so is every slot after the
        buffer itself was replaced (`append` past the capacity, a deep copy)."""
        h = self._h()
        keyed = (_lib.current_slot(), self.W.data_ptr())
        if keyed != self._keyed:
            check(lib.ffgp_trtri_diag(h, _ptr(self.W), self.n, self.ld), "ffgp_trtri_diag")
            self._keyed = keyed
        return h

    def _assemble(self, A, B, out, ld, lower, diag):
        if self.tree is not None:
            check(lib.ffgp_assemble_tree(self._h(), _ptr(A), A.shape[0], _ptr(B), B.shape[0], self.D, C.byref(self.tree[2]),
                                         _ptr(self.dadd) if diag else None, None, 0, None, 0, 0.0, 0.0, _ptr(out), ld, lower),
                  "ffgp_assemble_tree")
            return
        check(lib.ffgp_assemble(self._h(), _ptr(A), A.shape[0], _ptr(B), B.shape[0], self.D, _ptr(self.w), _ptr(self.amp),
                                self.clamp, _ptr(self.dadd) if diag else None, None, 0, None, 0, 0.0, 0.0, _ptr(out), ld, lower,
                                int(self.kfun[0]), float(self.kfun[1])), "ffgp_assemble")

    def _solve_alpha(self):
        self.alpha = self.Gamma.clone()
        check(lib.ffgp_trsm_lower_t(self._h_factor(), _ptr(self.W), self.n, self.ld, _ptr(self.alpha), self.d, self.d),
              "ffgp_trsm_lower_t")

    @torch.no_grad()
    def predict(self, Xs, full_cov=True, var_add_all=0.0):
        """mean [nt, d], covariance [nt, nt] (or variance [nt]) at Xs; the noise convention is the caller's
        (`var_add_all` lands on every entry, cigp_v10.py:44)."""
        dev, n = self.dev, self.n
        Xsd = _dev(Xs, dev)
        _check_same_D(self.X, Xsd)
        nt = Xsd.shape[0]
        if self.alpha is None:
            self._solve_alpha()
        Ks = torch.empty((n, nt), dtype=torch.float64, device=dev)
        self._assemble(self.X[:n], Xsd, Ks, nt, lower=0, diag=False)
        mean = _gemm(dev, 1, 1, Ks, self.alpha, nt, self.d, n, 1.0)                 # K_s^T alpha
        check(lib.ffgp_trsm_lower(self._h_factor(), _ptr(self.W), n, self.ld, _ptr(Ks), nt, nt), "ffgp_trsm_lower")   # V = L^-1 K_s
        if full_cov:
            var = torch.empty((nt, nt), dtype=torch.float64, device=dev)
            self._assemble(Xsd, Xsd, var, nt, lower=0, diag=False)
            var = var - _gemm(dev, 1, 1, Ks, Ks, nt, nt, n, 1.0) + var_add_all
        elif self.tree is not None:
            var = self._kernel(Xsd, Xsd).diagonal() - (Ks * Ks).sum(0) + var_add_all
        else:
            var = float(self.amp) - (Ks * Ks).sum(0) + var_add_all      # phi(0) = 1 for every radial profile
        return mean, var

    def _kernel(self, a, b):
        """the frozen kernel as a differentiable call (w.r.t. a, b)"""
        if self.tree is not None:
            return kernel_pair(a, b, self.tree[0], self.tree[1])
        return kernel_matrix(a, b, self.w, self.amp, self.clamp, kfun=self.kfun)

    def predict_diff(self, Xs, full_cov=True, var_add_all=0.0):
        """`predict` with autograd w.r.t. the query points: K_s and K_ss come from the differentiable kernel call, the
        solves run on the cached factor (`_PosteriorQuery`).  The hyper-parameters, X and Y are constants here -- use
        the model's own forward under autograd when their gradients are wanted as well.
        Rounding note: the triangular solves use the handle's inverted diagonal blocks of the factor.  A fused
        `optimize_acquisition` call rebuilds those blocks from the finished factor, where the factorisation had left its own;
        the two differ in the last bits, so `predict` / `predict_diff` results after such a call can differ at rounding level
        from the ones before it (both are solves on the same factor to working precision)."""
        dev, n = self.dev, self.n
        Xsd = Xs.to(device=dev, dtype=torch.float64)
        _check_same_D(self.X, Xsd)
        Ks = self._kernel(self.X[:n], Xsd)
        if full_cov:
            Kss = self._kernel(Xsd, Xsd)
        elif self.tree is not None:
            Kss = self._kernel(Xsd, Xsd).diagonal()
        else:
            Kss = self.amp.expand(Xsd.shape[0])                  # phi(0) = 1 for every radial profile
        mean, var = _PosteriorQuery.apply(self, Ks, Kss, full_cov)
        return mean, var + var_add_all

    def acq_fusable(self, X0):
        """whether `optimize_acquisition` from X0 takes the one-launch call (ffgp_acq_optimize): ONE radial library kernel, one output,
        n and D within the kernel's LDS-tile limits, the start points fp64 on this posterior's GPU"""
        return (self.tree is None and 0 <= int(self.kfun[0]) < FFGP_KFUN_LINEAR and self.d == 1 and 1 <= self.n <= _lib.FFGP_ACQ_MAX_N
                and 1 <= self.D <= _lib.FFGP_ACQ_MAX_D and isinstance(X0, torch.Tensor) and X0.is_cuda and X0.device == self.dev
                and X0.dtype == torch.float64 and X0.dim() == 2 and X0.shape[0] >= 1 and X0.shape[1] == self.D)

    def acq_staged_ok(self, X0):
        """whether `optimize_acquisition(..., staged=True)` from X0 may take the launch-per-stage call (ffgp_acq_optimize_stack_staged):
        `acq_fusable`'s conditions with n up to FFGP_ACQ_STAGED_MAX_N = 2048 in place of 256 -- ONE radial library kernel (no descriptor
        tree, no LinearKernel), one output, D <= 16, the start points fp64 on this posterior's GPU"""
        return (self.tree is None and 0 <= int(self.kfun[0]) < FFGP_KFUN_LINEAR and self.d == 1 and 1 <= self.n <= _lib.FFGP_ACQ_STAGED_MAX_N
                and 1 <= self.D <= _lib.FFGP_ACQ_MAX_D and isinstance(X0, torch.Tensor) and X0.is_cuda and X0.device == self.dev
                and X0.dtype == torch.float64 and X0.dim() == 2 and X0.shape[0] >= 1 and X0.shape[1] == self.D)

    def acq_tree_fusable(self, X0):
        """whether `optimize_acquisition(..., fuse_composed=True)` from X0 takes the one-launch call for composed kernels
        (ffgp_acq_optimize_tree): a descriptor tree of 2-4 library leaves (radial profiles and LinearKernel), one output, n and D
        within the kernel's LDS-tile limits, the start points fp64 on this posterior's GPU"""
        return (self.tree is not None and 2 <= len(self.tree[0]) <= 4
                and all(0 <= int(dsc["kfun"]) <= FFGP_KFUN_LINEAR for dsc in self.tree[0]) and self.d == 1
                and 1 <= self.n <= _lib.FFGP_ACQ_MAX_N and 1 <= self.D <= _lib.FFGP_ACQ_MAX_D and isinstance(X0, torch.Tensor) and X0.is_cuda
                and X0.device == self.dev and X0.dtype == torch.float64 and X0.dim() == 2 and X0.shape[0] >= 1 and X0.shape[1] == self.D)

    def acq_tree_staged_ok(self, X0):
        """whether `optimize_acquisition(..., fuse_composed=True, staged=True)` from X0 may take the launch-per-stage call for composed
        kernels (ffgp_acq_optimize_stack_tree_staged): `acq_tree_fusable`'s conditions with n up to FFGP_ACQ_STAGED_MAX_N = 2048 in
        place of 256 -- a descriptor tree of 2-4 library leaves, one output, D <= 16, the start points fp64 on this posterior's GPU"""
        return (self.tree is not None and 2 <= len(self.tree[0]) <= 4
                and all(0 <= int(dsc["kfun"]) <= FFGP_KFUN_LINEAR for dsc in self.tree[0]) and self.d == 1
                and 1 <= self.n <= _lib.FFGP_ACQ_STAGED_MAX_N and 1 <= self.D <= _lib.FFGP_ACQ_MAX_D and isinstance(X0, torch.Tensor)
                and X0.is_cuda and X0.device == self.dev and X0.dtype == torch.float64 and X0.dim() == 2 and X0.shape[0] >= 1
                and X0.shape[1] == self.D)

    def optimize_acquisition(self, X0, steps=30, lr=0.1, acq="ucb", kappa=2.0, xi=0.01, f_best=0.0, var_add_all=0.0, var_floor=1e-12,
                             betas=(0.9, 0.999), eps=1e-8, state=None, fuse_composed=False, staged=False):
        """`steps` Adam iterations of the reference's acquisition optimiser on this frozen posterior
        (Bayesian_optimization/acq.py:48-68: zero_grad(); loss = -acq(X).sum(); loss.backward(); Adam.step()), from the start points
        X0 [Q, D] (left untouched).  acq = "ucb": mean + kappa sqrt(max(var, var_floor)); "ei": acq.py:161-181 with f_best, xi.
        Returns (X [Q, D], trace [steps, Q] = the acquisition values BEFORE each step's update, hist [steps + 1, Q, D] = the points
        before each step and the final ones, state).  `state` carries Adam's moments and step count into a following call and reports
        the path as state["fused"]: ONE kernel launch for the whole loop when `acq_fusable(X0)` and steps <= 4096 (csrc/acq.hip),
        otherwise the per-step loop -- `predict_diff` and torch.optim.Adam -- which covers composed kernels, LinearKernel, several
        outputs (the values of a point's outputs are summed, as the reference's `.sum()` does) and larger n.
        The fused call rebuilds the handle's inverted diagonal blocks from the factor (one extra launch per call), so its result
        depends on the factor alone; later `predict` / `predict_diff` calls then solve with those blocks (see `predict_diff`).
        `fuse_composed=True` opts a composed kernel in: when `acq_tree_fusable(X0)` and steps <= 4096 the loop is ONE launch as well
        (ffgp_acq_optimize_tree, csrc/acq_tree.hip: Sum / Product trees of 2-4 leaves, LinearKernel included), with the same return
        values, `state` contract and state["fused"] = True; otherwise, and by default, such a posterior takes the per-step loop.
        `staged=True` opts larger models in: a posterior that is not `acq_fusable(X0)` but `acq_staged_ok(X0)` (n up to 2048) runs the
        loop launch per stage inside ONE library call (ffgp_acq_optimize_stack_staged, csrc/acq_staged.hip) -- same return values and
        `state` contract, state["staged"] = True and state["fused"] = False; an `acq_fusable` problem takes the one-launch call exactly
        as without the keyword, and `staged="force"` sends it to the staged call as well (tests, tools/acq_staged_bench.py).
        `fuse_composed=True` together with `staged=True` opts a large composed-kernel model in: a posterior that is not
        `acq_tree_fusable(X0)` but `acq_tree_staged_ok(X0)` (2-4 leaves, n up to 2048) runs the staged loop for composed kernels
        (ffgp_acq_optimize_stack_tree_staged, csrc/acq_staged_tree.hip), with state["staged"] = True and state["fused"] = False; one of
        up to 256 points keeps its one-launch call bit for bit unless `staged="force"`.  `staged=True` alone leaves a composed kernel
        on the per-step loop: composed kernels stay opt-in through `fuse_composed`."""
        acq = str(acq).lower()
        if acq not in ("ucb", "ei"):
            raise ValueError("acq must be 'ucb' or 'ei', got %r" % (acq,))
        # one posterior is the stack of one member with coefficient 1: the checks, the per-step loop and the fused call live there
        single = _TreePosterior if fuse_composed and self.tree is not None else _SinglePosterior
        return single([self], [1.0]).optimize_acquisition(X0, steps=steps, lr=lr, acq=acq, kappa=kappa, xi=xi, f_best=f_best,
                                                          var_floor=var_floor, betas=betas, eps=eps, var_adds=[var_add_all], state=state,
                                                          fuse_composed=fuse_composed, staged=staged)

    @torch.no_grad()
    def append(self, X_new, Y_new):
        """Extend the factor by k points: the new block row of L is a TRSM on the cached factor, the new diagonal
        block a k x k Cholesky of the Schur complement."""
        dev, n = self.dev, self.n
        Xn, Yn = _dev(X_new, dev), _dev(Y_new, dev)
        _check_same_D(self.X, Xn, "X_new")
        if Yn.dim() != 2 or Yn.shape != (Xn.shape[0], self.d):
            raise ValueError("Y_new must be [%d, %d], got shape %s" % (Xn.shape[0], self.d, tuple(Yn.shape)))
        k = Xn.shape[0]
        if n + k > self.cap or n + k > self.W.shape[0]:       # grow geometrically; the factor is copied once
            cap = max(n + k, 2 * self.cap)
            ld = _pad_ld(cap)
            W = torch.zeros((cap, ld), dtype=torch.float64, device=dev)
            W[:n, :n] = self.W[:n, :n]
            Xb = torch.empty((cap, self.D), dtype=torch.float64, device=dev)
            Xb[:n] = self.X[:n]
            self.W, self.X, self.cap, self.ld = W, Xb, cap, ld
        B = torch.empty((n, k), dtype=torch.float64, device=dev)
        self._assemble(self.X[:n], Xn, B, k, lower=0, diag=False)
        check(lib.ffgp_trsm_lower(self._h_factor(), _ptr(self.W), n, self.ld, _ptr(B), k, k), "ffgp_trsm_lower")   # L^-1 K_nk = L21^T
        ks = _pad_ld(k)
        S = torch.zeros((k, ks), dtype=torch.float64, device=dev)
        self._assemble(Xn, Xn, S, ks, lower=0, diag=True)
        S[:, :k] -= _gemm(dev, 1, 1, B, B, k, k, n, 1.0)                                                 # Schur complement
        # the small factor goes through a second handle: this handle's store of inverted diagonal blocks stays
        # attached to the big factor and is only extended by the new blocks
        h2 = _lib.handle(dev.index, 1)
        _lib.bind_stream(h2, dev.index)
        rc = check(lib.ffgp_potrf(h2, _ptr(S), k, ks), "ffgp_potrf")
        if rc > 0:
            _raise_not_pd(n + rc, "linalg.cholesky")
        G_new = Yn - _gemm(dev, 1, 1, B, self.Gamma, k, self.d, n, 1.0)                                  # y_new - L21 Gamma
        check(lib.ffgp_trsm_lower(h2, _ptr(S), k, ks, _ptr(G_new), self.d, self.d), "ffgp_trsm_lower")
        self.W[n:n + k, :n] = B.T
        self.W[n:n + k, n:n + k] = torch.tril(S[:, :k])
        self.X[n:n + k] = Xn
        self.Gamma = torch.cat([self.Gamma, G_new], 0)
        self.n = n + k
        self.alpha = None


class PosteriorStack:
    """A stack of frozen per-fidelity posteriors queried as ONE model: the posterior of the reference's AR / ResGP / CAR
    (FidelityFusion_Models/AR_autoRegression.py:56-89)
        mean = sum_f mean_coef_f mean_f,   var = sum_f var_coef_f var_f      over the members 0..level (`to_fidelity`)
    with mean_coefs = (1, rho_0, rho_1, ...) for AR and all ones for ResGP; `var_coefs` defaults to mean_coefs^2.  Every member is a
    `Posterior` on the same GPU with the same input dimension; the members' n and kernels are their own."""

    def __init__(self, members, mean_coefs, var_coefs=None):
        members = list(members)
        if not members or not all(isinstance(m, Posterior) for m in members):
            raise ValueError("members must be a non-empty list of Posterior")
        if any(m.dev != members[0].dev or m.D != members[0].D for m in members):
            raise ValueError("the members of a PosteriorStack share one device and one input dimension")
        self.members = members
        self.mean_coefs = [float(c) for c in mean_coefs]
        self.var_coefs = [c * c for c in self.mean_coefs] if var_coefs is None else [float(c) for c in var_coefs]
        if len(self.mean_coefs) != len(members) or len(self.var_coefs) != len(members):
            raise ValueError("one mean coefficient and one variance coefficient per member")
        self.dev, self.D, self.F = members[0].dev, members[0].D, len(members)

    def _var_adds(self, var_adds):
        va = [0.0] * self.F if var_adds is None else [float(v) for v in var_adds]
        if len(va) != self.F:
            raise ValueError("var_adds holds one value per member")
        return va

    def _level(self, level, Q):
        """None, or an int32 tensor [Q] on the stack's device with values in 0..F-1 (an int applies to every point)"""
        if level is None:
            return None
        if isinstance(level, torch.Tensor):
            lv = level.to(device=self.dev, dtype=torch.int32).reshape(-1).contiguous()
        else:
            lv = torch.full((Q,), int(level), dtype=torch.int32, device=self.dev)
        if lv.shape[0] != Q or int(lv.min()) < 0 or int(lv.max()) >= self.F:
            raise ValueError("level must hold %d values in 0..%d" % (Q, self.F - 1))
        return lv

    def predict_diff(self, Xs, level=None, var_adds=None):
        """The combined mean [nt, d] and diagonal variance [nt] at Xs, differentiable w.r.t. Xs (the members' `predict_diff`);
        `level` (int or [nt]) cuts the sums after member level[q]; `var_adds[f]` is member f's noise (its 1 / beta)."""
        va = self._var_adds(var_adds)
        lv = self._level(level, Xs.shape[0])
        top = self.F - 1 if lv is None else int(lv.max())
        mean = var = None
        for f in range(top + 1):
            m, v = self.members[f].predict_diff(Xs, full_cov=False, var_add_all=va[f])
            cm, cv = self.mean_coefs[f], self.var_coefs[f]
            if lv is not None:
                on = (lv >= f).to(torch.float64)
                m, v = m * on.unsqueeze(1), v * on
            mean = cm * m if mean is None else mean + cm * m
            var = cv * v if var is None else var + cv * v
        return mean, var

    def acq_fusable(self, X0):
        """whether `optimize_acquisition` from X0 takes the one-launch call (ffgp_acq_optimize_stack)"""
        return self.F <= _lib.FFGP_ACQ_MAX_MEMBERS and all(m.acq_fusable(X0) for m in self.members)

    def acq_staged_ok(self, X0):
        """whether `optimize_acquisition(..., staged=True)` from X0 may take the launch-per-stage call (ffgp_acq_optimize_stack_staged):
        at most 8 members, each of them `Posterior.acq_staged_ok` (one radial library kernel, d = 1, D <= 16, n <= 2048)"""
        return self.F <= _lib.FFGP_ACQ_MAX_MEMBERS and all(m.acq_staged_ok(X0) for m in self.members)

    def acq_tree_fusable(self, X0):
        """whether `optimize_acquisition(..., fuse_composed=True)` from X0 takes a one-launch call: at most 8 members, each of them
        `acq_fusable` (one radial library kernel) or `acq_tree_fusable` (a descriptor tree of 2-4 library leaves)"""
        return self.F <= _lib.FFGP_ACQ_MAX_MEMBERS and all(m.acq_fusable(X0) or m.acq_tree_fusable(X0) for m in self.members)

    def acq_tree_staged_ok(self, X0):
        """whether `optimize_acquisition(..., fuse_composed=True, staged=True)` from X0 may take the launch-per-stage call for stacks
        with composed members (ffgp_acq_optimize_stack_tree_staged): at most 8 members, each of them `acq_staged_ok` (one radial
        library kernel) or `acq_tree_staged_ok` (a descriptor tree of 2-4 library leaves), n <= 2048"""
        return self.F <= _lib.FFGP_ACQ_MAX_MEMBERS and all(m.acq_staged_ok(X0) or m.acq_tree_staged_ok(X0) for m in self.members)

    def _acq_route(self, X0, fuse_composed, staged):
        """(the C entry's caller or None for the per-step loop, whether it is a launch-per-stage call)"""
        one = self._acq_call if self.acq_fusable(X0) else self._acq_call_trees if fuse_composed and self.acq_tree_fusable(X0) else None
        if staged and (staged == "force" or one is None):
            if self.acq_staged_ok(X0):      # no composed member
                return self._acq_call_staged, True
            if fuse_composed and self.acq_tree_staged_ok(X0):
                return self._acq_call_trees_staged, True
        return one, False

    def optimize_acquisition(self, X0, steps=30, lr=0.1, acq="ucb", kappa=2.0, xi=0.01, f_best=0.0, var_floor=1e-12, betas=(0.9, 0.999),
                             eps=1e-8, level=None, var_adds=None, accumulate_grad=False, state=None, fuse_composed=False, staged=False):
        """`Posterior.optimize_acquisition` on the stack's posterior, with the same return tuple (X, trace, hist, state).
        acq = "ucb" / "ei" as there, or "ucb_var": mean + kappa var, the multi-fidelity drivers' form
        (MF_BayesianOptimization/Discrete/DMF_acq.py:49-63).  `level` (int or [Q]) gives every point its own `to_fidelity`, so one
        call optimises the acquisition at every fidelity; `accumulate_grad=True` runs the drivers' loop as it stands
        (DMF_acq.py:246-255: no zero_grad, Adam sees the running sum of the gradients; the sum travels as state["grad_sum"]).
        ONE kernel launch (csrc/acq_stack.hip) when every member is `acq_fusable` and there are at most 8 of them, otherwise the
        per-step loop on `predict_diff` and torch.optim.Adam; state["fused"] says which.
        `fuse_composed=True` opts members with composed kernels in, as for a single posterior: a stack with at least one tree member
        that is `acq_tree_fusable(X0)` is ONE launch as well (ffgp_acq_optimize_stack_tree, csrc/acq_stack_tree.hip: radial members
        and Sum / Product trees of 2-4 leaves mixed freely), with the same return values and `state` contract.  A stack without a
        tree member takes the call above whatever the keyword says; without the keyword nothing changes.
        `staged=True` opts members beyond the one-launch kernels' n <= 256 in: a stack that is not `acq_fusable(X0)` but
        `acq_staged_ok(X0)` (radial members of up to 2048 points) runs the loop launch per stage inside ONE library call
        (ffgp_acq_optimize_stack_staged, csrc/acq_staged.hip: levels, coefficients, `var_adds`, all three acquisitions and
        `accumulate_grad` as in the one-launch call, whose `state` it continues and hands on); state["staged"] = True and
        state["fused"] = False then.  An `acq_fusable` stack takes the one-launch call exactly as without the keyword;
        `staged="force"` sends it to the staged call too (tests, tools/acq_staged_bench.py).
        `fuse_composed=True` together with `staged=True` opts large stacks with composed members in: a stack that takes no one-launch
        call and has a composed member, but is `acq_tree_staged_ok(X0)` (radial members and trees of 2-4 leaves mixed freely, every
        n <= 2048), runs the staged loop for composed kernels (ffgp_acq_optimize_stack_tree_staged, csrc/acq_staged_tree.hip), with
        the same return values, `state` contract and state["staged"] = True; a stack without a composed member takes the radial
        staged call, and one that takes a one-launch call keeps it bit for bit unless `staged="force"`.  `staged=True` alone leaves
        a stack with a composed member on the per-step loop.  The NAR chain (`PosteriorChain`) has a staged call of its own
        (ffgp_acq_optimize_chain_staged), behind the same keyword."""
        if staged not in (False, True, "force"):
            raise ValueError("staged must be False, True or 'force', got %r" % (staged,))
        acq = str(acq).lower()
        if acq not in ("ucb", "ei", "ucb_var"):
            raise ValueError("acq must be 'ucb', 'ei' or 'ucb_var', got %r" % (acq,))
        steps = int(steps)
        if steps < 1:
            raise ValueError("steps must be at least 1")
        if not isinstance(X0, torch.Tensor) or X0.dim() != 2 or X0.shape[1] != self.D:
            raise ValueError("X0 must be [Q, %d] like the training inputs" % self.D)
        va = self._var_adds(var_adds)
        lv = self._level(level, X0.shape[0])
        step0 = int(state["step"]) if state is not None else 0
        if steps <= _lib.FFGP_ACQ_MAX_STEPS:
            call, stage = self._acq_route(X0, fuse_composed, staged)
            if call is not None:
                return self._optimize_acq_fused(X0, steps, lr, acq, kappa, xi, f_best, var_floor, betas, eps, lv, va, accumulate_grad, state, step0,
                                                call, stage)
        dev = self.dev
        X = X0.detach().to(device=dev, dtype=torch.float64).clone().requires_grad_(True)
        opt = torch.optim.Adam([X], lr=lr, betas=betas, eps=eps)
        if state is not None:
            opt.state[X] = {"step": torch.tensor(float(step0)), "exp_avg": _dev(state["exp_avg"], dev).clone(),
                            "exp_avg_sq": _dev(state["exp_avg_sq"], dev).clone()}
            if accumulate_grad and state.get("grad_sum") is not None:
                X.grad = _dev(state["grad_sum"], dev).clone()
        Q = X.shape[0]
        trace = torch.empty((steps, Q), dtype=torch.float64, device=dev)
        hist = torch.empty((steps + 1, Q, self.D), dtype=torch.float64, device=dev)
        for k in range(steps):
            if not accumulate_grad:
                opt.zero_grad()
            mean, var = self.predict_diff(X, level=lv, var_adds=va)
            var = var.reshape(-1, 1)
            if acq == "ucb":
                a = mean + kappa * torch.sqrt(torch.clamp_min(var, var_floor))
            elif acq == "ucb_var":
                a = mean + kappa * var
            else:
                s = torch.clamp(torch.sqrt(var), min=1e-9)
                u = mean - f_best - xi
                Z = (u / s).detach()      # the reference takes Phi and phi from scipy on detached values
                a = u * (0.5 * torch.erfc(-Z / math.sqrt(2.0))) + s * (torch.exp(-0.5 * Z * Z) / math.sqrt(2.0 * math.pi))
            (-a.sum()).backward()
            hist[k] = X.detach()
            trace[k] = a.detach().sum(1)
            opt.step()
        hist[steps] = X.detach()
        st = opt.state[X]
        out = {"fused": False, "step": step0 + steps, "exp_avg": st["exp_avg"].detach(), "exp_avg_sq": st["exp_avg_sq"].detach()}
        if accumulate_grad:
            out["grad_sum"] = X.grad.detach().clone()
        return (X.detach().to(device=X0.device, dtype=X0.dtype), trace.to(X0.device), hist.to(X0.device), out)

    def _member_table(self, va, keep):
        """the ctypes array of ffgp_acq_member; `keep` collects the tensors its pointers refer to.  A member on a descriptor tree
        carries no kernel of its own (w_dev, amp_dev NULL, kfun 0): ffgp_acq_optimize_stack_tree reads its tree (`_tree_table`)"""
        tab = (_lib.AcqMember * self.F)()
        for f, m in enumerate(self.members):
            if m.alpha is None:
                m._solve_alpha()
            alpha = m.alpha.reshape(-1).contiguous()
            keep.append(alpha)
            own = m.tree is None
            tab[f] = _lib.AcqMember(n=m.n, D=m.D, d=1, X_dev=m.X.data_ptr(), L_dev=m.W.data_ptr(), ldl=m.ld, alpha_dev=alpha.data_ptr(),
                                    w_dev=m.w.data_ptr() if own else None, amp_dev=m.amp.data_ptr() if own else None,
                                    clamp_min=float(m.clamp) if own else 0.0, kfun=int(m.kfun[0]) if own else 0,
                                    kparam=float(m.kfun[1]) if own else 1.0, var_add_all=va[f], mean_coef=self.mean_coefs[f],
                                    var_coef=self.var_coefs[f])
        return tab

    def _tree_table(self):
        """the host array `trees` of ffgp_acq_optimize_stack_tree: each member's ffgp_ktree, NULL for a member with a kernel of its own"""
        trees = (C.POINTER(_lib.KTree) * self.F)()
        for f, m in enumerate(self.members):
            if m.tree is not None:
                trees[f] = C.pointer(m.tree[2])
        return trees

    @torch.no_grad()
    def _optimize_acq_fused(self, X0, steps, lr, acq, kappa, xi, f_best, var_floor, betas, eps, lv, va, accumulate_grad, state, step0, call,
                            staged=False):
        """the buffers of a C-side loop and its returned state; `staged`: the launch-per-stage call took it, not a one-launch kernel"""
        dev, Q, D = self.dev, X0.shape[0], self.D
        X = X0.detach().clone().contiguous()
        buf = torch.zeros((3 if accumulate_grad else 2, Q, D), dtype=torch.float64, device=dev)
        if state is not None:
            buf[0] = _dev(state["exp_avg"], dev)
            buf[1] = _dev(state["exp_avg_sq"], dev)
            if accumulate_grad and state.get("grad_sum") is not None:
                buf[2] = _dev(state["grad_sum"], dev)
        trace = torch.empty((steps, Q), dtype=torch.float64, device=dev)
        hist = torch.empty((steps + 1, Q, D), dtype=torch.float64, device=dev)
        code = {"ucb": _lib.FFGP_ACQ_UCB, "ei": _lib.FFGP_ACQ_EI, "ucb_var": _lib.FFGP_ACQ_UCB_VAR}[acq]
        opt = _lib.Adam(float(lr), float(betas[0]), float(betas[1]), float(eps))
        call(va, lv, dict(var_floor=float(var_floor), acq=code, kappa=float(kappa), xi=float(xi), f_best=float(f_best)), accumulate_grad,
             (_ptr(X), Q, steps, C.byref(opt), _ptr(buf), step0, _ptr(trace), _ptr(hist), None))
        out = {"fused": not staged, "step": step0 + steps, "exp_avg": buf[0], "exp_avg_sq": buf[1]}
        if staged:
            out["staged"] = True
        if accumulate_grad:
            out["grad_sum"] = buf[2]
        return X, trace, hist, out

    def _acq_call(self, va, lv, acq_fields, accumulate_grad, call):
        """the C entry of the fused call; `call`: its arguments after the problem description"""
        keep = []
        s = _lib.AcqStack(F=self.F, members=self._member_table(va, keep), level_dev=lv.data_ptr() if lv is not None else None,
                          accumulate_grad=1 if accumulate_grad else 0, **acq_fields)
        check(lib.ffgp_acq_optimize_stack(self.members[0]._h(), C.byref(s), *call), "ffgp_acq_optimize_stack")

    def _acq_call_staged(self, va, lv, acq_fields, accumulate_grad, call):
        """the C entry of the launch-per-stage call: ffgp_acq_optimize_stack's arguments, a single posterior as the stack of one"""
        keep = []
        s = _lib.AcqStack(F=self.F, members=self._member_table(va, keep), level_dev=lv.data_ptr() if lv is not None else None,
                          accumulate_grad=1 if accumulate_grad else 0, **acq_fields)
        check(lib.ffgp_acq_optimize_stack_staged(self.members[0]._h(), C.byref(s), *call), "ffgp_acq_optimize_stack_staged")

    def _acq_call_trees(self, va, lv, acq_fields, accumulate_grad, call):
        """the C entry of the fused call on a stack with tree members"""
        keep = []
        s = _lib.AcqStack(F=self.F, members=self._member_table(va, keep), level_dev=lv.data_ptr() if lv is not None else None,
                          accumulate_grad=1 if accumulate_grad else 0, **acq_fields)
        check(lib.ffgp_acq_optimize_stack_tree(self.members[0]._h(), C.byref(s), self._tree_table(), *call), "ffgp_acq_optimize_stack_tree")


    def _acq_call_trees_staged(self, va, lv, acq_fields, accumulate_grad, call):
        """the C entry of the launch-per-stage call on a stack with tree members, a single tree posterior as the stack of one"""
        keep = []
        s = _lib.AcqStack(F=self.F, members=self._member_table(va, keep), level_dev=lv.data_ptr() if lv is not None else None,
                          accumulate_grad=1 if accumulate_grad else 0, **acq_fields)
        check(lib.ffgp_acq_optimize_stack_tree_staged(self.members[0]._h(), C.byref(s), self._tree_table(), *call),
              "ffgp_acq_optimize_stack_tree_staged")


class _SinglePosterior(PosteriorStack):
    """`Posterior.optimize_acquisition`: the stack of that one member with coefficient 1, whose fused call is the single-posterior
    entry (ffgp_acq_optimize, its own kernel in csrc/acq.hip)"""

    def _acq_call(self, va, lv, acq_fields, accumulate_grad, call):
        assert self.F == 1 and lv is None and not accumulate_grad, "ffgp_acq_optimize serves one posterior, without levels or accumulation"
        m = self.members[0]
        if m.alpha is None:
            m._solve_alpha()
        alpha = m.alpha.reshape(-1).contiguous()
        p = _lib.AcqProblem(n=m.n, D=m.D, d=1, X_dev=m.X.data_ptr(), L_dev=m.W.data_ptr(), ldl=m.ld, alpha_dev=alpha.data_ptr(),
                            w_dev=m.w.data_ptr(), amp_dev=m.amp.data_ptr(), clamp_min=float(m.clamp), kfun=int(m.kfun[0]),
                            kparam=float(m.kfun[1]), var_add_all=va[0], **acq_fields)
        check(lib.ffgp_acq_optimize(m._h(), C.byref(p), *call), "ffgp_acq_optimize")


class _TreePosterior(PosteriorStack):
    """`Posterior.optimize_acquisition(..., fuse_composed=True)` on a composed kernel: the stack of that one member, whose fused call
    is ffgp_acq_optimize_tree (csrc/acq_tree.hip) on the posterior's own descriptor tree"""

    def acq_fusable(self, X0):
        return self.F == 1 and self.members[0].acq_tree_fusable(X0)

    def _acq_call(self, va, lv, acq_fields, accumulate_grad, call):
        assert self.F == 1 and lv is None and not accumulate_grad, "ffgp_acq_optimize_tree serves one posterior, without levels or accumulation"
        m = self.members[0]
        if m.alpha is None:
            m._solve_alpha()
        alpha = m.alpha.reshape(-1).contiguous()
        p = _lib.AcqTreeProblem(n=m.n, D=m.D, d=1, X_dev=m.X.data_ptr(), L_dev=m.W.data_ptr(), ldl=m.ld, alpha_dev=alpha.data_ptr(),
                                tree=C.pointer(m.tree[2]), var_add_all=va[0], **acq_fields)
        check(lib.ffgp_acq_optimize_tree(m._h(), C.byref(p), *call), "ffgp_acq_optimize_tree")


class PosteriorChain(PosteriorStack):
    """A chain of frozen per-fidelity posteriors queried as ONE model: the posterior of the reference's NAR
    (FidelityFusion_Models/NAR.py:30-61).  members[0] is a `Posterior` on x [D]; members[f > 0] are posteriors on [x, m_{f-1}(x)],
    the lower member's predicted mean as one more input column (D + 1 inputs).  The model's mean and variance are those of the member a
    point stops at (`level`, the reference's `to_fidelity`); the lower members' variances are discarded, as the reference discards
    them.  The acquisition loop, its buffers and its return values are `PosteriorStack`'s."""

    def __init__(self, members):
        members = list(members)
        if not members or not all(isinstance(m, Posterior) for m in members):
            raise ValueError("members must be a non-empty list of Posterior")
        D = members[0].D
        if any(m.dev != members[0].dev for m in members) or any(m.D != D + 1 for m in members[1:]):
            raise ValueError("the members of a PosteriorChain share one device; members[0] takes D inputs, the others D + 1")
        self.members = members
        self.mean_coefs = self.var_coefs = [1.0] * len(members)      # reserved by the C entry: a chain member has no weight
        self.dev, self.D, self.F = members[0].dev, D, len(members)

    def predict_diff(self, Xs, level=None, var_adds=None):
        """The mean [nt, 1] and variance [nt] of the member each point stops at (`level`: int or [nt], None = the top member),
        differentiable w.r.t. Xs through the whole chain: member f is queried at [Xs, mean of member f - 1]; `var_adds[f]` is member
        f's noise (its 1 / beta).  A per-point level selects by exact 0 / 1 masks."""
        va = self._var_adds(var_adds)
        lv = self._level(level, Xs.shape[0])
        top = self.F - 1 if lv is None else int(lv.max())
        Xd = Xs.to(device=self.dev, dtype=torch.float64)
        mean = var = low = None
        for f in range(top + 1):
            z = Xd if f == 0 else torch.cat([Xd, low.reshape(-1, 1)], dim=-1)
            m, v = self.members[f].predict_diff(z, full_cov=False, var_add_all=va[f])
            low = m
            if lv is None:
                mean, var = m, v
            else:
                on = (lv == f).to(torch.float64)
                mean = m * on.unsqueeze(1) if mean is None else mean + m * on.unsqueeze(1)
                var = v * on if var is None else var + v * on
        return mean, var

    def acq_staged_ok(self, X0):
        """never: the stacks' launch-per-stage calls do not serve the chain, which has its own (`acq_chain_staged_ok`)"""
        return False

    def acq_tree_staged_ok(self, X0):
        """never, for the same reason"""
        return False

    def _acq_starts_ok(self, X0):
        return (isinstance(X0, torch.Tensor) and X0.is_cuda and X0.device == self.dev and X0.dtype == torch.float64 and X0.dim() == 2
                and X0.shape[0] >= 1 and X0.shape[1] == self.D)

    def _acq_members_ok(self, nmax):
        def member_ok(m):
            return (m.tree is None and 0 <= int(m.kfun[0]) < FFGP_KFUN_LINEAR and m.d == 1 and 1 <= m.n <= nmax)
        return self.F <= _lib.FFGP_ACQ_MAX_MEMBERS and 1 <= self.D <= _lib.FFGP_ACQ_MAX_D - 1 and all(member_ok(m) for m in self.members)

    def acq_fusable(self, X0):
        """whether `optimize_acquisition` from X0 takes the one-launch call (ffgp_acq_optimize_chain): at most 8 members, each ONE
        radial library kernel with one output and n <= 256, D + 1 <= 16, the start points fp64 [Q, D] on the chain's GPU"""
        return self._acq_members_ok(_lib.FFGP_ACQ_MAX_N) and self._acq_starts_ok(X0)

    def acq_chain_staged_ok(self, X0):
        """whether `optimize_acquisition(..., staged=True)` from X0 may take the launch-per-stage call (ffgp_acq_optimize_chain_staged):
        `acq_fusable`'s conditions with n up to FFGP_ACQ_STAGED_MAX_N = 2048 in place of 256"""
        return self._acq_members_ok(_lib.FFGP_ACQ_STAGED_MAX_N) and self._acq_starts_ok(X0)

    def acq_tree_fusable(self, X0):
        """whether `optimize_acquisition(..., fuse_composed=True)` from X0 takes a one-launch call (ffgp_acq_optimize_chain_tree when
        some member is composed): `acq_fusable`'s size rules -- at most 8 members, one output, n <= 256, D + 1 <= 16, the start points
        fp64 [Q, D] on the chain's GPU -- with every member ONE radial library kernel or a descriptor tree of 2-4 library leaves
        (radial profiles and LinearKernel) on its own D_f inputs"""
        return self._acq_tree_members_ok(_lib.FFGP_ACQ_MAX_N) and self._acq_starts_ok(X0)

    def _acq_tree_members_ok(self, nmax):
        def member_ok(m):
            if m.d != 1 or not 1 <= m.n <= nmax:
                return False
            if m.tree is None:
                return 0 <= int(m.kfun[0]) < FFGP_KFUN_LINEAR
            return 2 <= len(m.tree[0]) <= 4 and all(0 <= int(dsc["kfun"]) <= FFGP_KFUN_LINEAR for dsc in m.tree[0])
        return self.F <= _lib.FFGP_ACQ_MAX_MEMBERS and 1 <= self.D <= _lib.FFGP_ACQ_MAX_D - 1 and all(member_ok(m) for m in self.members)

    def acq_chain_tree_staged_ok(self, X0):
        """whether `optimize_acquisition(..., fuse_composed="staged", staged=True)` from X0 may take the launch-per-stage call for
        chains with composed members (ffgp_acq_optimize_chain_tree_staged): `acq_tree_fusable`'s conditions with n up to
        FFGP_ACQ_STAGED_MAX_N = 2048 in place of 256"""
        return self._acq_tree_members_ok(_lib.FFGP_ACQ_STAGED_MAX_N) and self._acq_starts_ok(X0)

    def _acq_route(self, X0, fuse_composed, staged):
        """(the C entry's caller or None for the per-step loop, whether it is a launch-per-stage call)"""
        one = self._acq_call if self.acq_fusable(X0) else self._acq_call_trees if fuse_composed and self.acq_tree_fusable(X0) else None
        if staged and (staged == "force" or one is None):
            if self.acq_chain_staged_ok(X0):      # no composed member
                return self._acq_call_chain_staged, True
            if fuse_composed == "staged" and self.acq_chain_tree_staged_ok(X0):
                return self._acq_call_chain_trees_staged, True
        return one, False

    def optimize_acquisition(self, X0, steps=30, lr=0.1, acq="ucb", kappa=2.0, xi=0.01, f_best=0.0, var_floor=1e-12, betas=(0.9, 0.999),
                             eps=1e-8, level=None, var_adds=None, accumulate_grad=False, state=None, staged=False, **opt_in):
        """`PosteriorStack.optimize_acquisition` on the chain's posterior: the same arguments, the same return tuple
        (X, trace, hist, state).  ONE kernel launch (ffgp_acq_optimize_chain, csrc/acq_chain.hip) when `acq_fusable(X0)` and
        steps <= 4096 -- only the member a point stops at pays for the triangular solves -- otherwise the per-step loop on
        `predict_diff` and torch.optim.Adam (composed kernels, n > 256, D + 1 > 16, more than 8 members); state["fused"] says which.
        `staged=True` opts members beyond n <= 256 in: a chain that is not `acq_fusable(X0)` but `acq_chain_staged_ok(X0)` (radial
        members of up to 2048 points) runs the loop launch per stage inside ONE library call (ffgp_acq_optimize_chain_staged,
        csrc/acq_staged_chain.hip: levels, `var_adds`, all three acquisitions and `accumulate_grad` as in the one-launch call, whose
        `state` it continues and hands on); state["staged"] = True and state["fused"] = False then.  An `acq_fusable` chain takes the
        one-launch call exactly as without the keyword; `staged="force"` sends it to the staged call too (tests,
        tools/acq_chain_staged_bench.py).  More than 8 members, D + 1 > 16 and n > 2048 keep the per-step loop.
        `fuse_composed=True` opts members with composed kernels in, as for a stack: a chain that is not `acq_fusable(X0)` but
        `acq_tree_fusable(X0)` (radial members and Sum / Product trees of 2-4 leaves mixed freely, LinearKernel included, every
        n <= 256) is ONE launch as well (ffgp_acq_optimize_chain_tree, csrc/acq_chain_tree.hip), with the same return values, `state`
        contract and state["fused"] = True.  An all-radial chain takes ffgp_acq_optimize_chain whatever the keyword says; without the
        keyword nothing changes: a chain with a composed member runs the per-step loop.  With `fuse_composed=True` and `staged=True`
        together a radial chain goes staged and a chain with a composed member past 256 points keeps the per-step loop.
        `fuse_composed="staged"` (the chain only) means what True means and also permits the staged call for composed chains: with
        `staged=True` a chain that takes no one-launch call but is `acq_chain_tree_staged_ok(X0)` (radial members and trees of 2-4
        leaves mixed freely, every n <= 2048) runs the loop launch per stage inside ONE library call
        (ffgp_acq_optimize_chain_tree_staged, csrc/acq_staged_chain_tree.hip), with the same return values and `state` contract --
        a state moves between it, the one-launch calls and the radial staged call -- and state["staged"] = True,
        state["fused"] = False.  A chain of up to 256 points per member keeps its one-launch call unless `staged="force"`.  Any
        other value of `fuse_composed` raises ValueError.  The keyword travels in `**opt_in`, which takes `fuse_composed` (default
        False) and nothing else: the chain's explicit signature is the radial call's and stays as tests/test_acq_stack_tree_host.py
        holds it."""
        fuse_composed = opt_in.pop("fuse_composed", False)
        if opt_in:
            raise TypeError("optimize_acquisition() got an unexpected keyword argument %r" % sorted(opt_in)[0])
        if fuse_composed not in (False, True, "staged"):
            raise ValueError("fuse_composed must be False, True or 'staged', got %r" % (fuse_composed,))
        return super().optimize_acquisition(X0, steps=steps, lr=lr, acq=acq, kappa=kappa, xi=xi, f_best=f_best, var_floor=var_floor,
                                            betas=betas, eps=eps, level=level, var_adds=var_adds, accumulate_grad=accumulate_grad, state=state,
                                            fuse_composed=fuse_composed, staged=staged)

    def _acq_call(self, va, lv, acq_fields, accumulate_grad, call):
        keep = []
        c = _lib.AcqChain(F=self.F, members=self._member_table(va, keep), level_dev=lv.data_ptr() if lv is not None else None,
                          accumulate_grad=1 if accumulate_grad else 0, **acq_fields)
        check(lib.ffgp_acq_optimize_chain(self.members[0]._h(), C.byref(c), *call), "ffgp_acq_optimize_chain")

    def _acq_call_trees(self, va, lv, acq_fields, accumulate_grad, call):
        """the C entry of the fused call on a chain with tree members: ffgp_acq_optimize_chain's arguments and the members' trees"""
        keep = []
        c = _lib.AcqChain(F=self.F, members=self._member_table(va, keep), level_dev=lv.data_ptr() if lv is not None else None,
                          accumulate_grad=1 if accumulate_grad else 0, **acq_fields)
        check(lib.ffgp_acq_optimize_chain_tree(self.members[0]._h(), C.byref(c), self._tree_table(), *call), "ffgp_acq_optimize_chain_tree")

    def _acq_call_chain_staged(self, va, lv, acq_fields, accumulate_grad, call):
        """the C entry of the chain's launch-per-stage call: ffgp_acq_optimize_chain's arguments"""
        keep = []
        c = _lib.AcqChain(F=self.F, members=self._member_table(va, keep), level_dev=lv.data_ptr() if lv is not None else None,
                          accumulate_grad=1 if accumulate_grad else 0, **acq_fields)
        check(lib.ffgp_acq_optimize_chain_staged(self.members[0]._h(), C.byref(c), *call), "ffgp_acq_optimize_chain_staged")

    def _acq_call_chain_trees_staged(self, va, lv, acq_fields, accumulate_grad, call):
        """the C entry of the launch-per-stage call on a chain with tree members: ffgp_acq_optimize_chain_tree's arguments"""
        keep = []
        c = _lib.AcqChain(F=self.F, members=self._member_table(va, keep), level_dev=lv.data_ptr() if lv is not None else None,
                          accumulate_grad=1 if accumulate_grad else 0, **acq_fields)
        check(lib.ffgp_acq_optimize_chain_tree_staged(self.members[0]._h(), C.byref(c), self._tree_table(), *call),
              "ffgp_acq_optimize_chain_tree_staged")


class PosteriorCache:
    """Keeps the `Posterior` of a model while the SAME tensor objects (training inputs, targets, every parameter) come
    back with unchanged in-place version counters: in-place updates bump `_version`, `p.data = ...` moves the pointer,
    and weak references make sure a recycled address can never alias.  Not part of a model's state (pickles empty).

    Invalidation rule: edits that bypass the version counter -- `p.data.copy_(...)`, `.data.clamp_()`, writes through a
    numpy array that shares the tensor's memory (`torch.from_numpy`) -- are NOT seen; call the model's
    `clear_posterior_cache()` after such an edit (the reference refactorises on every call and needs no such rule).  The
    cache pins one N x N fp64 factor per model (2 GB at N = 16384); `clear_posterior_cache()` releases it, and
    `model.cache_posterior = False` turns the cache off for that model (every call refactorises, as the reference)."""

    def __init__(self):
        self._c = None
        self.enabled = True

    def __getstate__(self):
        return {"_c": None, "enabled": self.enabled}

    def get(self, objs, build):
        """(posterior, fresh): the cached one if `objs` are unchanged, else `build()` (which is then cached)"""
        vers = tuple((t._version, t.data_ptr()) for t in objs)
        c = self._c
        if c is not None and len(c[0]) == len(objs) and all(r() is t for r, t in zip(c[0], objs)) and c[1] == vers:
            return c[2], False
        post = build()
        self._c = ([weakref.ref(t) for t in objs], vers, post) if self.enabled else None
        return post, True

    @property
    def posterior(self):
        return self._c[2] if self._c is not None else None

    def clear(self):
        self._c = None


class PosteriorCacheMixin:
    """`clear_posterior_cache()` / `cache_posterior` for the GP modules that keep a `_pcache` (see PosteriorCache)."""

    def clear_posterior_cache(self):
        self._pcache.clear()

    @property
    def cache_posterior(self):
        return self._pcache.enabled

    @cache_posterior.setter
    def cache_posterior(self, on):
        self._pcache.enabled = bool(on)
        if not on:
            self._pcache.clear()
