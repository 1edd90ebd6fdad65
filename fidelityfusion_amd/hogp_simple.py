"""`HOGP_simple` -- the high-order GP block of GAR (reference: FidelityFusion_Models/two_fidelity_models/
hogp_simple.py:15-126, used by GAR.py:27-31,60-66,94,119) on the device.

Same constructor, parameters (`noise_variance`, the shared kernel, `grid`, `mapping_vector`), cached attributes
(`K`, `K_eigen`, `A`, `g`) and return values: `log_likelihood` returns +NLL / (N * prod(d)) with the true pi,
`forward(x_train, x_test)` the posterior mean and the reference's variance expression.

What runs where: the covariance matrices come from the library's assembly (differentiable `kernel_matrix`), every
mode product -- the O(N^2 prod(d)) part: 550 GFLOP each at N = 8192, d = 64 x 64 -- runs on the fp64 matrix-core
GEMM (`functional.matmul_nt`, forward and backward).  Symmetric eigendecompositions: matrices up to 64 x 64 -- the
per-mode kernels -- run on the hand-written LDS Jacobi solver (`ffgp_syevj_small`); an input kernel of 65 ... `LDS_EIGH_MAX_N`
rows can run in one launch on the one-image LDS solver (`ffgp_syev_lds`; see the constant below); a larger N x N input kernel runs on the
library's two-stage solver (`eigh.eigh` -> `ffgp_syevd`: band reduction, bulge chasing, divide & conquer, two
back-transformations; 0.26 s at N = 8192 where rocSOLVER's syevd takes 0.66 s).  No vendor library is called anywhere in
this module (the GPU tests substitute their own `eigen_pairs` built on torch.linalg.eigh as the comparator); "jacobi" is the
round-2 block Jacobi (slow, independent cross-check).  The likelihood's backward is closed-form (`_KronNLL`): GEMMs only,
no differentiation through `eigh`.

Kept quirks: ONE kernel module is shared by the input space and every output mode (:27-29); the per-mode grids are
0..d-1 as float columns; `forward` needs `log_likelihood` to have been called (it reads the cached `K`, `K_eigen`,
`A`, `g`); the "variance" is diag(K) + (A-weighted squared eigenvector products) (:60-75).

`variance_mode` (constructor keyword, attribute): "explicit_inverse" (default; "reference" is accepted as its old name) evaluates
`K_star @ K_x.inverse() @ U_x` in the reference's order of operations (:68) with an EXPLICIT inverse of the jitter-free kernel
matrix followed by two GEMMs -- but the inverse is NOT the reference's LU inverse: it is formed from the eigenpairs the likelihood
call already produced, K_x^-1 = (U / lambda) U^T on the fp64 GEMM (the reference's `.inverse()` is LAPACK's LU; on these
numerically singular matrices -- cond 5e6 ... 1e13 on the fixtures -- any two inverses agree to ~cond * eps, which is also what
the fixtures of the reference's own LU hold this to; tiny or negative computed eigenvalues are amplified by 1 / lambda exactly as
they are by any other inverse of such a matrix).  "eigen"
evaluates the same matrix as `K_star @ (U_x / lambda_x)` without forming the inverse.  Which one is "right" is moot (the
expression is not a variance); the default keeps the reference's arithmetic shape.

`train_many` (below) runs K Adam steps of HOGP blocks -- train_GAR's loop, residual fidelities with their Tensor_linear matrix included -- per
library call (ffgp_train_hogp_raw: the Kronecker likelihood and `_KronNLL`'s backward as device code on raw parameters, n <= 128).
"""
import math

import torch
import torch.nn as nn

from . import functional as F


EIGENSOLVER = "ffgp"    # n > LDS_EIGH_MAX_N: "ffgp" = the library's two-stage solver (default); "jacobi" = its block Jacobi (slow cross-check)
LDS_EIGH_MAX_N = 128    # 64 < n <= this: the one-workgroup LDS solver (ffgp_syev_lds, n <= 128); 64 sends every n > 64 to EIGENSOLVER's route


class eigen_pairs:
    """matrices up to 64 x 64 (the per-mode kernels; tiny input sets) go to the hand-written LDS Jacobi solver
    (`ffgp_syevj_small`), 64 < n <= `LDS_EIGH_MAX_N` to the one-workgroup, one-launch LDS solver (`ffgp_syev_lds`), larger ones --
    the N x N input kernel -- to the library's two-stage solver (`ffgp_syevd`).
    Reference: `eigen_pairs`, two_fidelity_models/hogp_simple.py:15-19.

    There is no vendor or CPU route: the matrix must live on the MI355X.  The pairs of an n > 64 matrix are computed on a
    DETACHED copy (`value`, `vector` carry no autograd history): the likelihood's gradient is the closed form of `_KronNLL`, which
    never differentiates through eigenvectors, and `forward()`'s variance expression treats the cached pairs as constants, as the
    reference's cached `K_eigen` of the last likelihood call are used there (:60-75)."""

    def __init__(self, matrix):
        if not matrix.is_cuda:
            raise F._lib.FFGPError("eigen_pairs: the matrix must be on the GPU (fidelityfusion_amd has no CPU path)")
        if matrix.shape[0] <= 64:
            self.value, self.vector = F.eigh_small(matrix)
        elif matrix.shape[0] <= LDS_EIGH_MAX_N:
            with torch.no_grad():
                ev, Q = F._syev_lds_checked(matrix.detach().to(torch.float64)[None])      # (NaN eigenvalues if the kernel's status is not 0)
                self.value, self.vector = ev[0], Q[0]
        elif EIGENSOLVER in ("ffgp", "jacobi"):
            from . import eigh as _eigh
            with torch.no_grad():
                fn = _eigh.eigh if EIGENSOLVER == "ffgp" else _eigh.jacobi_eigh
                self.value, self.vector = fn(matrix.detach().to(torch.float64))
        else:
            raise ValueError("unknown EIGENSOLVER %r" % (EIGENSOLVER,))


class _InvFromEigen(torch.autograd.Function):
    """K^-1 = (U / lambda) U^T from the eigenpairs of the symmetric K (explicit inverse on the fp64 GEMM); backward
    d K = -K^-1 (d K^-1) K^-1"""

    @staticmethod
    def forward(ctx, K, lam, U):
        Kinv = F.matmul_nt(U / lam.unsqueeze(0), U)
        ctx.save_for_backward(Kinv)
        return Kinv

    @staticmethod
    def backward(ctx, dKi):
        (Kinv,) = ctx.saved_tensors
        t = F.matmul_nt(Kinv, dKi.T.contiguous())          # K^-1 dKi   (K^-1 is symmetric)
        return -F.matmul_nt(t, Kinv), None, None


def mode_dot(t, M, mode):
    """mode-n product (contracts t's axis `mode` with M's axis 1) on the fp64 GEMM"""
    tm = t.movedim(mode, -1)
    r = F.matmul_nt(tm.reshape(-1, tm.shape[-1]), M)
    return r.reshape(*tm.shape[:-1], M.shape[0]).movedim(-1, mode)


def multi_mode_dot(t, Ms):
    for i, M in enumerate(Ms):
        t = mode_dot(t, M, i)
    return t


def _outer(vs):
    """tucker_to_tensor((1, [v_i as columns])): the outer product of the vectors"""
    out = vs[0].reshape(-1)
    for v in vs[1:]:
        out = out.unsqueeze(-1) * v.reshape(*([1] * out.dim()), -1)
    return out


class _KronNLL(torch.autograd.Function):
    """+NLL / numel of vec(Y) ~ N(0, K_0 (x) K_1 (x) ... + diag(tau)) through the per-mode eigendecompositions
    (hogp_simple.py:92-117 of the reference), with a closed-form backward instead of autograd through `eigh`:

        S = (x)K_m + diag(tau),  A = (x)lambda_m + tau,  g = S^-1 y  (the tensor the reference caches as `self.g`)
        dNLL/dY    = g
        dNLL/dA    = 1/2 (1/A - (T_1/A)^2)   elementwise in the eigenbasis, where tau is added (summed for a scalar tau)
        dNLL/dK_m  = 1/2 U_m diag(c_m) U_m^T  -  1/2 g_(m) [g x_{m' != m} K_m']_(m)^T,
                     c_m[i] = sum_{others} (prod_{m' != m} lambda_m') / A

    No eigenvector derivatives (the 1 / (lambda_i - lambda_j) terms of eigh's backward, ill-defined for the clustered
    spectra kernel matrices have) appear; every O(N^2 prod d) / O(N^3) product runs on the fp64 matrix-core GEMM.
    That form holds for the reference's scalar tau = 1/noise (+ scalar y_var).  An elementwise y_var is added to A in
    the eigenbasis (MFGP_ver2023May/base_gp/hogp.py:118), which makes S depend on the eigenvectors themselves; that
    case takes the general eigh pullback, written out in `backward`.
    """

    @staticmethod
    def forward(ctx, cache, y, tau, *Ks):
        es = [eigen_pairs(K) for K in Ks]
        A = _outer([e.value for e in es]) + tau
        Ainv = A.reciprocal()
        T_1 = multi_mode_dot(y, [e.vector.T.contiguous() for e in es])
        W = T_1 * Ainv
        g = multi_mode_dot(W, [e.vector for e in es])
        nd = A.numel()
        nll = 0.5 * nd * math.log(2 * math.pi) + 0.5 * torch.log(A).sum() + 0.5 * (T_1 * W).sum()
        cache.update(eigen=es, A=A, g=g)
        ctx.pack = (es, Ainv, W, g, Ks, tau.shape, nd)
        return nll / nd

    @staticmethod
    def backward(ctx, dl):
        es, Ainv, W, g, Ks, tau_shape, nd = ctx.pack
        s = dl / nd
        need = ctx.needs_input_grad
        dY = g * s if need[1] else None
        dtau = None
        if need[2]:
            # tau sits on A (the eigenbasis diagonal): d/dA [1/2 log A + 1/2 T_1^2 / A] = 1/2 (1/A - W^2)
            dtau = (0.5 * s * (Ainv - W * W)).sum_to_size(tau_shape)
        n = len(Ks)
        dKs = [None] * n
        uniform = math.prod(tau_shape) == 1
        if any(need[3:]):
            P0 = mode_dot(g, Ks[0], 0) if uniform and any(need[4:]) else None   # the one N^2 prod(d) product the modes m >= 1 share
            for m in range(n):
                if not need[3 + m]:
                    continue
                t = Ainv if uniform else Ainv - W * W
                for mp in range(n):
                    if mp != m:
                        shape = [1] * n
                        shape[mp] = -1
                        t = t * es[mp].value.reshape(shape)
                c = t.sum(dim=[a for a in range(n) if a != m])
                U = es[m].vector
                if uniform:
                    term1 = F.matmul_nt(U * c.unsqueeze(0), U)
                    P = g if m == 0 else P0
                    for mp in range(1, n):
                        if mp != m:
                            P = mode_dot(P, Ks[mp], mp)
                    gm = g.movedim(m, 0).reshape(g.shape[m], -1)
                    Pm = P.movedim(m, 0).reshape(g.shape[m], -1)
                    dKs[m] = (0.5 * s) * (term1 - F.matmul_nt(gm, Pm))
                else:
                    # an elementwise tau lives in the eigenbasis, so S depends on the eigenvectors themselves: the
                    # general eigh pullback U (diag(dlambda) + (U^T dU) / (lambda_j - lambda_i)) U^T with U^T dU = T_1(m) W(m)^T
                    lam = es[m].value
                    T1m = (W / Ainv).movedim(m, 0).reshape(g.shape[m], -1)
                    Wm = W.movedim(m, 0).reshape(g.shape[m], -1)
                    E = lam.unsqueeze(0) - lam.unsqueeze(1)
                    E.diagonal().fill_(float("inf"))
                    X = F.matmul_nt(T1m, Wm) / E
                    X.diagonal().add_(0.5 * c)
                    dKs[m] = s * F.matmul_nt(F.matmul_nt(U, X.T.contiguous()), U)
        return (None, dY, dtau) + tuple(dKs)


def kron_nll(y, tau, Ks):
    """(loss, cache): loss = +NLL / numel; cache holds the (detached) `eigen` pairs, `A` and `g` of this evaluation"""
    cache = {}
    loss = _KronNLL.apply(cache, y, tau, *Ks)
    return loss, cache


class HOGP_simple(nn.Module):
    def __init__(self, kernel, noise_variance, output_shape, learnable_grid=False, learnable_map=False,
                 variance_mode="explicit_inverse"):
        super().__init__()
        if variance_mode == "reference":          # (the mode's name until round 4: it never was the reference's LU inverse)
            variance_mode = "explicit_inverse"
        if variance_mode not in ("explicit_inverse", "eigen"):
            raise ValueError("variance_mode must be 'explicit_inverse' or 'eigen', got %r" % (variance_mode,))
        self.variance_mode = variance_mode
        self.noise_variance = nn.Parameter(torch.tensor([noise_variance]))
        self.K = []
        self.K_eigen = []
        self.kernel_list = nn.ModuleList([kernel for _ in range(len(output_shape) + 1)])   # the same module, shared
        self.grid = nn.ParameterList([nn.Parameter(torch.tensor(range(v)).reshape(-1, 1).float()) for v in output_shape])
        if learnable_grid is False:
            for p in self.grid:
                p.requires_grad = False
        self.mapping_vector = nn.ParameterList([nn.Parameter(torch.eye(v)) for v in output_shape])
        if learnable_map is False:
            for p in self.mapping_vector:
                p.requires_grad = False

    def _dev(self):
        return F._device_of(*list(self.parameters()))

    def _kernel(self, i, a, b):
        """kernel_list[i](a, b) on the device in fp64; a 1-column grid meets a D-dimensional ARD kernel through the
        same broadcast the reference's `x / length_scales` performs"""
        k = self.kernel_list[i]
        ls = getattr(k, "length_scales", None)
        if ls is not None and a.shape[1] == 1 and ls.numel() > 1:
            a, b = a.expand(-1, ls.numel()), b.expand(-1, ls.numel())
        return F.kernel_on_device(k, a, b)

    def log_likelihood(self, x_train, y_train):
        if isinstance(y_train, list):
            y_train = y_train[0]          # the variance part is not used (reference :83-86,108-109)
        dev = self._dev()
        y = y_train.to(device=dev, dtype=torch.float64)
        self.K.clear()
        self._K_inv = None            # (reference variance mode: the explicit inverse is formed once per likelihood call)
        self.K.append(self._kernel(0, x_train, x_train))
        for i in range(len(self.kernel_list) - 1):
            _in = mode_dot(self.grid[i].to(device=dev, dtype=torch.float64), self.mapping_vector[i].to(device=dev, dtype=torch.float64), 0)
            self.K.append(self._kernel(i + 1, _in, _in))
        loss, cache = kron_nll(y, self.noise_variance.to(dev).pow(-1), self.K)
        self.K_eigen[:] = cache["eigen"]
        self.A = cache["A"]
        self.g = cache["g"]
        odt = y_train.dtype if y_train.dtype.is_floating_point else torch.float64
        return loss.to(device=y_train.device, dtype=odt)

    def forward(self, x_train, x_test):
        dev = self._dev()
        K_star = self._kernel(0, x_test, x_train)
        predict_u = multi_mode_dot(self.g, [K_star] + self.K[1:])
        n_dim = len(self.K_eigen) - 1
        diag_K_dims = _outer([K.diag() for K in self.K[1:]]).unsqueeze(0)
        diag_K_x = self._kernel(0, x_test, x_test).diag()
        for _ in range(n_dim):
            diag_K_x = diag_K_x.unsqueeze(-1)
        diag_K = diag_K_x * diag_K_dims
        S_2 = (self.A * self.A.pow(-1 / 2)).pow(2)
        e0 = self.K_eigen[0]
        if self.variance_mode in ("explicit_inverse", "reference"):   # K_star @ K_x^-1 @ U_x in the reference's order of operations (:68)
            if torch.is_grad_enabled() and self.K[0].requires_grad:
                K_inv = _InvFromEigen.apply(self.K[0], e0.value.detach(), e0.vector.detach())
            else:
                if getattr(self, "_K_inv", None) is None:
                    with torch.no_grad():
                        self._K_inv = _InvFromEigen.apply(self.K[0].detach(), e0.value.detach(), e0.vector.detach())
                K_inv = self._K_inv
            ev_x = F.matmul_nt(F.matmul_nt(K_star, K_inv.T.contiguous()), e0.vector.T.contiguous()).pow(2)
        else:                                   # the same matrix from the cached eigenpairs: K_x^-1 U_x = U_x / lambda
            ev_x = mode_dot(K_star, (e0.vector / e0.value.unsqueeze(0)).T.contiguous(), 1).pow(2)
        evs = [ev_x] + [self.K_eigen[i + 1].vector.pow(2) for i in range(n_dim)]
        var_diag = diag_K + multi_mode_dot(S_2, evs)
        odt = x_test.dtype if x_test.dtype.is_floating_point else torch.float64
        return predict_u.to(device=x_test.device, dtype=odt), var_diag.to(device=x_test.device, dtype=odt)


# ---- K Adam steps per library call -------------------------------------------------------------------------------------------
TRAIN_MAX_MODELS = 16      # blocks per ffgp_train_hogp_raw call (include/ffgp.h); longer lists are trained in chunks
TRAIN_MAX_N = 128          # FFGP_SYEV_LDS_MAX_N: the fused loop's eigensolvers end there
TRAIN_MAX_MODE = 64        # points per output mode (ffgp_syevj_small)
TRAIN_MAX_OUT = 4096       # FFGP_HOGP_MAX_OUT: prod(output shape); two images of a sample's tensor live in LDS


class HOGPTrainState:
    """What `train_many` carries between calls.
    fused   which route ran: True = ffgp_train_hogp_raw, False = the reference's loop on the drop-in modules
    buf     (fused) torch.optim.Adam's moments on the device, one row per model: [exp_avg (P) | exp_avg_sq (P)] with the parameters
            in the order [length scale(s) (nw) | signal_variance | noise_variance | the Tensor_linear's last matrix (h * l, row-major;
            residual models only)], P = nw + 2 (+ h * l); `moments(f)` returns the two halves of model f
    npar    P per model
    steps   updates taken per model: after a call in which model f failed at step k, steps[f] has advanced by k, the others by `steps`
    failed  {model index: failing step} of the LAST call (empty: every model completed)
    opts    (reference route) the per-model torch.optim.Adam"""

    def __init__(self, fused, n_models):
        self.fused = fused
        self.buf = None
        self.npar = [0] * n_models
        self.steps = [0] * n_models
        self.failed = {}
        self.opts = [None] * n_models

    def moments(self, f):
        P = self.npar[f]
        return self.buf[f, :P], self.buf[f, P:2 * P]


def _mean_of(y):
    return y[0] if isinstance(y, (list, tuple)) else y


def _train_eligible(model, x, y, res):
    """the description `train_many`'s fused route needs -- the shared kernel's `links()`, the targets or the residual link's tensors --
    or None: see `train_many` for the rule"""
    if not isinstance(model, HOGP_simple) or not isinstance(x, torch.Tensor) or x.dim() != 2:
        return None
    if any(p.requires_grad for p in list(model.grid) + list(model.mapping_vector)):
        return None
    k = model.kernel_list[0]
    if any(kk is not k for kk in model.kernel_list):
        return None
    lk = k.links() if hasattr(k, "links") else None
    if lk is None or lk["kfun"] not in (0, 1, 2, 3) or isinstance(lk.get("kparam"), torch.Tensor):
        return None
    w, amp, nv = lk["w"], lk["amp"], model.noise_variance
    n, D = x.shape
    dims = tuple(int(g.shape[0]) for g in model.grid)
    # (the fused loop routes its eigenproblems as `eigen_pairs` does with the default LDS_EIGH_MAX_N: a lowered constant keeps n above it per-step)
    if not (1 <= n <= max(64, min(TRAIN_MAX_N, LDS_EIGH_MAX_N)) and 1 <= D <= 128 and 1 <= len(dims) <= 3 and all(1 <= d <= TRAIN_MAX_MODE for d in dims)
            and math.prod(dims) <= TRAIN_MAX_OUT):
        return None
    if w.numel() not in (1, D) or amp.numel() != 1 or nv.numel() != 1:
        return None
    if not all(t.requires_grad and t.is_leaf for t in (w, amp, nv)) or x.requires_grad:
        return None
    if {id(p) for p in model.parameters() if p.requires_grad} != {id(w), id(amp), id(nv)}:
        return None      # (a kernel with further learnable parameters)
    # the call forms the mode inputs itself, 0..d-1 under the identity map: a frozen grid or map that holds other values (rescaled, or
    # loaded from a run with learnable_map=True) is not what it would train on
    for gr, mp in zip(model.grid, model.mapping_vector):
        d = gr.shape[0]
        if tuple(gr.shape) != (d, 1) or tuple(mp.shape) != (d, d):
            return None
        if not torch.equal(gr.detach().reshape(-1).double().cpu(), torch.arange(d, dtype=torch.float64)):
            return None
        if not torch.equal(mp.detach().double().cpu(), torch.eye(d, dtype=torch.float64)):
            return None
    out = {"lk": lk, "dims": dims, "V": None}
    if res is None:
        y = _mean_of(y)
        if not isinstance(y, torch.Tensor) or tuple(y.shape) != (n,) + dims or y.requires_grad or not F.raw_ok(x, y, w, amp, nv):
            return None
        out["y"] = y
        return out
    tl, yl, yh = res[0], _mean_of(res[1]), _mean_of(res[2])
    vecs = getattr(tl, "vectors", None)
    if vecs is None or len(vecs) != len(dims) or not isinstance(yl, torch.Tensor) or not isinstance(yh, torch.Tensor):
        return None
    V = vecs[len(dims) - 1]
    if V.dim() != 2 or V.shape[0] != dims[-1] or not (1 <= V.shape[1] <= TRAIN_MAX_MODE) or not (V.requires_grad and V.is_leaf):
        return None
    if tuple(yh.shape) != (n,) + dims or tuple(yl.shape) != (n,) + dims[:-1] + (int(V.shape[1]),) or yl.requires_grad or yh.requires_grad:
        return None
    # (the bilinear initialisation of Tensor_linear is a transposed view: V travels with its strides)
    if not F.raw_ok(x, yl, yh, V if V.is_contiguous() else V.T, w, amp, nv):
        return None
    out.update(V=V, yl=yl, yh=yh)
    return out


def _train_reference(models, xs, ys, steps, lr, betas, eps, state, residual):
    """the reference's loop itself (GAR.py:76-126 per fidelity) on the drop-in modules: one torch.optim.Adam per model over its own
    parameters and, for a residual model, its Tensor_linear's"""
    trace = torch.empty((len(models), steps), dtype=torch.float64)
    for f, (m, x, y) in enumerate(zip(models, xs, ys)):
        res = residual[f] if residual is not None else None
        if state.opts[f] is None:
            pars = list(m.parameters()) + (list(res[0].parameters()) if res is not None else [])
            state.opts[f] = torch.optim.Adam(pars, lr=lr, betas=betas, eps=eps)
        for k in range(steps):
            state.opts[f].zero_grad()
            if res is not None:
                y = _mean_of(res[2]) - res[0](_mean_of(res[1]))
            loss = m.log_likelihood(x, y)
            loss.backward()
            state.opts[f].step()
            trace[f, k] = float(loss.detach())
        state.steps[f] += steps
    return trace.to(xs[0].device)


def train_many(models, xs, ys, steps, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, state=None, residual=None):
    """`steps` Adam iterations on every `HOGP_simple` of `models` (independent blocks; `xs[f]` [n, D], `ys[f]` [n, d_1, ...] or a
    [mean, var] list whose mean is used), each exactly train_GAR's iteration (FidelityFusion_Models/GAR.py:76-126): loss =
    log_likelihood(x, y) (+NLL / numel), gradients, torch.optim.Adam(lr, betas, eps).  Returns `(trace, state)`: trace [F, steps]
    (float64) = the loss of model f at step k BEFORE that step's update, `state` a `HOGPTrainState` to pass back in to continue the
    same optimisers.
    `residual[f]` = (tensor_linear, y_low, y_high) with `ys[f]` = None makes model f one of train_GAR's fidelities above 0: every step
    trains it on y_high - tensor_linear(y_low) and the Tensor_linear's LAST matrix -- the only one that acts
    (gp_computation_pack.Tensor_linear) -- is a further Adam parameter, updated in place.  y_low / y_high may be [mean, var] lists.
    The fused route (ffgp_train_hogp_raw: launch per stage on the device, no host synchronisation inside the loop, up to 16 blocks per
    call) takes a call in which EVERY model is a `HOGP_simple` with learnable_grid = learnable_map = False over a single library radial
    kernel with `links()` and no further learnable parameter, with parameters and data on one GPU in fp64, n <= 128 points and 1-3
    output modes of at most 64 points each whose product is at most 4096, grids and maps at their initial values (0..d-1, identity).
    Any other call runs the reference's loop on the drop-in modules, same return values;
    `state.fused` says which route ran.
    After a fused call the parameters (and the Tensor_linear matrix) hold the trained values, without `.grad`; `K`, `K_eigen`, `A`, `g`
    hold what the per-step loop would have left (those of the last step taken) and `_K_inv` is cleared, so `forward` can follow.
    Failure (fused route): a model whose loss is not finite at some step -- noise_variance crossed zero and an entry of A is not
    positive -- or whose eigensolver does not converge stops ALONE: its trace holds NaN from that step on, its parameters and moments
    the values that step began with, the others complete.  No exception is raised (the reference's loop goes on with NaN silently); a
    RuntimeWarning is issued and `state.failed` = {model: failing step}; `state.steps` advances per model, so continuing with the
    returned state gives a survivor the trajectory of an uninterrupted run."""
    import ctypes as C
    import warnings
    from . import _lib
    models, xs, ys = list(models), list(xs), list(ys)
    nF = len(models)
    if not (nF == len(xs) == len(ys)) or nF == 0 or steps <= 0:
        raise ValueError("train_many: models, xs, ys must have one length and steps must be positive")
    if residual is not None:
        residual = list(residual)
        if len(residual) != nF:
            raise ValueError("train_many: residual must have one entry per model")
    for f in range(nF):
        res = residual[f] if residual is not None else None
        if res is not None and (ys[f] is not None or len(res) != 3):
            raise ValueError("train_many: a residual model takes (tensor_linear, y_low, y_high) and ys[f] = None")
        if res is None and ys[f] is None:
            raise ValueError("train_many: model %d has neither targets nor a residual link" % f)
    elig = [_train_eligible(m, x, y, residual[f] if residual is not None else None) for f, (m, x, y) in enumerate(zip(models, xs, ys))]
    fused = all(e is not None for e in elig) and len({x.device for x in xs}) == 1
    if state is None:
        state = HOGPTrainState(fused, nF)
    if len(state.steps) != nF:
        raise ValueError("train_many: this state belongs to %d models" % len(state.steps))
    state.failed = {}
    if not fused or not state.fused:
        if state.fused:
            raise ValueError("train_many: this state belongs to fused training; the models no longer qualify for it")
        return _train_reference(models, xs, ys, steps, lr, betas, eps, state, residual), state
    dev = xs[0].device
    npar = [e["lk"]["w"].numel() + 2 + (e["V"].numel() if e["V"] is not None else 0) for e in elig]
    stride = 2 * max(npar)
    if state.buf is None:
        state.buf = torch.zeros((nF, stride), dtype=torch.float64, device=dev)
        state.npar = npar
    elif state.npar != npar or state.buf.device != dev:
        raise ValueError("train_many: this state belongs to other models")
    trace = torch.empty((nF, steps), dtype=torch.float64, device=dev)
    opt = _lib.Adam(float(lr), float(betas[0]), float(betas[1]), float(eps))
    h = _lib.handle(dev.index)
    _lib.bind_stream(h, dev.index)
    for c0 in range(0, nF, TRAIN_MAX_MODELS):
        idx = list(range(c0, min(c0 + TRAIN_MAX_MODELS, nF)))
        nc = len(idx)
        M = (_lib.HogpModel * nc)()
        L = (_lib.Links * nc)()
        R = (_lib.HogpResidual * nc)()
        Cc = (_lib.HogpCache * nc)()
        s0 = (C.c_long * nc)(*[state.steps[f] for f in idx])
        fail = (C.c_int * nc)()
        outs = []
        for j, f in enumerate(idx):
            e, x = elig[f], xs[f]
            lk, dims = e["lk"], e["dims"]
            n, D = x.shape
            M[j].n, M[j].D, M[j].X_dev, M[j].nmodes = n, D, x.data_ptr(), len(dims)
            for q, d in enumerate(dims):
                M[j].dims[q] = d
            M[j].w_dev, M[j].amp_dev, M[j].noise_dev = lk["w"].data_ptr(), lk["amp"].data_ptr(), models[f].noise_variance.data_ptr()
            kp = lk.get("kparam")
            M[j].clamp_min, M[j].kfun, M[j].kparam = lk["clamp"], lk["kfun"], (1.0 if kp is None else float(kp))
            L[j].w_link, L[j].w_c, L[j].w_broadcast = lk["w_link"], lk["w_c"], 1 if lk["w"].numel() == 1 and D > 1 else 0
            L[j].amp_link, L[j].amp_c, L[j].out_scale = lk["amp_link"], 0.0, 1.0
            if e["V"] is not None:
                R[j].V_dev, R[j].y_low_dev, R[j].y_high_dev, R[j].l = e["V"].data_ptr(), e["yl"].data_ptr(), e["yh"].data_ptr(), e["V"].shape[1]
                R[j].V_row_stride, R[j].V_col_stride = e["V"].stride(0), e["V"].stride(1)
            else:
                M[j].Y_dev = e["y"].data_ptr()
            sizes = (n,) + dims
            o = {"K": [torch.empty((d, d), dtype=torch.float64, device=dev) for d in sizes],
                 "U": [torch.empty((d, d), dtype=torch.float64, device=dev) for d in sizes],
                 "lam": [torch.empty((d,), dtype=torch.float64, device=dev) for d in sizes],
                 "A": torch.empty(sizes, dtype=torch.float64, device=dev), "g": torch.empty(sizes, dtype=torch.float64, device=dev)}
            for q in range(len(sizes)):
                Cc[j].K_dev[q], Cc[j].evals_dev[q], Cc[j].evecs_dev[q] = o["K"][q].data_ptr(), o["lam"][q].data_ptr(), o["U"][q].data_ptr()
            Cc[j].A_dev, Cc[j].g_dev = o["A"].data_ptr(), o["g"].data_ptr()
            outs.append(o)
        st = state.buf[c0:c0 + nc]
        _lib.check(_lib.lib.ffgp_train_hogp_raw(h, nc, M, L, R, int(steps), C.byref(opt), st.data_ptr(), st.stride(0), s0,
                                                trace[c0:c0 + nc].data_ptr(), trace.stride(0), Cc, fail), "ffgp_train_hogp_raw")
        for j, f in enumerate(idx):
            if fail[j] >= 0:
                state.failed[f] = int(fail[j])
                state.steps[f] += int(fail[j])
            else:
                state.steps[f] += steps
            m, o = models[f], outs[j]
            m.K[:] = o["K"]
            pairs = []
            for lam, U in zip(o["lam"], o["U"]):
                ep = object.__new__(eigen_pairs)
                ep.value, ep.vector = lam, U
                pairs.append(ep)
            m.K_eigen[:] = pairs
            m.A, m.g, m._K_inv = o["A"], o["g"], None
    # the library wrote the parameters behind autograd's back: bump their version counters
    bump = getattr(torch.autograd.graph, "increment_version", None)
    with torch.no_grad():
        for e, m in zip(elig, models):
            for q in [e["lk"]["w"], e["lk"]["amp"], m.noise_variance] + ([e["V"]] if e["V"] is not None else []):
                if bump is not None:
                    bump(q)
                else:
                    q.add_(0.0)
    if state.failed:
        warnings.warn("hogp_simple.train_many: the loss of model(s) %s stopped being finite (or their eigensolver did not converge) at "
                      "step(s) %s; they kept the parameters that step began with" %
                      (sorted(state.failed), [state.failed[f] for f in sorted(state.failed)]), RuntimeWarning)
    return trace, state
