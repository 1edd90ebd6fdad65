"""K Adam training steps per library call (`train_many`): the reference's hot loop -- per fidelity 100-1000 iterations of
`optimizer.zero_grad(); loss = -model.negative_log_likelihood(x, y); loss.backward(); optimizer.step()`
(FidelityFusion_Models/ResGP.py:78-112, AR_autoRegression.py:95-137, GaussianProcess/cigp_v10.py:92-104) at N = 16 ... 500 -- runs
as ONE call of ffgp_train_raw: likelihood, closed-form gradients and torch.optim.Adam's update of the raw parameters on the device,
the loss trace returned, the factorisation status read once.  Through the drop-in modules a step costs 0.28-0.32 ms at N <= 128 (one
Python round trip, one autograd graph, one status read-back); here it costs its GPU work.
Models whose kernel is a SumKernel / ProductKernel tree of up to four library kernels -- SumKernel(LinearKernel, MaternKernel) is the
kernel of the reference's demos and two-fidelity models -- take the same route through ffgp_train_tree_raw (launch per stage, every size),
or, with `tree_one_launch=True` and at most TREE_ONE_LAUNCH_MAX_N points, through ffgp_train_tree_lds_raw: one launch for all their steps.
With `wide_one_launch=True` single-kernel `cigp` models of at most 128 points with MORE than 16 target columns -- CIGAR's fidelity 0 on a
field, ResGP's and AR's residual fidelities -- are trained in one launch as well (ffgp_train_wide_raw), on targets compressed to at most
n (a residual member: 2 n) columns by `compress_targets`.
With `fuse_composed=True` train_AR's residual fidelities on such a kernel and `GP_basic` blocks over one are trained by the library too
(ffgp_train_tree_res_raw; in one launch: ffgp_train_tree_lds_res_raw).
`residual[f]` = (tensor_linear, y_low, y_high) makes model f one of train_CIGAR's fidelities above 0 (FidelityFusion_Models/CIGAR.py:110-134):
a `cigp` on y_high - Tensor_linear(y_low) with the map's matrix under the same Adam (ffgp_train_tlin_raw: one launch for all steps up to
128 points with D, h <= 16, launch per stage above).
"""
import ctypes as C

import torch

from . import _lib
from ._common import _raise_not_pd
from ._lib import FFGP_LL_V1, Problem, check, lib

TRAIN_MAX_MODELS = 16      # models per ffgp_train_raw call (include/ffgp.h); longer lists are trained in chunks
TRAIN_THREADS = 4          # host threads (handle + stream each) that train the larger models of one call side by side
TREE_ONE_LAUNCH_MAX_N = 128   # composed-kernel models up to this size take ffgp_train_tree_lds_raw under `tree_one_launch=True`: the largest
                              # N at which it beat the launch-per-stage call by more than the run's spread (profiles/train_tree_lds_bench.txt)


WIDE_KFUN_MAX = 3             # ffgp_train_wide_raw covers FFGP_KFUN_SE ... FFGP_KFUN_MATERN52


def compress_targets(*mats):
    """Row blocks of Z_eff with Z_eff Z_eff^T = Z Z^T, Z the matrices [n_i, d] stacked row-wise (m = sum n_i rows): the V1 likelihood
    and its gradients -- a residual member's dloss/drho included -- depend on the targets only through inner products of their rows, so
    training on the blocks of Z_eff [m, m] in place of the matrices gives the same loss and gradients whatever d is, as long as the
    likelihood keeps the true d in its log-determinant term and constant (ffgp_train_wide_raw's d_true).  Z_eff = U sqrt(max(Lambda, 0))
    from the eigendecomposition of the Gram Z Z^T: the Gram on the fp64 GEMM, the decomposition on the package's own solver (the
    one-workgroup LDS solver up to 128 rows, the two-stage solver above: a residual member at n = 128 has m = 256), negative
    eigenvalues -- rounding -- clamped to zero.  With d <= m there is nothing to gain and the inputs come back unchanged."""
    from . import eigh as E
    from . import functional as F
    m, d = sum(t.shape[0] for t in mats), mats[0].shape[1]
    if d <= m:
        return mats
    with torch.no_grad():
        Z = torch.cat(mats, 0) if len(mats) > 1 else mats[0]
        G = F.matmul_nt(Z, Z)
        if m <= 128:
            ev, U = F._syev_lds_checked(G[None])
            ev, U = ev[0], U[0]
        else:
            ev, U = E.eigh(G)
        Zeff = U * ev.clamp_min(0.0).sqrt()
        out, r0 = [], 0
        for t in mats:
            out.append(Zeff[r0:r0 + t.shape[0]].contiguous())
            r0 += t.shape[0]
    return tuple(out)


class AdamState:
    """torch.optim.Adam's per-parameter state of the models of one `train_many` chunk, kept on the device between calls:
    buf[f] = [exp_avg (nw + 2) | exp_avg_sq (nw + 2)] in the order length scales, signal variance, log_beta (a residual model:
    [exp_avg (nw + 3) | exp_avg_sq (nw + 3)], rho last; a `GP_basic`: noise_variance in log_beta's place; a CAR model: [exp_avg (nw + 5) |
    exp_avg_sq (nw + 5)] in the order length scales, signal variance, noise_variance, b, l_z, sigma_z; a model with a `Tensor_linear`
    link: [exp_avg (P) | exp_avg_sq (P)], P = nw + 2 + h l, in the order length scales, signal variance, log_beta, the map's matrix V [h, l]
    row-major -- whatever V's strides are); `step` = updates taken.
    A chunk of composed-kernel models (ffgp_train_tree_raw): buf[f] = [exp_avg (P) | exp_avg_sq (P)], P = sum over the leaves of
    (length scales + 1 + the centre's D for a LinearKernel) + 1, in the order leaf by leaf in the tree's canonical leaf order
    (`kernel._Pair.tree_links`: length scales, signal variance, centre), then log_beta (a `GP_basic`: noise_variance); a residual member
    of such a chunk (ffgp_train_tree_res_raw): [exp_avg (P + 1) | exp_avg_sq (P + 1)], rho last."""

    def __init__(self, buf, stride, step=0):
        self.buf, self.stride, self.step = buf, stride, step


def _jitter_and_pi():
    from .cigp_v10 import JITTER, PI
    return JITTER, PI


def _eligible(model, x, y, fuse_composed=False):
    """the model's links when ffgp_train_raw can train it: a `cigp` (or a `GP_basic`: `_eligible_gp_basic`) with a library kernel whose raw-parameter path applies (everything
    on one GPU in fp64, no learnable profile parameter, no gradient-carrying inputs), all three parameters trainable"""
    from . import functional as F
    if isinstance(y, list):
        y, y_var = y[0], y[1]
    else:
        y_var = None
    from .gp_basic import GP_basic
    if isinstance(model, GP_basic):
        return _eligible_gp_basic(model, x, y, y_var, fuse_composed)
    if not (hasattr(model, "kernel") and hasattr(model, "log_beta")):
        return None
    if y_var is not None and not F.raw_ok(y_var):
        return None
    if hasattr(model.kernel, "tree_links"):      # SumKernel / ProductKernel: ffgp_train_tree_raw, or the reference's loop
        return _eligible_tree(model, x, y, y_var)
    with torch.enable_grad():
        lk = F.raw_path(model.kernel, x, y, model.log_beta)
    if lk is None or isinstance(lk.get("kparam"), torch.Tensor) or y.requires_grad:
        return None
    if not (lk["w"].requires_grad and lk["amp"].requires_grad and model.log_beta.requires_grad):
        return None
    if {id(q) for q in model.parameters()} != {id(lk["w"]), id(lk["amp"]), id(model.log_beta)}:
        return None      # a kernel with further learnable parameters (MaternKernel's rho is a constant; RQ's alpha is not)
    return lk, y, y_var


def _eligible_gp_basic(model, x, y, y_var, fuse_composed=False):
    """`_eligible` for a `GP_basic` (GaussianProcess/gp_basic.py): Sigma = K + noise_variance^2 I without jitter and the FFGP_LL_V2
    likelihood.  The links dict carries the two differences from a `cigp`: "diag" = (raw diagonal parameter, its link, its constant)
    and "ll" = (variant, pi).  A list y (the FULL y_var matrix enters Sigma), a composed kernel or further parameters: the reference's loop.
    Under `fuse_composed` a composed kernel goes by `_eligible_tree`'s rules, noise_variance in log_beta's place."""
    import math
    from . import functional as F
    if y_var is not None or not isinstance(y, torch.Tensor):
        return None
    nv = model.noise_variance
    if hasattr(model.kernel, "tree_links"):
        if not fuse_composed:
            return None
        e = _eligible_tree(model, x, y, None, nv)
        if e is not None:
            e[0]["diag"] = (nv, _lib.LINK_SQUARE, 0.0)
            e[0]["ll"] = (_lib.FFGP_LL_V2, math.pi)
        return e
    with torch.enable_grad():
        lk = F.raw_path(model.kernel, x, y, nv)
    if lk is None or isinstance(lk.get("kparam"), torch.Tensor) or y.requires_grad or nv.numel() != 1:
        return None
    if not (lk["w"].requires_grad and lk["amp"].requires_grad and nv.requires_grad):
        return None
    if {id(q) for q in model.parameters()} != {id(lk["w"]), id(lk["amp"]), id(nv)}:
        return None
    lk = dict(lk)
    lk["diag"] = (nv, _lib.LINK_SQUARE, 0.0)
    lk["ll"] = (_lib.FFGP_LL_V2, math.pi)
    return lk, y, None


def _eligible_car(model, x, car):
    """`_eligible` for one of train_CAR's fidelities above 0 (`car` = (b, y_low, y_high)): a `GP_basic` (or `cigp`) over a
    `kernel.FidelityKernelMCMC` whose base kernel is a library radial kernel with `links()`, a one-element l_z, everything on one GPU in
    fp64, and exactly the six groups of parameters -- the base kernel's two, l_z, sigma_z, b, the noise parameter -- all trainable.
    The links dict is the base kernel's, with "car" = the kernel's `car_links()` (the samples of this call inside)."""
    import math
    from . import functional as F
    from .kdesc import FFGP_KFUN_LINEAR
    b, yl, yh = car
    k = model.kernel
    cl = k.car_links()      # (draws the samples: the global generator is left as one reference step leaves it)
    lk = cl["base"]
    from .gp_basic import GP_basic
    v1 = hasattr(model, "log_beta")
    if not (v1 or isinstance(model, GP_basic)):
        return None
    dpar = model.log_beta if v1 else model.noise_variance
    if lk is None or lk["kfun"] == FFGP_KFUN_LINEAR or isinstance(lk.get("kparam"), torch.Tensor) or cl["l_z"].numel() != 1:
        return None
    if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.shape[1] <= 128 and isinstance(yl, torch.Tensor) and isinstance(yh, torch.Tensor)):
        return None
    pars = [lk["w"], lk["amp"], dpar, cl["l_z"], cl["sigma_z"], b]
    if not F.raw_ok(x, yl, yh, *pars):
        return None
    if yh.dim() != 2 or yh.shape[0] != x.shape[0] or yl.shape != yh.shape or x.requires_grad or yl.requires_grad or yh.requires_grad:
        return None
    if lk["w"].numel() not in (1, x.shape[1]) or lk["amp"].numel() != 1 or dpar.numel() != 1 or cl["sigma_z"].numel() != 1 or b.numel() != 1:
        return None
    if not all(t.requires_grad and t.is_leaf for t in pars) or cl["z1"].numel() > 128:
        return None
    if len({id(t) for t in pars}) != 6 or {id(q) for q in model.parameters()} != {id(t) for t in pars}:
        return None
    lk = dict(lk)
    lk["car"] = cl
    if not v1:
        lk["diag"] = (dpar, _lib.LINK_SQUARE, 0.0)
        lk["ll"] = (_lib.FFGP_LL_V2, math.pi)
    return lk, yh, None


def _car_targets(car, b):
    """train_CAR's residual at this b (CAR_ContinuousAutoRegression.py:134-136): [y_high - exp(b) * y_low, None]"""
    with torch.no_grad():
        return [car[2] - b.exp() * car[1], None]


def _loss(m, x, y):
    """the loss the reference's loops minimise: -negative_log_likelihood of a `cigp`, -log_likelihood of a `GP_basic` (train_CAR,
    CAR_ContinuousAutoRegression.py:116-142)"""
    if hasattr(m, "negative_log_likelihood"):
        return -m.negative_log_likelihood(x, y)
    return (-m.log_likelihood(x, y)).sum()


def _eligible_tree(model, x, y, y_var, dpar=None):
    """`_eligible` for a composed kernel: ({"tree": (leaf modules, (shape, ops), leaf links)}, y, y_var) when ffgp_train_tree_raw can
    train the model -- `kernel.tree_links()` applies, everything fp64, contiguous and on one GPU, every leaf parameter (length scales,
    signal variance, a linear leaf's centre) and log_beta (`dpar`: a `GP_basic`'s noise_variance in its place) trainable and together
    exactly the model's parameters, data without gradients"""
    from . import functional as F
    dpar = model.log_beta if dpar is None else dpar
    tl = model.kernel.tree_links()
    if tl is None or not (isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor)):
        return None
    pars = [t for lk in tl[2] for t in (lk["w"], lk["amp"], lk.get("center")) if t is not None] + [dpar]
    if not F.raw_ok(x, y, y_var, *pars):
        return None
    if x.dim() != 2 or y.dim() != 2 or x.shape[0] != y.shape[0] or x.shape[1] > 128 or dpar.numel() != 1:
        return None
    D = x.shape[1]
    for lk in tl[2]:
        if lk["w"].numel() not in (1, D) or lk["amp"].numel() != 1 or (lk.get("center") is not None and lk["center"].numel() != D):
            return None
    if x.requires_grad or y.requires_grad or (y_var is not None and y_var.requires_grad) or not all(t.requires_grad for t in pars):
        return None
    if len({id(t) for t in pars}) != len(pars) or {id(q) for q in model.parameters()} != {id(t) for t in pars}:
        return None
    return {"tree": tl}, y, y_var


def _is_tree(e):
    return e is not None and "tree" in e[0]


def _split_residual(res):
    """(rho, y_low, y_high) in train_AR's forms -> rho, y_low mean, y_high mean, v_low, v_high (the variances None in the subset form)"""
    rho, yl, yh = res
    if isinstance(yl, (list, tuple)):
        return rho, yl[0], yh[0], yl[1], yh[1]
    return rho, yl, yh, None, None


def _is_tlin(res):
    """a residual link whose first entry is a `Tensor_linear` module (train_CIGAR's form) instead of a scalar rho (train_AR's)"""
    return res is not None and isinstance(res[0], torch.nn.Module)


def _tlin_ok(res, x, e):
    """a `Tensor_linear` link the fused call can train on a model with links `e`: a one-mode map whose matrix V = vectors[-1] [h, l] is
    an fp64 leaf that requires grad on x's device (contiguous, or the transposed view of the bilinear initialisation), y_low [n, l] and
    y_high [n, h] fp64, contiguous, without gradient, variances [n, n] on both sides or on neither; the model a plain `cigp` over one
    radial library kernel"""
    from . import functional as F
    from .kdesc import FFGP_KFUN_LINEAR
    tl, yl, yh, vl, vh = _split_residual(res)
    vecs = getattr(tl, "vectors", None)
    if vecs is None or len(vecs) != 1 or _is_tree(e) or "diag" in e[0] or e[0]["kfun"] == FFGP_KFUN_LINEAR:
        return False
    V = vecs[0]
    if not (isinstance(V, torch.Tensor) and V.dim() == 2 and V.dtype == torch.float64 and V.device == x.device and V.requires_grad and V.is_leaf
            and (V.is_contiguous() or V.T.is_contiguous()) and {id(q) for q in tl.parameters()} == {id(V)}):
        return False
    n, (h, l) = x.shape[0], V.shape
    for t, c in ((yl, l), (yh, h)):
        if not (isinstance(t, torch.Tensor) and tuple(t.shape) == (n, c) and t.dtype == torch.float64 and t.device == x.device
                and t.is_contiguous() and not t.requires_grad):
            return False
    if (vl is None) != (vh is None) or not 1 <= l <= h:
        return False
    for v in (vl, vh):
        if v is not None and not (isinstance(v, torch.Tensor) and tuple(v.shape) == (n, n) and v.device == x.device and not v.requires_grad
                                  and F.raw_ok(v)):
            return False
    return True


def _tlin_targets(res, V):
    """train_CIGAR's residual at this V (CIGAR.py:119-123): [y_high - y_low V^T, |v_high - v_low| or None]"""
    _, yl, yh, vl, vh = _split_residual(res)
    with torch.no_grad():
        return [yh - yl @ V.T, None if vl is None else (vh - vl).abs()]


def _residual_targets(res, rho):
    """train_AR's residual at this rho (AR_autoRegression.py:125-126,131-132): [y_high - rho * y_low, |v_high - rho * v_low| or None]"""
    _, yl, yh, vl, vh = _split_residual(res)
    with torch.no_grad():
        return [yh - rho * yl, None if vl is None else (vh - rho * vl).abs()]


def _reference_loop(models, xs, ys, steps, lr, betas, eps, opts, residual=None, targets=None, car=None):
    """the reference's loop itself (one torch.optim.Adam per model, rho in a residual model's; a CAR model's b is one of its own
    parameters): models that the fused call cannot train"""
    trace = torch.empty((len(models), steps), dtype=torch.float64)
    for f, (m, x, y) in enumerate(zip(models, xs, ys)):
        res = residual[f] if residual is not None else None
        cr = car[f] if car is not None else None
        if opts[f] is None:
            extra = [] if res is None else (list(res[0].parameters()) if _is_tlin(res) else [res[0]])
            opts[f] = torch.optim.Adam(list(m.parameters()) + extra, lr=lr, betas=betas, eps=eps)
        for k in range(steps):
            opts[f].zero_grad()
            if _is_tlin(res):        # train_CIGAR's residual at the current map, with its graph (CIGAR.py:116-133)
                tl, yl, yh, vl, vh = _split_residual(res)
                y = [yh - tl(yl), (vh - vl).abs()] if vl is not None else yh - tl(yl)
                if k == steps - 1:
                    targets[f] = [y[0].detach(), y[1].detach()] if vl is not None else [y.detach(), None]
            elif res is not None:    # the residual at the current rho, with its graph (AR_autoRegression.py:123-137)
                rho, yl, yh, vl, vh = _split_residual(res)
                y = [yh - rho * yl, (vh - rho * vl).abs()] if vl is not None else yh - rho * yl
                if k == steps - 1:
                    targets[f] = [y[0].detach(), y[1].detach()] if vl is not None else [y.detach(), None]
            if cr is not None:       # train_CAR's residual at the current b, with its graph (CAR_ContinuousAutoRegression.py:132-139)
                y = cr[2] - cr[0].exp() * cr[1]
                if k == steps - 1:
                    targets[f] = [y.detach(), None]
            loss = _loss(m, x, y)
            loss.backward()
            opts[f].step()
            trace[f, k] = float(loss.detach())
    return trace


def _residual_ok(res, x):
    """a residual link the fused call can train: a one-element fp64 rho that requires grad, fp64 targets [n, d] (and [n, n] variances)
    on x's device that carry no gradient"""
    from . import functional as F
    rho, yl, yh, vl, vh = _split_residual(res)
    if not (isinstance(rho, torch.Tensor) and rho.numel() == 1 and rho.dtype == torch.float64 and rho.device == x.device and rho.requires_grad
            and rho.is_leaf):
        return False
    n = x.shape[0]
    for t in (yl, yh):
        if not (isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[0] == n and t.shape == yh.shape and t.dtype == torch.float64
                and t.device == x.device and t.is_contiguous() and not t.requires_grad):
            return False
    if (vl is None) != (vh is None):
        return False
    for v in (vl, vh):
        if v is not None and not (isinstance(v, torch.Tensor) and v.dim() == 2 and tuple(v.shape) == (n, n) and v.device == x.device
                                  and not v.requires_grad and F.raw_ok(v)):
            return False
    return True


def train_many(models, xs, ys, steps, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, state=None, residual=None, tree_one_launch=False, car=None,
               fuse_composed=False, wide_one_launch=False):
    """`steps` Adam iterations on every model of `models` (independent `cigp` models, `xs[f]`, `ys[f]` their training data; y may be
    `[y, y_var]`), each exactly the reference's iteration (FidelityFusion_Models/ResGP.py:82-88): loss = -negative_log_likelihood,
    gradients of the three raw parameters, torch.optim.Adam(lr, betas, eps) update.  Returns `(trace, state)`:
    trace [F, steps] (float64, on the models' device) = the loss of model f at step k BEFORE that step's update -- what the reference
    prints -- and `state`, to be passed back in to continue the same optimisers (`state=None`: fresh optimisers).
    `GP_basic` models (noise_variance^2 on the diagonal, no jitter, the FFGP_LL_V2 likelihood; loss = -log_likelihood as train_CAR's
    loop minimises it) with a library kernel and a plain-tensor y train the same way, and may share a call with `cigp` models.
    Models on one GPU in fp64 with a library kernel are trained by ffgp_train_raw, up to 16 per call (small models -- N <= 128, D,
    d <= 16 -- take ONE kernel launch for ALL their steps: csrc/train.hip, a persistent workgroup per model); anything else runs the
    reference's loop through the drop-in modules.
    Models whose kernel is a SumKernel / ProductKernel composition with `tree_links()` (2-4 library kernels, LinearKernel with its
    trained centre included; every leaf parameter and log_beta trainable, and nothing else) are trained by ffgp_train_tree_raw, launch
    per stage: those of at most 128 points up to 16 per call -- calls of their own, beside the plain and residual models' -- and every
    larger one in a call of its own, side by side with the other large models.  A not-PD Sigma in one model of such a call stops all
    of that call's models at that step.  A composed-kernel model given a `residual=` link is NOT fused unless `fuse_composed` (below): it (and with it the whole
    `train_many` call, state["fused"] = False) keeps the reference's loop, as do compositions with a RationalQuadraticKernel leaf, a
    module used as two leaves, or kernel.FUSE_PAIRS = False.
    `tree_one_launch=True` sends the composed-kernel models of at most TREE_ONE_LAUNCH_MAX_N points with D <= 16 and d <= 16 through
    ffgp_train_tree_lds_raw instead, up to 16 per call: ONE kernel launch for all their steps (csrc/train_tree_lds.hip, a persistent
    workgroup per model), with the plain small models' failure rule -- a not-PD Sigma stops that model alone, the others of the call
    complete their steps.  The Adam state has the same layout on both routes, so a `state` may be continued with either value of the
    keyword; the two routes agree to rounding, not bit for bit.  Every other model is routed as without the keyword.
    state["tree_one_launch"] lists the indices of the models that took this route in the last call.
    `fuse_composed=True` (off by default: without it nothing changes) fuses two kinds of model that otherwise keep the loop.  A
    `cigp` over a composed kernel with a `residual=` link -- both forms, subset and non-subset with [n, n] variances -- is trained by
    ffgp_train_tree_res_raw (csrc/train_tree_res.hip: launch per stage at every size; per step one launch forms the residual members'
    targets, and the Adam launch reduces dloss/drho in a fixed order and moves P + 1 parameters), and a `GP_basic` over a composed
    kernel goes through the tree entries with noise_variance under the square link, no jitter and the FFGP_LL_V2 likelihood --
    `_eligible_tree`'s rules with noise_variance in log_beta's place; plain targets, or a residual link in the subset form (a list y or
    residual variances would add a FULL matrix to Sigma: the reference's loop, as before).  Plain and residual tree members of at most
    128 points may share a call; larger ones run side by side.  Under `tree_one_launch=True` the members of at most 128 points (D, d <= 16)
    go to ffgp_train_tree_lds_res_raw instead -- ONE launch for all steps of a chunk's V1 members and one for its V2 members, a member
    that is not positive definite stops alone -- and state["tree_one_launch"] lists them; the state is portable between the routes.  state["residual_targets"][f] and the parameters' version
    counters behave as for residual members on a single radial kernel.
    A Sigma that is not positive definite raises torch.linalg.LinAlgError as the reference's loop would; the failing model's parameters
    then hold the values they had when that step began (the other small models of the same call have completed their steps; the
    optimiser state of a failed call is not advanced).
    Two differences from running the loop yourself: the parameters are updated in place on the device and are left WITHOUT `.grad`
    (there is no autograd pass), and the Adam moments live in the returned `state`, not in a `torch.optim.Adam` -- there is no
    `optimizer.state_dict()` to checkpoint; keep `state` (and the step count inside it) instead.
    `residual[f]` = (rho, y_low, y_high) makes model f one of train_AR's residual fidelities (AR_autoRegression.py:123-137; `ys[f]` is then
    None): every step trains it on y_high - rho * y_low -- y_low, y_high tensors [n, d] (subset form) or [mean, var] lists with var [n, n]
    (then |v_high - rho * v_low| is the y_var whose diagonal enters Sigma) -- and rho (a one-element fp64 parameter) is a fourth Adam
    parameter, updated in place like the others.  state["residual_targets"][f] = [res_mean, res_var] (res_var None in the subset form)
    is that residual at the rho of the start of the last step, computed with torch: what train_AR hands to add_data.
    `residual[f]` = (tensor_linear, y_low, y_high) -- a `gp_computation_pack.Tensor_linear` in rho's place, the form `hogp_simple.train_many`
    takes -- makes model f one of train_CIGAR's fidelities above 0 (CIGAR.py:110-134; `ys[f]` is then None): every step trains it on
    y_high - tensor_linear(y_low) -- y_low [n, l], y_high [n, h] tensors (subset form) or [mean, var] lists with var [n, n] (then
    |v_high - v_low|, which does not depend on the map, is the y_var whose diagonal enters Sigma) -- and the map's matrix V = vectors[-1]
    [h, l] is h l further Adam parameters, updated in place through its strides (the bilinear initialisation for l < h is a transposed
    view) with its version counter bumped like the others.  Fused (ffgp_train_tlin_raw) when the map has one mode, V is an fp64 leaf that
    requires grad on the model's GPU, y_low / y_high are fp64, contiguous and carry no gradient, variances are [n, n] on both sides or on
    neither, and the model is eligible as a plain `cigp` over one radial library kernel; a multi-mode map, a composed kernel, a `GP_basic` or
    CPU tensors run the reference's loop instead (Adam over the model's parameters plus the map's; state["fused"] = False; same return
    values).  Link members form chunks of their own -- those with n <= 128, D <= 16, h <= 16 up to 16 per call, trained in ONE launch for
    all steps (csrc/train.hip: V, its moments and its gradient in LDS; a member that is not positive definite stops alone), every larger
    one a call of its own, launch per stage, the two products y_low V^T and dloss/dV = -A^T y_low on the fp64 GEMM from n l h = 8192 on --
    and share a `train_many` call freely with plain, rho, CAR and tree members.  state["residual_targets"][f] = [y_high -
    tensor_linear(y_low), |v_high - v_low| or None] at the V of the start of the last step, computed with torch: what train_CIGAR hands
    to add_data.  A link together with `ys[f]` or with `car[f]` raises ValueError.
    `car[f]` = (b, y_low, y_high) makes model f one of train_CAR's fidelities above 0 (CAR_ContinuousAutoRegression.py:116-142; `ys[f]`
    is then None): a `GP_basic` over a `kernel.FidelityKernelMCMC` whose `b` is that very tensor, trained on y_high - exp(b) * y_low
    under kernel1 * s(b, l_z, sigma_z); six groups of parameters move per step -- the base kernel's two, l_z, sigma_z, b and
    noise_variance (ffgp_train_car_raw: one launch for all steps up to 128 points, launch per stage above).  The Monte-Carlo samples are
    drawn once per call, after `torch.manual_seed(105)`, which leaves the global generator as one reference step leaves it.
    state["residual_targets"][f] = [y_high - exp(b) * y_low, None] at the b of the start of the last step.  A tree or
    RationalQuadraticKernel base kernel, an l_z of several elements or CPU tensors: the reference's loop, same return values.
    `car=` and `residual=` on one model raise ValueError.
    `wide_one_launch=True` (off by default: without it nothing changes) sends the WIDE-output models of the call -- a `cigp` over one
    library radial kernel (SE / ARD, Matern 1/2, 3/2, 5/2) on one GPU in fp64 with n <= 128, D <= 16 and d > 16 target columns, plain (y
    or [y, y_var]) or with a `residual=` link in either form -- through ffgp_train_wide_raw, up to 16 per call: ONE kernel launch for
    all their steps (csrc/train_wide.hip).  Their targets are compressed once per call by `compress_targets` -- Y to at most n columns,
    a residual member's [y_high; y_low] to at most 2 n -- and the likelihood keeps the true d, so a step's cost does not depend on d.
    Without the keyword these models run ffgp_train_raw's launch-per-stage form, 13 dependent launches per step at n = 128.  Every other
    model of the call keeps its route.  Return values, in-place updates, state["residual_targets"], the failure rule (a not-PD Sigma
    stops that model alone; LinAlgError) and the version counters are the one-launch route's; the Adam state of such a model is kept
    per model under the key the launch-per-stage route uses, so a `state` may be continued with either value of the keyword (the
    routes agree to rounding).  state["wide_one_launch"] lists the models that took the route in the last call, state["wide_status"]
    their status words (0, or the failing pivot) and state["wide_trace"] their rows of the trace (NaN from a failing step on), which a
    raising call does not return.  Without a GPU the keyword raises FFGPError: there is no other way to run this route."""
    models, xs, ys = list(models), list(xs), list(ys)
    nF = len(models)
    if wide_one_launch and not torch.cuda.is_available():
        raise _lib.FFGPError("train_many(wide_one_launch=True) needs an MI355X (gfx950) GPU: ffgp_train_wide_raw has no CPU path")
    if not (nF == len(xs) == len(ys)) or steps <= 0:
        raise ValueError("train_many: models, xs, ys must have one length and steps must be positive")
    if residual is not None:
        residual = list(residual)
        if len(residual) != nF:
            raise ValueError("train_many: residual must have one entry per model")
        for f, res in enumerate(residual):
            if res is not None and (ys[f] is not None or len(res) != 3):
                raise ValueError("train_many: a residual model takes (rho or a Tensor_linear, y_low, y_high) and ys[f] = None")
            if res is None and ys[f] is None and (car is None or car[f] is None):
                raise ValueError("train_many: model %d has neither targets nor a residual link" % f)
    if car is not None:
        car = list(car)
        if len(car) != nF:
            raise ValueError("train_many: car must have one entry per model")
        for f, cr in enumerate(car):
            if cr is None:
                continue
            if residual is not None and residual[f] is not None:
                raise ValueError("train_many: model %d has both a car and a residual link" % f)
            if ys[f] is not None or len(cr) != 3:
                raise ValueError("train_many: a CAR model takes (b, y_low, y_high) and ys[f] = None")
            if not hasattr(models[f].kernel, "car_links") or models[f].kernel.b is not cr[0]:
                raise ValueError("train_many: a CAR model's kernel is a FidelityKernelMCMC whose b is the tensor given in car=")
    car_of = (lambda f: car[f]) if car is not None else (lambda f: None)
    res_of = (lambda f: residual[f]) if residual is not None else (lambda f: None)
    # a residual model's eligibility is judged on its y_high (same shape as its targets) and its link
    ys_e = [ys[f] if res_of(f) is None else _split_residual(res_of(f))[2] for f in range(nF)]
    elig = [_eligible(m, x, y, fuse_composed) if car_of(f) is None else _eligible_car(m, x, car_of(f)) for f, (m, x, y) in enumerate(zip(models, xs, ys_e))]
    tlin = {f for f in range(nF) if _is_tlin(res_of(f))}
    for f in range(nF):
        if f in tlin:      # (a Tensor_linear link: ffgp_train_tlin_raw, or the reference's loop)
            if elig[f] is not None and not _tlin_ok(res_of(f), xs[f], elig[f]):
                elig[f] = None
            continue
        if res_of(f) is not None and elig[f] is not None and ((_is_tree(elig[f]) and not fuse_composed) or not _residual_ok(res_of(f), xs[f])):
            elig[f] = None      # (a composed kernel with a residual link: the reference's loop unless `fuse_composed` -- ffgp_train_tree_res_raw)
        if res_of(f) is not None and _is_tree(elig[f]) and "diag" in elig[f][0] and _split_residual(res_of(f))[3] is not None:
            elig[f] = None      # (a `GP_basic` over a tree: it adds the FULL residual variance matrix to Sigma -- the reference's loop)
    fused = all(e is not None for e in elig) and len({x.device for x in xs}) == 1
    if state is None:
        state = {"fused": fused, "chunks": {}, "opts": [None] * nF}
    state["residual_targets"] = [None] * nF
    state["tree_one_launch"] = []
    if wide_one_launch or "wide_one_launch" in state:      # (a state that has been on the route: nothing of it took it in THIS call yet)
        state["wide_one_launch"], state["wide_status"], state["wide_trace"] = [], {}, {}
    if not fused or not state["fused"]:
        if state["fused"]:
            raise ValueError("train_many: this state belongs to fused training; the models no longer qualify for it")
        trace = _reference_loop(models, xs, ys, steps, lr, betas, eps, state["opts"], residual, state["residual_targets"], car)
        return trace, state
    JITTER, PI = _jitter_and_pi()
    from . import functional as F
    from .blocks import threaded_blocks
    dev = xs[0].device
    trace = torch.empty((nF, steps), dtype=torch.float64, device=dev)
    opt = _lib.Adam(float(lr), float(betas[0]), float(betas[1]), float(eps))
    rho_last = {f: torch.empty_like(res_of(f)[0].detach()) for f in range(nF) if res_of(f) is not None and f not in tlin}
    # a Tensor_linear member's matrix, V at the start of the last step (row-major) and its constant diagonal extra |diag(v_high) - diag(v_low)|
    tl_V = {f: res_of(f)[0].vectors[0] for f in tlin}
    V_last = {f: torch.empty(tuple(tl_V[f].shape), dtype=torch.float64, device=dev) for f in tlin}
    tl_dvec = {}
    for f in tlin:
        _, _, _, vl, vh = _split_residual(res_of(f))
        if vl is not None:
            with torch.no_grad():
                tl_dvec[f] = (vh.diagonal() - vl.diagonal()).abs().contiguous()
    b_last = {f: torch.empty_like(car_of(f)[0].detach()) for f in range(nF) if car_of(f) is not None}
    zdev = {}      # the CAR members' samples on the device (alive until the calls have returned)

    def describe(f):
        lk, y, y_var = elig[f]
        x, m = xs[f], models[f]
        n, D = x.shape
        p = Problem()
        p.n, p.D, p.d = n, D, y.shape[1]
        p.X_dev, p.Y_dev, p.w_dev, p.amp_dev = x.data_ptr(), y.data_ptr(), lk["w"].data_ptr(), lk["amp"].data_ptr()
        dpar, dlink, dc = lk["diag"] if "diag" in lk else (m.log_beta, _lib.LINK_EXP_NEG, JITTER)
        p.diag_add_dev = dpar.data_ptr()
        p.clamp_min = lk["clamp"]
        if y_var is not None:
            p.diag_stride = y_var.shape[1] + 1 if y_var.dim() == 2 else 1
            p.diag_vec_dev = y_var.data_ptr()
        p.ll_variant, p.pi_const = lk["ll"] if "ll" in lk else (FFGP_LL_V1, PI)
        kp = lk.get("kparam")
        p.kfun, p.kparam = lk["kfun"], (1.0 if kp is None else float(kp))
        ll = _lib.Links()
        ll.w_link, ll.w_c, ll.w_broadcast = lk["w_link"], lk["w_c"], 1 if lk["w"].numel() == 1 and D > 1 else 0
        ll.amp_link, ll.amp_c = lk["amp_link"], 0.0
        ll.dadd_link, ll.dadd_c = dlink, dc
        ll.out_scale = 1.0          # the value is the loss the reference minimises: -negative_log_likelihood = +nll
        rs, tk = _lib.Residual(), _lib.TlinLink()
        if f in tlin:
            _, yl, yh, _, _ = _split_residual(res_of(f))
            V = tl_V[f]
            p.Y_dev, p.diag_vec_dev, p.diag_stride = None, None, 0
            if f in tl_dvec:
                p.diag_vec_dev, p.diag_stride = tl_dvec[f].data_ptr(), 1
            tk.V_dev, tk.V_row_stride, tk.V_col_stride, tk.l = V.data_ptr(), V.stride(0), V.stride(1), V.shape[1]
            tk.y_low_dev, tk.y_high_dev, tk.V_last_dev = yl.data_ptr(), yh.data_ptr(), V_last[f].data_ptr()
        elif res_of(f) is not None:
            rho, yl, yh, vl, vh = _split_residual(res_of(f))
            p.diag_vec_dev, p.diag_stride = None, 0
            rs.rho_dev, rs.y_low_dev, rs.y_high_dev = rho.data_ptr(), yl.data_ptr(), yh.data_ptr()
            if vl is not None:
                rs.v_low_dev, rs.v_low_stride = vl.data_ptr(), vl.stride(0) + vl.stride(1)
                rs.v_high_dev, rs.v_high_stride = vh.data_ptr(), vh.stride(0) + vh.stride(1)
            rs.rho_last_dev = rho_last[f].data_ptr()
        cl = _lib.CarLink()
        if car_of(f) is not None:
            c, (b, yl, yh) = lk["car"], car_of(f)
            z1, z2 = zdev[f] = (c["z1"].to(dev).contiguous(), c["z2"].to(dev).contiguous())
            cl.b_dev, cl.zls_dev, cl.zamp_dev, cl.zeps = b.data_ptr(), c["l_z"].data_ptr(), c["sigma_z"].data_ptr(), c["eps"]
            if z1.dtype == torch.float64:      # (drawn under torch.set_default_dtype(float64): other numbers, all of the scalar in fp64)
                cl.z1d_dev, cl.z2d_dev = z1.data_ptr(), z2.data_ptr()
            else:
                zdev[f] = z1, z2 = z1.float(), z2.float()
                cl.z1_dev, cl.z2_dev = z1.data_ptr(), z2.data_ptr()
            cl.nz, cl.lf, cl.hf = z1.numel(), c["lf"], c["hf"]
            cl.y_low_dev, cl.y_high_dev, cl.b_last_dev = yl.data_ptr(), yh.data_ptr(), b_last[f].data_ptr()
        if f in tlin:
            return p, ll, rs, cl, tk, lk["w"].numel() + tl_V[f].numel()
        return p, ll, rs, cl, tk, lk["w"].numel() + (1 if res_of(f) is not None else 0) + (3 if car_of(f) is not None else 0)

    def describe_tree(f, keep):
        """model f with a composed kernel: its problem (the tree's leaves on their RAW parameters) and ffgp_tree_links; P = its number
        of raw parameters.  The ctypes arrays the problem points to are appended to `keep`."""
        (tl, y, y_var), x, m = elig[f], xs[f], models[f]
        _, form, lks = tl["tree"]
        n, D = x.shape
        shape, ops = form
        p = Problem()
        p.n, p.D, p.d = n, D, y.shape[1]
        dpar, dlink, dc = tl["diag"] if "diag" in tl else (m.log_beta, _lib.LINK_EXP_NEG, JITTER)
        p.X_dev, p.Y_dev, p.diag_add_dev = x.data_ptr(), y.data_ptr(), dpar.data_ptr()
        if y_var is not None:
            p.diag_stride = y_var.shape[1] + 1 if y_var.dim() == 2 else 1
            p.diag_vec_dev = y_var.data_ptr()
        p.ll_variant, p.pi_const = tl["ll"] if "ll" in tl else (FFGP_LL_V1, PI)
        rs = _lib.Residual()
        if res_of(f) is not None:      # (only under `fuse_composed`: ffgp_train_tree_res_raw)
            rho, yl, yh, vl, vh = _split_residual(res_of(f))
            p.Y_dev, p.diag_vec_dev, p.diag_stride = None, None, 0
            rs.rho_dev, rs.y_low_dev, rs.y_high_dev = rho.data_ptr(), yl.data_ptr(), yh.data_ptr()
            if vl is not None:
                rs.v_low_dev, rs.v_low_stride = vl.data_ptr(), vl.stride(0) + vl.stride(1)
                rs.v_high_dev, rs.v_high_stride = vh.data_ptr(), vh.stride(0) + vh.stride(1)
            rs.rho_last_dev = rho_last[f].data_ptr()
        arr = (_lib.KDesc * len(lks))()
        tree, tk = _lib.KTree(), _lib.TreeLinks()
        P = 1 + (1 if res_of(f) is not None else 0)
        for e, lk in enumerate(lks):
            arr[e].kfun, arr[e].clamp_min, arr[e].kparam = lk["kfun"], lk["clamp"], float(lk.get("kparam", 1.0))
            arr[e].w_dev, arr[e].amp_dev = lk["w"].data_ptr(), lk["amp"].data_ptr()
            le = tk.leaf[e]
            le.w_link, le.w_c, le.w_broadcast = lk["w_link"], lk["w_c"], 1 if lk["w"].numel() == 1 and D > 1 else 0
            le.amp_link, le.amp_c = lk["amp_link"], 0.0
            if lk.get("center") is not None:
                arr[e].center_dev, le.center_train = lk["center"].data_ptr(), 1
            P += lk["w"].numel() + 1 + (D if lk.get("center") is not None else 0)
        tree.n_leaves, tree.shape, tree.leaf = len(lks), shape, arr
        for i, o in enumerate(ops):
            tree.op[i] = o
        p.tree = C.pointer(tree)
        tk.dadd_link, tk.dadd_c, tk.out_scale = dlink, dc, 1.0
        keep += [arr, tree]
        return p, tk, rs, P

    def run_tree(idx):
        """one ffgp_train_tree_raw call -- ffgp_train_tree_lds_raw for a chunk of `one_launch`, ffgp_train_tree_res_raw for a chunk with
        residual members -- for the composed-kernel models `idx` (<= 16); Adam state [exp_avg (P) | exp_avg_sq (P)] per model, rho
        the (P + 1)-th parameter of a residual one"""
        anyres = any(res_of(f) is not None for f in idx)
        anyv2 = any("ll" in elig[f][0] for f in idx)
        if idx[0] in one_launch:      # (a chunk without a residual or V2 member keeps ffgp_train_tree_lds_raw: bit for bit the call it was)
            name = "ffgp_train_tree_lds_res_raw" if anyres or anyv2 else "ffgp_train_tree_lds_raw"
        else:
            name = "ffgp_train_tree_res_raw" if anyres else "ffgp_train_tree_raw"
        fn = getattr(lib, name)
        h = _lib.handle(dev.index)
        _lib.bind_stream(h, dev.index)
        P = (Problem * len(idx))()
        L = (_lib.TreeLinks * len(idx))()
        R = (_lib.Residual * len(idx))()
        keep, npar = [], []
        for j, f in enumerate(idx):
            P[j], L[j], R[j], n_ = describe_tree(f, keep)
            npar.append(n_)
        if name.endswith("res_raw"):
            return launch(idx, 2 * max(npar), lambda st, tr: check(
                fn(h, len(idx), P, L, R, int(steps), C.byref(opt), st.buf.data_ptr(), st.stride, int(st.step), tr.data_ptr(), tr.stride(0)), name))
        return launch(idx, 2 * max(npar), lambda st, tr: check(
            fn(h, len(idx), P, L, int(steps), C.byref(opt), st.buf.data_ptr(), st.stride, int(st.step), tr.data_ptr(), tr.stride(0)), name))

    def run_wide(idx, step0):
        """one ffgp_train_wide_raw call for the wide models `idx` (<= 16, all at Adam step `step0`): targets compressed, the true d
        apart.  Every model keeps an Adam state of its own under the key (f,) -- the launch-per-stage route's, which trains such a
        model in a call of its own."""
        h = _lib.handle(dev.index)
        _lib.bind_stream(h, dev.index)
        nm = len(idx)
        P = (Problem * nm)()
        L = (_lib.Links * nm)()
        R = (_lib.Residual * nm)()
        DT = (C.c_int * nm)()
        INFO = (C.c_int * nm)()
        keep, strides = [], []
        for j, f in enumerate(idx):
            P[j], L[j], R[j], _, _, nw = describe(f)
            DT[j] = P[j].d
            if res_of(f) is not None:
                _, yl, yh, _, _ = _split_residual(res_of(f))
                yhc, ylc = compress_targets(yh, yl)
                R[j].y_high_dev, R[j].y_low_dev, P[j].d = yhc.data_ptr(), ylc.data_ptr(), yhc.shape[1]
                keep += [yhc, ylc]
            else:
                yc, = compress_targets(elig[f][1])
                P[j].Y_dev, P[j].d = yc.data_ptr(), yc.shape[1]
                keep.append(yc)
            strides.append(2 * (nw + 2))
        # the models' states ([1, stride] each, the only copy kept between calls) are staged through a block of the call's: one short
        # copy per model in, one out
        smax = max(strides)
        blk = torch.zeros((nm, smax), dtype=torch.float64, device=dev)
        sts = []
        for j, f in enumerate(idx):
            st = state["chunks"].get((f,))
            if st is None or st.stride != strides[j] or st.buf.device != dev:
                st = state["chunks"][(f,)] = AdamState(torch.zeros((1, strides[j]), dtype=torch.float64, device=dev), strides[j], step0)
            blk[j, :strides[j]].copy_(st.buf[0])
            sts.append(st)
        tr = torch.empty((nm, steps), dtype=torch.float64, device=dev)
        rc = check(lib.ffgp_train_wide_raw(h, nm, P, L, R, DT, int(steps), C.byref(opt), blk.data_ptr(), smax, int(step0),
                                           tr.data_ptr(), tr.stride(0), INFO), "ffgp_train_wide_raw")
        for j, st in enumerate(sts):
            st.buf[0].copy_(blk[j, :strides[j]])
        if rc == 0:      # (a call that failed leaves its optimisers where they were: the caller sees LinAlgError)
            for st in sts:
                st.step += steps
        trace[list(idx)] = tr
        for j, f in enumerate(idx):
            state["wide_status"][f] = int(INFO[j])
            state["wide_trace"][f] = tr[j]
        del keep
        return rc

    def launch(idx, stride, call):
        """the chunk's Adam state and trace rows around one library call `call(state, trace rows)`; returns the status"""
        key = tuple(idx)
        st = state["chunks"].get(key)
        if st is None or st.stride != stride or st.buf.device != dev:
            st = AdamState(torch.zeros((len(idx), stride), dtype=torch.float64, device=dev), stride)
            state["chunks"][key] = st
        # the chunk's rows of the trace: contiguous when the models are consecutive, else through a staging block
        contiguous = list(idx) == list(range(idx[0], idx[0] + len(idx)))
        tr = trace[idx[0]:idx[0] + len(idx)] if contiguous else torch.empty((len(idx), steps), dtype=torch.float64, device=dev)
        rc = call(st, tr)
        if rc == 0:      # (a call that failed leaves its optimisers where they were: the caller sees LinAlgError)
            st.step += steps
        if not contiguous:
            trace[list(idx)] = tr
        return rc

    def run(idx):
        """one ffgp_train_raw call for the models `idx` (<= 16) on the calling thread's handle and stream; returns the status"""
        if _is_tree(elig[idx[0]]):
            return run_tree(idx)
        h = _lib.handle(dev.index)
        _lib.bind_stream(h, dev.index)
        P = (Problem * len(idx))()
        L = (_lib.Links * len(idx))()
        R = (_lib.Residual * len(idx))()
        Cl = (_lib.CarLink * len(idx))()
        Tl = (_lib.TlinLink * len(idx))()
        nws = []
        for j, f in enumerate(idx):
            P[j], L[j], R[j], Cl[j], Tl[j], nw = describe(f)
            nws.append(nw)
        anyres = any(res_of(f) is not None for f in idx)
        stride = 2 * (max(nws) + 2)
        if idx[0] in tlin:      # (chunks of their own: `groups` below; Adam state [exp_avg (P) | exp_avg_sq (P)], P = nw + 2 + h l, V row-major last)
            return launch(idx, stride, lambda st, tr: check(
                lib.ffgp_train_tlin_raw(h, len(idx), P, L, Tl, int(steps), C.byref(opt), st.buf.data_ptr(), stride, int(st.step),
                                        tr.data_ptr(), tr.stride(0)), "ffgp_train_tlin_raw"))
        if any(car_of(f) is not None for f in idx):      # (never in one chunk with residual members: `groups` below)
            return launch(idx, stride, lambda st, tr: check(
                lib.ffgp_train_car_raw(h, len(idx), P, L, Cl, int(steps), C.byref(opt), st.buf.data_ptr(), stride, int(st.step),
                                       tr.data_ptr(), tr.stride(0)), "ffgp_train_car_raw"))
        if anyres:
            return launch(idx, stride, lambda st, tr: check(
                lib.ffgp_train_residual_raw(h, len(idx), P, L, R, int(steps), C.byref(opt), st.buf.data_ptr(), stride, int(st.step),
                                            tr.data_ptr(), tr.stride(0)), "ffgp_train_residual_raw"))
        return launch(idx, stride, lambda st, tr: check(
            lib.ffgp_train_raw(h, len(idx), P, L, int(steps), C.byref(opt), st.buf.data_ptr(), stride, int(st.step), tr.data_ptr(),
                               tr.stride(0)), "ffgp_train_raw"))

    # small models (one workgroup each: ONE launch per step for up to 16 of them) go together; every larger model is a call of its
    # own -- and, when there are several, they train SIDE BY SIDE from host threads with a handle and a stream each
    # (blocks.threaded_blocks: the calls only enqueue and wait once, ctypes drops the GIL inside them), so that one model's
    # latency-bound chain of small kernels runs in the gaps of the others'
    # Models with a composed kernel (ffgp_train_tree_raw) form calls of their own: up to 16 of at most 128 points per call, the larger
    # ones one call each beside the other large models.
    shapes = [(xs[f].shape[0], xs[f].shape[1], elig[f][1].shape[1]) for f in range(nF)]
    trees = {f for f in range(nF) if _is_tree(elig[f])}
    small = [f for f in range(nF) if f not in trees and shapes[f][0] <= F.SMALL_BATCH_MAX_N and shapes[f][1] <= F.SMALL_BATCH_MAX_D
             and shapes[f][2] <= F.SMALL_BATCH_MAX_d]
    # ... and under `tree_one_launch` those the LDS trainer covers form calls of ffgp_train_tree_lds_raw, up to 16 per call.
    # (residual and V2 members among them: ffgp_train_tree_lds_res_raw, plain and residual members sharing chunks)
    one_launch = {f for f in trees if tree_one_launch and shapes[f][0] <= TREE_ONE_LAUNCH_MAX_N and shapes[f][1] <= F.SMALL_BATCH_MAX_D
                  and shapes[f][2] <= F.SMALL_BATCH_MAX_d}
    lds_trees = sorted(one_launch)
    small_trees = [f for f in sorted(trees) if shapes[f][0] <= F.SMALL_BATCH_MAX_N and f not in one_launch]
    large = [f for f in range(nF) if f not in set(small) and f not in set(small_trees) and f not in one_launch]      # (set(small): CAR ones too)
    state["tree_one_launch"] = lds_trees
    # ... and under `wide_one_launch` the wide-output models ffgp_train_wide_raw covers leave `large` for calls of up to 16, models
    # at one Adam step sharing a call (ffgp_train_wide_raw takes one step0)
    wide = []
    if wide_one_launch:
        wide = [f for f in large if f not in trees and f not in tlin and car_of(f) is None and shapes[f][0] <= F.SMALL_BATCH_MAX_N
                and shapes[f][1] <= F.SMALL_BATCH_MAX_D and shapes[f][2] > F.SMALL_BATCH_MAX_d and "ll" not in elig[f][0]
                and "diag" not in elig[f][0] and elig[f][0]["kfun"] <= WIDE_KFUN_MAX]
        large = [f for f in large if f not in set(wide)]
        state["wide_one_launch"] = wide
    # (CAR members have an entry point of their own: their small ones form chunks apart from the plain and residual models')
    small_car = [f for f in small if car_of(f) is not None]
    # ... and so have Tensor_linear members: the small ones (n <= 128, D, h <= 16) up to 16 per call, every larger one a call of its own
    small_tlin = [f for f in small if f in tlin]
    small = [f for f in small if car_of(f) is None and f not in tlin]
    if len(small) == 1:      # (a lone small model gains nothing from the batch kernel: its own call folds the tail launches)
        large, small = sorted(large + small), []
    if len(small_car) == 1:
        large, small_car = sorted(large + small_car), []
    if len(small_tlin) == 1:
        large, small_tlin = sorted(large + small_tlin), []
    rcs = []
    for group in (small, small_car, small_tlin, small_trees, lds_trees):
        for c0 in range(0, len(group), TRAIN_MAX_MODELS):
            rcs.append((group[c0:c0 + TRAIN_MAX_MODELS], run(group[c0:c0 + TRAIN_MAX_MODELS])))
    by_step = {}
    for f in wide:
        st = state["chunks"].get((f,))
        by_step.setdefault(st.step if st is not None else 0, []).append(f)
    for step0, group in sorted(by_step.items()):
        for c0 in range(0, len(group), TRAIN_MAX_MODELS):
            rcs.append((group[c0:c0 + TRAIN_MAX_MODELS], run_wide(group[c0:c0 + TRAIN_MAX_MODELS], step0)))
    if len(large) >= 2 and _lib.current_slot() == 0:
        outs = threaded_blocks([(lambda f=f: run([f])) for f in large], nslots=min(TRAIN_THREADS, len(large)), device_index=dev.index)
        rcs += [([f], rc) for f, rc in zip(large, outs)]
    else:
        rcs += [([f], run([f])) for f in large]
    # the library wrote the parameters behind autograd's back: bump their version counters (cached posteriors key on them)
    bump = getattr(torch.autograd.graph, "increment_version", None)      # (torch >= 2.1: no kernel; else an in-place no-op add)
    with torch.no_grad():
        for f, m in enumerate(models):
            for q in list(m.parameters()) + ([] if res_of(f) is None else ([tl_V[f]] if f in tlin else [res_of(f)[0]])):
                if bump is not None:
                    bump(q)
                else:
                    q.add_(0.0)
    for idx, rc in rcs:
        if rc > 0:
            _raise_not_pd(rc, "linalg.cholesky (train_many, model%s %s)" % ("s" if len(idx) > 1 else "", ", ".join(map(str, idx))))
    for f, rl in rho_last.items():      # train_AR's data for the fidelity: the residual at the rho of the start of the last step
        state["residual_targets"][f] = _residual_targets(res_of(f), rl.reshape(res_of(f)[0].shape))
    for f, vl_ in V_last.items():       # train_CIGAR's data for the fidelity: the residual at the V of the start of the last step
        state["residual_targets"][f] = _tlin_targets(res_of(f), vl_)
    for f, bl in b_last.items():        # train_CAR's data for the fidelity: the residual at the b of the start of the last step
        state["residual_targets"][f] = _car_targets(car_of(f), bl.reshape(car_of(f)[0].shape))
    return trace, state
