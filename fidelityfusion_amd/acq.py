"""The acquisition optimiser of the Bayesian-optimisation drivers (reference: Bayesian_optimization/acq.py:10-181).

`UCB` and `EI` are the reference's classes on any `mean_func` / `variance_func` callables, as differentiable torch code.
`optimize_acqf` is its Adam loop with its selection rule (acq.py:48-68).  For a frozen `cigp` (or a `functional.Posterior`) the
whole loop is ONE kernel launch (`Posterior.optimize_acquisition`, csrc/acq.hip) whenever the posterior is a single radial library
kernel of the kernel's sizes; otherwise -- and for acquisition objects on arbitrary callables -- it runs step by step.  The start
points are the caller's: the reference draws them inside the function, in fp32.  PI, KG and PF are not provided: the reference gives
them no gradient or a random one.
`optimize_acqf_mf` is the same loop on the posterior of a multi-fidelity stack (AR, ResGP: a list of per-fidelity `cigp`), the
drivers' MF_BayesianOptimization/Discrete/DMF_acq.py:226-262 -- every fidelity level in one launch (`PosteriorStack`, csrc/acq_stack.hip);
with `fuse_composed=True` also when fidelities run on SumKernel / ProductKernel trees, the reference's own
SumKernel(LinearKernel, MaternKernel) of its two-fidelity AR and ResGP (csrc/acq_stack_tree.hip).
`optimize_acqf_nar` is that loop on NAR (FidelityFusion_Models/NAR.py:30-61), whose upper fidelities take the lower fidelity's predicted
mean as an input -- one launch as well (`PosteriorChain`, csrc/acq_chain.hip); with `fuse_composed=True` also when fidelities run on
SumKernel / ProductKernel trees, the reference's own SumKernel(LinearKernel, MaternKernel) of its two-fidelity NAR
(csrc/acq_chain_tree.hip; up to 256 points per fidelity).
Past the one-launch kernels' 256 training points, `staged=True` on `optimize_acqf` / `optimize_acqf_mf` keeps the loop on the device:
launch per stage, every step enqueued by one library call (csrc/acq_staged.hip), for radial-kernel models of up to 2048 points; with
`fuse_composed=True` as well, the same holds for SumKernel / ProductKernel models and stacks with such fidelities
(csrc/acq_staged_tree.hip) -- the reference's cigp and AR on SumKernel(LinearKernel, MaternKernel) once a run has passed 256 points.
`staged=True` on `optimize_acqf_nar` does the same for a NAR chain of radial-kernel models of up to 2048 points per fidelity
(csrc/acq_staged_chain.hip), and with `fuse_composed="staged"` for a chain whose fidelities run on SumKernel / ProductKernel trees
(csrc/acq_staged_chain_tree.hip)."""
import inspect
import math

import torch

from .posterior import Posterior, PosteriorChain, PosteriorStack


def _norm_cdf(z):
    return 0.5 * torch.erfc(-z / math.sqrt(2.0))


def _norm_pdf(z):
    return torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


class UCB:
    """mean + kappa * sqrt(variance)  (acq.py:118-144)"""

    def __init__(self, mean_func, variance_func, kappa=2.0):
        self.mean_func = mean_func
        self.variance_func = variance_func
        self.kappa = kappa

    def forward(self, X):
        return self.mean_func(X) + self.kappa * torch.sqrt(self.variance_func(X))


class EI:
    """(mean - f_best - xi) Phi(Z) + std phi(Z), Z = (mean - f_best - xi) / std, std clamped at 1e-9 (acq.py:147-181).  Phi and phi
    are taken on detached values, as the reference takes them from scipy -- which leaves d/dmean = Phi and d/dstd = phi, the exact
    derivative -- but stay in the dtype and on the device of the inputs."""

    def __init__(self, mean_func, variance_func, xi=0.01):
        self.mean_func = mean_func
        self.variance_func = variance_func
        self.xi = xi

    def forward(self, X, f_best):
        mean = self.mean_func(X)
        std = torch.clamp(torch.sqrt(self.variance_func(X)), min=1e-9)
        u = mean - f_best - self.xi
        Z = (u / std).detach()
        return u * _norm_cdf(Z) + std * _norm_pdf(Z)


def select_best(X0, trace, hist):
    """the reference's selection (acq.py:52-66): best = X0 with the loss at X0; after step k, if that step's loss (evaluated before
    its update: -trace[k].sum()) is below the best so far, best_x becomes X after that update (hist[k + 1])"""
    losses = (-trace.sum(1)).tolist()
    best_x, best_value = X0, losses[0]      # (the loss at X0 is step 0's own loss)
    for k, loss in enumerate(losses):
        if loss < best_value:
            best_value = loss
            best_x = hist[k + 1]
    return best_x.detach().clone()


def _generic_loop(acq, X0, f_best, steps, lr):
    """acq.py:48-62 on an acquisition object with forward(X) or forward(X, f_best): plain torch, wherever X0 lives"""
    two = len(inspect.signature(acq.forward).parameters) == 2
    X = X0.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([X], lr=lr)
    trace, hist = [], []
    for _ in range(steps):
        opt.zero_grad()
        a = acq.forward(X, f_best) if two else acq.forward(X)
        (-a.sum()).backward()
        hist.append(X.detach().clone())
        trace.append(a.detach().reshape(X.shape[0], -1).sum(1))
        opt.step()
    hist.append(X.detach().clone())
    return X.detach(), torch.stack(trace), torch.stack(hist)


def optimize_acqf(model, x_train=None, y_train=None, X0=None, steps=30, lr=0.1, acq="ucb", kappa=2.0, xi=0.01, f_best=0.0,
                  var_floor=1e-12, return_best_only=True, fuse_composed=False, staged=False):
    """The reference's `optimize_acqf` from the start points X0 [Q, D] (untouched): `steps` (its `num_restarts`) Adam iterations at
    `lr` on loss = -acq(X).sum(), then its selection rule (`select_best`); `return_best_only=False` returns the final points.
      * model = a `cigp`: the posterior of (x_train, y_train) the model caches, with the noise `cigp.forward` adds to the variance
        (1 / beta); model = a `functional.Posterior`: as it stands (no noise added).  acq = "ucb" (kappa, var_floor) or "ei" (f_best, xi);
        `fuse_composed=True` runs a composed kernel's loop (SumKernel / ProductKernel trees, the reference's own
        SumKernel(LinearKernel, MaternKernel)) in one launch as well (`Posterior.optimize_acquisition`, csrc/acq_tree.hip);
        `staged=True` runs a radial-kernel model of 257 ... 2048 points launch per stage inside one library call
        (csrc/acq_staged.hip) instead of the per-step loop; models of up to 256 points keep the one-launch call; both keywords
        together do the same for a composed-kernel model of 257 ... 2048 points (csrc/acq_staged_tree.hip);
      * model = an acquisition object (`UCB`, `EI`, anything with forward(X) or forward(X, f_best)): the step-by-step torch loop."""
    if X0 is None:
        raise ValueError("optimize_acqf needs the start points X0 [Q, D]")
    if isinstance(model, Posterior) or hasattr(model, "_cached_posterior"):
        if isinstance(model, Posterior):
            post, noise = model, 0.0
        else:
            y = y_train[0] if isinstance(y_train, list) else y_train
            post = model._cached_posterior(x_train, y)[0]
            noise = float(model.log_beta.detach().exp().pow(-1))
        X, trace, hist, _ = post.optimize_acquisition(X0, steps=steps, lr=lr, acq=acq, kappa=kappa, xi=xi, f_best=f_best,
                                                      var_add_all=noise, var_floor=var_floor, fuse_composed=fuse_composed, staged=staged)
    else:
        X, trace, hist = _generic_loop(model, X0, f_best, steps, lr)
    return select_best(X0, trace, hist) if return_best_only else X


def optimize_acqf_mf(models, data, X0, rho=None, level=None, steps=10, lr=0.001, acq="ucb", kappa=2.0, xi=0.01, f_best=0.0, var_floor=1e-12,
                     accumulate_grad=False, return_best_only=True, fuse_composed=False, staged=False):
    """The multi-fidelity drivers' acquisition optimiser (DMF_acq.py:226-262) on the posterior of AR / ResGP
    (FidelityFusion_Models/AR_autoRegression.py:56-89): `models` is the trainers' `gpr_list` (frozen `cigp`), data[f] = (x_f, y_f) the
    data model f was trained on (for f > 0 the residuals), rho = (rho_0, ...) AR's scale factors -- None: all ones, ResGP.  Member f
    is model f's cached posterior with that model's 1 / beta added to its variance, weighted by (1, rho_0, rho_1, ...) in the mean
    and by the squares in the variance.  `level` (int or [Q]) is each start point's `to_fidelity` (None: the top level), so the
    drivers' loop over the fidelities is ONE call; acq = "ucb", "ei" or "ucb_var" (mean + kappa var, the drivers' UCB_MF with
    kappa = 0.2 D); `accumulate_grad=True` omits zero_grad as the drivers' loop does.  `fuse_composed=True` runs the loop in one launch
    also when models carry composed kernels (`PosteriorStack.optimize_acquisition`, csrc/acq_stack_tree.hip); by default such a stack
    takes the per-step loop.  `staged=True` runs a stack of radial-kernel models with a fidelity of 257 ... 2048 points -- the
    reference's demo trains on 300 / 300 / 250 -- launch per stage inside one library call (csrc/acq_staged.hip) instead of the per-step
    loop; with `fuse_composed=True` as well, so does a stack whose models carry composed kernels (csrc/acq_staged_tree.hip), while
    `staged=True` alone leaves such a stack on the per-step loop.  Returns `select_best` on the trace, or the final points with `return_best_only=False`."""
    if X0 is None:
        raise ValueError("optimize_acqf_mf needs the start points X0 [Q, D]")
    models = list(models)
    if len(data) != len(models):
        raise ValueError("data holds one (x, y) pair per model")
    coefs = [1.0] + ([1.0] * (len(models) - 1) if rho is None else [float(r) for r in rho])
    if len(coefs) != len(models):
        raise ValueError("rho holds one factor per model above the first")
    members, noise = [], []
    for m, (x, y) in zip(models, data):
        y = y[0] if isinstance(y, list) else y
        members.append(m._cached_posterior(x, y)[0])
        noise.append(float(m.log_beta.detach().exp().pow(-1)))
    stack = PosteriorStack(members, coefs)
    X, trace, hist, _ = stack.optimize_acquisition(X0, steps=steps, lr=lr, acq=acq, kappa=kappa, xi=xi, f_best=f_best, var_floor=var_floor,
                                                   level=level, var_adds=noise, accumulate_grad=accumulate_grad, fuse_composed=fuse_composed,
                                                   staged=staged)
    return select_best(X0, trace, hist) if return_best_only else X


def optimize_acqf_nar(models, data, X0, level=None, steps=10, lr=0.001, acq="ucb", kappa=2.0, xi=0.01, f_best=0.0, var_floor=1e-12,
                      accumulate_grad=False, return_best_only=True, staged=False, fuse_composed=False):
    """The multi-fidelity drivers' acquisition optimiser (DMF_acq.py:226-262) on the posterior of NAR (FidelityFusion_Models/NAR.py:30-61):
    `models` is the NAR trainer's `gpr_list` (frozen `cigp`), data[0] = (x_0, y_0), data[f > 0] = the 'concat-f' set the trainer stored:
    inputs [x, y_low_mean] and y, possibly as the list [y, y_var] (`cigp.forward` ignores y_var; y[0] is used, as `optimize_acqf_mf`
    does).  Member f is model f's cached posterior with that model's 1 / beta added to its variance; member f > 0 is queried at
    [x, mean of member f - 1] and the model reports the mean and variance of the member a point stops at.  `level` (int or [Q]) is each
    start point's `to_fidelity` (None: the top level), so the drivers' loop over the fidelities is ONE call; acq, `accumulate_grad` and
    the return value as in `optimize_acqf_mf`.  `staged=True` runs a chain of radial-kernel models with a fidelity of 257 ... 2048
    points -- NAR's demo trains on 300 / 300 / 250 -- launch per stage inside one library call (`PosteriorChain.optimize_acquisition`,
    csrc/acq_staged_chain.hip) instead of the per-step loop; a chain of up to 256 points per fidelity keeps the one-launch call.
    `fuse_composed=True` runs the loop in one launch also when models carry composed kernels (SumKernel / ProductKernel trees of 2-4
    library kernels, LinearKernel included; csrc/acq_chain_tree.hip) and every fidelity has at most 256 points; by default such a chain
    takes the per-step loop, and with `fuse_composed=True` it keeps that loop past 256 points.  `fuse_composed="staged"` means what
    True means and, together with `staged=True`, runs a chain with composed-kernel fidelities of 257 ... 2048 points -- the
    reference's NAR on SumKernel(LinearKernel, MaternKernel) at its demo's 300 / 300 / 250 -- launch per stage inside one library call
    as well (csrc/acq_staged_chain_tree.hip); the value is passed through to `PosteriorChain.optimize_acquisition`."""
    if X0 is None:
        raise ValueError("optimize_acqf_nar needs the start points X0 [Q, D]")
    models = list(models)
    if len(data) != len(models):
        raise ValueError("data holds one (x, y) pair per model")
    members, noise = [], []
    for m, (x, y) in zip(models, data):
        y = y[0] if isinstance(y, list) else y
        members.append(m._cached_posterior(x, y)[0])
        noise.append(float(m.log_beta.detach().exp().pow(-1)))
    chain = PosteriorChain(members)
    X, trace, hist, _ = chain.optimize_acquisition(X0, steps=steps, lr=lr, acq=acq, kappa=kappa, xi=xi, f_best=f_best, var_floor=var_floor,
                                                   level=level, var_adds=noise, accumulate_grad=accumulate_grad, staged=staged,
                                                   fuse_composed=fuse_composed)
    return select_best(X0, trace, hist) if return_best_only else X
