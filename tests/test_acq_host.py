"""CPU: the torch-level half of the acquisition module (fidelityfusion_amd/acq.py) -- `UCB` / `EI` on arbitrary callables against the
reference's formulas (Bayesian_optimization/acq.py:132-144,161-181) and `optimize_acqf`'s generic loop with the reference's selection
rule (acq.py:48-68) against the same loop written out here.  No GPU: nothing below creates a library handle."""
import math
import os
import re

import pytest

torch = pytest.importorskip("torch")


def mean_func(X):
    return torch.sin(3.0 * X).sum(1, keepdim=True) + 0.3 * X[:, :1]


def variance_func(X):
    return 0.6 + 0.4 * torch.cos(2.0 * X).prod(1, keepdim=True)


@pytest.fixture()
def X0():
    return 2.0 * torch.rand(17, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(3))


def test_binding_declares_the_entry_point_and_its_limits():
    from fidelityfusion_amd import _lib
    assert "ffgp_acq_optimize" in _lib.EXPORTS and _lib.lib.ffgp_acq_optimize is not None
    assert (_lib.FFGP_ACQ_UCB, _lib.FFGP_ACQ_EI) == (0, 1)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ffgp.h")).read()
    for name in ("FFGP_ACQ_MAX_N", "FFGP_ACQ_MAX_D", "FFGP_ACQ_MAX_STEPS"):
        assert re.search(r"#define %s %d\b" % (name, getattr(_lib, name)), hdr), name


def test_ucb_forward_matches_the_formula(X0):
    from fidelityfusion_amd import acq
    got = acq.UCB(mean_func, variance_func, kappa=1.7).forward(X0)
    want = mean_func(X0) + 1.7 * torch.sqrt(variance_func(X0))
    assert got.shape == (17, 1) and float((got - want).abs().max()) <= 1e-15


def test_ei_forward_matches_the_formula(X0):
    from fidelityfusion_amd import acq
    got = acq.EI(mean_func, variance_func, xi=0.02).forward(X0, 0.4)
    m, s = mean_func(X0), torch.sqrt(variance_func(X0))
    for i in range(X0.shape[0]):
        u = float(m[i]) - 0.4 - 0.02
        sd = max(float(s[i]), 1e-9)
        Z = u / sd
        want = u * 0.5 * math.erfc(-Z / math.sqrt(2.0)) + sd * math.exp(-0.5 * Z * Z) / math.sqrt(2.0 * math.pi)
        assert abs(float(got[i]) - want) <= 1e-15 * max(1.0, abs(want)), (i, float(got[i]), want)


def test_ei_gradient_treats_cdf_and_pdf_as_constants(X0):
    """d ei / d mean = Phi(Z), d ei / d std = phi(Z): what the reference's scipy constants leave, and the exact derivative"""
    from fidelityfusion_amd import acq
    mu = torch.tensor([[0.2], [0.9]], dtype=torch.float64, requires_grad=True)
    var = torch.tensor([[0.5], [0.1]], dtype=torch.float64, requires_grad=True)
    acq.EI(lambda X: mu, lambda X: var, xi=0.01).forward(None, 0.4).sum().backward()
    for i in range(2):
        sd = math.sqrt(float(var[i].detach()))
        Z = (float(mu[i].detach()) - 0.41) / sd
        assert abs(float(mu.grad[i]) - 0.5 * math.erfc(-Z / math.sqrt(2.0))) <= 1e-15
        assert abs(float(var.grad[i]) - math.exp(-0.5 * Z * Z) / math.sqrt(2.0 * math.pi) / (2.0 * sd)) <= 1e-15


def reference_loop(obj, X0, steps, lr):
    """acq.py:48-68 from given start points: Adam on -acq(X).sum(), best_x = X after the last step whose loss beat the best so far"""
    X = X0.clone().requires_grad_(True)
    opt = torch.optim.Adam([X], lr=lr)
    best_x = X.clone().detach()
    best_value = float(obj(best_x))
    for _ in range(steps):
        opt.zero_grad()
        loss = obj(X)
        loss.backward()
        opt.step()
        if loss.item() < best_value:
            best_value = loss.item()
            best_x = X.clone().detach()
    return best_x, X.detach().clone()


@pytest.mark.parametrize("name", ["ucb", "ei"])
def test_generic_loop_selects_as_the_reference_does(X0, name):
    from fidelityfusion_amd import acq
    if name == "ucb":
        a = acq.UCB(mean_func, variance_func)
        obj = lambda X: -a.forward(X).sum()
    else:
        a = acq.EI(mean_func, variance_func)
        obj = lambda X: -a.forward(X, 0.4).sum()
    keep = X0.clone()
    want_best, want_final = reference_loop(obj, X0, 30, 0.1)
    best = acq.optimize_acqf(a, None, None, X0, steps=30, lr=0.1, f_best=0.4)
    assert torch.equal(X0, keep)
    assert torch.equal(best, want_best)
    assert not torch.equal(best, X0)      # some step did improve
    assert torch.equal(acq.optimize_acqf(a, None, None, X0, steps=30, lr=0.1, f_best=0.4, return_best_only=False), want_final)


def test_generic_loop_returns_x0_when_no_step_improves(X0):
    """the first step's loss is the loss at X0 itself, so a single step is never selected"""
    from fidelityfusion_amd import acq
    a = acq.UCB(mean_func, variance_func)
    best = acq.optimize_acqf(a, None, None, X0, steps=1, lr=0.1)
    assert torch.equal(best, X0) and best.data_ptr() != X0.data_ptr()
    assert not torch.equal(acq.optimize_acqf(a, None, None, X0, steps=1, lr=0.1, return_best_only=False), X0)


def test_select_best_rule():
    from fidelityfusion_amd import acq
    hist = torch.arange(5.0).reshape(5, 1, 1)
    # losses 3, 2, 2.5, 1 -> steps 1 and 3 improve; the result is X after step 3's update
    trace = -torch.tensor([[3.0], [2.0], [2.5], [1.0]])
    assert float(acq.select_best(hist[0], trace, hist)) == 4.0
    assert float(acq.select_best(hist[0], -torch.tensor([[1.0], [1.0], [2.0], [1.0]]), hist)) == 0.0
