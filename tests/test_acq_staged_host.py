"""The launch-per-stage acquisition call's host side, without a GPU: the export, the ctypes declaration, the cap in the header against
the Python constant, the `staged` keyword of the four Python entry points, and the `acq_staged_ok` predicate."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ffgp_acq_optimize_stack_staged"


def test_the_library_exports_the_entry():
    so = os.path.join(ROOT, "fidelityfusion_amd", "libffgp.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT %s\b" % NAME, out), "libffgp.so does not export %s" % NAME


def test_lib_declares_the_function():
    from fidelityfusion_amd import _lib
    fn = getattr(_lib.lib, NAME)
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == list(_lib.lib.ffgp_acq_optimize_stack.argtypes)      # the stack entry's arguments, one for one


def test_the_cap_in_the_header_is_the_python_constant():
    from fidelityfusion_amd import _lib
    src = open(os.path.join(ROOT, "include", "ffgp.h")).read()
    m = re.search(r"^#define FFGP_ACQ_STAGED_MAX_N (\d+)\b", src, flags=re.M)
    assert m and int(m.group(1)) == _lib.FFGP_ACQ_STAGED_MAX_N
    assert _lib.FFGP_ACQ_STAGED_MAX_N >= 2048
    assert re.search(r"^#define FFGP_ACQ_MAX_N 256\b", src, flags=re.M) and _lib.FFGP_ACQ_MAX_N == 256      # the one-launch limit stays


def test_the_four_entry_points_accept_staged():
    from fidelityfusion_amd import acq
    from fidelityfusion_amd.posterior import Posterior, PosteriorStack
    for fn in (Posterior.optimize_acquisition, PosteriorStack.optimize_acquisition, acq.optimize_acqf, acq.optimize_acqf_mf):
        p = inspect.signature(fn).parameters
        assert "staged" in p and p["staged"].default is False, fn


class _OnGpu(torch.Tensor):
    """a CPU tensor that reports itself on cuda:0: the predicate reads is_cuda, device, dtype and shape, and never the data"""
    is_cuda = property(lambda self: True)
    device = property(lambda self: torch.device("cuda:0"))


def _posterior(n=300, D=2, d=1, kfun=0, tree=None):
    from fidelityfusion_amd.posterior import Posterior
    p = object.__new__(Posterior)      # the predicate's fields alone: nothing is factored
    p.dev, p.n, p.D, p.d, p.kfun, p.tree = torch.device("cuda:0"), n, D, d, (kfun, 1.0), tree
    return p


def _starts(Q=5, D=2, dtype=torch.float64):
    return torch.zeros(Q, D, dtype=dtype).as_subclass(_OnGpu)


def test_acq_staged_ok():
    from fidelityfusion_amd import _lib
    from fidelityfusion_amd.posterior import PosteriorStack
    cap = _lib.FFGP_ACQ_STAGED_MAX_N
    X0 = _starts()
    assert _posterior().acq_staged_ok(X0) and not _posterior().acq_fusable(X0)      # n = 300: past the one-launch limit, within the cap
    assert _posterior(n=cap).acq_staged_ok(X0)
    assert _posterior(n=40).acq_staged_ok(X0) and _posterior(n=40).acq_fusable(X0)
    assert not _posterior().acq_staged_ok(torch.zeros(5, 2, dtype=torch.float64))      # CPU start points
    assert not _posterior().acq_staged_ok(_starts(dtype=torch.float32))
    assert not _posterior(d=2).acq_staged_ok(X0)
    assert not _posterior(D=17).acq_staged_ok(_starts(D=17))
    assert _posterior(D=16).acq_staged_ok(_starts(D=16))
    assert not _posterior(tree=([{}, {}], None, None)).acq_staged_ok(X0)      # a composed kernel
    assert not _posterior(kfun=5).acq_staged_ok(X0)                           # LinearKernel
    assert not _posterior(n=cap + 1).acq_staged_ok(X0)
    assert not _posterior(n=0).acq_staged_ok(X0)
    # the stack: every member, and at most 8 of them
    stack = lambda members: PosteriorStack(members, [1.0] * len(members))
    assert stack([_posterior(300), _posterior(300), _posterior(250)]).acq_staged_ok(X0)
    assert not stack([_posterior(300), _posterior(cap + 1)]).acq_staged_ok(X0)
    assert not stack([_posterior(300), _posterior(40, tree=([{}, {}], None, None))]).acq_staged_ok(X0)
    assert not stack([_posterior(12)] * 9).acq_staged_ok(X0)


def test_staged_takes_three_values_only():
    from fidelityfusion_amd.posterior import PosteriorStack
    with pytest.raises(ValueError):
        PosteriorStack([_posterior()], [1.0]).optimize_acquisition(_starts(), staged="always")
