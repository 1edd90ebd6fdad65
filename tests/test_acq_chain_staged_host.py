"""The chain's launch-per-stage acquisition call, its host side without a GPU: the export from both libraries, the ctypes declaration
and the header's argument list against ffgp_acq_optimize_chain's, the new kernels' private segments (tools/check_isa.py),
`PosteriorChain.acq_chain_staged_ok` on hand-made posteriors (test_acq_staged_host.py's `_posterior` / `_starts`, imported as they
stand), and the route each value of `staged` takes."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

from test_acq_staged_host import _posterior, _starts      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ffgp_acq_optimize_chain_staged"
SE, LINEAR = 0, 5


def test_both_libraries_export_the_entry():
    for so in ("libffgp.so", "libffgp_roles.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "fidelityfusion_amd", so)], check=True, capture_output=True,
                             text=True).stdout
        assert re.search(r"\bT %s\b" % NAME, out), "%s does not export %s" % (so, NAME)


def test_lib_declares_the_function():
    from fidelityfusion_amd import _lib
    fn = getattr(_lib.lib, NAME)
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == list(_lib.lib.ffgp_acq_optimize_chain.argtypes)      # the chain entry's arguments, one for one


def test_the_header_declares_the_entry_with_the_chain_entrys_arguments():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ffgp.h")).read(), flags=re.S)
    args = lambda name: re.sub(r"\s+", " ", re.search(r"\bint %s\s*\(([^)]*)\)" % name, src).group(1)).strip()
    assert args(NAME) == args("ffgp_acq_optimize_chain")


def test_the_new_kernels_keep_no_scratch():
    """.private_segment_fixed_size of the census, K_s, value and gradient kernels (every DM) in the gfx950 code object's metadata"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_isa
    sizes = check_isa.check_acq_staged_chain_no_scratch()
    assert len(sizes) == 8 and set(sizes.values()) == {0}, sizes


def test_the_two_entry_points_accept_staged():
    from fidelityfusion_amd import acq
    from fidelityfusion_amd.posterior import PosteriorChain
    for fn in (PosteriorChain.optimize_acquisition, acq.optimize_acqf_nar):
        p = inspect.signature(fn).parameters
        assert "staged" in p and p["staged"].default is False, fn


def chain(ns, D=2, **kw):
    """a chain on x [D] of hand-made posteriors: member 0 takes D inputs, the others D + 1; `kw` goes to the LAST member"""
    from fidelityfusion_amd.posterior import PosteriorChain
    last = len(ns) - 1
    return PosteriorChain([_posterior(n, D=D + (1 if f else 0), **(kw if f == last else {})) for f, n in enumerate(ns)])


def test_acq_chain_staged_ok():
    from fidelityfusion_amd import _lib
    cap = _lib.FFGP_ACQ_STAGED_MAX_N
    assert cap == 2048
    X0 = _starts()
    big = chain((300, 300, 250))
    assert big.acq_chain_staged_ok(X0) and not big.acq_fusable(X0)      # n = 300: past the one-launch limit, within the cap
    assert chain((300, cap)).acq_chain_staged_ok(X0) and chain((cap,)).acq_chain_staged_ok(X0)
    small = chain((40, 24))
    assert small.acq_chain_staged_ok(X0) and small.acq_fusable(X0)
    assert not chain((300, cap + 1)).acq_chain_staged_ok(X0) and not chain((cap + 1, 300)).acq_chain_staged_ok(X0)
    assert not chain((300, 0)).acq_chain_staged_ok(X0) and not chain((0,)).acq_chain_staged_ok(X0)
    assert not chain((300, 300), d=2).acq_chain_staged_ok(X0)
    assert chain((300, 300), D=15).acq_chain_staged_ok(_starts(D=15))           # D + 1 = 16
    assert not chain((300, 300), D=16).acq_chain_staged_ok(_starts(D=16))       # D + 1 = 17
    assert not chain((300, 300), tree=([{}, {}], None, None)).acq_chain_staged_ok(X0)      # a composed kernel
    assert not chain((300, 300), kfun=LINEAR).acq_chain_staged_ok(X0)
    assert not chain((300,), kfun=LINEAR).acq_chain_staged_ok(X0)
    assert chain((12,) * 8).acq_chain_staged_ok(X0) and not chain((12,) * 9).acq_chain_staged_ok(X0)
    assert not big.acq_chain_staged_ok(torch.zeros(5, 2, dtype=torch.float64))      # CPU start points
    assert not big.acq_chain_staged_ok(_starts(dtype=torch.float32))
    assert not big.acq_chain_staged_ok(_starts(D=3))                               # the width of x, not of z
    assert not big.acq_chain_staged_ok(torch.zeros(2, dtype=torch.float64))
    # the stacks' predicates stay False for a chain
    for c in (big, small):
        assert not c.acq_staged_ok(X0) and not c.acq_tree_staged_ok(X0)


def test_the_route_of_each_value_of_staged():
    """`_acq_route` on hand-made posteriors: which C entry a call takes, nothing is launched"""
    X0 = _starts()
    name = lambda r: (r[0].__name__ if r[0] is not None else None, r[1])
    big, small, outside = chain((300, 300)), chain((40, 24)), chain((2049,))
    for st, want in [(False, (None, False)), (True, ("_acq_call_chain_staged", True)), ("force", ("_acq_call_chain_staged", True))]:
        assert name(big._acq_route(X0, False, st)) == want, st
    for st, want in [(False, ("_acq_call", False)), (True, ("_acq_call", False)), ("force", ("_acq_call_chain_staged", True))]:
        assert name(small._acq_route(X0, False, st)) == want, st
    for st in (False, True, "force"):
        assert name(outside._acq_route(X0, False, st)) == (None, False), st
    # a composed member keeps the per-step loop whatever the keyword says
    odd = chain((300, 300), tree=([{}, {}], None, None))
    for st in (False, True, "force"):
        assert name(odd._acq_route(X0, False, st)) == (None, False), st


def test_staged_takes_three_values_only():
    with pytest.raises(ValueError):
        chain((300, 300)).optimize_acquisition(_starts(), staged="always")
