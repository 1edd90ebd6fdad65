"""The launch-per-stage acquisition call for composed kernels, its host side without a GPU: the export, the ctypes declaration against
ffgp_acq_optimize_stack_tree's, the `acq_tree_staged_ok` predicates on hand-made posteriors (test_acq_staged_host.py's `_posterior` /
`_OnGpu`, imported as they stand), and `acq_staged_ok`, which stays False for trees."""
import ctypes
import os
import re
import subprocess

import pytest

torch = pytest.importorskip("torch")

from test_acq_staged_host import _posterior, _starts      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ffgp_acq_optimize_stack_tree_staged"
SE, M52, LINEAR = 0, 3, 5


def test_the_library_exports_the_entry():
    for so in ("libffgp.so", "libffgp_roles.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "fidelityfusion_amd", so)], check=True, capture_output=True,
                             text=True).stdout
        assert re.search(r"\bT %s\b" % NAME, out), "%s does not export %s" % (so, NAME)


def test_lib_declares_the_function():
    from fidelityfusion_amd import _lib
    fn = getattr(_lib.lib, NAME)
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == list(_lib.lib.ffgp_acq_optimize_stack_tree.argtypes)      # that entry's arguments, one for one


def test_the_header_declares_the_entry_with_the_tree_entrys_arguments():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ffgp.h")).read(), flags=re.S)
    args = lambda name: re.sub(r"\s+", " ", re.search(r"\bint %s\s*\(([^)]*)\)" % name, src).group(1)).strip()
    assert args(NAME) == args("ffgp_acq_optimize_stack_tree")


def tree(*kfuns):
    """the descriptor list the predicate reads: a `kfun` per leaf"""
    return ([{"kfun": k} for k in kfuns], None, None)


def test_acq_tree_staged_ok():
    from fidelityfusion_amd import _lib
    cap = _lib.FFGP_ACQ_STAGED_MAX_N
    X0, t2 = _starts(), tree(LINEAR, M52)
    p = _posterior(300, tree=t2)
    assert p.acq_tree_staged_ok(X0) and not p.acq_tree_fusable(X0)      # n = 300: past the one-launch limit, within the cap
    assert _posterior(cap, tree=t2).acq_tree_staged_ok(X0)
    assert _posterior(40, tree=t2).acq_tree_staged_ok(X0) and _posterior(40, tree=t2).acq_tree_fusable(X0)
    assert _posterior(300, tree=tree(SE, LINEAR, M52)).acq_tree_staged_ok(X0)
    assert _posterior(300, tree=tree(SE, LINEAR, M52, SE)).acq_tree_staged_ok(X0)
    assert _posterior(300, D=16, tree=t2).acq_tree_staged_ok(_starts(D=16))
    assert not _posterior(cap + 1, tree=t2).acq_tree_staged_ok(X0)      # n = 2049
    assert not _posterior(0, tree=t2).acq_tree_staged_ok(X0)
    assert not _posterior(300, d=2, tree=t2).acq_tree_staged_ok(X0)
    assert not _posterior(300, D=17, tree=t2).acq_tree_staged_ok(_starts(D=17))
    assert not p.acq_tree_staged_ok(torch.zeros(5, 2, dtype=torch.float64))      # CPU start points
    assert not p.acq_tree_staged_ok(_starts(dtype=torch.float32))
    assert not p.acq_tree_staged_ok(_starts(D=3))
    assert not _posterior(300, tree=tree(M52)).acq_tree_staged_ok(X0)                           # one leaf
    assert not _posterior(300, tree=tree(SE, LINEAR, M52, SE, SE)).acq_tree_staged_ok(X0)       # five
    assert not _posterior(300, tree=tree(SE, 6)).acq_tree_staged_ok(X0)                         # not a library leaf
    assert not _posterior(300).acq_tree_staged_ok(X0)                                           # no tree: the radial staged call's business


def test_the_stack_predicate_takes_mixed_stacks_of_at_most_eight_members():
    from fidelityfusion_amd import _lib
    from fidelityfusion_amd.posterior import PosteriorChain, PosteriorStack
    cap = _lib.FFGP_ACQ_STAGED_MAX_N
    X0, t2 = _starts(), tree(LINEAR, M52)
    stack = lambda members: PosteriorStack(members, [1.0] * len(members))
    assert stack([_posterior(300, tree=t2), _posterior(300, tree=t2), _posterior(250, tree=t2)]).acq_tree_staged_ok(X0)
    mixed = stack([_posterior(300), _posterior(40, tree=t2), _posterior(2048, tree=tree(SE, LINEAR, M52, SE))])
    assert mixed.acq_tree_staged_ok(X0) and not mixed.acq_staged_ok(X0) and not mixed.acq_tree_fusable(X0)
    assert stack([_posterior(300), _posterior(250)]).acq_tree_staged_ok(X0)      # all radial: eligible, though the radial call is routed first
    assert not stack([_posterior(300, tree=t2), _posterior(cap + 1)]).acq_tree_staged_ok(X0)
    assert not stack([_posterior(300, tree=t2), _posterior(cap + 1, tree=t2)]).acq_tree_staged_ok(X0)
    assert not stack([_posterior(300), _posterior(40, kfun=LINEAR)]).acq_tree_staged_ok(X0)      # a bare LinearKernel member
    assert not stack([_posterior(300, tree=t2), _posterior(40, tree=tree(SE, LINEAR, M52, SE, SE))]).acq_tree_staged_ok(X0)
    assert stack([_posterior(12, tree=t2)] * 8).acq_tree_staged_ok(X0)
    assert not stack([_posterior(12, tree=t2)] * 9).acq_tree_staged_ok(X0)
    chain = PosteriorChain([_posterior(300, D=2), _posterior(300, D=3)])
    assert not chain.acq_tree_staged_ok(X0) and not chain.acq_staged_ok(X0)


def test_acq_staged_ok_is_unchanged_for_trees():
    X0 = _starts()
    assert not _posterior(300, tree=tree(LINEAR, M52)).acq_staged_ok(X0)
    assert not _posterior(40, tree=tree(SE, M52)).acq_staged_ok(X0)
    assert not _posterior(300, kfun=LINEAR).acq_staged_ok(X0)
    assert _posterior(300).acq_staged_ok(X0)


def test_the_route_of_each_keyword_combination():
    """`_acq_route` on hand-made posteriors: which C entry a call takes, nothing is launched"""
    from fidelityfusion_amd.posterior import PosteriorStack, _TreePosterior
    X0, t2 = _starts(), tree(LINEAR, M52)
    name = lambda r: (r[0].__name__ if r[0] is not None else None, r[1])
    big, small = PosteriorStack([_posterior(300, tree=t2), _posterior(300)], [1.0, 0.8]), PosteriorStack([_posterior(40, tree=t2)], [1.0])
    radial = PosteriorStack([_posterior(300), _posterior(250)], [1.0, 0.8])
    for fc, st, want in [(False, False, (None, False)), (True, False, (None, False)), (False, True, (None, False)),
                         (False, "force", (None, False)), (True, True, ("_acq_call_trees_staged", True)),
                         (True, "force", ("_acq_call_trees_staged", True))]:
        assert name(big._acq_route(X0, fc, st)) == want, (fc, st)
    for fc, st, want in [(False, False, (None, False)), (True, False, ("_acq_call_trees", False)), (False, True, (None, False)),
                         (True, True, ("_acq_call_trees", False)), (True, "force", ("_acq_call_trees_staged", True))]:
        assert name(small._acq_route(X0, fc, st)) == want, (fc, st)
    for fc, st, want in [(False, False, (None, False)), (True, False, (None, False)), (False, True, ("_acq_call_staged", True)),
                         (True, True, ("_acq_call_staged", True))]:
        assert name(radial._acq_route(X0, fc, st)) == want, (fc, st)
    one = _TreePosterior([_posterior(300, tree=t2)], [1.0])      # Posterior.optimize_acquisition(..., fuse_composed=True)
    assert name(one._acq_route(X0, True, True)) == ("_acq_call_trees_staged", True) and name(one._acq_route(X0, True, False)) == (None, False)
    one = _TreePosterior([_posterior(256, tree=t2)], [1.0])
    assert name(one._acq_route(X0, True, True)) == ("_acq_call", False) and name(one._acq_route(X0, True, "force")) == ("_acq_call_trees_staged", True)
    outside = _TreePosterior([_posterior(2049, tree=t2)], [1.0])
    assert name(outside._acq_route(X0, True, True)) == (None, False)
