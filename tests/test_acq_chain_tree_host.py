"""CPU: the binding of the acquisition optimiser on chains with composed-kernel members (ffgp_acq_optimize_chain_tree, include/ffgp.h),
the routing predicates and the keyword of `PosteriorChain.optimize_acquisition` / `acq.optimize_acqf_nar`, and the fixture of the
reference's multi-fidelity loop on NAR with SumKernel(LinearKernel, MaternKernel) fidelities (tests/golden/mf_acq_nar_sum.npz, written
by gen_nar_acq_sum_goldens.py).  No GPU: nothing below creates a library handle."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SE, M52, LINEAR = 0, 3, 5


def header():
    return open(os.path.join(ROOT, "include", "ffgp.h")).read()


def test_header_declares_the_entry_and_the_binding_matches():
    from fidelityfusion_amd import _lib
    assert "ffgp_acq_optimize_chain_tree" in _lib.EXPORTS and _lib.lib.ffgp_acq_optimize_chain_tree is not None
    decl = re.search(r"int ffgp_acq_optimize_chain_tree\(([^;]*)\);", header())
    assert decl, "include/ffgp.h does not declare ffgp_acq_optimize_chain_tree"
    args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    assert args[:3] == ["ffgp_handle* h", "const ffgp_acq_chain* c", "const ffgp_ktree* const* trees"]
    # the chain entry's arguments with the host array of trees behind the chain
    chain, new = _lib.EXPORTS["ffgp_acq_optimize_chain"], _lib.EXPORTS["ffgp_acq_optimize_chain_tree"]
    assert new[0] is C.c_int and len(new[1]) == len(args) == len(chain[1]) + 1
    assert new[1][:2] == chain[1][:2] and new[1][3:] == chain[1][2:]
    assert new[1][2] is C.POINTER(C.POINTER(_lib.KTree))
    assert new[1][1] is C.POINTER(_lib.AcqChain)      # the chain's structure serves as it stands
    # ... and the same shape as the stack's entry of the same kind
    assert [a for a in new[1][2:]] == [a for a in _lib.EXPORTS["ffgp_acq_optimize_stack_tree"][1][2:]]


def test_the_library_exports_the_entry_and_the_version_script_lists_it():
    import subprocess
    import sys
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "fidelityfusion_amd", "csrc", "gen_exports.py"),
                                   os.path.join(ROOT, "include", "ffgp.h")], text=True)
    assert "    ffgp_acq_optimize_chain_tree;\n" in out
    src = open(os.path.join(ROOT, "fidelityfusion_amd", "csrc", "Makefile")).read()
    assert " acq_chain_tree.hip" in src


def test_python_interface_has_the_keyword_off_by_default(monkeypatch):
    from fidelityfusion_amd import acq
    from fidelityfusion_amd.posterior import PosteriorChain, PosteriorStack
    assert inspect.signature(acq.optimize_acqf_nar).parameters["fuse_composed"].default is False
    assert inspect.signature(PosteriorChain.optimize_acquisition).parameters["staged"].default is False
    assert callable(PosteriorChain.acq_tree_fusable)
    # the chain's explicit signature stays the radial call's (tests/test_acq_stack_tree_host.py holds it); the keyword travels in a
    # catch-all that takes `fuse_composed` and nothing else, and reaches the stack's loop as False unless given
    params = inspect.signature(PosteriorChain.optimize_acquisition).parameters
    assert [p.name for p in params.values() if p.kind is inspect.Parameter.VAR_KEYWORD] == ["opt_in"]
    seen = []
    monkeypatch.setattr(PosteriorStack, "optimize_acquisition", lambda self, X0, **kw: seen.append(kw) or "ran")
    ch = PosteriorChain.__new__(PosteriorChain)
    assert ch.optimize_acquisition(None) == "ran" and seen[-1]["fuse_composed"] is False and seen[-1]["staged"] is False
    assert ch.optimize_acquisition(None, fuse_composed=True, staged=True) == "ran"
    assert seen[-1]["fuse_composed"] is True and seen[-1]["staged"] is True
    with pytest.raises(TypeError, match="fuse_compose"):
        ch.optimize_acquisition(None, fuse_compose=True)      # a misspelt keyword is refused, not swallowed
    assert len(seen) == 2


# ---- routing, on stand-ins for the members (the predicates read attributes only; no handle, no device) ----------------------------------
def _member(n, D, kfuns, d=1):
    """a stand-in with what the predicates read: one radial kernel (kfuns an int) or a descriptor tree (a list of leaf kfuns)"""
    m = types.SimpleNamespace(n=n, D=D, d=d, dev=torch.device("cuda", 0))
    if isinstance(kfuns, int):
        m.tree, m.kfun = None, (kfuns, 1.0)
    else:
        m.tree, m.kfun = ([{"kfun": k} for k in kfuns], None, None), (0, 1.0)
    return m


def _chain(members):
    from fidelityfusion_amd.posterior import PosteriorChain
    ch = PosteriorChain.__new__(PosteriorChain)
    ch.members, ch.dev, ch.D, ch.F = members, members[0].dev, members[0].D, len(members)
    ch._acq_starts_ok = lambda X0: True      # the start points' device is the GPU tests' business
    return ch


def test_routing_predicates():
    radial = _chain([_member(40, 2, SE), _member(24, 3, SE)])
    mixed = _chain([_member(40, 2, SE), _member(24, 3, [LINEAR, M52])])
    assert radial.acq_fusable(None) and radial.acq_tree_fusable(None)
    assert not mixed.acq_fusable(None) and mixed.acq_tree_fusable(None)
    # without the keyword a composed chain keeps the per-step loop; with it, the new call; an all-radial chain the radial call either way
    assert mixed._acq_route(None, False, False) == (None, False)
    assert mixed._acq_route(None, True, False) == (mixed._acq_call_trees, False)
    assert radial._acq_route(None, True, False) == (radial._acq_call, False) and radial._acq_route(None, False, False) == (radial._acq_call, False)
    # the size rules are acq_fusable's
    assert _chain([_member(256, 2, [LINEAR, M52])]).acq_tree_fusable(None)
    assert not _chain([_member(257, 2, [LINEAR, M52])]).acq_tree_fusable(None)
    assert _chain([_member(40, 15, SE), _member(24, 16, [LINEAR, M52])]).acq_tree_fusable(None)
    assert not _chain([_member(40, 16, SE), _member(24, 17, [LINEAR, M52])]).acq_tree_fusable(None)
    assert _chain([_member(12, 2, [LINEAR, M52])] + [_member(12, 3, SE)] * 7).acq_tree_fusable(None)
    assert not _chain([_member(12, 2, [LINEAR, M52])] + [_member(12, 3, SE)] * 8).acq_tree_fusable(None)
    assert not _chain([_member(40, 2, [LINEAR, M52], d=2)]).acq_tree_fusable(None)
    # the trees the C entry accepts: 2-4 library leaves; a lone linear kernel is no radial member
    assert not _chain([_member(40, 2, [LINEAR])]).acq_tree_fusable(None)
    assert not _chain([_member(40, 2, [SE] * 5)]).acq_tree_fusable(None)
    assert not _chain([_member(40, 2, [SE, 6])]).acq_tree_fusable(None)
    assert not _chain([_member(40, 2, LINEAR)]).acq_tree_fusable(None)
    assert _chain([_member(40, 2, [SE, LINEAR, M52, 4])]).acq_tree_fusable(None)


def test_past_256_points_both_keywords_keep_the_route_of_today():
    big_radial = _chain([_member(300, 2, SE), _member(24, 3, SE)])
    big_mixed = _chain([_member(300, 2, SE), _member(24, 3, [LINEAR, M52])])
    assert big_radial._acq_route(None, True, True) == (big_radial._acq_call_chain_staged, True)      # a radial chain goes staged
    assert big_mixed._acq_route(None, True, True) == (None, False)                                   # a composed one: the per-step loop
    assert big_mixed._acq_route(None, True, "force") == (None, False)
    small_mixed = _chain([_member(40, 2, SE), _member(24, 3, [LINEAR, M52])])
    assert small_mixed._acq_route(None, True, True) == (small_mixed._acq_call_trees, False)          # the one-launch call is kept
    assert small_mixed._acq_route(None, False, True) == (None, False)                                # composed kernels stay opt-in


def test_fixture_loads_and_is_well_conditioned():
    z = np.load(os.path.join(ROOT, "tests", "golden", "mf_acq_nar_sum.npz"))
    assert float(z["twin_distance"]) <= 1e-11
    ns = [z["x_%d" % f].shape[0] for f in range(3)]
    assert ns == [24, 17, 12] and all(z["y_%d" % f].shape == (ns[f], 1) for f in range(3))
    assert [z["x_%d" % f].shape[1] for f in range(3)] == [2, 3, 3]      # above fidelity 0 the mean below is one more input
    assert [z["lin_center_%d" % f].shape for f in range(3)] == [(2,), (3,), (3,)]
    assert not z["lin_center_0"].any() and not z["lin_center_2"].any() and z["lin_center_1"].all()      # the middle member, mean coordinate included
    steps = int(z["steps"])
    assert steps == 10 and float(z["lr"]) == 0.01 and z["X0"].shape == (3, 6, 2) and float(z["kappa"]) == 0.4
    assert all(z[k].shape == (3,) for k in ("lin_length_scale", "lin_signal_variance", "matern_length_scale", "matern_signal_variance", "log_beta"))
    radial = np.load(os.path.join(ROOT, "tests", "golden", "mf_acq_nar.npz"))
    assert np.array_equal(z["X0"], radial["X0"]) and np.array_equal(z["x_0"], radial["x_0"]) and np.array_equal(z["log_beta"], radial["log_beta"])
    for tag in ("zg", "acc"):
        assert z["trace_" + tag].shape == (3, steps, 6) and z["hist_" + tag].shape == (3, steps + 1, 6, 2)
        assert np.array_equal(z["hist_" + tag][:, 0], z["X0"])
        assert np.isfinite(z["trace_" + tag]).all() and np.isfinite(z["hist_" + tag]).all()
        moved = np.abs(z["hist_" + tag][:, -1] - z["X0"]).max()
        assert 0.05 < moved < 0.2, moved
    # the first step sees the same gradient either way; from the second on the accumulating loop differs
    assert np.array_equal(z["hist_zg"][:, 1], z["hist_acc"][:, 1]) and not np.array_equal(z["hist_zg"][:, 2], z["hist_acc"][:, 2])
