"""CPU: the binding of the acquisition optimiser on stacks with composed-kernel members (ffgp_acq_optimize_stack_tree, include/ffgp.h)
and the fixture of the reference's multi-fidelity loop on SumKernel(LinearKernel, MaternKernel) fidelities
(tests/golden/mf_acq_ar_sum.npz, written by gen_mf_acq_ar_sum_goldens.py).  No GPU: nothing below creates a library handle."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "ffgp.h")).read()


def test_header_declares_the_entry_and_the_binding_matches():
    from fidelityfusion_amd import _lib
    assert "ffgp_acq_optimize_stack_tree" in _lib.EXPORTS and _lib.lib.ffgp_acq_optimize_stack_tree is not None
    hdr = header()
    decl = re.search(r"int ffgp_acq_optimize_stack_tree\(([^;]*)\);", hdr)
    assert decl, "include/ffgp.h does not declare ffgp_acq_optimize_stack_tree"
    args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    assert args[:3] == ["ffgp_handle* h", "const ffgp_acq_stack* s", "const ffgp_ktree* const* trees"]
    # the stack entry's arguments with the host array of trees behind the stack
    stack, new = _lib.EXPORTS["ffgp_acq_optimize_stack"], _lib.EXPORTS["ffgp_acq_optimize_stack_tree"]
    assert new[0] is C.c_int and len(new[1]) == len(args) == len(stack[1]) + 1
    assert new[1][:2] == stack[1][:2] and new[1][3:] == stack[1][2:]
    assert new[1][2] is C.POINTER(C.POINTER(_lib.KTree))
    # the stack's structures serve as they stand
    assert new[1][1] is C.POINTER(_lib.AcqStack)


def test_limits_and_structures_are_unchanged():
    from fidelityfusion_amd import _lib
    hdr = header()
    for name, value in (("FFGP_ACQ_MAX_N", 256), ("FFGP_ACQ_MAX_D", 16), ("FFGP_ACQ_MAX_MEMBERS", 8), ("FFGP_ACQ_MAX_STEPS", 4096),
                        ("FFGP_ACQ_UCB_VAR", 2)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
        assert getattr(_lib, name) == value
    assert C.sizeof(_lib.AcqMember) == 16 + 16 + 8 + 24 + 8 + 8 + 32
    assert C.sizeof(_lib.AcqStack) == 8 + 8 + 8 + 8 + 8 + 24 + 8
    # natural alignment on LP64: 2 ints | 3 ints (+4) | pointer
    assert C.sizeof(_lib.KTree) == 8 + 16 + 8


def test_python_interface_has_the_keyword_off_by_default():
    from fidelityfusion_amd import acq
    from fidelityfusion_amd.posterior import PosteriorChain, PosteriorStack
    assert inspect.signature(PosteriorStack.optimize_acquisition).parameters["fuse_composed"].default is False
    assert inspect.signature(acq.optimize_acqf_mf).parameters["fuse_composed"].default is False
    assert callable(PosteriorStack.acq_tree_fusable)
    assert "fuse_composed" not in inspect.signature(PosteriorChain.optimize_acquisition).parameters      # NAR keeps its signature and routing


def test_fixture_loads_and_is_well_conditioned():
    z = np.load(os.path.join(ROOT, "tests", "golden", "mf_acq_ar_sum.npz"))
    assert float(z["twin_distance"]) <= 1e-11
    ns = [z["x_%d" % f].shape[0] for f in range(3)]
    assert ns == [24, 17, 12] and all(z["x_%d" % f].shape[1] == 2 and z["y_%d" % f].shape == (ns[f], 1) for f in range(3))
    steps = int(z["steps"])
    assert steps == 10 and float(z["lr"]) == 0.01 and z["X0"].shape == (3, 6, 2) and list(z["rho"]) == [0.8, 1.2]
    assert z["lin_center"].shape == (3, 2) and np.any(z["lin_center"] != 0.0)      # a non-zero linear centre on one fidelity
    assert all(z[k].shape == (3,) for k in ("lin_length_scale", "lin_signal_variance", "matern_length_scale", "matern_signal_variance", "log_beta"))
    for tag in ("zg", "acc"):
        assert z["trace_" + tag].shape == (3, steps, 6) and z["hist_" + tag].shape == (3, steps + 1, 6, 2)
        assert np.array_equal(z["hist_" + tag][:, 0], z["X0"])
        assert np.isfinite(z["trace_" + tag]).all() and np.isfinite(z["hist_" + tag]).all()
    # the first step sees the same gradient either way; from the second on the accumulating loop differs
    assert np.array_equal(z["hist_zg"][:, 1], z["hist_acc"][:, 1]) and not np.array_equal(z["hist_zg"][:, 2], z["hist_acc"][:, 2])
