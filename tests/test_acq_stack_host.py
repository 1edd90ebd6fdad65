"""CPU: the binding of the stack acquisition optimiser (ffgp_acq_optimize_stack, include/ffgp.h) and the fixture of the reference's
multi-fidelity loop (tests/golden/mf_acq_ar.npz, written by gen_mf_acq_goldens.py).  No GPU: nothing below creates a library handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "ffgp.h")).read()


def struct_fields(hdr, name):
    """the field names of `typedef struct { ... } name;` in declaration order"""
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} %s;" % name, hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = re.sub(r"^\s*(const\s+)?\w+\s*\**", "", decl.strip(), count=1)      # drop the type
        names += [n.strip(" *\n") for n in decl.split(",") if n.strip(" *\n")]
    return names


def test_binding_declares_the_stack_entry_and_its_limits():
    from fidelityfusion_amd import _lib
    assert "ffgp_acq_optimize_stack" in _lib.EXPORTS and _lib.lib.ffgp_acq_optimize_stack is not None
    hdr = header()
    assert re.search(r"#define FFGP_ACQ_MAX_MEMBERS %d\b" % _lib.FFGP_ACQ_MAX_MEMBERS, hdr)
    assert re.search(r"#define FFGP_ACQ_UCB_VAR %d\b" % _lib.FFGP_ACQ_UCB_VAR, hdr)
    assert _lib.FFGP_ACQ_MAX_MEMBERS == 8 and _lib.FFGP_ACQ_UCB_VAR == 2
    assert re.search(r"int ffgp_acq_optimize_stack\(ffgp_handle\*", hdr)
    # same arguments as the single entry but for the problem structure
    one, stack = _lib.EXPORTS["ffgp_acq_optimize"], _lib.EXPORTS["ffgp_acq_optimize_stack"]
    assert stack[0] is C.c_int and len(stack[1]) == len(one[1]) and stack[1][2:] == one[1][2:]
    assert stack[1][1] is C.POINTER(_lib.AcqStack) or stack[1][1]._type_ is _lib.AcqStack


def test_binding_structures_follow_the_header():
    from fidelityfusion_amd import _lib
    hdr = header()
    assert [f[0] for f in _lib.AcqMember._fields_] == struct_fields(hdr, "ffgp_acq_member")
    assert [f[0] for f in _lib.AcqStack._fields_] == struct_fields(hdr, "ffgp_acq_stack")
    assert dict(_lib.AcqMember._fields_)["ldl"] is C.c_long      # `long ldl`, where ffgp_acq_problem has an int
    # natural alignment on LP64: 3 ints (+4) | 2 pointers | long | 3 pointers | double | int (+4) | 4 doubles
    assert C.sizeof(_lib.AcqMember) == 16 + 16 + 8 + 24 + 8 + 8 + 32
    assert C.sizeof(_lib.AcqStack) == 8 + 8 + 8 + 8 + 8 + 24 + 8


def test_fixture_loads_and_is_well_conditioned():
    z = np.load(os.path.join(ROOT, "tests", "golden", "mf_acq_ar.npz"))
    assert float(z["twin_distance"]) <= 1e-11
    ns = [z["x_%d" % f].shape[0] for f in range(3)]
    assert ns == [24, 17, 12] and all(z["x_%d" % f].shape[1] == 2 and z["y_%d" % f].shape == (ns[f], 1) for f in range(3))
    steps = int(z["steps"])
    assert steps == 10 and float(z["lr"]) == 0.01 and z["X0"].shape == (3, 6, 2) and list(z["rho"]) == [0.8, 1.2]
    for tag in ("zg", "acc"):
        assert z["trace_" + tag].shape == (3, steps, 6) and z["hist_" + tag].shape == (3, steps + 1, 6, 2)
        assert np.array_equal(z["hist_" + tag][:, 0], z["X0"])
        assert np.isfinite(z["trace_" + tag]).all() and np.isfinite(z["hist_" + tag]).all()
    # the first step sees the same gradient either way; from the second on the accumulating loop differs
    assert np.array_equal(z["hist_zg"][:, 1], z["hist_acc"][:, 1]) and not np.array_equal(z["hist_zg"][:, 2], z["hist_acc"][:, 2])


def test_posterior_stack_checks_its_arguments_without_a_gpu():
    from fidelityfusion_amd import functional as F
    from fidelityfusion_amd.posterior import PosteriorStack
    assert F.PosteriorStack is PosteriorStack
    with pytest.raises(ValueError):
        PosteriorStack([], [])
    with pytest.raises(ValueError):
        PosteriorStack([object()], [1.0])
