"""CPU: the binding of the chain acquisition optimiser (ffgp_acq_optimize_chain, include/ffgp.h), `PosteriorChain`'s argument checks and
the fixture of the reference's multi-fidelity loop on its NAR (tests/golden/mf_acq_nar.npz, written by gen_nar_acq_goldens.py).  No GPU:
nothing below creates a library handle."""
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


def test_binding_declares_the_chain_entry():
    from fidelityfusion_amd import _lib
    assert "ffgp_acq_optimize_chain" in _lib.EXPORTS and _lib.lib.ffgp_acq_optimize_chain is not None
    hdr = header()
    assert re.search(r"int ffgp_acq_optimize_chain\(ffgp_handle\*", hdr)
    # same arguments as the stack entry but for the problem structure, whose fields are the stack's, one by one
    stack, chain = _lib.EXPORTS["ffgp_acq_optimize_stack"], _lib.EXPORTS["ffgp_acq_optimize_chain"]
    assert chain[0] is C.c_int and len(chain[1]) == len(stack[1]) and chain[1][2:] == stack[1][2:]
    assert chain[1][1]._type_ is _lib.AcqChain
    assert [f[0] for f in _lib.AcqChain._fields_] == struct_fields(hdr, "ffgp_acq_chain") == struct_fields(hdr, "ffgp_acq_stack")
    assert [f[1] for f in _lib.AcqChain._fields_] == [f[1] for f in _lib.AcqStack._fields_]
    assert C.sizeof(_lib.AcqChain) == C.sizeof(_lib.AcqStack)


def test_fixture_loads_and_is_well_conditioned():
    z = np.load(os.path.join(ROOT, "tests", "golden", "mf_acq_nar.npz"))
    assert float(z["twin_distance"]) <= 1e-11
    ns = [z["x_%d" % f].shape[0] for f in range(3)]
    assert ns == [24, 17, 12] and all(z["y_%d" % f].shape == (ns[f], 1) for f in range(3))
    assert [z["x_%d" % f].shape[1] for f in range(3)] == [2, 3, 3]      # the concat sets carry the mean below as a third column
    steps = int(z["steps"])
    assert steps == 10 and float(z["lr"]) == 0.01 and z["X0"].shape == (3, 6, 2) and float(z["kappa"]) == 0.4
    for tag in ("zg", "acc"):
        assert z["trace_" + tag].shape == (3, steps, 6) and z["hist_" + tag].shape == (3, steps + 1, 6, 2)
        assert np.array_equal(z["hist_" + tag][:, 0], z["X0"])
        assert np.isfinite(z["trace_" + tag]).all() and np.isfinite(z["hist_" + tag]).all()
    # the first step sees the same gradient either way; from the second on the accumulating loop differs
    assert np.array_equal(z["hist_zg"][:, 1], z["hist_acc"][:, 1]) and not np.array_equal(z["hist_zg"][:, 2], z["hist_acc"][:, 2])


def test_posterior_chain_checks_its_arguments_without_a_gpu():
    from fidelityfusion_amd import acq, functional as F
    from fidelityfusion_amd.posterior import PosteriorChain, PosteriorStack
    assert F.PosteriorChain is PosteriorChain and issubclass(PosteriorChain, PosteriorStack)
    # the loop and the buffers are the stack class's own, not a copy
    assert PosteriorChain._optimize_acq_fused is PosteriorStack._optimize_acq_fused and PosteriorChain._member_table is PosteriorStack._member_table
    with pytest.raises(ValueError):
        PosteriorChain([])
    with pytest.raises(ValueError):
        PosteriorChain([object()])
    with pytest.raises(ValueError):
        acq.optimize_acqf_nar([], [], None)
    with pytest.raises(ValueError):
        acq.optimize_acqf_nar([object()], [], torch.zeros(1, 2))
