"""CPU: the launch-per-stage acquisition call for NAR chains with composed-kernel members (ffgp_acq_optimize_chain_tree_staged,
include/ffgp.h; csrc/acq_staged_chain_tree.hip), its host side without a GPU: the declaration, the export list and the Makefile, the new
kernels' private segments (tools/check_isa.py), `PosteriorChain.acq_chain_tree_staged_ok` and the route of every
(`fuse_composed`, `staged`) pair on test_acq_chain_tree_host.py's stand-ins, imported as they stand, the values `fuse_composed` takes,
and the fixture of the reference's loop at NAR's demo sizes (tests/golden/mf_acq_nar_sum_n300.npz, written by
gen_nar_acq_sum_staged_goldens.py).  Nothing below creates a library handle."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_acq_chain_tree_host import LINEAR, M52, SE, _chain, _member, header      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ffgp_acq_optimize_chain_tree_staged"
TREE = [LINEAR, M52]


def test_header_declares_the_entry_with_the_chain_tree_entrys_arguments():
    from fidelityfusion_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    args = lambda name: re.sub(r"\s+", " ", re.search(r"\bint %s\s*\(([^)]*)\)" % name, src).group(1)).strip()
    assert args(NAME) == args("ffgp_acq_optimize_chain_tree")      # one for one
    assert NAME in _lib.EXPORTS and getattr(_lib.lib, NAME) is not None
    new, old = _lib.EXPORTS[NAME], _lib.EXPORTS["ffgp_acq_optimize_chain_tree"]
    assert new[0] is C.c_int and list(new[1]) == list(old[1])
    # the workspace formula stands beside the declaration
    doc = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int %s\(" % NAME, header(), flags=re.S).group(1)
    for piece in ("3 n_f Qp", "Qp DM", "28 F", "1 + Qp"):
        assert piece in doc, piece


def test_the_export_list_and_the_makefile_hold_the_new_file():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "fidelityfusion_amd", "csrc", "gen_exports.py"),
                                   os.path.join(ROOT, "include", "ffgp.h")], text=True)
    assert "    %s;\n" % NAME in out
    src = open(os.path.join(ROOT, "fidelityfusion_amd", "csrc", "Makefile")).read()
    assert " acq_staged_chain_tree.hip" in re.search(r"^SRCS = (.*)$", src, flags=re.M).group(1)
    assert os.path.exists(os.path.join(ROOT, "fidelityfusion_amd", "csrc", "acq_staged_chain_tree.hip"))


def test_both_libraries_export_the_entry():
    for so in ("libffgp.so", "libffgp_roles.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "fidelityfusion_amd", so)], check=True, capture_output=True,
                             text=True).stdout
        assert re.search(r"\bT %s\b" % NAME, out), "%s does not export %s" % (so, NAME)


def test_the_new_kernels_keep_no_scratch():
    """.private_segment_fixed_size of the K_s, value and gradient kernels (every DM) in the gfx950 code object's metadata; the census
    kernel stays where it was, and that file's count stays 8"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_isa
    sizes = check_isa.check_acq_staged_chain_tree_no_scratch()
    assert len(sizes) == 7 and set(sizes.values()) == {0}, sizes
    assert sum("ks_kernel" in k for k in sizes) == 3 and sum("grad_kernel" in k for k in sizes) == 3 and sum("value_kernel" in k for k in sizes) == 1
    assert len(check_isa.check_acq_staged_chain_no_scratch()) == 8


def mixed(ns, D=2, top=TREE, **kw):
    """a radial chain on x [D] whose LAST member carries the tree `top` (a list of leaf kfuns) or the radial kernel `top` (an int)"""
    last = len(ns) - 1
    return _chain([_member(n, D + (1 if f else 0), top if f == last else SE, **(kw if f == last else {})) for f, n in enumerate(ns)])


def test_acq_chain_tree_staged_ok():
    from fidelityfusion_amd import _lib
    from fidelityfusion_amd.posterior import PosteriorChain
    cap = _lib.FFGP_ACQ_STAGED_MAX_N
    assert cap == 2048
    ok = lambda ch: ch.acq_chain_tree_staged_ok(None)
    assert ok(mixed((257, 24))) and ok(mixed((24, 257))) and not mixed((257, 24)).acq_tree_fusable(None)
    assert ok(mixed((cap, 24))) and ok(mixed((24, cap))) and ok(mixed((cap,)))
    assert not ok(mixed((cap + 1, 24))) and not ok(mixed((24, cap + 1))) and not ok(mixed((0, 24)))
    assert ok(mixed((300, 300, 250))) and ok(mixed((40, 24)))      # the one-launch sizes are within the rules too
    assert ok(mixed((300, 300), D=15)) and not ok(mixed((300, 300), D=16))      # D + 1 = 16 | 17
    assert ok(_chain([_member(300, 2, TREE)] + [_member(12, 3, SE)] * 7)) and not ok(_chain([_member(300, 2, TREE)] + [_member(12, 3, SE)] * 8))
    assert not ok(mixed((300, 300), d=2))
    assert not ok(mixed((300, 300), top=[LINEAR])) and not ok(mixed((300, 300), top=[SE] * 5))      # leaf counts 1 and 5
    assert ok(mixed((300, 300), top=[SE, LINEAR, M52, 4]))
    assert not ok(mixed((300, 300), top=[SE, 6]))                  # an unknown leaf kfun
    assert not ok(mixed((300, 300), top=LINEAR)) and not ok(mixed((300,), top=LINEAR))      # a lone LINEAR radial member
    assert ok(mixed((300, 300), top=SE))                           # an all-radial chain satisfies the rules (the radial staged call takes it first)
    # the start points, through the real predicate
    big = mixed((300, 300))
    big._acq_starts_ok = lambda X0: PosteriorChain._acq_starts_ok(big, X0)
    assert not big.acq_chain_tree_staged_ok(torch.zeros(5, 2, dtype=torch.float64))      # on the CPU
    assert not big.acq_chain_tree_staged_ok(torch.zeros(5, 2, dtype=torch.float32))
    # the stacks' predicates stay False for a chain
    assert not big.acq_staged_ok(None) and not big.acq_tree_staged_ok(None)


FC, ST = (False, True, "staged"), (False, True, "force")


def test_the_route_of_every_pair_of_keywords():
    name = lambda r: (r[0].__name__ if r[0] is not None else None, r[1])
    new = ("_acq_call_chain_trees_staged", True)
    big, small, radial, outside = mixed((300, 24)), mixed((40, 24)), mixed((300, 24), top=SE), mixed((2049, 24))
    for fc in FC:
        for st in ST:
            got = name(big._acq_route(None, fc, st))
            assert got == (new if fc == "staged" and st in (True, "force") else (None, False)), (fc, st, got)
            got = name(small._acq_route(None, fc, st))
            want = (None, False) if fc is False else new if (fc, st) == ("staged", "force") else ("_acq_call_trees", False)
            assert got == want, (fc, st, got)
            got = name(radial._acq_route(None, fc, st))
            assert got == (("_acq_call_chain_staged", True) if st else (None, False)), (fc, st, got)
            assert name(outside._acq_route(None, fc, st)) == (None, False), (fc, st)
    assert name(big._acq_route(None, True, True)) == (None, False)                  # today's route is kept without the new value
    assert name(small._acq_route(None, "staged", True)) == ("_acq_call_trees", False)      # the one-launch call stays the route at n <= 256


def test_fuse_composed_takes_three_values_only():
    ch = mixed((300, 24))
    for bad in ("force", "Staged", 2, None):
        with pytest.raises(ValueError, match="fuse_composed"):
            ch.optimize_acquisition(torch.zeros(5, 2, dtype=torch.float64), fuse_composed=bad)
    with pytest.raises(TypeError, match="fuse_compose"):
        ch.optimize_acquisition(torch.zeros(5, 2, dtype=torch.float64), fuse_compose="staged")


def test_fixture_loads_and_is_well_conditioned():
    z = np.load(os.path.join(ROOT, "tests", "golden", "mf_acq_nar_sum_n300.npz"))
    small = np.load(os.path.join(ROOT, "tests", "golden", "mf_acq_nar_sum.npz"))
    assert float(z["twin_distance"]) <= 1e-11
    ns = [z["x_%d" % f].shape[0] for f in range(3)]
    assert ns == [300, 300, 250] and all(z["y_%d" % f].shape == (ns[f], 1) for f in range(3))
    assert [z["x_%d" % f].shape[1] for f in range(3)] == [2, 3, 3]
    assert sorted(z.files) == sorted(small.files)      # the keys and layouts of the small fixture
    for k in ("lin_length_scale", "lin_signal_variance", "matern_length_scale", "matern_signal_variance", "log_beta", "kappa", "lr", "steps",
              "lin_center_0", "lin_center_1", "lin_center_2"):
        assert np.array_equal(z[k], small[k]), k
    assert float(z["lin_center_1"][2]) != 0.0      # the middle member's linear leaf is centred on the mean coordinate too
    steps = int(z["steps"])
    assert steps == 10 and z["X0"].shape == (3, 6, 2)
    for tag in ("zg", "acc"):
        assert z["trace_" + tag].shape == (3, steps, 6) and z["hist_" + tag].shape == (3, steps + 1, 6, 2)
        assert np.array_equal(z["hist_" + tag][:, 0], z["X0"])
        assert np.isfinite(z["trace_" + tag]).all() and np.isfinite(z["hist_" + tag]).all()
        moved = np.abs(z["hist_" + tag][:, -1] - z["X0"]).max()
        assert 0.05 < moved < 0.2, moved
    assert np.array_equal(z["hist_zg"][:, 1], z["hist_acc"][:, 1]) and not np.array_equal(z["hist_zg"][:, 2], z["hist_acc"][:, 2])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mf_acq_nar_sum_n300.npz")) < 64 * 1024
