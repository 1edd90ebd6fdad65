"""Host-side checks of the composed-kernel trainer (no GPU needed): ffgp_train_tree_raw is declared, exported and bound; the leaves'
links and `tree_links()` give the ids, leaf order and refusals train_many routes on; the reference fixtures hold numbers only."""
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_tree_export_is_declared_exported_and_bound():
    from fidelityfusion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ffgp.h")).read()
    assert re.search(r"\bint ffgp_train_tree_raw\s*\(", hdr)
    assert "ffgp_leaf_links" in hdr and "ffgp_tree_links" in hdr
    so = os.path.join(ROOT, "fidelityfusion_amd", "libffgp.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT ffgp_train_tree_raw\b", syms)
    assert "ffgp_train_tree_raw" in _lib.EXPORTS and _lib.lib.ffgp_train_tree_raw is not None
    # the ctypes mirrors have the C layout: int, double, int, int, double, int -> 40 bytes a leaf; 4 leaves + int + 2 doubles
    assert _lib.LeafLinks.w_c.offset == 8 and _lib.LeafLinks.center_train.offset == 32
    assert (_lib.TreeLinks.dadd_link.offset, _lib.TreeLinks.dadd_c.offset, _lib.TreeLinks.out_scale.offset) == (160, 168, 176)


def test_linear_kernel_links():
    from fidelityfusion_amd import _lib, functional as F, kernel
    k = kernel.LinearKernel(3)
    lk = k.links()
    assert lk["w"] is k.length_scales and lk["amp"] is k.signal_variance and lk["center"] is k.center
    assert (lk["w_link"], lk["w_c"], lk["amp_link"], lk["kfun"]) == (_lib.LINK_INV, 0.0, _lib.LINK_ABS, F.FFGP_KFUN_LINEAR)
    # on its own a linear kernel keeps the composed likelihood path: no raw-parameter call exists for it
    x, y = torch.rand(5, 3, dtype=torch.float64), torch.rand(5, 1, dtype=torch.float64)
    assert F.raw_path(k, x, y) is None


def test_tree_links_order_and_refusals():
    from fidelityfusion_amd import _lib, functional as F, kernel
    lin, mat = kernel.LinearKernel(2), kernel.MaternKernel(2)
    leaves, form, lks = kernel.SumKernel(lin, mat).tree_links()
    assert leaves == [lin, mat] and form == (F.FFGP_TREE_CHAIN, (F.FFGP_KOP_SUM,))
    assert [lk["w_link"] for lk in lks] == [_lib.LINK_INV, _lib.LINK_INV_ABS_EPS] and [lk["kfun"] for lk in lks] == [5, 3]
    assert lks[1].get("center") is None and lks[0]["center"] is lin.center
    # the deeper operand first (commutative nodes): Matern + (Linear * ARD) -> leaves Linear, ARD, Matern; ops (product, sum)
    ard = kernel.ARDKernel(2)
    leaves, form, _ = kernel.SumKernel(mat, kernel.ProductKernel(lin, ard)).tree_links()
    assert leaves == [lin, ard, mat] and form == (F.FFGP_TREE_CHAIN, (F.FFGP_KOP_PRODUCT, F.FFGP_KOP_SUM))
    se, m12 = kernel.SquaredExponentialKernel(), kernel.MaternKernel(2, nu=0.5)
    leaves, form, lks = kernel.ProductKernel(kernel.SumKernel(lin, mat), kernel.SumKernel(se, m12)).tree_links()
    assert leaves == [lin, mat, se, m12] and form == (F.FFGP_TREE_BALANCED, (F.FFGP_KOP_SUM, F.FFGP_KOP_SUM, F.FFGP_KOP_PRODUCT))
    assert (lks[2]["w_link"], lks[2]["amp_link"], lks[3]["kfun"]) == (_lib.LINK_EXP_NEG, _lib.LINK_EXP_SQ, 1)
    leaves, form, _ = kernel.SumKernel(kernel.SumKernel(kernel.ProductKernel(ard, se), mat), lin).tree_links()
    assert leaves == [ard, se, mat, lin] and form == (F.FFGP_TREE_CHAIN, (F.FFGP_KOP_PRODUCT, F.FFGP_KOP_SUM, F.FFGP_KOP_SUM))
    # refusals
    assert kernel.SumKernel(kernel.RationalQuadraticKernel(), mat).tree_links() is None            # learnable profile parameter
    assert kernel.SumKernel(lin, kernel.MaternKernel(2, nu=3.5)).tree_links() is None              # a leaf without links
    assert kernel.SumKernel(ard, ard).tree_links() is None                                         # one module, two leaves
    twin = kernel.ARDKernel(2)
    twin.length_scales = ard.length_scales
    assert kernel.SumKernel(ard, twin).tree_links() is None                                        # one parameter, two leaves
    five = kernel.SumKernel(kernel.SumKernel(kernel.SumKernel(lin, mat), kernel.SumKernel(se, m12)), kernel.ARDKernel(2))
    assert five.tree_links() is None                                                               # more than four leaves

    class User(torch.nn.Module):
        def forward(self, a, b):
            return a @ b.T
    assert kernel.SumKernel(User(), mat).tree_links() is None
    kernel.FUSE_PAIRS = False
    try:
        assert kernel.SumKernel(lin, mat).tree_links() is None
    finally:
        kernel.FUSE_PAIRS = True


def test_cpu_models_are_not_eligible():
    from fidelityfusion_amd import kernel, train
    from fidelityfusion_amd.cigp_v10 import cigp
    m = cigp(kernel.SumKernel(kernel.LinearKernel(2), kernel.MaternKernel(2)), 1.0).double()
    x, y = torch.rand(6, 2, dtype=torch.float64), torch.rand(6, 1, dtype=torch.float64)
    assert train._eligible(m, x, y) is None


@pytest.mark.parametrize("name,npar", [("train_tree_demo1", 6), ("train_tree_demo2", 6), ("train_tree_prod", 5), ("train_tree_nest3", 8)])
def test_train_tree_fixtures_hold_numbers_only(golden, name, npar):
    g = golden(name)
    assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in g.values())
    steps = int(g["steps"])
    assert g["trace"].shape == (steps,) and g["x"].shape[0] == g["y"].shape[0]
    assert sorted(k for k in g if k.startswith("init_")) == ["init_%d" % i for i in range(npar)]
    assert all(g["init_%d" % i].shape == g["final_%d" % i].shape for i in range(npar))
    assert float(g["twin_distance"]) <= 1e-11      # the generator's own conditioning check
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 64 * 1024
