"""The composed-kernel batched prediction call's host side, without a GPU: the export, the ctypes declaration, the signatures of the two
`forward_many_composed` functions, and which members share which library call (on fake-device tensors, as
tests/test_forward_many_host.py does)."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ffgp_predict_small_tree_batch"


def test_the_library_exports_the_entry():
    """fails before ffgp_predict_small_tree_batch: the library has no such symbol"""
    so = os.path.join(ROOT, "fidelityfusion_amd", "libffgp.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT %s\b" % NAME, out), "libffgp.so does not export %s" % NAME


def test_lib_declares_the_function():
    from fidelityfusion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ffgp.h")).read()
    assert re.search(r"\bint %s\s*\(ffgp_handle\* h, int F, const ffgp_problem\* p, const ffgp_tree_links\* links,\s*"
                     r"const ffgp_predict_member\* m,\s*int\* status\);" % NAME, hdr)
    assert NAME in _lib.EXPORTS
    fn = getattr(_lib.lib, NAME)
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(_lib.Problem), ctypes.POINTER(_lib.TreeLinks),
                                 ctypes.POINTER(_lib.PredictMember), ctypes.POINTER(ctypes.c_int)]
    # ffgp_predict_small_batch's parameter list with the tree's links in place of the single kernel's
    other = _lib.EXPORTS["ffgp_predict_small_batch"]
    assert _lib.EXPORTS[NAME][0] is other[0]
    assert [a for i, a in enumerate(_lib.EXPORTS[NAME][1]) if i != 3] == [a for i, a in enumerate(other[1]) if i != 3]


def test_both_modules_have_forward_many_composed():
    from fidelityfusion_amd import cigp_v10, gp_basic
    for mod in (cigp_v10, gp_basic):
        p = inspect.signature(mod.forward_many_composed).parameters
        assert list(p) == ["models", "xs", "ys", "x_tests", "state"], mod
        assert p["state"].default is None
        assert list(inspect.signature(mod.forward_many_composed_fused).parameters) == ["models", "xs", "ys", "x_tests"]
        # forward_many keeps its own
        assert list(inspect.signature(mod.forward_many).parameters) == ["models", "xs", "ys", "x_tests", "state"]


class _OnGpu(torch.Tensor):
    """a CPU tensor that reports itself on cuda:0: the predicate reads is_cuda, device, dtype, shape and contiguity, never the data"""
    is_cuda = property(lambda self: True)
    device = property(lambda self: torch.device("cuda:0"))


def _gpu(*shape, dtype=torch.float64):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_OnGpu)


class _Leaf:
    """an ARDKernel's `links()` and `descriptor()` on fake-device parameters: a leaf `kernel._flatten` accepts"""

    def __init__(self, D, dtype=torch.float64):
        self.w, self.amp = _gpu(D, dtype=dtype), _gpu(1, dtype=dtype)

    def links(self):
        from fidelityfusion_amd import _lib
        return {"w": self.w, "w_link": _lib.LINK_INV_ABS_EPS, "w_c": 1e-9, "amp": self.amp, "amp_link": _lib.LINK_ABS, "clamp": 1e-30, "kfun": 0}

    def descriptor(self):
        raise AssertionError("the route reads the leaves' links, never their effective values")


def _sum(D, dtype=torch.float64):
    from fidelityfusion_amd import kernel
    return kernel.SumKernel(_Leaf(D, dtype), _Leaf(D, dtype))


def _cigp(kernel_, dtype=torch.float64):
    return types.SimpleNamespace(kernel=kernel_, log_beta=_gpu(1, dtype=dtype))


def _basic(kernel_):
    return types.SimpleNamespace(kernel=kernel_, noise_variance=_gpu(1))


def test_which_members_share_which_call():
    from fidelityfusion_amd import cigp_v10, gp_basic, kernel

    def fused(m, n, D, d, nt=5, mod=cigp_v10, **kw):
        got = mod.forward_many_composed_fused([m], [_gpu(n, D, **kw)], [_gpu(n, d, **kw)], [_gpu(nt, D, **kw)])
        assert got in (([0], [0]), ([], [])), got
        return got == ([0], [0])

    assert fused(_cigp(_sum(2)), 40, 2, 1)
    assert fused(_cigp(_sum(2)), 128, 2, 1) and not fused(_cigp(_sum(2)), 129, 2, 1)      # the one-workgroup image holds 128 points
    assert fused(_cigp(_sum(2)), 40, 2, 16) and not fused(_cigp(_sum(2)), 40, 2, 17)      # ... and 16 target columns
    assert fused(_cigp(_sum(16)), 40, 16, 1) and not fused(_cigp(_sum(17)), 40, 17, 1)
    assert fused(_cigp(_sum(2)), 1, 2, 1, nt=1)
    assert not fused(_cigp(_sum(2, torch.float32), torch.float32), 40, 2, 1, dtype=torch.float32)
    assert not fused(_cigp(_sum(2, torch.float32)), 40, 2, 1)                              # fp32 leaf parameters alone
    assert not fused(_cigp(_sum(2), torch.float32), 40, 2, 1)                              # an fp32 noise parameter alone
    assert fused(_basic(_sum(2)), 40, 2, 1, mod=gp_basic)
    # a leaf with a learnable profile parameter; five leaves
    assert not fused(_cigp(kernel.SumKernel(_Leaf(2), kernel.RationalQuadraticKernel())), 40, 2, 1)
    five = kernel.SumKernel(kernel.ProductKernel(kernel.SumKernel(_Leaf(2), _Leaf(2)), _Leaf(2)), kernel.SumKernel(_Leaf(2), _Leaf(2)))
    assert not fused(_cigp(five), 40, 2, 1)
    four = kernel.SumKernel(kernel.ProductKernel(_Leaf(2), _Leaf(2)), kernel.SumKernel(_Leaf(2), _Leaf(2)))
    assert fused(_cigp(four), 40, 2, 1)
    # a length-scale vector that is neither one value nor D
    assert not fused(_cigp(kernel.SumKernel(_Leaf(3), _Leaf(2))), 40, 2, 1)
    # the test points: the model's D, the model's GPU, at least one
    one = lambda xt: cigp_v10.forward_many_composed_fused([_cigp(_sum(2))], [_gpu(40, 2)], [_gpu(40, 1)], [xt]) == ([0], [0])
    assert one(_gpu(7, 2)) and not one(_gpu(7, 3)) and not one(_gpu(0, 2)) and not one(torch.zeros(7, 2, dtype=torch.float64))
    # CPU training data
    assert cigp_v10.forward_many_composed_fused([_cigp(_sum(2))], [torch.zeros(40, 2, dtype=torch.float64)], [_gpu(40, 1)],
                                                [_gpu(5, 2)]) == ([], [])
    # cigp.forward drops y_var, so `[y, y_var]` stays in the call; GP_basic.forward adds the full matrix, so it leaves it
    ylist = [_gpu(40, 1), _gpu(40, 40)]
    assert cigp_v10.forward_many_composed_fused([_cigp(_sum(2))], [_gpu(40, 2)], [ylist], [_gpu(5, 2)]) == ([0], [0])
    assert gp_basic.forward_many_composed_fused([_basic(_sum(2)), _basic(_sum(2))], [_gpu(40, 2)] * 2, [ylist, _gpu(40, 1)],
                                                [_gpu(5, 2)] * 2) == ([1], [1])


def test_a_mixed_call_gives_each_kind_its_own_list_in_the_callers_order():
    from fidelityfusion_amd import cigp_v10
    radial = lambda D: types.SimpleNamespace(kernel=_Leaf(D), log_beta=_gpu(1))      # (a single kernel with `links()`: forward_many's route)
    models = [_cigp(_sum(2)), radial(2), _cigp(_sum(2)), radial(3), _cigp(_sum(3)), radial(2)]
    xs = [_gpu(20, 2), _gpu(129, 2), _gpu(129, 2), _gpu(64, 3), _gpu(30, 3), _gpu(30, 2)]
    ys = [_gpu(20, 1), _gpu(129, 1), _gpu(129, 1), _gpu(64, 1), _gpu(30, 2), _gpu(30, 2)]
    xts = [_gpu(9, 2), _gpu(9, 2), _gpu(9, 2), _gpu(40, 3), _gpu(9, 3), _gpu(9, 2)]
    assert cigp_v10.forward_many_composed_fused(models, xs, ys, xts) == ([0, 3, 4, 5], [0, 4])
    # forward_many on the same call still leaves every composed member out
    assert cigp_v10.forward_many_fused(models, xs, ys, xts) == [3, 5]
