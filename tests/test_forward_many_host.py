"""The batched prediction call's host side, without a GPU: the export, the ctypes declaration, the limits in the header against the
Python constants, the signatures of the two `forward_many` functions, and which members share the library call (on fake-device
tensors, as tests/test_acq_staged_host.py does)."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ffgp_predict_small_batch"


def test_the_library_exports_the_entry():
    so = os.path.join(ROOT, "fidelityfusion_amd", "libffgp.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT %s\b" % NAME, out), "libffgp.so does not export %s" % NAME


def test_lib_declares_the_function_and_the_member_struct():
    from fidelityfusion_amd import _lib
    fn = getattr(_lib.lib, NAME)
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(_lib.Problem), ctypes.POINTER(_lib.Links),
                                 ctypes.POINTER(_lib.PredictMember), ctypes.POINTER(ctypes.c_int)]
    assert [f[0] for f in _lib.PredictMember._fields_] == ["Xs_dev", "nt", "mean_dev", "var_dev", "var_add_noise"]
    # the header's struct, field for field: pointer, int, pointer, pointer, int -> 40 bytes with the C compiler's padding
    assert ctypes.sizeof(_lib.PredictMember) == 40 and _lib.PredictMember.mean_dev.offset == 16
    assert NAME in _lib.EXPORTS


def test_the_limits_in_the_header_are_the_python_constants():
    from fidelityfusion_amd import _lib
    from fidelityfusion_amd import functional as F
    src = open(os.path.join(ROOT, "include", "ffgp.h")).read()
    for key in ("N", "D", "d", "F"):
        m = re.search(r"^#define FFGP_PREDICT_SMALL_MAX_%s (\d+)\b" % key, src, flags=re.M)
        assert m and int(m.group(1)) == getattr(_lib, "FFGP_PREDICT_SMALL_MAX_" + key), key
    assert (_lib.FFGP_PREDICT_SMALL_MAX_N, _lib.FFGP_PREDICT_SMALL_MAX_D, _lib.FFGP_PREDICT_SMALL_MAX_d) == (128, 16, 16)
    assert _lib.FFGP_PREDICT_SMALL_MAX_F >= 64
    # ... which are the limits `raw_many_ok` routes the small batch by
    assert (F.SMALL_BATCH_MAX_N, F.SMALL_BATCH_MAX_D, F.SMALL_BATCH_MAX_d) == (128, 16, 16)
    assert re.search(r"typedef struct ffgp_predict_member \{[^}]*const double\* Xs_dev; int nt;[^}]*double\* mean_dev;[^}]*double\* var_dev;"
                     r"[^}]*int var_add_noise;[^}]*\} ffgp_predict_member;", src, flags=re.S)


def test_both_modules_have_forward_many():
    from fidelityfusion_amd import cigp_v10, gp_basic
    for mod in (cigp_v10, gp_basic):
        p = inspect.signature(mod.forward_many).parameters
        assert list(p) == ["models", "xs", "ys", "x_tests", "state"], mod
        assert p["state"].default is None
        assert list(inspect.signature(mod.forward_many_fused).parameters) == ["models", "xs", "ys", "x_tests"]


class _OnGpu(torch.Tensor):
    """a CPU tensor that reports itself on cuda:0: the predicate reads is_cuda, device, dtype, shape and contiguity, never the data"""
    is_cuda = property(lambda self: True)
    device = property(lambda self: torch.device("cuda:0"))


def _gpu(*shape, dtype=torch.float64):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_OnGpu)


class _Kernel:
    """an ARDKernel's `links()` on fake-device parameters"""

    def __init__(self, D, kparam=None):
        self.D, self.kparam = D, kparam

    def links(self):
        from fidelityfusion_amd import _lib
        lk = {"w": _gpu(self.D), "w_link": _lib.LINK_INV_ABS_EPS, "w_c": 1e-9, "amp": _gpu(1), "amp_link": _lib.LINK_ABS, "clamp": 1e-30,
              "kfun": 0}
        if self.kparam is not None:
            lk["kparam"] = self.kparam
        return lk


def _cigp(D, kernel=None):
    return types.SimpleNamespace(kernel=kernel or _Kernel(D), log_beta=_gpu(1))


def _basic(D, kernel=None):
    return types.SimpleNamespace(kernel=kernel or _Kernel(D), noise_variance=_gpu(1))


def test_which_members_share_the_call():
    from fidelityfusion_amd import cigp_v10, gp_basic, kernel
    fused = lambda m, n, D, d, nt=5, **kw: cigp_v10.forward_many_fused([m], [_gpu(n, D, **kw)], [_gpu(n, d, **kw)], [_gpu(nt, D, **kw)]) == [0]
    assert fused(_cigp(2), 40, 2, 1)
    assert fused(_cigp(2), 128, 2, 1) and not fused(_cigp(2), 129, 2, 1)      # the one-workgroup image holds 128 points
    assert fused(_cigp(2), 40, 2, 16) and not fused(_cigp(2), 40, 2, 17)      # ... and 16 target columns
    assert fused(_cigp(16), 40, 16, 1) and not fused(_cigp(17), 40, 17, 1)
    assert fused(_cigp(2), 1, 2, 1, nt=1)
    assert not fused(_cigp(2), 40, 2, 1, dtype=torch.float32)
    assert not fused(_cigp(2, kernel.SumKernel(kernel.ARDKernel(2), kernel.ARDKernel(2))), 40, 2, 1)      # a composed kernel
    assert not fused(_cigp(2, kernel.RationalQuadraticKernel()), 40, 2, 1)                                # a learnable profile parameter
    assert not fused(_cigp(2, _Kernel(2, kparam=_gpu(1))), 40, 2, 1)
    assert fused(_cigp(2, _Kernel(2, kparam=1.5)), 40, 2, 1)                                              # Matern's constant rho
    # the test points: the model's D, the model's GPU, at least one
    one = lambda xt: cigp_v10.forward_many_fused([_cigp(2)], [_gpu(40, 2)], [_gpu(40, 1)], [xt]) == [0]
    assert one(_gpu(7, 2)) and not one(_gpu(7, 3)) and not one(_gpu(0, 2)) and not one(torch.zeros(7, 2, dtype=torch.float64))
    # CPU training data
    assert cigp_v10.forward_many_fused([_cigp(2)], [torch.zeros(40, 2, dtype=torch.float64)], [_gpu(40, 1)], [_gpu(5, 2)]) == []
    # cigp.forward drops y_var, so `[y, y_var]` stays in the call; GP_basic.forward adds the full matrix, so it leaves it
    ylist = [_gpu(40, 1), _gpu(40, 40)]
    assert cigp_v10.forward_many_fused([_cigp(2)], [_gpu(40, 2)], [ylist], [_gpu(5, 2)]) == [0]
    assert gp_basic.forward_many_fused([_basic(2), _basic(2)], [_gpu(40, 2)] * 2, [ylist, _gpu(40, 1)], [_gpu(5, 2)] * 2) == [1]
    # a FidelityKernelMCMC has no links of its own: its member runs its own forward
    fk = kernel.FidelityKernelMCMC(1, kernel.ARDKernel(2), 0.0, 1.0, torch.tensor(1.0))
    assert gp_basic.forward_many_fused([_basic(2, fk)], [_gpu(40, 2)], [_gpu(40, 1)], [_gpu(5, 2)]) == []
    # a mixed call keeps the caller's order
    models = [_cigp(2), _cigp(2), _cigp(3), _cigp(2, kernel.SumKernel(kernel.ARDKernel(2), kernel.ARDKernel(2)))]
    xs = [_gpu(129, 2), _gpu(30, 2), _gpu(64, 3), _gpu(20, 2)]
    ys = [_gpu(129, 1), _gpu(30, 2), _gpu(64, 1), _gpu(20, 1)]
    xts = [_gpu(9, 2), _gpu(9, 2), _gpu(40, 3), _gpu(9, 2)]
    assert cigp_v10.forward_many_fused(models, xs, ys, xts) == [1, 2]
