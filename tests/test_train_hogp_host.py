"""Host-side checks of `hogp_simple.train_many` (no GPU needed): the eligibility rules of the fused route on CPU tensors, the
argument checking, the layout of the Adam state, and the declaration, export and binding of ffgp_train_hogp_raw."""
import os
import re
import subprocess

import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def on_host(monkeypatch):
    """the residency test of the raw-parameter path (`raw_ok`: one GPU) replaced by its dtype / layout half, so that the REST of the
    eligibility rules can be exercised on CPU tensors"""
    from fidelityfusion_amd import functional, nlml

    def ok(*ts):
        ts = [t for t in ts if t is not None]
        return bool(ts) and all(isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.is_contiguous() for t in ts)

    monkeypatch.setattr(nlml, "raw_ok", ok)
    monkeypatch.setattr(functional, "raw_ok", ok)


def _block(k=None, shape=(4, 3), **kw):
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.hogp_simple import HOGP_simple
    return HOGP_simple(k if k is not None else kernel.ARDKernel(2), 0.5, shape, **kw).double()


def test_eligibility_rules(on_host):
    from fidelityfusion_amd import _lib, kernel
    from fidelityfusion_amd import hogp_simple as H
    from fidelityfusion_amd.gp_computation_pack import Tensor_linear
    x, y = torch.rand(9, 2, dtype=torch.float64), torch.rand(9, 4, 3, dtype=torch.float64)
    m = _block()
    e = H._train_eligible(m, x, y, None)
    assert e is not None and e["dims"] == (4, 3) and e["y"] is y and e["V"] is None
    assert e["lk"]["w"] is m.kernel_list[0].length_scales and e["lk"]["w_link"] == _lib.LINK_INV_ABS_EPS
    assert H._train_eligible(m, x, [y, torch.rand(9, 9, dtype=torch.float64)], None)["y"] is y      # the mean of a [mean, var] list
    for kk in (kernel.SquaredExponentialKernel(), kernel.MaternKernel(2, nu=2.5)):
        assert H._train_eligible(_block(kk), x, y, None) is not None
    # learnable grids or maps, composed kernels, a learnable profile parameter, frozen parameters: the reference's loop
    assert H._train_eligible(_block(learnable_map=True), x, y, None) is None
    assert H._train_eligible(_block(learnable_grid=True), x, y, None) is None
    assert H._train_eligible(_block(kernel.SumKernel(kernel.ARDKernel(2), kernel.MaternKernel(2))), x, y, None) is None
    assert H._train_eligible(_block(kernel.RationalQuadraticKernel()), x, y, None) is None
    assert H._train_eligible(_block(kernel.LinearKernel(2)), x, y, None) is None
    frozen = _block()
    frozen.noise_variance.requires_grad_(False)
    assert H._train_eligible(frozen, x, y, None) is None
    # sizes: n <= 128, 1-3 modes of at most 64, targets of the block's own shape, fp64
    assert H._train_eligible(m, torch.rand(129, 2, dtype=torch.float64), torch.rand(129, 4, 3, dtype=torch.float64), None) is None
    assert H._train_eligible(_block(shape=(65,)), x, torch.rand(9, 65, dtype=torch.float64), None) is None
    assert H._train_eligible(_block(shape=(2, 2, 2, 2)), x, torch.rand(9, 2, 2, 2, 2, dtype=torch.float64), None) is None
    assert H._train_eligible(_block(shape=(64,)), x, torch.rand(9, 64, dtype=torch.float64), None) is not None
    # ... and a product of at most 4096: (16, 16, 17) has every mode within 64 and 4352 outputs
    assert H._train_eligible(_block(shape=(16, 16, 17)), x, torch.rand(9, 16, 16, 17, dtype=torch.float64), None) is None
    assert H._train_eligible(_block(shape=(16, 16, 16)), x, torch.rand(9, 16, 16, 16, dtype=torch.float64), None) is not None
    # frozen grids and maps must still hold 0..d-1 and the identity: the call forms the mode inputs itself
    moved = _block()
    with torch.no_grad():
        moved.grid[1].mul_(0.5)
    assert H._train_eligible(moved, x, y, None) is None
    mapped = _block()
    with torch.no_grad():
        mapped.mapping_vector[0][0, 1] = 0.25
    assert H._train_eligible(mapped, x, y, None) is None
    assert H._train_eligible(m, x, torch.rand(9, 3, 4, dtype=torch.float64), None) is None
    assert H._train_eligible(m, x, y.float(), None) is None
    assert H._train_eligible(object(), x, y, None) is None
    # residual blocks: the Tensor_linear's LAST matrix is the parameter, y_low is coarser (or equal) in the last mode only
    tl = Tensor_linear((4, 2), (4, 3)).double()
    yl = torch.rand(9, 4, 2, dtype=torch.float64)
    e = H._train_eligible(m, x, None, (tl, [yl, None], y))
    assert e is not None and e["V"] is tl.vectors[1] and tuple(e["V"].shape) == (3, 2) and e["yl"] is yl and e["yh"] is y
    assert e["V"].stride() == (1, 3)      # the bilinear initialisation is a transposed view: the call takes V with its strides
    assert H._train_eligible(m, x, None, (tl, torch.rand(9, 4, 3, dtype=torch.float64), y)) is None
    assert H._train_eligible(m, x, None, (Tensor_linear((2,), (3,)).double(), yl, y)) is None
    tl.vectors[1].requires_grad_(False)
    assert H._train_eligible(m, x, None, (tl, yl, y)) is None


def test_cpu_tensors_are_not_eligible():
    from fidelityfusion_amd import hogp_simple as H
    assert H._train_eligible(_block(), torch.rand(9, 2, dtype=torch.float64), torch.rand(9, 4, 3, dtype=torch.float64), None) is None


def test_argument_checking():
    from fidelityfusion_amd import hogp_simple as H
    m = _block()
    x, y = torch.rand(9, 2, dtype=torch.float64), torch.rand(9, 4, 3, dtype=torch.float64)
    with pytest.raises(ValueError):
        H.train_many([m], [x, x], [y], 2)
    with pytest.raises(ValueError):
        H.train_many([m], [x], [y], 0)
    with pytest.raises(ValueError):
        H.train_many([m], [x], [None], 2)                                   # neither targets nor a residual link
    with pytest.raises(ValueError):
        H.train_many([m], [x], [y], 2, residual=[(None, y, y)])             # a residual model takes ys[f] = None
    with pytest.raises(ValueError):
        H.train_many([m], [x], [None], 2, residual=[(None, y)])
    with pytest.raises(ValueError):
        H.train_many([m], [x], [y], 2, residual=[None, None])
    with pytest.raises(ValueError):
        H.train_many([m], [x], [y], 2, state=H.HOGPTrainState(False, 3))    # a state of another list of models


def test_state_layout():
    """[exp_avg (P) | exp_avg_sq (P)] per row, whatever the row's stride"""
    from fidelityfusion_amd import hogp_simple as H
    st = H.HOGPTrainState(True, 2)
    st.buf = torch.arange(2 * 12, dtype=torch.float64).reshape(2, 12)
    st.npar = [4, 6]
    ea, es = st.moments(0)
    assert ea.tolist() == [0, 1, 2, 3] and es.tolist() == [4, 5, 6, 7]
    ea, es = st.moments(1)
    assert ea.tolist() == [12, 13, 14, 15, 16, 17] and es.tolist() == [18, 19, 20, 21, 22, 23]
    assert st.steps == [0, 0] and st.failed == {} and st.fused is True


def test_export_is_declared_exported_and_bound():
    import ctypes as C
    from fidelityfusion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ffgp.h")).read()
    assert re.search(r"\bint ffgp_train_hogp_raw\s*\(", hdr)
    for s in ("ffgp_hogp_model", "ffgp_hogp_residual", "ffgp_hogp_cache"):
        assert re.search(r"\}\s*%s;" % s, hdr), s
    assert "ffgp_train_hogp_raw" in _lib.EXPORTS
    so = os.path.join(ROOT, "fidelityfusion_amd", "libffgp.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT ffgp_train_hogp_raw\b", syms)
    # the structs as the header lays them out
    assert C.sizeof(_lib.HogpModel) == 88 and _lib.HogpModel.dims.offset == 20 and _lib.HogpModel.Y_dev.offset == 32
    assert _lib.HogpModel.kparam.offset == 80
    assert C.sizeof(_lib.HogpResidual) == 48 and _lib.HogpResidual.l.offset == 24 and _lib.HogpResidual.V_col_stride.offset == 40
    assert C.sizeof(_lib.HogpCache) == 14 * 8 and _lib.HogpCache.A_dev.offset == 12 * 8
    assert "train_hogp.hip" in open(os.path.join(ROOT, "fidelityfusion_amd", "csrc", "Makefile")).read()
