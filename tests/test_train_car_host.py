"""Build-time and host-side checks of train_many's GP_basic / CAR routes (no GPU needed): `kernel.FidelityKernelMCMC.car_links()`, the
eligibility rules of `train._eligible` / `train._eligible_car`, the declaration, export and binding of ffgp_train_car_raw, the register
and LDS budgets of the new one-launch kernels of csrc/train.hip, and the closed forms of the fidelity integral s and its three partials
(include/ffgp.h, ffgp_car_link) against autograd on the reference's expression."""
import os
import re
import subprocess

import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


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


def _car_model(base=None, input_dim=1, b0=1.0, dtype=torch.float64):
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.gp_basic import GP_basic
    b = torch.nn.Parameter(torch.tensor(b0))
    k = kernel.FidelityKernelMCMC(input_dim, base if base is not None else kernel.ARDKernel(1), 1, 2, b)
    return GP_basic(k, 0.7).to(dtype), b


def test_car_links_fields_and_reference_draws():
    from fidelityfusion_amd import _lib, kernel
    assert kernel.fidelity_kernel_MCMC is kernel.FidelityKernelMCMC
    m, b = _car_model()
    k = m.kernel
    torch.manual_seed(3)
    cl = k.car_links()
    after = torch.rand(1)
    assert cl["b"] is b and cl["l_z"] is k.length_scales and cl["sigma_z"] is k.signal_variance
    assert (cl["eps"], cl["lf"], cl["hf"]) == (1e-3, 1.0, 2.0)
    assert cl["base"]["w"] is k.kernel1.length_scales and cl["base"]["amp"] is k.kernel1.signal_variance
    assert cl["base"]["w_link"] == _lib.LINK_INV_ABS_EPS and cl["base"]["amp_link"] == _lib.LINK_ABS
    # the reference's draws (CAR_ContinuousAutoRegression.py:56-59), and the generator left where one reference step leaves it
    torch.manual_seed(105)
    z1 = torch.rand(100) * (2 - 1) + 1
    z2 = torch.rand(100) * (2 - 1) + 1
    assert cl["z1"].dtype == torch.float32 and torch.equal(cl["z1"], z1) and torch.equal(cl["z2"], z2)
    assert torch.equal(after, torch.rand(1))
    # a base kernel without links (a composition, RationalQuadraticKernel): no base links
    assert _car_model(kernel.SumKernel(kernel.ARDKernel(1), kernel.MaternKernel(1)))[0].kernel.car_links()["base"] is None
    assert _car_model(kernel.RationalQuadraticKernel())[0].kernel.car_links()["base"] is None


def test_fidelity_kernel_is_the_harness_module():
    """scale(), effective, kfun and forward as in tests/mf_harness.py"""
    import mf_harness as H
    from fidelityfusion_amd import kernel
    b = torch.nn.Parameter(torch.tensor(0.7, dtype=torch.float64))
    a = kernel.FidelityKernelMCMC(1, kernel.MaternKernel(1), 0, 1, b).double()
    h = H.fidelity_kernel_MCMC(1, kernel.MaternKernel(1), 0, 1, b).double()
    with torch.no_grad():
        for q in (a, h):
            q.length_scales.fill_(-0.8)
            q.signal_variance.fill_(-1.3)
    assert torch.equal(a.scale(), h.scale()) and a.kfun() == h.kfun()
    wa, aa, ca = a.effective()
    wh, ah, ch = h.effective()
    assert torch.equal(wa, wh) and torch.equal(aa, ah) and ca == ch
    assert [n for n, _ in a.named_parameters()] == [n for n, _ in h.named_parameters()]


def test_eligibility_rules(on_host, f64):
    from fidelityfusion_amd import _lib, kernel, train
    from fidelityfusion_amd.gp_basic import GP_basic
    x, y = torch.rand(9, 1), torch.rand(9, 2)
    m = GP_basic(kernel.MaternKernel(1), 0.5).double()
    e = train._eligible(m, x, y)
    assert e is not None and e[0]["diag"][0] is m.noise_variance and e[0]["diag"][1:] == (_lib.LINK_SQUARE, 0.0)
    assert e[0]["ll"][0] == _lib.FFGP_LL_V2 and abs(e[0]["ll"][1] - 3.141592653589793) == 0.0
    assert train._eligible(m, x, [y, torch.eye(9)]) is None                                  # the FULL y_var matrix enters Sigma
    assert train._eligible(GP_basic(kernel.SumKernel(kernel.ARDKernel(1), kernel.MaternKernel(1)), 0.5).double(), x, y) is None
    assert train._eligible(GP_basic(kernel.RationalQuadraticKernel(), 0.5).double(), x, y) is None
    frozen = GP_basic(kernel.ARDKernel(1), 0.5).double()
    frozen.noise_variance.requires_grad_(False)
    assert train._eligible(frozen, x, y) is None
    # CAR members
    yl, yh = torch.rand(9, 2), torch.rand(9, 2)
    cm, b = _car_model()
    e = train._eligible_car(cm, x, (b, yl, yh))
    assert e is not None and e[0]["car"]["b"] is b and e[1] is yh and e[0]["ll"][0] == _lib.FFGP_LL_V2
    for base in (kernel.SumKernel(kernel.ARDKernel(1), kernel.MaternKernel(1)), kernel.RationalQuadraticKernel()):
        cm2, b2 = _car_model(base)
        assert train._eligible_car(cm2, x, (b2, yl, yh)) is None
    cm3, b3 = _car_model(kernel.ARDKernel(2), input_dim=2)                                   # l_z with several elements
    assert train._eligible_car(cm3, torch.rand(9, 2), (b3, yl, yh)) is None


def test_cpu_tensors_are_not_eligible(f64):
    from fidelityfusion_amd import kernel, train
    from fidelityfusion_amd.gp_basic import GP_basic
    x, y = torch.rand(9, 1), torch.rand(9, 2)
    assert train._eligible(GP_basic(kernel.ARDKernel(1), 0.5).double(), x, y) is None
    cm, b = _car_model()
    assert train._eligible_car(cm, x, (b, y, y.clone())) is None


def test_car_and_residual_on_one_model_raise(f64):
    from fidelityfusion_amd import train
    cm, b = _car_model()
    x, yl, yh = torch.rand(9, 1), torch.rand(9, 1), torch.rand(9, 1)
    rho = torch.nn.Parameter(torch.tensor(1.0))
    with pytest.raises(ValueError):
        train.train_many([cm], [x], [None], 2, car=[(b, yl, yh)], residual=[(rho, yl, yh)])
    other = torch.nn.Parameter(torch.tensor(1.0))
    with pytest.raises(ValueError):      # the kernel's b must be the tensor given
        train.train_many([cm], [x], [None], 2, car=[(other, yl, yh)])


def test_car_export_is_declared_exported_and_bound():
    import ctypes as C
    from fidelityfusion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ffgp.h")).read()
    assert re.search(r"\bint ffgp_train_car_raw\s*\(", hdr) and re.search(r"\}\s*ffgp_car_link;", hdr)
    assert "ffgp_train_car_raw" in _lib.EXPORTS
    so = os.path.join(ROOT, "fidelityfusion_amd", "libffgp.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT ffgp_train_car_raw\b", syms)
    assert _lib.lib.ffgp_train_car_raw is not None
    # the struct as the header lays it out: three pointers, zeps, two pointers, nz (padded), lf, hf, three pointers, the fp64 draws
    assert C.sizeof(_lib.CarLink) == 14 * 8 and _lib.CarLink.lf.offset == 7 * 8 and _lib.CarLink.b_last_dev.offset == 11 * 8
    # ffgp_residual's layout is untouched
    assert C.sizeof(_lib.Residual) == 8 * 8


def _meta(asm, name):
    ks = asm[asm.index("amdhsa.kernels:"):]
    for blk in re.split(r"\n  - ", ks)[1:]:
        m = re.search(r"\.name:\s+(\S+)", blk)
        if m and name in m.group(1):
            return {k: int(v) for k, v in re.findall(r"\.([a-z_]+):\s+(\d+)\n", blk)}
    raise AssertionError("kernel %s not found" % name)


def test_new_trainer_instantiations_fit_registers_and_lds():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from check_isa import device_asm
    asm = device_asm("train.hip")
    plain16 = _meta(asm, "ffgp_train_persist_kernelILi16E")
    for name in ("ffgp_train_v2_kernelILi8E", "ffgp_train_v2_kernelILi16E", "ffgp_train_car_kernelILi8ELb0E", "ffgp_train_car_kernelILi16ELb0E",
                 "ffgp_train_car_kernelILi8ELb1E", "ffgp_train_car_kernelILi16ELb1E"):
        m = _meta(asm, name)
        assert m["private_segment_fixed_size"] <= plain16["private_segment_fixed_size"], (name, m["private_segment_fixed_size"])
        assert m["group_segment_fixed_size"] <= 163840, name
    # the dynamic LDS the launches ask for (the layouts' static_asserts in train.hip guard the same bound at build time)
    src = open(os.path.join(ROOT, "fidelityfusion_amd", "csrc", "train.hip")).read()
    assert "static_assert(TR_LDS_DOUBLES_CAR * sizeof(double) <= 160 * 1024" in src


def _closed_forms(b, lz, sz, z1, z2, lf, hf, eps):
    """include/ffgp.h (ffgp_car_link): s and ds/db, ds/dl_z, ds/dsigma_z, everything in fp64"""
    sgn = lambda v: (v > 0) * 1.0 - (v < 0) * 1.0
    l = abs(lz) + eps
    w2 = (hf - lf) ** 2
    e = -b * (z1 - hf) - b * (z2 - hf) - 0.5 * ((z1 - z2) / l) ** 2
    ex = e.exp()
    m = ex.mean()
    s = abs(sz) * m * w2
    ds_db = -abs(sz) * w2 * (ex * ((z1 - hf) + (z2 - hf))).mean()
    ds_dl = abs(sz) * w2 * sgn(lz) * (ex * (z1 - z2) ** 2).mean() / l ** 3
    ds_ds = sgn(sz) * m * w2
    return s, ds_db, ds_dl, ds_ds


@pytest.mark.parametrize("b0,lz0,sz0", [(1.0, 1.0, 1.0), (-0.4, -0.8, 1.3), (1.0, 0.6, -0.7), (-0.4, -1.7, -2.1)])
def test_closed_forms_of_the_fidelity_integral(f64, b0, lz0, sz0):
    """value and three partials against autograd on the reference's expression (fp64 draws: nothing is binary32 then)"""
    from fidelityfusion_amd import kernel
    b = torch.nn.Parameter(torch.tensor(b0))
    k = kernel.FidelityKernelMCMC(1, kernel.ARDKernel(1), 1, 2, b)
    with torch.no_grad():
        k.length_scales.fill_(lz0)
        k.signal_variance.fill_(sz0)
    s = k.scale()
    s.sum().backward()
    z1, z2 = k.samples()
    assert z1.dtype == torch.float64
    got = _closed_forms(b0, lz0, sz0, z1, z2, 1.0, 2.0, k.eps)
    want = (s.detach().reshape(()), b.grad, k.length_scales.grad.reshape(()), k.signal_variance.grad.reshape(()))
    for g, w in zip(got, want):
        assert abs(float(g) - float(w)) <= 1e-12 * abs(float(w)), (float(g), float(w))
