"""Build-time check of the one-workgroup LDS eigensolver (csrc/eig_lds.hip; no GPU needed: hipcc cross-compiles): its kernel runs
entirely in registers and LDS -- no private (scratch) segment, no vector register spilled, in each of its five instantiations
(4 .. 8 rows of a column per lane) -- and its static LDS plus the dynamic request of the largest problem (n = 128: one [128][129]
fp64 image and the waves' partial Rayleigh quotients) fits the CU's 160 KiB.  Metadata only, as test_acq_isa.py."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def lds_kernels():
    """{kernel name: its metadata block (amdhsa.kernels) as a dict of the integer fields}"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from check_isa import device_asm
    asm = device_asm("eig_lds.hip")
    ks = asm[asm.index("amdhsa.kernels:"):]
    out = {}
    for blk in re.split(r"\n  - ", ks)[1:]:
        m = re.search(r"\.name:\s+(\S+)", blk)
        if m:
            out[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.([a-z_]+):\s+(\d+)\n", blk)}
    return out


def _dynamic_lds_bytes(n):
    """the host's request (el_lds_bytes in eig_lds.hip): the image [n][16 rows + 1] and one row of n partial sums per wave"""
    threads = 1024 if n > 64 else 512 if n > 32 else 256
    rows = (n + 15) // 16 if n > 64 else 4
    return (n * (16 * rows + 1) + (threads // 64) * n) * 8


def test_eig_lds_has_its_five_instantiations(lds_kernels):
    assert len(lds_kernels) == 5 and all("ffgp_syev_lds_kernel" in name for name in lds_kernels), sorted(lds_kernels)


def test_eig_lds_kernel_uses_no_scratch(lds_kernels):
    for name, meta in lds_kernels.items():
        assert meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_spill_count"] == 0, (name, meta)
        assert meta["agpr_count"] <= meta["vgpr_count"] <= 512, (name, meta)


def test_eig_lds_kernel_fits_the_cu_lds_at_128(lds_kernels):
    src = open(os.path.join(ROOT, "fidelityfusion_amd", "csrc", "eig_lds.hip")).read()
    assert "n * el_ld(n) + (size_t)(el_threads(n) / 64) * n) * sizeof(double)" in src      # the formula restated above
    assert "return n > 64 ? 1024 : n > 32 ? 512 : 256;" in src and "return EL_GROUP * el_rows(n) + 1;" in src
    assert "return n > 64 ? (n + EL_GROUP - 1) / EL_GROUP : 4;" in src and "#define EL_GROUP 16" in src
    for name, meta in lds_kernels.items():
        assert meta["max_flat_workgroup_size"] == 1024, (name, meta)
        assert meta["group_segment_fixed_size"] + _dynamic_lds_bytes(128) <= LDS_PER_CU, (name, meta)
        assert _dynamic_lds_bytes(65) < _dynamic_lds_bytes(128) // 2      # sized from n: a small matrix does not claim the CU
