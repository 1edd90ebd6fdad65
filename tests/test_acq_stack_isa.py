"""Build-time check of the stack acquisition optimiser's kernel (csrc/acq_stack.hip; no GPU needed: hipcc cross-compiles): every
instantiation runs entirely in registers -- no private (scratch) segment, no vector register spilled -- although it carries two
running gradient partials (2 DM doubles) on top of the single-posterior kernel's registers.  (Scalar registers parked in vector
lanes, which both acquisition kernels have, cost no memory and are not counted here.)  Metadata only, as test_acq_isa.py."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def stack_kernels():
    """{kernel name: its metadata block (amdhsa.kernels) as a dict of the integer fields}"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from check_isa import device_asm
    asm = device_asm("acq_stack.hip")
    ks = asm[asm.index("amdhsa.kernels:"):]
    out = {}
    for blk in re.split(r"\n  - ", ks)[1:]:
        m = re.search(r"\.name:\s+(\S+)", blk)
        if m and "ffgp_stack_acq_kernel" in m.group(1):
            out[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.([a-z_]+):\s+(\d+)\n", blk)}
    return out


def test_stack_kernel_has_its_three_instantiations(stack_kernels):
    assert len(stack_kernels) == 3, sorted(stack_kernels)      # D <= 2, D <= 8, D <= 16
    assert not any("ffgp_acq_kernel" in name for name in stack_kernels)      # test_acq_isa.py counts those


def test_stack_kernel_uses_no_scratch(stack_kernels):
    for name, meta in stack_kernels.items():
        assert meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_spill_count"] == 0, (name, meta)


def test_stack_kernel_fits_a_256_thread_workgroup(stack_kernels):
    """a SIMD has 512 VGPRs per lane and the workgroup's four waves sit one per SIMD, so any unified count up to 512 runs"""
    for name, meta in stack_kernels.items():
        assert meta["max_flat_workgroup_size"] == 256, (name, meta)
        assert meta["agpr_count"] <= meta["vgpr_count"] <= 512, (name, meta)
        assert meta["group_segment_fixed_size"] == 0, (name, meta)      # dynamic LDS only, sized from the largest member by the host
