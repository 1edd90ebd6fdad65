"""Build-time check of the chain acquisition optimiser's kernel (csrc/acq_chain.hip; no GPU needed: hipcc cross-compiles): every
instantiation runs entirely in registers -- no private (scratch) segment, no vector register spilled -- with the point's coordinates
and one running gradient partial (2 DM doubles) beside the block chains' operands.  (Scalar registers parked in vector lanes, which
every acquisition kernel has, cost no memory and are not counted here.)  Metadata only, as test_acq_stack_isa.py."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def chain_kernels():
    """{kernel name: its metadata block (amdhsa.kernels) as a dict of the integer fields}"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from check_isa import device_asm
    asm = device_asm("acq_chain.hip")
    ks = asm[asm.index("amdhsa.kernels:"):]
    out = {}
    for blk in re.split(r"\n  - ", ks)[1:]:
        m = re.search(r"\.name:\s+(\S+)", blk)
        if m and "ffgp_chain_acq_kernel" in m.group(1):
            out[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.([a-z_]+):\s+(\d+)\n", blk)}
    return out


def test_chain_kernel_has_its_three_instantiations(chain_kernels):
    assert len(chain_kernels) == 3, sorted(chain_kernels)      # D + 1 <= 2, D + 1 <= 8, D + 1 <= 16
    assert not any("ffgp_acq_kernel" in name for name in chain_kernels)      # test_acq_isa.py counts those


def test_chain_kernel_uses_no_scratch(chain_kernels):
    for name, meta in chain_kernels.items():
        assert meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_spill_count"] == 0, (name, meta)


def test_chain_kernel_fits_a_256_thread_workgroup(chain_kernels):
    """a SIMD has 512 VGPRs per lane and the workgroup's four waves sit one per SIMD, so any unified count up to 512 runs"""
    for name, meta in chain_kernels.items():
        assert meta["max_flat_workgroup_size"] == 256, (name, meta)
        assert meta["agpr_count"] <= meta["vgpr_count"] <= 512, (name, meta)
        assert meta["group_segment_fixed_size"] == 0, (name, meta)      # dynamic LDS only, sized from the largest member by the host
