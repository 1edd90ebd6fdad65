"""Build-time check of the composed-kernel acquisition optimiser's kernel (csrc/acq_tree.hip; no GPU needed: hipcc cross-compiles):
every instantiation runs entirely in registers -- no private (scratch) segment, no spills -- fits a 256-thread workgroup on a CU and
takes its LDS dynamically, sized from n by the host.  Metadata only (the `amdhsa.kernels` block)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tree_kernels():
    """{kernel name: its metadata block (amdhsa.kernels) as a dict of the integer fields}"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from check_isa import device_asm
    asm = device_asm("acq_tree.hip")
    ks = asm[asm.index("amdhsa.kernels:"):]
    out = {}
    for blk in re.split(r"\n  - ", ks)[1:]:
        m = re.search(r"\.name:\s+(\S+)", blk)
        if m and "ffgp_tree_acq_kernel" in m.group(1):
            out[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.([a-z_]+):\s+(\d+)\n", blk)}
    return out


def test_tree_acq_kernel_has_its_three_instantiations(tree_kernels):
    assert len(tree_kernels) == 3, sorted(tree_kernels)      # D <= 2, D <= 8, D <= 16; the leaf count is a run-time argument
    assert not any("ffgp_acq_kernel" in name for name in tree_kernels)      # (test_acq_isa.py counts that substring in acq.hip)


def test_tree_acq_kernel_uses_no_scratch(tree_kernels):
    assert tree_kernels
    for name, meta in tree_kernels.items():
        print(name, {k: meta[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count")})
        assert meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_spill_count"] == 0, (name, meta)


def test_tree_acq_kernel_fits_a_256_thread_workgroup(tree_kernels):
    """a SIMD has 512 VGPRs per lane and the workgroup's four waves sit one per SIMD, so any unified count (`vgpr_count`: arch + acc)
    up to 512 runs -- and 256 threads are what the kernel is launched with"""
    assert tree_kernels
    for name, meta in tree_kernels.items():
        assert meta["max_flat_workgroup_size"] == 256, (name, meta)
        assert meta["agpr_count"] <= meta["vgpr_count"] <= 512, (name, meta)
        assert meta["group_segment_fixed_size"] == 0, (name, meta)      # dynamic LDS only, sized from n by the host
