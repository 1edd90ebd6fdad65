"""Build-time check of the four acquisition optimisers' kernels (csrc/acq.hip, acq_stack.hip, acq_tree.hip, acq_chain.hip; no GPU
needed: hipcc cross-compiles): every instantiation runs entirely in registers -- no private (scratch) segment, no vector register
spilled -- fits a 256-thread workgroup on a CU and takes its LDS dynamically, sized from n by the host.  The stack kernel carries two
running gradient partials (2 DM doubles) on top of the single-posterior kernel's registers, the chain kernel the point's coordinates
and one.  (Scalar registers parked in vector lanes, which every acquisition kernel has, cost no memory and are not counted here.)
Metadata only (the `amdhsa.kernels` block)."""
import functools
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (source file, kernel-name substring)
KERNELS = [("acq.hip", "ffgp_acq_kernel"), ("acq_stack.hip", "ffgp_stack_acq_kernel"), ("acq_tree.hip", "ffgp_tree_acq_kernel"),
           ("acq_chain.hip", "ffgp_chain_acq_kernel")]


@functools.lru_cache(maxsize=None)
def kernels_of(src, substr):
    """{kernel name: its metadata block (amdhsa.kernels) as a dict of the integer fields}"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from check_isa import device_asm
    asm = device_asm(src)
    ks = asm[asm.index("amdhsa.kernels:"):]
    out = {}
    for blk in re.split(r"\n  - ", ks)[1:]:
        m = re.search(r"\.name:\s+(\S+)", blk)
        if m and substr in m.group(1):
            out[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.([a-z_]+):\s+(\d+)\n", blk)}
    return out


@pytest.fixture(params=KERNELS, ids=[k for _, k in KERNELS])
def acq_kernels(request):
    src, substr = request.param
    return src, kernels_of(src, substr)


def test_acq_kernel_has_its_three_instantiations(acq_kernels):
    src, kernels = acq_kernels
    assert len(kernels) == 3, sorted(kernels)      # D <= 2, D <= 8, D <= 16 (chain: D + 1; tree: the leaf count is a run-time argument)
    if src != "acq.hip":                           # the single kernel's substring counts acq.hip's instantiations alone
        assert not any("ffgp_acq_kernel" in name for name in kernels)
        assert not kernels_of(src, "ffgp_acq_kernel")


def test_acq_kernel_uses_no_scratch(acq_kernels):
    _, kernels = acq_kernels
    assert kernels
    for name, meta in kernels.items():
        print(name, {k: meta[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count")})
        assert meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_spill_count"] == 0, (name, meta)


def test_acq_kernel_fits_a_256_thread_workgroup(acq_kernels):
    """a SIMD has 512 VGPRs per lane and the workgroup's four waves sit one per SIMD, so any unified count (`vgpr_count`: arch + acc)
    up to 512 runs -- and 256 threads are what the kernel is launched with"""
    _, kernels = acq_kernels
    assert kernels
    for name, meta in kernels.items():
        assert meta["max_flat_workgroup_size"] == 256, (name, meta)
        assert meta["agpr_count"] <= meta["vgpr_count"] <= 512, (name, meta)
        assert meta["vgpr_spill_count"] == 0, (name, meta)
        assert meta["group_segment_fixed_size"] == 0, (name, meta)      # dynamic LDS only, sized from n (the largest member) by the host
