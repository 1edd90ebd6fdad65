"""Build-time check of the composed-kernel trainer's two kernels (no GPU needed: hipcc cross-compiles): both run entirely in
registers -- no private (scratch) segment."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tree_asm():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from check_isa import device_asm
    return device_asm("train_tree.hip")


def _meta(asm, name):
    """the kernel's metadata block (amdhsa.kernels) as a dict of its integer fields"""
    ks = asm[asm.index("amdhsa.kernels:"):]
    for blk in re.split(r"\n  - ", ks)[1:]:
        m = re.search(r"\.name:\s+(\S+)", blk)
        if m and m.group(1) == name:
            return {k: int(v) for k, v in re.findall(r"\.([a-z_]+):\s+(\d+)\n", blk)}
    raise AssertionError("kernel %s not found" % name)


@pytest.mark.parametrize("name", ["ffgp_tree_link_fwd", "ffgp_tree_adam_kernel"])
def test_tree_trainer_kernels_use_no_scratch(tree_asm, name):
    meta = _meta(tree_asm, name)
    assert meta["private_segment_fixed_size"] == 0, meta
    assert meta["vgpr_count"] <= 128, meta      # (256 threads a workgroup: no pressure on occupancy either)
