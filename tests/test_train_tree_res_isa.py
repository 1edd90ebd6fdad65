"""Build-time check of the kernels a residual member adds to the launch-per-stage composed-kernel trainer (csrc/train_tree_res.hip;
no GPU needed: hipcc cross-compiles).  Metadata only, as test_train_tree_isa.py: both small kernels run entirely in registers -- no
private (scratch) segment, no spilled vector register -- the Adam kernel's static LDS is its two reduction rows, and the residual
table fits the kernel-argument segment."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from check_isa import device_asm
    asm = device_asm("train_tree_res.hip")
    ks = asm[asm.index("amdhsa.kernels:"):]
    out = {}
    for blk in re.split(r"\n  - ", ks)[1:]:
        m = re.search(r"\.name:\s+(\S+)", blk)
        if m:
            out[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.([a-z_]+):\s+(\d+)\n", blk)}
    return out


def test_the_unit_holds_exactly_its_two_kernels(kernels):
    assert sorted(kernels) == ["ffgp_tree_res_adam_kernel", "ffgp_tree_resid_form"]


@pytest.mark.parametrize("name", ["ffgp_tree_resid_form", "ffgp_tree_res_adam_kernel"])
def test_no_scratch_and_no_spilled_vector_register(kernels, name):
    meta = kernels[name]
    assert meta["private_segment_fixed_size"] == 0, meta
    assert meta["vgpr_spill_count"] == 0, meta
    assert meta["vgpr_count"] <= 128, meta      # (256 threads a workgroup: no pressure on occupancy either)


def test_lds_and_kernel_arguments_of_the_small_kernels(kernels):
    # part[256] and drho[16] doubles, far below a CU's 160 KiB; the residual table travels by value: 16 members of twelve 8-byte
    # fields and one int, inside the 4 KiB kernel-argument segment
    assert kernels["ffgp_tree_res_adam_kernel"]["group_segment_fixed_size"] == (256 + 16) * 8
    assert kernels["ffgp_tree_resid_form"]["group_segment_fixed_size"] == 0
    for name, meta in kernels.items():
        assert meta["kernarg_segment_size"] <= 4096, (name, meta)
    for name, meta in kernels.items():      # compiled for the 256 threads the reductions assume and the launches use
        assert meta["max_flat_workgroup_size"] == 256, (name, meta)


LDS_PER_CU = 160 * 1024
# The one-launch unit: four instantiations, (DM = 8 | 16) x (V1 | V2), each with residual members.  The <8> pair runs in registers and LDS
# alone; the <16> pair spills two vector registers to 12 B of scratch (train.hip's <16> has 116 B): pinned as upper bounds.
SCRATCH_MAX = {"ILi8E": (0, 0), "ILi16E": (12, 2)}


@pytest.fixture(scope="module")
def lds_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from check_isa import device_asm
    asm = device_asm("train_tree_lds_res.hip")
    ks = asm[asm.index("amdhsa.kernels:"):]
    out = {}
    for blk in re.split(r"\n  - ", ks)[1:]:
        m = re.search(r"\.name:\s+(\S+)", blk)
        if m:
            out[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.([a-z_]+):\s+(\d+)\n", blk)}
    return out


def test_the_four_one_launch_instantiations_are_there(lds_kernels):
    assert len(lds_kernels) == 4 and all("ffgp_train_tree_lds_res_kernel" in name for name in lds_kernels), sorted(lds_kernels)
    for dm in ("ILi8E", "ILi16E"):
        for v2 in ("Lb0E", "Lb1E"):
            assert any(dm + v2 in name for name in lds_kernels), (dm, v2)


def test_one_launch_kernels_workgroup_lds_and_scratch(lds_kernels):
    # the request, TTL_RES_LDS_DOUBLES of train_tree_lds.h restated: train_tree_lds.hip's layout and two [128] variance rows behind it
    blocks, ints = 36 * 16 * 17, 136 + 4 + 5 + 3 + 16
    request = (blocks + 128 * 17 + 3 * 128 * 16 + 2 * 128 + (3 * 4 * 16 + 4 * 4) + 4 * 136 + 8 + ints // 2 + 2 * 128) * 8
    hdr = open(os.path.join(ROOT, "fidelityfusion_amd", "csrc", "train_tree_lds.h")).read()
    for piece in ("#define TTL_OFF_VAR TTL_LDS_DOUBLES", "#define TTL_RES_LDS_DOUBLES (TTL_OFF_VAR + 2 * TR_N)",
                  "#define TTL_LDS_DOUBLES (TTL_OFF_INT + TTL_INTS / 2)", "#define TTL_PPAD 136"):
        assert piece in hdr, piece
    for name, meta in lds_kernels.items():
        assert meta["max_flat_workgroup_size"] == 512, (name, meta)
        assert meta["group_segment_fixed_size"] + request <= LDS_PER_CU, (name, meta)
        scratch, spills = SCRATCH_MAX["ILi8E" if "ILi8E" in name else "ILi16E"]
        assert meta["private_segment_fixed_size"] <= scratch, (name, meta)
        assert meta["vgpr_spill_count"] <= spills, (name, meta)
