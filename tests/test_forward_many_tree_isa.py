"""Build-time check of the composed-kernel prediction launch (csrc/predict_small_tree.hip; no GPU needed: hipcc cross-compiles): each
instantiation of its kernel runs entirely in registers and LDS -- no private (scratch) segment, no vector register spilled -- its
dynamic LDS request fits the CU's 160 KiB, and it is compiled for the 512 threads it is launched with.  Metadata only, as
test_train_tree_lds_isa.py."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def kernels():
    """{kernel name: its metadata block (amdhsa.kernels) as a dict of the integer fields}"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from check_isa import device_asm
    asm = device_asm("predict_small_tree.hip")
    ks = asm[asm.index("amdhsa.kernels:"):]
    out = {}
    for blk in re.split(r"\n  - ", ks)[1:]:
        m = re.search(r"\.name:\s+(\S+)", blk)
        if m:
            out[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.([a-z_]+):\s+(\d+)\n", blk)}
    return out


def _dynamic_lds_bytes():
    """the host's request, PST_LDS_DOUBLES of predict_small_tree.hip restated: the block image, X [128][17], three [128][16] images,
    pivots and the (unused) diagonal extra, the leaves' tables, 8 scalars, the tile's test points [16][17], vsq [32][16], the int table"""
    blocks, ints = 36 * 16 * 17, 4 + 5 + 3 + 16
    return (blocks + 128 * 17 + 3 * 128 * 16 + 2 * 128 + (3 * 4 * 16 + 4 * 4) + 8 + 16 * 17 + 32 * 16 + ints // 2) * 8


def test_the_two_instantiations_are_there(kernels):
    assert len(kernels) == 2 and all("ffgp_predict_small_tree_kernel" in name for name in kernels), sorted(kernels)
    assert any("ILi8E" in name for name in kernels) and any("ILi16E" in name for name in kernels)


def test_no_scratch_and_no_spilled_vector_register(kernels):
    for name, meta in kernels.items():
        assert meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_spill_count"] == 0, (name, meta)


def test_lds_fits_the_cu_and_the_launch_matches_the_bounds(kernels):
    csrc = os.path.join(ROOT, "fidelityfusion_amd", "csrc")
    src = open(os.path.join(csrc, "predict_small_tree.hip")).read()
    tile = open(os.path.join(csrc, "train_tile.h")).read()
    # the formula restated above: the head the one-launch kernels share (train_tile.h), then this kernel's tail
    for piece in ("#define TR_OFF_XS (NBLK_LOWER * BLKSZ)", "#define TR_OFF_YM (TR_OFF_XS + TR_N * (TR_D + 1))",
                  "#define TR_OFF_GAM (TR_OFF_YM + TR_N * TR_Y)", "#define TR_OFF_AM (TR_OFF_GAM + TR_N * TR_Y)",
                  "#define TR_OFF_PIV (TR_OFF_AM + TR_N * TR_Y)", "#define TR_OFF_DVEC (TR_OFF_PIV + TR_N)",
                  "#define TR_OFF_TAIL (TR_OFF_DVEC + TR_N)", "#define TR_N 128", "#define TR_D 16", "#define TR_Y 16", "#define TR_T 512"):
        assert piece in tile, piece
    for piece in ("#define PST_OFF_LEAF TR_OFF_TAIL", "#define PST_OFF_SC (PST_OFF_LEAF + 3 * TTL_L * TR_D + 4 * TTL_L)",
                  "#define PST_OFF_XT (PST_OFF_SC + 8)", "#define PST_OFF_VSQ (PST_OFF_XT + 16 * (TR_D + 1))",
                  "#define PST_OFF_INT (PST_OFF_VSQ + 32 * 16)", "#define PST_INTS (4 + 5 + 3 + 16)",
                  "#define PST_LDS_DOUBLES (PST_OFF_INT + PST_INTS / 2)",
                  "static_assert(PST_LDS_DOUBLES * sizeof(double) <= 160 * 1024",
                  "const size_t lds_bytes = PST_LDS_DOUBLES * sizeof(double);",
                  "hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes)",
                  "hipLaunchKernelGGL(kernel, dim3(F, split), dim3(TR_T), lds_bytes, h->stream, tab, info);"):
        assert piece in src, piece
    for name, meta in kernels.items():
        assert meta["max_flat_workgroup_size"] == 512, (name, meta)
        assert meta["group_segment_fixed_size"] + _dynamic_lds_bytes() <= LDS_PER_CU, (name, meta)
