"""The k loop of the trailing update's kernel, ffgp_gemm_f64<0, 0, 1, 1, 128, 128>, as compiled for gfx950 (CPU: hipcc cross-compiles).

The rotation of gemm_tile_fast128 (csrc/gemm.hip) is a property of the generated code, not of the source: the scheduler is free to sink
the next-stage LDS reads below the last MFMA of a k-tile, which gives the same values at the old speed, and a few more registers or
bytes of LDS cost the second resident workgroup of every CU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import gemm_loop_isa  # noqa: E402


@pytest.fixture(scope="module")
def asm():
    return gemm_loop_isa.device_asm("gemm.hip")


def test_two_workgroups_per_cu(asm):
    meta = gemm_loop_isa.kernel_meta(asm, gemm_loop_isa.SYRK)
    print(meta)
    assert meta[".vgpr_count"] <= 256
    assert meta[".vgpr_spill_count"] == 0
    assert meta[".group_segment_fixed_size"] == 65536


def test_k_loop_is_rotated(asm):
    rep = gemm_loop_isa.loop_report(gemm_loop_isa.k_loop(asm))
    print(rep)
    assert rep["barriers"] == 1, "one barrier per k-tile"
    assert rep["mfma_after_barrier"] >= 16, "the MFMAs of kq = 3 follow the barrier"
    assert rep["mfma_before_barrier"] >= 16, "the barrier sits inside the k-tile's MFMA stream, not at its seam"
    assert rep["ds_read_after_barrier"] >= 4, "the first operands of the next k-tile are read behind the barrier, under those MFMAs"
    assert rep["v_lshl_add_u64"] == 0, "operand loads are SGPR base + 32-bit lane offset: no 64-bit vector address arithmetic"
