"""The staging of the trailing update's k loop, ffgp_gemm_f64<0, 0, 1, 1, 128, 128>, as compiled for gfx950 (CPU: hipcc cross-compiles).

K-major operands go global -> LDS directly (`buffer_load_dwordx4 ... offen lds`, gemm_tile_fast128 in csrc/gemm.hip): no staging
registers, no LDS store pass, and the only wait for memory is the one in front of the k-tile's barrier.  All of that is a property of
the generated code: the compiler counts these loads itself and is free to drain them in front of an LDS read it thinks may alias."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import gemm_loop_isa  # noqa: E402

PARENT_VALU = 13      # vector-ALU instructions of the register-staged loop this one replaced


@pytest.fixture(scope="module")
def asm():
    return gemm_loop_isa.device_asm("gemm.hip")


def test_resources(asm):
    meta = gemm_loop_isa.kernel_meta(asm, gemm_loop_isa.SYRK)
    print(meta)
    assert meta[".vgpr_count"] <= 256
    assert meta[".vgpr_spill_count"] == 0
    assert meta[".group_segment_fixed_size"] == 65536


def test_k_loop_stages_by_dma(asm):
    rep = gemm_loop_isa.loop_report(gemm_loop_isa.k_loop(asm))
    print(rep)
    assert rep["vmem_loads"] == 8 and rep["lds_dma_loads"] == 8, "8 vector loads per k-tile, all of them direct-to-LDS"
    assert rep["ds_write"] == 0, "no LDS store pass"
    assert rep["vmcnt_waits"] == 1 and rep["vmcnt_wait_in_front_of_barrier"], \
        "one wait for the pieces, between the last MFMA in front of the barrier and the barrier"
    assert rep["vmcnt_wait_between_dma_and_ds_read"] == 0, "the pieces are not drained in front of the LDS reads that follow them"
    assert rep["v_lshl_add_u64"] == 0
    assert rep["valu"] <= PARENT_VALU
