"""The LDS image of a K-major 128 x 16 operand tile under direct-to-LDS staging (gemm_tile_fast128, csrc/gemm.hip), on the CPU.

A `buffer_load_dwordx4 ... lds` writes its 64 lanes to consecutive 16-byte slots, so lane idx = tid + 256 i of the workgroup lands at
row idx >> 3, slot idx & 7 of the [row][16] image, and the image's XOR swizzle is applied to the chunk the lane FETCHES
(dma_lane_offsets).  The image must be the one sstore writes from registers -- the fragment reads (frag_offsets) did not change."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import emulate_kernels as emu  # noqa: E402

ROWS, LD = 128, 272      # the tile sits in a wider array (leading dimension 272 doubles), k-tile at column 34


def dma_source_chunk(idx):
    """(row, chunk) lane idx fetches; its destination is byte 16 * idx of the operand buffer"""
    row, slot = idx >> 3, idx & 7
    return row, slot ^ ((row >> 1) & 7)


def test_dma_image_is_the_sstore_image():
    rng = np.random.default_rng(1)
    P = rng.standard_normal((ROWS, LD))
    k0 = 34
    ref = np.zeros(4 * emu.OPBUF)
    for tid in range(256):
        emu.sstore(emu.KMAJOR, ref, 0, tid, emu.gload(emu.KMAJOR, P, 0, ROWS, k0, LD, tid))
    img = np.zeros(4 * emu.OPBUF)
    for idx in range(1024):
        row, ch = dma_source_chunk(idx)
        img[2 * idx: 2 * idx + 2] = P[row, k0 + 2 * ch: k0 + 2 * ch + 2]      # lane-linear destination, swizzled source
    assert np.array_equal(img[:ROWS * 16], ref[:ROWS * 16])
    assert np.array_equal(np.sort(ref[:ROWS * 16]), np.sort(P[:, k0:k0 + 16].ravel())), "the image holds the tile, every element once"


def test_a_rows_lanes_fetch_a_permutation_of_its_chunks():
    for row in range(ROWS):
        got = [dma_source_chunk(8 * row + slot) for slot in range(8)]
        assert all(r == row for r, _ in got), "a lane fetched from another row"
        assert sorted(c for _, c in got) == list(range(8)), "the 8 lanes of a row cover its 128-byte line once, nothing outside it"


def test_lane_offsets_derive_from_the_register_form():
    """dma_lane_offsets: voff + (chunk - slot) * 16 bytes, voff the register form's row * ld * 8 + slot * 16"""
    for idx in range(1024):
        row, slot = idx >> 3, idx & 7
        voff = (row * LD + slot * 2) * 8
        dv = voff + ((slot ^ ((row >> 1) & 7)) - slot) * 16
        r, ch = dma_source_chunk(idx)
        assert dv == (r * LD + 2 * ch) * 8 and dv >= 0
