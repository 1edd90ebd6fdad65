"""The k loop of the 128 x 128 fast GEMM tile as the compiler emitted it for gfx950 (no GPU needed: hipcc cross-compiles).

kernel_meta(asm, name)   the .amdhsa metadata entries of one kernel (.vgpr_count, .vgpr_spill_count, .group_segment_fixed_size ...)
k_loop(asm, name)        the instructions of the innermost loop that holds 64 negate-A MFMAs (one k-tile of the alpha = -1 fast form)
loop_report(loop)        what tests/test_gemm_loop_isa.py asserts on: barriers, MFMAs / LDS reads behind the barrier, 64-bit vector adds;
                         and tests/test_gemm_dma_loop_isa.py: direct-to-LDS loads, LDS stores, where the vmcnt waits sit

`python tools/gemm_loop_isa.py` prints the report for the trailing update's instantiation.
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_isa import device_asm  # noqa: E402

SYRK = "ffgp_gemm_f64ILi0ELi0ELi1ELi1ELi128ELi128EE"     # ffgp_gemm_f64<0, 0, 1, 1, 128, 128>


def kernel_meta(asm, name):
    """{key: int} of the kernel's entry in the amdhsa.kernels metadata."""
    m = re.search(r"\.name:\s+_Z\w*%s\w*\n" % re.escape(name), asm)
    assert m, "no metadata entry for " + name
    lines = asm.splitlines()
    at = asm[:m.start()].count("\n")
    item = re.compile(r"^  - \.\w+:")                                                   # first key of a kernel's list item
    lo = max(i for i in range(at + 1) if item.match(lines[i]))
    hi = next((i for i in range(at + 1, len(lines)) if item.match(lines[i]) or not lines[i].startswith(" ")), len(lines))
    out = {}
    for l in lines[lo:hi]:
        mm = re.match(r"\s*-?\s*(\.\w+):\s+(\d+)\s*$", l)
        if mm:
            out[mm.group(1)] = int(mm.group(2))
    return out


def function_body(asm, name):
    """All lines of the kernel, label to .Lfunc_end (a kernel with early returns has several s_endpgm)."""
    lines = asm.splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*%s\w*:" % re.escape(name), l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def instructions(body):
    return [l.strip() for l in body if l.strip() and not l.strip().startswith(";") and not l.strip().startswith(".") or re.match(r"^\.LBB\d+_\d+:", l)]


def k_loop(asm, name=SYRK, mfmas=64, marker="neg:[1,0,0]"):
    """Instruction list (labels included), loop header to back edge, of the smallest loop with `mfmas` marked MFMAs on 16 distinct
    accumulators: the 4 x 4 MFMA tiles of a wave of the 128 x 128 tile.  (The split tail's 64 x 64 tiles live in the same kernel; their
    loop is unrolled over four k-tiles, which is 64 MFMAs as well, on 4 accumulators.)"""
    body = instructions(function_body(asm, name))
    labels = {l.split(":")[0]: i for i, l in enumerate(body) if re.match(r"^\.LBB\d+_\d+:", l)}
    best = None
    for i, l in enumerate(body):
        m = re.match(r"s_(?:cbranch_\w+|branch) (\.LBB\d+_\d+)", l)
        if not m or m.group(1) not in labels or labels[m.group(1)] > i:
            continue
        loop = body[labels[m.group(1)]:i + 1]
        mf = [x for x in loop if x.startswith("v_mfma") and marker in x]
        if len(mf) == mfmas and len({x.split()[1] for x in mf}) == 16 and (best is None or len(loop) < len(best)):
            best = loop
    assert best is not None, "no loop with %d MFMAs carrying %s in %s" % (mfmas, marker, name)
    return best


def loop_report(loop):
    bars = [i for i, l in enumerate(loop) if l.startswith("s_barrier")]
    after = loop[bars[-1] + 1:] if bars else []
    vmem = [i for i, l in enumerate(loop) if re.match(r"(global|buffer)_load", l)]
    dma = [i for i in vmem if re.search(r"\blds$", loop[i])]                # direct-to-LDS: the register load's mnemonic + `lds`
    vmw = [i for i, l in enumerate(loop) if l.startswith("s_waitcnt") and "vmcnt" in l]
    last_mfma_before_bar = max([i for i, l in enumerate(loop[:bars[0]]) if l.startswith("v_mfma")], default=-1) if bars else -1
    # a DMA followed (cyclically: the loop's top follows its back edge) by a vmcnt wait before the next LDS read
    ring = loop + loop
    drained = 0
    for i in dma:
        for l in ring[i + 1:i + 1 + len(loop)]:
            if l.startswith("ds_read"):
                break
            if l.startswith("s_waitcnt") and "vmcnt" in l:
                drained += 1
                break
    return {
        "lds_dma_loads": len(dma),
        "ds_write": sum(1 for l in loop if l.startswith("ds_write")),
        "vmcnt_waits": len(vmw),
        "vmcnt_wait_in_front_of_barrier": bool(bars) and len(vmw) == 1 and last_mfma_before_bar < vmw[0] < bars[0],
        "vmcnt_wait_between_dma_and_ds_read": drained,
        "instructions": len(loop),
        "barriers": len(bars),
        "mfma_before_barrier": sum(1 for l in (loop[:bars[0]] if bars else []) if l.startswith("v_mfma")),
        "mfma_after_barrier": sum(1 for l in after if l.startswith("v_mfma")),
        "ds_read_after_barrier": sum(1 for l in after if l.startswith("ds_read")),
        "v_lshl_add_u64": sum(1 for l in loop if l.startswith("v_lshl_add_u64")),
        "s_nop": sum(1 for l in loop if l.startswith("s_nop")),
        "valu": sum(1 for l in loop if l.startswith("v_") and not l.startswith("v_mfma")),
        "vmem_loads": sum(1 for l in loop if re.match(r"(global|buffer)_load", l)),
        "lds_drain_before_first_mfma": any(re.match(r"s_waitcnt .*lgkmcnt\(0\)", l)
                                           for l in loop[:next(i for i, x in enumerate(loop) if x.startswith("v_mfma"))]),
    }


if __name__ == "__main__":
    asm = open(sys.argv[1]).read() if len(sys.argv) > 1 else device_asm("gemm.hip")
    meta = kernel_meta(asm, SYRK)
    print({k: meta.get(k) for k in (".vgpr_count", ".vgpr_spill_count", ".sgpr_count", ".group_segment_fixed_size")})
    print(loop_report(k_loop(asm)))
