"""Build-time checks of the residual trainer (no GPU needed): the new one-launch instantiations of csrc/train.hip stay within the
register file the existing ones use, and ffgp_train_residual_raw is declared, exported and bound."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _meta(asm, name):
    """the kernel's metadata block (amdhsa.kernels) as a dict of its integer fields"""
    ks = asm[asm.index("amdhsa.kernels:"):]
    for blk in re.split(r"\n  - ", ks)[1:]:
        m = re.search(r"\.name:\s+(\S+)", blk)
        if m and name in m.group(1):
            return {k: int(v) for k, v in re.findall(r"\.([a-z_]+):\s+(\d+)\n", blk)}
    raise AssertionError("kernel %s not found" % name)


@pytest.fixture(scope="module")
def train_asm():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from check_isa import device_asm
    return device_asm("train.hip")


def test_residual_trainer_instantiations_spill_no_more_than_the_plain_ones(train_asm):
    plain8 = _meta(train_asm, "ffgp_train_persist_kernelILi8E")
    plain16 = _meta(train_asm, "ffgp_train_persist_kernelILi16E")
    res8 = _meta(train_asm, "ffgp_train_resid_kernelILi8E")
    res16 = _meta(train_asm, "ffgp_train_resid_kernelILi16E")
    assert plain8["private_segment_fixed_size"] == 0
    assert res8["private_segment_fixed_size"] == 0, res8
    assert res16["private_segment_fixed_size"] <= plain16["private_segment_fixed_size"], (res16, plain16)


def test_residual_export_is_declared_exported_and_bound():
    from fidelityfusion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ffgp.h")).read()
    assert re.search(r"\bint ffgp_train_residual_raw\s*\(", hdr)
    assert "ffgp_train_residual_raw" in _lib.EXPORTS
    so = os.path.join(ROOT, "fidelityfusion_amd", "libffgp.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT ffgp_train_residual_raw\b", syms)
    assert _lib.lib.ffgp_train_residual_raw is not None
