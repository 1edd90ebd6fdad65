"""CPU: the helper-wave hand-out of the diagonal-block kernels (HELPER_ROLES, fidelityfusion_amd/csrc/helper_roles.h) under every
placement the hardware could report.  tests/helper_roles_host.cpp expands the kernels' own macro on the host for all 4^8 tables
wave -> SIMD and checks what the stage loops need of the roles: 4 <= nh <= 7, wave 0 no helper, the helpers' indices 0 .. nh - 1 each
once, the trailing-update blocks of every stage partitioned, the inverse's seven columns each computed once.  (The kernels under forced
tables: test_gpu_helper_roles.py.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helper_roles_host.cpp")
CSRC = os.path.join(ROOT, "fidelityfusion_amd", "csrc")
# 4 C(7, k) 3^k tables leave k of the seven other waves off wave 0's SIMD; k < 4 (4624 tables) takes the fallback to nh = 7
CLEAN = "helper_roles_host: 65536 tables clean (nh = 4: 11340, 5: 20412, 6: 20412, 7: 13372, of which fallback: 4624)"


def _cxx():
    return os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"


def _build_and_run(tmp_path, flags, include=CSRC):
    exe = str(tmp_path / "helper_roles_host")
    subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", include, SRC, "-o", exe], check=True, timeout=300)
    return subprocess.run([exe], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_every_simd_table_hands_out_usable_roles(tmp_path, flags):
    p = _build_and_run(tmp_path, flags)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip() == CLEAN and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stdout + p.stderr


def test_the_program_notices_a_hand_out_without_the_fallback(tmp_path):
    """the same program against a copy of the header whose `nh < 4` branch is gone: the first table (all waves on one SIMD) fails"""
    src = open(os.path.join(CSRC, "helper_roles.h")).read()
    a, b = src.index("    if (nh < 4) {"), src.index("    hidx = FFGP_UNIFORM(hidx);")
    inc = tmp_path / "inc"
    inc.mkdir()
    (inc / "helper_roles.h").write_text(src[:a] + src[b:])
    p = _build_and_run(tmp_path, ["-O2"], str(inc))
    assert p.returncode == 1 and "table 0 0 0 0 0 0 0 0: nh = 0" in p.stdout, p.stdout + p.stderr


def test_the_kernels_publish_their_simd_through_the_seam():
    """every expansion of HELPER_ROLES reads a table written with wave_simd() and reports its roles; nothing else calls simd_id()"""
    import re
    expansions, direct = [], []
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".h")):
            continue
        txt = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, f)).read())
        if f not in ("helper_roles.h", "diag_block.h"):
            n = len(re.findall(r"\bHELPER_ROLES\(", txt))
            if n:
                expansions.append(f)
                assert len(re.findall(r"\bwave_simd\(wave\)", txt)) == n and len(re.findall(r"\bROLES_SEEN\(", txt)) == n, f
            if re.search(r"\bsimd_id\(", txt):
                direct.append(f)
    assert expansions == ["potrf.hip", "train.hip", "train_tree_lds.h"] and direct == []
