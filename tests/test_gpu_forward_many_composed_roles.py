"""GPU: the stage loop of the composed-kernel batched prediction kernel (ffgp_predict_small_tree_kernel, csrc/predict_small_tree.hip)
under every helper-wave placement -- test_gpu_forward_many_roles.py's check for the kernel that joined the users of the hand-out
(helper_roles(), csrc/diag_block.h).  The SIMD ids are forced through libffgp_roles.so's table of that translation unit; under every
table of helper_roles_child.TABLES the roles the kernel reports back are the table's expectation, the edge-shape check of
test_gpu_forward_many_composed.py passes as it stands, and every mean and variance is BIT-IDENTICAL to the natural table's.
FFGP_LIB is read when the package is imported, so the case runs in ONE fresh child process
(tests/forward_many_composed_roles_child.py), which is not retried; a child that ended on a signal or at its time limit fails the case."""
import json
import os
import subprocess
import sys

import pytest

import helper_roles_child as H
import forward_many_composed_roles_child as child

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLES_SO = os.path.join(ROOT, "fidelityfusion_amd", "libffgp_roles.so")
TIMEOUT_S = 240      # the child takes seconds; a time limit counts as a hang, so it is generous


@pytest.mark.parametrize("case", child.CASES)
def test_tree_predict_kernel_under_every_helper_placement(case, tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert os.path.exists(ROLES_SO), "libffgp_roles.so is missing: `make -C fidelityfusion_amd/csrc roles` (build() makes it)"
    out = str(tmp_path / "verdicts.json")
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "forward_many_composed_roles_child.py"), out],
                           env=dict(os.environ, FFGP_LIB=ROLES_SO), capture_output=True, text=True, timeout=TIMEOUT_S)
    except subprocess.TimeoutExpired:
        pytest.fail("the child did not finish in %d s" % TIMEOUT_S)
    if p.returncode != 0:
        pytest.fail("the child ended with status %d:\n%s" % (p.returncode, (p.stdout + p.stderr)[-3000:]))
    verdicts = json.load(open(out))
    print("%.1f s in the child" % verdicts["_seconds_total"])
    v = verdicts[case]
    assert sorted(v["roles"]) == sorted(H.TABLES) and sorted(v["identical"]) == sorted(H.TABLES)
    wrong = {t: r["seen"] for t, r in v["roles"].items() if not r["ok"]}
    assert not wrong, "roles the kernel used, against %s: %s" % ({t: H.TABLES[t][1] for t in wrong}, wrong)
    failed = {t: why for t, why in v["check"].items() if why}
    assert not failed, "the edge-shape check under forced tables: %s" % failed
    assert v["repeat"] == "", "result %r changed between two runs under the natural table" % v["repeat"]
    differs = {t: name for t, name in v["identical"].items() if name}
    assert not differs, "results that are not bit-identical to the natural table's: %s" % differs
