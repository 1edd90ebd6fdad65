"""GPU: the stage loop of the wide-output one-launch trainer (ffgp_train_wide_kernel, csrc/train_wide.hip) under every helper-wave
placement -- test_gpu_helper_roles.py's check for the kernel that joined the users of the hand-out (helper_roles(), csrc/diag_block.h).
The SIMD ids are forced through libffgp_roles.so's table of that translation unit; for every case and every table of
helper_roles_child.TABLES the roles the kernel reports back are the table's expectation, and every result -- loss trace, parameters,
rho -- is BIT-IDENTICAL to the natural table's.  (Against the per-step loop under the natural placement: test_gpu_train_wide.py.)
FFGP_LIB is read when the package is imported, so the cases run in ONE fresh child process (tests/train_wide_roles_child.py), which is
not retried; a child that ended on a signal or at its time limit fails every case."""
import json
import os
import subprocess
import sys

import pytest

import helper_roles_child as H
import train_wide_roles_child as child

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLES_SO = os.path.join(ROOT, "fidelityfusion_amd", "libffgp_roles.so")
TIMEOUT_S = 240      # the child takes seconds; a time limit counts as a hang, so it is generous
_verdicts = {}


def verdicts(tmp_path_factory):
    if "v" in _verdicts:
        return _verdicts["v"]
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert os.path.exists(ROLES_SO), "libffgp_roles.so is missing: `make -C fidelityfusion_amd/csrc roles` (build() makes it)"
    out = str(tmp_path_factory.mktemp("roles_train_wide") / "verdicts.json")
    _verdicts["v"] = None
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "train_wide_roles_child.py"), out], env=dict(os.environ, FFGP_LIB=ROLES_SO),
                           capture_output=True, text=True, timeout=TIMEOUT_S)
    except subprocess.TimeoutExpired:
        pytest.fail("the child did not finish in %d s" % TIMEOUT_S)
    if p.returncode != 0:
        pytest.fail("the child ended with status %d:\n%s" % (p.returncode, (p.stdout + p.stderr)[-3000:]))
    _verdicts["v"] = json.load(open(out))
    print("%.1f s in the child" % _verdicts["v"]["_seconds_total"])
    return _verdicts["v"]


@pytest.mark.parametrize("case", child.CASES)
def test_wide_trainer_under_every_helper_placement(case, tmp_path_factory):
    v = verdicts(tmp_path_factory)
    assert v is not None, "the child failed (reported by the first case)"
    v = v[case]
    assert sorted(v["roles"]) == sorted(H.TABLES) and sorted(v["identical"]) == sorted(H.TABLES)
    wrong = {t: r["seen"] for t, r in v["roles"].items() if not r["ok"]}
    assert not wrong, "roles the kernel used, against %s: %s" % ({t: H.TABLES[t][1] for t in wrong}, wrong)
    assert v["repeat"] == "", "result %r changed between two runs under the natural table" % v["repeat"]
    differs = {t: name for t, name in v["identical"].items() if name}
    assert not differs, "results that are not bit-identical to the natural table's: %s" % differs
