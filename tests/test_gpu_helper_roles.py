"""GPU: the diagonal-block stage loops under every helper-wave placement.  ffgp_potrf_diag128_v4 (plain and ragged / batched), tr_body
(train.hip) and the one-launch tree trainers (train_tree_lds.h) read their waves' SIMD ids at run time and turn them into the helpers'
roles (HELPER_ROLES, csrc/helper_roles.h); the suite otherwise only ever sees the placement an idle CU hands out.  Here the SIMD ids
are forced -- libffgp_roles.so, the -DFFGP_TEST_ROLES build (csrc/diag_block.h) -- through seven tables: the natural one, another set
of six helpers, five, four, seven, and the two that take the fallback.  For every case and every table:
  * the roles the kernels report back are the table's expectation (a forced table that was ignored fails here);
  * every result is BIT-IDENTICAL to the natural table's -- every block product and every inverse column is formed by one wave with
    one instruction sequence, whichever wave that is;
  * the natural table's results meet the high-precision reference at the bar of the neighbouring existing test.
FFGP_LIB is read when the package is imported, so each kernel family runs in a fresh child process (tests/helper_roles_child.py) that
walks all tables and writes its verdicts; one child at a time, none is retried, and after a child that ended on a signal or at its
time limit no further child is started.  (The hand-out itself for all 4^8 tables, on the CPU: test_helper_roles_host.py.)"""
import json
import os
import subprocess
import sys

import pytest

import helper_roles_child as child

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLES_SO = os.path.join(ROOT, "fidelityfusion_amd", "libffgp_roles.so")
# a child's time on an MI355X, all cases under all seven tables, python's start and the imports included: potrf 2.7 s, tr_body 4.2 s,
# tree 4.4 s.  A time limit counts as a hang, so it is generous: fifty times that and more
TIMEOUT_S = {"potrf": 240, "tr_body": 240, "tree": 240}
_ended_badly = []      # the family whose child ended on a signal or at its time limit: nothing more is started after it
_verdicts = {}


def verdicts_of(family, tmp_path_factory):
    if family in _verdicts:
        return _verdicts[family]
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if _ended_badly:
        pytest.fail("not started: the child of family %r ended on a signal or at its time limit" % _ended_badly[0])
    assert os.path.exists(ROLES_SO), "libffgp_roles.so is missing: `make -C fidelityfusion_amd/csrc roles` (build() makes it)"
    out = str(tmp_path_factory.mktemp("roles_" + family) / "verdicts.json")
    env = dict(os.environ, FFGP_LIB=ROLES_SO)
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helper_roles_child.py"), family, out], env=env, capture_output=True,
                           text=True, timeout=TIMEOUT_S[family])
    except subprocess.TimeoutExpired:
        _ended_badly.append(family)
        _verdicts[family] = None
        pytest.fail("the child of family %r did not finish in %d s" % (family, TIMEOUT_S[family]))
    if p.returncode < 0:
        _ended_badly.append(family)
    if p.returncode != 0:
        _verdicts[family] = None
        pytest.fail("the child of family %r ended with status %d:\n%s" % (family, p.returncode, (p.stdout + p.stderr)[-3000:]))
    _verdicts[family] = json.load(open(out))
    print("family %s: %.1f s in the child" % (family, _verdicts[family]["_seconds_total"]))
    return _verdicts[family]


CASES = [(family, case) for family in ("potrf", "tr_body", "tree") for case in child.FAMILIES[family]]


@pytest.mark.parametrize("family,case", CASES, ids=[c for _, c in CASES])
def test_stage_loops_under_every_helper_placement(family, case, tmp_path_factory):
    v = verdicts_of(family, tmp_path_factory)
    assert v is not None, "the child of family %r failed (reported by the first test of the family)" % family
    v = v[case]
    assert sorted(v["roles"]) == sorted(child.TABLES) and sorted(v["identical"]) == sorted(child.TABLES)
    # the roles read back from the kernels that ran are those the table forces
    wrong = {t: r["seen"] for t, r in v["roles"].items() if not r["ok"]}
    assert not wrong, "roles the kernels used, against %s: %s" % ({t: child.TABLES[t][1] for t in wrong}, wrong)
    # two runs under the natural table agree in every bit, and so does every other table with them
    assert v["repeat"] == "", "result %r changed between two runs under the natural table" % v["repeat"]
    differs = {t: name for t, name in v["identical"].items() if name}
    assert not differs, "results that are not bit-identical to the natural table's: %s" % differs
    # the natural table's results against the high-precision reference, at the existing tests' bars
    print(case, {k: "%.3g (bar %.0e)" % (e, b) for k, (e, b, _) in v["reference"].items()})
    missed = {k: (e, b) for k, (e, b, ok) in v["reference"].items() if not ok}
    assert not missed, missed


def test_the_tables_force_what_they_are_meant_to():
    """the expectations of the table walk, restated from the SIMD ids: helpers are the waves off wave 0's SIMD, fewer than four -> all
    seven; between them the tables reach nh = 4, 5, 6 (two helper sets), 7 and the fallback (from three helpers and from none)"""
    for name, (simd, (nh, hidx)) in child.TABLES.items():
        off = [w for w in range(1, 8) if simd[w] != simd[0]]
        helpers = off if len(off) >= 4 else list(range(1, 8))
        assert nh == len(helpers) and [w for w in range(8) if hidx[w] >= 0] == helpers, name
        assert [hidx[w] for w in helpers] == list(range(nh)) and hidx[0] == -1, name
    off = {name: sum(s != simd[0] for s in simd[1:]) for name, (simd, _) in child.TABLES.items()}
    assert off == {"natural": 6, "six_other_set": 6, "five": 5, "four": 4, "seven": 7, "three_fallback": 3, "none_fallback": 0}
    assert child.TABLES["natural"][1] != child.TABLES["six_other_set"][1]
