"""The child process of test_gpu_forward_many_composed_roles.py: the composed-kernel batched prediction kernel
(csrc/predict_small_tree.hip) under every forced SIMD table.

    python tests/forward_many_composed_roles_child.py OUT.json        (FFGP_LIB = fidelityfusion_amd/libffgp_roles.so, read at import)

The tables, the packing of a table and of the record read back, and the bitwise comparison are helper_roles_child.py's; the pattern is
forward_many_roles_child.py's.  Each table is set in turn (ffgp_test_roles_set_predict_small_tree, csrc/diag_block.h) and the edge-shape
check of test_gpu_forward_many_composed.py runs as it stands -- seven members in one call and each alone, bit-identical either way,
every member served by the composed call, the comparator's bar -- from the same members; the roles the kernel used are read back
(ffgp_test_roles_seen_predict_small_tree), and the verdicts are written as JSON:
    roles       table -> what was read back, and whether it is the expectation of TABLES
    check       table -> "" or the edge-shape check's failure under that table
    identical   table -> the first result that differs in ANY bit from the natural table's ("" = none)
    repeat      the same for a second run under the natural table
The parent asserts on every verdict."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["edge_shapes"]


def main(out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    torch.set_default_dtype(torch.float64)
    import helper_roles_child as H
    import test_gpu_forward_many_composed as FC
    from fidelityfusion_amd import _lib
    lib = _lib.lib
    t_all = time.perf_counter()
    members = [FC.member(FC.SUM_LIN_M52, n, D, d, nt, 9000 + 100 * n + D) for (n, D, d, nt) in FC.EDGE_SHAPES]
    loops = [FC.bits([FC.loop_diag(*mb[:4])])[0] for mb in members]

    def run():
        try:
            batch, _ = FC.edge_shape_figures(members, loops)
        except AssertionError as e:
            return None, "AssertionError: %s" % (e,)
        res = {}
        for f, (mean, var) in enumerate(batch):
            res["mean%d" % f], res["var%d" % f] = mean, var
        return res, ""

    def seen():
        o = C.c_uint(0)
        rc = lib.ffgp_test_roles_seen_predict_small_tree(C.byref(o))
        assert rc == 0, rc
        return o.value

    v = {"roles": {}, "identical": {}, "check": {}}
    base = None
    for name, (simd, (nh, hidx)) in H.TABLES.items():
        rc = lib.ffgp_test_roles_set_predict_small_tree(C.c_uint(H._pack(simd)))
        assert rc == 0, rc
        seen()
        res, why = run()
        got = H._unpack(seen())
        v["roles"][name] = {"seen": got, "ok": got == {"ran": True, "nh": nh, "hidx": list(hidx)}}
        v["check"][name] = why
        if res is None:
            v["identical"][name] = "no result"
            continue
        if base is None:
            base = res
            again, why2 = run()
            v["repeat"] = why2 if again is None else H.first_difference(again, base)
        v["identical"][name] = H.first_difference(res, base)
    lib.ffgp_test_roles_set_predict_small_tree(C.c_uint(H._pack(H.TABLES["natural"][0])))
    verdicts = {"edge_shapes": v, "_seconds_total": time.perf_counter() - t_all}
    with open(out, "w") as f:
        json.dump(verdicts, f)


if __name__ == "__main__":
    main(sys.argv[1])
