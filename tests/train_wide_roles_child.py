"""The child process of test_gpu_train_wide_roles.py: the wide-output one-launch trainer (csrc/train_wide.hip) under every forced SIMD table.

    python tests/train_wide_roles_child.py OUT.json        (FFGP_LIB = fidelityfusion_amd/libffgp_roles.so, read at import)

The tables, the packing of a table and of the record read back, and the bitwise comparison are helper_roles_child.py's.  For every case
each table is set in turn (ffgp_test_roles_set_train_wide, csrc/diag_block.h), the case runs from the same seeded inputs, the roles the
kernel used are read back (ffgp_test_roles_seen_train_wide), and the verdicts are written as JSON:
    roles       table -> what was read back, and whether it is the expectation of TABLES
    identical   table -> the first result that differs in ANY bit from the natural table's ("" = none)
    repeat      the same for a second run under the natural table
The parent asserts on every verdict; this script asserts nothing about the numbers itself, so that one run reports all of them."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["plain_n100_d300", "residual_n128_d600_var", "two_models_n17_n33"]      # 7 stages; 8 stages, 16 column blocks; 2 and 3 stages


def main(out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    torch.set_default_dtype(torch.float64)
    import helper_roles_child as H
    import test_gpu_train_wide as W
    from test_gpu_train_residual import make_residual
    from fidelityfusion_amd import _lib
    from fidelityfusion_amd.cigp_v10 import train_many
    lib = _lib.lib
    t_all = time.perf_counter()

    def run(case):
        if case == "plain_n100_d300":
            m, x, y = W.make_plain((100, 3, 300, "ard", False), 61)
            ms, xs, ys, rs = [m], [x], [y], [None]
        elif case == "residual_n128_d600_var":
            m, x, res = make_residual(128, 9, 600, "matern", "full", 62)
            ms, xs, ys, rs = [m], [x], [None], [res]
        else:
            a, b = W.make_plain((17, 2, 40, "se", False), 63), W.make_plain((33, 16, 100, "ard", True), 64)
            ms, xs, ys, rs = [a[0], b[0]], [a[1], b[1]], [a[2], b[2]], [None, None]
        trace, state = train_many(ms, xs, ys, 4, lr=1e-2, residual=rs, wide_one_launch=True)
        assert state["wide_one_launch"] == list(range(len(ms)))
        res = {"trace": trace.cpu().numpy()}
        for f, m in enumerate(ms):
            for i, p in enumerate(m.parameters()):
                res["p%d_%d" % (f, i)] = p.detach().cpu().numpy()
            if rs[f] is not None:
                res["rho%d" % f] = rs[f][0].detach().cpu().numpy()
        return res

    def seen():
        o = C.c_uint(0)
        rc = lib.ffgp_test_roles_seen_train_wide(C.byref(o))
        assert rc == 0, rc
        return o.value

    verdicts = {}
    for case in CASES:
        v = {"roles": {}, "identical": {}}
        base = None
        for name, (simd, (nh, hidx)) in H.TABLES.items():
            rc = lib.ffgp_test_roles_set_train_wide(C.c_uint(H._pack(simd)))
            assert rc == 0, rc
            seen()
            res = run(case)
            got = H._unpack(seen())
            v["roles"][name] = {"seen": got, "ok": got == {"ran": True, "nh": nh, "hidx": list(hidx)}}
            if base is None:
                base = res
                v["repeat"] = H.first_difference(run(case), base)
            v["identical"][name] = H.first_difference(res, base)
        lib.ffgp_test_roles_set_train_wide(C.c_uint(H._pack(H.TABLES["natural"][0])))
        verdicts[case] = v
    verdicts["_seconds_total"] = time.perf_counter() - t_all
    with open(out, "w") as f:
        json.dump(verdicts, f)


if __name__ == "__main__":
    main(sys.argv[1])
