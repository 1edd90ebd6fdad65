"""The child process of test_gpu_helper_roles.py: one kernel family of the diagonal-block stage loops under every forced SIMD table.

    python tests/helper_roles_child.py FAMILY OUT.json        (FFGP_LIB = fidelityfusion_amd/libffgp_roles.so, read at import)

For every case of the family it sets each table of TABLES in turn (ffgp_test_roles_set_*, csrc/diag_block.h), runs the case from the
same seeded inputs, reads back the roles the kernels used (ffgp_test_roles_seen_*) and writes its verdicts as JSON:
    roles           table -> what was read back, and whether it is the expectation of TABLES
    identical       table -> the first result that differs in ANY bit from the natural table's ("" = none)
    repeat          the same for a second run under the natural table
    reference       name -> [error, bar, within]: the natural table's results against the high-precision reference, at the bar of the
                    existing test named beside each bar below
The parent asserts on every verdict; this script asserts nothing about the numbers itself, so that one run reports all of them."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# wave 0 .. 7 -> SIMD, and the roles HELPER_ROLES must hand out: (nh, hidx of wave 0 .. 7)
TABLES = {
    "natural":        ((0, 1, 2, 3, 0, 1, 2, 3), (6, (-1, 0, 1, 2, -1, 3, 4, 5))),     # two waves per SIMD
    "six_other_set":  ((1, 0, 1, 2, 3, 0, 2, 3), (6, (-1, 0, -1, 1, 2, 3, 4, 5))),     # wave 2 is no helper, wave 4 is one
    "five":           ((0, 1, 2, 3, 0, 0, 1, 2), (5, (-1, 0, 1, 2, -1, -1, 3, 4))),
    "four":           ((0, 0, 1, 2, 0, 0, 3, 1), (4, (-1, -1, 0, 1, -1, -1, 2, 3))),   # helpers 2, 3, 6, 7
    "seven":          ((0, 1, 1, 2, 2, 3, 3, 1), (7, (-1, 0, 1, 2, 3, 4, 5, 6))),      # without the fallback
    "three_fallback": ((0, 0, 0, 1, 0, 0, 2, 3), (7, (-1, 0, 1, 2, 3, 4, 5, 6))),      # three waves off wave 0's SIMD
    "none_fallback":  ((0, 0, 0, 0, 0, 0, 0, 0), (7, (-1, 0, 1, 2, 3, 4, 5, 6))),
}
UNITS = ("potrf", "train", "train_tree_lds", "train_tree_lds_res")      # the translation units with a table of their own

POTRF_N = (16, 17, 33, 100, 113, 128, 129, 300)      # nst = 1, 2, 3, 7, 8, 8; a full block and a one-row block; three panels
FAMILIES = {
    "potrf": ["potrf_n%d" % n for n in POTRF_N] + ["bad_pivot_n300_row200", "ragged_300_250_129", "batched_3x300"],
    "tr_body": ["train_n17", "train_n100", "train_n128", "small_likelihood_41_128"],
    "tree": ["sum_n33", "prod_n33", "sum_n128", "prod_n128", "ar_residual_fixture"],
}
DEV = "cuda:0"


def _pack(simd):
    return sum(s << (2 * w) for w, s in enumerate(simd))


def _unpack(seen):
    return {"ran": bool(seen >> 31), "nh": (seen >> 24) & 7, "hidx": [((seen >> (3 * w)) & 7) - 1 for w in range(8)]}


class Roles:
    def __init__(self, lib):
        self.lib = lib

    def set(self, simd):
        for u in UNITS:
            rc = getattr(self.lib, "ffgp_test_roles_set_" + u)(C.c_uint(_pack(simd)))
            assert rc == 0, (u, rc)

    def seen(self, unit):
        """the roles the unit's kernels used since the last call (which clears the record)"""
        out = C.c_uint(0)
        rc = getattr(self.lib, "ffgp_test_roles_seen_" + unit)(C.byref(out))
        assert rc == 0, (unit, rc)
        return out.value


def first_difference(a, b):
    if sorted(a) != sorted(b):
        return "keys"
    for k in sorted(a):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():      # bytes: NaN poison and signed zeros count
            return k
    return ""


def walk(roles, unit, run):
    """run() -> {name: array} under every table (the natural one twice, first) -> (the natural results, the verdicts)"""
    v = {"roles": {}, "identical": {}, "seconds_natural": None}
    base = None
    for name, (simd, (nh, hidx)) in TABLES.items():
        roles.set(simd)
        for u in UNITS:
            roles.seen(u)
        t0 = time.perf_counter()
        res = run()
        dt = time.perf_counter() - t0
        got = _unpack(roles.seen(unit))
        v["roles"][name] = {"seen": got, "ok": got == {"ran": True, "nh": nh, "hidx": list(hidx)}}
        if base is None:
            base, v["seconds_natural"] = res, dt
            v["repeat"] = first_difference(run(), base)
        v["identical"][name] = first_difference(res, base)
    roles.set(TABLES["natural"][0])
    return base, v


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a.reshape(b.shape) - b).max() / max(np.abs(b).max(), 1e-300))


def bar(err, bound, strict=True):
    return [err, bound, bool(err < bound if strict else err <= bound)]


# ------------------------------------------------------------------------------------------------ ffgp_potrf_rows and what reads its inverse
def spd(n, rng, cond=1e3):      # test_gpu_kernels.spd
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (Q * np.logspace(0, np.log10(cond), n)) @ Q.T


def potrf_case(n, ctx):
    import scipy.linalg as sla
    import torch
    _lib, h, roles = ctx
    rng = np.random.default_rng(n)
    S = spd(n, rng)
    m = 3 if n in (100, 300) else 0      # passenger rows
    R = rng.standard_normal((m, n))
    B = rng.standard_normal((n, 5))
    ld = (n + 1) // 2 * 2 + 2
    W = np.full((n + m, ld), np.nan)
    W[:n, :n] = np.tril(S) + np.triu(np.full((n, n), 777.0), 1)      # poison above the diagonal: must not be read or written
    W[n:, :n] = R
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def run():
        Wd = dev(W)
        out = {"rc": np.array(_lib.lib.ffgp_potrf_rows(h, ptr(Wd), n, n + m, ld))}
        torch.cuda.synchronize()
        out["factor_image"] = Wd.cpu().numpy()      # the whole buffer: L, the poison above it, the passenger rows, the NaN padding
        for name, fn in (("trsm_lower", _lib.lib.ffgp_trsm_lower), ("trsm_lower_t", _lib.lib.ffgp_trsm_lower_t), ("potrs", _lib.lib.ffgp_potrs)):
            Bd = dev(B)
            out["rc_" + name] = np.array(fn(h, ptr(Wd), n, ld, ptr(Bd), 5, 5))
            torch.cuda.synchronize()
            out[name] = Bd.cpu().numpy()
        out["rc_potri"] = np.array(_lib.lib.ffgp_potri(h, ptr(Wd), n, ld))
        torch.cuda.synchronize()
        out["potri"] = np.tril(Wd.cpu().numpy()[:n, :n])
        return out

    base, v = walk(roles, "potrf", run)
    L = np.linalg.cholesky(S)
    img = base["factor_image"]
    v["reference"] = {
        "status": bar(float(max(abs(int(base[k])) for k in base if k.startswith("rc"))), 0.0, strict=False),
        "factor": bar(relerr(np.tril(img[:n, :n]), L), 1e-11),                                            # test_potrf_matches_lapack
        "poison_intact": bar(float((img[:n, :n][np.triu_indices(n, 1)] != 777.0).sum()), 0.0, strict=False),
        "trsm_lower": bar(relerr(base["trsm_lower"], sla.solve_triangular(L, B, lower=True)), 1e-10),     # test_trsm_and_potrs
        "trsm_lower_t": bar(relerr(base["trsm_lower_t"], sla.solve_triangular(L.T, B, lower=False)), 1e-10),
        "potrs": bar(relerr(base["potrs"], np.linalg.solve(S, B)), 1e-9),
        "potri": bar(relerr(base["potri"], np.tril(np.linalg.inv(S))), 1e-9),                             # test_potri
    }
    if m:
        v["reference"]["passenger_rows"] = bar(relerr(img[n:, :n], sla.solve_triangular(L, R.T, lower=True).T), 1e-10)      # test_potrf_passenger_rows
    return v


def bad_pivot_case(ctx):
    """test_potrf_diag_kernel_variants' last lines: a non-positive pivot inside a block reports its 1-based index, under every table"""
    import torch
    _lib, h, roles = ctx
    n = 300
    S = spd(n, np.random.default_rng(7))
    S[200, 200] = -5.0
    ld = n + 2

    def run():
        Wd = torch.tensor(np.pad(np.tril(S), ((0, 0), (0, 2))), dtype=torch.float64, device=DEV)
        rc = _lib.lib.ffgp_potrf_rows(h, C.c_void_p(Wd.data_ptr()), n, n, ld)
        torch.cuda.synchronize()
        return {"rc": np.array(rc)}

    base, v = walk(roles, "potrf", run)
    v["reference"] = {"reports_row_201": bar(float(abs(int(base["rc"]) - 201)), 0.0, strict=False)}
    return v


def likelihood_case(sizes, ctx, unit, value_bar, grad_bar):
    """negative_log_likelihood_many on ARD members of `sizes` points: values and every gradient; the reference is the numpy oracle"""
    import torch
    from fidelityfusion_amd import functional as F
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.cigp_v10 import cigp, negative_log_likelihood_many
    from oracle import gp_oracle as O
    _lib, h, roles = ctx
    data = []
    for f, n in enumerate(sizes):
        D, d = 2 + f, (2 if len(set(sizes)) == 1 else 1 + f % 2)      # (members of one size: one shape, as the batched chain wants)
        X, Y = O.synthetic_xy(n, D, d, seed=100 * n + f)
        rng = np.random.default_rng(n + f)
        data.append((X, Y, rng.uniform(0.5, 1.5, D) * rng.choice([-1.0, 1.0], D), [-0.9 + 0.2 * f], [0.4 + 0.1 * f]))
    entry = "ffgp_nlml_fused_batch" if unit == "potrf" else "ffgp_nlml_fused_small_batch"      # the one call that serves all members
    calls = []

    class _Spy:
        def __getattr__(self, name):
            real = getattr(_lib.lib, name)
            if name != entry:
                return real

            def counted(h_, nF, *a):
                calls.append(nF)
                return real(h_, nF, *a)
            return counted

    def run():
        models, xs, ys = [], [], []
        calls.clear()
        for X, Y, ls, sv, lb in data:
            k = kernel.ARDKernel(X.shape[1])
            with torch.no_grad():
                k.length_scales.copy_(torch.tensor(ls))
                k.signal_variance.copy_(torch.tensor(sv))
            models.append(cigp(k, lb[0]).double().to(DEV))
            xs.append(torch.tensor(X, device=DEV))
            ys.append(torch.tensor(Y, device=DEV, requires_grad=True))
        with F.patched_lib(_Spy()):
            vals = negative_log_likelihood_many(models, xs, ys)
            vals.sum().backward()
        torch.cuda.synchronize()
        out = {"values": vals.detach().cpu().numpy(), "members_per_batched_call": np.array(calls, dtype=np.int64)}
        for f, (m, y) in enumerate(zip(models, ys)):
            out["g%d_length_scales" % f] = m.kernel.length_scales.grad.cpu().numpy()
            out["g%d_signal_variance" % f] = m.kernel.signal_variance.grad.cpu().numpy()
            out["g%d_log_beta" % f] = m.log_beta.grad.cpu().numpy()
            out["g%d_Y" % f] = y.grad.cpu().numpy()
        return out

    base, v = walk(roles, unit, run)
    v["reference"] = {"one_%s_call_for_all_members" % entry: bar(float(base["members_per_batched_call"].tolist() != [len(sizes)]), 0.0, strict=False)}
    for f, (X, Y, ls, sv, lb) in enumerate(data):
        ll, g = O.cigp_ll_and_grads(X, Y, ls, sv, lb)
        v["reference"]["value_%d" % f] = bar(relerr(base["values"][f], ll), value_bar)
        for name in ("length_scales", "signal_variance", "log_beta", "Y"):
            v["reference"]["g%d_%s" % (f, name)] = bar(relerr(base["g%d_%s" % (f, name)], g[name]), grad_bar)
    return v


# ------------------------------------------------------------------------------------------------ tr_body as the trainer
def adam_state(state):
    return np.concatenate([state["chunks"][k].buf.detach().cpu().numpy().ravel() for k in sorted(state["chunks"])])


def train_case(n, D, d, ctx):
    """test_one_workgroup_kernel_edge_shapes_against_the_oracle, part (ii): three Adam steps against the reference's loop, 1e-11"""
    import copy
    import torch
    from fidelityfusion_amd import kernel
    from fidelityfusion_amd.cigp_v10 import cigp, train_many
    from test_gpu_train import params_of, reference_loop
    _lib, h, roles = ctx
    rng = np.random.default_rng(1000 * n + 10 * D + d)
    X, Y = rng.uniform(0, 1, (n, D)), rng.standard_normal((n, d))
    ls = rng.uniform(0.5, 1.5, D) * rng.choice([-1.0, 1.0], D)

    def make():
        k = kernel.ARDKernel(D)
        with torch.no_grad():
            k.length_scales.copy_(torch.tensor(ls))
            k.signal_variance.copy_(torch.tensor([-0.9]))
        return cigp(k, 0.4).double().to(DEV), torch.tensor(X, device=DEV), torch.tensor(Y, device=DEV)

    def run():
        m, x, y = make()
        trace, state = train_many([m], [x], [y], 3, lr=1e-2)
        torch.cuda.synchronize()
        assert state["fused"] is True
        out = {"trace": trace.cpu().numpy(), "adam_state": adam_state(state)}
        out.update({"param_%d" % i: p for i, p in enumerate(params_of(m))})
        return out

    base, v = walk(roles, "train", run)
    twin, x, y = make()
    ref = reference_loop([twin], [x], [y], 3, 1e-2)
    v["reference"] = {"trace": bar(relerr(base["trace"], ref), 1e-11)}
    for i, p in enumerate(params_of(twin)):
        v["reference"]["param_%d" % i] = bar(relerr(base["param_%d" % i], p), 1e-11)
    return v


# ------------------------------------------------------------------------------------------------ the one-launch tree trainers
SUM, PROD = ("sum", "lin", "m52"), ("prod", "ard", "m32")
TREE_MEMBERS = {"sum_n33": (33, 2, 2, SUM, False), "prod_n33": (33, 3, 1, PROD, False), "sum_n128": (128, 3, 1, SUM, False),
                "prod_n128": (128, 4, 1, PROD, False)}      # (prod_n128: test_gpu_train_tree.CASES["prod2_n128"])


def tree_case(name, ctx):
    """test_gpu_train_tree_lds._follows_the_loop at three steps: the per-step loop through the drop-in modules, the file's own metric, and
    the bound every case of its table has, 1e-12 (max(10 d0, 1e-12) with d0 <= 6.5e-14 measured over 40 steps)"""
    import copy
    import torch
    from fidelityfusion_amd.cigp_v10 import train_many
    from test_gpu_train_tree import LR, distance, make_models, params_of, reference_loop
    _lib, h, roles = ctx

    def run():
        models, xs, ys = make_models([TREE_MEMBERS[name]], 11)
        trace, state = train_many(models, xs, ys, 3, lr=LR, tree_one_launch=True)
        torch.cuda.synchronize()
        assert state["fused"] is True and state["tree_one_launch"] == [0]
        out = {"trace": trace.cpu().numpy(), "adam_state": adam_state(state)}
        out.update({"param_%d" % i: p for i, p in enumerate(params_of(models[0]))})
        return out, trace, models

    base, v = walk(roles, "train_tree_lds", lambda: run()[0])
    _, trace, models = run()
    twins, xs, ys = make_models([TREE_MEMBERS[name]], 11)
    ref = reference_loop(twins, xs, ys, 3, LR)
    v["reference"] = {"distance_to_the_per_step_loop": bar(distance(trace, models, ref, twins), 1e-12, strict=False)}
    return v


def ar_residual_case(ctx):
    """test_gpu_train_tree_residual.test_on_the_reference_fixtures[lds-train_tree_ar_subset]: the reference's own fp64 loop, 1e-8"""
    import torch
    from fidelityfusion_amd.cigp_v10 import cigp, train_many
    from test_gpu_train_tree import LM, T
    from test_gpu_train_tree_lds import build_kernel2
    _lib, h, roles = ctx
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "train_tree_ar_subset.npz")))

    def run():
        m = cigp(build_kernel2(LM, 1, np.random.default_rng(0)), 1.0).double().to(DEV)
        with torch.no_grad():
            for i, p in enumerate(m.parameters()):
                p.copy_(T(g["init_%d" % i]).reshape(p.shape))
        rho = torch.nn.Parameter(T(g["rho_init"]).reshape(()))
        res = (rho, T(g["y_low"]), T(g["y_high"]))
        trace, state = train_many([m], [T(g["x"])], [None], int(g["steps"]), lr=float(g["lr"]), residual=[res], fuse_composed=True,
                                  tree_one_launch=True)
        torch.cuda.synchronize()
        assert state["fused"] is True and state["tree_one_launch"] == [0]
        out = {"trace": trace[0].cpu().numpy(), "adam_state": adam_state(state), "rho": rho.detach().cpu().numpy(),
               "residual_targets": state["residual_targets"][0][0].cpu().numpy()}
        out.update({"param_%d" % i: p.detach().cpu().numpy() for i, p in enumerate(m.parameters())})
        return out

    base, v = walk(roles, "train_tree_lds_res", run)
    v["reference"] = {"trace": bar(relerr(base["trace"], g["trace"]), 1e-8, strict=False),
                      "rho": bar(relerr(base["rho"], g["rho_final"]), 1e-8, strict=False)}
    for i in range(6):
        v["reference"]["final_%d" % i] = bar(relerr(base["param_%d" % i], g["final_%d" % i]), 1e-8, strict=False)
    return v


def main(family, out_path):
    t_start = time.perf_counter()
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    from fidelityfusion_amd import _lib
    assert os.path.basename(_lib._SO) == "libffgp_roles.so", "FFGP_LIB must name the -DFFGP_TEST_ROLES build: %s" % _lib._SO
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    h = _lib.handle(0)
    _lib.bind_stream(h, 0)
    ctx = (_lib, h, Roles(_lib.lib))
    verdicts = {}
    for case in FAMILIES[family]:
        t0 = time.perf_counter()
        if case.startswith("potrf_n"):
            v = potrf_case(int(case[7:]), ctx)
        elif case == "bad_pivot_n300_row200":
            v = bad_pivot_case(ctx)
        elif case == "ragged_300_250_129":
            v = likelihood_case((300, 250, 129), ctx, "potrf", 1e-10, 1e-7)      # test_nlml_and_grads_vs_oracle
        elif case == "batched_3x300":
            v = likelihood_case((300, 300, 300), ctx, "potrf", 1e-10, 1e-7)
        elif case.startswith("train_n"):
            v = train_case(*{17: (17, 1, 3), 100: (100, 5, 2), 128: (128, 16, 16)}[int(case[7:])], ctx)
        elif case == "small_likelihood_41_128":
            v = likelihood_case((41, 128), ctx, "train", 1e-10, 1e-8)            # test_one_workgroup_kernel_edge_shapes_against_the_oracle (i)
        elif case == "ar_residual_fixture":
            v = ar_residual_case(ctx)
        else:
            v = tree_case(case, ctx)
        v["seconds"] = time.perf_counter() - t0
        verdicts[case] = v
    verdicts["_seconds_total"] = time.perf_counter() - t_start
    with open(out_path, "w") as f:
        json.dump(verdicts, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
