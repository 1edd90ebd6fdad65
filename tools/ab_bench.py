"""Parent-against-change A/B of bench.py, the project's protocol (profiles/r07a_gemm_rotate_ab.txt): every run a fresh process, arms
alternated P, C, P, C, ... on one box, `--steps 20 --warmup 5`, five runs per arm; per workload the medians, min-max and the bar (the
larger of the two arms' spreads).

    python tools/ab_bench.py PARENT_LIB [runs]      PARENT_LIB: libffgp.so built from the parent commit (arm P, through FFGP_LIB);
                                                    arm C is the tree's own library
A run that fails ends the script (nothing more is started on the GPU after a fault).
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = [("headline", []), ("c2_n8192", ["--workload", "c2", "--n", "8192"]), ("c2", ["--workload", "c2"]),
             ("cigar4", ["--workload", "cigar4"])]


def one(arm, parent_lib, extra):
    env = dict(os.environ)
    env.pop("FFGP_LIB", None)
    if arm == "P":
        env["FFGP_LIB"] = parent_lib
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"] + extra,
                         env=env, capture_output=True, text=True, timeout=300)
    if out.returncode != 0:
        sys.stdout.write(out.stdout[-2000:] + out.stderr[-2000:])
        raise SystemExit("arm %s %s: exit %d" % (arm, extra, out.returncode))
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    return res["ms_per_step"], res.get("nll", res.get("joint_nll"))


def main():
    parent_lib = os.path.abspath(sys.argv[1])
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    print("== bench.py --steps 20 --warmup 5 [workload args]: arm, run, ms_per_step ==", flush=True)
    for name, extra in WORKLOADS:
        print("-- " + name, flush=True)
        ms = {"P": [], "C": []}
        nll = {}
        for r in range(1, runs + 1):
            for arm in ("P", "C"):
                t, v = one(arm, parent_lib, extra)
                ms[arm].append(t)
                nll[arm] = v
                print("%s %d %s" % (arm, r, t), flush=True)
        for arm in ("P", "C"):
            print("%s median %.3f min %.3f max %.3f spread %.3f ; nll %r" % (arm, statistics.median(ms[arm]), min(ms[arm]), max(ms[arm]),
                                                                           max(ms[arm]) - min(ms[arm]), nll[arm]), flush=True)
        dm = statistics.median(ms["P"]) - statistics.median(ms["C"])
        bar = max(max(ms[a]) - min(ms[a]) for a in ("P", "C"))
        print("P - C median = %.3f ms (%.2f %%) ; bar = larger spread %.3f ms" % (dm, 100 * dm / statistics.median(ms["P"]), bar), flush=True)


if __name__ == "__main__":
    main()
