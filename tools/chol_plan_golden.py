"""Writes tests/golden/chol_plan.json: the look-ahead driver's block schedule, every panel's geometry, the chain_bound switches,
the queue driver's panel grid, the workspace layout and the Strassen scratch needs, as THIS tree's planner
(sympgpr_amd/csrc/chol_plan.hip) gives them -- the output of tests/chol_plan_main.cpp with the default tunables and with
la_max = 1024.  Run it only after the launches of the tree have been compared with the parent's on the device
(profiles/chol_split/same_bits.txt): the file pins the planner, it does not prove it.
    python tools/chol_plan_golden.py            # rewrite the file
    python tools/chol_plan_golden.py --check    # compare only (status 1 on a difference)"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "chol_plan.json")
SOURCES = [os.path.join(ROOT, "sympgpr_amd", "csrc", "chol_plan.hip"), os.path.join(ROOT, "sympgpr_amd", "csrc", "strassen_plan.hip"),
           os.path.join(ROOT, "tests", "chol_plan_main.cpp")]
RUNS = {"default": [], "la_max_1024": ["1024"]}


def build(exe, flags=("-O1",)):
    """the stand-alone planner program; returns the compiler's CompletedProcess"""
    return subprocess.run(["g++", "-x", "c++", "-std=c++17", "-Wall", "-Werror"] + list(flags) + SOURCES + ["-o", exe],
                          capture_output=True, text=True)


def run_all(exe):
    """{run: parsed document}; raises when the program reports a violated invariant"""
    out = {}
    for name, args in RUNS.items():
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
        if r.returncode != 0:
            raise RuntimeError("chol_plan_main %s: status %d\n%s" % (name, r.returncode, r.stderr[-4000:]))
        out[name] = json.loads(r.stdout)
    return out


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "chol_plan_main")
        b = build(exe)
        if b.returncode != 0:
            sys.exit(b.stderr)
        doc = run_all(exe)
    if "--check" in sys.argv[1:]:
        sys.exit(0 if json.load(open(GOLDEN)) == doc else 1)
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", GOLDEN)
