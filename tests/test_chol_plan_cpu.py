"""The host planner of the Cholesky drivers (sympgpr_amd/csrc/chol_plan.hip) on its own: the file holds no HIP call and includes
no HIP header, so it is compiled here as plain C++ (g++ -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined
-fno-sanitize-recover=all -Wall -Werror) together with the Strassen planner its sizing walk calls and tests/chol_plan_main.cpp,
which supplies tune() and set_error().  That program is run directly -- nothing is loaded into Python, nothing is preloaded --
with the default tunables and with la_max = 1024.  It walks the look-ahead driver's block schedule, every panel's geometry, the
queue driver's panel grid and the workspace layout, and ends with status 0 only if every invariant that follows from the panel
kernel's limits (panel.h) holds; a sanitizer report ends it with another status.  What it prints must be
tests/golden/chol_plan.json (tools/chol_plan_golden.py), and its workspace totals and Strassen scratch needs must be what the
built library reports for the same orders.  No GPU needed."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import chol_plan_golden as gold  # noqa: E402

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

# the library's side of the comparison, in a process of its own: "la_max" is read once per process
LIBRARY_SIDE = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
from sympgpr_amd import _lib as L
lib, probe = L.load_library(), L.load_probe_library()
if len(sys.argv) > 3:
    L.check(probe.sgpr_probe_tune(b"la_max", float(sys.argv[3])), "sgpr_probe_tune")
out = {"need": [], "workspace": []}
for n in json.loads(sys.argv[2]):
    two, top = (C.c_ulonglong * 2)(), (C.c_ulonglong * 2)()
    if n > 0:
        L.check(probe.sgpr_probe_strassen_rec_scratch(n, two), "rec_scratch")
        L.check(probe.sgpr_probe_strassen_top_scratch(n, top), "top_scratch")
        out["need"].append([n, int(two[0]), int(two[1]), int(top[0])])
    out["workspace"].append([n, int(lib.sgpr_potrf_workspace(n))])
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to build the stand-alone planner"
    exe = str(tmp_path_factory.mktemp("chol_plan") / "chol_plan_asan")
    b = gold.build(exe, SAN)     # plain g++: no HIP header is on its include path
    assert b.returncode == 0, b.stderr[-4000:]
    return gold.run_all(exe)     # raises unless both runs end with status 0


def library_side(orders, la_max=None):
    args = [sys.executable, "-c", LIBRARY_SIDE, ROOT, json.dumps(orders)] + ([str(la_max)] if la_max else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.splitlines()[-1])


def test_planner_alone_under_sanitizers_walks_every_order(planner):
    d, s = planner["default"], planner["la_max_1024"]
    assert d["la_max"] == 57344 and s["la_max"] == 1024
    assert len(d["blocks"]) == 11 * 2 * 2                       # eleven orders, nb = 0 / 256, fused or not
    assert {b["n"] for b in d["blocks"]} == {256, 384, 1000, 2048, 4096, 8192, 12288, 16384, 24576, 32768, 57344}
    assert any(b["fused"] and len(b["panels"]) == len(b["starts"]) - 1 for b in d["blocks"])
    assert [r["blocks"] for r in d["recursion_blocks"]] == [{"4096": 1}, {"32768": 2}, {"32768": 4}]
    assert [r["blocks"] for r in s["recursion_blocks"]] == [{"1024": 4}, {"1024": 64}, {"1024": 128}]
    assert all(q[4] <= 4 for q in d["queue"])


def test_planner_output_is_the_pinned_list(planner):
    with open(gold.GOLDEN) as f:
        want = json.load(f)
    assert planner == want


@pytest.mark.parametrize("run, la_max", [("default", None), ("la_max_1024", 1024)])
def test_needs_and_workspace_match_the_built_library(planner, run, la_max):
    doc = planner[run]
    orders = [row[0] for row in doc["layout"]]
    lib = library_side(orders, la_max)
    asked = {row[0] for row in doc["need"]}
    assert len(asked) == 13 and [r for r in lib["need"] if r[0] in asked] == doc["need"]
    assert any(r[1] > 0 for r in doc["need"]) and any(r[3] > 0 for r in doc["need"])     # orders that do reserve something
    # below the queue driver's window (and for n <= 0) the workspace holds no queue part: the totals must be equal; above it
    # the library's is larger by the queue's part, a multiple of 256 bytes
    for (n, total_lib), row in zip(lib["workspace"], doc["layout"]):
        assert row[0] == n
        if n < 13312:
            assert total_lib == row[5], n
        else:
            assert total_lib >= row[5] and (total_lib - row[5]) % 256 == 0, n
