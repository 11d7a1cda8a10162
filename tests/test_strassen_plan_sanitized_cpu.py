"""The Strassen planner (sympgpr_amd/csrc/strassen_plan.hip) under the host sanitizers: the file holds no HIP call and includes no
HIP header, so it is compiled here as plain C++ (g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all)
together with tests/strassen_plan_main.cpp, which supplies tune() and set_error() and walks the scaled-down grid of
tools/strassen_lists.py through every plan, need and schedule entry.  That program is run directly -- nothing is loaded into
Python, nothing is preloaded.  It must end with status 0 (a sanitizer report ends it with another), and the lists, records and word
sums it prints must be those the library gives through the probes for the same grid.  No GPU needed."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import strassen_lists as sl  # noqa: E402
import strassen_plan as sp  # noqa: E402
import strassen2_plan as sp2  # noqa: E402
import strassen_rec_plan as srp  # noqa: E402
import strassen_schedule as ssch  # noqa: E402
import strassen_top_plan as stp  # noqa: E402

FLAGS = ["-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror"]


@pytest.fixture
def small_tunables():
    srp.set_tunables(sl.SMALL)
    yield
    srp.set_tunables(dict(srp.SHIPPED, **stp.SHIPPED))


def library_counts():
    """{entry: [lists, records, sum of words]} of the grid through the probes"""
    t = {name: [0, 0, 0] for name in ("rec_plan", "top_plan", "schedule", "plan", "plan2", "cfg_plan", "need2", "need3")}

    def count(name, arr, extra=()):
        t[name][0] += 1
        t[name][1] += len(arr)
        t[name][2] += int(np.asarray(arr, dtype=np.int64).sum()) + sum(int(v) for v in extra)

    for lower in (0, 1):
        for m in sl.M_N:
            for n in ((m,) if lower else sl.M_N):
                for k in sl.K:
                    for cap in (sp.UNLIMITED, (m // 2 + n // 2) * 256):
                        plan, cfg = srp.fetch_plan(m, n, k, lower, cap)
                        count("rec_plan", plan, cfg.values())
                        top = stp.fetch_plan(m, n, k, lower, cap)
                        count("top_plan", top)
                        count("plan", sp.fetch_plan(m, n, k, lower, 128, 512, cap))
                        count("plan2", sp2.fetch_plan(m, n, k, lower, 128, 512, 256, 1024, cap))
                        if cap == sp.UNLIMITED:
                            t["need3"][0] += 1
                            t["need3"][2] += stp.scratch_need(top)
                    count("cfg_plan", stp.cfg_plan(m, n, k, lower, (128, 512, 256, 1024, 128)))
                    sched, info = ssch.fetch_schedule(m, n, k, lower, -1)
                    count("schedule", sched)
                    t["need2"][0] += 1
                    t["need2"][2] += sum(info["need"])
                    sched, info = ssch.fetch_schedule(m, n, k, lower, 4 * sum(info["need"]))
                    count("schedule", sched, info["need"] + info["buffers"] + [info["streams"], info["capacity"]])
    return t


def test_planner_alone_under_address_and_undefined_sanitizers(tmp_path, small_tunables):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone planner"
    exe = str(tmp_path / "strassen_plan_asan")
    build = subprocess.run([gxx] + FLAGS + [os.path.join(ROOT, "sympgpr_amd", "csrc", "strassen_plan.hip"),
                                           os.path.join(ROOT, "tests", "strassen_plan_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, run.stderr[-4000:]
    got = {f[0]: [int(v) for v in f[1:]] for f in (line.split() for line in run.stdout.splitlines())}
    want = library_counts()
    assert got == want
    assert want["rec_plan"][1] > want["rec_plan"][0] and want["top_plan"][1] > want["top_plan"][0]    # lists beyond one record each
    assert want["need2"][2] > 0 and want["need3"][2] > 0
