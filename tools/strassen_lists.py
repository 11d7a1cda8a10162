"""Digests of every list the Strassen planner (csrc/strassen_plan.hip) emits over a grid of calls, to pin a change of the host
code against the build before it: the lists come through the probes and the fetchers of the replay modules (tools/strassen*_plan.py,
tools/strassen_schedule.py) and are hashed (SHA-256 of the int64 arrays) -- nothing is replayed here.  No GPU needed.

Three child processes run the same grid, because SGPR_GEMM_STRASSEN and the library's own thresholds are read once per process:
"unset" (SGPR_GEMM_STRASSEN not in the environment), "one" (SGPR_GEMM_STRASSEN=1), "streams2" (tunable
gemm_strassen_overlap_streams = 2).  The grid: the scaled-down tunables of tests/test_strassen_top_plan_cpu.py (SMALL) at
m, n in M_N, k in K, and the shipped tunables at 32 times those extents; lower in {0, 1} (m = n when lower); scratch unlimited and
(m / 2 + n / 2) * 256 doubles.  Per grid point: sgpr_probe_strassen_rec_plan (records + the five resolved thresholds),
sgpr_probe_strassen_top_plan, sgpr_probe_strassen_schedule at capacity -1 and at 4 x the need (records + info); at the SMALL extents
also sgpr_probe_strassen_plan / strassen2_plan under 128 / 512 / 256 / 1024 and sgpr_probe_strassen_cfg_plan under (128, 512, 256,
1024, 128); and what potrf() reserves at whole orders.  One digest per (process, entry, tunable set, lower, m).

`python tools/strassen_lists.py --write FILE` writes the fixture (tests/golden/strassen_lists.json was written by the build before
the planner got files of its own); `--check FILE` compares and lists the groups that differ; `--shapes MODE` prints one digest per
call of one process, to find the call behind a group that differs.
Used by tests/test_strassen_lists_pinned_cpu.py."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

M_N = (256, 512, 768, 1024, 1536, 2048, 3072, 4096)
K = (64, 256, 512, 544, 1024, 1536, 2048, 2560, 4096)
SMALL = {"rec_strassen_min_gemm": 128, "rec_strassen_min_syrk": 128, "rec_strassen2_min_gemm": 256, "rec_strassen2_min_syrk": 256,
         "rec_strassen2_kslab_short": 512, "rec_strassen_kslab": 512, "rec_strassen2_kslab": 1024,
         "rec_strassen3_min": 512, "rec_strassen3_kslab": 2048, "rec_strassen3_kslab_short": 1024}
ORDERS = {"small": (1024, 2048, 4096, 8192), "shipped": (65536, 98304, 131072)}
MODES = {"unset": None, "one": "1", "streams2": None}


def _sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(np.asarray(a, dtype=np.int64))
        h.update(np.asarray(a.shape, dtype=np.int64).tobytes())
        h.update(a.tobytes())
    return h.hexdigest()


def run_grid(mode, per_shape=False):
    """the digests and the statistics of one process; call in a process of its own (the environment of `mode` already set)"""
    import strassen_plan as sp
    import strassen2_plan as sp2
    import strassen_rec_plan as srp
    import strassen_schedule as ssch
    import strassen_top_plan as stp

    if mode == "streams2":
        srp.set_tunables({"gemm_strassen_overlap_streams": 2})
    groups, shapes = {}, {}
    stats = {"calls": 0, "records": 0, "kinds": set(), "lists_with_kinds_6_to_9": 0, "schedules_with_second_buffers": 0,
             "capped_lists_that_differ": 0}

    def add(entry, tset, lower, m, shape, arrays):
        arrays = [np.asarray(a, dtype=np.int64) for a in arrays]
        groups.setdefault("%s/%s/lower%d/m%d" % (entry, tset, lower, m), []).extend([np.asarray(shape, dtype=np.int64)] + arrays)
        stats["calls"] += 1
        if per_shape:
            shapes["%s/%s/lower%d/%s" % (entry, tset, lower, "x".join(str(v) for v in shape))] = _sha(arrays)

    def lists(entry, tset, lower, m, n, k, fetch):
        """one list uncapped and capped; fetch(scratch) -> (records, extra words)"""
        got = []
        for cap in (sp.UNLIMITED, (m // 2 + n // 2) * 256):
            plan, extra = fetch(cap)
            add(entry, tset, lower, m, (m, n, k, cap), [plan, extra])
            stats["records"] += len(plan)
            kinds = set(int(v) for v in np.unique(plan[:, 0]))
            stats["kinds"] |= kinds
            stats["lists_with_kinds_6_to_9"] += bool(kinds & {6, 7, 8, 9})
            got.append(plan)
        stats["capped_lists_that_differ"] += not np.array_equal(got[0], got[1])

    for tset, values, scale in (("small", SMALL, 1), ("shipped", dict(srp.SHIPPED, **stp.SHIPPED), 32)):
        srp.set_tunables(values)
        for lower in (0, 1):
            for m in (scale * v for v in M_N):
                for n in ((m,) if lower else (scale * v for v in M_N)):
                    for k in (scale * v for v in K):
                        def rec(cap):
                            plan, cfg = srp.fetch_plan(m, n, k, lower, cap)
                            return plan, list(cfg.values())
                        lists("rec_plan", tset, lower, m, n, k, rec)
                        lists("top_plan", tset, lower, m, n, k, lambda cap: (stp.fetch_plan(m, n, k, lower, cap), []))
                        _, info = ssch.fetch_schedule(m, n, k, lower, -1)
                        for cap in (-1, 4 * sum(info["need"])):
                            sched, info = ssch.fetch_schedule(m, n, k, lower, cap)
                            words = info["need"] + info["buffers"] + [info["streams"], info["capacity"]]
                            add("schedule", tset, lower, m, (m, n, k, cap), [sched, words])
                            stats["records"] += len(sched)
                            stats["schedules_with_second_buffers"] += max(info["buffers"]) > 1
                        if scale != 1:
                            continue
                        lists("plan", tset, lower, m, n, k, lambda cap: (sp.fetch_plan(m, n, k, lower, 128, 512, cap), []))
                        lists("plan2", tset, lower, m, n, k, lambda cap: (sp2.fetch_plan(m, n, k, lower, 128, 512, 256, 1024, cap), []))
                        plan = stp.cfg_plan(m, n, k, lower, (128, 512, 256, 1024, 128))
                        add("cfg_plan", tset, lower, m, (m, n, k), [plan])
                        stats["records"] += len(plan)
        for order in ORDERS[tset]:
            add("rec_scratch", tset, 0, 0, (order,), [srp.scratch_of_order(order)])
            add("top_scratch", tset, 0, 0, (order,), [stp.scratch_of_order(order)])
    stats["kinds"] = sorted(stats["kinds"])
    out = {"digests": {key: _sha(v) for key, v in sorted(groups.items())}, "stats": stats}
    if per_shape:
        out["shapes"] = shapes
    return out


def run_all(per_shape=False):
    """every mode in a child process of its own, side by side -> {mode: {"digests": ..., "stats": ...}}"""
    procs = {}
    for mode, levels in MODES.items():
        env = {k: v for k, v in os.environ.items() if k != "SGPR_GEMM_STRASSEN"}
        if levels is not None:
            env["SGPR_GEMM_STRASSEN"] = levels
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode] + (["--per-shape"] if per_shape else [])
        procs[mode] = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out = {}
    for mode, p in procs.items():
        stdout, stderr = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("strassen_lists child %s: exit status %d\n%s" % (mode, p.returncode, stderr[-2000:]))
        out[mode] = json.loads(stdout.strip().splitlines()[-1])
    return out


def differences(golden, got):
    """the groups whose digests differ, as 'mode: group'"""
    bad = []
    for mode in MODES:
        a, b = golden[mode]["digests"], got[mode]["digests"]
        bad += ["%s: %s" % (mode, key) for key in sorted(set(a) | set(b)) if a.get(key) != b.get(key)]
    return bad


def main(argv):
    if argv[:1] == ["--child"]:
        print(json.dumps(run_grid(argv[1], "--per-shape" in argv)))
    elif argv[:1] == ["--write"]:
        with open(argv[1], "w") as f:
            json.dump(run_all(), f, indent=0, sort_keys=True)
            f.write("\n")
    elif argv[:1] == ["--check"]:
        with open(argv[1]) as f:
            bad = differences(json.load(f), run_all())
        print("\n".join(bad) if bad else "every group matches")
        return 1 if bad else 0
    elif argv[:1] == ["--shapes"]:
        for key, digest in sorted(run_all(per_shape=True)[argv[1]]["shapes"].items()):
            print(digest[:16], key)
    else:
        print(__doc__)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
