"""The two product classes of the n = 131072 factorisation that take the top Strassen level (csrc/strassen.hip:
strassen_top_gemm), alone on one MI355X: as the recursion issues them (sgpr_probe_gemm_strassen_top_dev), with the level off,
with its passes serial on the caller's stream, and with them on the low-priority stream (one and two buffer sets), on the same
seeded operands.  The scratch is per process, so every variant is a child process of its own (under a time limit); each prints the
HIP-event times of REPS runs, and the table shows the best and the spread of each.
    python tools/strassen_top_sweep.py > profiles/strassen_top/sweep.txt
    python tools/strassen_top_sweep.py --child off|serial|one_set|two_sets            (one variant, JSON lines)"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import strassen_top_plan as stp  # noqa: E402

# (m, n, k, lower, what it is at n = 131072)
CLASSES = [
    (65536, 32768, 32768, 0, "trsm_rec's largest product"),
    (65536, 65536, 65536, 1, "the lower update of order 65536"),
]
VARIANTS = {"off": {"rec_strassen3_min": 0}, "serial": {"rec_strassen3_overlap": 0}, "one_set": {"rec_strassen3_buffers": 1}, "two_sets": {}}
REPS = 3


def child(name):
    import torch
    from sympgpr_amd import _lib as L
    lib, probe = L.load_library(), L.load_probe_library()
    L.check(lib.sgpr_set_device(0))
    stp.set_tunables(VARIANTS[name])
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for (m, n, k, lower, _) in CLASSES:
        kd = stp.summary(stp.fetch_plan(m, n, k, lower))
        g = torch.Generator(device="cuda").manual_seed(m + n + k)
        A = torch.rand((k, m), dtype=torch.float64, device="cuda", generator=g) - 0.5
        B = A if lower else torch.rand((k, n), dtype=torch.float64, device="cuda", generator=g) - 0.5
        Cm = torch.zeros((n, m), dtype=torch.float64, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def run():
            return probe.sgpr_probe_gemm_strassen_top_dev(m, n, k, -1.0, p(A), m, p(B), n, 1.0, p(Cm), m, lower, None)
        L.check(run())                            # warm: clocks, code objects, the scratch allocations
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            ev[0].record()
            L.check(run())
            ev[1].record()
            torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]))
        # a fingerprint of the result after 1 + REPS updates: variants that take the same list agree bit for bit
        # (lower: its off-diagonal square, where the top level applies; Cm[j, i] = C(i, j))
        fp = float((Cm[:n // 2, m // 2:] if lower else Cm).sum().item())
        print(json.dumps({"shape": [m, n, k, lower], "ms": min(ts), "all_ms": ts, "sum": fp, "top_products": kd["products"],
                          "half_size_calls": kd["half_size_calls"]}), flush=True)
        del A, B, Cm
        torch.cuda.empty_cache()
    L.check(lib.sgpr_trim())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=list(VARIANTS))
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    rows = {}
    for name in VARIANTS:
        env = dict(os.environ)
        env.pop("SGPR_GEMM_STRASSEN", None)
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", name]
        r = subprocess.run(cmd, env=env, timeout=420, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("variant %s failed (%d): %s" % (name, r.returncode, r.stderr[-2000:]))
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                d = json.loads(ln)
                rows.setdefault(tuple(d["shape"]), {})[name] = d
    print("# C -= A B^T, fp64, as potrf_rec / trsm_rec issue it; best of %d (HIP events) and spread (max - min) of the %d runs, ms" % (REPS, REPS))
    print("# off: rec_strassen3_min = 0 (two levels, the call as it was); serial: the top passes on the caller's stream; one set / two sets:")
    print("# the passes on the low-priority stream with one / two buffer sets (two sets: the shipped form).  Gain against off.")
    for (m, n, k, lower, what) in CLASSES:
        d = rows[(m, n, k, lower)]
        print("%d x %d x %d%s (%s): top products %d, half-size calls %s" % (m, n, k, " lower" if lower else "", what, d["two_sets"]["top_products"],
                                                                            d["two_sets"]["half_size_calls"]))
        for name in VARIANTS:
            x = d[name]
            print("    %-9s %9.2f (%5.2f)  %+6.2f%%   same bits as two sets: %s" % (name, x["ms"], max(x["all_ms"]) - min(x["all_ms"]),
                  100.0 * (x["ms"] - d["off"]["ms"]) / d["off"]["ms"], x["sum"] == d["two_sets"]["sum"]))


if __name__ == "__main__":
    main()
