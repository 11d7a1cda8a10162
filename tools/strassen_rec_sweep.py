"""Sweep of the recursive factorisation's own Strassen thresholds (csrc/strassen_plan.hip: strassen_rec_values) on one MI355X: every
product class the n = 131072 factorisation issues, as the recursion would issue it (sgpr_probe_gemm_strassen_rec_dev), once with
the recursion's tunables at the library's values ("current": what the tree did before) and once with the candidates, on the same
seeded operands.  Tunables are read per call but the scratch is per process, so every variant is a child process of its own
(under a time limit); each prints the HIP-event times of REPS runs, and the table shows the best and the spread of each.
    python tools/strassen_rec_sweep.py > profiles/strassen_rec/sweep.txt
    python tools/strassen_rec_sweep.py --child current|candidate [--min M] [--min2 M2] [--kslab2-short K]    (one variant, JSON lines)"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import strassen_rec_plan as srp  # noqa: E402

# (m, n, k, lower, what it is at n = 131072, how many)
CLASSES = [
    (65536, 32768, 32768, 0, "trsm_rec, two levels today (control)", 1),
    (32768, 32768, 65536, 0, "SYRK square, two levels today (control)", 1),
    (65536, 16384, 16384, 0, "trsm_rec, one level today", 2),
    (32768, 16384, 16384, 0, "trsm_rec, one level today", 2),
    (16384, 16384, 65536, 0, "SYRK square, one level today", 2),
    (16384, 16384, 32768, 0, "SYRK square, one level today", 2),
    (65536, 8192, 8192, 0, "trsm_rec, classical today", 4),
    (32768, 8192, 8192, 0, "trsm_rec, classical today", 4),
    (16384, 16384, 65536, 1, "SYRK triangle, classical today", 4),
    (16384, 16384, 32768, 1, "SYRK triangle, classical today", 4),
]
REPS = 3


def child(args):
    import torch
    from sympgpr_amd import _lib as L
    lib, probe = L.load_library(), L.load_probe_library()
    L.check(lib.sgpr_set_device(0))
    if args.child == "current":
        srp.set_tunables(srp.LIBRARY)
    else:
        srp.set_tunables({"rec_strassen_min_gemm": args.min, "rec_strassen_min_syrk": args.min, "rec_strassen2_min_gemm": args.min2,
                          "rec_strassen2_min_syrk": args.min2, "rec_strassen2_kslab_short": args.kslab2_short})
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for (m, n, k, lower, _, _) in CLASSES:
        plan, cfg = srp.fetch_plan(m, n, k, lower)
        s = srp.summary(plan, cfg)
        g = torch.Generator(device="cuda").manual_seed(m + n + k)
        A = torch.rand((k, m), dtype=torch.float64, device="cuda", generator=g) - 0.5
        B = A if lower else torch.rand((k, n), dtype=torch.float64, device="cuda", generator=g) - 0.5
        Cm = torch.zeros((n, m), dtype=torch.float64, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def run():
            return probe.sgpr_probe_gemm_strassen_rec_dev(m, n, k, -1.0, p(A), m, p(B), n, 1.0, p(Cm), m, lower, None)
        L.check(run())                            # warm: clocks, code objects, the scratch allocation
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            ev[0].record()
            L.check(run())
            ev[1].record()
            torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]))
        # a fingerprint of the result after 1 + REPS updates: variants that take the same path agree bit for bit
        print(json.dumps({"shape": [m, n, k, lower], "ms": min(ts), "all_ms": ts, "sum": float(Cm.sum().item()), "outer_slab": cfg["kslab2"],
                          "products": s["products"], "outer_products": s["outer_products"], "classical": s["classical"], "sums": s["sums"],
                          "flop_ratio": s["flop"] / ((1.0 if lower else 2.0) * m * n * k)}), flush=True)
        del A, B, Cm
        torch.cuda.empty_cache()
    L.check(lib.sgpr_trim())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["current", "candidate"])
    ap.add_argument("--min", type=int, default=4096)
    ap.add_argument("--min2", type=int, default=8192)
    ap.add_argument("--kslab2-short", type=int, default=16384)
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = {}
    for name in ("current", "candidate"):
        env = dict(os.environ)
        env.pop("SGPR_GEMM_STRASSEN", None)
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", name, "--min", str(args.min),
                                                                              "--min2", str(args.min2), "--kslab2-short", str(args.kslab2_short)]
        r = subprocess.run(cmd, env=env, timeout=600, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("variant %s failed (%d): %s" % (name, r.returncode, r.stderr[-2000:]))
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                d = json.loads(ln)
                rows.setdefault(tuple(d["shape"]), {})[name] = d
    print("# C -= A B^T, fp64, as potrf_rec / trsm_rec issue it; best of %d (HIP events) and spread (max - min) of the %d runs" % (REPS, REPS))
    print("# current: the recursion's tunables at the library's values; candidate: inner threshold %d, outer threshold %d, outer slab %d for"
          % (args.min, args.min2, args.kslab2_short))
    print("# k below the library's slab.  flop: executed / classical.  A class gains if best(candidate) < best(current) by more than both spreads.")
    print("# %-32s %-42s %26s %26s %8s  %s" % ("m x n x k", "class at n = 131072", "current ms (spread) flop", "candidate ms (spread) flop",
                                                 "gain", "verdict"))
    for (m, n, k, lower, what, cnt) in CLASSES:
        d = rows[(m, n, k, lower)]
        cur, cand = d["current"], d["candidate"]
        sp = [max(x["all_ms"]) - min(x["all_ms"]) for x in (cur, cand)]
        gain = cur["ms"] - cand["ms"]
        same = cur["sum"] == cand["sum"] and cur["products"] == cand["products"]
        verdict = "same plan" if same else ("gains" if gain > sp[0] + sp[1] else "does not gain")
        print("  %-32s %-42s %10.2f (%5.2f) %6.4f %10.2f (%5.2f) %6.4f %+7.2f%%  %s"
              % ("%d x %d x %d%s" % (m, n, k, " lower" if lower else ""), "%s, x%d" % (what, cnt), cur["ms"], sp[0], cur["flop_ratio"],
                 cand["ms"], sp[1], cand["flop_ratio"], 100.0 * gain / cur["ms"], verdict))


if __name__ == "__main__":
    main()
