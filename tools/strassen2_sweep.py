"""Sweep of the outer Strassen level (csrc/strassen.hip) on one MI355X: C -= A B^T through the front end with two levels, with
one level and through the classical launch, on the same seeded operands -- the products of the n = 131072 factorisation that
take the outer level, and the candidates for a lower outer threshold.  SGPR_GEMM_STRASSEN and the tunables are read once per
process, so every variant is a child process of its own (under a time limit); each prints best-of-REPS HIP-event times.
    python tools/strassen2_sweep.py > profiles/strassen2/sweep.txt
    python tools/strassen2_sweep.py --child two|one|classical [--min2 M] [--kslab2 K]      (one variant, JSON lines)"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (m, n, k, lower): the trsm_rec product and the SYRK square of the flagship step, then the threshold candidates
SHAPES = [(65536, 32768, 32768, 0), (32768, 32768, 65536, 0), (65536, 16384, 16384, 0), (32768, 32768, 16384, 0)]
# outer (min half-size, k slab) per variant; a slab of 16384 (quarter k of 4096) lets k = 16384 in.  65536 x 16384 x 16384 can
# take the outer level under no setting of the outer tunables: its quarters of 4096 in n are below the inner threshold.
VARIANTS = [("two", 16384, 32768), ("two", 16384, 16384), ("one", 0, 0), ("classical", 0, 0)]
REPS = 2


def child(args):
    import torch
    from sympgpr_amd import _lib as L
    lib, probe = L.load_library(), L.load_probe_library()
    L.check(lib.sgpr_set_device(0))
    if args.child == "two":
        L.check(probe.sgpr_probe_tune(b"gemm_strassen2_min", float(args.min2)))
        L.check(probe.sgpr_probe_tune(b"gemm_strassen2_kslab", float(args.kslab2)))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for (m, n, k, lower) in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(m + n + k)
        A = torch.rand((k, m), dtype=torch.float64, device="cuda", generator=g) - 0.5
        B = torch.rand((k, n), dtype=torch.float64, device="cuda", generator=g) - 0.5
        Cm = torch.zeros((n, m), dtype=torch.float64, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def run():
            if args.child == "classical":
                return lib.sgpr_gemm_nt_dev(m, n, k, -1.0, p(A), m, p(B), n, 1.0, p(Cm), m, lower, 0, None)
            return probe.sgpr_probe_gemm_strassen_dev(m, n, k, -1.0, p(A), m, p(B), n, 1.0, p(Cm), m, lower, None)
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
        print(json.dumps({"shape": [m, n, k, lower], "ms": min(ts), "all_ms": ts, "sum": float(Cm.sum().item())}), flush=True)
        del A, B, Cm
        torch.cuda.empty_cache()
    L.check(lib.sgpr_trim())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["two", "one", "classical"])
    ap.add_argument("--min2", type=int, default=16384)
    ap.add_argument("--kslab2", type=int, default=32768)
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = {}
    for (name, min2, kslab2) in VARIANTS:
        env = dict(os.environ)
        env.pop("SGPR_GEMM_STRASSEN", None)
        if name != "classical":
            env["SGPR_GEMM_STRASSEN"] = "1" if name == "one" else "2"
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", name,
                                                                              "--min2", str(min2), "--kslab2", str(kslab2)]
        r = subprocess.run(cmd, env=env, timeout=600, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("variant %s %d %d failed (%d): %s" % (name, min2, kslab2, r.returncode, r.stderr[-2000:]))
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                d = json.loads(ln)
                rows.setdefault(tuple(d["shape"]), {})[(name, min2, kslab2)] = d
    print("# C -= A B^T, fp64, best of %d (HIP events): classical launch, one Strassen level, and two levels with the outer" % REPS)
    print("# thresholds (min half-size of m and n / k slab) of each column")
    hdr = ["%s %d/%d" % v if v[0] == "two" else v[0] for v in VARIANTS]
    print("# %-28s " % "m x n x k" + " ".join("%18s" % h for h in hdr) + "   gain of each 'two' over one level")
    for shape, d in rows.items():
        one = d[("one", 0, 0)]["ms"]
        cells = ["%10.2f ms %5.1f" % (d[v]["ms"], 2.0 * shape[0] * shape[1] * shape[2] / d[v]["ms"] / 1e9) for v in VARIANTS]
        gains = ["%+5.2f%%" % (100.0 * (one - d[v]["ms"]) / one) for v in VARIANTS if v[0] == "two"]
        print("  %-28s " % ("%d x %d x %d" % shape[:3]) + " ".join(cells) + "   " + " ".join(gains))
    print("# (second figure of each cell: classical-equivalent TFLOP/s)")


if __name__ == "__main__":
    main()
