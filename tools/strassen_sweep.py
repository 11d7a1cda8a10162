"""Size sweep of the Strassen front end (csrc/strassen.hip) against the classical launch on one MI355X: C -= A B^T for
square and 2:1 products, both paths on the same operands, best of REPS runs each (HIP events on the launch stream).
The threshold tunable is lowered so that every listed shape qualifies; `adds` is the front end's time outside its MFMA
launches (the ten operand sums per k slab and the launch gaps), from the per-launch profile window of the same run.
    python tools/strassen_sweep.py [--max-half 32768] > profiles/strassen/sweep.txt"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(8192, 8192, 8192), (16384, 8192, 8192), (16384, 16384, 8192), (16384, 16384, 16384), (32768, 16384, 16384),
          (32768, 32768, 16384), (32768, 32768, 32768), (65536, 32768, 32768), (65536, 65536, 16384)]
REPS = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-half", type=int, default=32768)
    args = ap.parse_args()
    import torch
    from sympgpr_amd import _lib as L
    import strassen_plan as sp
    lib, probe = L.load_library(), L.load_probe_library()
    L.check(lib.sgpr_set_device(0))
    L.check(probe.sgpr_probe_tune(b"gemm_strassen_min", 2048.0))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    print("# C -= A B^T, fp64, classical launch vs one Strassen level (7 products, 10 operand sums per k slab of 16384)")
    print("# %-22s %10s %8s %10s %8s %7s %9s %9s %9s" % ("m x n x k", "class ms", "TF/s", "strass ms", "TF/s eq", "gain", "adds ms", "adds GB", "adds TB/s"))
    for (m, n, k) in SHAPES:
        if max(m, n) // 2 > args.max_half:
            continue
        g = torch.Generator(device="cuda").manual_seed(m + n + k)
        A = torch.rand((k, m), dtype=torch.float64, device="cuda", generator=g) - 0.5
        B = torch.rand((k, n), dtype=torch.float64, device="cuda", generator=g) - 0.5
        Cm = torch.zeros((n, m), dtype=torch.float64, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def classical():
            return lib.sgpr_gemm_nt_dev(m, n, k, -1.0, p(A), m, p(B), n, 1.0, p(Cm), m, 0, 0, None)

        def strassen():
            return probe.sgpr_probe_gemm_strassen_dev(m, n, k, -1.0, p(A), m, p(B), n, 1.0, p(Cm), m, 0, None)

        def best(fn):
            ts = []
            for _ in range(REPS):
                torch.cuda.synchronize()
                ev[0].record()
                L.check(fn())
                ev[1].record()
                torch.cuda.synchronize()
                ts.append(ev[0].elapsed_time(ev[1]))
            return min(ts)
        L.check(classical())                      # warm: clocks, code objects
        t_c = best(classical)
        L.check(strassen())                       # warm: the scratch allocation happens here
        t_s = best(strassen)
        prof = np.zeros(12)
        L.check(lib.sgpr_profile_begin())
        torch.cuda.synchronize()
        ev[0].record()
        L.check(strassen())
        ev[1].record()
        torch.cuda.synchronize()
        L.check(lib.sgpr_profile_end(L.dptr(prof)))
        adds_ms = ev[0].elapsed_time(ev[1]) - (prof[2] + prof[5] + prof[10])
        plan = sp.fetch_plan(m, n, k, 0, smin=2048)
        gb = sp.summary(plan)["sum_bytes"] / 1e9
        flop = 2.0 * m * n * k
        print("  %-22s %10.2f %8.2f %10.2f %8.2f %6.1f%% %9.2f %9.2f %9.2f" % (
            "%d x %d x %d" % (m, n, k), t_c, flop / t_c / 1e9, t_s, flop / t_s / 1e9, 100.0 * (t_c - t_s) / t_c,
            adds_ms, gb, gb / max(adds_ms, 1e-9)), flush=True)
        del A, B, Cm
        torch.cuda.empty_cache()
    L.check(lib.sgpr_trim())


if __name__ == "__main__":
    main()
