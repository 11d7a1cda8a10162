"""The list one product of the recursive factorisation turns into (csrc/strassen_plan.hip: strassen_rec_plan) on the CPU: potrf_rec /
trsm_rec give every call thresholds of their own (tunables "rec_strassen_*", outer k slab chosen from the call's k), and the
third probe entry returns the list of one call under that configuration together with the thresholds it resolved to.  Replay with
NumPy goes through tools/strassen2_plan.py with the inner threshold that holds UNDER an outer product.  No GPU needed.
`python tools/strassen_rec_plan.py M N K [lower]` prints the call's thresholds and the list's summary; `--table N` prints every
product the recursion issues at order N (the table of DESIGN 3.5).
Used by tests/test_strassen_rec_plan_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import strassen_plan as sp  # noqa: E402
import strassen2_plan as sp2  # noqa: E402

REC = sp.REC
UNLIMITED = sp.UNLIMITED
# the recursion's tunables and the values that make it plan like the library (sgpr_probe_strassen2_plan with defaults)
LIBRARY = {"rec_strassen_min_gemm": 8192, "rec_strassen_min_syrk": 8192, "rec_strassen2_min_gemm": 16384,
           "rec_strassen2_min_syrk": 16384, "rec_strassen2_kslab_short": 0, "rec_strassen_kslab": 16384, "rec_strassen2_kslab": 32768}
# ... and the shipped ones (csrc/strassen_plan.hip: REC_*)
SHIPPED = {"rec_strassen_min_gemm": 4096, "rec_strassen_min_syrk": 8192, "rec_strassen2_min_gemm": 8192,
           "rec_strassen2_min_syrk": 8192, "rec_strassen2_kslab_short": 16384, "rec_strassen_kslab": 16384, "rec_strassen2_kslab": 32768}


def set_tunables(values):
    from sympgpr_amd import _lib as L
    probe = L.load_probe_library()
    for name, v in values.items():
        L.check(probe.sgpr_probe_tune(name.encode(), float(v)), "sgpr_probe_tune")


def fetch_plan(m, n, k, lower=0, scratch=UNLIMITED):
    """-> (int64 array (records, 16), {"smin", "kslab", "smin2", "kslab2", "smin_under"} as resolved for this call)"""
    from sympgpr_amd import _lib as L
    probe = L.load_probe_library()
    count, cfg = C.c_int(0), (C.c_long * 5)()
    L.check(probe.sgpr_probe_strassen_rec_plan(m, n, k, lower, scratch, cfg, None, 0, C.byref(count)), "sgpr_probe_strassen_rec_plan")
    buf = (C.c_longlong * (REC * max(count.value, 1)))()
    L.check(probe.sgpr_probe_strassen_rec_plan(m, n, k, lower, scratch, cfg, buf, count.value, C.byref(count)),
            "sgpr_probe_strassen_rec_plan")
    plan = np.frombuffer(buf, dtype=np.int64, count=REC * count.value).reshape(-1, REC).copy()
    return plan, dict(zip(("smin", "kslab", "smin2", "kslab2", "smin_under"), (int(v) for v in cfg)))


def scratch_of_order(n):
    """doubles of scratch potrf() reserves at order n: (both levels, one level)"""
    from sympgpr_amd import _lib as L
    probe = L.load_probe_library()
    out = (C.c_ulonglong * 2)()
    L.check(probe.sgpr_probe_strassen_rec_scratch(n, out), "sgpr_probe_strassen_rec_scratch")
    return int(out[0]), int(out[1])


def replay(plan, cfg, alpha, A, B, C0):
    return sp2.replay(plan, alpha, A, B, C0, smin=cfg["smin_under"], kslab=cfg["kslab"])


def summary(plan, cfg):
    dests, inner_sums, outer_sums, flop = sp2.launches(plan, cfg["smin_under"], cfg["kslab"])
    return {"products": sum(dests.values()) - int((plan[:, 0] == sp.CLASSIC).sum()), "classical": int((plan[:, 0] == sp.CLASSIC).sum()),
            "sums": inner_sums + outer_sums, "outer_products": int((plan[:, 0] == sp2.PROD2).sum()), "dests": dests, "flop": flop,
            "scratch_doubles": sp2.scratch_need(plan, cfg["smin_under"], cfg["kslab"])}


def recursion_calls(n, la_max=57344, leaf=128):
    """(m, n, k, lower) of every product potrf_rec / trsm_rec send to the front end at order n, in order (chol.hip), down to the
    sizes at which nothing can qualify any more (halves below 2048)"""
    calls = []

    def split(n):
        n1 = (n // 2 + leaf - 1) // leaf * leaf
        return n1 - leaf if n1 >= n else n1

    def trsm(m, n):
        if n <= leaf:
            return
        n1 = split(n)
        trsm(m, n1)
        if min(m, n - n1) >= 4096:
            calls.append((m, n - n1, n1, 0))
        trsm(m, n - n1)

    def potrf(n):
        if n <= la_max:
            return
        n1 = split(n)
        potrf(n1)
        trsm(n - n1, n1)
        calls.append((n - n1, n - n1, n1, 1))
        potrf(n - n1)

    potrf(n)
    return calls


if __name__ == "__main__":
    if sys.argv[1] == "--table":
        seen = {}
        for c in recursion_calls(int(sys.argv[2])):
            seen[c] = seen.get(c, 0) + 1
        for (m, n, k, lower), cnt in seen.items():
            p, cfg = fetch_plan(m, n, k, lower)
            s = summary(p, cfg)
            full = (1.0 if lower else 2.0) * m * n * k
            print("%6d x %6d x %6d %s x%d: outer slab %6d, products %4d (outer %2d), classical %2d, sums %4d, scratch %10d, flop / classical %.4f"
                  % (m, n, k, "lower" if lower else "     ", cnt, cfg["kslab2"], s["products"], s["outer_products"], s["classical"], s["sums"],
                     s["scratch_doubles"], s["flop"] / full))
        print("reserved at this order (both levels, one level): %d, %d doubles" % scratch_of_order(int(sys.argv[2])))
    else:
        a = [int(v) for v in sys.argv[1:]]
        lower = a[3] if len(a) > 3 else 0
        p, cfg = fetch_plan(a[0], a[1], a[2], lower)
        print("m=%d n=%d k=%d lower=%d: thresholds %s\n  %s" % (a[0], a[1], a[2], lower, cfg, summary(p, cfg)))
