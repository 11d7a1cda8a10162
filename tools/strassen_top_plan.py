"""The top Strassen level of the recursion's largest products (csrc/strassen_plan.hip: strassen_top_plan) on the CPU: fetch the list one
call of potrf_rec / trsm_rec turns into and replay it with NumPy.  Record layout: include/sympgpr_probe.h (kinds 6 - 10).  A top
product (kind 8) is replayed the way the device runs it: its half-size call's list is fetched under the thresholds the record
carries (sgpr_probe_strassen_cfg_plan) and replayed through tools/strassen2_plan.py into a zeroed temporary, which the
accumulate record (kind 9) then adds to its blocks of C.  No GPU needed.
`python tools/strassen_top_plan.py M N K [lower]` prints the list's summary; `--order N` the qualifying calls of the recursion
at order N and the scratch potrf() reserves.
Used by tests/test_strassen_top_plan_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import strassen_plan as sp  # noqa: E402
import strassen2_plan as sp2  # noqa: E402
import strassen_rec_plan as srp  # noqa: E402

REC = sp.REC
SUM3, ZERO3, PROD3, ACC3, PASS3 = 6, 7, 8, 9, 10
UNLIMITED = sp.UNLIMITED
# the shipped values (csrc/strassen_plan.hip: REC_SMIN3, REC_KSLAB3, REC_KSLAB3_SHORT)
SHIPPED = {"rec_strassen3_min": 16384, "rec_strassen3_kslab": 65536, "rec_strassen3_kslab_short": 32768}
set_tunables = srp.set_tunables


def _fetch(name, *args):
    from sympgpr_amd import _lib as L
    fn = getattr(L.load_probe_library(), name)
    count = C.c_int(0)
    L.check(fn(*args, None, 0, C.byref(count)), name)
    buf = (C.c_longlong * (REC * max(count.value, 1)))()
    L.check(fn(*args, buf, count.value, C.byref(count)), name)
    return np.frombuffer(buf, dtype=np.int64, count=REC * count.value).reshape(-1, REC).copy()


def fetch_plan(m, n, k, lower=0, scratch=UNLIMITED):
    """-> int64 array (records, 16): the top list of one call"""
    return _fetch("sgpr_probe_strassen_top_plan", m, n, k, lower, scratch)


def cfg_plan(m, n, k, lower, cfg):
    """the list (kinds 1 - 5) of one front-end call under the five thresholds a kind-8 / kind-10 record carries"""
    return _fetch("sgpr_probe_strassen_cfg_plan", m, n, k, lower, (C.c_long * 5)(*[int(v) for v in cfg]))


def scratch_of_order(n):
    """doubles of top-level scratch potrf() reserves at order n: (one buffer set, two)"""
    from sympgpr_amd import _lib as L
    out = (C.c_ulonglong * 2)()
    L.check(L.load_probe_library().sgpr_probe_strassen_top_scratch(n, out), "sgpr_probe_strassen_top_scratch")
    return int(out[0]), int(out[1])


def scratch_need(plan):
    """doubles of one buffer set: T + A side + B side"""
    need = [0, 0, 0]
    for r in plan:
        if r[0] == ZERO3:
            need[0] = max(need[0], int(r[1] * r[2]))
        elif r[0] == SUM3:
            need[1 + int(r[1])] = max(need[1 + int(r[1])], int(r[2] * r[3]))
    return sum(need)


def half_size_calls(plan):
    """(m, n, k) of every top product's half-size call"""
    return [(int(r[7]), int(r[8]), int(r[9])) for r in plan if r[0] == PROD3]


def _front_end(m, n, k, lower, cfg, alpha, A, B, C0):
    cfg = [int(v) for v in cfg]
    return sp2.replay(cfg_plan(m, n, k, lower, cfg), alpha, A, B, C0, smin=cfg[4], kslab=cfg[1])


def replay(plan, alpha, A, B, C0):
    """run the list in order on C0 (copied)"""
    Cm = C0.copy()
    S = [None, None]
    T = None
    ops = (A, B)
    for r in plan:
        r = [int(v) for v in r]
        if r[0] == SUM3:
            P, rows, cols = ops[r[1]], r[2], r[3]
            S[r[1]] = P[r[4]:r[4] + rows, r[5]:r[5] + cols] + r[8] * P[r[6]:r[6] + rows, r[7]:r[7] + cols]
        elif r[0] == ZERO3:
            T = np.zeros((r[1], r[2]))
        elif r[0] == PROD3:
            m, n, k = r[7], r[8], r[9]
            X = S[0] if r[1] else A[r[2]:r[2] + m, r[3]:r[3] + k]
            Y = S[1] if r[4] else B[r[5]:r[5] + n, r[6]:r[6] + k]
            assert X.shape == (m, k) and Y.shape == (n, k) and T.shape == (m, n), "a block does not have the product's extents"
            T = _front_end(m, n, k, 0, r[10:15], 1.0, X, Y, T)
        elif r[0] == ACC3:
            rows, cols = r[1], r[2]
            assert T.shape == (rows, cols)
            Cm[r[3]:r[3] + rows, r[4]:r[4] + cols] += alpha * r[5] * T
            if r[8]:
                Cm[r[6]:r[6] + rows, r[7]:r[7] + cols] += alpha * r[8] * T
        elif r[0] == PASS3:
            lower, m, n, k = r[1], r[6], r[7], r[8]
            blk = Cm[r[9]:r[9] + m, r[10]:r[10] + n]
            blk[...] = _front_end(m, n, k, lower, r[11:16], alpha, A[r[2]:r[2] + m, r[3]:r[3] + k], B[r[4]:r[4] + n, r[5]:r[5] + k], blk)
        else:
            raise ValueError("unknown record kind %d" % r[0])
    return Cm


def summary(plan):
    kd = {name: int((plan[:, 0] == v).sum()) for name, v in (("sums", SUM3), ("zeros", ZERO3), ("products", PROD3), ("accs", ACC3),
                                                               ("pass", PASS3))}
    kd["half_size_calls"] = sorted(set(half_size_calls(plan)))
    kd["scratch_doubles"] = scratch_need(plan)
    return kd


def recursion_calls(n, la_max=57344, leaf=128, floor=4096):
    """(m, n, k, lower) of every product potrf_rec / trsm_rec issue at order n (chol.hip), in order, with min(m, n) >= floor"""
    calls = []

    def split(n):
        n1 = (n // 2 + leaf - 1) // leaf * leaf
        return n1 - leaf if n1 >= n else n1

    def trsm(m, n):
        if n <= leaf:
            return
        n1 = split(n)
        trsm(m, n1)
        if min(m, n - n1) >= floor:
            calls.append((m, n - n1, n1, 0))
        trsm(m, n - n1)

    def potrf(n):
        if n <= leaf or (4 * leaf < n <= la_max):
            return
        n1 = split(n)
        potrf(n1)
        trsm(n - n1, n1)
        if n - n1 >= floor:
            calls.append((n - n1, n - n1, n1, 1))
        potrf(n - n1)

    potrf(n)
    return calls


def qualifying_calls(order, la_max=57344, floor=4096):
    """the calls of the recursion at that order whose list holds a top product"""
    return [c for c in recursion_calls(order, la_max, floor=floor) if (fetch_plan(*c)[:, 0] == PROD3).any()]


if __name__ == "__main__":
    if sys.argv[1] == "--order":
        n = int(sys.argv[2])
        for c in qualifying_calls(n):
            print("%6d x %6d x %6d %s: %s" % (c[0], c[1], c[2], "lower" if c[3] else "     ", summary(fetch_plan(*c))))
        print("top scratch reserved at this order (one set, two sets): %d, %d doubles" % scratch_of_order(n))
    else:
        a = [int(v) for v in sys.argv[1:]]
        print(summary(fetch_plan(a[0], a[1], a[2], a[3] if len(a) > 3 else 0)))
