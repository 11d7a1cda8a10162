"""The outer Strassen level's list (csrc/strassen_plan.hip: strassen_outer_plan) on the CPU: fetch what one call C -= A B^T turns into
with both levels (host code, no GPU needed) and replay it with NumPy.  Record layout: include/sympgpr_probe.h.  An outer
product (kind 5) is replayed the way the device runs it: the inner plan of its half-size product is fetched through the
existing probe (tools/strassen_plan.py) and every inner product is added to BOTH destination blocks.
`python tools/strassen2_plan.py M N K [lower] [smin] [kslab] [smin2] [kslab2]` prints the list's summary.
Used by tests/test_strassen2_plan_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import strassen_plan as sp  # noqa: E402

REC = sp.REC
SUM2, PROD2 = 4, 5
UNLIMITED = sp.UNLIMITED


def fetch_plan(m, n, k, lower=0, smin=-1, kslab=-1, smin2=-1, kslab2=-1, scratch=UNLIMITED):
    """-> int64 array (records, 16)"""
    from sympgpr_amd import _lib as L
    probe = L.load_probe_library()
    count = C.c_int(0)
    args = (m, n, k, lower, smin, kslab, smin2, kslab2, scratch)
    L.check(probe.sgpr_probe_strassen2_plan(*args, None, 0, C.byref(count)), "sgpr_probe_strassen2_plan")
    buf = (C.c_longlong * (REC * max(count.value, 1)))()
    L.check(probe.sgpr_probe_strassen2_plan(*args, buf, count.value, C.byref(count)), "sgpr_probe_strassen2_plan")
    return np.frombuffer(buf, dtype=np.int64, count=REC * count.value).reshape(-1, REC).copy()


def inner_plan(r, smin=-1, kslab=-1):
    """the inner plan of the outer product record r"""
    return sp.fetch_plan(int(r[7]), int(r[8]), int(r[9]), 0, smin, kslab)


def scratch_need(plan, smin=-1, kslab=-1):
    """doubles of scratch: inner pair (the list's own inner sums and those of the outer products' plans) + outer pair"""
    need = [0, 0, 0, 0]
    for r in plan:
        if r[0] in (sp.SUM, SUM2):
            i = (2 if r[0] == SUM2 else 0) + int(r[1])
            need[i] = max(need[i], int(r[2] * r[3]))
        elif r[0] == PROD2:
            for q in inner_plan(r, smin, kslab):
                if q[0] == sp.SUM:
                    need[int(q[1])] = max(need[int(q[1])], int(q[2] * q[3]))
    return sum(need)


def launches(plan, smin=-1, kslab=-1):
    """-> (product launches by number of destinations {1: .., 2: .., 4: ..}, inner sums, outer sums, flop of all launches)"""
    dests, inner_sums, outer_sums, flop = {1: 0, 2: 0, 4: 0}, 0, 0, 0.0
    for r in plan:
        if r[0] == SUM2:
            outer_sums += 1
        elif r[0] == sp.SUM:
            inner_sums += 1
        elif r[0] == sp.PROD:
            dests[2 if r[15] else 1] += 1
            flop += 2.0 * r[7] * r[8] * r[9]
        elif r[0] == sp.CLASSIC:
            dests[1] += 1
            flop += (1.0 if r[1] else 2.0) * r[6] * r[7] * r[8]
        elif r[0] == PROD2:
            outer = 2 if r[15] else 1
            for q in inner_plan(r, smin, kslab):
                if q[0] == sp.SUM:
                    inner_sums += 1
                elif q[0] == sp.PROD:
                    dests[outer * (2 if q[15] else 1)] += 1
                    flop += 2.0 * q[7] * q[8] * q[9]
                else:
                    dests[outer] += 1
                    flop += 2.0 * q[6] * q[7] * q[8]
    return dests, inner_sums, outer_sums, flop


def replay(plan, alpha, A, B, C0, kmax=0, smin=-1, kslab=-1):
    """run the list in order on C0 (copied).  Records of the inner level: tools/strassen_plan.replay, one at a time (the inner
    scratch does not outlive an outer product).  Outer product: P = the inner plan's replay on a zero block, added to both
    destinations -- the device adds every inner product to both directly; the sums are the same ones in the same order."""
    Cm = C0.copy()
    S = [None, None]          # outer scratch
    ops = (A, B)
    pending = []              # inner-level records wait here so that their sums reach the products that follow them

    def flush():
        nonlocal Cm
        if pending:
            Cm = sp.replay(np.array(pending), alpha, A, B, Cm, kmax)
            pending.clear()

    for r in plan:
        r = [int(v) for v in r]
        if r[0] in (sp.SUM, sp.PROD, sp.CLASSIC):
            pending.append(r)
            continue
        flush()
        if r[0] == SUM2:
            P, rows, cols = ops[r[1]], r[2], r[3]
            S[r[1]] = P[r[4]:r[4] + rows, r[5]:r[5] + cols] + r[8] * P[r[6]:r[6] + rows, r[7]:r[7] + cols]
        elif r[0] == PROD2:
            m, n, k = r[7], r[8], r[9]
            X = S[0] if r[1] else A[r[2]:r[2] + m, r[3]:r[3] + k]
            Y = S[1] if r[4] else B[r[5]:r[5] + n, r[6]:r[6] + k]
            assert X.shape == (m, k) and Y.shape == (n, k), "operand block does not have the product's extents"
            P = sp.replay(inner_plan(r, smin, kslab), 1.0, X, Y, np.zeros((m, n)), kmax)
            Cm[r[10]:r[10] + m, r[11]:r[11] + n] += alpha * r[12] * P
            if r[15]:
                Cm[r[13]:r[13] + m, r[14]:r[14] + n] += alpha * r[15] * P
        else:
            raise ValueError("unknown record kind %d" % r[0])
    flush()
    return Cm


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    m, n, k = a[:3]
    a += [-1] * (8 - len(a))
    lower = max(a[3], 0)
    p = fetch_plan(m, n, k, lower, a[4], a[5], a[6], a[7])
    d, si, so, flop = launches(p, a[4], a[5])
    full = (1.0 if lower else 2.0) * m * n * k
    print("m=%d n=%d k=%d lower=%d: records %d, product launches by destinations %s, inner sums %d, outer sums %d, scratch %d doubles, "
          "flop / classical = %.4f" % (m, n, k, lower, len(p), d, si, so, scratch_need(p, a[4], a[5]), flop / full))
