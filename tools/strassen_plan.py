"""The Strassen front end's plan (csrc/strassen_plan.hip: strassen_plan) on the CPU: fetch the list of operations one call
C -= A B^T turns into (host code, no GPU needed) and replay it with NumPy.  Record layout: include/sympgpr_probe.h.
`python tools/strassen_plan.py M N K [lower] [smin] [kslab]` prints the plan's summary.
Used by tests/test_strassen_plan_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REC = 16
SUM, PROD, CLASSIC = 1, 2, 3
UNLIMITED = 2 ** 62


def fetch_plan(m, n, k, lower=0, smin=-1, kslab=-1, scratch=UNLIMITED):
    """-> int64 array (records, 16)"""
    from sympgpr_amd import _lib as L
    probe = L.load_probe_library()
    count = C.c_int(0)
    L.check(probe.sgpr_probe_strassen_plan(m, n, k, lower, smin, kslab, scratch, None, 0, C.byref(count)), "sgpr_probe_strassen_plan")
    buf = (C.c_longlong * (REC * max(count.value, 1)))()
    L.check(probe.sgpr_probe_strassen_plan(m, n, k, lower, smin, kslab, scratch, buf, count.value, C.byref(count)),
            "sgpr_probe_strassen_plan")
    return np.frombuffer(buf, dtype=np.int64, count=REC * count.value).reshape(-1, REC).copy()


def scratch_need(plan):
    """doubles of scratch the plan's sums need (A side + B side)"""
    need = [0, 0]
    for r in plan:
        if r[0] == SUM:
            need[r[1]] = max(need[r[1]], int(r[2] * r[3]))
    return need[0] + need[1]


def replay(plan, alpha, A, B, C0, kmax=0):
    """run the records in order on C0 (copied): A (m x k), B (n x k); products deeper than kmax > 0 are cut into chunks
    that each add to every destination, like the device's launches.  A CLASSIC record with lower set updates the lower
    triangle of its block only."""
    Cm = C0.copy()
    S = [None, None]
    ops = (A, B)

    def product(X, Y):
        k = X.shape[1]
        if kmax <= 0 or k <= kmax:
            yield X @ Y.T
            return
        for k0 in range(0, k, kmax):
            yield X[:, k0:k0 + kmax] @ Y[:, k0:k0 + kmax].T

    for r in plan:
        r = [int(v) for v in r]
        if r[0] == SUM:
            P, rows, cols = ops[r[1]], r[2], r[3]
            S[r[1]] = P[r[4]:r[4] + rows, r[5]:r[5] + cols] + r[8] * P[r[6]:r[6] + rows, r[7]:r[7] + cols]
        elif r[0] == PROD:
            m, n, k = r[7], r[8], r[9]
            X = S[0] if r[1] else A[r[2]:r[2] + m, r[3]:r[3] + k]
            Y = S[1] if r[4] else B[r[5]:r[5] + n, r[6]:r[6] + k]
            assert X.shape == (m, k) and Y.shape == (n, k), "operand block does not have the product's extents"
            for part in product(X, Y):
                Cm[r[10]:r[10] + m, r[11]:r[11] + n] += alpha * r[12] * part
                if r[15]:
                    Cm[r[13]:r[13] + m, r[14]:r[14] + n] += alpha * r[15] * part
        elif r[0] == CLASSIC:
            m, n, k = r[6], r[7], r[8]
            for part in product(A[r[2]:r[2] + m, r[3]:r[3] + k], B[r[4]:r[4] + n, r[5]:r[5] + k]):
                if r[1]:
                    part = np.tril(part)
                Cm[r[9]:r[9] + m, r[10]:r[10] + n] += alpha * part
        else:
            raise ValueError("unknown record kind %d" % r[0])
    return Cm


def summary(plan):
    flop = sum(2.0 * r[7] * r[8] * r[9] for r in plan if r[0] == PROD)
    flop += sum((1.0 if r[1] else 2.0) * r[6] * r[7] * r[8] for r in plan if r[0] == CLASSIC)
    sum_bytes = sum(24.0 * r[2] * r[3] for r in plan if r[0] == SUM)
    return {"sums": int((plan[:, 0] == SUM).sum()), "products": int((plan[:, 0] == PROD).sum()),
            "classical": int((plan[:, 0] == CLASSIC).sum()), "flop": flop, "sum_bytes": sum_bytes,
            "scratch_doubles": scratch_need(plan)}


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    m, n, k = a[:3]
    lower = a[3] if len(a) > 3 else 0
    p = fetch_plan(m, n, k, lower, a[4] if len(a) > 4 else -1, a[5] if len(a) > 5 else -1)
    s = summary(p)
    full = (1.0 if lower else 2.0) * m * n * k
    print("m=%d n=%d k=%d lower=%d: %s  flop / classical = %.4f" % (m, n, k, lower, s, s["flop"] / full))
