"""The schedule one call of the Strassen front end is executed by when its operand sums run beside the products
(csrc/strassen_plan.hip: strassen_schedule, tunable gemm_strassen_overlap) on the CPU: the call's list with the inner plans of its outer
products expanded in place, every record annotated with its stream, the scratch buffers it writes / reads and the records it waits
for (layout: include/sympgpr_probe.h).  Fetched through the fourth probe entry and replayed with NumPy in any order the
annotations allow.  No GPU needed.

The replay models what the device may do: the records of the caller's stream (products, classical launches) run in list order; a
sum is ISSUED once the records it waits for have run and the sum before it on its own stream has completed, and COMPLETES some
time between that moment and the first record that waits for it.  An issued sum poisons its buffer with NaN, the value arrives when
it completes and is computed from its operands as they are THEN -- a product that reads a buffer too early or too late, or a sum
that overwrites a buffer still in use, gives NaN or other bits than the serial replay (tools/strassen_rec_plan.py).
  order "list":  every sum is issued and completed at its place in the list
  order "early": every sum completes as soon as it can be issued
  order "late":  every sum is issued as soon as it can be and completes only when a record that waits for it is due
`python tools/strassen_schedule.py M N K [lower] [capacity]` prints the schedule's summary.
Used by tests/test_strassen_overlap_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import strassen_plan as sp  # noqa: E402
import strassen2_plan as sp2  # noqa: E402

REC = sp.REC
SREC = 32
LEVEL, STREAM, BUF_A, BUF_B, NWAIT, WAIT0 = 16, 17, 18, 19, 20, 21
SUMS = (sp.SUM, sp2.SUM2)


def fetch_schedule(m, n, k, lower=0, capacity=-1):
    """-> (int64 array (records, 32), info): the schedule of the call as the recursion would plan it, for a scratch buffer of
    `capacity` doubles (< 0: exactly the call's need).  info: "need" (doubles per region: inner A, inner B, outer A, outer B),
    "buffers" (per region), "streams" (side streams), "capacity"."""
    from sympgpr_amd import _lib as L
    probe = L.load_probe_library()
    fn = probe.sgpr_probe_strassen_schedule
    count, info = C.c_int(0), (C.c_longlong * 12)()
    L.check(fn(m, n, k, lower, capacity, info, None, 0, C.byref(count)), "sgpr_probe_strassen_schedule")
    buf = (C.c_longlong * (SREC * max(count.value, 1)))()
    L.check(fn(m, n, k, lower, capacity, info, buf, count.value, C.byref(count)), "sgpr_probe_strassen_schedule")
    sched = np.frombuffer(buf, dtype=np.int64, count=SREC * count.value).reshape(-1, SREC).copy()
    v = [int(x) for x in info]
    return sched, {"need": v[0:4], "buffers": v[4:8], "streams": v[8], "capacity": v[9]}


def waits(q):
    return [int(w) for w in q[WAIT0:WAIT0 + int(q[NWAIT])]]


def region_of(q):
    """the scratch region a sum record writes: 0 inner A, 1 inner B, 2 outer A, 3 outer B"""
    return (2 if q[0] == sp2.SUM2 else 0) + int(q[1])


def replay(sched, alpha, A, B, C0, order="list", kmax=0):
    """run the schedule on C0 (copied) in one of the orders of the module docstring; the arithmetic of every record is that of
    tools/strassen2_plan.replay, so a correct schedule gives its bits"""
    assert order in ("list", "early", "late")
    S = [[int(v) for v in q] for q in sched]
    n = len(S)
    is_sum = [q[0] in SUMS for q in S]
    header = [-1] * n                 # the outer product a level-1 record belongs to
    h = -1
    for i, q in enumerate(S):
        if q[0] == sp2.PROD2:
            h = i
        header[i] = h if q[LEVEL] == 1 else -1
    Cm = C0.copy()
    bufs = {}                         # (region, buffer) -> array
    issued, done = [False] * n, [False] * n
    queues = {}                       # side stream -> its sums in list order
    for i, q in enumerate(S):
        if is_sum[i]:
            assert q[STREAM] >= 1, "a sum on the caller's stream"
            queues.setdefault(q[STREAM], []).append(i)
        else:
            assert q[STREAM] == 0, "a product beside the caller's stream"
    head = {s: 0 for s in queues}

    def operand(i, side):
        """what record i sees as the operand of that side: the matrix itself, or under an outer product its block / outer sum"""
        if header[i] < 0:
            return (A, B)[side]
        hq = S[header[i]]
        src, r0, c0, rows = (hq[1], hq[2], hq[3], hq[7]) if side == 0 else (hq[4], hq[5], hq[6], hq[8])
        if src:
            return bufs[(2 + side, hq[BUF_A + side])]
        return (A, B)[side][r0:r0 + rows, c0:c0 + hq[9]]

    def issue(i):
        q = S[i]
        bufs[(region_of(q), q[BUF_A])] = np.full((q[2], q[3]), np.nan)
        issued[i] = True

    def complete(i):
        q = S[i]
        P = operand(i, q[1])
        rows, cols = q[2], q[3]
        bufs[(region_of(q), q[BUF_A])] = P[q[4]:q[4] + rows, q[5]:q[5] + cols] + q[8] * P[q[6]:q[6] + rows, q[7]:q[7] + cols]
        done[i] = True
        head[q[STREAM]] += 1

    def can_issue(i):
        return all(done[w] for w in waits(S[i]))

    def pump():
        """issue (and in the early order complete) whatever sums may start now"""
        moved = True
        while moved:
            moved = False
            for s, lst in queues.items():
                if head[s] >= len(lst):
                    continue
                i = lst[head[s]]
                if not issued[i] and can_issue(i):
                    issue(i)
                    moved = True
                if issued[i] and not done[i] and order == "early":
                    complete(i)
                    moved = True

    def force(i):
        """record i is needed now: complete it, and first whatever has to come before it"""
        if done[i]:
            return
        assert is_sum[i], "record %d waits for a record of the caller's stream that has not run" % i
        q = S[i]
        lst = queues[q[STREAM]]
        while lst[head[q[STREAM]]] != i:
            force(lst[head[q[STREAM]]])
        for w in waits(q):
            force(w)
        if not issued[i]:
            issue(i)
        complete(i)

    def chunks(X, Y):
        k = X.shape[1]
        if kmax <= 0 or k <= kmax:
            yield X @ Y.T
            return
        for k0 in range(0, k, kmax):
            yield X[:, k0:k0 + kmax] @ Y[:, k0:k0 + kmax].T

    outer = None                      # [header record, accumulator of the outer product]

    def flush():
        nonlocal outer
        if outer is not None:
            r, P = outer
            m, nn = r[7], r[8]
            Cm[r[10]:r[10] + m, r[11]:r[11] + nn] += alpha * r[12] * P
            if r[15]:
                Cm[r[13]:r[13] + m, r[14]:r[14] + nn] += alpha * r[15] * P
            outer = None

    for i, q in enumerate(S):
        assert all(w < i for w in waits(q)), "record %d waits for a later record" % i
        if is_sum[i]:
            if q[LEVEL] == 0:
                flush()
            if order == "list":
                for w in waits(q):
                    assert done[w], "record %d: record %d it waits for has not run in list order" % (i, w)
                issue(i)
                complete(i)
            continue
        if q[LEVEL] == 0:
            flush()
        if order != "list":
            pump()
            for w in waits(q):
                force(w)
        else:
            for w in waits(q):
                assert done[w]
        if q[0] == sp2.PROD2:
            outer = [q, np.zeros((q[7], q[8]))]
        else:
            X0, Y0 = operand(i, 0), operand(i, 1)
            # under an outer product the records add to its accumulator with factor 1 (tools/strassen2_plan.replay)
            T, a = (outer[1], 1.0) if q[LEVEL] == 1 else (Cm, alpha)
            if q[0] == sp.PROD:
                m, nn, k = q[7], q[8], q[9]
                X = bufs[(0, q[BUF_A])] if q[1] else X0[q[2]:q[2] + m, q[3]:q[3] + k]
                Y = bufs[(1, q[BUF_B])] if q[4] else Y0[q[5]:q[5] + nn, q[6]:q[6] + k]
                assert X.shape == (m, k) and Y.shape == (nn, k), "operand block does not have the product's extents"
                for part in chunks(X, Y):
                    T[q[10]:q[10] + m, q[11]:q[11] + nn] += a * q[12] * part
                    if q[15]:
                        T[q[13]:q[13] + m, q[14]:q[14] + nn] += a * q[15] * part
            elif q[0] == sp.CLASSIC:
                m, nn, k = q[6], q[7], q[8]
                for part in chunks(X0[q[2]:q[2] + m, q[3]:q[3] + k], Y0[q[4]:q[4] + nn, q[5]:q[5] + k]):
                    if q[1]:
                        part = np.tril(part)
                    T[q[9]:q[9] + m, q[10]:q[10] + nn] += a * part
            else:
                raise ValueError("unknown record kind %d" % q[0])
        done[i] = True
    flush()
    assert all(done), "a sum nothing waited for was left over"
    return Cm


def summary(sched, info):
    sums = [q for q in sched if q[0] in SUMS]
    free = sum(1 for q in sums if q[NWAIT] == 0)
    return {"records": len(sched), "sums": len(sums), "sums that wait for nothing": free, "need": info["need"],
            "buffers": info["buffers"], "streams": info["streams"], "capacity": info["capacity"]}


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    lower = a[3] if len(a) > 3 else 0
    sched, info = fetch_schedule(a[0], a[1], a[2], lower, a[4] if len(a) > 4 else -1)
    print("m=%d n=%d k=%d lower=%d: %s" % (a[0], a[1], a[2], lower, summary(sched, info)))
