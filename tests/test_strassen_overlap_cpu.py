"""The schedule by which the Strassen front end runs its operand sums beside the products (sympgpr_amd/csrc/strassen_plan.hip:
strassen_schedule, host code; the device path executes exactly its records): the call's list, inner plans expanded, every record
annotated with its stream, its scratch buffers and the records it waits for.  Fetched through the fourth probe entry
(sgpr_probe_strassen_schedule) with the recursion's tunables scaled down as in tests/test_strassen_rec_plan_cpu.py, and replayed in
numpy (tools/strassen_schedule.py) in three orders the annotations allow: list order, every sum as early as its waits allow, every
sum as late as its consumer allows.  An issued sum poisons its buffer with NaN until it completes, so a missing edge -- a product
reading a buffer before its sum is there or after the next sum has started on it -- shows as NaN or as other bits.  No GPU needed.

All three orders must give the BITS of the serial replay of the plan (tools/strassen_rec_plan.py); that result is held to
C - A B^T by the rule of the plan tests: 1e-13 relative to max|C - A B^T| (operands uniform in [-1, 1], k <= 2304: classical
rounding about sqrt(k) u max|C| ~ 5e-15 relative, a factor 3 per Strassen level (Higham 23.2.2): 9 x 5e-15 stays below 1e-13).

Capacities: the call's need (no second buffer anywhere), the need plus the inner pair (second buffers for the inner regions only),
twice the need (every region)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import strassen_plan as sp  # noqa: E402
import strassen2_plan as sp2  # noqa: E402
import strassen_rec_plan as srp  # noqa: E402
import strassen_schedule as ss  # noqa: E402

# tests/test_strassen_rec_plan_cpu.py: scaled down by 32
SMALL = {"rec_strassen_min_gemm": 128, "rec_strassen_min_syrk": 128, "rec_strassen2_min_gemm": 256, "rec_strassen2_min_syrk": 256,
         "rec_strassen2_kslab_short": 512, "rec_strassen_kslab": 512, "rec_strassen2_kslab": 1024}
OVERLAP_DEFAULTS = {"gemm_strassen_overlap_slack": -1, "gemm_strassen_overlap_streams": 1}

SHAPES = [
    (2048, 1024, 1024, 0, "both levels, long slab"),
    (1024, 1024, 2304, 0, "two slabs and an inner-level remainder"),
    (2048, 2048, 1024, 1, "lower: splits twice, classical triangles beside Strassen squares"),
    (2048, 256, 256, 0, "one level only"),
]
CAPACITIES = ["need", "inner", "twice"]


@pytest.fixture
def tunables():
    """set tunables for one test, the shipped values afterwards"""
    yield srp.set_tunables
    srp.set_tunables(dict(srp.SHIPPED, **OVERLAP_DEFAULTS))


_cases = {}


def case(m, n, k, lower):
    """operands, the plan, its serial replay and the exact product, computed once per shape (the tunables are SMALL here)"""
    key = (m, n, k, lower)
    if key not in _cases:
        rng = np.random.default_rng(m + n + k + lower)
        A = rng.uniform(-1, 1, (m, k))
        B = A if lower else rng.uniform(-1, 1, (n, k))
        C0 = rng.uniform(-1, 1, (m, n))
        plan, cfg = srp.fetch_plan(m, n, k, lower)
        serial = srp.replay(plan, cfg, -1.0, A, B, C0)
        P = A @ B.T
        ref = C0 - (np.tril(P) if lower else P)
        for v in (A, B, C0, serial, ref):
            v.setflags(write=False)
        _cases[key] = (A, B, C0, plan, cfg, serial, ref)
    return _cases[key]


def capacity_of(which, need):
    return {"need": sum(need), "inner": sum(need) + need[0] + need[1], "twice": 2 * sum(need)}[which]


def fetch(m, n, k, lower, which):
    _, info = ss.fetch_schedule(m, n, k, lower, -1)
    return ss.fetch_schedule(m, n, k, lower, capacity_of(which, info["need"]))


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("which", CAPACITIES)
@pytest.mark.parametrize("m,n,k,lower,why", SHAPES)
def test_every_legal_order_gives_the_serial_bits(tunables, m, n, k, lower, why, which, streams):
    tunables(dict(SMALL, gemm_strassen_overlap_slack=-1, gemm_strassen_overlap_streams=streams))
    A, B, C0, plan, cfg, serial, ref = case(m, n, k, lower)
    assert np.abs(serial - ref).max() <= 1e-13 * np.abs(ref).max(), why
    sched, info = fetch(m, n, k, lower, which)
    assert info["streams"] == streams
    for order in ("list", "early", "late"):
        got = ss.replay(sched, -1.0, A, B, C0, order)
        assert not np.isnan(got).any(), (why, which, order)
        assert np.array_equal(got.view(np.uint64), serial.view(np.uint64)), (why, which, order)


@pytest.mark.parametrize("which", CAPACITIES)
@pytest.mark.parametrize("m,n,k,lower,why", SHAPES)
def test_records_are_the_plans_and_buffers_fit(tunables, m, n, k, lower, why, which):
    tunables(dict(SMALL, **OVERLAP_DEFAULTS))
    plan, cfg = srp.fetch_plan(m, n, k, lower)
    sched, info = fetch(m, n, k, lower, which)
    need, nbuf = info["need"], info["buffers"]
    # stripped of the annotations: the call's list, and behind every outer product its inner plan
    top = sched[sched[:, ss.LEVEL] == 0]
    assert np.array_equal(top[:, :ss.REC], plan), why
    at = 0
    while at < len(sched):
        q = sched[at]
        at += 1
        if q[0] != sp2.PROD2:
            continue
        inner = sp2.inner_plan(q[:ss.REC], cfg["smin_under"], cfg["kslab"])
        assert np.array_equal(sched[at:at + len(inner), :ss.REC], inner), why
        assert (sched[at:at + len(inner), ss.LEVEL] == 1).all()
        at += len(inner)
    assert (sched[:, ss.LEVEL] == 1).sum() == len(sched) - len(plan)
    # the scratch: what the plan needs, region by region, and second buffers only out of the capacity that is left
    assert sum(need) == srp.summary(plan, cfg)["scratch_doubles"]
    assert all(b in (1, 2) for b in nbuf)
    assert sum(v * b for v, b in zip(need, nbuf)) <= info["capacity"] == capacity_of(which, need)
    if which == "need":
        assert nbuf == [1, 1, 1, 1]
    elif which == "inner":
        assert nbuf == [2 if need[0] else 1, 2 if need[1] else 1, 1, 1]
    else:
        assert nbuf == [2 if v else 1 for v in need]
    # no record names a buffer its region does not have
    for q in sched:
        if q[0] in ss.SUMS:
            assert 0 <= q[ss.BUF_A] < nbuf[ss.region_of(q)]
        elif q[0] == sp2.PROD2:
            assert -1 <= q[ss.BUF_A] < nbuf[2] and -1 <= q[ss.BUF_B] < nbuf[3]
            assert (q[ss.BUF_A] >= 0) == bool(q[1]) and (q[ss.BUF_B] >= 0) == bool(q[4])
        elif q[0] == sp.PROD:
            assert -1 <= q[ss.BUF_A] < nbuf[0] and -1 <= q[ss.BUF_B] < nbuf[1]
            assert (q[ss.BUF_A] >= 0) == bool(q[1]) and (q[ss.BUF_B] >= 0) == bool(q[4])
    # with two buffers the sums of a region alternate
    for region in range(4):
        bufs = [int(q[ss.BUF_A]) for q in sched if q[0] in ss.SUMS and ss.region_of(q) == region]
        assert bufs == [i % nbuf[region] for i in range(len(bufs))]


@pytest.mark.parametrize("m,n,k,lower,why", SHAPES)
def test_slack_zero_means_single_buffers(tunables, m, n, k, lower, why):
    tunables(dict(SMALL, gemm_strassen_overlap_slack=0, gemm_strassen_overlap_streams=1))
    sched, info = fetch(m, n, k, lower, "twice")
    assert info["buffers"] == [1, 1, 1, 1]
    assert all(q[ss.BUF_A] == 0 for q in sched if q[0] in ss.SUMS)
    # ... and a cap between the inner and the outer pair's size stops where the slack ends
    need = info["need"]
    tunables(dict(SMALL, gemm_strassen_overlap_slack=need[0] + need[1], gemm_strassen_overlap_streams=1))
    _, info = fetch(m, n, k, lower, "twice")
    assert info["buffers"] == [2 if need[0] else 1, 2 if need[1] else 1, 1, 1]


def test_single_buffers_still_free_the_other_side(tunables):
    """one buffer per region: inside a seven-product slab the B sum of M3 waits for M1 only (M2 reads the A scratch and a raw B
    block), so it can run under M2; with second buffers the sums of M2 and M3 wait for nothing at all"""
    tunables(dict(SMALL, **OVERLAP_DEFAULTS))
    sched, info = fetch(2048, 256, 256, 0, "need")
    kinds = [int(q[0]) for q in sched]
    assert kinds[:7] == [sp.SUM, sp.SUM, sp.PROD, sp.SUM, sp.PROD, sp.SUM, sp.PROD]
    assert ss.waits(sched[3]) == [2] and ss.waits(sched[5]) == [2]       # sum A of M2, sum B of M3: behind M1
    assert sorted(ss.waits(sched[4])) == [3] and sorted(ss.waits(sched[6])) == [5]
    sched, info = fetch(2048, 256, 256, 0, "twice")
    assert ss.waits(sched[3]) == [] and ss.waits(sched[5]) == []
    assert ss.summary(sched, info)["sums that wait for nothing"] == 4


def test_capacity_below_the_need_is_refused(tunables):
    tunables(dict(SMALL, **OVERLAP_DEFAULTS))
    _, info = ss.fetch_schedule(2048, 1024, 1024, 0, -1)
    with pytest.raises(Exception):
        ss.fetch_schedule(2048, 1024, 1024, 0, sum(info["need"]) - 1)
