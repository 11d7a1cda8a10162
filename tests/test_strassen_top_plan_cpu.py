"""The top Strassen level of the recursion's largest products (sympgpr_amd/csrc/strassen_plan.hip: strassen_top_plan, host code): the list
of one call comes through sgpr_probe_strassen_top_plan and is replayed in numpy (tools/strassen_top_plan.py), the half-size and
pass-through calls of that list through the lists the front end gives them (sgpr_probe_strassen_cfg_plan).  No GPU needed: the
device path executes exactly this list.

Everything is scaled down by 32 as in tests/test_strassen_rec_plan_cpu.py (inner threshold 128, outer 256, slabs 512 / 1024 / 512),
the top level to a threshold of 512 with slabs of 2048 / 1024; the divisibility rules (m % 2048, n % 1024) are not scaled.

Tolerance: operands uniform in [-1, 1]; a classical product of depth k rounds to about sqrt(k) u max|C| relative to max|C|, and
every Strassen level multiplies the constant by at most 3 (Higham 23.2.2), 27 for three levels.  The bound used is
27 sqrt(k) eps with eps = 2 u, relative to max|C - A B^T|: 2.7e-13 at k = 2048."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import strassen2_plan as sp2  # noqa: E402
import strassen_rec_plan as srp  # noqa: E402
import strassen_top_plan as stp  # noqa: E402

SMALL = {"rec_strassen_min_gemm": 128, "rec_strassen_min_syrk": 128, "rec_strassen2_min_gemm": 256, "rec_strassen2_min_syrk": 256,
         "rec_strassen2_kslab_short": 512, "rec_strassen_kslab": 512, "rec_strassen2_kslab": 1024,
         "rec_strassen3_min": 512, "rec_strassen3_kslab": 2048, "rec_strassen3_kslab_short": 1024}
SHIPPED = dict(srp.SHIPPED, **stp.SHIPPED)
# 65536 x 32768 x 32768: T 32768 x 16384, A side 32768 x 16384, B side 16384 x 16384 (the lower update's square needs as much)
NEED_131072 = 32768 * 16384 + (32768 + 16384) * 16384


@pytest.fixture
def tunables():
    yield stp.set_tunables
    stp.set_tunables(SHIPPED)


def tol(k):
    return 27.0 * np.sqrt(k) * np.finfo(float).eps


def operands(m, n, k, seed, same=False):
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1, 1, (m, k))
    B = A if same else rng.uniform(-1, 1, (n, k))
    return A, B, rng.uniform(-1, 1, (m, n))


def kinds(plan):
    return tuple(int((plan[:, 0] == v).sum()) for v in (stp.SUM3, stp.ZERO3, stp.PROD3, stp.ACC3, stp.PASS3))


def test_every_level_applies(tunables):
    tunables(SMALL)
    m, n, k = 4096, 2048, 2048
    plan = stp.fetch_plan(m, n, k, 0)
    assert kinds(plan) == (10, 7, 7, 7, 0)
    assert stp.half_size_calls(plan) == [(2048, 1024, 1024)] * 7
    assert stp.scratch_need(plan) == 2048 * 1024 + (2048 + 1024) * 1024
    # each half-size call takes the two levels below: seven outer products, nothing classical
    for r in plan[plan[:, 0] == stp.PROD3]:
        assert [int(v) for v in r[10:15]] == [128, 512, 256, 1024, 128]
        half = stp.cfg_plan(2048, 1024, 1024, 0, r[10:15])
        assert int((half[:, 0] == sp2.PROD2).sum()) == 7 and int((half[:, 0] == 3).sum()) == 0
    # the order of the records of one product: its sums, the zeroing, the product, the accumulation
    order = [int(v) for v in plan[:5, 0]]
    assert order == [stp.SUM3, stp.SUM3, stp.ZERO3, stp.PROD3, stp.ACC3]
    A, B, C0 = operands(m, n, k, 1)
    ref = C0 - A @ B.T
    got = stp.replay(plan, -1.0, A, B, C0)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("4096 x 2048 x 2048: %.3e (bound %.3e)" % (err, tol(k)))
    assert err <= tol(k)


def test_remainder_of_k_passes_through_at_its_offset(tunables):
    tunables(SMALL)
    m, n, k = 4096, 2048, 2048 + 512
    plan = stp.fetch_plan(m, n, k, 0)
    assert kinds(plan) == (10, 7, 7, 7, 1)
    last = [int(v) for v in plan[-1]]
    assert last[:11] == [stp.PASS3, 0, 0, 2048, 0, 2048, m, n, 512, 0, 0]
    assert last[11:16] == [int(v) for v in srp.fetch_plan(m, n, 512, 0)[1].values()]
    A, B, C0 = operands(m, n, k, 2)
    ref = C0 - A @ B.T
    got = stp.replay(plan, -1.0, A, B, C0)
    assert np.abs(got - ref).max() <= tol(k) * np.abs(ref).max()
    # a k between the short and the long slab takes the short one
    plan = stp.fetch_plan(m, n, 1536, 0)
    assert kinds(plan) == (10, 7, 7, 7, 1) and stp.half_size_calls(plan)[0] == (2048, 1024, 512) and plan[-1][8] == 512


def test_lower_update_splits_around_its_square(tunables):
    tunables(SMALL)
    n, k = 4096, 2048
    plan = stp.fetch_plan(n, n, k, 1)
    assert kinds(plan) == (10, 7, 7, 7, 2)
    first, last = [int(v) for v in plan[0]], [int(v) for v in plan[-1]]
    assert first[:11] == [stp.PASS3, 1, 0, 0, 0, 0, 2048, 2048, k, 0, 0]
    assert last[:11] == [stp.PASS3, 1, 2048, 0, 2048, 0, 2048, 2048, k, 2048, 2048]
    # the two halves keep the lists the whole call gave them: the thresholds of a lower update with this k
    want = [int(v) for v in srp.fetch_plan(n, n, k, 1)[1].values()]
    assert first[11:16] == want and last[11:16] == want
    assert stp.half_size_calls(plan) == [(1024, 1024, 1024)] * 7
    A, _, C0 = operands(n, n, k, 3, same=True)
    ref = C0 - np.tril(A @ A.T)
    got = stp.replay(plan, -1.0, A, A, C0)
    assert np.abs(got - ref).max() <= tol(k) * np.abs(ref).max()
    assert np.array_equal(np.triu(got, 1), np.triu(C0, 1))


@pytest.mark.parametrize("m,n,k,lower,values,why", [
    (4096, 2048, 512, 0, SMALL, "k below the short top slab"),
    (3072, 2048, 2048, 0, SMALL, "m no multiple of 2048"),
    (4096, 1536, 2048, 0, SMALL, "n no multiple of 1024"),
    (4096, 2048, 2048, 0, dict(SMALL, rec_strassen3_min=2048), "n / 2 below the threshold"),
    (4096, 2048, 2048, 0, dict(SMALL, rec_strassen3_min=0), "the level is off"),
    (2048, 2048, 2048, 1, SMALL, "a lower update whose square is 1024 x 1024: halves of 512 are multiples of neither"),
])
def test_a_call_that_does_not_qualify_is_the_pass_through_record_alone(tunables, m, n, k, lower, values, why):
    tunables(values)
    plan = stp.fetch_plan(m, n, k, lower)
    assert len(plan) == 1, why
    r = [int(v) for v in plan[0]]
    assert r[:11] == [stp.PASS3, lower, 0, 0, 0, 0, m, n, k, 0, 0], why
    # ... with the thresholds the recursion gave this call before, so its list is the one it was
    cfg = srp.fetch_plan(m, n, k, lower)
    assert r[11:16] == [int(v) for v in cfg[1].values()]
    assert np.array_equal(stp.cfg_plan(m, n, k, lower, r[11:16]), cfg[0])


def test_shipped_values_take_exactly_the_two_largest_products():
    stp.set_tunables(SHIPPED)
    assert stp.qualifying_calls(131072) == [(65536, 32768, 32768, 0), (65536, 65536, 65536, 1)]
    trsm = stp.fetch_plan(65536, 32768, 32768, 0)
    assert kinds(trsm) == (10, 7, 7, 7, 0) and stp.half_size_calls(trsm) == [(32768, 16384, 16384)] * 7
    low = stp.fetch_plan(65536, 65536, 65536, 1)
    assert kinds(low) == (10, 7, 7, 7, 2) and stp.half_size_calls(low) == [(16384, 16384, 32768)] * 7
    # the half-size calls are planned as the recursion plans products of that shape today
    for plan, shape, kind in ((trsm, (32768, 16384, 16384), 0), (low, (16384, 16384, 32768), 1)):
        r = plan[plan[:, 0] == stp.PROD3][0]
        today = srp.fetch_plan(shape[0], shape[1], shape[2], 0)[0]
        assert np.array_equal(stp.cfg_plan(shape[0], shape[1], shape[2], 0, r[10:15]), today), kind
    for order in (98304, 32768, 16384):
        assert stp.qualifying_calls(order) == [], order


def test_scratch_at_the_flagship_order():
    stp.set_tunables(SHIPPED)
    assert NEED_131072 == 1342177280
    assert stp.scratch_of_order(131072) == (NEED_131072, 2 * NEED_131072)
    for shape in stp.qualifying_calls(131072):
        assert stp.scratch_need(stp.fetch_plan(*shape)) == NEED_131072
    assert stp.scratch_of_order(98304) == (0, 0)
    # the operand-sum scratch of the two levels below is what it was (tests/test_strassen_rec_plan_cpu.py pins it)
    assert srp.scratch_of_order(131072)[0] == (32768 + 16384) * 16384 + (16384 + 8192) * 8192
