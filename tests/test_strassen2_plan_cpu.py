"""The outer Strassen level of the fp64 NT product (sympgpr_amd/csrc/strassen_plan.hip, host code): the list one call C -= A B^T turns
into with both levels is fetched through the probe library and replayed in numpy (tools/strassen2_plan.py); the inner plans of
its outer products come through the existing probe.  No GPU needed: the device path executes exactly this list (run_plan2).

Tolerance 1e-13 relative to max|C - A B^T|, as in tests/test_strassen_plan_cpu.py: operands uniform in [-1, 1], k <= 1024, the
classical rounding error is about sqrt(k) u max|C| ~ 4e-15 relative and each Strassen level multiplies the constant of the bound
by 3 (Higham 23.2.2), the operand sums adding their own roundings: 9 x 4e-15 stays an order of magnitude below 1e-13."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import strassen_plan as sp  # noqa: E402
import strassen2_plan as sp2  # noqa: E402

IN, OUT = 128, 256          # inner / outer threshold of the small cases


def operands(m, n, k, seed, same=False):
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1, 1, (m, k))
    B = A if same else rng.uniform(-1, 1, (n, k))
    return A, B, rng.uniform(-1, 1, (m, n))


@pytest.mark.parametrize("m,n,k,kslab2", [
    (1024, 1024, 512, 512),
    (2048, 1024, 512, 512),       # the 2:1 shape of trsm_rec
    (1024, 1024, 1024, 512),      # two outer slabs
])
def test_outer_list_replay_is_the_product(m, n, k, kslab2):
    plan = sp2.fetch_plan(m, n, k, 0, IN, -1, OUT, kslab2)
    nslab = k // kslab2
    assert [int(v) for v in plan[:, 0]] == ([sp2.SUM2] * 2 + [sp2.PROD2] + ([sp2.SUM2, sp2.PROD2] * 4)
                                            + [sp2.SUM2] * 2 + [sp2.PROD2] + [sp2.SUM2] * 2 + [sp2.PROD2]) * nslab
    dests, inner_sums, outer_sums, flop = sp2.launches(plan, IN)
    assert outer_sums == 10 * nslab and inner_sums == 70 * nslab
    assert dests == {4: 25 * nslab, 2: 20 * nslab, 1: 4 * nslab}
    assert flop == pytest.approx(49.0 / 64.0 * 2.0 * m * n * k)
    prods = plan[plan[:, 0] == sp2.PROD2]
    assert all(p[7] == m // 2 and p[8] == n // 2 and p[9] == kslab2 // 2 for p in prods)
    assert sp2.scratch_need(plan, IN) == (m // 2 + n // 2) * (kslab2 // 2) + (m // 4 + n // 4) * (kslab2 // 4)
    A, B, C0 = operands(m, n, k, m + n + k)
    ref = C0 - A @ B.T
    got = sp2.replay(plan, -1.0, A, B, C0, smin=IN)
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


def test_k_remainder_takes_the_inner_level():
    """k = 1280 with outer slabs of 512: two slabs with both levels, the last 256 columns through plan_gemm at k offset 1024"""
    m = n = 1024
    plan = sp2.fetch_plan(m, n, 1280, 0, IN, -1, OUT, 512)
    assert int((plan[:, 0] == sp2.PROD2).sum()) == 14
    tail = plan[34:]
    one = sp.fetch_plan(m, n, 256, 0, IN)
    assert [int(v) for v in tail[:, 0]] == [int(v) for v in one[:, 0]] and int((tail[:, 0] == sp.PROD).sum()) == 7
    raw = tail[(tail[:, 0] == sp.PROD) & (tail[:, 1] == 0)]
    assert len(raw) and all(1024 <= r[3] < 1280 for r in raw)
    A, B, C0 = operands(m, n, 1280, 5)
    ref = C0 - A @ B.T
    got = sp2.replay(plan, -1.0, A, B, C0, smin=IN)
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


def test_lower_update_splits_at_the_outer_level_first():
    n, k = 2048, 512
    plan = sp2.fetch_plan(n, n, k, 1, IN, -1, OUT, 512)
    kinds = [int(v) for v in plan[:, 0]]
    # the off-diagonal square 1024 x 1024 takes both levels; the diagonal halves of order 1024 go to plan_syrk as it stands
    half = sp.fetch_plan(1024, 1024, k, 1, IN)
    assert kinds.count(sp2.PROD2) == 7 and kinds.count(sp2.SUM2) == 10
    assert kinds[:len(half)] == [int(v) for v in half[:, 0]] and kinds[-len(half):] == kinds[:len(half)]
    assert np.array_equal(plan[:len(half)], half)
    assert all(r[10] >= 1024 > r[11] for r in plan if r[0] == sp2.PROD2)            # destinations inside the square
    A, _, C0 = operands(n, n, k, n + k, same=True)
    ref = C0 - np.tril(A @ A.T)
    got = sp2.replay(plan, -1.0, A, A, C0, smin=IN)
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()
    assert np.array_equal(np.triu(got, 1), np.triu(C0, 1))


@pytest.mark.parametrize("m,n,k,lower,smin2,kslab2,scratch,why", [
    (1024, 1024, 512, 0, 1024, 512, sp.UNLIMITED, "halves below the outer threshold"),
    (1024, 1024, 512, 0, OUT, 1024, sp.UNLIMITED, "k shorter than one outer slab"),
    (1536, 1024, 512, 0, OUT, 512, sp.UNLIMITED, "m / 2 not a multiple of 512"),
    (1024, 768, 512, 0, OUT, 512, sp.UNLIMITED, "n / 2 not a multiple of 256"),
    (2048, 2048, 512, 1, 1024, 512, sp.UNLIMITED, "lower: halves of the square below the outer threshold"),
    (1024, 1024, 512, 0, OUT, 512, 1024 * 256 + 512 * 128 - 1, "scratch one double short of both pairs"),
])
def test_fall_through_is_the_one_level_list(m, n, k, lower, smin2, kslab2, scratch, why):
    plan = sp2.fetch_plan(m, n, k, lower, IN, -1, smin2, kslab2, scratch)
    one = sp.fetch_plan(m, n, k, lower, IN, -1, scratch)
    assert np.array_equal(plan, one), why
    assert int((one[:, 0] == sp.PROD).sum()) >= 7, "the inner level still applies"


def test_scratch_just_enough_takes_both_levels():
    plan = sp2.fetch_plan(1024, 1024, 512, 0, IN, -1, OUT, 512, 1024 * 256 + 512 * 128)
    assert int((plan[:, 0] == sp2.PROD2).sum()) == 7


@pytest.mark.parametrize("m,n,k", [(1000, 1024, 512), (1024, 1000, 512), (1024, 1024, 500), (1025, 1025, 513)])
def test_odd_sizes_take_one_level_or_none(m, n, k):
    plan = sp2.fetch_plan(m, n, k, 0, IN, -1, OUT, 512)
    assert np.array_equal(plan, sp.fetch_plan(m, n, k, 0, IN))
    assert not np.isin(plan[:, 0], (sp2.SUM2, sp2.PROD2)).any()


def test_inner_threshold_alone_does_not_switch_the_outer_level_on():
    """gemm_strassen_min lowered, the outer tunables at their defaults: the list is the one-level list"""
    for m, n, k, lower in [(2048, 2048, 1024, 0), (4096, 2048, 2048, 0), (4096, 4096, 1024, 1)]:
        assert np.array_equal(sp2.fetch_plan(m, n, k, lower, 256), sp.fetch_plan(m, n, k, lower, 256))


def test_default_thresholds_on_the_flagship_shapes():
    """built-in thresholds (outer: half-sizes >= 16384 in m and n, k slabs of 32768; inner: 8192, 16384) on the shapes the
    recursive factorisation produces at n = 131072"""
    def counts(m, n, k, lower=0):
        plan = sp2.fetch_plan(m, n, k, lower)
        return int((plan[:, 0] == sp2.PROD2).sum()), int((plan[:, 0] == sp.PROD).sum()), int((plan[:, 0] == sp.CLASSIC).sum()), plan

    o, i, c, plan = counts(65536, 32768, 32768)
    assert (o, i, c) == (7, 0, 0)
    assert sp2.scratch_need(plan) == (32768 + 16384) * 16384 + (16384 + 8192) * 8192
    dests, _, _, flop = sp2.launches(plan)
    assert dests == {4: 25, 2: 20, 1: 4} and flop == pytest.approx(49.0 / 64.0 * 2.0 * 65536 * 32768 * 32768)
    # lower update of order 65536, k = 65536: the 32768 square in two outer slabs; the two 16384 squares keep one level
    o, i, c, plan = counts(65536, 65536, 65536, 1)
    assert (o, i, c) == (14, 2 * 7 * 4, 4)
    assert all(r[7] == r[8] == 16384 and r[9] == 16384 for r in plan if r[0] == sp2.PROD2)
    for shape in [(65536, 16384, 16384), (32768, 16384, 16384)]:
        o, i, c, plan = counts(*shape)
        assert o == 0 and i >= 7 and c == 0
        assert np.array_equal(plan, sp.fetch_plan(*shape))
    o, i, c, plan = counts(16384, 8192, 8192)
    assert (o, i, c) == (0, 0, 1)
