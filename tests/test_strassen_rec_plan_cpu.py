"""The recursive factorisation's own Strassen thresholds (sympgpr_amd/csrc/strassen_plan.hip: strassen_rec_values / strassen_rec_cfg, host
code): potrf_rec / trsm_rec plan every product with thresholds chosen for that call.  The list of one call comes through the third
probe entry (sgpr_probe_strassen_rec_plan) and is replayed in numpy (tools/strassen_rec_plan.py).  No GPU needed: the device path
executes exactly this list.

The recursion's tunables are read at every call, so one process can scale them down (halves of 128 ... 256, orders <= 2048) and
set them back.  Tolerance 1e-13 relative to max|C - A B^T|, the rule of tests/test_strassen_plan_cpu.py and
tests/test_strassen2_plan_cpu.py: operands uniform in [-1, 1], k <= 1024, classical rounding about sqrt(k) u max|C| ~ 4e-15
relative, a factor 3 per Strassen level (Higham 23.2.2): 9 x 4e-15 stays an order of magnitude below 1e-13.

Scratch at n = 98304: the library's thresholds need 226 492 416 doubles there (one level everywhere).  With the recursion's own
thresholds the top products of that order (49152 x 24576 x 24576 and the 24576 square of its lower update) take a second level and
need 603 979 776: more than before at that order, and still below what the flagship order reserves before and after
(1 006 632 960).  The assertion below is that bound: no order up to the flagship's reserves more than the flagship's reservation
was before the change."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import strassen_plan as sp  # noqa: E402
import strassen2_plan as sp2  # noqa: E402
import strassen_rec_plan as srp  # noqa: E402

# scaled down by 32: inner threshold 128 (library 256), outer threshold 256 (library 512), inner slab 512, outer slabs 1024 / 512
SMALL = {"rec_strassen_min_gemm": 128, "rec_strassen_min_syrk": 128, "rec_strassen2_min_gemm": 256, "rec_strassen2_min_syrk": 256,
         "rec_strassen2_kslab_short": 512, "rec_strassen_kslab": 512, "rec_strassen2_kslab": 1024}
SMALL_LIBRARY = dict(SMALL, rec_strassen_min_gemm=256, rec_strassen_min_syrk=256, rec_strassen2_min_gemm=512, rec_strassen2_min_syrk=512,
                     rec_strassen2_kslab_short=0)
TODAY_131072 = (32768 + 16384) * 16384 + (16384 + 8192) * 8192      # tests/test_strassen2_plan_cpu.py: the largest product's need


@pytest.fixture
def tunables():
    """set the recursion's tunables for one test, the shipped values afterwards"""
    yield srp.set_tunables
    srp.set_tunables(srp.SHIPPED)


def operands(m, n, k, seed, same=False):
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1, 1, (m, k))
    B = A if same else rng.uniform(-1, 1, (n, k))
    return A, B, rng.uniform(-1, 1, (m, n))


def kinds(plan):
    return {name: int((plan[:, 0] == v).sum()) for name, v in (("sum", sp.SUM), ("prod", sp.PROD), ("classic", sp.CLASSIC),
                                                               ("sum2", sp2.SUM2), ("prod2", sp2.PROD2))}


@pytest.mark.parametrize("m,n,k,slab,outer,inner_direct,why", [
    (2048, 1024, 1024, 1024, 7, 0, "the 2:1 product of trsm_rec, k = one long slab"),
    (2048, 512, 512, 512, 7, 0, "k below the long slab: the short outer slab"),
    (1024, 1024, 768, 512, 7, 7, "short slab with a remainder of 256 behind it, which takes the inner level"),
    (1024, 1024, 2304, 1024, 14, 7, "two long slabs and a remainder of 256"),
    (2048, 256, 256, 1024, 0, 7, "halves of 128 in n: one level where the library's thresholds give none"),
])
def test_replay_is_the_product(tunables, m, n, k, slab, outer, inner_direct, why):
    tunables(SMALL)
    plan, cfg = srp.fetch_plan(m, n, k, 0)
    assert cfg == {"smin": 128, "kslab": 512, "smin2": 256, "kslab2": slab, "smin_under": 128}, why
    kd = kinds(plan)
    assert (kd["prod2"], kd["prod"], kd["classic"]) == (outer, inner_direct, 0), why
    assert kd["sum2"] == 10 * outer // 7 and kd["sum"] == 10 * inner_direct // 7
    A, B, C0 = operands(m, n, k, m + n + k)
    ref = C0 - A @ B.T
    got = srp.replay(plan, cfg, -1.0, A, B, C0)
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


def test_lower_update_that_splits_twice(tunables):
    """order 2048, k = 1024: the 1024 square takes both levels (quarters of 256), the two 512 squares one level in two k slabs
    (their halves of 256 are no multiple of the outer level's 512 x 256), then four triangles of order 512 (halves of 256 would
    leave the 256 x 128 tile grid)"""
    tunables(SMALL)
    n, k = 2048, 1024
    plan, cfg = srp.fetch_plan(n, n, k, 1)
    kd = kinds(plan)
    assert kd["prod2"] == 7 and kd["prod"] == 2 * 7 * 2 and kd["classic"] == 4
    assert all(r[1] == 1 and r[6] == r[7] == 512 for r in plan if r[0] == sp.CLASSIC)
    A, _, C0 = operands(n, n, k, n + k, same=True)
    ref = C0 - np.tril(A @ A.T)
    got = srp.replay(plan, cfg, -1.0, A, A, C0)
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()
    assert np.array_equal(np.triu(got, 1), np.triu(C0, 1))


def test_outer_slab_is_chosen_from_k(tunables):
    tunables(SMALL)
    for k, want in [(256, 1024), (512, 512), (768, 512), (1023, 512), (1024, 1024), (1536, 1024), (4096, 1024)]:
        assert srp.fetch_plan(1024, 1024, k, 0)[1]["kslab2"] == want, k
    tunables(srp.SHIPPED)
    for k, want in [(8192, 32768), (16384, 16384), (24576, 16384), (32768, 32768), (65536, 32768)]:
        assert srp.fetch_plan(65536, 16384, k, 0)[1]["kslab2"] == want, k


def test_library_values_give_the_existing_probes_lists(tunables):
    """the recursion's tunables at the library's values: every list is sgpr_probe_strassen2_plan's"""
    tunables(srp.LIBRARY)
    for (m, n, k, lower) in set(srp.recursion_calls(131072) + srp.recursion_calls(98304)):
        plan, cfg = srp.fetch_plan(m, n, k, lower)
        assert np.array_equal(plan, sp2.fetch_plan(m, n, k, lower)), (m, n, k, lower)
        assert cfg == {"smin": 8192, "kslab": 16384, "smin2": 16384, "kslab2": 32768, "smin_under": 8192}
    tunables(SMALL_LIBRARY)
    for (m, n, k, lower) in [(2048, 1024, 1024, 0), (2048, 512, 512, 0), (1024, 1024, 768, 0), (2048, 2048, 1024, 1), (1000, 1024, 512, 0)]:
        assert np.array_equal(srp.fetch_plan(m, n, k, lower)[0], sp2.fetch_plan(m, n, k, lower, 256, 512, 512, 1024)), (m, n, k, lower)


def test_two_largest_products_keep_their_lists():
    """65536 x 32768 x 32768 and the 32768 square of the first lower update (k = 65536): record for record what they were"""
    for (m, n, k) in [(65536, 32768, 32768), (32768, 32768, 65536)]:
        plan, cfg = srp.fetch_plan(m, n, k, 0)
        assert cfg["kslab2"] == 32768
        assert np.array_equal(plan, sp2.fetch_plan(m, n, k, 0))
        # ... and so are the inner plans of their outer products, under the lower inner threshold
        for r in plan[plan[:, 0] == sp2.PROD2]:
            assert np.array_equal(sp2.inner_plan(r, cfg["smin_under"], cfg["kslab"]), sp2.inner_plan(r))
    # inside the whole lower call the square's records are the same ones, at its place (rows from 32768, columns from 0)
    whole, _ = srp.fetch_plan(65536, 65536, 65536, 1)
    square = sp2.fetch_plan(32768, 32768, 65536, 0)
    at = [i for i, r in enumerate(whole) if r[0] == sp2.SUM2 and r[2] == 16384][0]
    part = whole[at:at + len(square)].copy()
    assert [int(v) for v in part[:, 0]] == [int(v) for v in square[:, 0]]
    for r in part:
        if r[0] == sp2.SUM2 and r[1] == 0:
            r[4] -= 32768
            r[6] -= 32768
        elif r[0] == sp2.PROD2:
            if not r[1]:
                r[2] -= 32768
            r[10] -= 32768
            if r[15]:
                r[13] -= 32768
    assert np.array_equal(part, square)


# (m, n, k, lower) -> (outer products, inner products issued directly, classical launches, all sums, outer slab): DESIGN 3.5
SHIPPED_TABLE = {
    (65536, 32768, 32768, 0): (7, 0, 0, 80, 32768),
    (65536, 65536, 65536, 1): (42, 0, 4, 480, 32768),       # four triangles of order 16384 stay classical
    (65536, 16384, 16384, 0): (7, 0, 0, 80, 16384),
    (32768, 16384, 16384, 0): (7, 0, 0, 80, 16384),
    (32768, 32768, 32768, 1): (7, 0, 2, 80, 32768),
    (65536, 8192, 8192, 0): (0, 7, 0, 10, 32768),
    (32768, 8192, 8192, 0): (0, 7, 0, 10, 32768),
    (65536, 4096, 4096, 0): (0, 0, 1, 0, 32768),
    (32768, 4096, 4096, 0): (0, 0, 1, 0, 32768),
}


def test_shipped_configuration_on_the_flagship_shapes():
    calls = set(srp.recursion_calls(131072))
    assert calls == set(SHIPPED_TABLE)
    for shape, (outer, inner, classic, sums, slab) in SHIPPED_TABLE.items():
        plan, cfg = srp.fetch_plan(*shape)
        kd, s = kinds(plan), srp.summary(plan, cfg)
        assert (kd["prod2"], kd["prod"], kd["classic"], s["sums"], cfg["kslab2"]) == (outer, inner, classic, sums, slab), shape


def test_scratch_does_not_grow():
    both, one = srp.scratch_of_order(131072)
    assert both == TODAY_131072 and one <= both
    # every call of the flagship order fits into what its largest product needed before
    for shape in set(srp.recursion_calls(131072)):
        plan, cfg = srp.fetch_plan(*shape)
        assert srp.summary(plan, cfg)["scratch_doubles"] <= TODAY_131072, shape
    # n = 98304: see the module docstring
    both, one = srp.scratch_of_order(98304)
    assert one <= both <= TODAY_131072
    need = max(srp.summary(*srp.fetch_plan(*shape))["scratch_doubles"] for shape in set(srp.recursion_calls(98304)))
    assert both == need
