"""The Strassen front end of the fp64 NT product (sympgpr_amd/csrc/strassen_plan.hip, host code): the list of operations it emits
for one call C -= A B^T -- which operand sums, which seven half-size products, which destination blocks and signs, and what
stays a classical launch -- is fetched through the probe library and replayed in numpy.  No GPU needed: the device path
executes exactly this list (run_plan), one launch per record.

Tolerance 1e-13 relative to max|C - A B^T|: operands are uniform in [-1, 1] with k <= 1024, so the classical rounding error is
about sqrt(k) u max|C| ~ 4e-15 relative and one Strassen level may cost a small multiple of it (Higham, Accuracy and Stability
of Numerical Algorithms, 23.2.2: the constant grows by 3 per level, plus the sums' own roundings)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import strassen_plan as sp  # noqa: E402


def operands(m, n, k, seed, same=False):
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1, 1, (m, k))
    B = A if same else rng.uniform(-1, 1, (n, k))
    C0 = rng.uniform(-1, 1, (m, n))
    return A, B, C0


def kinds(plan):
    return [int(v) for v in plan[:, 0]]


@pytest.mark.parametrize("m,n,k,kslab,kmax", [
    (1024, 1024, 512, 16384, 0),       # square
    (2048, 1024, 512, 16384, 0),       # 2:1, as in trsm_rec
    (1024, 1536, 768, 16384, 0),       # halves 512 x 768 x 384
    (1024, 1024, 1024, 512, 0),        # k in two slabs of 512
    (1024, 512, 1088, 512, 0),         # three slabs (384, 384, 320): the last one shorter
    (1024, 1024, 1024, 16384, 128),    # one slab, every product cut into k chunks that add to both destinations
])
def test_plan_replay_is_the_product(m, n, k, kslab, kmax):
    plan = sp.fetch_plan(m, n, k, 0, smin=256, kslab=kslab)
    s = sp.summary(plan)
    nslab = -(-k // kslab)
    assert (s["sums"], s["products"], s["classical"]) == (10 * nslab, 7 * nslab, 0)
    assert s["flop"] == pytest.approx(7.0 / 8.0 * 2.0 * m * n * k)
    # four of the seven take one raw operand block on one side, and five accumulate into two destinations
    prods = plan[plan[:, 0] == sp.PROD]
    assert int(((prods[:, 1] == 0) | (prods[:, 4] == 0)).sum()) == 4 * nslab
    assert int((prods[:, 15] != 0).sum()) == 5 * nslab
    # halves stay multiples of the 256 x 128 tile and of the k-step
    assert all(p[7] % 256 == 0 and p[8] % 128 == 0 and p[9] % 16 == 0 for p in prods)
    A, B, C0 = operands(m, n, k, m + n + k)
    ref = C0 - A @ B.T
    got = sp.replay(plan, -1.0, A, B, C0, kmax)
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


@pytest.mark.parametrize("n,k,smin", [(2048, 512, 256), (4096, 256, 256), (2048, 1024, 512)])
def test_syrk_decomposition_replay(n, k, smin):
    """lower update of a square block: diagonal halves recurse while their off-diagonal square qualifies, then take the
    triangular launch; the squares go through the seven products"""
    plan = sp.fetch_plan(n, n, k, 1, smin=smin)
    s = sp.summary(plan)
    levels = 0
    while (n >> (levels + 1)) // 2 >= smin and (n >> (levels + 1)) % 512 == 0:
        levels += 1
    assert levels >= 1
    assert s["classical"] == 2 ** levels and s["products"] == 7 * (2 ** levels - 1)
    assert all(r[1] == 1 and r[6] == r[7] == n >> levels for r in plan if r[0] == sp.CLASSIC)
    A, _, C0 = operands(n, n, k, n + k, same=True)
    ref = C0 - np.tril(A @ A.T)
    got = sp.replay(plan, -1.0, A, A, C0)
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()
    assert np.array_equal(np.triu(got, 1), np.triu(C0, 1))          # nothing above the diagonal is touched


def test_syrk_without_decomposition_and_with_other_alpha():
    plan = sp.fetch_plan(1024, 1024, 512, 1, smin=256)              # off-diagonal square 512: halves 256 qualify
    assert kinds(plan).count(sp.CLASSIC) == 2
    plan = sp.fetch_plan(768, 768, 512, 1, smin=256)                # halves 192 of the square: below the threshold
    assert kinds(plan) == [sp.CLASSIC] and [int(v) for v in plan[0, 1:11]] == [1, 0, 0, 0, 0, 768, 768, 512, 0, 0]
    A, B, C0 = operands(1024, 512, 512, 7)
    plan = sp.fetch_plan(1024, 512, 512, 0, smin=256)
    got = sp.replay(plan, 0.5, A, B, C0)
    ref = C0 + 0.5 * A @ B.T
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


@pytest.mark.parametrize("m,n,k,smin,kslab,scratch,why", [
    (1024, 1024, 512, 1024, 16384, sp.UNLIMITED, "halves below the threshold"),
    (1024, 1024, 256, 512, 16384, sp.UNLIMITED, "half of k below half the threshold"),
    (1280, 1024, 512, 256, 16384, sp.UNLIMITED, "m / 2 not a multiple of the 256-row tile"),
    (1024, 1152, 512, 256, 16384, sp.UNLIMITED, "n / 2 not a multiple of the 128-column tile"),
    (1024, 1024, 528, 256, 16384, sp.UNLIMITED, "k not a multiple of 32"),
    (1000, 1024, 512, 256, 16384, sp.UNLIMITED, "odd size"),
    (1024, 1024, 512, 256, 16384, 0, "no scratch"),
    (1024, 1024, 512, 256, 16384, 2 * 512 * 256 - 1, "scratch one double short"),
])
def test_fall_through_is_one_classical_launch(m, n, k, smin, kslab, scratch, why):
    plan = sp.fetch_plan(m, n, k, 0, smin=smin, kslab=kslab, scratch=scratch)
    assert kinds(plan) == [sp.CLASSIC], why
    assert [int(v) for v in plan[0, 1:11]] == [0, 0, 0, 0, 0, m, n, k, 0, 0]


def test_scratch_is_bounded_by_the_k_slab():
    plan = sp.fetch_plan(1024, 1024, 4096, 0, smin=256, kslab=512)
    assert sp.scratch_need(plan) == (512 + 512) * 256
    assert sp.fetch_plan(1024, 1024, 512, 0, smin=256, scratch=2 * 512 * 256)[:, 0].tolist().count(sp.PROD) == 7


def test_default_threshold_and_flagship_shapes():
    """the built-in threshold (half-sizes >= 8192 for m and n, >= 4096 for k; k slabs of 16384) on the shapes the recursive
    factorisation produces at n = 131072: the products listed in DESIGN 3.5 qualify, order-16384 halves and everything
    the look-ahead driver sees do not"""
    s = sp.summary(sp.fetch_plan(65536, 32768, 32768))
    assert (s["products"], s["classical"]) == (14, 0) and s["scratch_doubles"] == (32768 + 16384) * 8192
    s = sp.summary(sp.fetch_plan(65536, 65536, 65536, 1))
    assert (s["products"], s["classical"]) == (7 * 4 * 3, 4)           # one 32768 square + two 16384 squares, 4 slabs each
    assert sp.summary(sp.fetch_plan(32768, 16384, 16384))["products"] == 7
    for m, n, k in [(16384, 8192, 8192), (32768, 16384, 4096), (8192, 8192, 65536), (49152, 2048, 2048)]:
        assert kinds(sp.fetch_plan(m, n, k)) == [sp.CLASSIC]
    assert kinds(sp.fetch_plan(16384, 16384, 16384, 1)) == [sp.CLASSIC]
