"""Leave-one-point-out cross-validation of every problem of a batch of fits with d canonical pairs per point
(sgpr_fit_batch_nd_loo, fit.fit_batch_pairs_loo, func.loo_chol_pairs[_batch]), on both paths: one launch up to order 256, the mid
path above.

Fixtures, reference and tolerance are tests/ref_loo.py's: problem(oracle, fam, d, N, 7000 + 11 N + k), k = 0, 1, 2 (batches of
three); loo_blocks on the oracle's Ky; max(1e-10, 50 cond eps) relative to each quantity's magnitude.  Every row also against
SympFit.pairs(...).run().loo(resid=False, lpd=False) under the same rule.  Every case asserts cond <= 1e6 (50 cond eps <= 1.2e-8),
so the tolerance cannot loosen silently, and prints cond and the errors before asserting (ref_loo.compare).  On the CPU oracle
every Ky of the shapes below (families A - D) is positive definite with cond between 4 and 1.8e4."""
import numpy as np
import pytest

from tests import ref_loo as R
from tests.test_gpu_nll_grad_full import _user_is_c

pytestmark = pytest.mark.gpu

KEYS = ("loo", "press")
COND_MAX = 1e6
_cache = {}


def _batch(oracle, fam, d, N):
    """three problems of one shape with their host references: computed once, shared, never written to"""
    key = (fam, d, N)
    if key not in _cache:
        ofam = "C" if fam == "USER" else fam
        probs = [R.problem(oracle, fam, d, N, 7000 + 11 * N + k, ofam=ofam) for k in range(3)]
        refs = [R.loo_blocks(p["Ky"], p["z"], N, 2 * d) for p in probs]
        data = (np.array([p["X"] for p in probs]), np.array([p["z"] for p in probs]), np.array([p["hyp"] for p in probs]),
                np.array([p["s2"] for p in probs]))
        for a in data:
            a.setflags(write=False)
        _cache[key] = (data, refs, [p["cond"] for p in probs])
    return _cache[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _row(loo, b):
    return {"loo": loo[b, 0], "press": loo[b, 1]}


def _handle(fam, X, z, hyp, s2):
    from sympgpr_amd.fit import SympFit
    with SympFit.pairs(fam, X, z, hyp, s2) as f:
        return f.run().loo(resid=False, lpd=False)


def _check_rows(oracle, fam, d, N):
    """rows vs host and vs the handle, then the bits: nll / alpha / info of fit_batch_pairs, a repeated call, a permuted batch, a
    batch of one"""
    from sympgpr_amd.fit import fit_batch_pairs, fit_batch_pairs_loo
    (X, Z, H, S2), refs, conds = _batch(oracle, fam, d, N)
    al, nll, loo, info = fit_batch_pairs_loo(fam, X, Z, H, S2, want_alpha=True)
    assert loo.shape == (3, 2) and np.all(info == 0) and np.all(np.isfinite(nll))
    for b in range(3):
        what = "%s d=%d N=%d (n=%d) row %d" % (fam, d, N, 2 * d * N, b)
        assert conds[b] <= COND_MAX, (what, conds[b])
        R.compare(_row(loo, b), refs[b], conds[b], what + " vs host", KEYS)
        R.compare(_row(loo, b), _handle(fam, X[b], Z[b], H[b], S2[b]), conds[b], what + " vs SympFit.loo", KEYS)
    al0, nll0, info0 = fit_batch_pairs(fam, X, Z, H, S2, want_alpha=True)
    assert np.array_equal(info, info0) and _same(nll, nll0) and _same(al, al0)
    _, _, again, _ = fit_batch_pairs_loo(fam, X, Z, H, S2)                   # a repeated call
    assert _same(again, loo)
    perm = [2, 1, 0]
    _, _, lp, _ = fit_batch_pairs_loo(fam, X[perm], Z[perm], H[perm], S2[perm])
    assert _same(lp, loo[perm])
    for b in (0, 2):                                                         # a batch of one
        _, n1, l1, _ = fit_batch_pairs_loo(fam, X[b:b + 1], Z[b:b + 1], H[b:b + 1], S2[b:b + 1])
        assert _same(l1[0], loo[b]) and _same(n1, nll[b:b + 1])
    return loo


# ---- 1. the one-launch path
SMALL = [(2, 1), (2, 7), (2, 32),      # n = 4 (the smallest order), 28, 128 (one full leaf)
         (2, 33), (2, 64),             # 132 (the first order at which a point's rows lie in different leaves), 256 = BMAX
         (3, 21), (3, 22), (3, 42)]    # 126, 132, 252


@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
@pytest.mark.parametrize("d,N", SMALL)
def test_small_vs_host_and_handle(oracle, fam, d, N):
    _check_rows(oracle, fam, d, N)


# ---- 2. the mid path
@pytest.mark.parametrize("fam,d,N", [("A", 3, 43),         # n = 258, padded to 384
                                     ("C", 2, 128),        # 512
                                     ("D", 2, 160),        # 640: two panels
                                     ("C", 2, 300),        # 1200: two workgroups of mid_loo_kernel, the second ragged with 44 points
                                     ("D", 3, 171),        # 1026
                                     ("B", 3, 171)])
def test_mid_vs_host_and_handle(oracle, fam, d, N):
    _check_rows(oracle, fam, d, N)


def test_mid_chunks_give_the_same_bits(oracle):
    from sympgpr_amd import _lib as L
    from sympgpr_amd.fit import fit_batch_pairs_loo
    (X3, Z3, H3, S3), _, _ = _batch(oracle, "A", 3, 43)                      # n = 258
    idx = [0, 1, 2, 1, 0]                                                    # five problems
    X, Z, H, S2 = X3[idx], Z3[idx], H3[idx], S3[idx]
    al, nll, loo, info = fit_batch_pairs_loo("A", X, Z, H, S2, want_alpha=True)
    assert np.all(info == 0)
    tune = L.load_probe_library().sgpr_probe_tune
    L.check(tune(b"batch_gradmid_chunk", 2.0))                               # chunks of 2, 2 and 1 problems
    try:
        al2, nll2, loo2, info2 = fit_batch_pairs_loo("A", X, Z, H, S2, want_alpha=True)
    finally:
        L.check(tune(b"batch_gradmid_chunk", 0.0))
    assert np.array_equal(info, info2) and _same(al, al2) and _same(nll, nll2) and _same(loo, loo2)
    assert _same(loo[3], loo[1]) and _same(loo[4], loo[0])


# ---- 3. more problems than workgroups (the grid is capped at 1024)
def _population(fam, d, N, B, seed):
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.uniform(0, 2 * np.pi, (B, N, d)), rng.uniform(-3, 3, (B, N, d))], axis=2)
    Z = rng.standard_normal((B, 2 * d * N))
    h, s2 = R.nd_hyp(fam, N, d)
    H = h * rng.uniform(0.9, 1.1, (B, len(h)))
    return X, Z, H, s2 * rng.uniform(0.5, 2.0, B)


def test_bits_more_problems_than_workgroups():
    from sympgpr_amd.fit import fit_batch_pairs_loo
    X, Z, H, S2 = _population("A", 2, 10, 1500, 77)
    _, nll, loo, info = fit_batch_pairs_loo("A", X, Z, H, S2)
    assert np.all(info == 0) and np.all(np.isfinite(loo)) and np.all(np.isfinite(nll))
    for b in (0, 1023, 1024, 1499):
        _, n1, l1, _ = fit_batch_pairs_loo("A", X[b:b + 1], Z[b:b + 1], H[b:b + 1], S2[b:b + 1])
        assert _same(l1[0], loo[b]) and _same(n1, nll[b:b + 1])


# ---- 4. an indefinite row
@pytest.mark.parametrize("N", [20, 70])                                      # n = 80 (one launch), 280 (mid path)
def test_indefinite_row(N):
    from sympgpr_amd.fit import fit_batch_pairs, fit_batch_pairs_loo
    X, Z, H, S2 = _population("C", 2, N, 5, 9 + N)
    _, nll, loo, info = fit_batch_pairs_loo("C", X, Z, H, S2)
    assert np.all(info == 0) and np.all(np.isfinite(loo))
    Hb = H.copy()
    Hb[2, -1] = -1.3                                                         # sig < 0: Ky indefinite
    _, nllb, loob, infob = fit_batch_pairs_loo("C", X, Z, Hb, S2)
    _, nll0, info0 = fit_batch_pairs("C", X, Z, Hb, S2)
    assert infob[2] > 0 and np.array_equal(infob, info0)
    assert np.isnan(nllb[2]) and np.all(np.isnan(loob[2]))
    keep = [0, 1, 3, 4]
    assert _same(loob[keep], loo[keep]) and _same(nllb[keep], nll[keep])
    _, nlln, loon, _ = fit_batch_pairs_loo("C", X, Z, H, -S2)                # the noise enters as |sig2n|
    assert _same(loon, loo) and _same(nlln, nll)


# ---- 5. d = 1 through the d-pair entry against fit_batch_loo: another Gram stage, so the tolerance rule, not the bits
@pytest.mark.parametrize("fam", ["A", "D"])
@pytest.mark.parametrize("N", [70, 128])                                     # n = 140, 256
def test_d1_against_fit_batch_loo(oracle, fam, N):
    from sympgpr_amd.fit import fit_batch_loo, fit_batch_pairs_loo
    (X, Z, H, S2), refs, conds = _batch(oracle, fam, 1, N)
    _, nll, loo, info = fit_batch_pairs_loo(fam, X, Z, H, S2)
    _, nll1, loo1, info1 = fit_batch_loo(fam, np.ascontiguousarray(X[:, :, 0]), np.ascontiguousarray(X[:, :, 1]), Z, H, S2)
    assert np.all(info == 0) and np.all(info1 == 0)
    for b in range(3):
        what = "%s d=1 N=%d row %d" % (fam, N, b)
        assert conds[b] <= COND_MAX
        R.compare(_row(loo, b), refs[b], conds[b], what + " vs host", KEYS)
        R.compare(_row(loo, b), _row(loo1, b), conds[b], what + " vs fit_batch_loo", KEYS)
        assert abs(nll[b] - nll1[b]) <= 1e-10 * abs(nll1[b])


# ---- 6. the user's family against the handle
@pytest.mark.parametrize("N", [20, 70])                                      # n = 80, 280
def test_user_family(oracle, golden_dir, N):
    from sympgpr_amd.fit import SympFit, fit_batch_pairs_loo
    (X, Z, H, S2), refs, conds = _batch(oracle, "USER", 2, N)                # family C's Ky: its condition number if USER is C
    _, _, loo, info = fit_batch_pairs_loo("USER", X, Z, H, S2)
    assert np.all(info == 0)
    twin = _user_is_c(golden_dir)
    for b in range(3):
        what = "USER d=2 N=%d row %d" % (N, b)
        with SympFit.pairs("USER", X[b], Z[b], H[b], S2[b]) as f:
            ref = f.run().loo(resid=False, lpd=False)
            cond = conds[b] if twin else f.cond_estimate()["cond"]           # another family: the device's own estimate
        assert cond <= COND_MAX
        if twin:
            R.compare(_row(loo, b), refs[b], cond, what + " (= C) vs host", KEYS)
        R.compare(_row(loo, b), ref, cond, what + " vs SympFit.loo", KEYS)


# ---- 7. the wrappers of func
def test_func_wrappers(oracle):
    from sympgpr_amd import func
    func.set_family("D")
    try:
        for d, N in ((2, 25), (3, 43)):                                      # n = 100, 258
            (X, Z, H, S2), refs, conds = _batch(oracle, "D", d, N)
            hyps = np.column_stack([H[0] * np.linspace(0.92, 1.08, 4)[:, None], np.full(4, -S2[0])])
            hyps[0, :-1] = H[0]
            v = func.loo_chol_pairs_batch(hyps, X[0], Z[0])
            assert v.shape == (4,) and conds[0] <= COND_MAX
            R.compare({"loo": v[0]}, refs[0], conds[0], "loo_chol_pairs_batch D d=%d N=%d" % (d, N), ("loo",))
            for b in (0, 3):
                assert _same(np.array([func.loo_chol_pairs(hyps[b], X[0], Z[0])]), v[b:b + 1])
            bad = hyps.copy()
            bad[2, -2] = -1.0
            vb = func.loo_chol_pairs_batch(bad, X[0], Z[0])
            assert np.isnan(vb[2]) and _same(vb[[0, 1, 3]], v[[0, 1, 3]])
            with pytest.raises(np.linalg.LinAlgError):
                func.loo_chol_pairs(bad[2], X[0], Z[0])
    finally:
        func.set_family("A")


def test_func_wrappers_above_the_maximum_order():
    from sympgpr_amd import func
    from sympgpr_amd.fit import SympFit
    func.set_family("C")
    try:
        X, Z, H, S2 = _population("C", 2, 513, 2, 5)                        # n = 2052
        hyps = np.column_stack([H, [S2[0], -S2[1]]])
        v = func.loo_chol_pairs_batch(hyps, X[0], Z[0])
        with SympFit.pairs("C", X[0], Z[0], H[0], S2[0]) as f:
            for b in range(2):
                f.set_hyp(H[b], S2[b])
                assert f.run().loo(resid=False, lpd=False)["loo"] == v[b]
        assert func.loo_chol_pairs(hyps[1], X[0], Z[0]) == v[1]
    finally:
        func.set_family("A")
