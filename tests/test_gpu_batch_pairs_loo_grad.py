"""One leave-one-point-out objective and its exact gradient for every problem of a batch of fits with d canonical pairs per point
(sgpr_fit_batch_nd_loo_grad, fit.fit_batch_pairs_loo_grad, func.loo_chol_pairs_grad[_batch]); both objectives.

Fixtures as tests/test_gpu_batch_pairs_loo.py: ref_loo.problem(oracle, fam, d, N, 7000 + 11 N + k), k = 0, 1, 2.  Values against
ref_loo.loo_blocks under ref_loo.compare (max(1e-10, 50 cond eps) relative).  Gradients against ref_loograd.reference under
ref_loograd.compare: |g - g_ref| <= max(1e-9, 100 cond eps) S for the exact components (sig and sig2n for d > 1), 1e-6 in place of
1e-9 for the difference-based ones, S = 1/2 sum |W' dKy|; and against SympFit.pairs(...).run().loo_grad(objective) under the exact
rule on EVERY component (both are analytic; min |g| / S of the fixtures is as small as 1e-7, so the host's difference-based
components alone would not pin them).  Every case asserts cond <= 1e6 and prints cond and err / tol before asserting.  On the CPU
oracle the difference-based reference moves by at most 1.1e-9 S between the steps 1e-5 and 1e-4 for these shapes."""
import numpy as np
import pytest

from tests import ref_loo as R
from tests import ref_loograd as G
from tests.test_gpu_nll_grad_full import _user_is_c

pytestmark = pytest.mark.gpu

COND_MAX = 1e6
OBJECTIVES = ("loo", "press")
_cache = {}


def _batch(oracle, fam, d, N):
    """three problems of one shape: the inputs, the problems themselves (for the gradient reference) and the value references"""
    key = (fam, d, N)
    if key not in _cache:
        ofam = "C" if fam == "USER" else fam
        probs = [R.problem(oracle, fam, d, N, 7000 + 11 * N + k, ofam=ofam) for k in range(3)]
        vals = [R.loo_blocks(p["Ky"], p["z"], N, 2 * d) for p in probs]
        data = (np.array([p["X"] for p in probs]), np.array([p["z"] for p in probs]), np.array([p["hyp"] for p in probs]),
                np.array([p["s2"] for p in probs]))
        for a in data:
            a.setflags(write=False)
        _cache[key] = (data, probs, vals)
    return _cache[key]


def _gref(oracle, fam, d, N, b, objective):
    """the host gradient reference of problem b: computed once, never modified"""
    key = (fam, d, N, b, objective)
    if key not in _cache:
        _, probs, _ = _batch(oracle, fam, d, N)
        _cache[key] = G.reference(oracle, fam, d, probs[b], objective, ofam="C" if fam == "USER" else fam)
    return _cache[key]


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _handle(fam, X, z, hyp, s2, objective):
    from sympgpr_amd.fit import SympFit
    with SympFit.pairs(fam, X, z, hyp, s2) as f:
        return f.run().loo_grad(objective)


def _exact(ref):
    """the reference with every component under the exact rule (for analytic against analytic)"""
    return dict(ref, exact=np.ones_like(ref["exact"]))


def _check_rows(oracle, fam, d, N, objective):
    from sympgpr_amd.fit import fit_batch_pairs, fit_batch_pairs_loo, fit_batch_pairs_loo_grad
    (X, Z, H, S2), probs, vals = _batch(oracle, fam, d, N)
    col = OBJECTIVES.index(objective)
    al, nll, value, g, info = fit_batch_pairs_loo_grad(fam, X, Z, H, S2, objective=objective, want_alpha=True)
    assert g.shape == (3, H.shape[1] + 1) and value.shape == (3,) and np.all(info == 0) and np.all(np.isfinite(nll))
    for b in range(3):
        what = "%s d=%d N=%d (n=%d) %s row %d" % (fam, d, N, 2 * d * N, objective, b)
        ref = _gref(oracle, fam, d, N, b, objective)
        assert ref["cond"] <= COND_MAX, (what, ref["cond"])
        R.compare({objective: value[b]}, vals[b], ref["cond"], what + " value vs host", (objective,))
        G.compare(g[b], ref, what + " vs host")
        vh, gh = _handle(fam, X[b], Z[b], H[b], S2[b], objective)
        G.compare(g[b], dict(_exact(ref), g=gh), what + " vs SympFit.loo_grad")
        R.compare({objective: value[b]}, {objective: vh}, ref["cond"], what + " value vs SympFit.loo_grad", (objective,))
    # bits: the value is the loo entry's column, nll / alpha / info the fit's; a repeated call, a permuted batch, a batch of one
    _, nlll, loo, _ = fit_batch_pairs_loo(fam, X, Z, H, S2)
    assert _same(value, loo[:, col]) and _same(nll, nlll)
    al0, nll0, info0 = fit_batch_pairs(fam, X, Z, H, S2, want_alpha=True)
    assert np.array_equal(info, info0) and _same(nll, nll0) and _same(al, al0)
    _, _, v2, g2, _ = fit_batch_pairs_loo_grad(fam, X, Z, H, S2, objective=objective)
    assert _same(g2, g) and _same(v2, value)
    perm = [2, 1, 0]
    _, _, vp, gp, _ = fit_batch_pairs_loo_grad(fam, X[perm], Z[perm], H[perm], S2[perm], objective=objective)
    assert _same(gp, g[perm]) and _same(vp, value[perm])
    for b in (0, 2):
        _, n1, v1, g1, _ = fit_batch_pairs_loo_grad(fam, X[b:b + 1], Z[b:b + 1], H[b:b + 1], S2[b:b + 1], objective=objective)
        assert _same(g1[0], g[b]) and _same(v1, value[b:b + 1]) and _same(n1, nll[b:b + 1])


# ---- 1. rows against the host and the handle; the bits
SHAPES = [(2, 7), (2, 33), (2, 64), (3, 22), (3, 42)]        # n = 28, 132 (a point's rows in different leaves), 256, 132, 252


@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
@pytest.mark.parametrize("d,N", SHAPES)
def test_rows_vs_host_and_handle(oracle, fam, d, N, objective):
    _check_rows(oracle, fam, d, N, objective)


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_most_lanes_idle_in_every_fold(oracle, objective):
    _check_rows(oracle, "C", 2, 5, objective)                # n = 20


# ---- 2. more problems than workgroups (the grid is capped at 1024)
def _population(fam, d, N, B, seed):
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.uniform(0, 2 * np.pi, (B, N, d)), rng.uniform(-3, 3, (B, N, d))], axis=2)
    Z = rng.standard_normal((B, 2 * d * N))
    h, s2 = R.nd_hyp(fam, N, d)
    H = h * rng.uniform(0.9, 1.1, (B, len(h)))
    return X, Z, H, s2 * rng.uniform(0.5, 2.0, B)


def test_bits_more_problems_than_workgroups():
    from sympgpr_amd.fit import fit_batch_pairs_loo_grad
    X, Z, H, S2 = _population("A", 2, 10, 1500, 77)
    _, nll, v, g, info = fit_batch_pairs_loo_grad("A", X, Z, H, S2)
    assert np.all(info == 0) and np.all(np.isfinite(g)) and np.all(np.isfinite(v))
    for b in (0, 1023, 1024, 1499):
        _, n1, v1, g1, _ = fit_batch_pairs_loo_grad("A", X[b:b + 1], Z[b:b + 1], H[b:b + 1], S2[b:b + 1])
        assert _same(g1[0], g[b]) and _same(v1, v[b:b + 1]) and _same(n1, nll[b:b + 1])


# ---- 3. an indefinite row, and the sign of sig2n
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_indefinite_row_and_negative_noise(objective):
    from sympgpr_amd.fit import fit_batch_pairs, fit_batch_pairs_loo_grad
    X, Z, H, S2 = _population("C", 2, 20, 5, 29)                             # n = 80
    _, nll, v, g, info = fit_batch_pairs_loo_grad("C", X, Z, H, S2, objective=objective)
    assert np.all(info == 0) and np.all(np.isfinite(g))
    Hb = H.copy()
    Hb[2, -1] = -1.3                                                         # sig < 0: Ky indefinite
    _, nllb, vb, gb, infob = fit_batch_pairs_loo_grad("C", X, Z, Hb, S2, objective=objective)
    _, _, info0 = fit_batch_pairs("C", X, Z, Hb, S2)
    assert infob[2] > 0 and np.array_equal(infob, info0)
    assert np.isnan(nllb[2]) and np.isnan(vb[2]) and np.all(np.isnan(gb[2]))
    keep = [0, 1, 3, 4]
    assert _same(gb[keep], g[keep]) and _same(vb[keep], v[keep]) and _same(nllb[keep], nll[keep])
    S2n = S2.copy()
    S2n[[1, 3]] *= -1.0
    _, nlln, vn, gn, _ = fit_batch_pairs_loo_grad("C", X, Z, H, S2n, objective=objective)
    assert _same(nlln, nll) and _same(vn, v) and _same(gn[:, :-1], g[:, :-1])
    assert np.array_equal(gn[:, -1], np.where(S2n < 0, -g[:, -1], g[:, -1]))


# ---- 4. central differences (relative step 1e-5) of fit_batch_pairs_loo's own values
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("fam,d,N", [("D", 3, 22), ("C", 2, 64)])
def test_central_differences_of_the_batch_values(oracle, fam, d, N, objective):
    from sympgpr_amd.fit import fit_batch_pairs_loo, fit_batch_pairs_loo_grad
    (X, Z, H, S2), _, _ = _batch(oracle, fam, d, N)
    S = _gref(oracle, fam, d, N, 0, objective)["S"]
    _, _, _, g, info = fit_batch_pairs_loo_grad(fam, X[:1], Z[:1], H[:1], S2[:1], objective=objective)
    assert info[0] == 0
    full = np.append(H[0], S2[0])
    rel = 1e-5
    rows = []
    for k in range(len(full)):
        for sgn in (1, -1):
            h = full.copy()
            h[k] += sgn * rel * abs(full[k])
            rows.append(h)
    rows = np.array(rows)
    _, _, loo, info = fit_batch_pairs_loo(fam, X[0], Z[0], rows[:, :-1], rows[:, -1])
    assert np.all(info == 0)
    v = loo[:, OBJECTIVES.index(objective)]
    fd = (v[0::2] - v[1::2]) / (2 * rel * np.abs(full))
    print("fd %s d=%d N=%d %s: max |fd - g| / S %.3g" % (fam, d, N, objective, (np.abs(fd - g[0]) / S).max()))
    assert np.all(np.abs(fd - g[0]) <= 1e-5 * S + 1e-6 * np.abs(g[0])), (fd, g[0], np.abs(fd - g[0]) / S)


# ---- 5. order 258: the wrapper's slow path (values batched on the mid path, gradients from one handle per row)
def test_order_258_through_the_slow_path(oracle):
    from sympgpr_amd.fit import fit_batch_pairs_loo, fit_batch_pairs_loo_grad
    fam, d, N = "A", 3, 43
    (X, Z, H, S2), _, vals = _batch(oracle, fam, d, N)
    _, nll, value, g, info = fit_batch_pairs_loo_grad(fam, X, Z, H, S2, objective="press")
    _, nll0, loo, _ = fit_batch_pairs_loo(fam, X, Z, H, S2)
    assert np.all(info == 0) and _same(value, loo[:, 1]) and _same(nll, nll0)
    for b in range(3):
        ref = _gref(oracle, fam, d, N, b, "press")
        assert ref["cond"] <= COND_MAX
        G.compare(g[b], ref, "A d=3 N=43 (n=258) press row %d vs host" % b)
        assert _same(g[b], _handle(fam, X[b], Z[b], H[b], S2[b], "press")[1])


# ---- 6. the user's family against the handle
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_user_family(oracle, golden_dir, objective):
    from sympgpr_amd.fit import fit_batch_pairs_loo_grad
    d, N = 2, 20
    (X, Z, H, S2), _, _ = _batch(oracle, "USER", d, N)
    _, _, v, g, info = fit_batch_pairs_loo_grad("USER", X, Z, H, S2, objective=objective)
    assert np.all(info == 0)
    from sympgpr_amd.fit import SympFit
    twin = _user_is_c(golden_dir)
    for b in range(3):
        what = "USER d=2 N=20 %s row %d" % (objective, b)
        with SympFit.pairs("USER", X[b], Z[b], H[b], S2[b]) as f:
            vh, gh = f.run().loo_grad(objective)
            cond = f.cond_estimate()["cond"]                                 # the device's own estimate, for another family
        if twin:
            ref = _gref(oracle, "USER", d, N, b, objective)                  # family C's host reference: the scale and cond
            cond = ref["cond"]
            G.compare(g[b], dict(_exact(ref), g=gh), what + " (= C) vs SympFit.loo_grad")
            G.compare(g[b], ref, what + " (= C) vs host")
        else:
            assert np.all(np.abs(g[b] - gh) <= 1e-9 * np.abs(gh).max()), (g[b], gh)
        assert cond <= COND_MAX
        R.compare({objective: v[b]}, {objective: vh}, cond, what + " value vs SympFit.loo_grad", (objective,))


# ---- 7. d = 1 through the d-pair entry against fit_batch_loo_grad: another Gram stage, so the tolerance rule, not the bits
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("fam", ["A", "D"])
def test_d1_against_fit_batch_loo_grad(oracle, fam, objective):
    from sympgpr_amd.fit import fit_batch_loo_grad, fit_batch_pairs_loo_grad
    N = 40
    (X, Z, H, S2), _, vals = _batch(oracle, fam, 1, N)
    _, nll, v, g, info = fit_batch_pairs_loo_grad(fam, X, Z, H, S2, objective=objective)
    _, nll1, v1, g1, info1 = fit_batch_loo_grad(fam, np.ascontiguousarray(X[:, :, 0]), np.ascontiguousarray(X[:, :, 1]), Z, H, S2,
                                                objective=objective)
    assert np.all(info == 0) and np.all(info1 == 0)
    for b in range(3):
        what = "%s d=1 N=%d %s row %d" % (fam, N, objective, b)
        ref = _gref(oracle, fam, 1, N, b, objective)
        assert ref["cond"] <= COND_MAX
        G.compare(g[b], ref, what + " vs host")
        G.compare(g[b], dict(_exact(ref), g=g1[b]), what + " vs fit_batch_loo_grad")
        R.compare({objective: v[b]}, {objective: v1[b]}, ref["cond"], what + " value vs fit_batch_loo_grad", (objective,))
        assert abs(nll[b] - nll1[b]) <= 1e-10 * abs(nll1[b])


# ---- 8. the wrappers of func
def test_func_wrappers_match_batch():
    from sympgpr_amd import func
    from sympgpr_amd.fit import fit_batch_pairs_loo_grad
    func.set_family("D")
    try:
        X, Z, H, S2 = _population("D", 2, 25, 4, 12)
        hyps = np.column_stack([H, -S2])
        for objective in OBJECTIVES:
            v, g = func.loo_chol_pairs_grad_batch(hyps, X[0], Z[0], objective=objective)
            assert g.shape == hyps.shape
            _, _, vb, gb, _ = fit_batch_pairs_loo_grad("D", X[0], Z[0], H, S2, objective=objective)
            assert _same(v, vb) and _same(g[:, :-1], gb[:, :-1]) and np.array_equal(g[:, -1], -gb[:, -1])
            if objective == "loo":
                assert _same(v, func.loo_chol_pairs_batch(hyps, X[0], Z[0]))
            for b in (0, 3):
                v1, g1 = func.loo_chol_pairs_grad(hyps[b], X[0], Z[0], objective=objective)
                assert v1 == v[b] and _same(g1, g[b]) and g1.shape == (hyps.shape[1],)
        bad = hyps.copy()
        bad[1, -2] = -1.0
        v, g = func.loo_chol_pairs_grad_batch(hyps, X[0], Z[0])
        vbad, gbad = func.loo_chol_pairs_grad_batch(bad, X[0], Z[0])
        assert np.isnan(vbad[1]) and np.all(np.isnan(gbad[1])) and _same(vbad[[0, 2, 3]], v[[0, 2, 3]])
        assert _same(gbad[[0, 2, 3]], g[[0, 2, 3]])
        with pytest.raises(np.linalg.LinAlgError):
            func.loo_chol_pairs_grad(bad[1], X[0], Z[0])
    finally:
        func.set_family("A")


def test_lbfgs_with_jac_on_a_small_two_pair_map():
    from scipy.optimize import minimize
    from sympgpr_amd import func
    rng = np.random.default_rng(2025)
    N, d = 20, 2
    q, p = rng.uniform(0, 2 * np.pi, (N, d)), rng.uniform(-1, 1, (N, d))
    # the map of tests/test_gpu_batch_pairs_grad.py: F = 0.1 (cos q_1 + cos q_2) + 0.05 cos(q_1 - q_2) + 0.02 P_1 P_2, targets
    # (dF/dq, dF/dP), block by block
    dFdq = np.column_stack([-0.1 * np.sin(q[:, 0]) - 0.05 * np.sin(q[:, 0] - q[:, 1]),
                            -0.1 * np.sin(q[:, 1]) + 0.05 * np.sin(q[:, 0] - q[:, 1])])
    dFdP = 0.02 * p[:, ::-1]
    X = np.hstack((q, p))
    z = np.concatenate([dFdq[:, 0], dFdq[:, 1], dFdP[:, 0], dFdP[:, 1]])
    sig2n = 1e-6
    func.set_family("C")
    try:
        def fun(u):
            return func.loo_chol_pairs(np.hstack((10 ** u, [sig2n])), X, z)

        def fun_jac(u):
            h = 10 ** u
            v, g = func.loo_chol_pairs_grad(np.hstack((h, [sig2n])), X, z)
            return v, g[:-1] * h * np.log(10.0)
        u0 = np.array((0.3, 0.3, 0.0, 0.0, -1.0))                            # lq = 2, lP = 1, sig = 0.1
        # box: lengths 0.32 .. 6.3 (q spans 2 pi, P spans 2), sig 1e-3 .. 10.  Without it the first line search of this objective
        # steps to sig = 1e64 and lengths of 1e5 .. 1e26, where Ky is not positive definite in fp64 and loo_chol_pairs raises, by
        # its convention; inside the box cond(Ky) <= 4.4e4 on the host oracle along the whole run
        box = [(-0.5, 0.8)] * 4 + [(-3.0, 1.0)]
        r1 = minimize(fun_jac, u0, jac=True, method="L-BFGS-B", bounds=box)
        r0 = minimize(fun, u0, method="L-BFGS-B", bounds=box)
    finally:
        func.set_family("A")
    print("L-BFGS-B on loo: with jac %d evaluations, fun %.10g; without %d, fun %.10g" % (r1.nfev, r1.fun, r0.nfev, r0.fun))
    assert r1.success, r1
    assert r1.nfev < r0.nfev, (r1.nfev, r0.nfev)
