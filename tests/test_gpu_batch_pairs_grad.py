"""The NLL gradient of every problem of a batch of fits with d canonical pairs per point (sgpr_fit_batch_nd_grad,
fit.fit_batch_pairs_grad, func.nll_chol_pairs_grad[_batch]), on both paths: one launch up to order 256, the mid path above.

Reference as in tests/test_gpu_nll_grad_full.py (_reference): Ky from oracle.build_K_nd, factored on the host, W = Ky^-1 - alpha
alpha^T in NumPy, central differences (relative step 1e-5) for lengths and periods, exact for sig and sig2n; each component within
tol * S, S = 1/2 sum |W_ij dKy_ij|, tol = max(1e-9, 100 cond eps) for exact components and max(1e-6, 100 cond eps) for
difference-based ones.  Against SympFit.pairs(...).nll_grad_full() every component takes the exact tolerance (both are analytic).

Inputs: q ~ U(0, 2 pi), P ~ U(-3, 3), z standard normal, hyp, s2 = _nd_hyp(fam, N, d) with hyp times U(0.9, 1.1) per problem, seed
1000 d + 10 N + ord(fam).  On the CPU oracle (families A - D, every shape below up to order 1026) every Ky is positive definite
with cond between 1.9 and 1.5e4, so 100 cond eps <= 3.2e-10 and the bounds are the floors 1e-9 / 1e-6; the difference-based
reference moves by at most 2.0e-8 S between the steps 1e-5 and 1e-4.  Every case asserts cond <= 4e6 (100 cond eps <= 1e-9), so
the tolerance cannot loosen silently, and prints cond and max err / S."""
import numpy as np
import pytest

from tests.test_gpu_nll_grad_full import EPS, _nd_hyp, _reference, _user_is_c

pytestmark = pytest.mark.gpu

COND_MAX = 4e6
_CASES = {}          # (fam, d, N, B) -> the inputs of a case; (fam, d, N, B, b) -> the host reference of its problem b


def _case(fam, d, N, B):
    """B problems of one shape: X (B, N, 2d), Z (B, n), H (B, nhyp), S2 (B,); drawn once per session"""
    key = (fam, d, N, B)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * d + 10 * N + ord(fam[0]))
        hfam = "C" if fam == "USER" else fam
        X = np.empty((B, N, 2 * d))
        Z = np.empty((B, 2 * d * N))
        h0, s2 = _nd_hyp(hfam, N, d)
        H = np.empty((B, len(h0)))
        for b in range(B):
            X[b] = np.column_stack([rng.uniform(0, 2 * np.pi, N) for _ in range(d)] + [rng.uniform(-3, 3, N) for _ in range(d)])
            Z[b] = rng.standard_normal(2 * d * N)
            H[b] = h0 * rng.uniform(0.9, 1.1, len(h0))
        _CASES[key] = (X, Z, H, np.full(B, s2))
    return _CASES[key]


def _ref(oracle, fam, d, N, B, b):
    """the host reference (grad, S, cond, exact mask) of problem b of a case; computed once, never modified"""
    key = (fam, d, N, B, b)
    if key not in _CASES:
        X, Z, H, S2 = _case(fam, d, N, B)
        ofam = "C" if fam == "USER" else fam
        ref = _reference(lambda h: oracle.build_K_nd(ofam, X[b], X[b], h), H[b], S2[b], Z[b], {})
        for a in ref[:2] + ref[3:]:
            a.setflags(write=False)
        _CASES[key] = ref
    return _CASES[key]


def _scale_only(oracle, fam, X, z, hyp, s2):
    """S = 1/2 sum |W dKy| per component as _reference forms it (central differences of step 1e-5 for lengths and periods), without
    the condition number: for the order at which the SVD alone takes longer than a test may"""
    build = lambda h: oracle.build_K_nd(fam, X, X, np.asarray(h, dtype=float))
    K = build(hyp)
    n = K.shape[0]
    Ky = K + abs(s2) * np.eye(n)
    Kinv = np.linalg.inv(Ky)
    Kinv = 0.5 * (Kinv + Kinv.T)
    alpha = Kinv @ z
    W = Kinv - np.outer(alpha, alpha)
    nh = len(hyp)
    S = np.empty(nh + 1)
    for k in range(nh - 1):
        hp, hm = np.array(hyp, dtype=float), np.array(hyp, dtype=float)
        step = 1e-5 * abs(hyp[k])
        hp[k] += step
        hm[k] -= step
        S[k] = 0.5 * np.sum(np.abs(W * ((build(hp) - build(hm)) / (2 * step))))
    S[nh - 1] = 0.5 * np.sum(np.abs(W * K)) / abs(hyp[-1])
    S[nh] = 0.5 * (np.trace(np.abs(Kinv)) + alpha @ alpha)
    return S


def _compare(g, gref, S, cond, ex, what):
    """|g - gref| <= tol S per component; ex: the mask of components that take the exact tolerance"""
    assert cond <= COND_MAX, (what, cond)
    assert g.shape == gref.shape and np.all(np.isfinite(g)), (what, g)
    tol = np.where(ex, max(1e-9, 100 * cond * EPS), max(1e-6, 100 * cond * EPS)) * S
    err = np.abs(g - gref)
    print("%s: cond %.3g  max err/S %.3g" % (what, cond, (err / np.maximum(S, 1e-300)).max()))
    assert np.all(err <= tol), (what, g, gref, err / np.maximum(S, 1e-300))


def _handle_grad(fam, X, z, hyp, s2):
    from sympgpr_amd.fit import SympFit
    with SympFit.pairs(fam, X, z, hyp, s2) as f:
        return f.run().nll_grad_full()


def _check_rows(oracle, fam, d, N, B, host=True):
    from sympgpr_amd.fit import fit_batch_pairs_grad
    X, Z, H, S2 = _case(fam, d, N, B)
    _, nll, g, info = fit_batch_pairs_grad(fam, X, Z, H, S2)
    assert g.shape == (B, H.shape[1] + 1) and np.all(info == 0) and np.all(np.isfinite(nll))
    for b in range(B):
        what = "%s d=%d N=%d (n=%d) row %d" % (fam, d, N, 2 * d * N, b)
        gh = _handle_grad(fam, X[b], Z[b], H[b], S2[b])
        if host:
            gref, S, cond, ex = _ref(oracle, fam, d, N, B, b)
            _compare(g[b], gref, S, cond, ex, what + " vs host")
            _compare(g[b], gh, S, cond, np.ones_like(ex), what + " vs nll_grad_full")
        else:
            # no condition number at this order: the exact tolerance at its floor, 1e-9 S (the rule's bound is never below it)
            S = _scale_only(oracle, fam, X[b], Z[b], H[b], S2[b])
            err = np.abs(g[b] - gh)
            print("%s vs nll_grad_full: max err/S %.3g" % (what, (err / S).max()))
            assert np.all(np.isfinite(g[b])) and np.all(err <= 1e-9 * S), (what, g[b], gh, err / S)
    return g


# ---- 1. the one-launch path against the host and against the handle
SMALL = [(2, 1), (2, 7), (2, 32),      # n = 4, 28, 128 (one leaf)
         (2, 33), (2, 64),             # 132 (the first two-leaf order), 256 = BMAX
         (3, 21), (3, 22), (3, 42),    # 126, 132, 252
         (1, 70)]                      # d = 1 through the d-pair entry


@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])          # B: all-zero off-diagonal blocks; D: 8 sums at d = 2, 11 at d = 3
@pytest.mark.parametrize("d,N", SMALL)
def test_small_vs_host_and_nll_grad_full(oracle, fam, d, N):
    _check_rows(oracle, fam, d, N, 3)


# ---- 2. the mid path
@pytest.mark.parametrize("fam,d,N,B", [("A", 3, 43, 3),        # n = 258, padded to 384
                                       ("C", 2, 128, 3),       # 512: the last one-panel order
                                       ("D", 2, 160, 2),       # 640: two panels
                                       ("D", 3, 171, 2),       # 1026; 11 sums: wider than the d = 1 partial
                                       ("B", 3, 171, 2)])
def test_mid_vs_host_and_nll_grad_full(oracle, fam, d, N, B):
    _check_rows(oracle, fam, d, N, B)


def test_mid_order_2048_vs_nll_grad_full(oracle):
    _check_rows(oracle, "C", 2, 512, 2, host=False)


def test_mid_chunks_give_the_same_bits(oracle):
    from sympgpr_amd import _lib as L
    from sympgpr_amd.fit import fit_batch_pairs_grad
    X, Z, H, S2 = _case("A", 3, 43, 5)                           # n = 258
    al, nll, g, info = fit_batch_pairs_grad("A", X, Z, H, S2, want_alpha=True)
    assert np.all(info == 0)
    tune = L.load_probe_library().sgpr_probe_tune
    L.check(tune(b"batch_gradmid_chunk", 2.0))                   # chunks of 2, 2 and 1 problems
    try:
        al2, nll2, g2, info2 = fit_batch_pairs_grad("A", X, Z, H, S2, want_alpha=True)
    finally:
        L.check(tune(b"batch_gradmid_chunk", 0.0))
    assert np.array_equal(info, info2)
    for a, b in ((al, al2), (nll, nll2), (g, g2)):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 3. bits
def _population(fam, d, N, B, seed):
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.uniform(0, 2 * np.pi, (B, N, d)), rng.uniform(-3, 3, (B, N, d))], axis=2)
    Z = rng.standard_normal((B, 2 * d * N))
    h, s2 = _nd_hyp(fam, N, d)
    H = h * rng.uniform(0.9, 1.1, (B, len(h)))
    return X, Z, H, s2 * rng.uniform(0.5, 2.0, B)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("fam,d,N", [("A", 2, 20), ("D", 3, 30), ("C", 2, 70)])      # n = 80, 180 (two leaves), 280 (mid path)
def test_bits(fam, d, N):
    from sympgpr_amd.fit import fit_batch_pairs, fit_batch_pairs_grad
    X, Z, H, S2 = _population(fam, d, N, 6, 50 + N)
    al, nll, g, info = fit_batch_pairs_grad(fam, X, Z, H, S2, want_alpha=True)
    assert np.all(info == 0) and np.all(np.isfinite(g))
    al0, nll0, info0 = fit_batch_pairs(fam, X, Z, H, S2, want_alpha=True)
    assert np.array_equal(info, info0) and _same(nll, nll0) and _same(al, al0)
    _, nll2, g2, _ = fit_batch_pairs_grad(fam, X, Z, H, S2)                  # a repeated call
    assert _same(g, g2) and _same(nll, nll2)
    first = [5, 0, 1, 2]                                                     # problem 5 first in a batch of 4 ...
    _, _, gf, _ = fit_batch_pairs_grad(fam, X[first], Z[first], H[first], S2[first])
    assert _same(gf[0], g[5])                                                # ... and last in the batch of 6


def test_bits_more_problems_than_workgroups():
    from sympgpr_amd.fit import fit_batch_pairs_grad
    X, Z, H, S2 = _population("A", 2, 10, 1500, 77)
    _, nll, g, info = fit_batch_pairs_grad("A", X, Z, H, S2)
    assert np.all(info == 0) and np.all(np.isfinite(g)) and np.all(np.isfinite(nll))
    for b in (0, 1023, 1024, 1499):
        _, n1, g1, _ = fit_batch_pairs_grad("A", X[b:b + 1], Z[b:b + 1], H[b:b + 1], S2[b:b + 1])
        assert _same(g1[0], g[b]) and _same(n1, nll[b:b + 1])


# ---- 4. an indefinite row, and the sign of sig2n
@pytest.mark.parametrize("N", [20, 70])                                      # n = 80 (one launch), 280 (mid path)
def test_indefinite_row_and_negative_noise(N):
    from sympgpr_amd.fit import fit_batch_pairs, fit_batch_pairs_grad
    X, Z, H, S2 = _population("A", 2, N, 5, 9 + N)
    _, nll, g, info = fit_batch_pairs_grad("A", X, Z, H, S2)
    assert np.all(info == 0)
    Hb = H.copy()
    Hb[2, -1] = -1.3                                                         # sig < 0: Ky indefinite
    _, nllb, gb, infob = fit_batch_pairs_grad("A", X, Z, Hb, S2)
    _, nll0, info0 = fit_batch_pairs("A", X, Z, Hb, S2)
    assert infob[2] > 0 and np.array_equal(infob, info0)
    assert np.isnan(nllb[2]) and np.all(np.isnan(gb[2]))
    keep = [0, 1, 3, 4]
    assert _same(gb[keep], g[keep]) and _same(nllb[keep], nll[keep])
    S2n = S2.copy()
    S2n[[1, 3]] *= -1.0
    _, nlln, gn, _ = fit_batch_pairs_grad("A", X, Z, H, S2n)
    assert _same(nlln, nll) and _same(gn[:, :-1], g[:, :-1])
    assert np.array_equal(gn[:, -1], np.where(S2n < 0, -g[:, -1], g[:, -1]))


# ---- 5. central differences of the batch's own nll
@pytest.mark.parametrize("fam,d,N", [("D", 3, 22), ("C", 2, 70)])
def test_central_differences_of_batch_nll(oracle, fam, d, N):
    from sympgpr_amd.fit import fit_batch_pairs, fit_batch_pairs_grad
    X, Z, H, S2 = _case(fam, d, N, 1)
    S = _ref(oracle, fam, d, N, 1, 0)[1]
    _, _, g, info = fit_batch_pairs_grad(fam, X, Z, H, S2)
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
    _, nll, info = fit_batch_pairs(fam, X[0], Z[0], rows[:, :-1], rows[:, -1], want_alpha=False)
    assert np.all(info == 0)
    fd = (nll[0::2] - nll[1::2]) / (2 * rel * np.abs(full))
    print("fd %s d=%d N=%d: max |fd - g| / S %.3g" % (fam, d, N, (np.abs(fd - g[0]) / S).max()))
    assert np.all(np.abs(fd - g[0]) <= 1e-5 * S + 1e-6 * np.abs(g[0])), (fd, g[0], np.abs(fd - g[0]) / S)


# ---- 6. d = 1 through the d-pair entry against fit_batch_grad: another order of the same sums, not the same bits
@pytest.mark.parametrize("fam", ["A", "D"])
@pytest.mark.parametrize("N", [40, 128])
def test_d1_against_fit_batch_grad(oracle, fam, N):
    from sympgpr_amd.fit import fit_batch_grad, fit_batch_pairs_grad
    B = 2
    X, Z, H, S2 = _case(fam, 1, N, B)
    _, nll, g, info = fit_batch_pairs_grad(fam, X, Z, H, S2)
    _, nll1, g1, info1 = fit_batch_grad(fam, np.ascontiguousarray(X[:, :, 0]), np.ascontiguousarray(X[:, :, 1]), Z, H, S2)
    assert np.all(info == 0) and np.all(info1 == 0)
    for b in range(B):
        _, S, cond, ex = _ref(oracle, fam, 1, N, B, b)
        _compare(g[b], g1[b], S, cond, np.ones_like(ex), "%s d=1 N=%d row %d vs fit_batch_grad" % (fam, N, b))
        assert abs(nll[b] - nll1[b]) <= 1e-10 * abs(nll1[b])


# ---- 7. the user's family
@pytest.mark.parametrize("N", [20, 70])
def test_user_family(oracle, golden_dir, N):
    from sympgpr_amd.fit import fit_batch_pairs_grad
    d, B = 2, 2
    X, Z, H, S2 = _case("USER", d, N, B)
    _, _, g, info = fit_batch_pairs_grad("USER", X, Z, H, S2)
    assert np.all(info == 0)
    twin = _user_is_c(golden_dir)
    for b in range(B):
        gh = _handle_grad("USER", X[b], Z[b], H[b], S2[b])
        if twin:
            _, S, cond, ex = _ref(oracle, "USER", d, N, B, b)               # family C's host reference: the scale
            _compare(g[b], gh, S, cond, np.ones_like(ex), "USER (= C) d=2 N=%d row %d vs nll_grad_full" % (N, b))
        else:
            assert np.all(np.abs(g[b] - gh) <= 1e-9 * np.abs(gh).max()), (g[b], gh)


# ---- 8. the wrappers of func
def test_func_wrappers_match_batch():
    from sympgpr_amd import func
    func.set_family("D")
    try:
        X, Z, H, S2 = _population("D", 2, 25, 4, 12)
        hyps = np.column_stack([H, -S2])
        nll, g = func.nll_chol_pairs_grad_batch(hyps, X[0], Z[0])
        assert g.shape == hyps.shape
        assert _same(nll, func.nll_chol_pairs_batch(hyps, X[0], Z[0]))
        for b in range(4):
            v, gb = func.nll_chol_pairs_grad(hyps[b], X[0], Z[0])
            assert v == nll[b] and _same(gb, g[b]) and gb.shape == (hyps.shape[1],)
        pos = np.column_stack([H, S2])
        _, gp = func.nll_chol_pairs_grad_batch(pos, X[0], Z[0])
        assert _same(gp[:, :-1], g[:, :-1]) and np.array_equal(gp[:, -1], -g[:, -1])
        bad = hyps.copy()
        bad[1, -2] = -1.0
        nb, gbad = func.nll_chol_pairs_grad_batch(bad, X[0], Z[0])
        assert nb[1] == np.inf and np.all(np.isnan(gbad[1])) and _same(nb[[0, 2, 3]], nll[[0, 2, 3]])
        assert _same(gbad[[0, 2, 3]], g[[0, 2, 3]])
        with pytest.raises(np.linalg.LinAlgError):
            func.nll_chol_pairs_grad(bad[1], X[0], Z[0])
    finally:
        func.set_family("A")


def test_func_wrappers_above_the_maximum_order():
    from sympgpr_amd import func
    from sympgpr_amd.fit import SympFit
    func.set_family("C")
    try:
        X, Z, H, S2 = _population("C", 2, 513, 2, 5)                        # n = 2052
        hyps = np.column_stack([H, [S2[0], -S2[1]]])
        nll, g = func.nll_chol_pairs_grad_batch(hyps, X[0], Z[0])
        with SympFit.pairs("C", X[0], Z[0], H[0], S2[0]) as f:
            for b in range(2):
                f.set_hyp(H[b], S2[b])
                assert f.run().nll() == nll[b]
                gh = f.nll_grad_full()
                gh[-1] *= 1.0 if b == 0 else -1.0
                assert _same(gh, g[b])
    finally:
        func.set_family("A")


def test_lbfgs_with_jac_on_a_small_two_pair_map():
    from scipy.optimize import minimize
    from sympgpr_amd import func
    rng = np.random.default_rng(2025)
    N, d = 20, 2
    q, p = rng.uniform(0, 2 * np.pi, (N, d)), rng.uniform(-1, 1, (N, d))
    # a smooth near-identity map from the generating function F = 0.1 (cos q_1 + cos q_2) + 0.05 cos(q_1 - q_2) + 0.02 P_1 P_2:
    # targets (dF/dq, dF/dP), block by block
    dFdq = np.column_stack([-0.1 * np.sin(q[:, 0]) - 0.05 * np.sin(q[:, 0] - q[:, 1]),
                            -0.1 * np.sin(q[:, 1]) + 0.05 * np.sin(q[:, 0] - q[:, 1])])
    dFdP = 0.02 * p[:, ::-1]
    X = np.hstack((q, p))
    z = np.concatenate([dFdq[:, 0], dFdq[:, 1], dFdP[:, 0], dFdP[:, 1]])
    sig2n = 1e-6
    func.set_family("C")
    try:
        def fun(u):
            return func.nll_chol_pairs(np.hstack((10 ** u, [sig2n])), X, z)

        def fun_jac(u):
            h = 10 ** u
            v, g = func.nll_chol_pairs_grad(np.hstack((h, [sig2n])), X, z)
            return v, g[:-1] * h * np.log(10.0)
        u0 = np.array((0.3, 0.3, 0.0, 0.0, -1.0))                            # lq = 2, lP = 1, sig = 0.1
        r1 = minimize(fun_jac, u0, jac=True, method="L-BFGS-B")
        r0 = minimize(fun, u0, method="L-BFGS-B")
    finally:
        func.set_family("A")
    print("L-BFGS-B: with jac %d evaluations, fun %.10g; without %d, fun %.10g" % (r1.nfev, r1.fun, r0.nfev, r0.fun))
    assert r1.success, r1
    assert r1.nfev < r0.nfev, (r1.nfev, r0.nfev)
