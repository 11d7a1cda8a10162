"""The NLL gradient of every problem of a batch of small fits (sgpr_fit_batch_grad, fit.fit_batch_grad, func.nll_chol_grad,
func.nll_chol_grad_batch).

Reference as in tests/test_gpu_nll_grad_full.py: Ky from the oracle's host Gram builders, W = Ky^-1 - alpha alpha^T in NumPy,
exact dK for lx / ly (oracle.build_dK / build_dKreg) and sig (K / sig), central differences for a period; each component
within tol * S, tol = max(1e-9, 100 cond eps) (1e-6 for difference-based components).  Also: every row against
SympFit.nll_grad_full, nll / alpha bits against fit_batch, bits independent of the batch, NaN rows, the sign of sig2n,
central differences of the batch's own nll, the order-600 fallback, and L-BFGS-B with jac=True on a regGP-style section."""
import numpy as np
import pytest

from tests.test_gpu_nll_grad_full import EPS, _pair_hyp, _reference, _user_is_c

pytestmark = pytest.mark.gpu


def _compare(g, ref, what):
    gref, S, cond, ex = ref
    assert g.shape == gref.shape
    assert np.all(np.isfinite(g)), (what, g)
    tol = np.where(ex, max(1e-9, 100 * cond * EPS), max(1e-6, 100 * cond * EPS)) * S
    err = np.abs(g - gref)
    assert np.all(err <= tol), (what, g, gref, err / np.maximum(S, 1e-300))


def _problem(oracle, fam, npts, reg, seed, ofam=None, s2_sign=1.0):
    """one problem and its host reference gradient"""
    ofam = ofam or fam
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, 2 * np.pi, npts), rng.uniform(-3, 3, npts)
    n = npts if reg else 2 * npts
    z = rng.standard_normal(n)
    hyp, s2 = _pair_hyp(fam, n)
    hyp = np.array(hyp) * rng.uniform(0.9, 1.1, len(hyp))
    s2 *= s2_sign
    if reg:
        build = lambda h: oracle.buildKreg(ofam, x, y, x, y, h, threads=16)
        dK = (lambda: oracle.build_dKreg(ofam, x, y, x, y, hyp)) if ofam != "D" else None
    else:
        build = lambda h: oracle.build_K(ofam, x, y, x, y, h, threads=16)
        dK = (lambda: oracle.build_dK(ofam, x, y, x, y, hyp)) if ofam != "D" else None
    exact = dict(enumerate(dK())) if dK else {}
    return (x, y, z, hyp, s2), _reference(build, hyp, s2, z, exact)


def _batch(oracle, fam, npts, reg, seeds, ofam=None):
    probs = [_problem(oracle, fam, npts, reg, s, ofam) for s in seeds]
    X, Y, Z, H, S2 = (np.array([p[0][k] for p in probs]) for k in range(5))
    return (X, Y, Z, H, S2), [p[1] for p in probs]


ORDERS_PAIR = [1, 40, 64, 70, 100, 128]            # n = 2, 80, 128 (one leaf), 140, 200 (n2 = 72), 256 (two full leaves)
ORDERS_REG = [1, 80, 128, 129, 140, 200, 256]      # 129: odd, one row past the first leaf


@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
@pytest.mark.parametrize("npts", ORDERS_PAIR)
def test_pairs_vs_host_and_nll_grad_full(oracle, fam, npts):
    from sympgpr_amd.fit import SympFit, fit_batch_grad
    (X, Y, Z, H, S2), refs = _batch(oracle, fam, npts, False, [1000 + 7 * npts + k for k in range(3)])
    _, nll, g, info = fit_batch_grad(fam, X, Y, Z, H, S2)
    assert g.shape == (3, H.shape[1] + 1) and np.all(info == 0) and np.all(np.isfinite(nll))
    for b in range(3):
        _compare(g[b], refs[b], "pairs %s n=%d row %d" % (fam, 2 * npts, b))
        with SympFit(fam, X[b], Y[b], Z[b], H[b], S2[b]) as f:
            _compare(g[b], (f.run().nll_grad_full(),) + refs[b][1:], "pairs %s n=%d row %d vs nll_grad_full" % (fam, 2 * npts, b))


@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
@pytest.mark.parametrize("npts", ORDERS_REG)
def test_reg_vs_host_and_nll_grad_full(oracle, fam, npts):
    from sympgpr_amd.fit import SympFit, fit_batch_grad
    (X, Y, Z, H, S2), refs = _batch(oracle, fam, npts, True, [2000 + 7 * npts + k for k in range(3)])
    _, nll, g, info = fit_batch_grad(fam, X, Y, Z, H, S2, reg=True)
    assert np.all(info == 0) and np.all(np.isfinite(nll))
    for b in range(3):
        _compare(g[b], refs[b], "reg %s n=%d row %d" % (fam, npts, b))
        with SympFit(fam, X[b], Y[b], Z[b], H[b], S2[b], reg=True) as f:
            _compare(g[b], (f.run().nll_grad_full(),) + refs[b][1:], "reg %s n=%d row %d vs nll_grad_full" % (fam, npts, b))


@pytest.mark.parametrize("reg,npts", [(False, 70), (False, 128), (True, 129)])
def test_user_family_vs_family_c(oracle, golden_dir, reg, npts):
    if not _user_is_c(golden_dir):
        pytest.skip("USER_FAMILY has been edited: no hand-written twin to compare with")
    from sympgpr_amd.fit import fit_batch_grad
    (X, Y, Z, H, S2), refs = _batch(oracle, "USER", npts, reg, [3000 + npts, 3001 + npts], ofam="C")
    _, _, g, info = fit_batch_grad("USER", X, Y, Z, H, S2, reg=reg)
    assert np.all(info == 0)
    for b in range(2):
        _compare(g[b], refs[b], "USER (= C) reg=%s n=%d" % (reg, npts))


def _population(fam, npts, reg, B, seed):
    rng = np.random.default_rng(seed)
    n = npts if reg else 2 * npts
    X, Y = rng.uniform(0, 2 * np.pi, (B, npts)), rng.uniform(-3, 3, (B, npts))
    Z = rng.standard_normal((B, n))
    h, s2 = _pair_hyp(fam, n)
    H = np.array(h) * rng.uniform(0.8, 1.25, (B, len(h)))
    return X, Y, Z, H, s2 * rng.uniform(0.5, 2.0, B)


@pytest.mark.parametrize("fam,npts,reg", [("A", 70, False), ("D", 100, False), ("C", 129, True), ("B", 40, False)])
def test_bits(fam, npts, reg):
    from sympgpr_amd.fit import fit_batch, fit_batch_grad
    X, Y, Z, H, S2 = _population(fam, npts, reg, 2000, 50 + npts)      # more problems than the grid (1024)
    al, nll, g, info = fit_batch_grad(fam, X, Y, Z, H, S2, reg=reg, want_alpha=True)
    assert np.all(info == 0)
    al0, nll0, info0 = fit_batch(fam, X, Y, Z, H, S2, reg=reg, want_alpha=True)
    assert np.array_equal(info, info0)
    assert np.array_equal(nll.view(np.uint64), nll0.view(np.uint64))
    assert np.array_equal(al.view(np.uint64), al0.view(np.uint64))
    _, nll2, g2, _ = fit_batch_grad(fam, X, Y, Z, H, S2, reg=reg)           # a repeated call
    assert np.array_equal(g.view(np.uint64), g2.view(np.uint64)) and np.array_equal(nll2.view(np.uint64), nll.view(np.uint64))
    for b in (0, 1500):                                                     # alone, and at another position of a small batch
        _, n1, g1, _ = fit_batch_grad(fam, X[b:b + 1], Y[b:b + 1], Z[b:b + 1], H[b:b + 1], S2[b:b + 1], reg=reg)
        assert np.array_equal(g1[0].view(np.uint64), g[b].view(np.uint64)) and n1[0] == nll[b]
        perm = [3, b, 7]
        _, _, g3, _ = fit_batch_grad(fam, X[perm], Y[perm], Z[perm], H[perm], S2[perm], reg=reg)
        assert np.array_equal(g3[1].view(np.uint64), g[b].view(np.uint64))


def test_indefinite_row_and_negative_noise():
    from sympgpr_amd.fit import fit_batch, fit_batch_grad
    X, Y, Z, H, S2 = _population("A", 70, False, 5, 9)
    _, nll, g, info = fit_batch_grad("A", X, Y, Z, H, S2)
    assert np.all(info == 0)
    Hb = H.copy()
    Hb[2, -1] = -1.3                                                        # sig < 0: Ky indefinite
    _, nllb, gb, infob = fit_batch_grad("A", X, Y, Z, Hb, S2)
    _, nll0, info0 = fit_batch("A", X, Y, Z, Hb, S2)
    assert infob[2] > 0 and np.array_equal(infob, info0)
    assert np.isnan(nllb[2]) and np.all(np.isnan(gb[2]))
    keep = [0, 1, 3, 4]
    assert np.array_equal(gb[keep].view(np.uint64), g[keep].view(np.uint64))
    assert np.array_equal(nllb[keep].view(np.uint64), nll[keep].view(np.uint64))
    S2n = S2.copy()
    S2n[[1, 3]] *= -1.0
    _, nlln, gn, _ = fit_batch_grad("A", X, Y, Z, H, S2n)
    assert np.array_equal(nlln.view(np.uint64), nll.view(np.uint64))
    assert np.array_equal(gn[:, :-1].view(np.uint64), g[:, :-1].view(np.uint64))
    assert np.array_equal(gn[:, -1], np.where(S2n < 0, -g[:, -1], g[:, -1]))


@pytest.mark.parametrize("fam,npts,reg", [("D", 70, False), ("C", 100, False), ("D", 140, True), ("A", 128, True)])
def test_central_differences_of_batch_nll(oracle, fam, npts, reg):
    from sympgpr_amd.fit import fit_batch, fit_batch_grad
    (x, y, z, hyp, s2), ref = _problem(oracle, fam, npts, reg, 77 + npts)
    _, _, g, _ = fit_batch_grad(fam, x[None], y[None], z[None], hyp[None], s2, reg=reg)
    full = np.append(hyp, s2)
    rel = 1e-5
    rows = []
    for k in range(len(full)):
        for sgn in (1, -1):
            h = full.copy()
            h[k] += sgn * rel * abs(full[k])
            rows.append(h)
    rows = np.array(rows)
    B = len(rows)
    _, nll, info = fit_batch(fam, np.repeat(x[None], B, 0), np.repeat(y[None], B, 0), np.repeat(z[None], B, 0), rows[:, :-1],
                             rows[:, -1], reg=reg)
    assert np.all(info == 0)
    fd = (nll[0::2] - nll[1::2]) / (2 * rel * np.abs(full))
    S = ref[1]
    assert np.all(np.abs(fd - g[0]) <= 1e-5 * S + 1e-6 * np.abs(g[0])), (fd, g[0], np.abs(fd - g[0]) / S)


def test_mid_order_fallback():
    from sympgpr_amd.fit import SympFit, fit_batch, fit_batch_grad
    X, Y, Z, H, S2 = _population("C", 300, False, 3, 600)                  # n = 600
    H[1, -1] = -1.0                                                          # one row not positive definite
    al, nll, g, info = fit_batch_grad("C", X, Y, Z, H, S2, want_alpha=True)
    al0, nll0, info0 = fit_batch("C", X, Y, Z, H, S2, want_alpha=True)
    assert np.array_equal(info, info0) and info[1] > 0
    assert np.isnan(nll[1]) and np.array_equal(nll[[0, 2]].view(np.uint64), nll0[[0, 2]].view(np.uint64))
    assert np.all(np.isnan(g[1]))
    for b in (0, 2):
        with SympFit("C", X[b], Y[b], Z[b], H[b], S2[b]) as f:
            assert np.array_equal(f.run().nll_grad_full(), g[b])


def test_func_wrappers_match_batch():
    from sympgpr_amd import func
    func.set_family("D")
    try:
        X, Y, Z, H, S2 = _population("D", 50, False, 4, 12)
        x, y = np.concatenate([X[0], Y[0]]), Z[0]
        hyps = np.column_stack([H, -S2])
        nll, g = func.nll_chol_grad_batch(hyps, x, y, 100)
        for b in range(4):
            v, gb = func.nll_chol_grad(hyps[b], x, y, 100)
            assert v == nll[b] and np.array_equal(gb, g[b]) and gb.shape == (len(hyps[b]),)
            assert v == func.nll_chol(hyps[b], x, y, 100)
        bad = hyps.copy()
        bad[1, -2] = -1.0
        nb, gbad = func.nll_chol_grad_batch(bad, x, y, 100)
        assert nb[1] == np.inf and np.all(np.isnan(gbad[1])) and np.array_equal(nb[[0, 2, 3]], nll[[0, 2, 3]])
        with pytest.raises(np.linalg.LinAlgError):
            func.nll_chol_grad(bad[1], x, y, 100)
        vr, gr = func.nll_chol_grad(hyps[0], x, y, 50, reg=True)
        assert vr == func.nll_chol_reg(hyps[0], x, y, 50) and gr.shape == (len(hyps[0]),)
    finally:
        func.set_family("A")


def test_lbfgs_with_jac_on_a_section():
    from scipy.optimize import minimize
    from sympgpr_amd import func
    rng = np.random.default_rng(2024)
    N = 40
    q, p = rng.uniform(0, 2 * np.pi, N), rng.uniform(-1, 1, N)
    P = p + 0.1 * np.sin(q) + 0.05 * p * np.cos(q)
    x, z = np.hstack((q, p)), P - p
    sig2n = 1e-8
    func.set_family("C")
    try:
        def fun(u):
            return func.nll_chol_reg(np.hstack((10 ** u, [sig2n])), x, z, N)

        def fun_jac(u):
            h = 10 ** u
            v, g = func.nll_chol_grad(np.hstack((h, [sig2n])), x, z, N, reg=True)
            return v, g[:3] * h * np.log(10.0)
        u0 = np.array((-1.0, 0.0, 1.0))                                     # regGP's start
        r1 = minimize(fun_jac, u0, jac=True, method="L-BFGS-B")
        r0 = minimize(fun, u0, method="L-BFGS-B")
    finally:
        func.set_family("A")
    assert r1.success, r1
    assert r1.nfev < r0.nfev, (r1.nfev, r0.nfev)
    assert r1.fun <= r0.fun + 1e-8 * abs(r0.fun), (r1.fun, r0.fun)
