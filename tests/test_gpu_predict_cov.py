"""Predictive covariance on the device (sgpr_fit_predict_cov, SympFit.predict_cov / predict_pairs_cov) against the oracle's
host Gram builders: Sigma = K_tt - K_tx Ky^-1 K_xt with Ky = K_xx + |sig2n| I factored by SciPy, point t's D x D block.
Tolerance 100 cond(Ky) eps max|diag K_tt|, cond from numpy on the host Ky (at n = 16 384 the device estimate).
Both solve paths are covered: orders that are not a multiple of 128 (or 1 column) take the transposed panel solve,
the others the strip solves' forward passes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _points(rng, N):
    return rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N)


def _hyp(fam, N, d=1):
    l = 2.0 * np.sqrt(12 * np.pi) * N ** (-1.0 / (2 * d))
    if d > 1:
        return np.append(np.full(2 * d, l), 1.0), 1e-2 / l**2
    return ([l, l, 0.5, 1.0] if fam == "D" else [l, l, 1.0]), 1e-2 / l**2


def _sigma(Kxx, s2, Ktx, Kxt, Ktt):
    import scipy.linalg
    Ky = Kxx + abs(s2) * np.eye(Kxx.shape[0])
    cond = float(np.linalg.cond(Ky))
    S = Ktt - Ktx @ scipy.linalg.cho_solve(scipy.linalg.cho_factor(Ky, lower=True), Kxt)
    return S, cond


def _blocks(A, m, D):
    """point t's D x D block of a (D m x D m) matrix whose output a of point t sits at row / column a m + t"""
    idx = np.arange(D)[None, :] * m + np.arange(m)[:, None]          # (m, D)
    return A[idx[:, :, None], idx[:, None, :]]


def _check(cov, Sig, Kss, cond, what):
    m, D, _ = cov.shape
    tol = 100 * cond * EPS * np.abs(np.diagonal(Kss, axis1=1, axis2=2)).max()
    err = np.abs(cov - Sig).max()
    print("%s: cond(Ky) = %.3g  max|cov - Sigma| = %.3g  tol = %.3g" % (what, cond, err, tol))
    assert np.all(np.isfinite(cov))
    assert err <= tol, (what, err, tol)
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2)), "not exactly symmetric"
    assert np.linalg.eigvalsh(cov).min() >= -tol
    assert np.all(np.diagonal(cov, axis1=1, axis2=2) <= np.diagonal(Kss, axis1=1, axis2=2) + tol)


def _pair_case(oracle, fam, N, m, seed):
    rng = np.random.default_rng(seed)
    q, P = _points(rng, N)
    qt, Pt = _points(rng, m)
    z = rng.standard_normal(2 * N)
    hyp, s2 = _hyp(fam, N)
    Kxx = oracle.build_K(fam, q, P, q, P, hyp, threads=16)
    Ktx = oracle.build_K(fam, qt, Pt, q, P, hyp, threads=16)
    Kxt = oracle.build_K(fam, q, P, qt, Pt, hyp, threads=16)
    Ktt = oracle.build_K(fam, qt, Pt, qt, Pt, hyp, threads=16)
    S, cond = _sigma(Kxx, s2, Ktx, Kxt, Ktt)
    return (q, P, z, hyp, s2), (qt, Pt), _blocks(S, m, 2), _blocks(Ktt, m, 2), cond


@pytest.mark.parametrize("fam,N,m", [("A", 100, 37),      # n = 200: the transposed panel solve
                                     ("A", 512, 50),      # n = 1024: strip solves, one pass
                                     ("A", 2048, 300),    # n = 4096: 3 chunks (128, 128, 44 points), 4 + 4 + 2 passes
                                     ("B", 512, 50), ("C", 512, 50), ("D", 512, 50)])
def test_predict_cov_pairs_vs_oracle(oracle, fam, N, m):
    from sympgpr_amd.fit import SympFit
    (q, P, z, hyp, s2), (qt, Pt), Sig, Kss, cond = _pair_case(oracle, fam, N, m, 300 + N)
    assert cond <= 1e6
    with SympFit(fam, q, P, z, hyp, s2) as f:
        f.run()
        mean, cov = f.predict_cov(qt, Pt)
        op, oq = f.predict_rows(qt, Pt)
        mean2, cov2 = f.predict_cov(qt, Pt)
    assert mean.shape == (m, 2) and cov.shape == (m, 2, 2)
    assert np.array_equal(mean[:, 0], op) and np.array_equal(mean[:, 1], oq)
    assert np.array_equal(mean, mean2) and np.array_equal(cov, cov2), "two identical calls differ"
    _check(cov, Sig, Kss, cond, "%s N=%d m=%d" % (fam, N, m))


@pytest.mark.parametrize("N,m", [(1024, 300),    # n = 1024, strips; 2 chunks (256 + 44 points)
                                 (300, 40)])     # n = 300: not a multiple of 128, the transposed panel solve
def test_predict_cov_reg_vs_oracle(oracle, N, m):
    from sympgpr_amd.fit import SympFit
    rng = np.random.default_rng(700 + N)
    q, P = _points(rng, N)
    qt, Pt = _points(rng, m)
    z = rng.standard_normal(N)
    hyp, s2 = _hyp("A", N)
    Kxx = oracle.buildKreg("A", q, P, q, P, hyp, threads=16)
    Ktx = oracle.buildKreg("A", qt, Pt, q, P, hyp, threads=16)
    Kxt = oracle.buildKreg("A", q, P, qt, Pt, hyp, threads=16)
    Ktt = oracle.buildKreg("A", qt, Pt, qt, Pt, hyp, threads=16)
    S, cond = _sigma(Kxx, s2, Ktx, Kxt, Ktt)
    assert cond <= 1e6
    with SympFit("A", q, P, z, hyp, s2, reg=True) as f:
        f.run()
        mean, cov = f.predict_cov(qt, Pt)
        op, _ = f.predict_rows(qt, Pt)
    assert mean.shape == (m, 1) and cov.shape == (m, 1, 1)
    assert np.array_equal(mean[:, 0], op)
    _check(cov, _blocks(S, m, 1), _blocks(Ktt, m, 1), cond, "reg N=%d m=%d" % (N, m))


@pytest.mark.parametrize("fam,d,N,m", [("A", 2, 256, 100),    # n = 1024, D = 4: chunks of 64 points
                                       ("C", 3, 128, 100)])   # n = 768, D = 6: chunks of 42 points
def test_predict_pairs_cov_vs_oracle(oracle, fam, d, N, m):
    from sympgpr_amd.fit import SympFit
    rng = np.random.default_rng(900 + N)
    X = np.column_stack([rng.uniform(0, 2 * np.pi, (N, d)), rng.uniform(-3, 3, (N, d))])
    Xt = np.column_stack([rng.uniform(0, 2 * np.pi, (m, d)), rng.uniform(-3, 3, (m, d))])
    z = rng.standard_normal(2 * d * N)
    hyp, s2 = _hyp(fam, N, d)
    S, cond = _sigma(oracle.build_K_nd(fam, X, X, hyp), s2, oracle.build_K_nd(fam, Xt, X, hyp),
                     oracle.build_K_nd(fam, X, Xt, hyp), oracle.build_K_nd(fam, Xt, Xt, hyp))
    Ktt = oracle.build_K_nd(fam, Xt, Xt, hyp)
    assert cond <= 1e6
    with SympFit.pairs(fam, X, z, hyp, s2) as f:
        f.run()
        mean, cov = f.predict_pairs_cov(Xt)
        ref_mean = f.predict_pairs(Xt)
    D = 2 * d
    assert mean.shape == (m, D) and cov.shape == (m, D, D)
    assert np.array_equal(mean, ref_mean)
    _check(cov, _blocks(S, m, D), _blocks(Ktt, m, D), cond, "%s d=%d N=%d m=%d" % (fam, d, N, m))


@pytest.mark.parametrize("N", [100, 512])   # n = 200 (transposed panel solve), n = 1024 (strips)
def test_predict_cov_chunking_is_invisible(N):
    """a point's covariance does not depend on the chunk it is computed in, nor on the other points of the call"""
    from sympgpr_amd.fit import SympFit
    rng = np.random.default_rng(11 + N)
    q, P = _points(rng, N)
    qt, Pt = _points(rng, 300)
    hyp, s2 = _hyp("A", N)
    with SympFit("A", q, P, rng.standard_normal(2 * N), hyp, s2) as f:
        f.run()
        mean, cov = f.predict_cov(qt, Pt)
        for t in (0, 130, 270):                # first, second and (partial) third chunk of 128 points
            m1, c1 = f.predict_cov(qt[t:t + 1], Pt[t:t + 1])
            assert np.array_equal(c1[0], cov[t]), t
            assert np.array_equal(m1[0], mean[t]), t


def test_predict_cov_at_training_points():
    """small noise: at a training point the posterior variance is far below the prior"""
    from sympgpr_amd.fit import SympFit
    rng = np.random.default_rng(21)
    N = 100
    q, P = _points(rng, N)
    hyp, _ = _hyp("A", N)
    s2 = 1e-4 / hyp[0] ** 2
    with SympFit("A", q, P, rng.standard_normal(2 * N), hyp, s2) as f:
        f.run()
        _, cov = f.predict_cov(q[:20], P[:20])
        _, prior = f.predict_cov(q[:20] + np.pi, P[:20] + 40.0)       # far from every training point: the prior itself
    var, var0 = np.diagonal(cov, axis1=1, axis2=2), np.diagonal(prior, axis1=1, axis2=2)
    print("variance / prior at training points: max %.3g" % (var / var0).max())
    assert np.all(var <= 1e-3 * var0)


def test_predict_cov_errors():
    from sympgpr_amd import _lib as L, SympGPRError
    from sympgpr_amd.fit import SympFit
    rng = np.random.default_rng(3)
    N = 64
    q, P = _points(rng, N)
    hyp, s2 = _hyp("A", N)
    Xt, mean, cov = np.zeros((2, 2), order="F"), np.zeros(4), np.zeros(8)
    args = lambda f: (f._h, 2, L.dptr(Xt), 2, L.dptr(mean), L.dptr(cov))
    with SympFit("A", q, P, rng.standard_normal(2 * N), hyp, s2) as f:
        assert f._lib.sgpr_fit_predict_cov(*args(f)) == L.E_STATE      # before run()
        with pytest.raises(SympGPRError):
            f.predict_cov(q[:2], P[:2])
        f.run()
        mean0, cov0 = f.predict_cov(np.empty(0), np.empty(0))
        assert mean0.shape == (0, 2) and cov0.shape == (0, 2, 2)
        assert f._lib.sgpr_fit_predict_cov(f._h, 2, L.dptr(Xt), 1, L.dptr(mean), L.dptr(cov)) == L.E_ARG   # ldxt < m
        assert f._lib.sgpr_fit_predict_cov(f._h, -1, L.dptr(Xt), 2, L.dptr(mean), L.dptr(cov)) == L.E_ARG
    with SympFit("A", q, P, rng.standard_normal(N), hyp, s2, block="qq") as f:
        f.run()
        assert f._lib.sgpr_fit_predict_cov(*args(f)) == L.E_STATE


def test_predict_cov_n16384():
    """a size users run: against the existing two-sided block solve on the device (solve_rhs on K*^T gives Ky^-1 K*^T),
    K* (Ky^-1 K*^T) formed in numpy from the device Gram builder.  Also shows the forward-only path agrees with it."""
    from sympgpr_amd import ops
    from sympgpr_amd.fit import SympFit
    rng = np.random.default_rng(16384)
    N, m = 8192, 64
    q, P = _points(rng, N)
    qt, Pt = _points(rng, m)
    hyp, s2 = _hyp("A", N)
    Kxt = np.empty((2 * N, 2 * m), order="F")
    Ktx = np.empty((2 * m, 2 * N), order="F")
    Ktt = np.empty((2 * m, 2 * m), order="F")
    ops.build_k(q, P, qt, Pt, hyp, Kxt, family="A")
    ops.build_k(qt, Pt, q, P, hyp, Ktx, family="A")
    ops.build_k(qt, Pt, qt, Pt, hyp, Ktt, family="A")
    with SympFit("A", q, P, rng.standard_normal(2 * N), hyp, s2) as f:
        f.run()
        mean, cov = f.predict_cov(qt, Pt)
        op, oq = f.predict_rows(qt, Pt)
        X = f.solve_rhs(Kxt)
        cond = f.cond_estimate(40)["cond"]
    assert cond <= 1e6
    assert np.array_equal(mean, np.column_stack((op, oq)))
    S = Ktt - Ktx @ X
    _check(cov, _blocks(S, m, 2), _blocks(Ktt, m, 2), cond, "A N=8192 m=64 (device reference)")


def test_predict_cov_give_up_is_reported():
    """a strip pass that gives up on a hand-off (forced through the probe library's tunable, as for the two-sided block
    solves) makes the call fail with SGPR_E_HIP instead of returning what the pass left; the next call is clean"""
    from sympgpr_amd import _lib as L
    from sympgpr_amd.fit import SympFit
    probe = L.load_probe_library()
    rng = np.random.default_rng(31)
    N = 512                                      # n = 1024: strips; 50 points = 100 columns = 2 passes
    q, P = _points(rng, N)
    qt, Pt = _points(rng, 50)
    hyp, s2 = _hyp("A", N)
    with SympFit("A", q, P, rng.standard_normal(2 * N), hyp, s2) as f:
        f.run()
        mean, cov = f.predict_cov(qt, Pt)
        L.check(probe.sgpr_probe_tune(b"trsm_force_giveup_pass", 1.0))
        try:
            with pytest.raises(L.SympGPRError):
                f.predict_cov(qt, Pt)
        finally:
            L.check(probe.sgpr_probe_tune(b"trsm_force_giveup_pass", -1.0))
        mean2, cov2 = f.predict_cov(qt, Pt)
    assert np.array_equal(mean, mean2) and np.array_equal(cov, cov2)
