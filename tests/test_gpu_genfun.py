"""The generating function F of a fit on the device (sgpr_fit_predict_genfun: SympFit.predict_genfun / predict_pairs_genfun,
maps.genfun_along) against tests/ref_genfun.py, the NumPy restatement tests/test_genfun_cpu.py pins to the reference.

Mean: |F_dev - F_ref| <= (32 + n0) eps T_t per point, T_t = sum_j sum_c |term|: n0 eps T is the worst case of any summation
order, 32 eps covers the pair evaluation (the pair forms are pinned to the Fortran at <= 4e-15 ~ 18 eps; the rest is the
product with g and alpha).  The host reference uses the device fit's own alpha().  Every reference value has to exceed 1e3 x
its tolerance, so a kernel that returns zeros cannot pass.
Variance: 100 cond(Ky) eps max prior, tests/test_gpu_predict_cov.py's, with cond <= 1e6 asserted."""
import numpy as np
import pytest

from tests import ref_genfun as RG
from tests.test_genfun_cpu import d1_case, nd_case

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _check_mean(F, ref, n0, what):
    tol = (32 + n0) * EPS * ref["T"]
    err = np.abs(F - ref["F"])
    print("%s: max err / tol = %.3g   min |F_ref| / tol = %.3g" % (what, (err / tol).max(), (np.abs(ref["F"]) / tol).min()))
    assert np.all(np.abs(ref["F"]) > 1e3 * tol), what
    assert np.all(err <= tol), (what, (err / tol).max())


@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])      # one lane; the wave's tail; five trips with a ragged last one
def test_mean_d1_vs_ref(oracle, fam, N):
    from sympgpr_amd.fit import SympFit
    q, P, z, qt, Pt, hyp, s2 = d1_case(N, fam)
    with SympFit(fam, q, P, z, hyp, s2) as f:
        f.run()
        alpha = f.alpha()
        F = f.predict_genfun(qt, Pt)
    assert F.shape == (37,)
    _check_mean(F, RG.genfun_d1(oracle, fam, q, P, hyp, alpha, qt, Pt), N, "%s N=%d" % (fam, N))


@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("N", [40, 130])
def test_mean_pairs_vs_ref(fam, d, N):
    from sympgpr_amd.fit import SympFit
    X, z, Xt, hyp, s2 = nd_case(N, d, fam)
    with SympFit.pairs(fam, X, z, hyp, s2) as f:
        f.run()
        alpha = f.alpha()
        F = f.predict_pairs_genfun(Xt)
    ref = RG.genfun_nd(fam, X, hyp, alpha, Xt)
    _check_mean(F, ref, N, "%s d=%d N=%d" % (fam, d, N))
    if d == 1:      # the same fit through the reference's layout: its own alpha (the d = 1 solve), the same bound
        with SympFit(fam, X[:, 0], X[:, 1], z, hyp, s2) as f1:
            f1.run()
            F1 = f1.predict_genfun(Xt[:, 0], Xt[:, 1])
            ref1 = RG.genfun_nd(fam, X, hyp, f1.alpha(), Xt)
        _check_mean(F1, ref1, N, "%s d=1 N=%d through SympFit(...)" % (fam, N))
        assert np.all(np.abs(F - F1) <= (32 + N) * EPS * ref["T"])


@pytest.mark.parametrize("fam", ["A", "B", "C", "D", "USER"])
@pytest.mark.parametrize("d", [1, 2])
def test_gradient_of_F_is_what_the_predictors_return(fam, d):
    """central differences of F on the device (h = 1e-5 l) against predict_rows / predict_pairs, every family"""
    from sympgpr_amd import _lib as L
    from sympgpr_amd.fit import SympFit
    N, m = 100, 37
    has_p = L.family_has_p(fam)
    X, z, Xt, hyp, s2 = nd_case(N, d, "D" if has_p else "A")
    h = 1e-5 * hyp[0]
    grad = np.empty((m, 2 * d))
    if d == 1:
        with SympFit(fam, X[:, 0], X[:, 1], z, hyp, s2) as f:
            f.run()
            rows = np.column_stack(f.predict_rows(Xt[:, 0], Xt[:, 1]))
            grad[:, 0] = (f.predict_genfun(Xt[:, 0] + h, Xt[:, 1]) - f.predict_genfun(Xt[:, 0] - h, Xt[:, 1])) / (2 * h)
            grad[:, 1] = (f.predict_genfun(Xt[:, 0], Xt[:, 1] + h) - f.predict_genfun(Xt[:, 0], Xt[:, 1] - h)) / (2 * h)
    else:
        with SympFit.pairs(fam, X, z, hyp, s2) as f:
            f.run()
            rows = f.predict_pairs(Xt)
            for a in range(2 * d):
                e = np.zeros(2 * d)
                e[a] = h
                grad[:, a] = (f.predict_pairs_genfun(Xt + e) - f.predict_pairs_genfun(Xt - e)) / (2 * h)
    scale = max(1.0, np.abs(rows).max())
    err = np.abs(grad - rows).max()
    print("%s d=%d: max|dF - rows| = %.3g  tol %.3g  max|rows| %.3g" % (fam, d, err, 1e-6 * scale, np.abs(rows).max()))
    assert np.abs(rows).max() > 1e-3          # not a comparison of zeros
    assert err <= 1e-6 * scale


@pytest.mark.parametrize("fam,d,N,m", [("A", 1, 100, 37),     # n = 200: the transposed panel solve
                                       ("A", 1, 512, 37),     # n = 1024: the strip passes
                                       ("B", 1, 512, 37),
                                       ("A", 1, 512, 300),    # two chunks (256 + 44 points)
                                       ("C", 2, 256, 37)])    # n = 1024, D = 4
def test_variance_vs_host(oracle, fam, d, N, m):
    from sympgpr_amd.fit import SympFit
    X, z, Xt, hyp, s2 = nd_case(N, d, fam, m=m, seed=7)
    Ky = oracle.build_K_nd(fam, X, X, hyp) + abs(s2) * np.eye(2 * d * N)
    cond = float(np.linalg.cond(Ky))
    assert cond <= 1e6
    x0 = np.append(np.full(d, 3.0), np.full(d, 0.5))
    Xr = np.vstack((Xt, x0))                            # the reference point as one more test point: its F is exactly 0
    with (SympFit(fam, X[:, 0], X[:, 1], z, hyp, s2) if d == 1 else SympFit.pairs(fam, X, z, hyp, s2)) as f:
        f.run()
        alpha = f.alpha()
        call = (lambda Y, **kw: f.predict_genfun(Y[:, 0], Y[:, 1], **kw)) if d == 1 else f.predict_pairs_genfun
        F, var = call(Xt, var=True)
        Fr, varr = call(Xr, ref=x0, var=True)
        F_only = call(Xt)
    res = RG.genfun_nd(fam, X, hyp, alpha, Xr)
    hv, prior = RG.host_variance(res, Ky)
    hvr, priorr = RG.host_variance(res, Ky, ref=m)
    tol, tolr = 100 * cond * EPS * prior.max(), 100 * cond * EPS * priorr.max()
    print("%s d=%d N=%d m=%d: cond %.3g  max|var - host| = %.3g (tol %.3g)  with ref %.3g (tol %.3g)  var %.3g .. %.3g, "
          "of differences %.3g .. %.3g" % (fam, d, N, m, cond, np.abs(var - hv[:m]).max(), tol, np.abs(varr - hvr).max(), tolr,
                                           var.min(), var.max(), varr.min(), varr.max()))
    assert var.shape == (m,) and varr.shape == (m + 1,)
    assert np.array_equal(F, F_only), "the variance changes the mean"
    assert np.all(np.abs(var - hv[:m]) <= tol)
    assert np.all(np.abs(varr - hvr) <= tolr)
    assert np.all(var >= -tol) and np.all(var <= prior[:m] + tol)
    assert np.all(np.abs(F - res["F"][:m]) <= (32 + N) * EPS * res["T"][:m])
    assert np.all(np.abs(Fr[:m] - (res["F"][:m] - res["F"][m])) <= (32 + N) * EPS * (res["T"][:m] + res["T"][m]))
    assert Fr[m] == 0.0 and abs(varr[m]) <= tolr


def test_bits_do_not_depend_on_the_call():
    """a repeated call returns identical arrays; F and var of a point are the same bits alone, first, last or among 300 points
    (chunks of 256); alpha, nll and predict_rows are left as they were"""
    from sympgpr_amd.fit import SympFit
    N = 512
    X, z, Xt, hyp, s2 = nd_case(N, 1, "A", m=300, seed=3)
    x0 = np.array([1.0, -0.5])
    with SympFit("A", X[:, 0], X[:, 1], z, hyp, s2) as f:
        f.run()
        before = (f.alpha(), f.nll(), f.predict_rows(Xt[:5, 0], Xt[:5, 1]))
        for ref in (None, x0):
            F, var = f.predict_genfun(Xt[:, 0], Xt[:, 1], ref=ref, var=True)
            F2, var2 = f.predict_genfun(Xt[:, 0], Xt[:, 1], ref=ref, var=True)
            assert np.array_equal(F, F2) and np.array_equal(var, var2), "two identical calls differ"
            for t in (0, 130, 299):                  # first and second chunk, the last point
                F1, v1 = f.predict_genfun(Xt[t:t + 1, 0], Xt[t:t + 1, 1], ref=ref, var=True)
                assert F1[0] == F[t] and v1[0] == var[t], ("alone", t)
            sel = np.r_[270, 0:40]                   # point 270 first, point 39 last
            Fs, vs = f.predict_genfun(Xt[sel, 0], Xt[sel, 1], ref=ref, var=True)
            assert np.array_equal(Fs, F[sel]) and np.array_equal(vs, var[sel])
        after = (f.alpha(), f.nll(), f.predict_rows(Xt[:5, 0], Xt[:5, 1]))
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    assert np.array_equal(before[2][0], after[2][0]) and np.array_equal(before[2][1], after[2][1])


def test_edges():
    from sympgpr_amd import SympGPRError
    from sympgpr_amd.fit import SympFit
    N = 64
    X, z, Xt, hyp, s2 = nd_case(N, 1, "A")
    q, P = Xt[:, 0].copy(), Xt[:, 1].copy()
    with SympFit("A", X[:, 0], X[:, 1], z, hyp, s2) as f:
        with pytest.raises(SympGPRError) as e_rows:
            f.predict_rows(q, P)
        with pytest.raises(SympGPRError) as e_gen:
            f.predict_genfun(q, P)
        assert type(e_gen.value) is type(e_rows.value) and "not solved" in str(e_gen.value) and "not solved" in str(e_rows.value)
        f.run()
        F, var = f.predict_genfun(q, P, ref=[1.0, 0.0], var=True)
        qn = q.copy()
        qn[5] = np.nan
        Fn, varn = f.predict_genfun(qn, P, ref=[1.0, 0.0], var=True)
        keep = np.arange(len(q)) != 5
        assert np.isnan(Fn[5]) and np.isnan(varn[5])
        assert np.array_equal(Fn[keep], F[keep]) and np.array_equal(varn[keep], var[keep])
        F0, var0 = f.predict_genfun(np.empty(0), np.empty(0), var=True)
        assert F0.shape == (0,) and var0.shape == (0,)
        assert f.predict_pairs_genfun(np.empty((0, 2))).shape == (0,)
        with pytest.raises(ValueError):
            f.predict_genfun(q, P, ref=[1.0, 0.0, 2.0])
    with SympFit("A", X[:, 0], X[:, 1], z[:N], hyp, s2, reg=True) as f:
        f.run()
        with pytest.raises(ValueError):
            f.predict_genfun(q, P)
        with pytest.raises(ValueError):
            f.predict_pairs_genfun(Xt)
        from sympgpr_amd import _lib as L
        Fb = np.zeros(len(q))
        assert f._lib.sgpr_fit_predict_genfun(f._h, len(q), L.dptr(np.asfortranarray(Xt)), len(q), None, L.dptr(Fb), None) == L.E_ARG
    X2, z2, Xt2, hyp2, s22 = nd_case(40, 2, "A")
    with SympFit.pairs("A", X2, z2, hyp2, s22) as f:
        f.run()
        with pytest.raises(ValueError):
            f.predict_genfun(q, P)                   # the d = 1 entry on a d = 2 fit
        with pytest.raises(ValueError):
            f.predict_pairs_genfun(Xt)               # (m, 2) points on a d = 2 fit


@pytest.mark.parametrize("d", [1, 2])
def test_genfun_along(d):
    """F(q_k, P_{k+1}) along a 5-step map of 7 orbits: the bits of predict_*_genfun on the stacked points; an orbit that starts at
    NaN gives a NaN column"""
    from sympgpr_amd import maps
    from sympgpr_amd.fit import SympFit
    N, nm, Nt = 100, 6, 7
    rng = np.random.default_rng(40 + d)
    q, p = rng.uniform(0, 2 * np.pi, (N, d)), rng.uniform(-1, 1, (N, d))
    Pn = p - 0.05 * np.sin(q)                          # a kicked rotor per pair: P = p - eps sin q, Q = q + eps P
    Qn = q + 0.1 * Pn
    X, z = np.column_stack((q, Pn)), np.concatenate(((p - Pn).T.ravel(), (Qn - q).T.ravel()))
    hyp, s2 = [1.5] * (2 * d) + [1.0], 1e-4
    Q0, P0 = rng.uniform(1, 5, (Nt, d)), rng.uniform(-0.5, 0.5, (Nt, d))
    Q0[3, 0] = np.nan
    ref = X[0]
    with SympFit.pairs("A", X, z, hyp, s2) as f:
        f.run()
        qmap, pmap = f.applymap_pairs(nm, Q0, P0)
        assert np.all(np.isfinite(qmap[:, np.arange(Nt) != 3])), "the test's map lost an orbit it should keep"
        for r in (None, ref):
            if d == 1:
                G = maps.genfun_along(f, qmap[:, :, 0], pmap[:, :, 0], ref=r)
                G3 = maps.genfun_along(f, qmap, pmap, ref=r)
                assert np.array_equal(G, G3, equal_nan=True)
                want = f.predict_genfun(qmap[:-1, :, 0].ravel(), pmap[1:, :, 0].ravel(), ref=r)
            else:
                G = maps.genfun_along(f, qmap, pmap, ref=r)
                want = f.predict_pairs_genfun(np.hstack((qmap[:-1].reshape(-1, d), pmap[1:].reshape(-1, d))), ref=r)
            assert G.shape == (nm - 1, Nt)
            assert np.array_equal(G, want.reshape(nm - 1, Nt), equal_nan=True)
            assert np.all(np.isnan(G[:, 3])) and np.all(np.isfinite(G[:, np.arange(Nt) != 3]))
            assert np.abs(G[:, np.arange(Nt) != 3]).max() > 0.0
