"""The NLL gradient in all hyperparameters on the device (sgpr_fit_nll_grad_full, SympFit.nll_grad_full).

Reference: Ky from the oracle's host Gram builders (build_K, buildKreg, build_K_nd), factored on the host, and
    grad_theta = 1/2 sum_ij (Ky^-1 - alpha alpha^T)_ij dKy_ij / dtheta
in float64 NumPy.  dK is exact for lx / ly (oracle.build_dK / build_dKreg) and for sig (K / sig); for a period p and the
d > 1 lengths it is a central difference of the oracle's K with a relative step of 1e-5.  Each component is compared
against the size of its own sum, S = 1/2 sum_ij |W_ij dKy_ij|: |g - g_ref| <= tol S with tol = max(rtol, 100 cond eps)
(rtol 1e-9 for exact components, 1e-6 for difference-based ones; cond from NumPy on the host Ky).  Mid-size and large
fits are checked against central differences of the device's own nll()."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
USER_AS_C = "exp(-(x_a - x_b)**2/(2*lx**2))*exp(-(y_a - y_b)**2/(2*ly**2))"


def _user_is_c(golden_dir):
    import os
    uf = np.load(os.path.join(golden_dir, "user_family.npz"))
    return str(uf["definition"]) == USER_AS_C


def _ell(N, d=1):
    return 2.0 * np.sqrt(12 * np.pi) * N ** (-1.0 / (2 * d))


def _pair_hyp(fam, N):
    l = _ell(N)
    return ([0.9 * l, 1.1 * l, 0.45, 1.3] if fam == "D" else [0.9 * l, 1.1 * l, 1.3]), 1e-2 / l**2


def _nd_hyp(fam, N, d):
    l = _ell(N, d) * np.linspace(0.9, 1.15, 2 * d)
    h = list(l) + ([0.45 + 0.05 * m for m in range(d)] if fam == "D" else []) + [1.2]
    return np.array(h), 1e-2 / l.mean() ** 2


def _central(build, hyp, k, rel=1e-5):
    h = np.array(hyp, dtype=float)
    step = rel * abs(h[k])
    hp, hm = h.copy(), h.copy()
    hp[k] += step
    hm[k] -= step
    return (build(hp) - build(hm)) / (2 * step)


def _reference(build, hyp, s2, z, exact):
    """-> (grad_ref, scale, cond, exact_mask); build(hyp) = K (no noise); exact: {index: dK} for the exact components"""
    K = build(np.asarray(hyp, dtype=float))
    n = K.shape[0]
    Ky = K + abs(s2) * np.eye(n)
    cond = float(np.linalg.cond(Ky))
    Kinv = np.linalg.inv(Ky)
    Kinv = 0.5 * (Kinv + Kinv.T)
    alpha = np.linalg.solve(Ky, z)
    W = Kinv - np.outer(alpha, alpha)
    nh = len(hyp)
    g, S, ex = np.empty(nh + 1), np.empty(nh + 1), np.zeros(nh + 1, bool)
    for k in range(nh):
        if k == nh - 1:
            dK, ex[k] = K / hyp[-1], True
        elif k in exact:
            dK, ex[k] = exact[k], True
        else:
            dK = _central(build, hyp, k)
        g[k] = 0.5 * np.sum(W * dK)
        S[k] = 0.5 * np.sum(np.abs(W * dK))
    sgn = -1.0 if s2 < 0 else 1.0
    g[nh] = sgn * 0.5 * (np.trace(Kinv) - alpha @ alpha)
    S[nh] = 0.5 * (np.trace(np.abs(Kinv)) + alpha @ alpha)
    ex[nh] = True
    return g, S, cond, ex


def _compare(g, ref, what):
    gref, S, cond, ex = ref
    assert g.shape == gref.shape
    assert np.all(np.isfinite(g))
    tol = np.where(ex, max(1e-9, 100 * cond * EPS), max(1e-6, 100 * cond * EPS)) * S
    err = np.abs(g - gref)
    print("%s: cond %.3g  max err/S %.3g  (exact %s)" % (what, cond, (err / np.maximum(S, 1e-300)).max(), ex.astype(int)))
    assert np.all(err <= tol), (what, g, gref, err / S)


def _pair_case(oracle, fam, N, seed, s2_sign=1.0, ofam=None):
    ofam = ofam or fam
    rng = np.random.default_rng(seed)
    q, P = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N)
    z = rng.standard_normal(2 * N)
    hyp, s2 = _pair_hyp(fam, N)
    s2 *= s2_sign
    build = lambda h: oracle.build_K(ofam, q, P, q, P, h, threads=16)
    exact = {}
    if ofam != "D":
        dKx, dKy = oracle.build_dK(ofam, q, P, q, P, hyp)
        exact = {0: dKx, 1: dKy}
    return (q, P, z, hyp, s2), _reference(build, hyp, s2, z, exact)


@pytest.mark.parametrize("fam,N", [("A", 700),    # n = 1400 < nb: one panel, not a multiple of 128
                                   ("B", 300), ("C", 300), ("D", 700),
                                   ("A", 1),      # N = 1
                                   ("C", 1100)])  # n = 2200: two panels (2048 + 152), the q / P boundary inside the first
def test_pairs_vs_host(oracle, fam, N):
    from sympgpr_amd.fit import SympFit
    (q, P, z, hyp, s2), ref = _pair_case(oracle, fam, N, 100 + N)
    with SympFit(fam, q, P, z, hyp, s2) as f:
        f.run()
        g = f.nll_grad_full()
        assert g.shape == (len(hyp) + 1,)
        _compare(g, ref, "pairs %s N=%d" % (fam, N))
        if N > 1:
            old = f.nll_grad()
            np.testing.assert_allclose(g[:2], old, rtol=1e-9, atol=1e-9 * np.abs(ref[1][:2]).max())


def test_pairs_negative_noise(oracle):
    from sympgpr_amd.fit import SympFit
    (q, P, z, hyp, s2), ref = _pair_case(oracle, "A", 300, 7, s2_sign=-1.0)
    assert s2 < 0
    with SympFit("A", q, P, z, hyp, s2) as f:
        f.run()
        g = f.nll_grad_full()
    _compare(g, ref, "pairs A, sig2n < 0")
    (_, _, _, _, s2p), refp = _pair_case(oracle, "A", 300, 7)
    assert ref[0][-1] == pytest.approx(-refp[0][-1], rel=1e-12)


def test_user_pairs_vs_family_c(oracle, golden_dir):
    if not _user_is_c(golden_dir):
        pytest.skip("USER_FAMILY has been edited: no hand-written twin to compare with")
    from sympgpr_amd.fit import SympFit
    (q, P, z, hyp, s2), ref = _pair_case(oracle, "USER", 600, 11, ofam="C")
    with SympFit("USER", q, P, z, hyp, s2) as f:
        f.run()
        g = f.nll_grad_full()
    _compare(g, ref, "pairs USER (= C) N=600")


@pytest.mark.parametrize("fam,N", [("A", 1500), ("B", 900), ("C", 2500), ("D", 1500), ("A", 1)])
def test_reg_vs_host(oracle, fam, N):
    from sympgpr_amd.fit import SympFit
    rng = np.random.default_rng(200 + N)
    x, y = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N)
    z = rng.standard_normal(N)
    hyp, s2 = _pair_hyp(fam, 2 * N)
    build = lambda h: oracle.buildKreg(fam, x, y, x, y, h, threads=16)
    exact = {}
    if fam != "D":
        dKx, dKy = oracle.build_dKreg(fam, x, y, x, y, hyp)
        exact = {0: dKx, 1: dKy}
    ref = _reference(build, hyp, s2, z, exact)
    with SympFit(fam, x, y, z, hyp, s2, reg=True) as f:
        f.run()
        g = f.nll_grad_full()
        _compare(g, ref, "reg %s N=%d" % (fam, N))
        if N > 1:
            np.testing.assert_allclose(g[:2], f.nll_grad(), rtol=1e-9, atol=1e-9 * np.abs(ref[1][:2]).max())


@pytest.mark.parametrize("fam,d,N", [("A", 2, 600),    # n = 2400: two panels, three part boundaries inside the first
                                     ("C", 2, 160),
                                     ("A", 3, 333),    # n = 1998
                                     ("D", 3, 200),
                                     ("B", 2, 200)])
def test_nd_vs_host(oracle, fam, d, N):
    from sympgpr_amd.fit import SympFit
    rng = np.random.default_rng(300 + 10 * d + N)
    X = np.column_stack([rng.uniform(0, 2 * np.pi, N) for _ in range(d)] + [rng.uniform(-3, 3, N) for _ in range(d)])
    z = rng.standard_normal(2 * d * N)
    hyp, s2 = _nd_hyp(fam, N, d)
    build = lambda h: oracle.build_K_nd(fam, X, X, h)
    ref = _reference(build, hyp, s2, z, {})
    with SympFit.pairs(fam, X, z, hyp, s2) as f:
        f.run()
        g = f.nll_grad_full()
    assert g.shape == (len(hyp) + 1,)
    _compare(g, ref, "nd %s d=%d N=%d" % (fam, d, N))


def test_user_nd_vs_family_c(oracle, golden_dir):
    if not _user_is_c(golden_dir):
        pytest.skip("USER_FAMILY has been edited: no hand-written twin to compare with")
    from sympgpr_amd.fit import SympFit
    d, N = 2, 250
    rng = np.random.default_rng(41)
    X = np.column_stack([rng.uniform(0, 2 * np.pi, N) for _ in range(d)] + [rng.uniform(-3, 3, N) for _ in range(d)])
    z = rng.standard_normal(2 * d * N)
    hyp, s2 = _nd_hyp("C", N, d)
    ref = _reference(lambda h: oracle.build_K_nd("C", X, X, h), hyp, s2, z, {})
    with SympFit.pairs("USER", X, z, hyp, s2) as f:
        f.run()
        g = f.nll_grad_full()
    _compare(g, ref, "nd USER (= C) d=2")


def _fd_check(make, hyp, s2, comps, what, rel=1e-4, rtol=1e-5):
    """central differences of the device's own nll() against the device gradient"""
    hyp = np.array(hyp, dtype=float)
    with make(hyp, s2) as f:
        f.run()
        g = f.nll_grad_full()
        gscale = np.abs(g).max()
        for k in comps:
            h = rel * abs(hyp[k] if k < len(hyp) else s2)
            vals = []
            for sgn in (1.0, -1.0):
                hp, sp = hyp.copy(), s2
                if k < len(hyp):
                    hp[k] += sgn * h
                else:
                    sp += sgn * h
                f.set_hyp(hp, sp)
                f.run()
                vals.append(f.nll())
            fd = (vals[0] - vals[1]) / (2 * h)
            print("%s: component %d  grad %.12g  fd %.12g  rel %.3g" % (what, k, g[k], fd, abs(fd - g[k]) / max(abs(g[k]), 1e-3 * gscale)))
            assert abs(fd - g[k]) <= rtol * max(abs(g[k]), 1e-3 * gscale), (what, k, g[k], fd)
    return g


def test_pairs_fd_mid():
    from sympgpr_amd.fit import SympFit
    N = 8500                                    # n = 17 000: 5 panels (4 x 4096 + 616), N not a multiple of nb
    rng = np.random.default_rng(5)
    q, P, z = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N), rng.standard_normal(2 * N)
    hyp, s2 = _pair_hyp("D", 2 * N)
    _fd_check(lambda h, s: SympFit("D", q, P, z, h, s), hyp, s2, range(len(hyp) + 1), "pairs D n=17000")


def test_reg_fd_mid():
    from sympgpr_amd.fit import SympFit
    N = 16384
    rng = np.random.default_rng(6)
    x, y, z = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N), rng.standard_normal(N)
    hyp, s2 = _pair_hyp("A", N)
    _fd_check(lambda h, s: SympFit("A", x, y, z, h, s, reg=True), hyp, s2, range(len(hyp) + 1), "reg A n=16384")


def test_nd_fd_mid():
    from sympgpr_amd.fit import SympFit
    d, N = 3, 3000                              # n = 18 000
    rng = np.random.default_rng(8)
    X = np.column_stack([rng.uniform(0, 2 * np.pi, N) for _ in range(d)] + [rng.uniform(-3, 3, N) for _ in range(d)])
    z = rng.standard_normal(2 * d * N)
    hyp, s2 = _nd_hyp("D", N, d)
    _fd_check(lambda h, s: SympFit.pairs("D", X, z, h, s), hyp, s2, range(len(hyp) + 1), "nd D d=3 n=18000")


def test_purity_and_determinism(oracle):
    from sympgpr_amd.fit import SympFit
    rng = np.random.default_rng(9)
    N = 1100
    q, P, z = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N), rng.standard_normal(2 * N)
    qt, Pt = rng.uniform(0, 2 * np.pi, 20), rng.uniform(-3, 3, 20)
    hyp, s2 = _pair_hyp("A", N)
    with SympFit("A", q, P, z, hyp, s2) as f:
        f.run()
        a0, v0, r0, c0 = f.alpha(), f.nll(), f.predict_rows(qt, Pt), f.predict_cov(qt, Pt)
        g1 = f.nll_grad_full()
        a1, v1, r1, c1 = f.alpha(), f.nll(), f.predict_rows(qt, Pt), f.predict_cov(qt, Pt)
        g2 = f.nll_grad_full()
    assert np.array_equal(a0, a1) and v0 == v1
    assert all(np.array_equal(u, w) for u, w in zip(r0, r1)) and all(np.array_equal(u, w) for u, w in zip(c0, c1))
    assert np.array_equal(g1, g2), "two calls differ"


def test_errors():
    from sympgpr_amd import _lib as L
    from sympgpr_amd.fit import SympFit
    rng = np.random.default_rng(10)
    N = 200
    q, P, z = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N), rng.standard_normal(2 * N)
    hyp, s2 = _pair_hyp("A", N)
    lib = L.load_library()
    with SympFit("A", q, P, z, hyp, s2) as f:
        with pytest.raises(RuntimeError):
            f.nll_grad_full()                  # before run()
        g = np.zeros(len(hyp) + 1)
        assert lib.sgpr_fit_nll_grad_full(f._h, L.dptr(g), len(hyp) + 1) == L.E_STATE
        f.run()
        assert lib.sgpr_fit_nll_grad_full(f._h, L.dptr(g), len(hyp)) == L.E_ARG
        assert b"nll_grad_full" in lib.sgpr_last_error()
        assert lib.sgpr_fit_nll_grad_full(f._h, None, len(hyp) + 1) == L.E_ARG
    with SympFit("A", q, P, z[:N], hyp, s2, block="qq") as f:
        f.run()
        g = np.zeros(len(hyp) + 1)
        assert lib.sgpr_fit_nll_grad_full(f._h, L.dptr(g), len(hyp) + 1) == L.E_STATE


def test_large_pairs_fd():
    """n = 65 536 at d = 1 (the old path's two n x n scratch matrices would be 69 GB next to the factor)"""
    from sympgpr_amd.fit import SympFit
    N = 32768
    rng = np.random.default_rng(12)
    q, P, z = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N), rng.standard_normal(2 * N)
    hyp, s2 = _pair_hyp("A", 2 * N)
    _fd_check(lambda h, s: SympFit("A", q, P, z, h, s), hyp, s2, [0, 2, 3], "pairs A n=65536")
