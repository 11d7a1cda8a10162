"""Every public entry point that evaluates a kernel formula, against tests/golden/range.npz: 50-digit values from a sympy
differentiation of the four one-line kernel definitions (make_range_golden.py), over lengths 1e-2 .. 1e2 (times 1.37),
sig 1e-2 .. 1e2, coincident points, both zeros of the Hessian entries, |dx| ~ pi, exponents in the denormal band and below
the exp clamp.  The bound is ref_range.py's: |got - v| <= C eps T + F with C = 4 * C_REF, C_REF measured on the fp64 oracle
by test_range_cpu.py.  mpmath is not evaluated here.  WORST collects the worst device ratio per (site, family)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_range as R  # noqa: E402

pytestmark = pytest.mark.gpu

G = R.load()
PAIR_CASES = [str(k) for k in G["pair_cases"]]
ND_CASES = [str(k) for k in G["nd_cases"]]
FIT_CASES = [str(k) for k in G["fit_cases"]]
WHICH = {"k": 0, "kxx": 1, "kyy": 2, "kxy": 3}
WORST = {}
_MODEL = {}


def model(key):
    if key not in _MODEL:
        c = R.case(G, key)
        _MODEL[key] = (c, R.pair_model(key[0], c["x"], c["y"], c["x0"], c["y0"], c["hyp"]))
    return _MODEL[key]


def hold(site, fam, got, v, m, what, extra=None):
    """got against v under the site's bound; prints the figure before it asserts"""
    S, T, F, Z = m
    if extra is not None:
        F = F + extra
    r, _, _ = R.ratio(got, v, S, T, F, Z)
    WORST[(site, fam)] = max(WORST.get((site, fam), 0.0), r)
    print("%-26s %-8s %s ratio %.3f (bound %.1f)" % (what, site, fam, r, R.C[site]))
    assert r <= R.C[site], (what, site, fam, r)


def hold_gram(fam, K, c, m, what, sfx=""):
    n, n0 = c["kxx"].shape
    for e, blk in (("kxx", K[:n, :n0]), ("kxy", K[n:, :n0]), ("kxy", K[:n, n0:]), ("kyy", K[n:, n0:])):
        hold(e + sfx, fam, blk, c[e + sfx], m[e + sfx], what)


def hold_dgram(fam, D, c, m, what, sfx):
    n, n0 = c["kxx"].shape
    for e, blk in (("kxx", D[:n0, :n]), ("kxy", D[n0:, :n]), ("kxy", D[:n0, n:]), ("kyy", D[n0:, n:])):
        hold(e + sfx, fam, blk.T, c[e + sfx], m[e + sfx], what)


@pytest.fixture(scope="module")
def ops():
    from sympgpr_amd import _lib as L
    from sympgpr_amd import ops
    lib = L.load_library()
    if lib.sgpr_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need the MI355X")
    return ops


def gram_pairs_ocml(fam, x, y, x0, y0, hyp):
    """the device-libs instance of pair_eval: sgpr_gram_pairs_dev with SGPR_G_OCML"""
    import torch
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    n, n0 = len(x), len(x0)
    dev = [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to("cuda") for v in (x, y, x0, y0)]
    out = [torch.full((n0, n), float("nan"), dtype=torch.float64, device="cuda") for _ in range(4)]   # column-major n x n0
    h = np.ascontiguousarray(hyp, dtype=np.float64)
    torch.cuda.synchronize()
    rc = lib.sgpr_gram_pairs_dev(L.family_id(fam), n, n0, *[C.c_void_p(t.data_ptr()) for t in dev], L.dptr(h), len(h),
                                 *[C.c_void_p(t.data_ptr()) for t in out], n, 0, 0.0, L.G_ALL | L.G_OCML, None)
    assert rc == 0, lib.sgpr_last_error()
    torch.cuda.synchronize()
    qq, Pq, qP, PP = (t.cpu().numpy().T for t in out)
    return np.block([[qq, qP], [Pq, PP]])


@pytest.mark.parametrize("key", PAIR_CASES)
def test_build_k(ops, key):
    """pair_eval (both math instances) and kern_eval through build_k, sgpr_gram_pairs_dev and buildkreg"""
    fam = key[0]
    c, m = model(key)
    n, n0 = len(c["x"]), len(c["x0"])
    K = np.full((2 * n, 2 * n0), np.nan, order="F")
    ops.build_k(c["x"], c["y"], c["x0"], c["y0"], c["hyp"], K, family=fam)
    hold_gram(fam, K, c, m, "build_k " + key)
    hold_gram(fam, gram_pairs_ocml(fam, c["x"], c["y"], c["x0"], c["y0"], c["hyp"]), c, m, "gram_pairs OCML " + key)
    Kr = np.full((n, n0), np.nan, order="F")
    ops.buildkreg(c["x"], c["y"], c["x0"], c["y0"], c["hyp"], Kr, family=fam)
    hold("k", fam, Kr, c["k"], m["k"], "buildkreg " + key)


@pytest.mark.parametrize("key", PAIR_CASES)
def test_kernel_eval(ops, key):
    """the four scalar functions; they return the entry without sig, the product adds one rounding (eps |v|)"""
    fam = key[0]
    c, m = model(key)
    xa, xb = np.broadcast_arrays(c["x0"][None, :], c["x"][:, None])
    ya, yb = np.broadcast_arrays(c["y0"][None, :], c["y"][:, None])
    for site, w in WHICH.items():
        got = c["hyp"][-1] * ops.kernel_eval(w, xa, ya, xb, yb, c["hyp"][:-1], family=fam)
        hold(site, fam, got, c[site], m[site], "kernel_eval %d %s" % (w, key), extra=R.EPS * np.abs(got))


@pytest.mark.parametrize("key", PAIR_CASES)
def test_build_dk(ops, key):
    """pair_eval_d, kern_eval_d and the generated pair_dlx / pair_dly through build_dk and build_dkreg"""
    fam = key[0]
    c, m = model(key)
    dK = ops.build_dk(c["x"], c["y"], c["x0"], c["y0"], c["hyp"], family=fam)
    dKr = ops.build_dkreg(c["x"], c["y"], c["x0"], c["y0"], c["hyp"], family=fam)
    for w, sfx in enumerate(("_dlx", "_dly")):
        hold_dgram(fam, dK[w], c, m, "build_dk " + key, sfx)
        hold("k" + sfx, fam, dKr[w], c["k" + sfx], m["k" + sfx], "build_dkreg " + key)


@pytest.mark.parametrize("key", ND_CASES)
def test_build_k_nd(ops, key):
    """coord and weights of gram_nd.hip, d = 2, 3"""
    fam, d = key[3], int(key[4])
    c = R.case(G, key)
    S, T, F, Z, diag = R.nd_model(fam, d, c["X"], c["X0"], c["hyp"])
    K = ops.build_k_nd(c["X"], c["X0"], c["hyp"], family=fam)
    for site, sel in (("nd_diag", diag), ("nd_off", ~diag)):
        hold(site, fam, K[sel], c["K"][sel], (S[sel], T[sel], F[sel], Z[sel]), "build_k_nd " + key)


@pytest.mark.parametrize("key", PAIR_CASES)
def test_build_k_nd_one_pair(ops, key):
    """the d = 1 instance against the build_k values: it forms x_col - x_row, build_k the opposite order"""
    fam = key[0]
    c, m = model(key)
    hold_gram(fam, ops.build_k_nd(np.column_stack((c["x"], c["y"])), np.column_stack((c["x0"], c["y0"])), c["hyp"], family=fam),
              c, m, "build_k_nd d=1 " + key)


@pytest.mark.parametrize("key", [k for k in FIT_CASES if k[5] == "1"])
def test_fit_batch_nll(ops, key):
    """pair_eval inside batch.hip (order 16, reg: 8): nll against the mpmath Cholesky of the same 8-point problem,
    relative tolerance 64 cond eps"""
    from sympgpr_amd.fit import SympFit, fit_batch
    fam, reg = key[4], key[6] == "r"
    c = R.case(G, key)
    x, y = c["X"][:, 0], c["X"][:, 1]
    _, nll, info = fit_batch(fam, x[None], y[None], c["z"][None], c["hyp"][None], float(c["sig2n"]), reg=reg, want_alpha=False)
    assert info[0] == 0
    with SympFit(fam, x, y, c["z"], c["hyp"], float(c["sig2n"]), reg=reg) as f:
        nll1 = f.run().nll()
    tol = 64.0 * float(c["cond"]) * R.EPS * abs(float(c["nll"]))
    for what, v in (("fit_batch", nll[0]), ("SympFit", nll1)):
        print("%s %s nll %.17g exact %.17g  err/tol %.3g  cond %.3g" % (what, key, v, float(c["nll"]),
                                                                        abs(v - float(c["nll"])) / tol, float(c["cond"])))
        assert abs(v - float(c["nll"])) <= tol


GRAD_CASES = [k for k in FIT_CASES if k[4] != "B"]


@pytest.mark.parametrize("key", GRAD_CASES)
def test_nll_gradient(ops, key):
    """pair_grad / reg_grad through SympFit.nll_grad_full and fit_batch_grad: every entry (lengths, periods, sig, sig2n)
    against 1/2 tr(W dK) from mpmath, |g - g_exact| <= C_G eps cond sum |W_ij| |dK_ij|"""
    from sympgpr_amd.fit import SympFit, fit_batch_grad
    fam, d, reg = key[4], int(key[5]), key[6] == "r"
    c = R.case(G, key)
    s2 = float(c["sig2n"])
    got = {}
    if d == 1:
        x, y = c["X"][:, 0], c["X"][:, 1]
        with SympFit(fam, x, y, c["z"], c["hyp"], s2, reg=reg) as f:
            got["nll_grad_full"] = f.run().nll_grad_full()
        _, _, grad, info = fit_batch_grad(fam, x[None], y[None], c["z"][None], c["hyp"][None], s2, reg=reg)
        assert info[0] == 0
        got["fit_batch_grad"] = grad[0]
    else:
        with SympFit.pairs(fam, c["X"], c["z"], c["hyp"], s2) as f:
            got["nll_grad_full"] = f.run().nll_grad_full()
    bound = R.EPS * float(c["cond"]) * c["absum"]
    for what, g in got.items():
        assert g.shape == c["grad"].shape
        r = float((np.abs(g - c["grad"]) / bound).max())
        WORST[("grad " + what, key[4:])] = r
        print("%-15s %-12s ratio %.4g (bound %.3g)" % (what, key, r, R.C_G))
        assert r <= R.C_G, (what, key, r)


def _uniform(fam):
    c = R.case(G, fam + "2")
    return c["x0"], c["y0"], c["x"][7:], c["y"][7:]


@pytest.mark.parametrize("fam", "ABCD")
def test_low_bound_of_the_scalar_optimiser(ops, fam):
    """l = 1e-10, the low bound of the scalar-kernel GP's search: off the diagonal exactly 0.0, the diagonal 1 (2 for the sum
    kernel), every derivative finite"""
    x0, y0, _, _ = _uniform(fam)
    hyp = [1e-10, 1e-10, 0.75, 1.0] if fam == "D" else [1e-10, 1e-10, 1.0]
    n = len(x0)
    K = np.full((n, n), np.nan, order="F")
    ops.buildkreg(x0, y0, x0, y0, hyp, K, family=fam)
    off = ~np.eye(n, dtype=bool)
    assert np.all(K[off] == 0.0)
    assert np.all(np.diag(K) == (2.0 if fam == "B" else 1.0))
    for D in ops.build_dkreg(x0, y0, x0, y0, hyp, family=fam):
        assert np.all(np.isfinite(D))


@pytest.mark.parametrize("l", [1e-2, 1e2])
@pytest.mark.parametrize("fam", "ABCD")
def test_ends_of_the_range_are_finite(ops, fam, l):
    x0, y0, x, y = _uniform(fam)
    hyp = [l, l, 0.75, 1.0] if fam == "D" else [l, l, 1.0]
    K = np.full((2 * len(x), 2 * len(x0)), np.nan, order="F")
    ops.build_k(x, y, x0, y0, hyp, K, family=fam)
    assert np.all(np.isfinite(K))
    for D in ops.build_dk(x, y, x0, y0, hyp, family=fam):
        assert np.all(np.isfinite(D))


@pytest.mark.parametrize("fam", "ABCD")
def test_negative_lx(ops, fam):
    """an unbounded L-BFGS-B step makes lx < 0: K is even in lx bit for bit, dK/dlx is the exact negative, dK/dly unchanged"""
    c = R.case(G, fam + "7")
    hyp = c["hyp"].copy()
    neg = hyp.copy()
    neg[0] = -neg[0]
    shape = (2 * len(c["x"]), 2 * len(c["x0"]))
    Kp, Kn = np.full(shape, np.nan, order="F"), np.full(shape, np.nan, order="F")
    ops.build_k(c["x"], c["y"], c["x0"], c["y0"], hyp, Kp, family=fam)
    ops.build_k(c["x"], c["y"], c["x0"], c["y0"], neg, Kn, family=fam)
    assert np.all(np.isfinite(Kp)) and np.array_equal(Kp.view(np.uint64), Kn.view(np.uint64))
    Dp = ops.build_dk(c["x"], c["y"], c["x0"], c["y0"], hyp, family=fam)
    Dn = ops.build_dk(c["x"], c["y"], c["x0"], c["y0"], neg, family=fam)
    assert np.all(np.isfinite(Dp[0])) and np.array_equal(Dn[0], -Dp[0])
    assert np.array_equal(Dn[1], Dp[1])


@pytest.mark.parametrize("fam", "ABD")
def test_cos2h_switch_is_seamless(ops, fam):
    """cos 2h is 1 - 2 sin^2 h while lx^2 <= 1 and has its own reduction above (devmath.h): at lx = 1 and at the next fp64
    above it, with a row point at the zero of kxx, the two forms agree within twice the kxx bound (plus the step in lx
    itself, 2^-52 |d kxx / d lx|), through build_k, the device-libs instance and the d = 1 instance of build_k_nd"""
    c = R.case(G, fam + "2")
    hs = c["hyp"][2] if fam == "D" else 0.5
    lo, hi = 0.0, np.pi / 4                                  # the root of cos 2h = (sin h cos h)^2 (lx = 1), by bisection
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if np.cos(2 * mid) - (np.sin(mid) * np.cos(mid)) ** 2 > 0 else (lo, mid)
    x, y, x0, y0 = c["x"].copy(), c["y"].copy(), c["x0"], c["y0"]
    x[1] = x0[1] + np.round(lo / hs * 2.0 ** 24) * 2.0 ** -24
    n, n0 = len(x), len(x0)
    hyps = []
    for lx in (1.0, np.nextafter(1.0, 2.0)):
        h = c["hyp"].copy()
        h[0] = lx
        hyps.append(h)
    m = R.pair_model(fam, x, y, x0, y0, hyps[0])
    bound = 2.0 * R.C["kxx"] * R.EPS * m["kxx"][1] + 2.0 * R.EPS * m["kxx_dlx"][1] + 2.0 * m["kxx"][2]
    assert abs(m["kxx"][0][1, 1]) > 0

    def three(h):
        K = np.full((2 * n, 2 * n0), np.nan, order="F")
        ops.build_k(x, y, x0, y0, h, K, family=fam)
        return [K[:n, :n0], gram_pairs_ocml(fam, x, y, x0, y0, h)[:n, :n0],
                ops.build_k_nd(np.column_stack((x, y)), np.column_stack((x0, y0)), h, family=fam)[:n, :n0]]

    for what, a, b in zip(("build_k", "OCML", "build_k_nd"), three(hyps[0]), three(hyps[1])):
        r = float((np.abs(a - b) / bound).max())
        print("%s %s: worst |kxx(1) - kxx(1+)| / bound %.3f" % (what, fam, r))
        assert np.all(np.isfinite(a)) and r <= 1.0
