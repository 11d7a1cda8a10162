"""GPU tests of the d-pair symplectic map (csrc/map_nd.hip: applymap_nd_kernel; sgpr_fit_applymap_nd, sgpr_applymap_nd_host;
SympFit.applymap_pairs, maps.run_map_nd) against the implicit equation solved on the CPU: K* rows from the oracle's build_K_nd,
MINPACK hybrd (scipy.optimize.fsolve, xtol 1e-13) from P = p -- the solver and tolerance of _ref_map in test_gpu_examples.py --,
then the Q update.  Tolerance: rtol = atol = 1e-8, the reference's own map tolerance (test_sympgpr.py:92-93).  Every output is
finite on this data and every entry is compared."""
import numpy as np
import pytest
import scipy.optimize

pytestmark = pytest.mark.gpu

TWO_PI = 2.0 * np.pi
TOL = dict(rtol=1e-8, atol=1e-8)
NT, NTEST, NM = 40, 5, 6
CASES = [(fam, d) for fam in "ACD" for d in (2, 3)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    import sympgpr_amd
    if sympgpr_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need the MI355X")


def _hyp(fam, d):
    return np.array((1.2,) * d + (1.5,) * d + ((0.5,) * d if fam == "D" else ()) + (1.0,))


def _training(d, Nt=NT, eps=0.25, c=0.4):
    """F = eps sum cos q_i + eps/2 sum P_i^2 + c eps cos(sum q_i) (1 + 1/2 sum P_i^2);  z = (dF/dq blocks, dF/dP blocks)"""
    rng = np.random.default_rng(11)
    q, P = rng.uniform(0, TWO_PI, (Nt, d)), rng.uniform(-1, 1, (Nt, d))
    s, h = q.sum(axis=1), 1.0 + 0.5 * (P * P).sum(axis=1)
    Fq = -eps * np.sin(q) - (c * eps * np.sin(s) * h)[:, None]
    FP = eps * P + (c * eps * np.cos(s))[:, None] * P
    return np.hstack((q, P)), np.concatenate((Fq.T.ravel(), FP.T.ravel()))


def _starts(d, Ntest=NTEST):
    rng = np.random.default_rng(5)
    return rng.uniform(0.5, 5.5, (Ntest, d)), rng.uniform(-0.6, 0.6, (Ntest, d))


def _ref_map_nd(oracle, fam, d, hyp, X, alpha, nm, Q0, P0, wrap_q, explicit=False):
    """the recurrence on the CPU; returns (qmap, pmap, max |G| met on the way)"""
    Ntest = Q0.shape[0]
    qr, pr = np.zeros((nm, Ntest, d)), np.zeros((nm, Ntest, d))
    qr[0], pr[0] = Q0, P0
    gmax = 0.0

    def G(q, P):
        nonlocal gmax
        g = oracle.build_K_nd(fam, np.concatenate((q, P))[None, :], X, hyp) @ alpha
        gmax = max(gmax, float(np.abs(g).max()))
        return g

    for i in range(nm - 1):
        for k in range(Ntest):
            q, p = qr[i, k], pr[i, k]
            if explicit:
                Pn = p - G(q, p)[:d]
            else:
                Pn, _, ier, msg = scipy.optimize.fsolve(lambda P: G(q, P)[:d] - p + P, p, xtol=1e-13, full_output=True)
                assert ier == 1, msg
            Qn = q + G(q, Pn)[d:]
            pr[i + 1, k] = Pn
            qr[i + 1, k] = np.mod(Qn, TWO_PI) if wrap_q else Qn
    return qr, pr, gmax


@pytest.fixture(scope="module")
def refs(oracle):
    """per (family, d): training data, the oracle's alpha, the start points and the CPU orbits -- computed once, never changed"""
    out = {}
    for fam, d in CASES:
        X, z = _training(d)
        hyp = _hyp(fam, d)
        alpha = oracle.fit_nd(fam, X, z, hyp, 1e-8)[0]
        Q0, P0 = _starts(d)
        wrap = fam != "C"
        qr, pr, _ = _ref_map_nd(oracle, fam, d, hyp, X, alpha, NM, Q0, P0, wrap)
        assert np.isfinite(qr).all() and np.isfinite(pr).all()
        for a in (X, z, hyp, alpha, Q0, P0, qr, pr):
            a.setflags(write=False)
        out[fam, d] = dict(X=X, z=z, hyp=hyp, alpha=alpha, Q0=Q0, P0=P0, wrap=wrap, q=qr, p=pr)
    return out


def _compare(q, p, r):
    assert q.shape == r["q"].shape and p.shape == r["p"].shape
    assert np.isfinite(q).all() and np.isfinite(p).all()
    print("max |dq| = %.3e  max |dp| = %.3e" % (np.abs(q - r["q"]).max(), np.abs(p - r["p"]).max()))
    np.testing.assert_allclose(p, r["p"], **TOL)
    np.testing.assert_allclose(q, r["q"], **TOL)


@pytest.mark.parametrize("fam,d", CASES)
def test_parity_stateless_entry_with_the_oracles_alpha(refs, fam, d):
    from sympgpr_amd import maps
    r = refs[fam, d]
    q, p = maps.run_map_nd(fam, d, maps.WRAP_Q if r["wrap"] else 0, NM, r["hyp"], r["X"], r["alpha"], r["Q0"], r["P0"])
    _compare(q, p, r)


@pytest.mark.parametrize("fam,d", CASES)
def test_parity_handle_entry_and_newton_iterations(refs, fam, d):
    """SympFit.pairs(...).run().applymap_pairs(...) against the same CPU orbits; and the Jacobian is really used: every solve
    takes between 1 and 6 Newton iterations (the CPU needs 4 from P = p with a central-difference Jacobian; the margin of 2
    covers the kernel's own stopping pass and rounding -- a wrong or missing Jacobian loses quadratic convergence)."""
    from sympgpr_amd.fit import SympFit
    r = refs[fam, d]
    with SympFit.pairs(fam, r["X"], r["z"], r["hyp"], 1e-8) as f:
        q, p, it = f.run().applymap_pairs(NM, r["Q0"], r["P0"], wrap_q=r["wrap"], return_iters=True)
    _compare(q, p, r)
    print("Newton iterations: min %d max %d" % (it.min(), it.max()))
    assert it.shape == (NM - 1, NTEST) and it.dtype == np.int32
    assert it.min() >= 1 and it.max() <= 6, it


def test_d1_pairs_fit_against_the_one_pair_map(oracle):
    """the D = 2 instance against the existing d = 1 kernel (secant from the regular-GP guess): another solver and start point,
    the same root.  Both maps get the fit's own alpha: Ky of this data has cond 1e9, and the inverse-based alpha of the
    `_training` helper differs from a Cholesky solve by 9e-5 relative, which is no property of either map."""
    from tests.test_gpu_examples import _training as training_d1
    from sympgpr_amd import maps
    from sympgpr_amd.fit import SympFit
    t = training_d1(oracle, "A")
    nm, Ntest = 6, 5
    rng = np.random.default_rng(5)
    Q0, P0 = rng.uniform(0.5, 5.5, Ntest), rng.uniform(-0.6, 0.6, Ntest)
    with SympFit.pairs("A", np.column_stack((t["q"], t["pn"])), t["ztrain"], t["hyp"], 1e-8) as f:
        alpha = f.run().alpha()
        q, p = f.applymap_pairs(nm, Q0, P0, wrap_q=True)                # (Ntest,) start points: d = 1 only
        q2, p2 = f.applymap_pairs(nm, Q0[:, None], P0[:, None], wrap_q=True)
    qr, pr = maps.run_map_alpha(maps.WRAP_Q, nm, Ntest, t["hyp"], Q0, P0, t["q"], t["pn"], alpha, hypp=t["hypp"],
                                xp=t["q"], yp=t["p_old"], alphap=t["alphap"], family="A")
    assert np.isfinite(qr).all() and np.isfinite(pr).all()
    assert q.shape == (nm, Ntest, 1) and np.isfinite(q).all() and np.isfinite(p).all()
    print("max |dq| = %.3e  max |dp| = %.3e" % (np.abs(q[:, :, 0] - qr).max(), np.abs(p[:, :, 0] - pr).max()))
    np.testing.assert_allclose(p[:, :, 0], pr, **TOL)
    np.testing.assert_allclose(q[:, :, 0], qr, **TOL)
    assert q.tobytes() == q2.tobytes() and p.tobytes() == p2.tobytes()


def test_explicit_mode_family_b(oracle):
    """P = p - G_q(q, p), Q = q + G_P(q, P) with the sum kernel, no solve: iters all 0.  Training data: the SEPARABLE part of the
    generating function (c = 0), which is what a sum kernel k = sum_m f_m can represent.  With the coupling term the fit at
    sig2n = 1e-8 answers with |alpha| = 1.6e7, and eps * sum_j |K*_j alpha_j| = 8.7e-9 per evaluation of G: the rounding of the
    sums alone then exceeds 1e-8 after a few steps, in any arithmetic (measured on the device with that data: max |dq| 8.0e-8,
    max |dp| 7.9e-9).  With c = 0: |alpha| = 1.3e3 and 1.7e-12 per evaluation."""
    from sympgpr_amd import maps
    d = 2
    X, z = _training(d, c=0.0)
    hyp = _hyp("B", d)
    alpha = oracle.fit_nd("B", X, z, hyp, 1e-8)[0]
    Q0, P0 = _starts(d)
    qr, pr, _ = _ref_map_nd(oracle, "B", d, hyp, X, alpha, NM, Q0, P0, True, explicit=True)
    assert np.isfinite(qr).all() and np.isfinite(pr).all()
    q, p, it = maps.run_map_nd("B", d, maps.WRAP_Q | maps.EXPLICIT, NM, hyp, X, alpha, Q0, P0, return_iters=True)
    _compare(q, p, dict(q=qr, p=pr))
    assert (it == 0).all()


def test_bits_do_not_depend_on_the_call_or_the_batch(refs):
    from sympgpr_amd import maps
    r = refs["A", 3]
    args = ("A", 3, maps.WRAP_Q, NM, r["hyp"], r["X"], r["alpha"])
    q1, p1, i1 = maps.run_map_nd(*args, r["Q0"], r["P0"], return_iters=True)
    q2, p2, i2 = maps.run_map_nd(*args, r["Q0"], r["P0"], return_iters=True)
    assert q1.tobytes() == q2.tobytes() and p1.tobytes() == p2.tobytes() and i1.tobytes() == i2.tobytes()
    q3, p3, i3 = maps.run_map_nd(*args, r["Q0"][3:4], r["P0"][3:4], return_iters=True)
    assert q3[:, 0].tobytes() == q1[:, 3].tobytes() and p3[:, 0].tobytes() == p1[:, 3].tobytes()
    assert i3[:, 0].tobytes() == i1[:, 3].tobytes()


def test_lost_orbits(refs):
    from sympgpr_amd import maps
    r = refs["A", 2]
    args = ("A", 2, maps.WRAP_Q, NM, r["hyp"], r["X"], r["alpha"])
    q0, p0, i0 = maps.run_map_nd(*args, r["Q0"], r["P0"], return_iters=True)
    Q0 = r["Q0"].copy()
    Q0[1, 1] = np.nan                                   # one start value NaN: that orbit is NaN at every later step
    q, p, it = maps.run_map_nd(*args, Q0, r["P0"], return_iters=True)
    assert np.isnan(q[1:, 1]).all() and np.isnan(p[1:, 1]).all() and (it[:, 1] == -1).all()
    keep = [0, 2, 3, 4]
    assert q[:, keep].tobytes() == q0[:, keep].tobytes() and p[:, keep].tobytes() == p0[:, keep].tobytes()
    assert it[:, keep].tobytes() == i0[:, keep].tobytes()
    # far outside the data G = 0: P = p, Q = q is the solution, found at once, and the orbit is not marked lost
    rc = refs["C", 2]
    Q0, P0 = rc["Q0"].copy(), rc["P0"].copy()
    P0[2] = 1e6
    q, p, it = maps.run_map_nd("C", 2, 0, NM, rc["hyp"], rc["X"], rc["alpha"], Q0, P0, return_iters=True)
    assert np.isfinite(q).all() and np.isfinite(p).all() and (it >= 1).all()
    assert (p[:, 2] == 1e6).all() and (q[:, 2] == Q0[2]).all()


@pytest.mark.parametrize("n0", [1, 63, 255, 257, 1025])
def test_kernel_edges(oracle, n0):
    """training-set sizes around the wave, the workgroup and the staging capacity of the D = 6 instance (csrc/map_nd.hip,
    MAPND_STAGE_PTS = 1024 points in LDS; 1025 runs the 512-thread instance from memory), random X and alpha through the
    stateless entry.
    atol scales with max |G|: the sums are larger than on the fitted data."""
    from sympgpr_amd import maps
    d, Ntest, nm = 3, 3, 2
    rng = np.random.default_rng(100 + n0)
    X = np.hstack((rng.uniform(0, TWO_PI, (n0, d)), rng.uniform(-1, 1, (n0, d))))
    alpha = rng.standard_normal(2 * d * n0) * 0.1 / np.sqrt(n0)
    hyp = _hyp("A", d)
    Q0, P0 = _starts(d, Ntest)
    qr, pr, gmax = _ref_map_nd(oracle, "A", d, hyp, X, alpha, nm, Q0, P0, True)
    assert np.isfinite(qr).all() and np.isfinite(pr).all()
    q, p = maps.run_map_nd("A", d, maps.WRAP_Q, nm, hyp, X, alpha, Q0, P0)
    assert np.isfinite(q).all() and np.isfinite(p).all()
    atol = 1e-8 * max(1.0, gmax)
    print("n0 = %d  max |G| = %.3g  max |dq| = %.3e  max |dp| = %.3e" % (n0, gmax, np.abs(q - qr).max(), np.abs(p - pr).max()))
    np.testing.assert_allclose(p, pr, rtol=1e-8, atol=atol)
    np.testing.assert_allclose(q, qr, rtol=1e-8, atol=atol)


def test_degenerate_calls(refs):
    from sympgpr_amd import maps
    r = refs["A", 2]
    q, p, it = maps.run_map_nd("A", 2, 0, 4, r["hyp"], r["X"], r["alpha"], np.zeros((0, 2)), np.zeros((0, 2)), return_iters=True)
    assert q.shape == (4, 0, 2) and p.shape == (4, 0, 2) and it.shape == (3, 0)
    q, p, it = maps.run_map_nd("A", 2, 0, 1, r["hyp"], r["X"], r["alpha"], r["Q0"], r["P0"], return_iters=True)
    assert it.shape == (0, NTEST)
    assert np.array_equal(q[0], r["Q0"]) and np.array_equal(p[0], r["P0"])


def test_state_errors(refs):
    """an unsolved fit, a reg=True fit and a block="qq" fit: SGPR_E_STATE (-5), the SympGPRError L.check raises for it"""
    from sympgpr_amd import SympGPRError
    from sympgpr_amd.fit import SympFit
    r = refs["A", 2]
    with SympFit.pairs("A", r["X"], r["z"], r["hyp"], 1e-8) as f:
        with pytest.raises(SympGPRError, match=r"\(-5\).*not solved"):
            f.applymap_pairs(3, r["Q0"], r["P0"])
    x, y = r["X"][:, 0], r["X"][:, 2]
    with SympFit("A", x, y, r["z"][:NT], [1.2, 1.5, 1.0], 1e-2, reg=True) as f:
        with pytest.raises(SympGPRError, match=r"\(-5\).*scalar-kernel"):
            f.run().applymap_pairs(3, x[:3], y[:3])
    with SympFit("A", x, y, r["z"][:NT], [1.2, 1.5, 1.0], 1e-2, block="qq") as f:
        with pytest.raises(SympGPRError, match=r"\(-5\).*single-block"):
            f.run().applymap_pairs(3, x[:3], y[:3])
