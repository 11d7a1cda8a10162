"""GPU tests of the backward step of the d-pair symplectic map (csrc/map_nd.hip: applymap_nd_inverse_kernel;
sgpr_fit_applymap_nd_inverse, sgpr_applymap_nd_inverse_host; SympFit.applymap_pairs_inverse, maps.run_map_nd_inverse) on the data of
tests/test_gpu_applymap_nd.py: NT = 40, NTEST = 5, NM = 6, families A, C, D at d = 2, 3.

Reference: the backward recurrence on the CPU -- K* rows from the oracle's build_K_nd, MINPACK hybrd (scipy.optimize.fsolve,
xtol 1e-13) on q + G_P(q, P) - Q = 0 from q = Q, then p = P + G_q(q, P) --, run backwards from the end point of that file's CPU
forward orbit.  Tolerance: rtol = atol = 1e-8, the project's and the reference's map tolerance; a wrapped q is compared by its
distance on the circle, so that a value at 0 / 2 pi cannot fail.  The Newton counts are held against those of the NumPy
restatement tests/ref_inverse.py (which tests/test_applymap_inverse_cpu.py holds against central differences) plus 2, the margin
the forward test gives over its CPU count: the kernel's own stopping pass and rounding."""
import numpy as np
import pytest
import scipy.optimize

from tests import ref_inverse as RI
from tests.test_gpu_applymap_nd import CASES, NM, NT, NTEST, TWO_PI, _hyp, _ref_map_nd, _starts, _training

pytestmark = pytest.mark.gpu

TOL = 1e-8


@pytest.fixture(scope="module", autouse=True)
def _device():
    import sympgpr_amd
    if sympgpr_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need the MI355X")


def _ref_inverse_nd(oracle, fam, d, hyp, X, alpha, nm, Q0, P0, wrap_q):
    """the backward recurrence on the CPU; returns (qmap, pmap, max |G| met on the way)"""
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
            Q, P = qr[i, k], pr[i, k]
            f = lambda q: q + G(q, P)[d:] - Q
            qn, _, ier, msg = scipy.optimize.fsolve(f, Q, xtol=1e-13, full_output=True)
            if ier != 1:
                # hybrd's progress test can fire at the rounding floor of the residual although it stands on the root (ier = 5;
                # test_gpu_applymap_tangent.py: _cpu_step meets the same).  The point is taken only if a second run of the same
                # solver from it ends with ier = 1 without moving: the solver's own statement of convergence.
                q2, _, ier, msg = scipy.optimize.fsolve(f, qn, xtol=1e-13, full_output=True)
                assert ier == 1 and np.abs(q2 - qn).max() <= 1e-13 * max(1.0, np.abs(qn).max()), msg
                qn = q2
            pr[i + 1, k] = P + G(qn, P)[:d]
            qr[i + 1, k] = np.mod(qn, TWO_PI) if wrap_q else qn
    return qr, pr, gmax


def _case(oracle, fam, d, c=None):
    X, z = _training(d) if c is None else _training(d, c=c)
    hyp = _hyp(fam, d)
    alpha = oracle.fit_nd(fam, X, z, hyp, 1e-8)[0]
    Q0, P0 = _starts(d)
    return X, z, hyp, alpha, Q0, P0


@pytest.fixture(scope="module")
def refs(oracle):
    """per (family, d): training data, the oracle's alpha, the CPU forward orbit from the start points, the CPU backward orbit
    from its end point, and the restatement's Newton counts along it -- computed once, never changed"""
    out = {}
    for fam, d in CASES:
        X, z, hyp, alpha, Q0, P0 = _case(oracle, fam, d)
        wrap = fam != "C"
        qf, pf, _ = _ref_map_nd(oracle, fam, d, hyp, X, alpha, NM, Q0, P0, wrap)
        Qe, Pe = qf[-1].copy(), pf[-1].copy()
        qb, pb, _ = _ref_inverse_nd(oracle, fam, d, hyp, X, alpha, NM, Qe, Pe, wrap)
        assert np.isfinite(qb).all() and np.isfinite(pb).all()
        its = RI.backward_orbit(fam, d, hyp, X, alpha, NM, Qe, Pe, wrap)[2]
        for a in (X, z, hyp, alpha, Q0, P0, qf, pf, Qe, Pe, qb, pb, its):
            a.setflags(write=False)
        out[fam, d] = dict(X=X, z=z, hyp=hyp, alpha=alpha, Q0=Q0, P0=P0, wrap=wrap, qf=qf, pf=pf, Qe=Qe, Pe=Pe, q=qb, p=pb, its=its)
    return out


def _dist(q, qr, wrap):
    return RI.circle_distance(q, qr) if wrap else np.abs(q - qr)


def _compare(q, p, qr, pr, wrap, atol=TOL, what=""):
    """|x - ref| <= atol + 1e-8 |ref| for every entry (numpy.testing.assert_allclose's rule), q on the circle where it is wrapped"""
    assert q.shape == qr.shape and p.shape == pr.shape
    assert np.isfinite(q).all() and np.isfinite(p).all()
    dq, dp = _dist(q, qr, wrap), np.abs(p - pr)
    print("%smax |dq| = %.3e  max |dp| = %.3e" % (what, dq.max(), dp.max()))
    assert (dp <= atol + TOL * np.abs(pr)).all(), dp.max()
    assert (dq <= atol + TOL * np.abs(qr)).all(), dq.max()


@pytest.mark.parametrize("fam,d", CASES)
def test_parity_stateless_entry_with_the_oracles_alpha(refs, fam, d):
    from sympgpr_amd import maps
    r = refs[fam, d]
    q, p = maps.run_map_nd_inverse(fam, d, maps.WRAP_Q if r["wrap"] else 0, NM, r["hyp"], r["X"], r["alpha"], r["Qe"], r["Pe"])
    assert np.array_equal(q[0], r["Qe"]) and np.array_equal(p[0], r["Pe"])
    _compare(q, p, r["q"], r["p"], r["wrap"], what="%s d = %d stateless: " % (fam, d))
    # ... and the backward orbit is the forward orbit read from its end (the CPU's own, so this holds the reference too)
    _compare(q, p, r["qf"][::-1], r["pf"][::-1], r["wrap"], what="%s d = %d against the CPU forward orbit: " % (fam, d))


@pytest.mark.parametrize("fam,d", CASES)
def test_parity_handle_entry_and_newton_iterations(refs, fam, d):
    """SympFit.pairs(...).run().applymap_pairs_inverse(...) against the same CPU orbits; and the transposed Jacobian is really used:
    every solve takes at least 1 and at most (the restatement's largest count from q = Q) + 2 Newton iterations -- a wrong or
    missing Jacobian, the untransposed one among them, loses quadratic convergence."""
    from sympgpr_amd.fit import SympFit
    r = refs[fam, d]
    with SympFit.pairs(fam, r["X"], r["z"], r["hyp"], 1e-8) as f:
        q, p, it = f.run().applymap_pairs_inverse(NM, r["Qe"], r["Pe"], wrap_q=r["wrap"], return_iters=True)
    _compare(q, p, r["q"], r["p"], r["wrap"], what="%s d = %d handle: " % (fam, d))
    cpu = int(r["its"].max())
    print("Newton iterations: device min %d max %d, restatement min %d max %d" % (it.min(), it.max(), r["its"].min(), cpu))
    assert it.shape == (NM - 1, NTEST) and it.dtype == np.int32
    assert cpu <= 5                                          # what the restatement needs on this data (4 - 5)
    assert it.min() >= 1 and it.max() <= cpu + 2, it


@pytest.mark.parametrize("fam,d", CASES + [("B", 2)])
def test_round_trip_on_the_device(oracle, refs, fam, d):
    """NM - 1 steps forward by applymap_pairs, then NM - 1 backward by applymap_pairs_inverse from the last row: row i is forward
    row NM - 1 - i within 1e-8.  Family B: the separable (c = 0) data of test_explicit_mode_family_b, mode 0 -- the implicit map,
    which is the explicit one for a sum kernel -- and at most 2 Newton iterations, the first being exact."""
    from sympgpr_amd.fit import SympFit
    if fam == "B":
        X, z, hyp, alpha, Q0, P0 = _case(oracle, fam, d, c=0.0)
        wrap = False
    else:
        r = refs[fam, d]
        X, z, hyp, Q0, P0, wrap = r["X"], r["z"], r["hyp"], r["Q0"], r["P0"], r["wrap"]
    with SympFit.pairs(fam, X, z, hyp, 1e-8) as f:
        qf, pf = f.run().applymap_pairs(NM, Q0, P0, wrap_q=wrap)
        q, p, it = f.applymap_pairs_inverse(NM, qf[-1], pf[-1], wrap_q=wrap, return_iters=True)
    assert np.isfinite(qf).all() and np.isfinite(pf).all() and np.isfinite(q).all() and np.isfinite(p).all()
    dq, dp = _dist(q, qf[::-1], wrap), np.abs(p - pf[::-1])
    print("%s d = %d device round trip: max |dq| = %.3e  max |dp| = %.3e  iterations %d..%d" % (fam, d, dq.max(), dp.max(), it.min(), it.max()))
    assert dq.max() <= TOL and dp.max() <= TOL
    assert (it >= 1).all()
    if fam == "B":
        assert it.max() <= 2, it


def test_d1_pairs_fit_undoes_the_one_pair_map(oracle):
    """the D = 2 instance backwards from the end of the teamed d = 1 kernel's forward orbit (another kernel, a secant solve from
    the regular-GP guess): its rows come back within 1e-8.  Both get the fit's own alpha, as in the forward test."""
    from tests.test_gpu_examples import _training as training_d1
    from sympgpr_amd import maps
    from sympgpr_amd.fit import SympFit
    t = training_d1(oracle, "A")
    nm, Ntest = 6, 5
    rng = np.random.default_rng(5)
    Q0, P0 = rng.uniform(0.5, 5.5, Ntest), rng.uniform(-0.6, 0.6, Ntest)
    with SympFit.pairs("A", np.column_stack((t["q"], t["pn"])), t["ztrain"], t["hyp"], 1e-8) as f:
        alpha = f.run().alpha()
        qf, pf = maps.run_map_alpha(maps.WRAP_Q, nm, Ntest, t["hyp"], Q0, P0, t["q"], t["pn"], alpha, hypp=t["hypp"],
                                    xp=t["q"], yp=t["p_old"], alphap=t["alphap"], family="A")
        assert np.isfinite(qf).all() and np.isfinite(pf).all()
        q, p = f.applymap_pairs_inverse(nm, qf[-1], pf[-1], wrap_q=True)                # (Ntest,) start points: d = 1 only
        q2, p2 = f.applymap_pairs_inverse(nm, qf[-1][:, None], pf[-1][:, None], wrap_q=True)
    assert q.shape == (nm, Ntest, 1) and np.isfinite(q).all() and np.isfinite(p).all()
    dq, dp = RI.circle_distance(q[:, :, 0], qf[::-1]), np.abs(p[:, :, 0] - pf[::-1])
    print("d = 1 against the one-pair map: max |dq| = %.3e  max |dp| = %.3e" % (dq.max(), dp.max()))
    assert dq.max() <= TOL and dp.max() <= TOL
    assert q.tobytes() == q2.tobytes() and p.tobytes() == p2.tobytes()


@pytest.mark.parametrize("n0", [1, 63, 255, 257, 1025])
def test_kernel_edges(oracle, n0):
    """training-set sizes around the wave, the workgroup and the staging capacity of the D = 6 instance (1025 is the smallest
    size that runs the 512-thread instance from memory), the random X and alpha of the forward test_kernel_edges with its seeds.
    One backward step from the image of the forward test's start points under the CPU map, against the CPU backward step;
    atol scales with max |G|, as there."""
    from sympgpr_amd import maps
    d, Ntest, nm = 3, 3, 2
    rng = np.random.default_rng(100 + n0)
    X = np.hstack((rng.uniform(0, TWO_PI, (n0, d)), rng.uniform(-1, 1, (n0, d))))
    alpha = rng.standard_normal(2 * d * n0) * 0.1 / np.sqrt(n0)
    hyp = _hyp("A", d)
    Q0, P0 = _starts(d, Ntest)
    qf, pf, g1 = _ref_map_nd(oracle, "A", d, hyp, X, alpha, nm, Q0, P0, True)
    qr, pr, g2 = _ref_inverse_nd(oracle, "A", d, hyp, X, alpha, nm, qf[1], pf[1], True)
    assert np.isfinite(qr).all() and np.isfinite(pr).all()
    q, p, it = maps.run_map_nd_inverse("A", d, maps.WRAP_Q, nm, hyp, X, alpha, qf[1], pf[1], return_iters=True)
    atol = 1e-8 * max(1.0, g1, g2)
    _compare(q, p, qr, pr, True, atol=atol, what="n0 = %d  max |G| = %.3g  iterations %d..%d  " % (n0, max(g1, g2), it.min(), it.max()))
    _compare(q[1:], p[1:], Q0[None], P0[None], True, atol=atol, what="n0 = %d against the start of the CPU forward step: " % n0)
    assert (it >= 1).all()


def test_lost_orbits_and_bits(refs):
    """the kernel's own NaN path, with the inputs of the forward test_lost_orbits: a NaN start coordinate loses that orbit and no
    other; bits depend on nothing but the orbit's own start point"""
    from sympgpr_amd import maps
    r = refs["A", 2]
    args = ("A", 2, maps.WRAP_Q, NM, r["hyp"], r["X"], r["alpha"])
    q0, p0, i0 = maps.run_map_nd_inverse(*args, r["Qe"], r["Pe"], return_iters=True)
    assert np.isfinite(q0).all() and (i0 >= 1).all()
    Qe = r["Qe"].copy()
    Qe[1, 1] = np.nan                                   # one start value NaN: that orbit is NaN at every later step
    q, p, it = maps.run_map_nd_inverse(*args, Qe, r["Pe"], return_iters=True)
    assert np.isnan(q[1:, 1]).all() and np.isnan(p[1:, 1]).all() and (it[:, 1] == -1).all()
    keep = [0, 2, 3, 4]
    assert q[:, keep].tobytes() == q0[:, keep].tobytes() and p[:, keep].tobytes() == p0[:, keep].tobytes()
    assert it[:, keep].tobytes() == i0[:, keep].tobytes()
    Pe = r["Pe"].copy()
    Pe[3, 0] = np.inf                                   # ... and an infinite P
    q, p, it = maps.run_map_nd_inverse(*args, r["Qe"], Pe, return_iters=True)
    assert np.isnan(q[1:, 3]).all() and np.isnan(p[1:, 3]).all() and (it[:, 3] == -1).all()
    # a repeated call, another ntest, another index
    q2, p2, i2 = maps.run_map_nd_inverse(*args, r["Qe"], r["Pe"], return_iters=True)
    assert q2.tobytes() == q0.tobytes() and p2.tobytes() == p0.tobytes() and i2.tobytes() == i0.tobytes()
    q3, p3, i3 = maps.run_map_nd_inverse(*args, r["Qe"][3:4], r["Pe"][3:4], return_iters=True)
    assert q3[:, 0].tobytes() == q0[:, 3].tobytes() and p3[:, 0].tobytes() == p0[:, 3].tobytes()
    assert i3[:, 0].tobytes() == i0[:, 3].tobytes()
    # far outside the data G = 0: q = Q, p = P is the solution, found at once, and the orbit is not marked lost
    rc = refs["C", 2]
    Q0, P0 = rc["Q0"].copy(), rc["P0"].copy()
    P0[2] = 1e6
    q, p, it = maps.run_map_nd_inverse("C", 2, 0, NM, rc["hyp"], rc["X"], rc["alpha"], Q0, P0, return_iters=True)
    assert np.isfinite(q).all() and np.isfinite(p).all() and (it >= 1).all()
    assert (p[:, 2] == 1e6).all() and (q[:, 2] == Q0[2]).all()


def test_degenerate_calls(refs):
    from sympgpr_amd import maps
    r = refs["A", 2]
    q, p, it = maps.run_map_nd_inverse("A", 2, 0, 4, r["hyp"], r["X"], r["alpha"], np.zeros((0, 2)), np.zeros((0, 2)), return_iters=True)
    assert q.shape == (4, 0, 2) and p.shape == (4, 0, 2) and it.shape == (3, 0)
    q, p, it = maps.run_map_nd_inverse("A", 2, 0, 1, r["hyp"], r["X"], r["alpha"], r["Qe"], r["Pe"], return_iters=True)
    assert it.shape == (0, NTEST)
    assert np.array_equal(q[0], r["Qe"]) and np.array_equal(p[0], r["Pe"])


def test_state_errors(refs):
    """an unsolved fit, a reg=True fit and a block="qq" fit: SGPR_E_STATE (-5), the SympGPRError L.check raises for it"""
    from sympgpr_amd import SympGPRError
    from sympgpr_amd.fit import SympFit
    r = refs["A", 2]
    with SympFit.pairs("A", r["X"], r["z"], r["hyp"], 1e-8) as f:
        with pytest.raises(SympGPRError, match=r"\(-5\): fit_applymap_nd_inverse.*not solved"):
            f.applymap_pairs_inverse(3, r["Qe"], r["Pe"])
    x, y = r["X"][:, 0], r["X"][:, 2]
    with SympFit("A", x, y, r["z"][:NT], [1.2, 1.5, 1.0], 1e-2, reg=True) as f:
        with pytest.raises(SympGPRError, match=r"\(-5\).*scalar-kernel"):
            f.run().applymap_pairs_inverse(3, x[:3], y[:3])
    with SympFit("A", x, y, r["z"][:NT], [1.2, 1.5, 1.0], 1e-2, block="qq") as f:
        with pytest.raises(SympGPRError, match=r"\(-5\).*single-block"):
            f.run().applymap_pairs_inverse(3, x[:3], y[:3])


def test_the_handle_is_unchanged_by_the_call(refs):
    from sympgpr_amd.fit import SympFit
    r = refs["C", 3]
    with SympFit.pairs("C", r["X"], r["z"], r["hyp"], 1e-8) as f:
        f.run()
        a0, n0 = f.alpha(), f.nll()
        qf0, pf0, if0 = f.applymap_pairs(NM, r["Q0"], r["P0"], return_iters=True)
        q1, p1 = f.applymap_pairs_inverse(NM, r["Qe"], r["Pe"])
        a1, n1 = f.alpha(), f.nll()
        qf1, pf1, if1 = f.applymap_pairs(NM, r["Q0"], r["P0"], return_iters=True)
        q2, p2 = f.applymap_pairs_inverse(NM, r["Qe"], r["Pe"])
    assert a0.tobytes() == a1.tobytes() and np.float64(n0).tobytes() == np.float64(n1).tobytes()
    assert qf0.tobytes() == qf1.tobytes() and pf0.tobytes() == pf1.tobytes() and if0.tobytes() == if1.tobytes()
    assert q1.tobytes() == q2.tobytes() and p1.tobytes() == p2.tobytes()


def test_the_forward_map_did_not_move(refs):
    """maps.run_map_nd and run_map_nd_tangent on the A, d = 3 data: the same bits before and after a backward call"""
    from sympgpr_amd import maps
    r = refs["A", 3]
    args = ("A", 3, maps.WRAP_Q, NM, r["hyp"], r["X"], r["alpha"], r["Q0"], r["P0"])
    q0, p0, i0 = maps.run_map_nd(*args, return_iters=True)
    t0 = maps.run_map_nd_tangent(*args)
    qb, pb = maps.run_map_nd_inverse("A", 3, maps.WRAP_Q, NM, r["hyp"], r["X"], r["alpha"], q0[-1], p0[-1])
    assert np.isfinite(qb).all() and np.isfinite(pb).all()
    q1, p1, i1 = maps.run_map_nd(*args, return_iters=True)
    t1 = maps.run_map_nd_tangent(*args)
    assert q0.tobytes() == q1.tobytes() and p0.tobytes() == p1.tobytes() and i0.tobytes() == i1.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(t0[:3], t1[:3]))
    assert sorted(t0[3]) == sorted(t1[3]) == ["jac", "lyap", "mono"]
    assert all(t0[3][k].tobytes() == t1[3][k].tobytes() for k in t0[3])
    assert t0[0].tobytes() == q0.tobytes() and t0[1].tobytes() == p0.tobytes()
