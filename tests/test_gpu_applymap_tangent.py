"""GPU tests of the tangent map of the d-pair symplectic map (csrc/maptan.h, the TAN instances of applymap_nd_kernel;
sgpr_fit_applymap_nd_tangent, sgpr_applymap_nd_tangent_host; SympFit.applymap_pairs_tangent, maps.run_map_nd_tangent) on the
data of tests/test_gpu_applymap_nd.py: NT = 40, NTEST = 5, NM = 6, families A, C, D at d = 2, 3.

References: central differences (h = 1e-5) of that file's own CPU map (_ref_map_nd: MINPACK hybrd, xtol 1e-13), one step at a
time from the reference orbit's points; and tests/ref_tangent.py, the NumPy restatement of the formulas, which
tests/test_applymap_tangent_cpu.py holds against sympy.  Every entry of every step is compared.

Tolerances, none taken from the device:
  * against central differences: rtol = atol = 1e-6 -- the quotient carries at most 1e-13 / 1e-5 = 1e-8 of solver noise plus
    O(h^2) truncation; the factor 100 covers both;
  * against ref_tangent's M: 64 D eps kappa_inf(I + B_ref) max(1, |M_ref|_inf);
  * symplectic defect of every jac[i, k]: 256 eps kappa_inf(I + B_ref) max(1, |M_ref|_inf^2);
  * mono against the ordered product of the device's jac: (nm - 1) D eps prod |M_i|_inf;
  * exponents against ref_tangent's Gram-Schmidt on ref_tangent's Jacobians along the reference orbit: LYAP_TOL = 2.22e-14,
    100 x 2.22e-16, which is how far Gram-Schmidt and numpy.linalg.qr disagree at most on those reference matrices (measured on
    the CPU over the six cases: 1.2e-16 .. 2.22e-16); and |sum_c lyap_c| <= D (nm - 1) 256 eps, because det M = 1."""
import numpy as np
import pytest
import scipy.optimize

from tests import ref_tangent as RT
from tests.test_gpu_applymap_nd import CASES, NM, NT, NTEST, TWO_PI, _hyp, _ref_map_nd, _starts, _training

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
FD_TOL = dict(rtol=1e-6, atol=1e-6)
LYAP_TOL = 100 * 2.22e-16
H_FD = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _device():
    import sympgpr_amd
    if sympgpr_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need the MI355X")


def _kappa_norm(M, K):
    """per step and orbit: kappa_inf(I + B), |M|_inf"""
    kap = np.array([[np.linalg.cond(K[i, k], np.inf) for k in range(K.shape[1])] for i in range(K.shape[0])])
    return kap, np.abs(M).sum(axis=-1).max(axis=-1)


def _cpu_step(oracle, fam, d, hyp, X, alpha, q, p, explicit):
    """one unwrapped step of test_gpu_applymap_nd.py's CPU map from (q, p).  For a few of the perturbed starts hybrd ends with
    ier = 5 ("not making good progress") although it stands on the root -- with xtol = 1e-13 its progress test can fire at the
    rounding floor of the residual, 1e-16 here (seen on the CPU at 1 of 200 starts of A and D and 2 of 200 of C at d = 2) -- and
    _ref_map_nd asserts ier = 1.  Such a start is solved again here by the same solver with the same xtol, and the point is
    taken only if a second hybrd run started from it ends with ier = 1 without moving: the solver's own statement of convergence."""
    try:
        qs, ps, _ = _ref_map_nd(oracle, fam, d, hyp, X, alpha, 2, q[None, :], p[None, :], False, explicit=explicit)
        return np.concatenate((qs[1, 0], ps[1, 0]))
    except AssertionError:
        G = lambda P: oracle.build_K_nd(fam, np.concatenate((q, P))[None, :], X, hyp) @ alpha
        f = lambda P: G(P)[:d] - p + P
        P1 = scipy.optimize.fsolve(f, p, xtol=1e-13, full_output=True)[0]
        P2, _, ier, msg = scipy.optimize.fsolve(f, P1, xtol=1e-13, full_output=True)
        assert ier == 1 and np.abs(P2 - P1).max() <= 1e-13 * max(1.0, np.abs(P1).max()), msg
        return np.concatenate((q + G(P2)[d:], P2))


def _fd_jacobians(oracle, fam, d, hyp, X, alpha, q, p, explicit=False):
    """central differences of one CPU step from every point (q_i, p_i) of the orbit"""
    nm, Ntest = q.shape[:2]
    D = 2 * d
    z = np.concatenate((q[:-1], p[:-1]), axis=-1).reshape(-1, D)                      # (steps * Ntest, D)
    out = np.empty((len(z), D, D))
    for s, zs in enumerate(z):
        for j in range(D):
            e = H_FD * np.eye(D)[j]
            plus = _cpu_step(oracle, fam, d, hyp, X, alpha, (zs + e)[:d], (zs + e)[d:], explicit)
            minus = _cpu_step(oracle, fam, d, hyp, X, alpha, (zs - e)[:d], (zs - e)[d:], explicit)
            out[s, :, j] = (plus - minus) / (2 * H_FD)
    return out.reshape(nm - 1, Ntest, D, D)


@pytest.fixture(scope="module")
def refs(oracle):
    """per (family, d): the data and CPU orbits of test_gpu_applymap_nd.py and ref_tangent's Jacobians along them -- computed
    once, never changed"""
    out = {}
    for fam, d in CASES:
        X, z = _training(d)
        hyp = _hyp(fam, d)
        alpha = oracle.fit_nd(fam, X, z, hyp, 1e-8)[0]
        Q0, P0 = _starts(d)
        wrap = fam != "C"
        qr, pr, _ = _ref_map_nd(oracle, fam, d, hyp, X, alpha, NM, Q0, P0, wrap)
        assert np.isfinite(qr).all() and np.isfinite(pr).all()
        M, K = RT.jacobians(fam, d, hyp, X, alpha, qr, pr)
        for a in (X, z, hyp, alpha, Q0, P0, qr, pr, M, K):
            a.setflags(write=False)
        out[fam, d] = dict(X=X, z=z, hyp=hyp, alpha=alpha, Q0=Q0, P0=P0, wrap=wrap, q=qr, p=pr, M=M, K=K)
    return out


def _run(r, fam, d, **kw):
    from sympgpr_amd import maps
    return maps.run_map_nd_tangent(fam, d, maps.WRAP_Q if r["wrap"] else 0, NM, r["hyp"], r["X"], r["alpha"], r["Q0"], r["P0"], **kw)


@pytest.mark.parametrize("fam,d", CASES)
def test_orbits_have_the_plain_entries_bits(refs, fam, d):
    from sympgpr_amd import maps
    from sympgpr_amd.fit import SympFit
    r = refs[fam, d]
    q0, p0, i0 = maps.run_map_nd(fam, d, maps.WRAP_Q if r["wrap"] else 0, NM, r["hyp"], r["X"], r["alpha"], r["Q0"], r["P0"],
                                 return_iters=True)
    q, p, it, out = _run(r, fam, d)
    assert q.tobytes() == q0.tobytes() and p.tobytes() == p0.tobytes() and it.tobytes() == i0.tobytes()
    q, p, it, none = _run(r, fam, d, jac=False, mono=False, lyap=False)                  # no output wanted: the same launch
    assert none == {} and q.tobytes() == q0.tobytes() and p.tobytes() == p0.tobytes() and it.tobytes() == i0.tobytes()
    with SympFit.pairs(fam, r["X"], r["z"], r["hyp"], 1e-8) as f:
        f.run()
        qh0, ph0, ih0 = f.applymap_pairs(NM, r["Q0"], r["P0"], wrap_q=r["wrap"], return_iters=True)
        qh, ph, ih, outh = f.applymap_pairs_tangent(NM, r["Q0"], r["P0"], wrap_q=r["wrap"])
    assert qh.tobytes() == qh0.tobytes() and ph.tobytes() == ph0.tobytes() and ih.tobytes() == ih0.tobytes()
    D = 2 * d
    assert outh["jac"].shape == (NM - 1, NTEST, D, D) and outh["mono"].shape == (NTEST, D, D) and outh["lyap"].shape == (NTEST, D)
    assert all(np.isfinite(v).all() for v in outh.values())
    # the fit's own alpha is another solve of the same system: the same Jacobians to the parity tolerance of the map itself
    np.testing.assert_allclose(outh["jac"], out["jac"], rtol=1e-8, atol=1e-8)


def test_bits_do_not_depend_on_the_call_or_the_batch(refs):
    from sympgpr_amd import maps
    r = refs["A", 3]
    args = ("A", 3, maps.WRAP_Q, NM, r["hyp"], r["X"], r["alpha"])
    a = maps.run_map_nd_tangent(*args, r["Q0"], r["P0"])
    b = maps.run_map_nd_tangent(*args, r["Q0"], r["P0"])
    for name in ("jac", "mono", "lyap"):
        assert a[3][name].tobytes() == b[3][name].tobytes(), name
    c = maps.run_map_nd_tangent(*args, r["Q0"][3:4], r["P0"][3:4])                      # alone
    e = maps.run_map_nd_tangent(*args, r["Q0"][2:5], r["P0"][2:5])                      # at index 1 of a batch of 3
    for got, at in ((c, 0), (e, 1)):
        assert got[0][:, at].tobytes() == a[0][:, 3].tobytes() and got[1][:, at].tobytes() == a[1][:, 3].tobytes()
        assert got[3]["jac"][:, at].tobytes() == a[3]["jac"][:, 3].tobytes()
        assert got[3]["mono"][at].tobytes() == a[3]["mono"][3].tobytes()
        assert got[3]["lyap"][at].tobytes() == a[3]["lyap"][3].tobytes()


@pytest.mark.parametrize("fam,d", CASES)
def test_jacobian_against_central_differences_and_the_restatement(refs, oracle, fam, d):
    r = refs[fam, d]
    D = 2 * d
    jac = _run(r, fam, d, mono=False, lyap=False)[3]["jac"]
    assert jac.shape == r["M"].shape and np.isfinite(jac).all()
    fd = _fd_jacobians(oracle, fam, d, r["hyp"], r["X"], r["alpha"], r["q"], r["p"])
    kap, nrm = _kappa_norm(r["M"], r["K"])
    bound = 64 * D * EPS * kap * np.maximum(1.0, nrm)
    err = np.abs(jac - r["M"]).max(axis=(-2, -1))
    print("%s d=%d  max |jac - fd| = %.3e  max |jac - M_ref| = %.3e (bound %.3e .. %.3e, worst ratio %.3f)  max kappa %.3f  max |M| %.3f"
          % (fam, d, np.abs(jac - fd).max(), err.max(), bound.min(), bound.max(), (err / bound).max(), kap.max(), nrm.max()))
    np.testing.assert_allclose(jac, fd, **FD_TOL)
    assert (err <= bound).all(), (err / bound).max()


@pytest.mark.parametrize("fam,d", CASES)
def test_symplecticity_and_the_product(refs, fam, d):
    from sympgpr_amd import maps
    r = refs[fam, d]
    D = 2 * d
    out = _run(r, fam, d)[3]
    kap, nrm = _kappa_norm(r["M"], r["K"])
    bound = 256 * EPS * kap * np.maximum(1.0, nrm ** 2)
    defect = maps.symplectic_defect(out["jac"])
    assert defect.shape == (NM - 1, NTEST)
    print("%s d=%d  max defect = %.3e (bound %.3e .. %.3e, worst ratio %.3f)" % (fam, d, defect.max(), bound.min(), bound.max(),
                                                                               (defect / bound).max()))
    assert (defect <= bound).all()
    for k in range(NTEST):
        prod = RT.monodromy(out["jac"][:, k])
        tol = (NM - 1) * D * EPS * np.prod(np.abs(out["jac"][:, k]).sum(axis=-1).max(axis=-1))
        err = np.abs(out["mono"][k] - prod).max()
        print("  orbit %d: max |mono - prod jac| = %.3e (bound %.3e)" % (k, err, tol))
        assert err <= tol


@pytest.mark.parametrize("fam,d", CASES)
def test_exponents(refs, fam, d):
    r = refs[fam, d]
    D = 2 * d
    lyap = _run(r, fam, d, jac=False, mono=False)[3]["lyap"]
    want = np.array([RT.benettin(r["M"][:, k]) for k in range(NTEST)])
    print("%s d=%d  max |lyap - ref| = %.3e (tol %.3e)  max |sum lyap| = %.3e (bound %.3e)  max |lyap| = %.3f"
          % (fam, d, np.abs(lyap - want).max(), LYAP_TOL, np.abs(lyap.sum(axis=1)).max(), D * (NM - 1) * 256 * EPS, np.abs(want).max()))
    assert np.abs(want).max() > 1e-2
    np.testing.assert_allclose(lyap, want, rtol=0, atol=LYAP_TOL)
    assert (np.abs(lyap.sum(axis=1)) <= D * (NM - 1) * 256 * EPS).all()


@pytest.mark.parametrize("n0", [0, 1])
def test_tiny_training_sets(n0):
    """n0 = 0: M = I exactly and the exponents are 0; n0 = 1 against the restatement"""
    from sympgpr_amd import maps
    d, D, nm, Ntest = 3, 6, 3, 2
    rng = np.random.default_rng(40 + n0)
    X = np.hstack((rng.uniform(0, TWO_PI, (n0, d)), rng.uniform(-1, 1, (n0, d))))
    alpha = rng.standard_normal(D * n0) * 0.1
    hyp = _hyp("A", d)
    Q0, P0 = _starts(d, Ntest)
    q, p, it, out = maps.run_map_nd_tangent("A", d, 0, nm, hyp, X, alpha, Q0, P0)
    q0, p0 = maps.run_map_nd("A", d, 0, nm, hyp, X, alpha, Q0, P0)
    assert q.tobytes() == q0.tobytes() and p.tobytes() == p0.tobytes()
    if n0 == 0:
        assert (out["jac"] == np.eye(D)).all() and (out["mono"] == np.eye(D)).all() and (out["lyap"] == 0.0).all()
        return
    M, K = RT.jacobians("A", d, hyp, X, alpha, q, p)
    kap, nrm = _kappa_norm(M, K)
    assert np.abs(M - np.eye(D)).max() > 1e-4
    assert (np.abs(out["jac"] - M).max(axis=(-2, -1)) <= 64 * D * EPS * kap * np.maximum(1.0, nrm)).all()


@pytest.mark.parametrize("n0", [1024, 1025])
def test_both_sides_of_the_staging_switch(oracle, n0):
    """the staged 256-thread instance (n0 = 1024) and the 512-thread instance that reads from memory (1025) at d = 3, nm = 3,
    alpha drawn at random and scaled as in test_gpu_applymap_nd.py::test_kernel_edges, where every solve converges; the CPU
    orbit is checked to be finite before it is used, and the restatement is evaluated along it."""
    from sympgpr_amd import maps
    d, D, Ntest, nm = 3, 6, 3, 3
    rng = np.random.default_rng(100 + n0)
    X = np.hstack((rng.uniform(0, TWO_PI, (n0, d)), rng.uniform(-1, 1, (n0, d))))
    alpha = rng.standard_normal(D * n0) * 0.1 / np.sqrt(n0)
    hyp = _hyp("A", d)
    Q0, P0 = _starts(d, Ntest)
    qr, pr, gmax = _ref_map_nd(oracle, "A", d, hyp, X, alpha, nm, Q0, P0, True)
    assert np.isfinite(qr).all() and np.isfinite(pr).all()
    q, p, it, out = maps.run_map_nd_tangent("A", d, maps.WRAP_Q, nm, hyp, X, alpha, Q0, P0)
    q0, p0 = maps.run_map_nd("A", d, maps.WRAP_Q, nm, hyp, X, alpha, Q0, P0)
    assert q.tobytes() == q0.tobytes() and p.tobytes() == p0.tobytes() and (it >= 1).all()
    np.testing.assert_allclose(q, qr, rtol=1e-8, atol=1e-8 * max(1.0, gmax))
    M, K = RT.jacobians("A", d, hyp, X, alpha, qr, pr)
    kap, nrm = _kappa_norm(M, K)
    bound = 64 * D * EPS * kap * np.maximum(1.0, nrm)
    err = np.abs(out["jac"] - M).max(axis=(-2, -1))
    print("n0 = %d  max |jac - M_ref| = %.3e (bound %.3e)  max |M - I| = %.3e  defect %.3e" %
          (n0, err.max(), bound.min(), np.abs(M - np.eye(D)).max(), maps.symplectic_defect(out["jac"]).max()))
    assert np.abs(M - np.eye(D)).max() > 1e-4
    assert (err <= bound).all()
    assert (maps.symplectic_defect(out["jac"]) <= 256 * EPS * kap * np.maximum(1.0, nrm ** 2)).all()
    want = np.array([RT.benettin(M[:, k]) for k in range(Ntest)])
    np.testing.assert_allclose(out["lyap"], want, rtol=0, atol=LYAP_TOL)
    np.testing.assert_allclose(out["mono"], np.array([RT.monodromy(M[:, k]) for k in range(Ntest)]), rtol=0,
                               atol=(nm - 1) * 64 * D * EPS * (kap * np.maximum(1.0, nrm)).max() * nrm.max())


def test_d1_handle_greene_residue(oracle):
    """a d = 1 pairs fit (family A) runs the D = 2 instance: Greene's residue of mono against the restatement's, along the
    device orbit with the fit's own alpha"""
    from tests.test_gpu_examples import _training as training_d1
    from sympgpr_amd import maps
    from sympgpr_amd.fit import SympFit
    t = training_d1(oracle, "A")
    nm, Ntest = 6, 5
    rng = np.random.default_rng(5)
    Q0, P0 = rng.uniform(0.5, 5.5, Ntest), rng.uniform(-0.6, 0.6, Ntest)
    X = np.column_stack((t["q"], t["pn"]))
    with SympFit.pairs("A", X, t["ztrain"], t["hyp"], 1e-8) as f:
        alpha = f.run().alpha()
        q0, p0 = f.applymap_pairs(nm, Q0, P0, wrap_q=True)
        q, p, it, out = f.applymap_pairs_tangent(nm, Q0, P0, wrap_q=True)
    assert q.tobytes() == q0.tobytes() and p.tobytes() == p0.tobytes()
    assert np.isfinite(q).all() and out["mono"].shape == (Ntest, 2, 2)
    M, K = RT.jacobians("A", 1, t["hyp"], X, alpha, q, p)
    want = np.array([RT.monodromy(M[:, k]) for k in range(Ntest)])
    kap, nrm = _kappa_norm(M, K)
    tol = (nm - 1) * 64 * 2 * EPS * (kap * np.maximum(1.0, nrm)).max() * np.prod(nrm.max(axis=1))
    res, res_ref = maps.greene_residue(out["mono"]), maps.greene_residue(want)
    print("residues", res, " max |diff| = %.3e (tol %.3e)" % (np.abs(res - res_ref).max(), tol))
    assert np.abs(res - res_ref).max() <= tol
    assert (maps.symplectic_defect(out["jac"]) <= 256 * EPS * kap * np.maximum(1.0, nrm ** 2)).all()


def test_explicit_mode_family_b(oracle):
    """the sum kernel's explicit map at d = 2 on the separable data of test_gpu_applymap_nd.py::test_explicit_mode_family_b:
    jac against central differences of the explicit CPU recurrence (rtol = atol = 1e-6, as above), and the symplecticity bound
    with kappa = 1 (B = 0)"""
    from sympgpr_amd import maps
    d = 2
    X, z = _training(d, c=0.0)
    hyp = _hyp("B", d)
    alpha = oracle.fit_nd("B", X, z, hyp, 1e-8)[0]
    Q0, P0 = _starts(d)
    qr, pr, _ = _ref_map_nd(oracle, "B", d, hyp, X, alpha, NM, Q0, P0, True, explicit=True)
    assert np.isfinite(qr).all() and np.isfinite(pr).all()
    mode = maps.WRAP_Q | maps.EXPLICIT
    q, p, it, out = maps.run_map_nd_tangent("B", d, mode, NM, hyp, X, alpha, Q0, P0)
    q0, p0, i0 = maps.run_map_nd("B", d, mode, NM, hyp, X, alpha, Q0, P0, return_iters=True)
    assert q.tobytes() == q0.tobytes() and p.tobytes() == p0.tobytes() and it.tobytes() == i0.tobytes() and (it == 0).all()
    fd = _fd_jacobians(oracle, "B", d, hyp, X, alpha, qr, pr, explicit=True)
    nrm = np.abs(fd).sum(axis=-1).max(axis=-1)
    defect = maps.symplectic_defect(out["jac"])
    print("B explicit  max |jac - fd| = %.3e  max defect = %.3e (bound %.3e)" % (np.abs(out["jac"] - fd).max(), defect.max(),
                                                                                 (256 * EPS * np.maximum(1.0, nrm ** 2)).min()))
    assert np.abs(fd - np.eye(2 * d)).max() > 1e-2
    np.testing.assert_allclose(out["jac"], fd, **FD_TOL)
    assert (defect <= 256 * EPS * np.maximum(1.0, nrm ** 2)).all()


def test_user_family_is_family_c(refs, golden_dir):
    """the USER slot as shipped is family C printed by the generator: gen::factor3 against the hand form, 1e-12"""
    import os
    uf = np.load(os.path.join(golden_dir, "user_family.npz"))
    if str(uf["definition"]) != "exp(-(x_a - x_b)**2/(2*lx**2))*exp(-(y_a - y_b)**2/(2*ly**2))":
        pytest.skip("USER_FAMILY has been edited: no hand-written twin to compare with")
    r = refs["C", 3]
    a = _run(r, "C", 3)
    b = _run(r, "USER", 3)
    np.testing.assert_allclose(b[0], a[0], rtol=0, atol=1e-12)
    for name in ("jac", "mono", "lyap"):
        np.testing.assert_allclose(b[3][name], a[3][name], rtol=0, atol=1e-12, err_msg=name)


def test_lost_orbit(refs):
    from sympgpr_amd import maps
    r = refs["A", 2]
    args = ("A", 2, maps.WRAP_Q, NM, r["hyp"], r["X"], r["alpha"])
    base = maps.run_map_nd_tangent(*args, r["Q0"], r["P0"])
    Q0 = r["Q0"].copy()
    Q0[1, 1] = np.nan                                   # an orbit that starts NaN stays NaN: nothing is provoked
    q, p, it, out = maps.run_map_nd_tangent(*args, Q0, r["P0"])
    assert np.isnan(q[1:, 1]).all() and (it[:, 1] == -1).all()
    assert np.isnan(out["jac"][:, 1]).all() and np.isnan(out["mono"][1]).all() and np.isnan(out["lyap"][1]).all()
    keep = [0, 2, 3, 4]
    assert q[:, keep].tobytes() == base[0][:, keep].tobytes() and p[:, keep].tobytes() == base[1][:, keep].tobytes()
    assert out["jac"][:, keep].tobytes() == base[3]["jac"][:, keep].tobytes()
    assert out["mono"][keep].tobytes() == base[3]["mono"][keep].tobytes()
    assert out["lyap"][keep].tobytes() == base[3]["lyap"][keep].tobytes()


def test_degenerate_calls(refs):
    r = refs["A", 2]
    from sympgpr_amd import maps
    q, p, it, out = maps.run_map_nd_tangent("A", 2, 0, 1, r["hyp"], r["X"], r["alpha"], r["Q0"], r["P0"], lyap=False)
    assert out["jac"].shape == (0, NTEST, 4, 4) and (out["mono"] == np.eye(4)).all()
    q, p, it, out = maps.run_map_nd_tangent("A", 2, 0, 4, r["hyp"], r["X"], r["alpha"], np.zeros((0, 2)), np.zeros((0, 2)))
    assert out["jac"].shape == (3, 0, 4, 4) and out["lyap"].shape == (0, 4)


def test_errors(refs):
    """explicit mode with a product family raises through the Python layer (SGPR_E_ARG, -1); an unsolved fit, a reg=True fit and
    a block="qq" fit give SGPR_E_STATE (-5)"""
    from sympgpr_amd import SympGPRError, maps
    from sympgpr_amd.fit import SympFit
    r = refs["A", 2]
    with pytest.raises(SympGPRError, match=r"applymap_nd_tangent_host.*sum kernels"):
        maps.run_map_nd_tangent("A", 2, maps.EXPLICIT, NM, r["hyp"], r["X"], r["alpha"], r["Q0"], r["P0"])
    with SympFit.pairs("A", r["X"], r["z"], r["hyp"], 1e-8) as f:
        with pytest.raises(SympGPRError, match=r"\(-5\).*not solved"):
            f.applymap_pairs_tangent(3, r["Q0"], r["P0"])
        with pytest.raises(SympGPRError, match=r"fit_applymap_nd_tangent.*sum kernels"):
            f.run().applymap_pairs_tangent(3, r["Q0"], r["P0"], explicit=True)
    x, y = r["X"][:, 0], r["X"][:, 2]
    with SympFit("A", x, y, r["z"][:NT], [1.2, 1.5, 1.0], 1e-2, reg=True) as f:
        with pytest.raises(SympGPRError, match=r"\(-5\).*scalar-kernel"):
            f.run().applymap_pairs_tangent(3, x[:3], y[:3])
    with SympFit("A", x, y, r["z"][:NT], [1.2, 1.5, 1.0], 1e-2, block="qq") as f:
        with pytest.raises(SympGPRError, match=r"\(-5\).*single-block"):
            f.run().applymap_pairs_tangent(3, x[:3], y[:3])
