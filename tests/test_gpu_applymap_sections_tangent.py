"""GPU tests of the sectioned map's tangent (sgpr_applymap_sections_tangent_host, maps.run_map_sections_tangent,
maps.tangent_from_jac, examples/tokamak_split.applymap_tok_tangent).

The orbits are held to the plain entry bit for bit.  The step matrices are held to a long-double restatement of the Hessian sums
at the level of the sums themselves: from jac, T = jac[1,1], A = -jac[1,0] / T, C = jac[0,1] / T, B = 1 / T - 1, each against
the np.longdouble sum at (qmap[i], pmap[i+1]) of section (first + i) mod nsec with the bound
    (32 + n0) eps sum_j |term_j|  +  8 eps max(1, |H|)
-- the first part the project's form for summed device values, the second the recovery's few roundings.  (The d-pair test's
64 D eps kappa max(1, |M|) does not fit these fixtures: noise 1e-8, |alpha| up to 1.5e3 and a cancellation of 1e7 - 1e8 in the
sums leave a float64 evaluation of the reference itself 6 - 15 times outside it.)  jac[0,0] is held by det jac = 1.  Structure:
|det - 1| <= 256 eps |1 / (1 + B_ref)| max(1, |M_ref|_inf^2); mono against the ordered product of the device's jac,
(nm - 1) D eps prod |M_i|_inf; lyap against ref_tangent.benettin on the device's jac, 2.22e-14; |lyap_0 + lyap_1| <=
D (nm - 1) 256 eps; lyap against the reference's Jacobians within 4 x the first-order bound mean_i(dM_i |M_i^-1|_inf), dM_i
propagated from the Hessian bound.  And central differences of the plain entry, one step at a time (h = 1e-5, rtol = atol = 1e-6)."""
import functools
import os

import numpy as np
import pytest

from tests import ref_tangent as RT
from tests.test_gpu_applymap_sections import MODE_TOK, _compute_r, _run, _same, _sections, _starts

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = np.finfo(np.float64).eps
TWO_PI = 2.0 * np.pi
LYAP_TOL = 2.22e-14
D = 2
SUBSETS = [dict(jac=bool(b & 1), mono=bool(b & 2), lyap=bool(b & 4)) for b in range(8)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    import sympgpr_amd
    if sympgpr_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need the MI355X")


def _runt(d, mode, nm, Q0, P0, first=0, want_pdiff=False, **sw):
    from sympgpr_amd import maps
    return maps.run_map_sections_tangent(mode, nm, len(Q0), d["hyp"], d["xt"], d["yt"], d["alpha"], Q0, P0, d["hypp"], d["xp"],
                                         d["yp"], d["alphap"], first=first, want_pdiff=want_pdiff, family=d["fam"], **sw)


# ---- the reference: the three Hessian sums of one section at one point, term by term in long double

def _factor(periodic, hs, l, dx):
    """g = f'/f, nh = -f''/f, th = f'''/f and log f of one coordinate's factor at dx = x_train - x (long double)"""
    l2 = l * l
    if periodic:
        a = -np.sin(hs * dx) ** 2 / (2 * l2)
        a1 = -hs * np.sin(2 * hs * dx) / (2 * l2)
        a2 = -hs * hs * np.cos(2 * hs * dx) / l2
        a3 = 2 * hs ** 3 * np.sin(2 * hs * dx) / l2
    else:
        a, a1, a2, a3 = -dx * dx / (2 * l2), -dx / l2, -1 / l2 + 0 * dx, 0 * dx
    return a, a1, -(a2 + a1 * a1), a3 + 3 * a1 * a2 + a1 ** 3


def _terms(fam, hyp, x, y, al, q, P):
    """the per-point terms of A = H_qq, B = H_qP, C = H_PP -> (3, n0) long double"""
    hyp = np.asarray(hyp, dtype=LD)
    n0 = len(x)
    hs = hyp[2] if fam == "D" else LD(0.5)
    aq, gq, nq, tq = _factor(fam in "ABD", hs, hyp[0], np.asarray(x, dtype=LD) - LD(q))
    aP, gP, nP, tP = _factor(False, None, hyp[1], np.asarray(y, dtype=LD) - LD(P))
    a1, a2, sig = np.asarray(al[:n0], dtype=LD), np.asarray(al[n0:], dtype=LD), hyp[-1]
    if fam == "B":
        return np.stack((sig * np.exp(aq) * a1 * tq, 0 * aq, sig * np.exp(aP) * a2 * tP))
    E = sig * np.exp(aq + aP)
    return np.stack((E * (a1 * tq - nq * gP * a2), -E * (gP * nq * a1 + gq * nP * a2), E * (a2 * tP - nP * gq * a1)))


def _ref_hessians(d, first, q, p):
    """along the device's orbit: H (steps, n, 3) = (A, B, C) and S = the sums of |term|, float64 from long double; NaN where
    the step was not accepted (p[i + 1] NaN)"""
    steps, n = q.shape[0] - 1, q.shape[1]
    H, S = np.full((steps, n, 3), np.nan), np.full((steps, n, 3), np.nan)
    for i in range(steps):
        m = (first + i) % d["nsec"]
        for k in range(n):
            if np.isfinite(p[i + 1, k]):
                t = _terms(d["fam"], d["hyp"][m], d["xt"][:, m], d["yt"][:, m], d["alpha"][:, m], q[i, k], p[i + 1, k])
                H[i, k], S[i, k] = t.sum(axis=1).astype(np.float64), np.abs(t).sum(axis=1).astype(np.float64)
    return H, S


def _hess_bound(n0, H, S):
    return (32 + n0) * EPS * S + 8 * EPS * np.maximum(1.0, np.abs(H))


def _recover(jac):
    """(A, B, C) from the step matrices (..., 2, 2)"""
    T = jac[..., 1, 1]
    return np.stack((-jac[..., 1, 0] / T, 1.0 / T - 1.0, jac[..., 0, 1] / T), axis=-1)


def _step_matrices(H):
    """M (..., 2, 2) from H (..., 3) = (A, B, C)"""
    A, B, C = H[..., 0], H[..., 1], H[..., 2]
    T = 1.0 / (1.0 + B)
    return np.stack((np.stack((1.0 + B - C * T * A, C * T), axis=-1), np.stack((-T * A, T), axis=-1)), axis=-2)


def _check_hessians(label, d, first, q, p, jac):
    """test 2 on one launch's outputs -> H_ref, S_ref, the bound; asserts the NaN pattern of jac too"""
    n0 = d["xt"].shape[0]
    H, S = _ref_hessians(d, first, q, p)
    live = np.isfinite(p[1:])
    assert np.array_equal(np.isfinite(jac).all(axis=(2, 3)), live) and np.array_equal(np.isnan(jac).all(axis=(2, 3)), ~live)
    assert live.any()
    got, bound = _recover(jac), _hess_bound(n0, H, S)
    err = np.abs(got - H)
    ratio = (err[live] / bound[live]).max(axis=0)
    cancel = (S[live] / np.maximum(np.abs(H[live]), 1e-300))[:, [0, 2]].max()
    print("%s: max |H_dev - H_ref| / bound = A %.4f  B %.4f  C %.4f   (%d steps, max |H| %.3g, cancellation up to %.1e)"
          % (label, ratio[0], ratio[1], ratio[2], live.sum(), np.abs(H[live]).max(), cancel))
    assert (err[live] <= bound[live]).all()
    return H, S, bound, live


def _check_defect(label, jac, H, live):
    Mr = _step_matrices(H[live])
    nrm = np.abs(Mr).sum(axis=-1).max(axis=-1)
    bound = 256 * EPS * np.abs(1.0 / (1.0 + H[live][:, 1])) * np.maximum(1.0, nrm ** 2)
    J = jac[live]
    defect = np.abs(J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0] - 1.0)      # the symplectic defect of a 2 x 2 matrix
    print("%s: max |det jac - 1| / bound = %.4f (max defect %.3e)" % (label, (defect / bound).max(), defect.max()))
    assert (defect <= bound).all()


# ---- 1. the orbit's bits, every subset of the outputs

CASE1 = [(fam, first) for fam in ("A", "C", "D", "B") for first in (0, 1, 2)]
NM1 = 10


@functools.lru_cache(maxsize=None)
def _case1(fam, first):
    d = _sections(fam, 3, 40, 43)
    Q0, P0 = _starts(8, 6, 2)
    q, p, pd, t = _runt(d, MODE_TOK, NM1, Q0, P0, first=first, want_pdiff=True)
    return d, Q0, P0, q, p, pd, t


@pytest.mark.parametrize("fam,first", CASE1)
def test_orbit_bits_are_the_plain_entry_s(fam, first):
    d, Q0, P0, q, p, pd, t = _case1(fam, first)
    qr, pr, pdr = _run(d, MODE_TOK, NM1, Q0, P0, first=first, want_pdiff=True)
    lost = np.isnan(pr[-1])
    assert lost.any() and (~lost).any()
    assert _same(q, qr) and _same(p, pr) and _same(pd, pdr)
    assert t["jac"].shape == (NM1 - 1, 8, 2, 2) and t["mono"].shape == (8, 2, 2) and t["lyap"].shape == (8, 2)
    for sw in SUBSETS:
        out = _runt(d, MODE_TOK, NM1, Q0, P0, first=first, want_pdiff=True, **sw)
        assert _same(out[0], qr) and _same(out[1], pr) and _same(out[2], pdr), sw
        assert sorted(out[3]) == sorted(k for k, v in sw.items() if v)
        for k in out[3]:
            assert _same(out[3][k], t[k]), (sw, k)                   # an output does not depend on which others are asked for
        q2, p2, t2 = _runt(d, MODE_TOK, NM1, Q0, P0, first=first, **sw)
        assert _same(q2, qr) and _same(p2, pr)


# ---- 2. jac against the restatement, at the level of the Hessian sums

@pytest.mark.parametrize("fam,first", CASE1)
def test_hessian_sums_against_long_double(fam, first):
    d, Q0, P0, q, p, pd, t = _case1(fam, first)
    H, S, bound, live = _check_hessians("%s first %d" % (fam, first), d, first, q, p, t["jac"])
    if fam == "B":
        assert (H[live][:, 1] == 0).all() and (_recover(t["jac"])[live][:, 1] == 0).all()
    _check_defect("%s first %d" % (fam, first), t["jac"], H, live)          # ... and jac[0,0] through det jac = 1


@pytest.mark.parametrize("n0", [1, 63, 64, 65, 255, 256, 257])
def test_size_edges(n0):
    d = _sections("A", 2, n0, n0 + 3)
    Q0, P0 = _starts(3, 7)
    q, p, t = _runt(d, 1, 4, Q0, P0, first=1)
    qr, pr = _run(d, 1, 4, Q0, P0, first=1)
    assert _same(q, qr) and _same(p, pr) and np.isfinite(p[-1]).any()
    H, S, bound, live = _check_hessians("n0 = %d" % n0, d, 1, q, p, t["jac"])
    _check_defect("n0 = %d" % n0, t["jac"], H, live)


@pytest.mark.parametrize("n0,n0p", [(320, 320), (321, 320)], ids=["staged-8960", "unstaged-8964"])
def test_both_sides_of_the_staging_rule(n0, n0p):
    nsec, nm = 4, 5
    assert (nsec * (4 * n0 + 3 * n0p) <= 8960) == (n0 == 320) and (n0 != 320 or nsec * (4 * n0 + 3 * n0p) == 8960)
    d = _sections("A", nsec, n0, n0p)
    Q0, P0 = _starts(3, 8)
    q, p, t = _runt(d, 1, nm, Q0, P0, first=2)
    qr, pr = _run(d, 1, nm, Q0, P0, first=2)
    assert _same(q, qr) and _same(p, pr) and np.isfinite(p[-1]).any()
    H, S, bound, live = _check_hessians("n0 = %d, n0p = %d" % (n0, n0p), d, 2, q, p, t["jac"])
    _check_defect("n0 = %d" % n0, t["jac"], H, live)
    prod = np.array([RT.monodromy(t["jac"][:, k]) for k in range(3)])
    tol = (nm - 1) * D * EPS * np.prod(np.abs(t["jac"]).sum(axis=-1).max(axis=-1), axis=0)
    assert (np.abs(t["mono"] - prod).max(axis=(1, 2)) <= tol)[np.isfinite(p[-1])].all()


# ---- 3. structure: the product, the exponents

@pytest.mark.parametrize("fam,first", CASE1)
def test_product_and_exponents(fam, first):
    d, Q0, P0, q, p, pd, t = _case1(fam, first)
    jac, mono, lyap = t["jac"], t["mono"], t["lyap"]
    alive = np.isfinite(p[-1])
    assert np.isnan(mono[~alive]).all() and np.isnan(lyap[~alive]).all()
    assert np.isfinite(mono[alive]).all() and np.isfinite(lyap[alive]).all()
    H, S = _ref_hessians(d, first, q, p)
    dH = _hess_bound(d["xt"].shape[0], H, S)
    for k in np.nonzero(alive)[0]:
        prod = RT.monodromy(jac[:, k])
        tol = (NM1 - 1) * D * EPS * np.prod(np.abs(jac[:, k]).sum(axis=-1).max(axis=-1))
        err = np.abs(mono[k] - prod).max()
        want = RT.benettin(jac[:, k])
        # the reference's Jacobians along the same orbit; dM entrywise from dA, dB, dC to first order
        A, B, C = H[:, k].T
        dA, dB, dC = dH[:, k].T
        T = 1.0 / (1.0 + B)
        dT = T * T * dB
        dM = np.stack((np.stack((dB + np.abs(T * A) * dC + np.abs(C * T) * dA + np.abs(C * A) * dT, np.abs(T) * dC + np.abs(C) * dT),
                                axis=-1), np.stack((np.abs(T) * dA + np.abs(A) * dT, dT), axis=-1)), axis=-2)
        Mr = _step_matrices(H[:, k])
        aM = np.abs(Mr)                                 # |M^-1|_inf, M^-1 = [[M11, -M01], [-M10, M00]] for determinant 1
        inv = np.maximum(aM[:, 1, 1] + aM[:, 0, 1], aM[:, 1, 0] + aM[:, 0, 0])
        first_order = np.mean(dM.sum(axis=-1).max(axis=-1) * inv)
        ref = RT.benettin(Mr)
        print("%s first %d orbit %d: |mono - prod jac| %.3e (bound %.3e)  |lyap - benettin(jac)| %.3e (tol %.3e)  |sum lyap| %.3e "
              "(bound %.3e)  |lyap - benettin(M_ref)| %.3e (4 x first-order bound %.3e)  lyap %+.4f %+.4f"
              % (fam, first, k, err, tol, np.abs(lyap[k] - want).max(), LYAP_TOL, abs(lyap[k].sum()), D * (NM1 - 1) * 256 * EPS,
                 np.abs(lyap[k] - ref).max(), 4 * first_order, lyap[k, 0], lyap[k, 1]))
        assert err <= tol
        assert np.abs(lyap[k] - want).max() <= LYAP_TOL
        assert abs(lyap[k].sum()) <= D * (NM1 - 1) * 256 * EPS
        assert np.abs(lyap[k] - ref).max() <= 4 * first_order


# ---- 4. central differences of the plain entry

def _fd_check(label, d, mode, first, q, p, jac, steps, h=1e-5):
    """jac[i, k] against central differences of ONE plain step from (q[i, k], p[i, k]): four perturbed starts per orbit in one
    launch per step.  Steps whose start, end or perturbed ends are lost are skipped; at least 80 % of the live ones compare."""
    n = q.shape[1]
    live_n, done, worst = 0, 0, 0.0
    for i in range(steps):
        live = np.isfinite(p[i]) & np.isfinite(p[i + 1])
        live_n += live.sum()
        Q0 = np.concatenate((q[i] + h, q[i] - h, q[i], q[i]))
        P0 = np.concatenate((p[i], p[i], p[i] + h, p[i] - h))
        qq, pp = _run(d, mode, 2, Q0, P0, first=(first + i) % d["nsec"])
        Q1, P1 = qq[1].reshape(4, n), pp[1].reshape(4, n)
        ang = lambda a: np.mod(a + np.pi, TWO_PI) - np.pi
        fd = np.empty((n, 2, 2))
        fd[:, 0, 0], fd[:, 0, 1] = ang(Q1[0] - Q1[1]) / (2 * h), ang(Q1[2] - Q1[3]) / (2 * h)
        fd[:, 1, 0], fd[:, 1, 1] = (P1[0] - P1[1]) / (2 * h), (P1[2] - P1[3]) / (2 * h)
        ok = live & np.isfinite(fd).all(axis=(1, 2))
        done += ok.sum()
        if ok.any():
            worst = max(worst, np.abs(jac[i][ok] - fd[ok]).max())
            np.testing.assert_allclose(jac[i][ok], fd[ok], rtol=1e-6, atol=1e-6)
    print("%s: %d of %d live (step, orbit) pairs compared, max |jac - central difference| = %.3e" % (label, done, live_n, worst))
    assert live_n > 0 and done >= 0.8 * live_n


@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "driver_tokamak_split.npz"))
    N, nph, nm, Ntest = int(g["N"]), int(g["nphmap"]), int(g["nm"]), int(g["Ntest"])
    assert (N, nph, nm, Ntest) == (70, 4, 25, 8)
    d = dict(fam="A", nsec=nph, hyp=g["hyp"][:nph], hypp=g["hypp"][:nph], xt=g["q"], yt=g["P"], alpha=g["alpha"].T, xp=g["q"],
             yp=g["p"], alphap=g["alphap"].T)
    return g, d


def test_central_differences_on_the_reference_fixture():
    g, d = _golden()
    Q0, P0 = np.array(g["Q0map"], dtype=float), np.array(g["P0map"], dtype=float)
    q, p, t = _runt(d, MODE_TOK, 9, Q0, P0)
    _fd_check("fixture", d, MODE_TOK, 0, q, p, t["jac"], 8)


# ---- 5. chunks

@pytest.mark.parametrize("fam,first", [("A", 0), ("A", 2), ("D", 1)])
def test_chunks_repeat_the_jac_rows(fam, first):
    from sympgpr_amd import maps
    d, Q0, P0, q, p, pd, t = _case1(fam, first)
    qc, pc = np.zeros((NM1, 8)), np.zeros((NM1, 8))
    qc[0], pc[0] = Q0, P0
    rows = []
    for i in range(0, NM1 - 1, 4):
        kk = min(4, NM1 - 1 - i)
        qq, pp, tt = _runt(d, MODE_TOK, kk + 1, qc[i], pc[i], first=(first + i) % 3, mono=False, lyap=False)
        qc[i + 1:i + kk + 1], pc[i + 1:i + kk + 1] = qq[1:], pp[1:]
        rows.append(tt["jac"])
    jac = np.concatenate(rows)
    assert _same(qc, q) and _same(pc, p) and _same(jac, t["jac"])
    mono, lyap = maps.tangent_from_jac(jac)
    alive = np.isfinite(p[-1])
    assert np.isnan(mono[~alive]).all() and np.isnan(lyap[~alive]).all() and alive.any() and (~alive).any()
    tol = (NM1 - 1) * D * EPS * np.prod(np.abs(jac).sum(axis=-1).max(axis=-1), axis=0)
    err = np.abs(mono - t["mono"]).max(axis=(1, 2))
    print("%s first %d: max |tangent_from_jac mono - device mono| / bound = %.3f, max |lyap - device lyap| = %.3e (tol %.3e)"
          % (fam, first, (err / tol)[alive].max(), np.abs(lyap - t["lyap"])[alive].max(), LYAP_TOL))
    assert (err <= tol)[alive].all()
    assert np.abs(lyap - t["lyap"])[alive].max() <= LYAP_TOL


def test_applymap_tok_tangent_on_the_reference_fixture():
    from sympgpr_amd import maps
    from sympgpr_amd.examples import tokamak_split as ts
    g, d = _golden()
    N, nph, nm, Ntest = 70, 4, 25, 8
    xtrain, xtrainp = np.vstack((g["q"], g["P"])), np.vstack((g["q"], g["p"]))
    Kyinv, Kyinvp = np.stack([np.eye(2 * N)] * nph), np.stack([np.eye(N)] * nph)
    args = (nph, nm, Ntest, g["Q0map"], g["P0map"], xtrainp, g["alphap"].T, Kyinvp, g["hypp"], xtrain, g["alpha"].T, Kyinv, g["hyp"])
    qr, pr = ts.applymap_tok(*args, compute_r=_compute_r, steps_per_launch=4)
    out = [ts.applymap_tok_tangent(*args, compute_r=_compute_r, steps_per_launch=k) for k in (1, 4, 24)]
    q, p, t = out[0]
    assert _same(q, qr) and _same(p, pr)
    assert t["jac"].shape == (24, Ntest, 2, 2)
    lost = np.isnan(pr[1:])
    assert lost.any() and not lost.all()
    assert np.array_equal(np.isnan(t["jac"]).all(axis=(2, 3)), lost) and np.array_equal(np.isnan(t["jac"]).any(axis=(2, 3)), lost)
    for q2, p2, t2 in out[1:]:
        assert _same(q2, q) and _same(p2, p) and _same(t2["jac"], t["jac"]) and _same(t2["mono"], t["mono"]) and _same(t2["lyap"], t["lyap"])
    alive = ~lost[-1]
    assert np.isnan(t["lyap"][~alive]).all() and np.isfinite(t["lyap"][alive]).all() and np.isfinite(t["mono"][alive]).all()
    # without the callback: one launch, mono and lyap from the device, the same step matrices where both kept the orbit
    q1, p1, t1 = ts.applymap_tok_tangent(*args)
    q0, p0 = ts.applymap_tok(*args)
    assert _same(q1, q0) and _same(p1, p0)
    both = ~lost & np.isfinite(p1[1:])
    assert _same(t1["jac"][both], t["jac"][both])
    same = np.isfinite(p1[-1]) & alive
    assert same.any() and np.abs(t1["lyap"][same] - t["lyap"][same]).max() <= LYAP_TOL
    print("fixture: finite-time exponents of the 24 steps: %s; Greene residues %s"
          % (np.array2string(t1["lyap"][same][:, 0], precision=4), np.array2string(maps.greene_residue(t1["mono"][same]), precision=3)))


# ---- 6. independence and loss

def test_orbits_are_independent_and_a_lost_orbit_is_nan_from_its_step():
    d = _sections("A", 3, 40, 43)
    Q0, P0 = _starts(8, 9, 3)
    q, p, t = _runt(d, MODE_TOK, 6, Q0, P0, first=1)
    for k in range(8):
        q1, p1, t1 = _runt(d, MODE_TOK, 6, Q0[k:k + 1], P0[k:k + 1], first=1)
        assert _same(q1[:, 0], q[:, k]) and _same(p1[:, 0], p[:, k])
        assert _same(t1["jac"][:, 0], t["jac"][:, k]) and _same(t1["mono"][0], t["mono"][k]) and _same(t1["lyap"][0], t["lyap"][k])
    Qn, Pn = Q0.copy(), P0.copy()
    Qn[2], Pn[5] = np.nan, np.nan
    qn, pn, tn = _runt(d, MODE_TOK, 6, Qn, Pn, first=1)
    for k in (2, 5):
        assert np.isnan(tn["jac"][:, k]).all() and np.isnan(tn["mono"][k]).all() and np.isnan(tn["lyap"][k]).all()
    keep = [k for k in range(8) if k not in (2, 5)]
    assert _same(tn["jac"][:, keep], t["jac"][:, keep]) and _same(tn["mono"][keep], t["mono"][keep]) and _same(tn["lyap"][keep], t["lyap"][keep])
    # lost at step s: finite rows before s, NaN from s on, and NaN mono / lyap
    lost_at = np.where(np.isnan(p).any(axis=0), np.isnan(p).argmax(axis=0), 6)
    assert (lost_at < 6).any() and (lost_at == 6).any() and (lost_at[lost_at < 6] > 1).any()
    for k in range(8):
        s = lost_at[k]
        assert np.isfinite(t["jac"][:s - 1, k]).all() and np.isnan(t["jac"][s - 1:, k]).all()
        assert np.isnan(t["mono"][k]).all() == (s < 6) and np.isnan(t["lyap"][k]).all() == (s < 6)


# ---- 7. the explicit map of the sum kernel

def test_explicit_sum_kernel():
    d = _sections("B", 3, 40, 43)
    mode = 4 | 1
    Q0, P0 = _starts(8, 12)
    q, p, t = _runt(d, mode, NM1, Q0, P0, first=1)
    qr, pr = _run(d, mode, NM1, Q0, P0, first=1)
    assert _same(q, qr) and _same(p, pr) and np.isfinite(p).all()
    assert (t["jac"][:, :, 1, 1] == 1.0).all() and (_recover(t["jac"])[..., 1] == 0.0).all()
    _fd_check("explicit B", d, mode, 1, q, p, t["jac"], NM1 - 1)
    H, S, bound, live = _check_hessians("explicit B", d, 1, q, p, t["jac"])
    _check_defect("explicit B", t["jac"], H, live)


# ---- 8. degenerate calls

def test_degenerate_calls():
    d = _sections("A", 3, 40, 43)
    q, p, pd, t = _runt(d, MODE_TOK, 5, np.zeros(0), np.zeros(0), want_pdiff=True)
    assert q.shape == p.shape == pd.shape == (5, 0)
    assert t["jac"].shape == (4, 0, 2, 2) and t["mono"].shape == (0, 2, 2) and t["lyap"].shape == (0, 2)
    Q0, P0 = _starts(8, 11)
    q, p, pd, t = _runt(d, MODE_TOK, 1, Q0, P0, first=2, want_pdiff=True, lyap=False)
    assert np.array_equal(q, Q0[None]) and np.array_equal(p, P0[None]) and np.array_equal(pd, P0[None])
    assert t["jac"].shape == (0, 8, 2, 2) and np.array_equal(t["mono"], np.broadcast_to(np.eye(2), (8, 2, 2)))
    q, p, t = _runt(d, MODE_TOK, 2, Q0, P0, first=2)
    qr, pr = _run(d, MODE_TOK, 2, Q0, P0, first=2)
    assert _same(q, qr) and _same(p, pr) and np.isfinite(p).all()
    assert _same(t["mono"], t["jac"][0])
    want = np.array([RT.benettin(t["jac"][:, k]) for k in range(8)])
    assert np.abs(t["lyap"] - want).max() <= LYAP_TOL
