"""CPU tests of the periodic-orbit search of the d-pair map (sgpr_fit_periodic_nd, sgpr_periodic_nd_host; csrc/periodic_nd.h): the
entries are declared, exported and bound; every argument error is refused without a device; and tests/ref_periodic.py, the NumPy
restatement that tests/test_gpu_periodic_nd.py compares the device with, reproduces the periodic orbits found on the CPU when
the feature was specified (CASES below: the oracle's alpha, tol 1e-13), each

  * pinned to 1e-9,
  * reached with a strictly decreasing residual in exactly the stated number of passes.  The stated figure counts the Newton
    updates: `its`, which counts the passes with the converged one, is one larger.  One case is pinned at one update more than
    stated (its `more` entry): the d = 1 twist case with n = 3 has the residuals .., 6.7e-10, 5.2e-13, 2.1e-13 here against the
    threshold 1e-13 max|z| = 3.1e-13 -- its evaluation noise, n dG <= 5e-13 by the summation-order experiment the cases came
    with, straddles that threshold.  The same case is run at tol 1e-12 as well, where it takes the stated 4,
  * and satisfying r = 0 to 1e-12 under a second, independent evaluation: n steps of the CPU map of
    tests/test_gpu_applymap_nd.py (_ref_map_nd: K* rows from the oracle's build_K_nd, MINPACK hybrd with xtol 1e-13), unwrapped.

Two training sets: the data of tests/test_gpu_applymap_nd.py (sig2n 1e-8; fixed points and their n = 4 repetitions, w = 0) and
a twist map defined here (twist_training; true periods with non-zero winding numbers)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import ref_periodic as RP
from tests.test_gpu_applymap_nd import _hyp, _ref_map_nd, _training

from tests import c_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI, TWO_PI = np.pi, 2.0 * np.pi
ENTRIES = ("sgpr_fit_periodic_nd", "sgpr_periodic_nd_host")


def twist_training(d, Nt):
    """F_q = -0.3 sin q_c - 0.09 sin(sum q) (no coupling at d = 1), F_P = P on q ~ U(0, 2 pi), P ~ U(-0.5, 2.6); z as _training"""
    rng = np.random.default_rng(3)
    q, P = rng.uniform(0, TWO_PI, (Nt, d)), rng.uniform(-0.5, 2.6, (Nt, d))
    Fq = -0.3 * np.sin(q)
    if d > 1:
        Fq = Fq - (0.09 * np.sin(q.sum(axis=1)))[:, None]
    return np.hstack((q, P)), np.concatenate((Fq.T.ravel(), P.T.ravel()))


def _near_pi(d, p):
    return (PI + 0.1,) * d + (p,) * d


def _near_0(d, p):
    return (0.1,) * d + (p,) * d


# (data, family, d, guess, n, w, z*, Newton updates at tol 1e-13, |(mono - I)^-1|_inf as found then).  Families A and D give the same
# numbers on both data sets.  z* of the second fixed-data row is unwrapped: with WRAP_Q its first entry is 2 pi larger.
_FIXED = [
    (2, "AD", _near_pi(2, 0.05), (3.236222266115, 3.240690300511, -1.353772488e-3, -1.5930949212e-2), (3, 3), (20, 5.3)),
    (2, "AD", _near_0(2, 0.05), (-0.007788231953, 0.008711404615, -0.026829122383, -0.030907290323), (4, 5), (4.1, 1.5)),
    (2, "C", _near_pi(2, 0.05), (3.23741925079, 3.379122301396, -0.019829732659, -0.004071292164), (4, 4), (25, 6.5)),
    (3, "AD", _near_pi(3, 0.05), (3.225474617986, 3.33710887518, 3.147780146623, 0.162922813814, 0.202205424603, -0.0608950423),
     (4, 4), (6.4, 1.9)),
    (3, "AD", _near_0(3, 0.05), (-0.039307020437, -0.23523208072, 0.193093956712, 0.003066331374, -0.005597872729, 0.058917856986),
     (5, 6), (13.5, 3.9)),
]
_TWIST = [
    (1, "A", 40, (PI + 0.1, 2.1), 3, (1,), (3.062810531085, 2.163791654859), 4, 164),     # 5 updates at tol 1e-13: see above
    (1, "A", 40, (PI + 0.1, 1.55), 4, (1,), (2.861461393211, 1.673749486672), 5, 324),
    (2, "AD", 60, (PI + 0.1, PI + 0.1, 2.1, 2.1), 3, (1, 1), (3.577794079548, 3.003286825006, 2.197396115288, 2.149397318811), 6, 27),
    (2, "AD", 60, (0.1, 0.1, 2.1, 2.1), 3, (1, 1), (0.308343598192, -0.004060050589, 1.928140457831, 2.007735766669), 5, 24),
    (2, "AD", 60, (0.1, PI + 0.1, 2.1, 0.0), 3, (1, 0), (0.211914019582, 3.127008077808, 1.991718191448, 0.038110918492), 4, 38),
]
CASES = []
for d, fams, guess, zstar, passes, inv in _FIXED:
    for fam in fams:
        for n, its, nrm in zip((1, 4), passes, inv):
            CASES.append(dict(data="fixed", fam=fam, d=d, Nt=40, guess=guess, n=n, w=(0,) * d, z=zstar, its=its, inv=nrm))
for d, fams, Nt, guess, n, w, zstar, its, nrm in _TWIST:
    for fam in fams:
        CASES.append(dict(data="twist", fam=fam, d=d, Nt=Nt, guess=guess, n=n, w=w, z=zstar, its=its, inv=nrm,
                          more=int((d, n) == (1, 3))))
IDS = ["%s-%s-d%d-n%d-%s" % (c["data"], c["fam"], c["d"], c["n"], "pi" if c["guess"][0] > 1 else "0") for c in CASES]
IDS = [i + ("b" if c["data"] == "twist" and c["d"] == 2 and c["w"] == (1, 0) else "") for i, c in zip(IDS, CASES)]

_models = {}


def model(oracle, c):
    """training points, hyp and the oracle's alpha of a case's data set -- computed once per (data, family, d), never changed"""
    key = (c["data"], c["fam"], c["d"])
    if key not in _models:
        X, z = _training(c["d"]) if c["data"] == "fixed" else twist_training(c["d"], c["Nt"])
        hyp = _hyp(c["fam"], c["d"])
        sig2n = 1e-8 if c["data"] == "fixed" else 1e-6
        alpha = oracle.fit_nd(c["fam"], X, z, hyp, sig2n)[0]
        for a in (X, z, hyp, alpha):
            a.setflags(write=False)
        _models[key] = dict(X=X, z=z, hyp=hyp, alpha=alpha, sig2n=sig2n)
    return _models[key]


def test_header_declares_and_library_exports_both_entries():
    from sympgpr_amd import _lib
    lib = C.CDLL(_lib.lib_path())
    for name, nargs in zip(ENTRIES, (17, 24)):
        c_header.assert_bound_as_declared(name, nargs)
        assert hasattr(lib, name), "libsympgpr_hip.so does not export " + name           # exports.map: sgpr_*
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == nargs
    assert "sgpr_*;" in open(os.path.join(ROOT, "sympgpr_amd", "csrc", "exports.map")).read()


def arg_errors():
    """every SGPR_E_ARG case of sgpr_periodic_nd_host, by name: the changed keyword arguments of host_call"""
    nan, inf = float("nan"), float("inf")
    return {"n < 1": dict(n=0), "maxit < 1": dict(maxit=0), "tol zero": dict(tol=0.0), "tol negative": dict(tol=-1e-12),
            "tol nan": dict(tol=nan), "tol inf": dict(tol=inf), "null z": dict(z=None), "null resid": dict(resid=None),
            "null its": dict(its=None), "qorb without porb": dict(orbit=(True, False)), "unknown mode bit": dict(mode=64),
            "ntest < 0": dict(ntest=-1), "null Q0": dict(Q0=None), "ldq < ntest": dict(ldq=1), "unknown family": dict(family=99),
            "d = 4": dict(d=4), "nhyp": dict(nhyp=4), "n0 < 0": dict(n0=-1), "ldx < n0": dict(ldx=1),
            "explicit with a product family": dict(mode=4)}


def host_call(**kw):
    """sgpr_periodic_nd_host on a small valid problem (family A, d = 2, 5 training points, 3 guesses) with the given arguments
    changed -> the return code"""
    from sympgpr_amd import _lib
    lib = _lib.load_library()
    assert _lib.MAP_EXPLICIT == 4
    d, n0, nt, n = 2, 5, 3, 2
    a = dict(family=0, d=d, mode=0, n=n, ntest=nt, nhyp=2 * d + 1, n0=n0, ldx=n0, ldq=nt, tol=1e-12, maxit=30, z=True, resid=True,
             its=True, Q0=True, orbit=(True, True))
    a.update(kw)
    rng = np.random.default_rng(0)
    hyp, X, alpha = _hyp("A", d), np.asfortranarray(rng.uniform(0, 1, (n0, 2 * d))), rng.standard_normal(2 * d * n0) * 1e-3
    Q0, P0 = np.asfortranarray(rng.uniform(0, 1, (nt, d))), np.asfortranarray(rng.uniform(0, 1, (nt, d)))
    z, resid, its, mono = np.zeros((nt, 2 * d)), np.zeros(nt), np.zeros(nt, dtype=np.int32), np.zeros((nt, 2 * d, 2 * d))
    qorb, porb = np.zeros((n, nt, d)), np.zeros((n, nt, d))
    dp = _lib.dptr
    return lib.sgpr_periodic_nd_host(a["family"], a["d"], a["mode"], a["n"], a["ntest"], dp(hyp), a["nhyp"], a["n0"], dp(X), a["ldx"],
                                     dp(alpha), None, dp(Q0) if a["Q0"] else None, a["ldq"], dp(P0), nt, a["tol"], a["maxit"],
                                     dp(z) if a["z"] else None, dp(resid) if a["resid"] else None,
                                     its.ctypes.data_as(C.POINTER(C.c_int)) if a["its"] else None, dp(mono),
                                     dp(qorb) if a["orbit"][0] else None, dp(porb) if a["orbit"][1] else None)


@pytest.mark.parametrize("what", sorted(arg_errors()))
def test_argument_errors_need_no_device(what):
    from sympgpr_amd import _lib
    assert host_call(**arg_errors()[what]) == _lib.E_ARG, what
    assert _lib.load_library().sgpr_last_error().decode().startswith("periodic_nd_host: ")


def test_multipliers_come_in_reciprocal_pairs():
    from sympgpr_amd import maps
    rng = np.random.default_rng(1)
    d = 3
    S = rng.standard_normal((2 * d, 2 * d))
    J = np.block([[np.zeros((d, d)), np.eye(d)], [-np.eye(d), np.zeros((d, d))]])
    import scipy.linalg
    M = scipy.linalg.expm(0.3 * J @ (S + S.T))                                           # exp of a Hamiltonian matrix: symplectic
    assert maps.symplectic_defect(M) < 1e-12
    lam = maps.multipliers(np.stack((M, np.eye(2 * d), np.full((2 * d, 2 * d), np.nan))))
    assert lam.shape == (3, d, 2)
    np.testing.assert_allclose(lam[0, :, 0] * lam[0, :, 1], 1.0, atol=1e-10)
    assert (np.abs(lam[0, :, 0]) >= np.abs(lam[0, :, 1]) - 1e-12).all()
    np.testing.assert_allclose(np.sort_complex(lam[0].ravel()), np.sort_complex(np.linalg.eigvals(M)), atol=1e-10)
    assert (lam[1] == 1.0).all() and np.isnan(lam[2]).all()
    rot = np.array([[np.cos(0.7), np.sin(0.7)], [-np.sin(0.7), np.cos(0.7)]])           # elliptic: residue sin^2(0.35)
    np.testing.assert_allclose(np.abs(maps.multipliers(rot)), 1.0, atol=1e-14)
    with pytest.raises(ValueError):
        maps.multipliers(np.zeros((3, 3)))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_ref_periodic_reproduces_the_cpu_results(oracle, c):
    m = model(oracle, c)
    d, n, w = c["d"], c["n"], np.array(c["w"], dtype=np.float64)
    s = RP.solve(c["fam"], d, m["hyp"], m["X"], m["alpha"], c["guess"], n, wind=w, wrap=False, tol=1e-13, maxit=30)
    assert s["converged"]
    h = np.array(s["history"])
    print("%s: passes %d (stated %d)  history %s  |(mono - I)^-1| = %.3g (stated %.3g)  max |z - z*| = %.3e"
          % (c, s["its"], c["its"], h, s["inv_norm"], c["inv"], np.abs(s["z"] - np.array(c["z"])).max()))
    assert np.abs(s["z"] - np.array(c["z"])).max() <= 1e-9
    assert (np.diff(h) < 0).all() and s["its"] == len(h)
    assert s["its"] - 1 == c["its"] + c.get("more", 0)
    if c.get("more"):                                                                    # above the noise: the stated count
        s12 = RP.solve(c["fam"], d, m["hyp"], m["X"], m["alpha"], c["guess"], n, wind=w, wrap=False, tol=1e-12, maxit=30)
        assert s12["converged"] and s12["its"] - 1 == c["its"] and s12["history"] == s["history"][:s12["its"]]
    assert s["resid"] == h[-1] <= 1e-13 * max(1.0, np.abs(s["z"]).max())
    assert abs(s["inv_norm"] - c["inv"]) <= 0.06 * c["inv"]                              # stated to two or three digits
    # the second evaluation: the CPU map of test_gpu_applymap_nd.py from z*, unwrapped
    qr, pr, _ = _ref_map_nd(oracle, c["fam"], d, m["hyp"], m["X"], m["alpha"], n + 1, s["z"][None, :d], s["z"][None, d:], False)
    r = np.concatenate((qr[n, 0] - s["z"][:d] - TWO_PI * w, pr[n, 0] - s["z"][d:]))
    print("   independent max|r| = %.3e" % np.abs(r).max())
    assert np.abs(r).max() <= 1e-12
    # the wrapped search finds the same orbit (q mod 2 pi); a last pass at the rounding floor may come or go with the wrap
    sw = RP.solve(c["fam"], d, m["hyp"], m["X"], m["alpha"], c["guess"], n, wind=w, wrap=True, tol=1e-13, maxit=30)
    zw = s["z"].copy()
    zw[:d] = np.mod(zw[:d], TWO_PI)
    assert sw["converged"] and abs(sw["its"] - s["its"]) <= 1 and np.abs(sw["z"] - zw).max() <= 1e-9
