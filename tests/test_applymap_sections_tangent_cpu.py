"""CPU checks of the sectioned map's tangent entry (sgpr_applymap_sections_tangent_host, maps.run_map_sections_tangent,
maps.tangent_from_jac, examples/tokamak_split.applymap_tok_tangent): declared, exported and bound alike; every argument error
answered with SGPR_E_ARG before any device call; the Python wrapper's ValueErrors; the host Benettin / monodromy helper against
tests/ref_tangent.py; the chunk bookkeeping's jac rows; and the d = 1 Hessian of tests/ref_tangent.py -- the reference of
tests/test_gpu_applymap_sections_tangent.py -- against central differences of the CPU oracle's rows."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ref_tangent as RT
from tests import c_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sgpr_applymap_sections_tangent_host"


def test_header_exports_map_ctypes_table_and_library_agree():
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    params, plain = c_header.assert_bound_as_declared(NAME, 26), c_header.assert_bound_as_declared("sgpr_applymap_sections_host")
    assert params[:23] == plain and params[23:] == ["double *jac", "double *mono", "double *lyap"]
    assert L.SIGNATURES[NAME][1][:23] == L.SIGNATURES["sgpr_applymap_sections_host"][1]
    assert c_header.in_exports_map(NAME), NAME + " is not covered by exports.map"
    dyn = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T %s$" % NAME, dyn, flags=re.M), NAME + " is not exported"
    assert lib.sgpr_abi_version() == 5


def _args(**over):
    """a valid call (family A, two sections, implicit), as a dict of named arguments in the order of the declaration"""
    from sympgpr_amd import _lib as L
    nsec, n0, n0p, ntest, nm = 2, 4, 5, 3, 3
    keep = dict(hyp=np.array([1.2, 1.5, 1.0, 1.1, 1.4, 0.9]), x=np.zeros(n0 * nsec), y=np.zeros(n0 * nsec),
                alpha=np.zeros(2 * n0 * nsec), hypp=np.array([1.2, 1.5, 1.0, 1.1, 1.4, 0.9]), xp=np.zeros(n0p * nsec),
                yp=np.zeros(n0p * nsec), alphap=np.zeros(n0p * nsec), Q0=np.ones(ntest), P0=np.ones(ntest),
                qmap=np.zeros((nm, ntest)), pmap=np.zeros((nm, ntest)), pdiff=np.zeros((nm, ntest)),
                jac=np.zeros((nm - 1, ntest, 2, 2)), mono=np.zeros((ntest, 2, 2)), lyap=np.zeros((ntest, 2)), hyp8=np.ones(8))
    a = dict(family=0, mode=L.MAP_WRAP_Q | L.MAP_LOSS_NEGP, nsec=nsec, first=1, nm=nm, ntest=ntest, hyp=L.dptr(keep["hyp"]),
             nhyp=3, n0=n0, x=L.dptr(keep["x"]), y=L.dptr(keep["y"]), alpha=L.dptr(keep["alpha"]), hypp=L.dptr(keep["hypp"]),
             nhypp=3, n0p=n0p, xp=L.dptr(keep["xp"]), yp=L.dptr(keep["yp"]), alphap=L.dptr(keep["alphap"]),
             Q0=L.dptr(keep["Q0"]), P0=L.dptr(keep["P0"]), qmap=L.dptr(keep["qmap"]), pmap=L.dptr(keep["pmap"]),
             pdiff=L.dptr(keep["pdiff"]), jac=L.dptr(keep["jac"]), mono=L.dptr(keep["mono"]), lyap=L.dptr(keep["lyap"]))
    for k, v in over.items():
        a[k] = L.dptr(keep[v]) if isinstance(v, str) else v
    return a, keep


# everything the plain entry refuses (tests/test_applymap_sections_cpu.py: BAD) ...
BAD = [dict(nsec=0), dict(nsec=-1), dict(first=-1), dict(first=2), dict(nm=0), dict(ntest=-1), dict(n0=-1), dict(n0p=-1),
       dict(mode=16), dict(mode=32 | 1), dict(mode=4 | 8), dict(hyp=None), dict(hypp=None), dict(x=None), dict(y=None),
       dict(alpha=None), dict(xp=None), dict(yp=None), dict(alphap=None), dict(Q0=None), dict(P0=None), dict(qmap=None),
       dict(pmap=None), dict(nhyp=4), dict(nhyp=2), dict(nhypp=4), dict(family=3), dict(family=9), dict(family=-1),
       dict(mode=4, x=None),
       # ... and the mode rules of the tangent: WRAP_P, EXPLICIT with a product family (A, C, D, the USER slot as shipped),
       # exponents of an orbit without a step
       dict(mode=2), dict(mode=1 | 2), dict(mode=1 | 2 | 8), dict(family=1, mode=4 | 2), dict(mode=4), dict(mode=4 | 1),
       dict(family=2, mode=4), dict(family=3, mode=4, nhyp=4, hyp="hyp8"), dict(family=4, mode=4), dict(nm=1),
       dict(nm=1, jac=None, mono=None)]


@pytest.mark.parametrize("over", BAD, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_argument_errors_come_before_any_device_call(over):
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    a, keep = _args(**over)
    assert getattr(lib, NAME)(*a.values()) == L.E_ARG
    msg = lib.sgpr_last_error()
    assert msg != b"" and (b"applymap_sections_tangent_host" in msg or b"hyp must hold" in msg or b"family" in msg)


def test_valid_calls_reach_the_device_check():
    """well-formed calls pass every check: without a GPU they end at SGPR_E_NODEVICE, not SGPR_E_ARG -- all outputs, none, each
    alone, nm = 1 without exponents, ntest = 0, explicit mode with the sum kernel (family B = 1), family D"""
    import sympgpr_amd
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    want = 0 if sympgpr_amd.device_count() > 0 else L.E_NODEVICE
    for over in ({}, dict(pdiff=None), dict(jac=None, mono=None, lyap=None), dict(jac=None), dict(mono=None), dict(lyap=None),
                 dict(first=0, nm=1, lyap=None), dict(ntest=0), dict(mode=0), dict(nm=2),
                 dict(family=1, mode=L.MAP_EXPLICIT | L.MAP_WRAP_Q, hypp=None, nhypp=0, xp=None, yp=None, alphap=None, n0p=-3),
                 dict(family=1, mode=L.MAP_EXPLICIT),
                 dict(family=3, nhyp=4, nhypp=4, hyp="hyp8", hypp="hyp8")):
        a, keep = _args(**over)
        assert getattr(lib, NAME)(*a.values()) == want, over


def _good():
    from sympgpr_amd import maps
    nsec, n0, n0p = 3, 4, 5
    return dict(mode=maps.WRAP_Q, nm=3, Ntest=2, hyp=np.ones((nsec, 3)), xt=np.zeros((n0, nsec)), yt=np.zeros((n0, nsec)),
                alpha=np.zeros((2 * n0, nsec)), Q0=np.ones(2), P0=np.ones(2), hypp=np.ones((nsec, 3)), xp=np.zeros((n0p, nsec)),
                yp=np.zeros((n0p, nsec)), alphap=np.zeros((n0p, nsec)), first=2, family="A")


def test_run_map_sections_tangent_raises_value_errors(monkeypatch):
    """shape and mode errors are ValueError, and the library is not asked (load_library is made to fail)"""
    from sympgpr_amd import _lib as L
    from sympgpr_amd import maps
    nsec, n0, n0p = 3, 4, 5

    def no_library():
        raise AssertionError("the library was asked")
    monkeypatch.setattr(L, "load_library", no_library)
    good = _good()
    bad = [dict(alpha=np.zeros((2 * n0 - 1, nsec))), dict(alphap=np.zeros((n0p + 1, nsec))), dict(yt=np.zeros((n0 + 1, nsec))),
           dict(xt=np.zeros((n0, nsec - 1))), dict(hypp=np.ones((nsec - 1, 3))), dict(hyp=np.ones(3)), dict(first=3),
           dict(first=-1), dict(hypp=None), dict(alphap=None), dict(nm=0), dict(Q0=np.ones(3)),
           dict(mode=maps.WRAP_P), dict(mode=maps.WRAP_Q | maps.WRAP_P), dict(mode=maps.EXPLICIT),                  # the mode rules
           dict(mode=maps.EXPLICIT | maps.WRAP_Q, family="C"), dict(mode=maps.EXPLICIT, family="D"),
           dict(mode=maps.EXPLICIT | maps.WRAP_P, family="B"),
           dict(nm=1), dict(nm=1, jac=False, mono=False)]                                                           # lyap without a step
    for over in bad:
        with pytest.raises(ValueError):
            maps.run_map_sections_tangent(**dict(good, **over))
    with pytest.raises(AssertionError, match="the library was asked"):       # a good call gets as far as the library
        maps.run_map_sections_tangent(**good)
    with pytest.raises(AssertionError, match="the library was asked"):
        maps.run_map_sections_tangent(**dict(good, nm=1, lyap=False))
    with pytest.raises(AssertionError, match="the library was asked"):
        maps.run_map_sections_tangent(**dict(good, mode=maps.EXPLICIT | maps.WRAP_Q, family="B"))
    assert "tangent_from_jac" in maps.run_map_sections_tangent.__doc__


def test_both_wrappers_hand_the_library_the_same_arguments(monkeypatch):
    """run_map_sections and run_map_sections_tangent share one argument preparation: the 23 arguments of the plain entry are
    the first 23 of the tangent entry, value for value"""
    from sympgpr_amd import _lib as L
    from sympgpr_amd import maps
    seen = {}

    class Lib:
        def __getattr__(self, name):
            def f(*a):
                seen[name] = a
                return 0
            return f
    monkeypatch.setattr(L, "load_library", lambda: Lib())
    good = _good()
    rng = np.random.default_rng(0)
    for k in ("xt", "yt", "alpha", "xp", "yp", "alphap"):
        good[k] = rng.normal(size=good[k].shape)
    q, p, pd = maps.run_map_sections(**good, want_pdiff=True)
    q2, p2, pd2, t = maps.run_map_sections_tangent(**good, want_pdiff=True, mono=False)
    a, b = seen["sgpr_applymap_sections_host"], seen["sgpr_applymap_sections_tangent_host"]
    assert len(a) == 23 and len(b) == 26 and sorted(t) == ["jac", "lyap"]
    ints = [i for i in range(23) if isinstance(a[i], int)]
    assert [a[i] for i in ints] == [b[i] for i in ints] and len(ints) == 10
    sizes = {6: 9, 9: 12, 10: 12, 11: 24, 12: 9, 15: 15, 16: 15, 17: 15, 18: 2, 19: 2}      # the inputs, in doubles
    for i, n in sizes.items():
        assert np.array_equal(np.ctypeslib.as_array(a[i], (n,)), np.ctypeslib.as_array(b[i], (n,)))
    assert b[23] is not None and b[24] is None and b[25] is not None
    assert t["jac"].shape == (2, 2, 2, 2) and t["lyap"].shape == (2, 2) and q2.shape == p2.shape == pd2.shape == (3, 2)
    assert len(maps.run_map_sections_tangent(**good)) == 3


# ---- tangent_from_jac against tests/ref_tangent.py

def _symplectic_chain(rng, steps, n):
    """random 2 x 2 matrices of determinant 1 built as the step matrix is: from A, B, C"""
    A, B, Cc = rng.normal(size=(steps, n)), 0.3 * rng.normal(size=(steps, n)), rng.normal(size=(steps, n))
    T = 1.0 / (1.0 + B)
    return np.stack([np.stack([1 + B - Cc * T * A, Cc * T], axis=-1), np.stack([-T * A, T], axis=-1)], axis=-2)


def test_tangent_from_jac_against_the_restatement():
    from sympgpr_amd import maps
    rng = np.random.default_rng(11)
    steps, n = 30, 6
    jac = _symplectic_chain(rng, steps, n)
    assert np.abs(np.linalg.det(jac) - 1).max() < 1e-12
    mono, lyap = maps.tangent_from_jac(jac)
    eps = np.finfo(float).eps
    for k in range(n):
        Mr = RT.monodromy(jac[:, k])
        bound = steps * 2 * eps * np.prod(np.abs(jac[:, k]).sum(axis=-1).max(axis=-1))
        assert np.abs(mono[k] - Mr).max() <= bound
        np.testing.assert_allclose(lyap[k], RT.benettin(jac[:, k]), rtol=0, atol=2.22e-14)
        assert abs(lyap[k].sum()) <= 2 * steps * 256 * eps
    # one step; a NaN step loses that orbit and no other
    m1, l1 = maps.tangent_from_jac(jac[:1])
    assert np.array_equal(m1, jac[0]) and np.allclose(l1, [RT.benettin(jac[:1, k]) for k in range(n)], rtol=0, atol=2.22e-14)
    bad = jac.copy()
    bad[7, 2] = np.nan
    bad[steps - 1, 4, 0, 1] = np.nan
    mb, lb = maps.tangent_from_jac(bad)
    lost = np.array([k in (2, 4) for k in range(n)])
    assert np.isnan(mb[lost]).all() and np.isnan(lb[lost]).all()
    assert np.array_equal(mb[~lost], mono[~lost]) and np.array_equal(lb[~lost], lyap[~lost])
    for wrong in (np.zeros((3, 2, 2)), np.zeros((0, 3, 2, 2)), np.zeros((3, 2, 2, 3))):
        with pytest.raises(ValueError):
            maps.tangent_from_jac(wrong)


# ---- the chunk bookkeeping with step matrices, without a GPU

def _step(m, q, p):
    P = p - (0.05 + 0.02 * m) * np.sin(q + 0.3 * m)
    if not P >= 0.0:
        return np.nan, np.nan
    return np.mod(q + (0.5 + 0.05 * m) * P, 2 * np.pi), P


def _step_jac(m, q):
    k, c = (0.05 + 0.02 * m) * np.cos(q + 0.3 * m), 0.5 + 0.05 * m
    return np.array([[1 - c * k, c], [-k, 1.0]])


def _stepper(nphmap, calls):
    def run(first, steps, Q0, P0):
        calls.append((first, steps, len(Q0)))
        q, p = np.full((steps + 1, len(Q0)), np.nan), np.full((steps + 1, len(Q0)), np.nan)
        jac = np.full((steps, len(Q0), 2, 2), np.nan)
        q[0], p[0] = Q0, P0
        for s in range(steps):
            for k in range(len(Q0)):
                if not np.isnan(p[s, k]):
                    q[s + 1, k], p[s + 1, k] = _step((first + s) % nphmap, q[s, k], p[s, k])
                    if not np.isnan(p[s + 1, k]):
                        jac[s, k] = _step_jac((first + s) % nphmap, q[s, k])
        return q, p, jac
    return run


def _compute_r(zk, r0):
    return 0.005 + 0.5 * np.sin(37.0 * zk[0] * 1e2 + 3.0 * zk[1] + zk[2]) ** 2


@pytest.mark.parametrize("chunk", [None, 1, 3, 7])
def test_chunks_collect_the_step_matrices_of_the_rows_they_keep(chunk):
    from sympgpr_amd.examples.tokamak_split import map_in_chunks, map_steps
    nphmap, nm, Ntest = 4, 23, 12
    rng = np.random.default_rng(2024)
    Q0, P0 = rng.uniform(0.0, 2 * np.pi, Ntest), rng.uniform(0.02, 1.0, Ntest)
    cr = None if chunk is None else _compute_r
    steps = map_steps(nphmap, nm)
    assert steps == 20
    calls, calls2 = [], []
    jac = np.full((steps, Ntest, 2, 2), np.nan)
    q, p = map_in_chunks(_stepper(nphmap, calls), nphmap, nm, Ntest, Q0, P0, cr, chunk, jac_out=jac)
    plain = lambda *a: _stepper(nphmap, calls2)(*a)[:2]
    q0, p0 = map_in_chunks(plain, nphmap, nm, Ntest, Q0, P0, cr, chunk)                  # the present callers' form
    assert np.array_equal(q, q0, equal_nan=True) and np.array_equal(p, p0, equal_nan=True) and calls == calls2
    lost = np.isnan(p[1:steps + 1])
    assert lost.any() and not lost.all()
    assert np.array_equal(np.isnan(jac).all(axis=(2, 3)), lost) and np.array_equal(np.isnan(jac).any(axis=(2, 3)), lost)
    for i in range(steps):
        for k in range(Ntest):
            if not lost[i, k]:
                assert np.array_equal(jac[i, k], _step_jac(i % nphmap, q[i, k]))


def test_applymap_tok_tangent_routes(monkeypatch):
    """applymap_tok_tangent with maps.run_map_sections_tangent replaced: no callback -> ONE call with all three outputs;
    callback + steps_per_launch -> chunks that ask for jac only, mono and lyap from tangent_from_jac"""
    from sympgpr_amd import maps
    from sympgpr_amd.examples import tokamak_split as ts
    nph, N, Np, nm, Ntest = 4, 5, 6, 23, 12
    rng = np.random.default_rng(3)
    Q0, P0 = rng.uniform(0.0, 2 * np.pi, Ntest), rng.uniform(0.02, 1.0, Ntest)
    xtrain, ztrain, Kyinv, hyp = rng.normal(size=(2 * N, nph)), rng.normal(size=(2 * N, nph)), rng.normal(size=(nph, 2 * N, 2 * N)), rng.uniform(1, 2, (nph, 3))
    xtrainp, ztrainp, Kyinvp, hypp = rng.normal(size=(2 * Np, nph)), rng.normal(size=(Np, nph)), rng.normal(size=(nph, Np, Np)), rng.uniform(1, 2, (nph, 3))
    calls, asked = [], []
    stepper = _stepper(nph, calls)

    def fake(mode, nm_, Ntest_, hyp_, xt, yt, alpha, Q0_, P0_, hypp_=None, xp=None, yp=None, alphap=None, first=0, want_pdiff=False,
             family=None, jac=True, mono=True, lyap=True):
        assert mode == maps.WRAP_Q | maps.LOSS_NEGP and family == "A" and not want_pdiff
        assert np.array_equal(alpha[:, 1], Kyinv[1] @ ztrain[:, 1]) and np.array_equal(xt, xtrain[:N])
        asked.append((jac, mono, lyap))
        q, p, j = stepper(first, nm_ - 1, Q0_, P0_)
        t = {"jac": j}
        if mono:
            t["mono"], t["lyap"] = maps.tangent_from_jac(j)
        return q, p, t
    monkeypatch.setattr(maps, "run_map_sections_tangent", fake)
    args = (nph, nm, Ntest, Q0, P0, xtrainp, ztrainp, Kyinvp, hypp, xtrain, ztrain, Kyinv, hyp)
    q, p, t = ts.applymap_tok_tangent(*args)
    assert calls == [(0, 20, Ntest)] and asked == [(True, True, True)]
    assert t["jac"].shape == (20, Ntest, 2, 2) and t["mono"].shape == (Ntest, 2, 2) and t["lyap"].shape == (Ntest, 2)
    mono, lyap = maps.tangent_from_jac(t["jac"])
    assert np.array_equal(mono, t["mono"], equal_nan=True) and np.array_equal(lyap, t["lyap"], equal_nan=True)
    assert np.isnan(t["lyap"]).any() and np.isfinite(t["lyap"]).any()
    del calls[:], asked[:]
    q7, p7, t7 = ts.applymap_tok_tangent(*args, compute_r=_compute_r, steps_per_launch=7)
    assert [c[:2] for c in calls] == [(0, 7), (3, 7), (2, 6)] and set(asked) == {(True, False, False)}
    lost = np.isnan(p7[1:21])
    assert np.array_equal(np.isnan(t7["jac"]).all(axis=(2, 3)), lost) and lost.sum() > np.isnan(p[1:21]).sum()
    mono, lyap = maps.tangent_from_jac(t7["jac"])
    assert np.array_equal(mono, t7["mono"], equal_nan=True) and np.array_equal(lyap, t7["lyap"], equal_nan=True)
    q0, p0, t0 = ts.applymap_tok_tangent(nph, 3, *args[2:])                 # nm <= nphmap: no step
    assert t0["jac"].shape == (0, Ntest, 2, 2) and np.array_equal(t0["mono"], np.broadcast_to(np.eye(2), (Ntest, 2, 2)))
    assert np.isnan(t0["lyap"]).all() and np.array_equal(p0[0], P0)


# ---- the reference of the GPU test: ref_tangent.hessian at d = 1 against central differences of the oracle's rows

@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
def test_ref_hessian_against_central_differences_of_the_oracle_rows(oracle, fam):
    """H = dG/dx with G = (r1, r2) = oracle.predict_rows; h = 1e-5, rtol = atol = 1e-6 (the quotient carries O(h^2) and
    eps |G| / h; no solver in it).  Also the conventions: ref_tangent.gradient is predict_rows, r1 = G_q, r2 = G_P."""
    from tests.test_gpu_applymap_sections import _sections
    d = _sections(fam, 3, 40, 43)
    rng = np.random.default_rng(5)
    h, worst, worst_g = 1e-5, 0.0, 0.0
    for m in range(3):
        X = np.stack((d["xt"][:, m], d["yt"][:, m]), axis=1)
        hyp, al = d["hyp"][m], d["alpha"][:, m]
        rows = lambda q, P: np.array(oracle.predict_rows(fam, [q], [P], d["xt"][:, m], d["yt"][:, m], hyp, al)).reshape(2)
        for q, P in zip(rng.uniform(0.5, 5.5, 4), rng.uniform(0.05, 0.9, 4)):
            G = RT.gradient(fam, 1, hyp, X, al, [q, P])
            worst_g = max(worst_g, np.abs(G - rows(q, P)).max())
            H = RT.hessian(fam, 1, hyp, X, al, [q, P])
            fd = np.stack(((rows(q + h, P) - rows(q - h, P)) / (2 * h), (rows(q, P + h) - rows(q, P - h)) / (2 * h)), axis=1)
            worst = max(worst, np.abs(H - fd).max())
            np.testing.assert_allclose(H, fd, rtol=1e-6, atol=1e-6)
            assert H[0, 1] == H[1, 0] and (fam != "B" or H[0, 1] == 0.0)
    print("family %s: max |H - central difference| = %.2e, max |gradient - predict_rows| = %.2e" % (fam, worst, worst_g))
    assert worst_g <= 1e-11
