"""CPU checks of the tangent entries of the d-pair map (sgpr_fit_applymap_nd_tangent, sgpr_applymap_nd_tangent_host): declared,
exported and bound alike; every argument error answered with SGPR_E_ARG before any device call; the host helpers of maps.py;
and the NumPy restatement tests/ref_tangent.py -- the CPU reference of tests/test_gpu_applymap_tangent.py -- held against
sympy's own derivatives of the kernels tools/gen_kernels.py defines and against central differences of a CPU step."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ref_tangent as RT
from tests import c_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ip = C.POINTER(C.c_int)
NAMES = (("sgpr_fit_applymap_nd_tangent", 14), ("sgpr_applymap_nd_tangent_host", 21))


def test_header_exports_map_ctypes_table_and_library_agree():
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    dyn = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True, check=True).stdout
    for name, nargs in NAMES:
        c_header.assert_bound_as_declared(name, nargs)
        assert c_header.in_exports_map(name), name + " is not covered by exports.map"
        assert re.search(r" T %s$" % name, dyn, flags=re.M), name + " is not exported"
    assert lib.sgpr_abi_version() == 5


def _host_args(**over):
    """a valid sgpr_applymap_nd_tangent_host call (family A, d = 2), as a dict of named arguments"""
    from sympgpr_amd import _lib as L
    d, n0, ntest, nm = 2, 4, 3, 2
    D = 2 * d
    keep = dict(hyp=np.array([1.2, 1.2, 1.5, 1.5, 1.0]), X=np.zeros((n0, D), order="F"), alpha=np.zeros(D * n0),
                Q0=np.zeros((ntest, d), order="F"), P0=np.zeros((ntest, d), order="F"), qmap=np.zeros((nm, ntest, d)),
                pmap=np.zeros((nm, ntest, d)), iters=np.zeros((nm - 1, ntest), dtype=np.int32),
                jac=np.zeros((nm - 1, ntest, D, D)), mono=np.zeros((ntest, D, D)), lyap=np.zeros((ntest, D)), hyp7=np.ones(7))
    a = dict(family=0, d=d, mode=L.MAP_WRAP_Q, nm=nm, ntest=ntest, hyp=L.dptr(keep["hyp"]), nhyp=5, n0=n0, X=L.dptr(keep["X"]),
             ldx=n0, alpha=L.dptr(keep["alpha"]), Q0=L.dptr(keep["Q0"]), ldq=ntest, P0=L.dptr(keep["P0"]), ldp=ntest,
             qmap=L.dptr(keep["qmap"]), pmap=L.dptr(keep["pmap"]), iters=keep["iters"].ctypes.data_as(_ip),
             jac=L.dptr(keep["jac"]), mono=L.dptr(keep["mono"]), lyap=L.dptr(keep["lyap"]))
    for k, v in over.items():
        a[k] = L.dptr(keep[v]) if isinstance(v, str) else v
    return a, keep


# everything the plain entry refuses (tests/test_applymap_nd_cpu.py: HOST_BAD), explicit mode with the product families, and
# exponents of an orbit without a step
HOST_BAD = [dict(family=9), dict(family=-1), dict(d=0), dict(d=4), dict(mode=2), dict(mode=8), dict(mode=16), dict(nm=0),
            dict(ntest=-1), dict(hyp=None), dict(nhyp=4), dict(nhyp=7), dict(family=3, nhyp=5), dict(n0=-1), dict(X=None),
            dict(alpha=None), dict(ldx=3), dict(Q0=None), dict(P0=None), dict(ldq=2), dict(ldp=2), dict(qmap=None),
            dict(pmap=None), dict(mode=4), dict(mode=5), dict(family=2, mode=4), dict(family=3, nhyp=7, hyp="hyp7", mode=4),
            dict(nm=1)]


@pytest.mark.parametrize("over", HOST_BAD, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_host_entry_argument_errors_come_before_any_device_call(over):
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    a, keep = _host_args(**over)
    assert lib.sgpr_applymap_nd_tangent_host(*a.values()) == L.E_ARG
    assert b"applymap_nd_tangent_host" in lib.sgpr_last_error()


def test_host_entry_valid_calls_reach_the_device_check():
    """calls that pass every check end at SGPR_E_NODEVICE without a GPU, not at SGPR_E_ARG: all outputs, none of them, nm = 1
    without exponents, explicit mode with the sum kernel (family B = 1; the USER slot as shipped is a product kernel)"""
    import sympgpr_amd
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    for over in ({}, dict(jac=None, mono=None, lyap=None), dict(iters=None), dict(nm=1, lyap=None), dict(family=1, mode=4),
                 dict(family=1, mode=5), dict(family=3, nhyp=7, hyp="hyp7")):
        a, keep = _host_args(**over)
        rc = lib.sgpr_applymap_nd_tangent_host(*a.values())
        assert rc == (0 if sympgpr_amd.device_count() > 0 else L.E_NODEVICE), over


def test_handle_entry_argument_errors_come_before_any_device_call():
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    fn = lib.sgpr_fit_applymap_nd_tangent
    ntest, nm, d = 3, 2, 2
    Q0, P0 = np.zeros((ntest, d), order="F"), np.zeros((ntest, d), order="F")
    q, p = np.zeros((nm, ntest, d)), np.zeros((nm, ntest, d))
    good = dict(f=None, mode=0, nm=nm, ntest=ntest, Q0=L.dptr(Q0), ldq=ntest, P0=L.dptr(P0), ldp=ntest, qmap=L.dptr(q),
                pmap=L.dptr(p), iters=None, jac=None, mono=None, lyap=None)
    assert fn(*good.values()) == L.E_ARG                    # null handle
    assert b"fit_applymap_nd_tangent" in lib.sgpr_last_error()
    for over in (dict(mode=2), dict(nm=0), dict(Q0=None), dict(ldq=2)):      # ... whatever else is wrong with the call
        assert fn(*dict(good, **over).values()) == L.E_ARG


def test_python_wrappers_validate_before_the_library_is_asked():
    from sympgpr_amd import maps
    from sympgpr_amd.fit import SympFit
    assert callable(SympFit.applymap_pairs_tangent) and "bit for bit" in SympFit.applymap_pairs_tangent.__doc__
    hyp, X, alpha = [1.2, 1.2, 1.5, 1.5, 1.0], np.zeros((4, 4)), np.zeros(16)
    Q0, P0 = np.zeros((3, 2)), np.zeros((3, 2))
    bad = [dict(d=4, X=np.zeros((4, 8)), alpha=np.zeros(32)), dict(X=np.zeros((4, 6))), dict(alpha=np.zeros(15)),
           dict(Q0=np.zeros(3)), dict(P0=np.zeros((2, 2))), dict(mode=maps.WRAP_P), dict(nm=0), dict(nm=1)]
    for over in bad:
        a = dict(family="A", d=2, mode=maps.WRAP_Q, nm=3, hyp=hyp, X=X, alpha=alpha, Q0=Q0, P0=P0)
        a.update(over)
        with pytest.raises(ValueError):
            maps.run_map_nd_tangent(**a)
    out = maps.tangent_outputs_nd(4, 3, 2)
    assert out["jac"].shape == (3, 3, 4, 4) and out["mono"].shape == (3, 4, 4) and out["lyap"].shape == (3, 4)
    assert sorted(maps.tangent_outputs_nd(1, 3, 2, lyap=False)) == ["jac", "mono"]
    assert maps.tangent_outputs_nd(4, 3, 2, jac=False, mono=False, lyap=False) == {}


def test_symplectic_defect_and_greene_residue_on_hand_made_matrices():
    from sympgpr_amd import maps
    t = 0.7
    rot = np.array([[np.cos(t), np.sin(t)], [-np.sin(t), np.cos(t)]])
    shear = np.array([[1.0, 0.0], [3.0, 1.0]])
    assert maps.symplectic_defect(rot) <= 4e-16 and maps.symplectic_defect(shear) == 0.0
    assert maps.symplectic_defect(np.diag([2.0, 1.0])) == 1.0               # M^T J M = 2 J
    # D = 4: a rotation in each plane (q_i, p_i) in the order (q_1, q_2, p_1, p_2), a symmetric shear, a non-symplectic swap
    c, s = np.cos(t), np.sin(t)
    R4 = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1.0]])
    S4 = np.eye(4)
    S4[2:, :2] = [[1.0, 0.5], [0.5, -2.0]]
    swap = np.eye(4)[[1, 0, 2, 3]]
    d4 = maps.symplectic_defect(np.stack((R4, S4, R4 @ S4, swap)))
    assert d4.shape == (4,) and (d4[:3] <= 1e-15).all() and d4[3] == 1.0
    S4[2, 1] = 0.25                                                          # the shear's block no longer symmetric
    assert abs(maps.symplectic_defect(S4) - 0.25) <= 1e-16
    assert abs(maps.greene_residue(rot) - (2 - 2 * np.cos(t)) / 4) <= 1e-16     # elliptic: 0 < R < 1
    assert maps.greene_residue(shear) == 0.0                                      # parabolic
    assert maps.greene_residue(np.diag([2.0, 0.5])) == -0.125                     # hyperbolic
    assert maps.greene_residue(np.stack((rot, shear))).shape == (2,)
    for bad in (np.eye(4), np.zeros((2, 3)), np.zeros(4)):
        with pytest.raises(ValueError):
            maps.greene_residue(bad)
    with pytest.raises(ValueError):
        maps.symplectic_defect(np.eye(3))


# ---- tests/ref_tangent.py against sympy ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_kernels", os.path.join(ROOT, "tools", "gen_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _problem(fam, d=2, n0=7, seed=3):
    rng = np.random.default_rng(seed)
    X = np.hstack((rng.uniform(0, 2 * np.pi, (n0, d)), rng.uniform(-1, 1, (n0, d))))
    alpha = rng.standard_normal(2 * d * n0) * 0.2
    hyp = np.array([1.1, 0.9][:d] + [1.4, 1.7][:d] + ([0.45, 0.6][:d] if fam == "D" else []) + [1.3])
    x = np.concatenate((rng.uniform(0.5, 5.5, d), rng.uniform(-0.6, 0.6, d)))
    return X, alpha, hyp, x


@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
def test_restated_gradient_and_hessian_against_sympys_derivatives(gen, fam):
    """d = 2: k(u, v) built from the generator's own factor definitions; G_c(x) = sum_j sum_b d2k/du_c dv_b (x, X_j) alpha_bj and
    H_ce = sum_j sum_b d3k/du_c du_e dv_b alpha_bj by sympy.diff and lambdify.  Bound: the sums have 4 n0 = 28 terms of size up
    to max |alpha| max |d3k| ~ 10, each evaluated to a few ulp by either side: 1e-12 leaves a factor 100."""
    import sympy as sp
    d, D = 2, 4
    _, fq, fP, mode = gen.families()[fam]
    u, v = sp.symbols("u0:4", real=True), sp.symbols("v0:4", real=True)
    ls, ps = sp.symbols("l0:4", positive=True), sp.symbols("p0:2", positive=True)
    facs = [fq.subs({gen.x_a: v[m], gen.x_b: u[m], gen.lx: ls[m], gen.p: ps[m]}, simultaneous=True) for m in range(d)] + \
           [fP.subs({gen.y_a: v[d + m], gen.y_b: u[d + m], gen.ly: ls[d + m]}, simultaneous=True) for m in range(d)]
    k = sp.Mul(*facs) if mode == "prod" else sp.Add(*facs)
    X, alpha, hyp, x = _problem(fam)
    n0 = X.shape[0]
    al = alpha.reshape(D, n0)
    pv = hyp[D:D + d] if fam == "D" else np.ones(d)
    sig = hyp[-1]

    def total(expr, b):
        f = sp.lambdify(u + v + ls + ps, expr, "numpy")
        return sig * float(np.sum(np.broadcast_to(f(*x, *X.T, *hyp[:D], *pv), (n0,)) * al[b]))

    G = np.array([sum(total(sp.diff(k, u[c], v[b]), b) for b in range(D)) for c in range(D)])
    H = np.array([[sum(total(sp.diff(k, u[c], u[e], v[b]), b) for b in range(D)) for e in range(D)] for c in range(D)])
    Gr, Hr = RT.gradient(fam, d, hyp, X, alpha, x), RT.hessian(fam, d, hyp, X, alpha, x)
    print("family %s: max |dG| = %.3e  max |dH| = %.3e  (max |H| = %.3g)" % (fam, np.abs(G - Gr).max(), np.abs(H - Hr).max(), np.abs(H).max()))
    assert np.abs(H).max() > 1e-3 and np.array_equal(Hr, Hr.T)
    np.testing.assert_allclose(Gr, G, rtol=0, atol=1e-12)
    np.testing.assert_allclose(Hr, H, rtol=0, atol=1e-12)


@pytest.mark.parametrize("fam", ["A", "B", "C", "D", "USER"])
def test_kernels_hand_form_of_the_third_derivative_is_the_generated_one(gen, fam):
    """csrc/maptan.h takes th = f'''/f of the hand-written families from g = f'/f and nh = -f''/f:
    th = -g (4 hs^2 + 3 nh + 2 g^2) for the periodic factors (hs = 1/2, or p), -g (3 nh + 2 g^2) for the squared exponential.
    gen::factor3 is printed from diff(f, dx, 3) / f: the two agree as expressions, for every factor of every family."""
    import sympy as sp
    _, fq, fP, _ = gen.families()[fam]
    dx, l = sp.Symbol("dx", real=True), sp.Symbol("l", positive=True)
    for f, lsym, a, b in ((fq, gen.lx, gen.x_a, gen.x_b), (fP, gen.ly, gen.y_a, gen.y_b)):
        fd = f.subs({a: dx, b: 0, lsym: l})
        g, nh, th = sp.diff(fd, dx) / fd, -sp.diff(fd, dx, 2) / fd, sp.diff(fd, dx, 3) / fd
        periodic = fd.has(sp.sin)
        hs = (gen.p if gen.p in fd.free_symbols else sp.Rational(1, 2)) if periodic else 0
        assert sp.simplify(th + g * (4 * hs ** 2 + 3 * nh + 2 * g ** 2)) == 0


@pytest.mark.parametrize("fam,explicit", [("A", False), ("C", False), ("D", False), ("B", False), ("B", True)])
def test_restated_step_matrix_against_central_differences_of_a_cpu_step(fam, explicit):
    """one step (q, p) -> (Q, P) with ref_tangent.gradient and MINPACK hybrd (xtol 1e-13), differentiated by central differences
    with h = 1e-5: the quotient carries at most 1e-13 / 1e-5 = 1e-8 of solver noise plus O(h^2) truncation; rtol = atol = 1e-6
    covers both with a factor 100.  And M is symplectic to rounding, det M = 1."""
    import scipy.optimize
    from sympgpr_amd import maps
    d, D = 2, 4
    X, alpha, hyp, x = _problem(fam, n0=9, seed=8)

    def step(z):
        q, p = z[:d], z[d:]
        G = lambda P: RT.gradient(fam, d, hyp, X, alpha, np.concatenate((q, P)))
        if explicit:
            P = p - G(p)[:d]
        else:
            P, _, ier, msg = scipy.optimize.fsolve(lambda P: G(P)[:d] - p + P, p, xtol=1e-13, full_output=True)
            assert ier == 1, msg
        return np.concatenate((q + G(P)[d:], P))

    z1 = step(x)
    M, K = RT.step_matrix(RT.hessian(fam, d, hyp, X, alpha, np.concatenate((x[:d], z1[d:]))), d)
    h = 1e-5
    fd = np.column_stack([(step(x + h * e) - step(x - h * e)) / (2 * h) for e in np.eye(D)])
    print("family %s%s: max |M - fd| = %.3e  defect = %.3e  det - 1 = %.3e" %
          (fam, " explicit" if explicit else "", np.abs(M - fd).max(), maps.symplectic_defect(M), np.linalg.det(M) - 1))
    assert np.abs(M - np.eye(D)).max() > 1e-2
    np.testing.assert_allclose(M, fd, rtol=1e-6, atol=1e-6)
    assert maps.symplectic_defect(M) <= 256 * np.finfo(float).eps * np.linalg.cond(K, np.inf) * max(1.0, np.linalg.norm(M, np.inf) ** 2)
    assert abs(np.linalg.det(M) - 1) <= 1e-13


def test_gram_schmidt_and_benettin_of_the_restatement():
    rng = np.random.default_rng(4)
    Z = rng.standard_normal((6, 6))
    Q, r = RT.gram_schmidt(Z)
    Qn, Rn = np.linalg.qr(Z)
    assert np.abs(Q.T @ Q - np.eye(6)).max() <= 1e-13 and (r > 0).all()
    np.testing.assert_allclose(r, np.abs(np.diag(Rn)), rtol=1e-13)
    Ms = np.stack([np.diag([2.0, 0.5, 4.0, 0.25])] * 5)                     # exponents log 2, -log 2, log 4, -log 4 exactly
    np.testing.assert_allclose(RT.benettin(Ms), np.log([2.0, 0.5, 4.0, 0.25]), rtol=1e-15)
    assert np.array_equal(RT.monodromy(Ms), np.diag([32.0, 0.5 ** 5, 1024.0, 0.25 ** 5]))
