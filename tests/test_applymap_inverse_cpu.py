"""CPU checks of the backward entries of the d-pair map (sgpr_fit_applymap_nd_inverse, sgpr_applymap_nd_inverse_host): declared,
exported and bound alike; every argument error answered with SGPR_E_ARG before any device call, SGPR_MAP_EXPLICIT among them for
every family; the Python wrappers and maps.symplectic_inverse; and the NumPy restatement tests/ref_inverse.py -- the CPU reference
of tests/test_gpu_applymap_inverse.py -- held against central differences and against the forward step it undoes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ref_inverse as RI
from tests import ref_tangent as RT
from tests.test_applymap_nd_cpu import HOST_BAD as FORWARD_HOST_BAD
from tests.test_gpu_applymap_nd import _hyp, _starts, _training

from tests import c_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ip = C.POINTER(C.c_int)
NAMES = (("sgpr_fit_applymap_nd_inverse", 11), ("sgpr_applymap_nd_inverse_host", 18))


def test_header_exports_map_ctypes_table_and_library_agree():
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    dyn = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True, check=True).stdout
    for name, nargs in NAMES:
        c_header.assert_bound_as_declared(name, nargs)
        assert c_header.in_exports_map(name), name + " is not covered by exports.map"
        assert re.search(r" T %s$" % name, dyn, flags=re.M), name + " is not exported"
    # the same argument list as the forward pair, position by position
    for inv, fwd in (("sgpr_fit_applymap_nd_inverse", "sgpr_fit_applymap_nd"), ("sgpr_applymap_nd_inverse_host", "sgpr_applymap_nd_host")):
        assert L.SIGNATURES[inv] == L.SIGNATURES[fwd]
    assert lib.sgpr_abi_version() == 5


def _host_args(**over):
    """a valid sgpr_applymap_nd_inverse_host call (family A, d = 2), as a dict of named arguments"""
    from sympgpr_amd import _lib as L
    d, n0, ntest, nm = 2, 4, 3, 2
    keep = dict(hyp=np.array([1.2, 1.2, 1.5, 1.5, 1.0]), X=np.zeros((n0, 2 * d), order="F"), alpha=np.zeros(2 * d * n0),
                Q0=np.zeros((ntest, d), order="F"), P0=np.zeros((ntest, d), order="F"), qmap=np.zeros((nm, ntest, d)),
                pmap=np.zeros((nm, ntest, d)), iters=np.zeros((nm - 1, ntest), dtype=np.int32), hyp7=np.ones(7))
    a = dict(family=0, d=d, mode=L.MAP_WRAP_Q, nm=nm, ntest=ntest, hyp=L.dptr(keep["hyp"]), nhyp=5, n0=n0, X=L.dptr(keep["X"]),
             ldx=n0, alpha=L.dptr(keep["alpha"]), Q0=L.dptr(keep["Q0"]), ldq=ntest, P0=L.dptr(keep["P0"]), ldp=ntest,
             qmap=L.dptr(keep["qmap"]), pmap=L.dptr(keep["pmap"]), iters=keep["iters"].ctypes.data_as(_ip))
    for k, v in over.items():
        a[k] = L.dptr(keep[v]) if isinstance(v, str) else v
    return a, keep


# everything the forward entry refuses (tests/test_applymap_nd_cpu.py: HOST_BAD), and explicit mode: with the product families
# A (0) and USER (4), and with the sum kernel B (1) as well
HOST_BAD = FORWARD_HOST_BAD + [dict(mode=4), dict(mode=5), dict(family=1, mode=4), dict(family=1, mode=5), dict(family=4, mode=4),
                               dict(family=4, mode=5), dict(family=3, nhyp=7, hyp="hyp7", mode=4)]


@pytest.mark.parametrize("over", HOST_BAD, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_host_entry_argument_errors_come_before_any_device_call(over):
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    a, keep = _host_args(**over)
    assert lib.sgpr_applymap_nd_inverse_host(*a.values()) == L.E_ARG
    assert b"applymap_nd_inverse_host" in lib.sgpr_last_error()


def test_host_entry_valid_calls_reach_the_device_check():
    """calls that pass every check end at SGPR_E_NODEVICE without a GPU, not at SGPR_E_ARG: no iters, nm = 1, the sum kernel
    (family B = 1) with mode 0, family D with its periods"""
    import sympgpr_amd
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    for over in ({}, dict(iters=None), dict(nm=1), dict(family=1, mode=0), dict(mode=0), dict(family=3, nhyp=7, hyp="hyp7")):
        a, keep = _host_args(**over)
        rc = lib.sgpr_applymap_nd_inverse_host(*a.values())
        assert rc == (0 if sympgpr_amd.device_count() > 0 else L.E_NODEVICE), over


def test_handle_entry_argument_errors_come_before_any_device_call():
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    fn = lib.sgpr_fit_applymap_nd_inverse
    ntest, nm, d = 3, 2, 2
    Q0, P0 = np.zeros((ntest, d), order="F"), np.zeros((ntest, d), order="F")
    q, p = np.zeros((nm, ntest, d)), np.zeros((nm, ntest, d))
    good = dict(f=None, mode=0, nm=nm, ntest=ntest, Q0=L.dptr(Q0), ldq=ntest, P0=L.dptr(P0), ldp=ntest, qmap=L.dptr(q),
                pmap=L.dptr(p), iters=None)
    assert fn(*good.values()) == L.E_ARG                    # null handle
    assert b"fit_applymap_nd_inverse" in lib.sgpr_last_error()
    for over in (dict(mode=2), dict(nm=0), dict(Q0=None), dict(ldq=2)):      # ... whatever else is wrong with the call
        assert fn(*dict(good, **over).values()) == L.E_ARG


def test_python_wrappers_validate_before_the_library_is_asked():
    from sympgpr_amd import maps
    from sympgpr_amd.fit import SympFit
    import inspect
    assert list(inspect.signature(SympFit.applymap_pairs_inverse).parameters) == ["self", "nm", "Q0", "P0", "wrap_q", "return_iters"]
    assert "preimage" in SympFit.applymap_pairs_inverse.__doc__ and "symplectic_inverse" in SympFit.applymap_pairs_inverse.__doc__
    hyp, X, alpha = [1.2, 1.2, 1.5, 1.5, 1.0], np.zeros((4, 4)), np.zeros(16)
    Q0, P0 = np.zeros((3, 2)), np.zeros((3, 2))
    bad = [dict(d=4, X=np.zeros((4, 8)), alpha=np.zeros(32)), dict(X=np.zeros((4, 6))), dict(X=np.zeros(16)),
           dict(alpha=np.zeros(15)), dict(Q0=np.zeros(3)), dict(Q0=np.zeros((3, 3))), dict(P0=np.zeros((2, 2))),
           dict(mode=maps.WRAP_P), dict(mode=maps.LOSS_NEGP), dict(nm=0),
           dict(mode=maps.EXPLICIT), dict(mode=maps.EXPLICIT | maps.WRAP_Q), dict(family="B", mode=maps.EXPLICIT)]
    for over in bad:
        a = dict(family="A", d=2, mode=maps.WRAP_Q, nm=3, hyp=hyp, X=X, alpha=alpha, Q0=Q0, P0=P0)
        a.update(over)
        with pytest.raises(ValueError):
            maps.run_map_nd_inverse(**a)
    # the forward signature, name by name
    assert list(inspect.signature(maps.run_map_nd_inverse).parameters) == list(inspect.signature(maps.run_map_nd).parameters)


def test_symplectic_inverse_on_hand_made_matrices():
    from sympgpr_amd import maps
    t = 0.7
    rot = np.array([[np.cos(t), np.sin(t)], [-np.sin(t), np.cos(t)]])
    shear = np.array([[1.0, 0.0], [3.0, 1.0]])
    assert np.array_equal(maps.symplectic_inverse(rot), rot.T)                              # a rotation's inverse, exactly
    assert np.array_equal(maps.symplectic_inverse(shear), [[1.0, 0.0], [-3.0, 1.0]])
    assert np.array_equal(maps.symplectic_inverse(np.diag([2.0, 0.5])), np.diag([0.5, 2.0]))
    # D = 4 in the order (q_1, q_2, p_1, p_2): a rotation in the plane (q_1, p_1), a symmetric shear, their product.  M @ inv has
    # 4 products per entry of factors up to 2.5: a few ulp of I
    c, s = np.cos(t), np.sin(t)
    R4 = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1.0]])
    S4 = np.eye(4)
    S4[2:, :2] = [[1.0, 0.5], [0.5, -2.0]]
    Ms = np.stack((R4, S4, R4 @ S4, S4 @ R4 @ S4))
    inv = maps.symplectic_inverse(Ms)
    assert inv.shape == Ms.shape
    J = np.zeros((4, 4))
    J[:2, 2:], J[2:, :2] = np.eye(2), -np.eye(2)
    for M, Mi in zip(Ms, inv):
        assert np.array_equal(Mi, -J @ M.T @ J)                                             # the definition; +-1 and 0 factors only
        err = np.abs(M @ Mi - np.eye(4)).max()
        print("max |M inv - I| = %.2e" % err)
        assert err <= 8 * np.finfo(float).eps
    assert np.array_equal(maps.symplectic_inverse(maps.symplectic_inverse(Ms)), Ms)
    for bad in (np.eye(3), np.zeros((2, 3)), np.zeros(4), np.zeros((2, 4, 2))):
        with pytest.raises(ValueError):
            maps.symplectic_inverse(bad)


# ---- tests/ref_inverse.py ----------------------------------------------------------------------------------------------------

NT, NTEST, NM = 40, 5, 6          # 40 points, 5 starts, 5 steps
REF_CASES = [(fam, d) for fam in "ACDB" for d in (1, 2, 3)]


@pytest.fixture(scope="module")
def problems(oracle):
    """per (family, d): the data of tests/test_gpu_applymap_nd.py, alpha from a dense Cholesky solve at sig2n = 1e-8, and the
    forward orbit of the restatement -- computed once, never changed.  Family B gets the separable part of the generating
    function (c = 0), as test_explicit_mode_family_b of that file does and for its reason: a sum kernel cannot represent the
    coupling term, the fit answers it with |alpha| ~ 1e7, and the rounding of the sums of G alone is then 1e-8 per evaluation in
    any arithmetic (measured here with c = 0.4 at d = 1: round trip 6.9e-9 in q, with a closing residual of exactly 0)."""
    out = {}
    for fam, d in REF_CASES:
        X, z = _training(d, NT, c=0.0) if fam == "B" else _training(d, NT)
        hyp = _hyp(fam, d)
        alpha = oracle.fit_nd(fam, X, z, hyp, 1e-8)[0]
        Q0, P0 = _starts(d, NTEST)
        wrap = fam != "C"
        q, p, its, res = RI.forward_orbit(fam, d, hyp, X, alpha, NM, Q0, P0, wrap)
        assert np.isfinite(q).all() and np.isfinite(p).all()
        for a in (X, z, hyp, alpha, Q0, P0, q, p, its):
            a.setflags(write=False)
        out[fam, d] = dict(X=X, hyp=hyp, alpha=alpha, Q0=Q0, P0=P0, wrap=wrap, q=q, p=p, its=its)
    return out


@pytest.mark.parametrize("fam,d", REF_CASES)
def test_restated_backward_jacobian_against_central_differences(problems, fam, d):
    """I + B^T at the points (q_i, P_{i+1}) of the forward orbit against central differences of q -> q + G_P(q, P) with h = 1e-5:
    O(h^2) truncation (third derivatives of G of order 1: 1e-10) and rounding eps |G| / h ~ 1e-11 per entry; rtol = atol = 1e-6,
    the tolerance of the step-matrix test of tests/test_applymap_tangent_cpu.py, covers both with a large factor."""
    r = problems[fam, d]
    args = (fam, d, r["hyp"], r["X"], r["alpha"])
    h, worst = 1e-5, 0.0
    for i in range(NM - 1):
        for k in range(NTEST):
            q, P = r["q"][i, k], r["p"][i + 1, k]
            f = lambda qq: qq + RT.gradient(*args, np.concatenate((qq, P)))[d:]
            fd = np.column_stack([(f(q + h * e) - f(q - h * e)) / (2 * h) for e in np.eye(d)])
            Jb = RI.backward_jacobian(*args, q, P)
            worst = max(worst, float(np.abs(Jb - fd).max()))
            np.testing.assert_allclose(Jb, fd, rtol=1e-6, atol=1e-6)
    print("family %s d = %d: max |I + B^T - fd| = %.3e" % (fam, d, worst))


@pytest.mark.parametrize("fam,d", REF_CASES)
def test_restated_forward_then_backward_returns_the_start(problems, fam, d):
    """five forward steps, then five chained backward steps from the end point: row i of the backward orbit is row NM - 1 - i of
    the forward one within 1e-10 (wrapped q on the circle).  Each solve closes to 1e-13 relative and the d x d systems have
    |det(I + B)| >= 0.86, so a chain of five stays within a small multiple of the rounding of G, eps sum_j |K*_j alpha_j|: largest
    at d = 1, where Ky has cond 1e9 and alpha is large.  The restatement alone measures 1e-12 at d = 1, 2e-14 at d = 2, 2e-15 at
    d = 3 (printed)."""
    r = problems[fam, d]
    qb, pb, its, res = RI.backward_orbit(fam, d, r["hyp"], r["X"], r["alpha"], NM, r["q"][-1], r["p"][-1], r["wrap"])
    dq = RI.circle_distance(qb, r["q"][::-1]) if r["wrap"] else np.abs(qb - r["q"][::-1])
    dp = np.abs(pb - r["p"][::-1])
    print("family %s d = %d: round trip max |dq| = %.3e  max |dp| = %.3e  closing residual %.3e  backward iterations %d..%d "
          "(forward %d..%d)" % (fam, d, dq.max(), dp.max(), res.max(), its.min(), its.max(), r["its"].min(), r["its"].max()))
    assert dq.max() <= 1e-10 and dp.max() <= 1e-10
    if fam == "B":
        assert its.max() <= 2                               # G_P does not depend on q: the first step is exact
