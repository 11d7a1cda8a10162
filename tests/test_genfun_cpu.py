"""The generating function F of a fit (sgpr_fit_predict_genfun, SympFit.predict_genfun / predict_pairs_genfun) without a GPU: the
boundary (symbol, signature, argument errors, docstrings) and the NumPy restatement the GPU tests compare with
(tests/ref_genfun.py), pinned -- value and sign convention -- to the reference by central differences: the gradient of F is
what predict_rows / build_K_nd . alpha return.  Tolerance 1e-6 max(1, max|rows|), the project's for central differences with
h = 1e-5 l."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import ref_genfun as RG
from tests import c_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def d1_case(N, fam, m=37):
    """the inputs of the d = 1 mean tests (also tests/test_gpu_genfun.py)"""
    rng = np.random.default_rng(900 + N)
    q, P = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N)
    z = rng.standard_normal(2 * N)
    qt, Pt = rng.uniform(0, 2 * np.pi, m), rng.uniform(-3, 3, m)
    l = min(2.0, 2.0 * np.sqrt(12 * np.pi) * N ** -0.5)
    hyp = [l, l, 0.5, 1.0] if fam == "D" else [l, l, 1.0]
    return q, P, z, qt, Pt, hyp, 1e-2 / l**2


def nd_case(N, d, fam, m=37, seed=0):
    """the inputs of the d-pair tests: hyp = (lq.., lP.., [p..,] sig)"""
    rng = np.random.default_rng(950 + 10 * N + d + seed)
    X = np.column_stack([rng.uniform(0, 2 * np.pi, (N, d)), rng.uniform(-3, 3, (N, d))])
    Xt = np.column_stack([rng.uniform(0, 2 * np.pi, (m, d)), rng.uniform(-3, 3, (m, d))])
    z = rng.standard_normal(2 * d * N)
    l = min(2.0, 2.0 * np.sqrt(12 * np.pi) * N ** (-1.0 / (2 * d)))
    hyp = [l] * (2 * d) + ([0.5] * d if fam == "D" else []) + [1.0]
    return X, z, Xt, hyp, 1e-2 / l**2


def test_symbol_is_exported_and_bound_with_the_header_signature():
    from sympgpr_amd import _lib
    params = c_header.assert_bound_as_declared("sgpr_fit_predict_genfun")
    assert params == ["sgpr_fit_t f", "int m", "const double *Xt", "size_t ldxt", "const double *ref", "double *F", "double *var"]
    dp = C.POINTER(C.c_double)
    assert _lib.SIGNATURES["sgpr_fit_predict_genfun"] == (C.c_int, [C.c_void_p, C.c_int, dp, C.c_size_t, dp, dp, dp])
    assert hasattr(C.CDLL(_lib.lib_path()), "sgpr_fit_predict_genfun")
    assert _lib.load_library().sgpr_abi_version() == 5


def test_argument_errors_need_no_device():
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    Xt, F = np.zeros((2, 2), order="F"), np.zeros(2)
    for args in ((None, 2, L.dptr(Xt), 2, None, L.dptr(F), None),          # a null handle, whatever else is passed
                 (None, -1, L.dptr(Xt), 2, None, L.dptr(F), None),
                 (None, 2, L.dptr(Xt), 1, None, L.dptr(F), None),
                 (None, 2, None, 2, None, L.dptr(F), None),
                 (None, 2, L.dptr(Xt), 2, None, None, None),
                 (None, 0, None, 1, None, None, None)):
        assert lib.sgpr_fit_predict_genfun(*args) == L.E_ARG
        assert b"predict_genfun" in lib.sgpr_last_error()


def test_methods_exist_and_say_what_f_is():
    from sympgpr_amd import maps
    from sympgpr_amd.fit import SympFit
    for meth in (SympFit.predict_genfun, SympFit.predict_pairs_genfun):
        doc = " ".join(meth.__doc__.split())
        assert "dF/dq = predict_rows' out_p" in doc and "dF/dP = its out_q" in doc
        assert "latent" in doc and "no |sig2n|" in doc and "slightly negative" in doc
        assert "undetermined constant" in doc and "does not vanish with data" in doc
    assert callable(maps.genfun_along) and "F(q_k, P_{k+1})" in maps.genfun_along.__doc__


@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
@pytest.mark.parametrize("N", [1, 63, 257])
def test_central_differences_d1_vs_oracle_predict_rows(oracle, fam, N):
    q, P, z, qt, Pt, hyp, s2 = d1_case(N, fam)
    alpha, _, _ = oracle.fit(fam, q, P, z, hyp, s2, threads=4)
    op, oq = oracle.predict_rows(fam, qt, Pt, q, P, hyp, alpha)
    h = 1e-5 * hyp[0]
    F = lambda a, b: RG.genfun_d1(oracle, fam, q, P, hyp, alpha, a, b)["F"]
    dq = (F(qt + h, Pt) - F(qt - h, Pt)) / (2 * h)
    dP = (F(qt, Pt + h) - F(qt, Pt - h)) / (2 * h)
    scale = max(1.0, np.abs(op).max(), np.abs(oq).max())
    err = max(np.abs(dq - op).max(), np.abs(dP - oq).max())
    print("%s N=%d: max|dF - rows| = %.3g  (tol %.3g)" % (fam, N, err, 1e-6 * scale))
    assert err <= 1e-6 * scale


@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_central_differences_nd_vs_oracle_gram(oracle, fam, d):
    N = 40
    X, z, Xt, hyp, s2 = nd_case(N, d, fam)
    alpha, _, _ = oracle.fit_nd(fam, X, z, hyp, s2)
    m, D = Xt.shape
    rows = (oracle.build_K_nd(fam, Xt, X, hyp) @ alpha).reshape(D, m).T          # (m, D): column a = dF/dx_a
    h = 1e-5 * hyp[0]
    grad = np.empty((m, D))
    for a in range(D):
        e = np.zeros(D)
        e[a] = h
        grad[:, a] = (RG.genfun_nd(fam, X, hyp, alpha, Xt + e)["F"] - RG.genfun_nd(fam, X, hyp, alpha, Xt - e)["F"]) / (2 * h)
    scale = max(1.0, np.abs(rows).max())
    err = np.abs(grad - rows).max()
    print("%s d=%d: max|dF - K* alpha| = %.3g  (tol %.3g)" % (fam, d, err, 1e-6 * scale))
    assert err <= 1e-6 * scale


@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
def test_the_two_restatements_agree_at_d1(oracle, fam):
    """the per-coordinate forms at d = 1 are the oracle's dkdx_num / dkdy_num / kern_num to rounding"""
    q, P, z, qt, Pt, hyp, s2 = d1_case(63, fam)
    alpha = np.random.default_rng(5).standard_normal(2 * 63)
    a = RG.genfun_d1(oracle, fam, q, P, hyp, alpha, qt, Pt)
    b = RG.genfun_nd(fam, np.column_stack((q, P)), hyp, alpha, np.column_stack((qt, Pt)))
    assert np.abs(a["v"] - b["v"]).max() <= 32 * EPS * max(1.0, np.abs(a["v"]).max())
    assert np.abs(a["kappa"] - b["kappa"]).max() <= 32 * EPS * np.abs(a["kappa"]).max()
    assert np.all(np.abs(a["F"] - b["F"]) <= (32 + 63) * EPS * a["T"])


def test_host_variance_and_the_undetermined_constant(oracle):
    """derivative observations do not fix the constant of F: the pointwise variance stays a sizeable part of the prior, the
    variance of a difference F(x) - F(x0) is at least 10 x smaller (N = 257, family A)"""
    N, fam = 257, "A"
    q, P, z, qt, Pt, hyp, s2 = d1_case(N, fam)
    Ky = oracle.build_K(fam, q, P, q, P, hyp, threads=4) + abs(s2) * np.eye(2 * N)
    cond = float(np.linalg.cond(Ky))
    res = RG.genfun_nd(fam, np.column_stack((q, P)), hyp, np.zeros(2 * N), np.column_stack((qt, Pt)))
    var, prior = RG.host_variance(res, Ky)
    dvar, dprior = RG.host_variance(res, Ky, ref=0)
    tol = 100 * cond * EPS * max(prior.max(), dprior.max())
    print("cond %.3g  var/prior %.3g .. %.3g  var of differences max %.3g  ratio min %.3g"
          % (cond, (var / prior).min(), (var / prior).max(), dvar.max(), var.min() / dvar[1:].max()))
    assert cond <= 1e6
    assert np.all(var >= -tol) and np.all(dvar >= -tol) and np.all(var <= prior + tol)
    assert dvar[0] == 0.0 and dprior[0] == 0.0
    assert var.min() >= 10.0 * dvar[1:].max()
