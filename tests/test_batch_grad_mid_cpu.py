"""CPU checks of the mid-order batched NLL gradient (sgpr_fit_batch_grad_mid, fit.fit_batch_grad_mid): exported, declared and
bound alike, argument errors answered before any device is touched, and a NumPy restatement of the device's block-doubling
inverse (tests/ref_batch_inv.py) against np.linalg.inv.  The numbers are checked on the GPU (tests/test_gpu_batch_grad_mid.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ref_batch_inv as R
from tests import c_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sgpr_fit_batch_grad_mid"
EPS = np.finfo(np.float64).eps


def _lib():
    from sympgpr_amd import _lib as L
    return L, L.load_library()


def test_symbol_in_header_dynamic_table_and_signatures():
    L, lib = _lib()
    c_header.assert_bound_as_declared(NAME)
    assert L.SIGNATURES[NAME][1] == L.SIGNATURES["sgpr_fit_batch_grad"][1]
    nm = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT %s$" % NAME, nm, re.M)
    assert lib.sgpr_abi_version() == 5
    # the header documents the layout, the range, the scratch and who gives it back, next to the declaration
    doc = c_header.comment_above(NAME)
    for word in ("nhyp + 1", "sign(sig2n[b])", "<= 256", "sgpr_fit_batch_max_order()", "NaN", "scratch", "sgpr_trim"):
        assert word in doc, word
    # sgpr_fit_batch_grad keeps its limit and its text
    hdr = open(c_header.HEADER).read()
    old = re.search(r"\bint\s+sgpr_fit_batch_grad\s*\(", hdr)
    assert "n_pts with SGPR_FIT_REG) <= 256." in hdr[:old.start()].rsplit("/*", 1)[1]


def _call(lib, L, family=0, nbatch=2, n_pts=129, nhyp=3, flags=0, null=()):
    x = np.ones((max(nbatch, 1), max(n_pts, 1)))
    z = np.ones((max(nbatch, 1), 2 * max(n_pts, 1)))
    hyp = np.ones((max(nbatch, 1), 4))
    s2 = np.ones(max(nbatch, 1))
    nll = np.zeros(max(nbatch, 1))
    grad = np.zeros((max(nbatch, 1), 5))
    info = np.zeros(max(nbatch, 1), dtype=np.int32)
    p = {"x": L.dptr(x), "y": L.dptr(x), "z": L.dptr(z), "hyp": L.dptr(hyp), "sig2n": L.dptr(s2), "nll": L.dptr(nll),
         "grad": L.dptr(grad), "info": info.ctypes.data_as(C.POINTER(C.c_int))}
    for k in null:
        p[k] = None
    lib.sgpr_last_error()
    return getattr(lib, NAME)(family, nbatch, n_pts, p["x"], p["y"], p["z"], p["hyp"], nhyp, p["sig2n"], flags, None,
                              p["nll"], p["grad"], p["info"])


@pytest.mark.parametrize("kw,what", [
    (dict(n_pts=128), b"256"),                     # order 256, pairs: sgpr_fit_batch_grad's
    (dict(n_pts=256, flags=4), b"256"),            # order 256, reg
    (dict(n_pts=1025), b"2048"),                   # order 2050
    (dict(family=7), b"family"),
    (dict(family=-1), b"family"),
    (dict(nhyp=4), b"nhyp"),                       # family A has no period
    (dict(family=3, nhyp=3), b"nhyp"),             # family D has one
    (dict(flags=1), b"flag"),                      # SGPR_FIT_LOWER_ONLY is not a batch flag
    (dict(null=("x",)), b"null"),
    (dict(null=("y",)), b"null"),
    (dict(null=("z",)), b"null"),
    (dict(null=("hyp",)), b"null"),
    (dict(null=("sig2n",)), b"null"),
    (dict(null=("nll",)), b"null"),
    (dict(null=("grad",)), b"null"),
    (dict(null=("info",)), b"null"),
    (dict(nbatch=-1), b"nbatch"),
    (dict(n_pts=0), b"n_pts"),
])
def test_argument_errors_before_the_device(kw, what):
    L, lib = _lib()
    assert _call(lib, L, **kw) == L.E_ARG
    msg = lib.sgpr_last_error()
    assert b"fit_batch_grad_mid" in msg and what in msg, msg


def test_empty_batch_returns_zero():
    L, lib = _lib()
    assert _call(lib, L, nbatch=0, n_pts=129) == 0
    assert _call(lib, L, nbatch=0, n_pts=1024) == 0          # order 2048: the largest


def test_python_range_and_shape_errors():
    from sympgpr_amd import fit, func
    x = np.zeros((2, 128))
    with pytest.raises(ValueError, match="256"):
        fit.fit_batch_grad_mid("A", x, x, np.zeros((2, 256)), np.ones((2, 3)), 1e-6)             # order 256
    with pytest.raises(ValueError, match="256"):
        fit.fit_batch_grad_mid("A", np.zeros((2, 256)), np.zeros((2, 256)), np.zeros((2, 256)), np.ones((2, 3)), 1e-6, reg=True)
    with pytest.raises(ValueError):
        fit.fit_batch_grad_mid("A", np.zeros((2, 200)), np.zeros((2, 201)), np.zeros((2, 400)), np.ones((2, 3)), 1e-6)
    with pytest.raises(ValueError):
        func.nll_chol_grad_batch(np.ones((2, 4)), np.zeros(8), np.zeros(8), 8, mid="host")
    assert fit.batch_grad_mid_max_order() == fit.batch_max_order() == 2048


def _spd(n, seed):
    """a seeded SPD matrix with a condition number of about 1e4"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (Q * np.logspace(0, -4, n)) @ Q.T


@pytest.mark.parametrize("n,W,launches", [(258, 3, 5), (384, 3, 5), (600, 5, 7)])
def test_block_doubling_inverse_restated(n, W, launches):
    A = _spd(n, 7 + n)
    A = 0.5 * (A + A.T)
    img, npad, W_ = R.padded_image(A)
    assert W_ == W and npad == W * 128
    L, inv = R.factor_image(img)
    Limg = L.copy()
    U, nl = R.u_image(Limg, inv, W)
    assert nl == launches and nl <= 1 + 2 * int(np.ceil(np.log2(W)))
    cond = np.linalg.cond(A)
    Linv = np.linalg.inv(L)
    # the stored convention: U[i, k] = (L^-1)[k, i]; zero below the diagonal
    assert np.array_equal(np.tril(U, -1), np.zeros_like(U))
    assert np.max(np.abs(U.T - Linv)) <= 4 * n * EPS * np.sqrt(cond) * np.max(np.abs(Linv))
    # the factor itself is untouched on and below the diagonal (T lives above it)
    assert np.array_equal(np.tril(Limg), L)
    K = R.kinv_lower(U, Limg, W)
    Ainv = np.linalg.inv(A)
    err = np.max(np.abs(np.tril(K[:n, :n]) - np.tril(Ainv)))
    assert err <= 4 * n * EPS * cond * np.max(np.abs(Ainv)), (err, cond)
    # the padding: identity on its diagonal block, zero against the problem's rows
    assert np.array_equal(np.tril(K[n:, n:]), np.eye(npad - n))
    assert np.array_equal(K[n:, :n], np.zeros((npad - n, n)))
