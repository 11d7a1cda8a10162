"""CPU checks of the batched leave-one-point-out gradient (sgpr_fit_batch_loo_grad, fit.fit_batch_loo_grad,
func.loo_chol_grad_batch): exported, declared and bound alike, argument errors answered before any device is touched, and shape
and objective errors raised in Python before the library is called.  The numbers are checked on the GPU
(tests/test_gpu_batch_loo_grad.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import c_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sgpr_fit_batch_loo_grad"


def _lib():
    from sympgpr_amd import _lib as L
    return L, L.load_library()


def test_symbol_in_header_dynamic_table_and_signatures():
    L, lib = _lib()
    c_header.assert_bound_as_declared(NAME, 16)
    nm = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT %s$" % NAME, nm, re.M)
    assert lib.sgpr_abi_version() == 5
    assert (L.LOO_LPD, L.LOO_PRESS) == (0, 1)
    # the header documents the layout, the guarantees and the scratch next to the declaration
    doc = c_header.comment_above(NAME)
    for word in ("nhyp + 1", "sign(sig2n[b])", "<= 256", "NaN", "sgpr_fit_loo_grad", "bit-identical", "1.8 MiB"):
        assert word in doc, word


def _call(lib, L, family=0, nbatch=2, n_pts=5, nhyp=3, flags=0, which=0, null=()):
    x = np.ones((max(nbatch, 1), max(n_pts, 1)))
    z = np.ones((max(nbatch, 1), 2 * max(n_pts, 1)))
    hyp = np.ones((max(nbatch, 1), 4))
    s2 = np.ones(max(nbatch, 1))
    nll = np.zeros(max(nbatch, 1))
    value = np.zeros(max(nbatch, 1))
    grad = np.zeros((max(nbatch, 1), 5))
    info = np.zeros(max(nbatch, 1), dtype=np.int32)
    p = {"x": L.dptr(x), "y": L.dptr(x), "z": L.dptr(z), "hyp": L.dptr(hyp), "sig2n": L.dptr(s2), "nll": L.dptr(nll),
         "value": L.dptr(value), "grad": L.dptr(grad), "info": info.ctypes.data_as(C.POINTER(C.c_int))}
    for k in null:
        p[k] = None
    lib.sgpr_last_error()
    return getattr(lib, NAME)(family, nbatch, n_pts, p["x"], p["y"], p["z"], p["hyp"], nhyp, p["sig2n"], flags, which, None,
                              p["nll"], p["value"], p["grad"], p["info"])


@pytest.mark.parametrize("kw,what", [
    (dict(family=7), b"family"),
    (dict(family=-1), b"family"),
    (dict(nhyp=4), b"nhyp"),                       # family A has no period
    (dict(family=3, nhyp=3), b"nhyp"),             # family D has one
    (dict(flags=1), b"flag"),                      # SGPR_FIT_LOWER_ONLY is not a batch flag
    (dict(which=2), b"which"),
    (dict(which=-1), b"which"),
    (dict(nbatch=-1), b"nbatch"),
    (dict(n_pts=0), b"n_pts"),
    (dict(n_pts=-3), b"n_pts"),
    (dict(n_pts=129), b"256"),                     # order 258
    (dict(n_pts=257, flags=4), b"256"),            # reg order 257
    (dict(null=("nll",)), b"null"),
    (dict(null=("value",)), b"null"),
    (dict(null=("grad",)), b"null"),
    (dict(null=("info",)), b"null"),
    (dict(null=("x",)), b"null"),
    (dict(null=("y",)), b"null"),
    (dict(null=("z",)), b"null"),
    (dict(null=("hyp",)), b"null"),
    (dict(null=("sig2n",)), b"null"),
])
def test_argument_errors_before_the_device(kw, what):
    L, lib = _lib()
    assert _call(lib, L, **kw) == L.E_ARG
    msg = lib.sgpr_last_error()
    assert msg.startswith(b"fit_batch_loo_grad:") and what in msg, msg


def test_empty_batch_returns_zero():
    L, lib = _lib()
    assert _call(lib, L, nbatch=0) == 0
    assert _call(lib, L, nbatch=0, n_pts=128, which=1) == 0  # order 256: the largest
    assert _call(lib, L, nbatch=0, n_pts=256, flags=4) == 0  # reg order 256


def test_python_shape_and_objective_errors_before_the_library(monkeypatch):
    from sympgpr_amd import _lib as L
    from sympgpr_amd import fit, func

    def boom():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(L, "load_library", boom)
    x = np.zeros((3, 4))
    with pytest.raises(ValueError):
        fit.fit_batch_loo_grad("A", x, np.zeros((3, 5)), np.zeros((3, 8)), np.ones((3, 3)), 1e-6)
    with pytest.raises(ValueError):
        fit.fit_batch_loo_grad("A", x, x, np.zeros((3, 7)), np.ones((3, 3)), 1e-6)
    with pytest.raises(ValueError):
        fit.fit_batch_loo_grad("A", x, x, np.zeros((3, 4)), np.ones((2, 3)), 1e-6, reg=True)
    with pytest.raises(ValueError, match="objective"):
        fit.fit_batch_loo_grad("A", x, x, np.zeros((3, 8)), np.ones((3, 3)), 1e-6, objective="nll")
    with pytest.raises(ValueError):
        func.loo_chol_grad_batch(np.ones((2, 4)), np.zeros(6), np.zeros(8), 8)     # x holds 3 of 4 points
    with pytest.raises(ValueError):
        func.loo_chol_grad_batch(np.ones((2, 4)), np.zeros(8), np.zeros(5), 8)     # y holds 5 of 8 targets
    with pytest.raises(ValueError):
        func.loo_chol_grad_batch(np.ones((2, 1)), np.zeros(8), np.zeros(8), 8)     # no room for sig2_n
    with pytest.raises(ValueError):
        func.loo_chol_grad_batch(np.ones((2, 4)), np.zeros(8), np.zeros(8), 0)     # N must be positive
    with pytest.raises(ValueError, match="objective"):
        func.loo_chol_grad_batch(np.ones((2, 4)), np.zeros(8), np.zeros(8), 8, objective="lpd")
