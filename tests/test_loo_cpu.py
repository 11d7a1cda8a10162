"""CPU checks of leave-one-point-out cross-validation (sgpr_fit_loo, sgpr_fit_batch_loo, SympFit.loo, fit.fit_batch_loo,
func.loo_chol*): the block formulas the device uses (tests/ref_loo.py: loo_blocks) against the definition -- every point's D
rows and columns actually deleted, a NumPy refit on the rest, the left-out rows predicted -- and the boundary: both symbols
declared, bound and exported alike, argument errors answered before any device is touched.  The device's numbers are checked
on the GPU (tests/test_gpu_loo.py, tests/test_gpu_batch_loo.py).

Tolerance: the project's rule for ill-conditioned fixtures, max(1e-10, 50 cond eps) relative to the max-norm of each array
(ref_loo.tolerance).  The two CPU routes agree to 1e-12 or better on these fixtures (cond 7e2 .. 4e4), so the rule stands."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ref_loo as R
from tests import c_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(fam, kind, N) for fam in "ABCD" for kind, N in (("reg", 30), (1, 12), (1, 25), (2, 17), (3, 13))]


@pytest.mark.parametrize("fam,kind,N", CASES)
def test_block_formulas_against_deletion(oracle, fam, kind, N):
    p = R.problem(oracle, fam, kind, N, 100 + N)
    assert p["cond"] <= 1e8, p["cond"]
    blocks = R.loo_blocks(p["Ky"], p["z"], N, p["D"])
    deleted = R.loo_by_deletion(p["Ky"], p["z"], N, p["D"])
    R.compare(blocks, deleted, p["cond"], "%s %s N=%d" % (fam, kind, N))
    assert blocks["resid"].shape == (N, p["D"]) and blocks["cov"].shape == (N, p["D"], p["D"])
    assert np.all(np.linalg.eigvalsh(blocks["cov"]) > 0)


def _lib():
    from sympgpr_amd import _lib as L
    return L, L.load_library()


@pytest.mark.parametrize("name,like", [("sgpr_fit_loo", None), ("sgpr_fit_batch_loo", "sgpr_fit_batch_grad")])
def test_symbols_in_header_dynamic_table_and_signatures(name, like):
    L, lib = _lib()
    c_header.assert_bound_as_declared(name)
    if like:
        assert L.SIGNATURES[name][1] == L.SIGNATURES[like][1]
    nm = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT %s$" % name, nm, re.M)
    assert lib.sgpr_abi_version() == 5
    doc = c_header.comment_above(name)
    for word in ("press", "NaN", "scratch", "ABI 5 (an additional entry point)"):
        assert word in doc, word


def _call(lib, L, family=0, nbatch=2, n_pts=40, nhyp=3, flags=0, null=()):
    B, npts = max(nbatch, 1), max(n_pts, 1)
    x, z, hyp, s2 = np.ones((B, npts)), np.ones((B, 2 * npts)), np.ones((B, 4)), np.ones(B)
    nll, loo, info = np.zeros(B), np.zeros((B, 2)), np.zeros(B, dtype=np.int32)
    p = {"x": L.dptr(x), "y": L.dptr(x), "z": L.dptr(z), "hyp": L.dptr(hyp), "sig2n": L.dptr(s2), "nll": L.dptr(nll),
         "loo": L.dptr(loo), "info": info.ctypes.data_as(C.POINTER(C.c_int))}
    for k in null:
        p[k] = None
    return lib.sgpr_fit_batch_loo(family, nbatch, n_pts, p["x"], p["y"], p["z"], p["hyp"], nhyp, p["sig2n"], flags, None,
                                  p["nll"], p["loo"], p["info"])


@pytest.mark.parametrize("kw,what", [
    (dict(family=7), b"family"),
    (dict(family=-1), b"family"),
    (dict(nhyp=4), b"nhyp"),                       # family A has no period
    (dict(family=3, nhyp=3), b"nhyp"),             # family D has one
    (dict(flags=1), b"flag"),                      # SGPR_FIT_LOWER_ONLY is not a batch flag
    (dict(nbatch=-1), b"nbatch"),
    (dict(n_pts=0), b"n_pts"),
    (dict(n_pts=-3), b"n_pts"),
    (dict(n_pts=1025), b"2048"),                   # order 2050
    (dict(n_pts=2049, flags=4), b"2048"),          # reg, order 2049
    (dict(null=("nll",)), b"null"),
    (dict(null=("loo",)), b"null"),
    (dict(null=("info",)), b"null"),
    (dict(null=("x",)), b"null"),
    (dict(null=("sig2n",)), b"null"),
])
def test_batch_argument_errors_before_the_device(kw, what):
    L, lib = _lib()
    assert _call(lib, L, **kw) == L.E_ARG
    msg = lib.sgpr_last_error()
    assert b"fit_batch_loo" in msg and what in msg, msg


def test_empty_batch_returns_zero():
    L, lib = _lib()
    assert _call(lib, L, nbatch=0, n_pts=40) == 0
    assert _call(lib, L, nbatch=0, n_pts=129) == 0           # the mid path's range
    assert _call(lib, L, nbatch=0, n_pts=1024) == 0          # order 2048: the largest


def test_handle_entry_rejects_a_null_handle():
    L, lib = _lib()
    two = np.zeros(2)
    assert lib.sgpr_fit_loo(None, L.dptr(two), None, None, None) == L.E_ARG
    assert b"fit_loo" in lib.sgpr_last_error()


def test_python_calls_without_a_device_and_shape_errors():
    import sympgpr_amd
    from sympgpr_amd import fit, func
    x = np.linspace(0.1, 3.0, 8)
    with pytest.raises(ValueError):
        fit.fit_batch_loo("A", np.zeros((2, 20)), np.zeros((2, 21)), np.zeros((2, 40)), np.ones((2, 3)), 1e-6)
    with pytest.raises(ValueError):
        func.loo_chol(np.array([1.0, 1.0, 1.0, 1e-3]), np.zeros(8), np.zeros(8), 0)
    with pytest.raises(ValueError):
        func.loo_chol(np.array([1.0, 1.0, 1.0, 1e-3]), np.zeros(8), np.zeros(8), 12)     # x holds four points only
    assert callable(fit.SympFit.loo)
    calls = [lambda: fit.fit_batch_loo("A", x[None], x[None], np.ones((1, 16)), np.ones((1, 3)), 1e-3),
             lambda: func.loo_chol(np.array([1.0, 1.0, 1.0, 1e-3]), np.concatenate([x, x[::-1]]), np.ones(16), 16),
             lambda: func.loo_chol_reg(np.array([1.0, 1.0, 1.0, 1e-3]), np.concatenate([x, x[::-1]]), np.ones(8), 8),
             lambda: func.loo_chol_batch(np.array([[1.0, 1.0, 1.0, 1e-3]]), np.concatenate([x, x[::-1]]), np.ones(16), 16)]
    for call in calls:
        if sympgpr_amd.device_count() > 0:
            call()                                   # with a device the same calls go through
        else:
            with pytest.raises(sympgpr_amd.NoDeviceError):
                call()
