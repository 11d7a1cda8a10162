"""CPU checks of the full NLL gradient entry point (sgpr_fit_nll_grad_full): exported, bound with its SIGNATURES argtypes,
argument errors answered before any device is touched, the header and the binding agree, and SympFit.nll_grad_full
documents its layout.  The numbers are checked on the GPU (tests/test_gpu_nll_grad_full.py)."""
import os

import numpy as np

from tests import c_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_nll_grad_full_exported_and_bound():
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    fn = lib.sgpr_fit_nll_grad_full
    assert fn.argtypes == L.SIGNATURES["sgpr_fit_nll_grad_full"][1]
    assert fn.restype == L.SIGNATURES["sgpr_fit_nll_grad_full"][0]
    assert lib.sgpr_abi_version() == 5


def test_nll_grad_full_argument_errors():
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    fn = lib.sgpr_fit_nll_grad_full
    g = np.zeros(4)
    for args in ((None, L.dptr(g), 4),       # null handle
                 (None, None, 4),            # null handle and grad
                 (None, L.dptr(g), 0),       # wrong ngrad
                 (None, L.dptr(g), -3)):
        lib.sgpr_last_error()
        assert fn(*args) == L.E_ARG
        assert b"nll_grad_full" in lib.sgpr_last_error()


def test_header_and_signature_agree():
    from sympgpr_amd import _lib as L
    c_header.assert_bound_as_declared("sgpr_fit_nll_grad_full", 3)
    # the header documents the layout next to the declaration
    doc = c_header.comment_above("sgpr_fit_nll_grad_full")
    assert "nhyp + 1" in doc and "sign(sig2n)" in doc and "SGPR_E_STATE" in doc and "scratch" in doc


def test_sympfit_nll_grad_full_documents_layout():
    from sympgpr_amd.fit import SympFit
    meth = getattr(SympFit, "nll_grad_full")
    assert callable(meth)
    doc = " ".join((meth.__doc__ or "").split())
    assert "(nhyp + 1,)" in doc
    assert "(lx, ly, [p,] sig)" in doc and "(lq_1..lq_d, lP_1..lP_d, [p_1..p_d,] sig)" in doc
    assert "sign(sig2n)" in doc and "sign(0) = +1" in doc
    assert "jac=True" in doc
