"""CPU checks of the predictive-covariance entry point (sgpr_fit_predict_cov): exported, bound, argument errors answered
before any device is touched, and the SympFit methods exist.  The numbers are checked on the GPU
(tests/test_gpu_predict_cov.py)."""
import ctypes as C

import numpy as np


def test_predict_cov_exported_and_null_handle_is_arg_error():
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    fn = lib.sgpr_fit_predict_cov
    assert fn.argtypes == L.SIGNATURES["sgpr_fit_predict_cov"][1]
    Xt, mean, cov = np.zeros((4, 2), order="F"), np.zeros(8), np.zeros(16)
    assert fn(None, 4, L.dptr(Xt), 4, L.dptr(mean), L.dptr(cov)) == L.E_ARG
    assert b"predict_cov" in lib.sgpr_last_error()
    # a bad leading dimension or null outputs are argument errors too (the handle is checked first; none is needed here)
    assert fn(None, 4, L.dptr(Xt), 3, L.dptr(mean), L.dptr(cov)) == L.E_ARG
    assert fn(None, 4, L.dptr(Xt), 4, None, None) == L.E_ARG
    assert lib.sgpr_abi_version() == 5


def test_sympfit_has_covariance_methods():
    from sympgpr_amd.fit import SympFit
    for name in ("predict_cov", "predict_pairs_cov"):
        meth = getattr(SympFit, name)
        assert callable(meth)
        doc = " ".join((meth.__doc__ or "").split())
        assert "no |sig2n|" in doc and "negative" in doc, name
