"""CPU checks of the d-pair map entries (sgpr_fit_applymap_nd, sgpr_applymap_nd_host): declared, exported and bound alike,
every argument error answered with SGPR_E_ARG before any device call, and the Python wrappers validate shapes.  The numbers
are checked on the GPU (tests/test_gpu_applymap_nd.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import c_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ip = C.POINTER(C.c_int)


def test_header_ctypes_table_and_library_agree():
    from sympgpr_amd import _lib as L
    for name, nargs in (("sgpr_fit_applymap_nd", 11), ("sgpr_applymap_nd_host", 18)):
        c_header.assert_bound_as_declared(name, nargs)
    assert L.load_library().sgpr_abi_version() == 5


def _host_args(**over):
    """a valid sgpr_applymap_nd_host call (family A, d = 2), as a dict of named arguments"""
    from sympgpr_amd import _lib as L
    d, n0, ntest, nm = 2, 4, 3, 2
    keep = dict(hyp=np.array([1.2, 1.2, 1.5, 1.5, 1.0]), X=np.zeros((n0, 2 * d), order="F"), alpha=np.zeros(2 * d * n0),
                Q0=np.zeros((ntest, d), order="F"), P0=np.zeros((ntest, d), order="F"), qmap=np.zeros((nm, ntest, d)),
                pmap=np.zeros((nm, ntest, d)), iters=np.zeros((nm - 1, ntest), dtype=np.int32))
    a = dict(family=0, d=d, mode=L.MAP_WRAP_Q, nm=nm, ntest=ntest, hyp=L.dptr(keep["hyp"]), nhyp=5, n0=n0, X=L.dptr(keep["X"]),
             ldx=n0, alpha=L.dptr(keep["alpha"]), Q0=L.dptr(keep["Q0"]), ldq=ntest, P0=L.dptr(keep["P0"]), ldp=ntest,
             qmap=L.dptr(keep["qmap"]), pmap=L.dptr(keep["pmap"]), iters=keep["iters"].ctypes.data_as(_ip))
    a.update(over)
    return a, keep


HOST_BAD = [dict(family=9), dict(family=-1), dict(d=0), dict(d=4), dict(mode=2), dict(mode=8), dict(mode=16), dict(nm=0),
            dict(ntest=-1), dict(hyp=None), dict(nhyp=4), dict(nhyp=7), dict(family=3, nhyp=5), dict(n0=-1), dict(X=None),
            dict(alpha=None), dict(ldx=3), dict(Q0=None), dict(P0=None), dict(ldq=2), dict(ldp=2), dict(qmap=None),
            dict(pmap=None)]


@pytest.mark.parametrize("over", HOST_BAD, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_host_entry_argument_errors_come_before_any_device_call(over):
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    a, keep = _host_args(**over)
    assert lib.sgpr_applymap_nd_host(*a.values()) == L.E_ARG
    assert b"applymap_nd" in lib.sgpr_last_error()


def test_host_entry_valid_call_reaches_the_device_check():
    """the same arguments unchanged pass every check: without a GPU the call ends at SGPR_E_NODEVICE, not SGPR_E_ARG"""
    import sympgpr_amd
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    for over in ({}, dict(iters=None), dict(family=3, nhyp=7, hyp=L.dptr(np.ones(7)))):
        a, keep = _host_args(**over)
        rc = lib.sgpr_applymap_nd_host(*a.values())
        assert rc == (0 if sympgpr_amd.device_count() > 0 else L.E_NODEVICE)


def test_handle_entry_argument_errors_come_before_any_device_call():
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    fn = lib.sgpr_fit_applymap_nd
    ntest, nm, d = 3, 2, 2
    Q0, P0 = np.zeros((ntest, d), order="F"), np.zeros((ntest, d), order="F")
    q, p = np.zeros((nm, ntest, d)), np.zeros((nm, ntest, d))
    good = dict(f=None, mode=0, nm=nm, ntest=ntest, Q0=L.dptr(Q0), ldq=ntest, P0=L.dptr(P0), ldp=ntest, qmap=L.dptr(q),
                pmap=L.dptr(p), iters=None)
    assert fn(*good.values()) == L.E_ARG                    # null handle
    assert b"fit_applymap_nd" in lib.sgpr_last_error()
    for over in (dict(mode=2), dict(nm=0), dict(Q0=None), dict(ldq=2)):      # ... whatever else is wrong with the call
        assert fn(*dict(good, **over).values()) == L.E_ARG


def test_python_wrappers_validate_shapes():
    from sympgpr_amd import maps
    from sympgpr_amd.fit import SympFit
    assert callable(SympFit.applymap_pairs) and "Newton" in SympFit.applymap_pairs.__doc__
    hyp, X, alpha = [1.2, 1.2, 1.5, 1.5, 1.0], np.zeros((4, 4)), np.zeros(16)
    Q0, P0 = np.zeros((3, 2)), np.zeros((3, 2))
    bad = [dict(d=4, X=np.zeros((4, 8)), alpha=np.zeros(32)), dict(X=np.zeros((4, 6))), dict(X=np.zeros(16)),
           dict(alpha=np.zeros(15)), dict(Q0=np.zeros(3)), dict(Q0=np.zeros((3, 3))), dict(P0=np.zeros((2, 2))),
           dict(mode=maps.WRAP_P), dict(mode=maps.LOSS_NEGP), dict(nm=0)]
    for over in bad:
        a = dict(family="A", d=2, mode=maps.WRAP_Q, nm=3, hyp=hyp, X=X, alpha=alpha, Q0=Q0, P0=P0)
        a.update(over)
        with pytest.raises(ValueError):
            maps.run_map_nd(**a)
    # (Ntest,) start points are for d = 1 only
    q, p = maps.start_points_nd(np.zeros(3), np.zeros(3), 1)
    assert q.shape == p.shape == (3, 1) and q.flags.f_contiguous
    with pytest.raises(ValueError):
        maps.start_points_nd(np.zeros(3), np.zeros(3), 2)
    nm, qm, pm, it = maps.map_outputs_nd(4, 3, 2)
    assert qm.shape == pm.shape == (4, 3, 2) and it.shape == (3, 3) and it.dtype == np.int32
