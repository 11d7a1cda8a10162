"""The boundary of the batched d-pair fit (sgpr_fit_batch_nd, fit.fit_batch_pairs, func.nll_chol_pairs[_batch]) that needs no
device: every argument error of the C entry returns SGPR_E_ARG before a device is asked for, the Python wrappers refuse wrong
shapes, and the (n_pts, 2d) broadcast hands the library the documented layout."""
import ctypes as C

import numpy as np
import pytest


def _lib():
    from sympgpr_amd import _lib as L
    return L, L.load_library()


def _call(lib, L, family=0, d=2, nbatch=2, n_pts=5, nhyp=None, flags=0, null=()):
    """sgpr_fit_batch_nd with well-formed buffers for (d, nbatch, n_pts); `null`: the arguments passed as NULL"""
    D = 2 * d if 1 <= d <= 3 else 2
    nb, npt = max(nbatch, 1), max(n_pts, 1)
    nh = nhyp if nhyp is not None else (3 * d + 1 if family == 3 else 2 * d + 1)
    bufs = dict(X=np.ones(nb * D * npt), z=np.ones(nb * D * npt), hyp=np.ones(nb * max(nh, 1)), sig2n=np.full(nb, 1e-2),
                alpha=np.zeros(nb * D * npt), nll=np.zeros(nb))
    info = np.zeros(nb, dtype=np.int32)
    p = {k: (None if k in null else L.dptr(v)) for k, v in bufs.items()}
    pinfo = None if "info" in null else info.ctypes.data_as(C.POINTER(C.c_int))
    return lib.sgpr_fit_batch_nd(family, d, nbatch, n_pts, p["X"], p["z"], p["hyp"], nh, p["sig2n"], flags, p["alpha"], p["nll"],
                                 pinfo)


@pytest.mark.parametrize("kw", [
    dict(d=0), dict(d=4), dict(d=-1),
    dict(family=-1), dict(family=5),
    dict(nhyp=4), dict(nhyp=7), dict(family=3, nhyp=5), dict(d=3, nhyp=5), dict(d=1, nhyp=5),
    dict(flags=1), dict(flags=2),
    dict(nbatch=-1), dict(n_pts=0), dict(n_pts=-3),
    dict(d=2, n_pts=513), dict(d=3, n_pts=342), dict(d=1, n_pts=1025),
    dict(null=("X",)), dict(null=("z",)), dict(null=("hyp",)), dict(null=("sig2n",)), dict(null=("nll",)), dict(null=("info",)),
])
def test_every_argument_error_returns_before_a_device_is_needed(kw):
    L, lib = _lib()
    assert _call(lib, L, **kw) == L.E_ARG
    assert b"fit_batch_nd" in lib.sgpr_last_error()


def test_an_order_check_names_the_limit_and_an_empty_batch_returns_zero():
    L, lib = _lib()
    assert lib.sgpr_fit_batch_max_order() == 2048
    assert _call(lib, L, d=2, n_pts=513) == L.E_ARG
    assert b"2052" in lib.sgpr_last_error() and b"2048" in lib.sgpr_last_error()
    assert _call(lib, L, nbatch=0) == 0                      # nothing to do: no device call either
    assert _call(lib, L, nbatch=0, null=("alpha",)) == 0


def test_python_shape_errors():
    from sympgpr_amd import fit, func
    X, hyp = np.ones((3, 5, 4)), np.ones((3, 5))
    bad = [
        lambda: fit.fit_batch_pairs("A", X, np.ones((3, 20)), np.ones(5), 1e-2),              # hyp must have rows
        lambda: fit.fit_batch_pairs("A", np.ones((2, 5, 4)), np.ones((3, 20)), hyp, 1e-2),     # B of X against hyp
        lambda: fit.fit_batch_pairs("A", np.ones((3, 5, 3)), np.ones((3, 15)), hyp, 1e-2),     # odd number of coordinates
        lambda: fit.fit_batch_pairs("A", np.ones(20), np.ones((3, 20)), hyp, 1e-2),            # X with one axis
        lambda: fit.fit_batch_pairs("A", X, np.ones((3, 19)), hyp, 1e-2),                      # z too short
        lambda: fit.fit_batch_pairs("A", X, np.ones((2, 20)), hyp, 1e-2),                      # B of z
        lambda: fit.fit_batch_pairs("A", X, np.ones(21), hyp, 1e-2),                           # broadcast z of the wrong length
        lambda: fit.fit_batch_pairs("A", X, np.ones((3, 20)), hyp, np.ones(2)),                # sig2n of the wrong length
        lambda: func.nll_chol_pairs_batch(np.ones((2, 6)), np.ones((5, 3)), np.ones(15)),
        lambda: func.nll_chol_pairs_batch(np.ones((2, 6)), np.ones((5, 4)), np.ones(19)),
        lambda: func.nll_chol_pairs_batch(np.ones((2, 6)), np.ones(20), np.ones(20)),
        lambda: func.nll_chol_pairs(np.ones((2, 6)), np.ones((5, 4)), np.ones(20)),
    ]
    for call in bad:
        with pytest.raises(ValueError):
            call()


class _Recorder:
    """stands in for the loaded library: keeps the buffers sgpr_fit_batch_nd is handed"""

    def __init__(self):
        self.calls = []

    def sgpr_fit_batch_max_order(self):
        return 2048

    def sgpr_fit_batch_nd(self, family, d, nbatch, n_pts, X, z, hyp, nhyp, sig2n, flags, alpha, nll, info):
        n = 2 * d * n_pts
        self.calls.append(dict(family=family, d=d, nbatch=nbatch, n_pts=n_pts, nhyp=nhyp, flags=flags,
                               X=np.ctypeslib.as_array(X, (nbatch * n,)).copy(), z=np.ctypeslib.as_array(z, (nbatch * n,)).copy(),
                               hyp=np.ctypeslib.as_array(hyp, (nbatch * nhyp,)).copy(),
                               sig2n=np.ctypeslib.as_array(sig2n, (nbatch,)).copy(), alpha=alpha))
        np.ctypeslib.as_array(nll, (nbatch,))[:] = np.arange(nbatch)
        np.ctypeslib.as_array(info, (nbatch,))[1] = 3
        return 0


def test_broadcast_lays_X_out_as_documented(monkeypatch):
    from sympgpr_amd import _lib as L, fit, func
    rec = _Recorder()
    monkeypatch.setattr(L, "load_library", lambda: rec)
    rng = np.random.default_rng(3)
    n_pts, d, B = 5, 2, 3
    X = rng.standard_normal((n_pts, 2 * d))
    z = rng.standard_normal(2 * d * n_pts)
    hyp = rng.uniform(0.5, 1.5, (B, 2 * d + 1))
    alpha, nll, info = fit.fit_batch_pairs("C", X, z, hyp, 1e-2, want_alpha=False)
    c = rec.calls[-1]
    assert (c["family"], c["d"], c["nbatch"], c["n_pts"], c["nhyp"], c["flags"]) == (L.FAMILIES["C"], d, B, n_pts, 5, 0)
    assert c["alpha"] is None and alpha is None
    for b in range(B):
        for m in range(2 * d):
            for i in range(n_pts):
                assert c["X"][(b * 2 * d + m) * n_pts + i] == X[i, m]
        assert np.array_equal(c["z"][b * 20:(b + 1) * 20], z)
    assert np.array_equal(c["hyp"], hyp.ravel()) and np.array_equal(c["sig2n"], np.full(B, 1e-2))
    assert list(info) == [0, 3, 0] and np.isnan(nll[1]) and nll[0] == 0.0 and nll[2] == 2.0
    # one problem per row: the same layout from (B, n_pts, 2d)
    X3 = rng.standard_normal((B, n_pts, 2 * d))
    fit.fit_batch_pairs("C", X3, np.tile(z, (B, 1)), hyp, np.array([1e-2, 2e-2, 3e-2]))
    c = rec.calls[-1]
    assert c["alpha"] is not None
    assert np.array_equal(c["X"].reshape(B, 2 * d, n_pts), np.swapaxes(X3, 1, 2)) and list(c["sig2n"]) == [1e-2, 2e-2, 3e-2]
    # the population objective: the last column is the noise, its sign dropped; a failed row is +inf
    func.set_family("C")
    rows = np.column_stack((hyp, [1e-3, -2e-3, 3e-3]))
    got = func.nll_chol_pairs_batch(rows, X, z)
    c = rec.calls[-1]
    assert np.array_equal(c["hyp"], hyp.ravel()) and list(c["sig2n"]) == [1e-3, 2e-3, 3e-3] and c["alpha"] is None
    assert got[1] == np.inf and got[0] == 0.0 and got[2] == 2.0
