"""The boundary of the batched d-pair NLL gradient (sgpr_fit_batch_nd_grad, fit.fit_batch_pairs_grad, func.nll_chol_pairs_grad[_batch])
that needs no device: every argument error of the C entry returns SGPR_E_ARG before a device is asked for, the symbol is exported
under ABI 5, the arena layout of its two paths equals the formulas restated here, the Python wrappers refuse wrong shapes, and the
wrappers hand the library the documented layout and apply the documented signs and NaN / +inf rows."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import c_header

LEAF, BMAX, PER_WG = 128, 256, 98816          # leaf order, largest one-launch order, scratch doubles per workgroup of a plain fit
GT, GCJ, GPART_ND = 256, 64, 16                # mid gradient: rows / column points per workgroup, doubles per d-pair partial
FIT, GRAD, LOO, LOOGRAD = 0, 1, 2, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from sympgpr_amd import _lib as L
    return L, L.load_library()


def _call(lib, L, family=0, d=2, nbatch=2, n_pts=5, nhyp=None, flags=0, null=()):
    """sgpr_fit_batch_nd_grad with well-formed buffers for (d, nbatch, n_pts); `null`: the arguments passed as NULL"""
    D = 2 * d if 1 <= d <= 3 else 2
    nb, npt = max(nbatch, 1), max(n_pts, 1)
    nh = nhyp if nhyp is not None else (3 * d + 1 if family == 3 else 2 * d + 1)
    bufs = dict(X=np.ones(nb * D * npt), z=np.ones(nb * D * npt), hyp=np.ones(nb * max(nh, 1)), sig2n=np.full(nb, 1e-2),
                alpha=np.zeros(nb * D * npt), nll=np.zeros(nb), grad=np.zeros(nb * (max(nh, 1) + 1)))
    info = np.zeros(nb, dtype=np.int32)
    p = {k: (None if k in null else L.dptr(v)) for k, v in bufs.items()}
    pinfo = None if "info" in null else info.ctypes.data_as(C.POINTER(C.c_int))
    return lib.sgpr_fit_batch_nd_grad(family, d, nbatch, n_pts, p["X"], p["z"], p["hyp"], nh, p["sig2n"], flags, p["alpha"],
                                      p["nll"], p["grad"], pinfo)


@pytest.mark.parametrize("kw", [
    dict(d=0), dict(d=4), dict(d=-1),
    dict(family=-1), dict(family=5),
    dict(nhyp=4), dict(nhyp=7), dict(family=3, nhyp=5), dict(d=3, nhyp=5), dict(d=1, nhyp=5),
    dict(flags=1), dict(flags=2),
    dict(nbatch=-1), dict(n_pts=0), dict(n_pts=-3),
    dict(d=2, n_pts=513), dict(d=3, n_pts=342), dict(d=1, n_pts=1025),
    dict(null=("X",)), dict(null=("z",)), dict(null=("hyp",)), dict(null=("sig2n",)), dict(null=("nll",)), dict(null=("info",)),
    dict(null=("grad",)),
])
def test_every_argument_error_returns_before_a_device_is_needed(kw):
    L, lib = _lib()
    assert _call(lib, L, **kw) == L.E_ARG
    assert b"fit_batch_nd_grad" in lib.sgpr_last_error()


def test_an_order_check_names_the_limit_and_an_empty_batch_returns_zero():
    L, lib = _lib()
    assert lib.sgpr_fit_batch_max_order() == 2048
    assert _call(lib, L, d=2, n_pts=513) == L.E_ARG
    assert b"2052" in lib.sgpr_last_error() and b"2048" in lib.sgpr_last_error()
    assert _call(lib, L, nbatch=0) == 0                      # nothing to do: no device call either
    assert _call(lib, L, nbatch=0, null=("alpha",)) == 0


def test_abi_and_export():
    L, lib = _lib()
    assert lib.sgpr_abi_version() == 5
    c_header.assert_bound_as_declared("sgpr_fit_batch_nd_grad")
    assert c_header.in_exports_map("sgpr_fit_batch_nd_grad")


# ---- the arena layout for mode = GRAD with d > 0, against the formulas restated here

def up256(b):
    return (b + 255) // 256 * 256


def probe(path, mode, d, reg, nbatch, npts, nhyp):
    from sympgpr_amd import _lib as L
    out = (C.c_ulonglong * 24)()
    L.check(L.load_probe_library().sgpr_probe_batch_layout(path, mode, d, reg, nbatch, npts, nhyp, out))
    names = ("chunk nacc o_x o_y o_z o_kc o_no in_bytes o_al o_nll o_info out_bytes o_A o_inv o_fl o_fl2 o_r o_pub o_st o_part "
             "scr_bytes kconst ndconst flag_bytes").split()
    return dict(zip(names, (int(t) for t in out)))


def regions(starts, needs, total):
    """(start, need) in order -> the checks of one block: aligned, in order, disjoint, large enough"""
    for s in starts:
        assert s % 256 == 0
    ends = list(starts[1:]) + [total]
    for s, e, need in zip(starts, ends, needs):
        assert s <= e and e - s >= need
    assert total % 256 == 0


def check_grad_layout(path, d, nbatch, npts, nhyp, cap=0):
    got = probe(path, GRAD, d, 0, nbatch, npts, nhyp)
    n = 2 * d * npts
    nacc = nhyp + 1
    if path == 0:
        chunk = nbatch
    else:
        npad = -(-n // LEAF) * LEAF
        W = npad // LEAF
        img = npad * npad * 8
        chunk = min(nbatch, max(-(-256 // W), (2 << 30) // (2 * img)), 16384)      # two images per problem
        if cap > 0:
            chunk = min(chunk, cap)
    c = chunk
    assert got["chunk"] == chunk and got["nacc"] == nacc
    # input block: X | (no y) | z | NdConst | noise
    needs_in = [c * 2 * d * npts * 8, 0, c * n * 8, c * got["ndconst"], c * 8]
    regions([got[k] for k in ("o_x", "o_y", "o_z", "o_kc", "o_no")], needs_in, got["in_bytes"])
    assert got["o_x"] == 0 and got["in_bytes"] == sum(up256(b) for b in needs_in)
    # output block: alpha | nll + nacc sums per problem | info
    needs_out = [c * n * 8, c * (1 + nacc) * 8, c * 4]
    regions([got[k] for k in ("o_al", "o_nll", "o_info")], needs_out, got["out_bytes"])
    assert got["o_al"] == 0 and got["out_bytes"] == sum(up256(b) for b in needs_out)
    if path == 0:
        assert got["scr_bytes"] == min(nbatch, 1024) * (PER_WG + BMAX * BMAX) * 8
        assert got["flag_bytes"] == 0
        return
    flag = got["flag_bytes"]
    assert flag >= 4 * c
    ggx, ggy = -(-n // GT), -(-npts // GCJ)
    # L images, U images directly behind | leaf inverses | flags of panel 1 | of panel 2 | r | pub | state | partials
    # the partials: GPART_ND doubles per workgroup, wide enough for the 3d + 2 sums of a family with periods
    assert GPART_ND >= 3 * d + 2
    part = c * ggx * ggy * GPART_ND * 8
    needs_scr = [2 * c * img, c * W * LEAF * LEAF * 8, flag, flag, c * npad * 8, 2 * c * npad * 8, c * 8 * 4, part]
    regions([got[k] for k in ("o_A", "o_inv", "o_fl", "o_fl2", "o_r", "o_pub", "o_st", "o_part")], needs_scr, got["scr_bytes"])
    assert got["o_A"] == 0 and (c * img) % 256 == 0          # the U images start at image c of the L images
    assert got["scr_bytes"] == 2 * up256(c * img) + sum(up256(b) for b in needs_scr[1:])


@pytest.mark.parametrize("d,npts", [(2, 64), (3, 42), (1, 128)])
@pytest.mark.parametrize("nbatch", [1, 1024, 1500])
def test_small_path_layout(d, npts, nbatch):
    for nhyp in (2 * d + 1, 3 * d + 1):
        check_grad_layout(0, d, nbatch, npts, nhyp)


@pytest.fixture(params=[0, 2])
def chunk_cap(request):
    """the batch_gradmid_chunk tunable at 0 (none, the built-in value) and 2; back to 0 afterwards"""
    from sympgpr_amd import _lib as L
    tune = L.load_probe_library().sgpr_probe_tune
    L.check(tune(b"batch_gradmid_chunk", float(request.param)))
    yield request.param
    L.check(tune(b"batch_gradmid_chunk", 0.0))


@pytest.mark.parametrize("d,npts", [(3, 43), (2, 160), (3, 171), (2, 512)])
@pytest.mark.parametrize("nbatch", [1, 3, 70])
def test_mid_path_layout(d, npts, nbatch, chunk_cap):
    for nhyp in (2 * d + 1, 3 * d + 1):
        check_grad_layout(1, d, nbatch, npts, nhyp, chunk_cap)


def test_probe_still_refuses_d_pair_loo():
    from sympgpr_amd import _lib as L
    out = (C.c_ulonglong * 24)()
    lib = L.load_probe_library()
    for mode in (LOO, LOOGRAD):
        assert lib.sgpr_probe_batch_layout(0, mode, 2, 0, 4, 20, 5, out) != 0
    assert lib.sgpr_probe_batch_layout(1, LOO, 2, 0, 4, 160, 5, out) != 0
    assert lib.sgpr_probe_batch_layout(0, GRAD, 2, 1, 4, 20, 5, out) != 0         # no scalar-kernel d-pair fit
    assert lib.sgpr_probe_batch_layout(0, GRAD, 2, 0, 4, 65, 5, out) != 0         # order 260 on the one-launch path
    assert lib.sgpr_probe_batch_layout(1, GRAD, 2, 0, 4, 64, 5, out) != 0         # order 256 on the mid path
    assert lib.sgpr_probe_batch_layout(0, GRAD, 2, 0, 4, 20, 5, out) == 0


# ---- the Python wrappers

def test_python_shape_errors():
    from sympgpr_amd import fit, func
    X, hyp = np.ones((3, 5, 4)), np.ones((3, 5))
    bad = [
        lambda: fit.fit_batch_pairs_grad("A", X, np.ones((3, 20)), np.ones(5), 1e-2),              # hyp must have rows
        lambda: fit.fit_batch_pairs_grad("A", np.ones((2, 5, 4)), np.ones((3, 20)), hyp, 1e-2),     # B of X against hyp
        lambda: fit.fit_batch_pairs_grad("A", np.ones((3, 5, 3)), np.ones((3, 15)), hyp, 1e-2),     # odd number of coordinates
        lambda: fit.fit_batch_pairs_grad("A", np.ones(20), np.ones((3, 20)), hyp, 1e-2),            # X with one axis
        lambda: fit.fit_batch_pairs_grad("A", X, np.ones((3, 19)), hyp, 1e-2),                      # z too short
        lambda: fit.fit_batch_pairs_grad("A", X, np.ones((2, 20)), hyp, 1e-2),                      # B of z
        lambda: fit.fit_batch_pairs_grad("A", X, np.ones(21), hyp, 1e-2),                           # broadcast z of the wrong length
        lambda: fit.fit_batch_pairs_grad("A", X, np.ones((3, 20)), hyp, np.ones(2)),                # sig2n of the wrong length
        lambda: func.nll_chol_pairs_grad_batch(np.ones((2, 6)), np.ones((5, 3)), np.ones(15)),
        lambda: func.nll_chol_pairs_grad_batch(np.ones((2, 6)), np.ones((5, 4)), np.ones(19)),
        lambda: func.nll_chol_pairs_grad_batch(np.ones((2, 6)), np.ones(20), np.ones(20)),
        lambda: func.nll_chol_pairs_grad_batch(np.ones((2, 1)), np.ones((5, 4)), np.ones(20)),
        lambda: func.nll_chol_pairs_grad(np.ones((2, 6)), np.ones((5, 4)), np.ones(20)),
        lambda: func.nll_chol_pairs_grad(np.ones(6), np.ones((5, 3)), np.ones(15)),
    ]
    for call in bad:
        with pytest.raises(ValueError):
            call()


class _Recorder:
    """stands in for the loaded library: keeps the buffers sgpr_fit_batch_nd_grad is handed and answers with a pattern"""

    def __init__(self):
        self.calls = []
        self.fail = 1                     # the row that comes back with info > 0 (if the batch has it)

    def sgpr_fit_batch_max_order(self):
        return 2048

    def sgpr_fit_batch_nd_grad(self, family, d, nbatch, n_pts, X, z, hyp, nhyp, sig2n, flags, alpha, nll, grad, info):
        n = 2 * d * n_pts
        self.calls.append(dict(family=family, d=d, nbatch=nbatch, n_pts=n_pts, nhyp=nhyp, flags=flags,
                               X=np.ctypeslib.as_array(X, (nbatch * n,)).copy(), z=np.ctypeslib.as_array(z, (nbatch * n,)).copy(),
                               hyp=np.ctypeslib.as_array(hyp, (nbatch * nhyp,)).copy(),
                               sig2n=np.ctypeslib.as_array(sig2n, (nbatch,)).copy(), alpha=alpha))
        np.ctypeslib.as_array(nll, (nbatch,))[:] = np.arange(nbatch)
        # row b of the gradient: 100 b + k + 1, every entry positive
        np.ctypeslib.as_array(grad, (nbatch, nhyp + 1))[:] = 100.0 * np.arange(nbatch)[:, None] + np.arange(nhyp + 1)[None, :] + 1.0
        if self.fail < nbatch:
            np.ctypeslib.as_array(info, (nbatch,))[self.fail] = 3
        return 0


def test_wrappers_hand_over_the_documented_layout(monkeypatch):
    from sympgpr_amd import _lib as L, fit, func
    rec = _Recorder()
    monkeypatch.setattr(L, "load_library", lambda: rec)
    rng = np.random.default_rng(3)
    n_pts, d, B = 5, 2, 3
    X = rng.standard_normal((n_pts, 2 * d))
    z = rng.standard_normal(2 * d * n_pts)
    hyp = rng.uniform(0.5, 1.5, (B, 2 * d + 1))
    alpha, nll, grad, info = fit.fit_batch_pairs_grad("C", X, z, hyp, 1e-2)
    c = rec.calls[-1]
    assert (c["family"], c["d"], c["nbatch"], c["n_pts"], c["nhyp"], c["flags"]) == (L.FAMILIES["C"], d, B, n_pts, 5, 0)
    assert c["alpha"] is None and alpha is None                 # want_alpha defaults to False
    for b in range(B):
        for m in range(2 * d):
            for i in range(n_pts):
                assert c["X"][(b * 2 * d + m) * n_pts + i] == X[i, m]
        assert np.array_equal(c["z"][b * 20:(b + 1) * 20], z)
    assert np.array_equal(c["hyp"], hyp.ravel()) and np.array_equal(c["sig2n"], np.full(B, 1e-2))
    assert grad.shape == (B, 6)
    assert list(info) == [0, 3, 0] and np.isnan(nll[1]) and np.all(np.isnan(grad[1])) and nll[0] == 0.0 and nll[2] == 2.0
    assert np.array_equal(grad[0], np.arange(6) + 1.0) and np.array_equal(grad[2], 200.0 + np.arange(6) + 1.0)
    # one problem per row: the same layout from (B, n_pts, 2d)
    X3 = rng.standard_normal((B, n_pts, 2 * d))
    al3, _, _, _ = fit.fit_batch_pairs_grad("C", X3, np.tile(z, (B, 1)), hyp, np.array([1e-2, 2e-2, 3e-2]), want_alpha=True)
    c = rec.calls[-1]
    assert c["alpha"] is not None and al3.shape == (B, 20)
    assert np.array_equal(c["X"].reshape(B, 2 * d, n_pts), np.swapaxes(X3, 1, 2)) and list(c["sig2n"]) == [1e-2, 2e-2, 3e-2]
    # the population objective: the last column is the noise, handed over as |.|; its sign multiplies the last gradient column;
    # a failed row is +inf / NaN
    func.set_family("C")
    rows = np.column_stack((hyp, [-1e-3, -2e-3, 3e-3]))
    nlls, grads = func.nll_chol_pairs_grad_batch(rows, X, z)
    c = rec.calls[-1]
    assert np.array_equal(c["hyp"], hyp.ravel()) and list(c["sig2n"]) == [1e-3, 2e-3, 3e-3] and c["alpha"] is None
    assert nlls[1] == np.inf and nlls[0] == 0.0 and nlls[2] == 2.0
    assert np.all(np.isnan(grads[1]))
    assert np.array_equal(grads[0], [1.0, 2.0, 3.0, 4.0, 5.0, -6.0])               # sig2_n < 0: the last entry changes sign
    assert np.array_equal(grads[2], 200.0 + np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]))
    # one row: the same numbers; LinAlgError for the failed row
    v, g = func.nll_chol_pairs_grad(rows[0], X, z)
    assert v == 0.0 and np.array_equal(g, [1.0, 2.0, 3.0, 4.0, 5.0, -6.0])
    rec.fail = 0
    with pytest.raises(np.linalg.LinAlgError):
        func.nll_chol_pairs_grad(rows[0], X, z)
    func.set_family("A")
