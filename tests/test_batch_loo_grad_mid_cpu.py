"""The boundary of the batched leave-one-point-out gradient of orders 257 to 2048 (sgpr_fit_batch_loo_grad_mid,
sgpr_fit_batch_nd_loo_grad_mid, fit.fit_batch_loo_grad_mid, fit.fit_batch_pairs_loo_grad_mid and the mid keyword of
func.loo_chol_grad_batch / func.loo_chol_pairs_grad_batch) that needs no device: every argument error of the two C entries returns
SGPR_E_ARG before a device is asked for, the symbols are exported under ABI 5, the arena layout of the mode
(sgpr_probe_batch_layout_loograd_mid) equals the formulas restated here, and the Python wrappers make exactly one call of the new
entry under mid="device", keep their slow path under mid=None and apply the siblings' sign and NaN conventions."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import c_header

LEAF = 128
GT, GCJ, GPART, GPART_ND = 256, 64, 8, 16      # contraction: rows and column points per workgroup, doubles per partial
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XY, ND = "sgpr_fit_batch_loo_grad_mid", "sgpr_fit_batch_nd_loo_grad_mid"


def _lib():
    from sympgpr_amd import _lib as L
    return L, L.load_library()


def _call(lib, L, entry, family=0, d=2, nbatch=2, n_pts=None, nhyp=None, flags=0, which=0, null=()):
    """one of the two entries with well-formed buffers; `null`: the arguments passed as NULL.  The default n_pts gives order 260."""
    nd = entry == ND
    if n_pts is None:
        n_pts = 130 if not nd else {1: 130, 2: 65, 3: 44}.get(d, 65)
    D = (2 * d if 1 <= d <= 3 else 2) if nd else 2
    nb, npt = max(nbatch, 1), max(n_pts, 1)
    if nhyp is None:
        nhyp = (3 * d + 1 if family == 3 else 2 * d + 1) if nd else (4 if family == 3 else 3)
    nh = max(nhyp, 1)
    bufs = dict(X=np.ones(nb * D * npt), y=np.ones(nb * npt), z=np.ones(nb * D * npt), hyp=np.ones(nb * nh), sig2n=np.full(nb, 1e-2),
                alpha=np.zeros(nb * D * npt), nll=np.zeros(nb), value=np.zeros(nb), grad=np.zeros(nb * (nh + 1)))
    info = np.zeros(nb, dtype=np.int32)
    p = {k: (None if k in null else L.dptr(v)) for k, v in bufs.items()}
    pinfo = None if "info" in null else info.ctypes.data_as(C.POINTER(C.c_int))
    tail = (p["z"], p["hyp"], nhyp, p["sig2n"], flags, which, p["alpha"], p["nll"], p["value"], p["grad"], pinfo)
    if nd:
        return lib.sgpr_fit_batch_nd_loo_grad_mid(family, d, nbatch, n_pts, p["X"], *tail)
    return lib.sgpr_fit_batch_loo_grad_mid(family, nbatch, n_pts, p["X"], p["y"], *tail)


COMMON = [
    dict(family=-1), dict(family=5),
    dict(which=2), dict(which=-1),
    dict(nbatch=-1), dict(n_pts=0), dict(n_pts=-3),
    dict(null=("X",)), dict(null=("z",)), dict(null=("hyp",)), dict(null=("sig2n",)), dict(null=("nll",)), dict(null=("value",)),
    dict(null=("grad",)), dict(null=("info",)),
]


@pytest.mark.parametrize("kw", COMMON + [
    dict(nhyp=4), dict(nhyp=2), dict(family=3, nhyp=3),
    dict(flags=1), dict(flags=2), dict(flags=8),
    dict(n_pts=128), dict(n_pts=64), dict(n_pts=256, flags=4),                           # orders 256, 128, reg 256
    dict(n_pts=1025), dict(n_pts=2049, flags=4),                                         # orders 2050, reg 2049
    dict(null=("y",)),
])
def test_every_argument_error_of_the_xy_entry_returns_before_a_device_is_needed(kw):
    L, lib = _lib()
    assert _call(lib, L, XY, **kw) == L.E_ARG
    assert b"fit_batch_loo_grad_mid:" in lib.sgpr_last_error()


@pytest.mark.parametrize("kw", COMMON + [
    dict(d=0), dict(d=4), dict(d=-1),
    dict(nhyp=4), dict(nhyp=7), dict(family=3, nhyp=5), dict(d=3, nhyp=5), dict(d=1, nhyp=5),
    dict(flags=1), dict(flags=4),
    dict(d=2, n_pts=64), dict(d=3, n_pts=42), dict(d=1, n_pts=128),                      # orders 256, 252, 256
    dict(d=2, n_pts=513), dict(d=3, n_pts=342), dict(d=1, n_pts=1025),                   # orders 2052, 2052, 2050
])
def test_every_argument_error_of_the_nd_entry_returns_before_a_device_is_needed(kw):
    L, lib = _lib()
    assert _call(lib, L, ND, **kw) == L.E_ARG
    assert b"fit_batch_nd_loo_grad_mid:" in lib.sgpr_last_error()


def test_the_order_checks_name_the_order_and_the_limit_and_an_empty_batch_returns_zero():
    L, lib = _lib()
    assert lib.sgpr_fit_batch_max_order() == 2048
    for entry, low, high in ((XY, dict(n_pts=128), dict(n_pts=1026)), (ND, dict(d=2, n_pts=64), dict(d=2, n_pts=513))):
        assert _call(lib, L, entry, **low) == L.E_ARG
        msg = lib.sgpr_last_error()
        assert msg.count(b"256") >= 2, msg                                   # the order (256) and the limit (256)
        assert _call(lib, L, entry, **high) == L.E_ARG
        msg = lib.sgpr_last_error()
        assert b"2052" in msg and b"2048" in msg, msg
        assert _call(lib, L, entry, nbatch=0) == 0                           # nothing to do: no device call either
        assert _call(lib, L, entry, nbatch=0, null=("alpha",)) == 0
    assert _call(lib, L, XY, n_pts=257, flags=4, nbatch=0) == 0              # reg 257 is in range
    assert _call(lib, L, XY, n_pts=256, flags=4) == L.E_ARG and b"256" in lib.sgpr_last_error()


def test_the_existing_entries_keep_refusing_orders_above_256():
    L, lib = _lib()
    nb, npt = 2, 130
    one = lambda k: L.dptr(np.ones(k))
    info = np.zeros(nb, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    assert lib.sgpr_fit_batch_loo_grad(0, nb, npt, one(nb * npt), one(nb * npt), one(2 * nb * npt), one(3 * nb), 3, one(nb), 0, 0,
                                       None, one(nb), one(nb), one(4 * nb), info) == L.E_ARG
    assert lib.sgpr_fit_batch_nd_loo_grad(0, 2, nb, 65, one(4 * nb * 65), one(4 * nb * 65), one(5 * nb), 5, one(nb), 0, 0,
                                          None, one(nb), one(nb), one(6 * nb), info) == L.E_ARG


def test_abi_and_exports():
    L, lib = _lib()
    assert lib.sgpr_abi_version() == 5 and L.ABI_VERSION == 5
    for entry in (XY, ND):
        c_header.assert_bound_as_declared(entry)
        assert c_header.in_exports_map(entry), entry
    assert len(L.SIGNATURES[XY][1]) == len(L.SIGNATURES["sgpr_fit_batch_loo_grad"][1])
    assert len(L.SIGNATURES[ND][1]) == len(L.SIGNATURES["sgpr_fit_batch_nd_loo_grad"][1])
    c_header.assert_bound_as_declared("sgpr_probe_batch_layout_loograd_mid", probe=True)


# ---- the arena layout of the mode, against formulas restated here

def up256(b):
    return (b + 255) // 256 * 256


NAMES = ("chunk nacc o_x o_y o_z o_kc o_no in_bytes o_al o_nll o_info out_bytes o_A o_inv o_fl o_fl2 o_r o_pub o_st o_part "
         "scr_bytes kconst ndconst flag_bytes o_lpart o_wt o_v o_beta o_zero npad nimg spare").split()


def probe(d, reg, nbatch, npts, nhyp):
    from sympgpr_amd import _lib as L
    out = (C.c_ulonglong * 32)()
    L.check(L.load_probe_library().sgpr_probe_batch_layout_loograd_mid(d, reg, nbatch, npts, nhyp, out))
    return dict(zip(NAMES, (int(t) for t in out)))


def regions(starts, needs, total):
    """(start, need) in order -> the checks of one block: aligned, in order, disjoint, large enough"""
    for s in starts:
        assert s % 256 == 0
    ends = list(starts[1:]) + [total]
    for s, e, need in zip(starts, ends, needs):
        assert s <= e and e - s >= need, (s, e, need)
    assert total % 256 == 0


def check_layout(d, reg, nbatch, npts, nhyp, cap=0):
    got = probe(d, reg, nbatch, npts, nhyp)
    D = 2 * d if d else 1 if reg else 2
    n = D * npts
    npad = -(-n // LEAF) * LEAF
    W = npad // LEAF
    img = npad * npad * 8
    chunk = min(nbatch, max(-(-256 // W), (2 << 30) // (3 * img)), 16384)              # three images per problem
    if cap > 0:
        chunk = min(chunk, cap)
    c = chunk
    assert got["chunk"] == chunk and got["nacc"] == nhyp + 3 and got["npad"] == npad and got["nimg"] == 3
    # input block: x | y | z | consts | noise (d > 0: X, no y, NdConst)
    xb, yb = (2 * d * npts * 8, 0) if d else (npts * 8, npts * 8)
    needs_in = [c * xb, c * yb, c * n * 8, c * (got["ndconst"] if d else got["kconst"]), c * 8]
    regions([got[k] for k in ("o_x", "o_y", "o_z", "o_kc", "o_no")], needs_in, got["in_bytes"])
    assert got["o_x"] == 0 and got["in_bytes"] == sum(up256(b) for b in needs_in)
    # output block: alpha | nll + {loo, press, nhyp + 1 sums} per problem | info
    needs_out = [c * n * 8, c * (1 + nhyp + 3) * 8, c * 4]
    regions([got[k] for k in ("o_al", "o_nll", "o_info")], needs_out, got["out_bytes"])
    assert got["o_al"] == 0 and got["out_bytes"] == sum(up256(b) for b in needs_out)
    flag = got["flag_bytes"]
    assert flag >= 4 * c
    ggx, ggy, lnwg = -(-n // GT), -(-npts // GCJ), -(-npts // GT)
    gpart = c * ggx * ggy * (GPART_ND if d else GPART) * 8
    assert (GPART_ND if d else GPART) >= nhyp + 1
    T = D * (D + 1) // 2
    # L, U and M images one behind the other | leaf inverses | flags of panel 1 | of panel 2 | r | pub | state | the contraction's
    # partials | the point pass's partials | W~ | v | beta | zeros
    needs_scr = [3 * c * img, c * W * LEAF * LEAF * 8, flag, flag, c * npad * 8, 2 * c * npad * 8, c * 8 * 4, gpart, c * lnwg * 2 * 8,
                 c * T * npts * 8, c * npad * 8, c * npad * 8, c * npad * 8]
    keys = ("o_A", "o_inv", "o_fl", "o_fl2", "o_r", "o_pub", "o_st", "o_part", "o_lpart", "o_wt", "o_v", "o_beta", "o_zero")
    regions([got[k] for k in keys], needs_scr, got["scr_bytes"])
    assert got["o_A"] == 0 and (c * img) % 256 == 0          # image set k starts at image k c of the L images
    assert got["scr_bytes"] == 3 * up256(c * img) + sum(up256(b) for b in needs_scr[1:])
    assert 3 * c * img <= max(2 << 30, 3 * img * -(-256 // W))


@pytest.fixture(params=[0, 2])
def chunk_cap(request):
    """the batch_gradmid_chunk tunable at 0 (none, the built-in value) and 2; back to 0 afterwards"""
    from sympgpr_amd import _lib as L
    tune = L.load_probe_library().sgpr_probe_tune
    L.check(tune(b"batch_gradmid_chunk", float(request.param)))
    yield request.param
    L.check(tune(b"batch_gradmid_chunk", 0.0))


@pytest.mark.parametrize("d,reg,npts", [(1, 0, 129), (2, 0, 300), (3, 0, 171), (2, 0, 512), (0, 1, 257), (0, 0, 129), (0, 0, 1024)])
@pytest.mark.parametrize("nbatch", [1, 3, 70])
def test_mid_path_layout(d, reg, npts, nbatch, chunk_cap):
    for nhyp in ((2 * d + 1, 3 * d + 1) if d else (3, 4)):
        check_layout(d, reg, nbatch, npts, nhyp, chunk_cap)


def test_chunk_of_the_maximum_order():
    assert probe(0, 0, 70, 1024, 3)["chunk"] == 21           # 2 GiB / (3 x 32 MiB)
    assert probe(2, 0, 70, 65, 5)["chunk"] == 70             # order 260: W = 3, 1.2 MiB per image


def test_probes_refuse_what_the_entries_refuse():
    from sympgpr_amd import _lib as L
    P = L.load_probe_library()
    out = (C.c_ulonglong * 32)()
    new = P.sgpr_probe_batch_layout_loograd_mid
    assert new(2, 0, 4, 64, 5, out) != 0 and new(0, 0, 4, 128, 3, out) != 0 and new(0, 1, 4, 256, 3, out) != 0      # order 256
    assert new(2, 0, 4, 513, 5, out) != 0 and new(0, 0, 4, 1026, 3, out) != 0                                       # order 2052
    assert new(4, 0, 4, 40, 9, out) != 0 and new(-1, 0, 4, 200, 3, out) != 0 and new(2, 1, 4, 100, 5, out) != 0
    assert new(2, 0, 0, 100, 5, out) != 0 and new(2, 0, 4, 100, 5, None) != 0
    assert new(2, 0, 4, 65, 5, out) == 0 and new(0, 1, 4, 257, 3, out) == 0 and new(3, 0, 4, 341, 7, out) == 0
    # the two older probes keep refusing (path 1, loo gradient)
    old = (C.c_ulonglong * 24)()
    assert P.sgpr_probe_batch_layout(1, 3, 0, 0, 4, 150, 3, old) != 0
    assert P.sgpr_probe_batch_layout_nd_loo(1, 3, 2, 4, 160, 5, old) != 0


# ---- the Python wrappers, with a stand-in for the loaded library

class _Recorder:
    """stands in for the loaded library: records the calls of the batched entries and answers with a pattern"""

    def __init__(self):
        self.calls = []
        self.fail = 1                     # the row that comes back with info > 0 (if the batch has it)

    def sgpr_fit_batch_max_order(self):
        return 2048

    def _answer(self, entry, nbatch, nhyp, sig2n, which, nll, info, value=None, grad=None, loo=None):
        self.calls.append(dict(entry=entry, nbatch=nbatch, nhyp=nhyp, which=which, sig2n=np.ctypeslib.as_array(sig2n, (nbatch,)).copy()))
        np.ctypeslib.as_array(nll, (nbatch,))[:] = np.arange(nbatch)
        if value is not None:
            np.ctypeslib.as_array(value, (nbatch,))[:] = 10.0 * np.arange(nbatch) + 1.0 + which
            # row b of the gradient: 100 b + k + 1, every entry positive; the library applies the sign of sig2n itself (x | y entries)
            g = np.ctypeslib.as_array(grad, (nbatch, nhyp + 1))
            g[:] = 100.0 * np.arange(nbatch)[:, None] + np.arange(nhyp + 1)[None, :] + 1.0
        if loo is not None:
            np.ctypeslib.as_array(loo, (nbatch, 2))[:] = 10.0 * np.arange(nbatch)[:, None] + np.array([1.0, 2.0])[None, :]
        if self.fail < nbatch:
            np.ctypeslib.as_array(info, (nbatch,))[self.fail] = 3
        return 0

    def sgpr_fit_batch_loo_grad_mid(self, family, nbatch, n_pts, x, y, z, hyp, nhyp, sig2n, flags, which, alpha, nll, value, grad, info):
        return self._answer("xy_mid", nbatch, nhyp, sig2n, which, nll, info, value, grad)

    def sgpr_fit_batch_loo_grad(self, family, nbatch, n_pts, x, y, z, hyp, nhyp, sig2n, flags, which, alpha, nll, value, grad, info):
        return self._answer("xy_small", nbatch, nhyp, sig2n, which, nll, info, value, grad)

    def sgpr_fit_batch_loo(self, family, nbatch, n_pts, x, y, z, hyp, nhyp, sig2n, flags, alpha, nll, loo, info):
        return self._answer("xy_loo", nbatch, nhyp, sig2n, None, nll, info, loo=loo)

    def sgpr_fit_batch_nd_loo_grad_mid(self, family, d, nbatch, n_pts, X, z, hyp, nhyp, sig2n, flags, which, alpha, nll, value, grad,
                                       info):
        return self._answer("nd_mid", nbatch, nhyp, sig2n, which, nll, info, value, grad)

    def sgpr_fit_batch_nd_loo_grad(self, family, d, nbatch, n_pts, X, z, hyp, nhyp, sig2n, flags, which, alpha, nll, value, grad, info):
        return self._answer("nd_small", nbatch, nhyp, sig2n, which, nll, info, value, grad)

    def sgpr_fit_batch_nd_loo(self, family, d, nbatch, n_pts, X, z, hyp, nhyp, sig2n, flags, alpha, nll, loo, info):
        return self._answer("nd_loo", nbatch, nhyp, sig2n, None, nll, info, loo=loo)


class _Handle:
    """stands in for SympFit and SympFit.pairs: counts the handles created"""
    created = 0

    def __init__(self, family, x, y, z, hyp, sig2n, reg=False):
        type(self).created += 1
        self.ngrad = len(hyp) + 1

    @classmethod
    def pairs(cls, family, X, z, hyp, sig2n):
        return cls(family, None, None, z, hyp, sig2n)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def set_hyp(self, hyp, sig2n):
        pass

    def run(self):
        return self

    def loo_grad(self, objective="loo"):
        return 5.0, np.full(self.ngrad, 7.0)


def _xy(npts, B, seed=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(2 * npts), rng.standard_normal(2 * npts), rng.uniform(0.5, 1.5, (B, 3))


def test_fit_functions_call_the_new_entries_and_refuse_small_orders(monkeypatch):
    from sympgpr_amd import _lib as L, fit
    rec = _Recorder()
    monkeypatch.setattr(L, "load_library", lambda: rec)
    B, npts = 3, 130
    xx, z, hyp = _xy(npts, B)
    rep = lambda a: np.tile(a, (B, 1))
    for objective, which in (("loo", L.LOO_LPD), ("press", L.LOO_PRESS)):
        alpha, nll, value, grad, info = fit.fit_batch_loo_grad_mid("C", rep(xx[:npts]), rep(xx[npts:]), rep(z), hyp, 1e-2,
                                                                   objective=objective)
        c = rec.calls[-1]
        assert c["entry"] == "xy_mid" and c["which"] == which and c["nbatch"] == B
        assert alpha is None and value.shape == (B,) and grad.shape == (B, 4) and list(info) == [0, 3, 0]
        assert value[0] == 1.0 + which and value[2] == 21.0 + which and np.array_equal(grad[2], 200.0 + np.arange(4) + 1.0)
        X = np.ones((65, 4))
        alpha, nll, value, grad, info = fit.fit_batch_pairs_loo_grad_mid("C", X, np.ones(260), np.ones((B, 5)), 1e-2, objective=objective)
        c = rec.calls[-1]
        assert c["entry"] == "nd_mid" and c["which"] == which and c["nbatch"] == B
        assert alpha is None and list(info) == [0, 3, 0]
        assert np.isnan(nll[1]) and np.isnan(value[1]) and np.all(np.isnan(grad[1]))          # the d-pair wrappers blank failed rows
        assert value[0] == 1.0 + which and np.array_equal(grad[2], 200.0 + np.arange(6) + 1.0)
    n0 = len(rec.calls)
    with pytest.raises(ValueError):
        fit.fit_batch_loo_grad_mid("C", np.ones((B, 128)), np.ones((B, 128)), np.ones((B, 256)), hyp, 1e-2)             # order 256
    with pytest.raises(ValueError):
        fit.fit_batch_loo_grad_mid("C", np.ones((B, 256)), np.ones((B, 256)), np.ones((B, 256)), hyp, 1e-2, reg=True)   # reg 256
    with pytest.raises(ValueError):
        fit.fit_batch_pairs_loo_grad_mid("C", np.ones((64, 4)), np.ones(256), np.ones((B, 5)), 1e-2)                    # order 256
    with pytest.raises(ValueError):
        fit.fit_batch_loo_grad_mid("C", rep(xx[:npts]), rep(xx[npts:]), rep(z), hyp, 1e-2, objective="nll")
    with pytest.raises(ValueError):
        fit.fit_batch_pairs_loo_grad_mid("C", np.ones((65, 4)), np.ones(260), np.ones((B, 5)), 1e-2, objective="nll")
    assert len(rec.calls) == n0


def test_func_mid_device_makes_one_call_and_no_handle(monkeypatch):
    from sympgpr_amd import _lib as L, fit, func
    rec = _Recorder()
    monkeypatch.setattr(L, "load_library", lambda: rec)
    monkeypatch.setattr(fit, "SympFit", _Handle)
    monkeypatch.setattr(func, "SympFit", _Handle)
    func.set_family("C")
    try:
        B, npts = 3, 130
        xx, z, hyp = _xy(npts, B)
        rows = np.column_stack((hyp, [-1e-3, 2e-3, 3e-3]))
        for objective, which in (("loo", 0), ("press", 1)):
            # x | y, mid="device": one call of the new entry, no handle; the library is handed sig2_n with its sign
            _Handle.created, n0 = 0, len(rec.calls)
            v, g = func.loo_chol_grad_batch(rows, xx, z, 2 * npts, objective=objective, mid="device")
            assert [c["entry"] for c in rec.calls[n0:]] == ["xy_mid"] and _Handle.created == 0
            assert rec.calls[-1]["which"] == which and list(rec.calls[-1]["sig2n"]) == [-1e-3, 2e-3, 3e-3]
            assert v[0] == 1.0 + which and v[2] == 21.0 + which and np.array_equal(g[2], 200.0 + np.arange(4) + 1.0)
            # mid=None: the values from one fit_batch_loo call, a handle per row with info == 0
            _Handle.created, n0 = 0, len(rec.calls)
            v, g = func.loo_chol_grad_batch(rows, xx, z, 2 * npts, objective=objective)
            assert [c["entry"] for c in rec.calls[n0:]] == ["xy_loo"] and _Handle.created == 2
            assert v[0] == 1.0 + which and np.all(np.isnan(g[1])) and np.array_equal(g[0], np.full(4, 7.0))      # (the library blanks v[1])
            # d pairs, mid="device": one call, no handle; |sig2_n| goes in, its sign multiplies the last column; NaN rows
            X, zz, hh = np.ones((65, 4)), np.ones(260), np.column_stack((np.ones((B, 5)), [-1e-3, 2e-3, 3e-3]))
            _Handle.created, n0 = 0, len(rec.calls)
            v, g = func.loo_chol_pairs_grad_batch(hh, X, zz, objective=objective, mid="device")
            assert [c["entry"] for c in rec.calls[n0:]] == ["nd_mid"] and _Handle.created == 0
            assert rec.calls[-1]["which"] == which and list(rec.calls[-1]["sig2n"]) == [1e-3, 2e-3, 3e-3]
            assert v[0] == 1.0 + which and np.isnan(v[1]) and np.all(np.isnan(g[1])) and v[2] == 21.0 + which
            assert np.array_equal(g[0], [1.0, 2.0, 3.0, 4.0, 5.0, -6.0]) and np.array_equal(g[2], 200.0 + np.arange(6) + 1.0)
            # mid=None: unchanged
            _Handle.created, n0 = 0, len(rec.calls)
            func.loo_chol_pairs_grad_batch(hh, X, zz, objective=objective)
            assert [c["entry"] for c in rec.calls[n0:]] == ["nd_loo"] and _Handle.created == 2
        # at or below order 256 "device" changes nothing: the one-launch entries
        n0 = len(rec.calls)
        func.loo_chol_grad_batch(rows, xx[np.r_[0:50, npts:npts + 50]], z[:100], 100, mid="device")
        func.loo_chol_pairs_grad_batch(np.ones((B, 6)), np.ones((20, 4)), np.ones(80), mid="device")
        assert [c["entry"] for c in rec.calls[n0:]] == ["xy_small", "nd_small"]
        # above order 2048 the d-pair wrapper keeps its single-handle loop under either setting
        for mid in (None, "device"):
            _Handle.created, n0 = 0, len(rec.calls)
            func.loo_chol_pairs_grad_batch(np.ones((B, 6)), np.ones((513, 4)), np.ones(2052), mid=mid)
            assert len(rec.calls) == n0 and _Handle.created == 1
        for bad in ("host", 1, True):
            with pytest.raises(ValueError):
                func.loo_chol_grad_batch(rows, xx, z, 2 * npts, mid=bad)
            with pytest.raises(ValueError):
                func.loo_chol_pairs_grad_batch(np.ones((B, 6)), np.ones((65, 4)), np.ones(260), mid=bad)
    finally:
        func.set_family("A")
