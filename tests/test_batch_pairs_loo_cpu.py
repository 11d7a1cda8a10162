"""The boundary of the batched d-pair leave-one-point-out entries (sgpr_fit_batch_nd_loo, sgpr_fit_batch_nd_loo_grad,
fit.fit_batch_pairs_loo[_grad], func.loo_chol_pairs[_batch], func.loo_chol_pairs_grad[_batch]) that needs no device: every argument
error of the two C entries returns SGPR_E_ARG before a device is asked for, the symbols are exported under ABI 5, the arena layout
of their modes (sgpr_probe_batch_layout_nd_loo) equals the formulas restated here (those of tests/test_batch_layout_cpu.py), and the
Python wrappers hand the library the documented layout, apply the documented signs and NaN / LinAlgError conventions and switch to their slow paths above orders 256
and 2048."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import c_header

LEAF, BMAX, PER_WG = 128, 256, 98816          # leaf order, largest one-launch order, scratch doubles per workgroup of a plain fit
GT = 256                                       # mid loo: points per workgroup
FIT, GRAD, LOO, LOOGRAD = 0, 1, 2, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sgpr_fit_batch_nd_loo", "sgpr_fit_batch_nd_loo_grad")


def _lib():
    from sympgpr_amd import _lib as L
    return L, L.load_library()


def _call(lib, L, entry, family=0, d=2, nbatch=2, n_pts=5, nhyp=None, flags=0, which=0, null=()):
    """one of the two entries with well-formed buffers for (d, nbatch, n_pts); `null`: the arguments passed as NULL"""
    D = 2 * d if 1 <= d <= 3 else 2
    nb, npt = max(nbatch, 1), max(n_pts, 1)
    nh = nhyp if nhyp is not None else (3 * d + 1 if family == 3 else 2 * d + 1)
    bufs = dict(X=np.ones(nb * D * npt), z=np.ones(nb * D * npt), hyp=np.ones(nb * max(nh, 1)), sig2n=np.full(nb, 1e-2),
                alpha=np.zeros(nb * D * npt), nll=np.zeros(nb), loo=np.zeros(nb * 2), value=np.zeros(nb),
                grad=np.zeros(nb * (max(nh, 1) + 1)))
    info = np.zeros(nb, dtype=np.int32)
    p = {k: (None if k in null else L.dptr(v)) for k, v in bufs.items()}
    pinfo = None if "info" in null else info.ctypes.data_as(C.POINTER(C.c_int))
    lead = (family, d, nbatch, n_pts, p["X"], p["z"], p["hyp"], nh, p["sig2n"], flags)
    if entry == "sgpr_fit_batch_nd_loo":
        return lib.sgpr_fit_batch_nd_loo(*lead, p["alpha"], p["nll"], p["loo"], pinfo)
    return lib.sgpr_fit_batch_nd_loo_grad(*lead, which, p["alpha"], p["nll"], p["value"], p["grad"], pinfo)


COMMON = [
    dict(d=0), dict(d=4), dict(d=-1),
    dict(family=-1), dict(family=5),
    dict(nhyp=4), dict(nhyp=7), dict(family=3, nhyp=5), dict(d=3, nhyp=5), dict(d=1, nhyp=5),
    dict(flags=1), dict(flags=2),
    dict(nbatch=-1), dict(n_pts=0), dict(n_pts=-3),
    dict(d=2, n_pts=513), dict(d=3, n_pts=342), dict(d=1, n_pts=1025),                   # orders 2052, 2052, 2050
    dict(null=("X",)), dict(null=("z",)), dict(null=("hyp",)), dict(null=("sig2n",)), dict(null=("nll",)), dict(null=("info",)),
]


@pytest.mark.parametrize("kw", COMMON + [dict(null=("loo",))])
def test_every_argument_error_of_the_values_entry_returns_before_a_device_is_needed(kw):
    L, lib = _lib()
    assert _call(lib, L, "sgpr_fit_batch_nd_loo", **kw) == L.E_ARG
    assert b"fit_batch_nd_loo:" in lib.sgpr_last_error()


@pytest.mark.parametrize("kw", COMMON + [
    dict(which=2), dict(which=-1),
    dict(d=2, n_pts=65), dict(d=3, n_pts=43), dict(d=1, n_pts=129),                      # orders 260, 258, 258: above 256
    dict(null=("value",)), dict(null=("grad",)),
])
def test_every_argument_error_of_the_gradient_entry_returns_before_a_device_is_needed(kw):
    L, lib = _lib()
    assert _call(lib, L, "sgpr_fit_batch_nd_loo_grad", **kw) == L.E_ARG
    assert b"fit_batch_nd_loo_grad:" in lib.sgpr_last_error()


def test_the_order_checks_name_their_limits_and_an_empty_batch_returns_zero():
    L, lib = _lib()
    assert lib.sgpr_fit_batch_max_order() == 2048
    assert _call(lib, L, "sgpr_fit_batch_nd_loo", d=2, n_pts=513) == L.E_ARG
    assert b"2052" in lib.sgpr_last_error() and b"2048" in lib.sgpr_last_error()
    assert _call(lib, L, "sgpr_fit_batch_nd_loo_grad", d=2, n_pts=65) == L.E_ARG
    assert b"260" in lib.sgpr_last_error() and b"256" in lib.sgpr_last_error()
    for entry in ENTRIES:
        assert _call(lib, L, entry, nbatch=0) == 0                      # nothing to do: no device call either
        assert _call(lib, L, entry, nbatch=0, null=("alpha",)) == 0


def test_abi_and_exports():
    L, lib = _lib()
    assert lib.sgpr_abi_version() == 5
    for entry in ENTRIES:
        c_header.assert_bound_as_declared(entry)
        assert c_header.in_exports_map(entry), entry


# ---- the arena layout for d > 0 in the loo modes, against the formulas of tests/test_batch_layout_cpu.py restated here

def up256(b):
    return (b + 255) // 256 * 256


def probe(path, mode, d, nbatch, npts, nhyp):
    from sympgpr_amd import _lib as L
    out = (C.c_ulonglong * 24)()
    L.check(L.load_probe_library().sgpr_probe_batch_layout_nd_loo(path, mode, d, nbatch, npts, nhyp, out))
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


def check_layout(path, mode, d, nbatch, npts, nhyp, cap=0):
    got = probe(path, mode, d, nbatch, npts, nhyp)
    n = 2 * d * npts
    nacc = {LOO: 2, LOOGRAD: nhyp + 3}[mode]
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
        per_wg = PER_WG + BMAX * BMAX + (BMAX * BMAX if mode == LOOGRAD else 0)
        assert got["scr_bytes"] == min(nbatch, 1024) * per_wg * 8
        assert got["flag_bytes"] == 0
        return
    flag = got["flag_bytes"]
    assert flag >= 4 * c
    lnwg = -(-npts // GT)
    part = c * lnwg * 2 * 8
    # L images, U images directly behind | leaf inverses | flags of panel 1 | of panel 2 | r | pub | state | partials
    needs_scr = [2 * c * img, c * W * LEAF * LEAF * 8, flag, flag, c * npad * 8, 2 * c * npad * 8, c * 8 * 4, part]
    regions([got[k] for k in ("o_A", "o_inv", "o_fl", "o_fl2", "o_r", "o_pub", "o_st", "o_part")], needs_scr, got["scr_bytes"])
    assert got["o_A"] == 0 and (c * img) % 256 == 0          # the U images start at image c of the L images
    assert got["scr_bytes"] == 2 * up256(c * img) + sum(up256(b) for b in needs_scr[1:])


@pytest.mark.parametrize("mode", [LOO, LOOGRAD])
@pytest.mark.parametrize("d,npts", [(2, 64), (3, 42), (1, 128), (2, 1)])
@pytest.mark.parametrize("nbatch", [1, 1024, 1500])
def test_small_path_layout(d, npts, nbatch, mode):
    for nhyp in (2 * d + 1, 3 * d + 1):
        check_layout(0, mode, d, nbatch, npts, nhyp)


@pytest.fixture(params=[0, 2])
def chunk_cap(request):
    """the batch_gradmid_chunk tunable at 0 (none, the built-in value) and 2; back to 0 afterwards"""
    from sympgpr_amd import _lib as L
    tune = L.load_probe_library().sgpr_probe_tune
    L.check(tune(b"batch_gradmid_chunk", float(request.param)))
    yield request.param
    L.check(tune(b"batch_gradmid_chunk", 0.0))


@pytest.mark.parametrize("d,npts", [(3, 43), (2, 300), (3, 171), (2, 512), (1, 129)])
@pytest.mark.parametrize("nbatch", [1, 3, 70])
def test_mid_path_layout(d, npts, nbatch, chunk_cap):
    for nhyp in (2 * d + 1, 3 * d + 1):
        check_layout(1, LOO, d, nbatch, npts, nhyp, chunk_cap)


def test_probe_refuses_what_the_entries_refuse():
    from sympgpr_amd import _lib as L
    out = (C.c_ulonglong * 24)()
    layout = L.load_probe_library().sgpr_probe_batch_layout_nd_loo
    assert layout(1, LOOGRAD, 2, 4, 160, 5, out) != 0         # no loo gradient above order 256
    assert layout(0, LOOGRAD, 2, 4, 65, 5, out) != 0          # order 260 on the one-launch path
    assert layout(1, LOO, 2, 4, 64, 5, out) != 0              # order 256 on the mid path
    assert layout(1, LOO, 2, 4, 513, 5, out) != 0             # order 2052
    assert layout(0, LOO, 0, 4, 20, 3, out) != 0 and layout(0, LOO, 4, 4, 20, 9, out) != 0      # d outside 1 .. 3
    assert layout(0, FIT, 2, 4, 20, 5, out) != 0 and layout(0, GRAD, 2, 4, 20, 5, out) != 0     # sgpr_probe_batch_layout's modes
    assert layout(0, LOOGRAD, 2, 4, 64, 5, out) == 0 and layout(1, LOO, 3, 4, 43, 7, out) == 0


# ---- the Python wrappers, with a stand-in for the loaded library

def test_python_shape_and_objective_errors():
    from sympgpr_amd import fit, func
    X, hyp = np.ones((3, 5, 4)), np.ones((3, 5))
    bad = []
    for fn in (fit.fit_batch_pairs_loo, fit.fit_batch_pairs_loo_grad):
        bad += [
            lambda fn=fn: fn("A", X, np.ones((3, 20)), np.ones(5), 1e-2),                          # hyp must have rows
            lambda fn=fn: fn("A", np.ones((2, 5, 4)), np.ones((3, 20)), hyp, 1e-2),                 # B of X against hyp
            lambda fn=fn: fn("A", np.ones((3, 5, 3)), np.ones((3, 15)), hyp, 1e-2),                 # odd number of coordinates
            lambda fn=fn: fn("A", np.ones(20), np.ones((3, 20)), hyp, 1e-2),                        # X with one axis
            lambda fn=fn: fn("A", X, np.ones((3, 19)), hyp, 1e-2),                                  # z too short
            lambda fn=fn: fn("A", X, np.ones((2, 20)), hyp, 1e-2),                                  # B of z
            lambda fn=fn: fn("A", X, np.ones(21), hyp, 1e-2),                                       # broadcast z of the wrong length
            lambda fn=fn: fn("A", X, np.ones((3, 20)), hyp, np.ones(2)),                            # sig2n of the wrong length
        ]
    bad += [
        lambda: fit.fit_batch_pairs_loo_grad("A", X, np.ones((3, 20)), hyp, 1e-2, objective="nll"),
        lambda: func.loo_chol_pairs_batch(np.ones((2, 6)), np.ones((5, 3)), np.ones(15)),
        lambda: func.loo_chol_pairs_batch(np.ones((2, 6)), np.ones((5, 4)), np.ones(19)),
        lambda: func.loo_chol_pairs_batch(np.ones((2, 6)), np.ones(20), np.ones(20)),
        lambda: func.loo_chol_pairs_batch(np.ones((2, 1)), np.ones((5, 4)), np.ones(20)),
        lambda: func.loo_chol_pairs(np.ones((2, 6)), np.ones((5, 4)), np.ones(20)),
        lambda: func.loo_chol_pairs(np.ones(6), np.ones((5, 3)), np.ones(15)),
        lambda: func.loo_chol_pairs_grad_batch(np.ones((2, 6)), np.ones((5, 3)), np.ones(15)),
        lambda: func.loo_chol_pairs_grad_batch(np.ones((2, 6)), np.ones((5, 4)), np.ones(19)),
        lambda: func.loo_chol_pairs_grad_batch(np.ones((2, 6)), np.ones((5, 4)), np.ones(20), objective="nll"),
        lambda: func.loo_chol_pairs_grad(np.ones((2, 6)), np.ones((5, 4)), np.ones(20)),
        lambda: func.loo_chol_pairs_grad(np.ones(6), np.ones((5, 4)), np.ones(20), objective="nll"),
    ]
    for call in bad:
        with pytest.raises(ValueError):
            call()


class _Recorder:
    """stands in for the loaded library: keeps the buffers the two entries are handed and answers with a pattern"""

    def __init__(self):
        self.calls = []
        self.fail = 1                     # the row that comes back with info > 0 (if the batch has it)

    def sgpr_fit_batch_max_order(self):
        return 2048

    def _record(self, entry, family, d, nbatch, n_pts, X, z, hyp, nhyp, sig2n, flags, alpha, which=None):
        n = 2 * d * n_pts
        self.calls.append(dict(entry=entry, family=family, d=d, nbatch=nbatch, n_pts=n_pts, nhyp=nhyp, flags=flags, which=which,
                               X=np.ctypeslib.as_array(X, (nbatch * n,)).copy(), z=np.ctypeslib.as_array(z, (nbatch * n,)).copy(),
                               hyp=np.ctypeslib.as_array(hyp, (nbatch * nhyp,)).copy(),
                               sig2n=np.ctypeslib.as_array(sig2n, (nbatch,)).copy(), alpha=alpha))

    def sgpr_fit_batch_nd_loo(self, family, d, nbatch, n_pts, X, z, hyp, nhyp, sig2n, flags, alpha, nll, loo, info):
        self._record("loo", family, d, nbatch, n_pts, X, z, hyp, nhyp, sig2n, flags, alpha)
        np.ctypeslib.as_array(nll, (nbatch,))[:] = np.arange(nbatch)
        # row b: {10 b + 1, 10 b + 2}
        np.ctypeslib.as_array(loo, (nbatch, 2))[:] = 10.0 * np.arange(nbatch)[:, None] + np.array([1.0, 2.0])[None, :]
        if self.fail < nbatch:
            np.ctypeslib.as_array(info, (nbatch,))[self.fail] = 3
        return 0

    def sgpr_fit_batch_nd_loo_grad(self, family, d, nbatch, n_pts, X, z, hyp, nhyp, sig2n, flags, which, alpha, nll, value, grad,
                                   info):
        self._record("loo_grad", family, d, nbatch, n_pts, X, z, hyp, nhyp, sig2n, flags, alpha, which)
        np.ctypeslib.as_array(nll, (nbatch,))[:] = np.arange(nbatch)
        np.ctypeslib.as_array(value, (nbatch,))[:] = 10.0 * np.arange(nbatch) + 1.0 + which
        # row b of the gradient: 100 b + k + 1, every entry positive
        np.ctypeslib.as_array(grad, (nbatch, nhyp + 1))[:] = 100.0 * np.arange(nbatch)[:, None] + np.arange(nhyp + 1)[None, :] + 1.0
        if self.fail < nbatch:
            np.ctypeslib.as_array(info, (nbatch,))[self.fail] = 3
        return 0


def _data(n_pts, d, B, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_pts, 2 * d)), rng.standard_normal(2 * d * n_pts), rng.uniform(0.5, 1.5, (B, 2 * d + 1)), rng)


def test_fit_wrappers_hand_over_the_documented_layout(monkeypatch):
    from sympgpr_amd import _lib as L, fit
    rec = _Recorder()
    monkeypatch.setattr(L, "load_library", lambda: rec)
    n_pts, d, B = 5, 2, 3
    X, z, hyp, rng = _data(n_pts, d, B)

    def check_inputs(c, entry, which):
        assert (c["entry"], c["family"], c["d"], c["nbatch"], c["n_pts"], c["nhyp"], c["flags"], c["which"]) == \
            (entry, L.FAMILIES["C"], d, B, n_pts, 5, 0, which)
        for b in range(B):
            for m in range(2 * d):
                for i in range(n_pts):
                    assert c["X"][(b * 2 * d + m) * n_pts + i] == X[i, m]
            assert np.array_equal(c["z"][b * 20:(b + 1) * 20], z)
        assert np.array_equal(c["hyp"], hyp.ravel()) and np.array_equal(c["sig2n"], np.full(B, 1e-2))

    alpha, nll, loo, info = fit.fit_batch_pairs_loo("C", X, z, hyp, 1e-2)
    check_inputs(rec.calls[-1], "loo", None)
    assert rec.calls[-1]["alpha"] is None and alpha is None     # want_alpha defaults to False
    assert loo.shape == (B, 2) and list(info) == [0, 3, 0]
    assert np.isnan(nll[1]) and np.all(np.isnan(loo[1])) and nll[0] == 0.0 and nll[2] == 2.0
    assert np.array_equal(loo[0], [1.0, 2.0]) and np.array_equal(loo[2], [21.0, 22.0])
    for objective, which in (("loo", L.LOO_LPD), ("press", L.LOO_PRESS)):
        alpha, nll, value, grad, info = fit.fit_batch_pairs_loo_grad("C", X, z, hyp, 1e-2, objective=objective)
        check_inputs(rec.calls[-1], "loo_grad", which)
        assert alpha is None and value.shape == (B,) and grad.shape == (B, 6) and list(info) == [0, 3, 0]
        assert np.isnan(nll[1]) and np.isnan(value[1]) and np.all(np.isnan(grad[1]))
        assert value[0] == 1.0 + which and value[2] == 21.0 + which
        assert np.array_equal(grad[0], np.arange(6) + 1.0) and np.array_equal(grad[2], 200.0 + np.arange(6) + 1.0)
    # one problem per row: the same layout from (B, n_pts, 2d); alpha on request
    X3 = rng.standard_normal((B, n_pts, 2 * d))
    for fn in (fit.fit_batch_pairs_loo, fit.fit_batch_pairs_loo_grad):
        out = fn("C", X3, np.tile(z, (B, 1)), hyp, np.array([1e-2, 2e-2, 3e-2]), want_alpha=True)
        c = rec.calls[-1]
        assert c["alpha"] is not None and out[0].shape == (B, 20)
        assert np.array_equal(c["X"].reshape(B, 2 * d, n_pts), np.swapaxes(X3, 1, 2)) and list(c["sig2n"]) == [1e-2, 2e-2, 3e-2]


class _Handle:
    """stands in for SympFit.pairs: counts the handles created and answers run / loo / loo_grad with a pattern of the row's sig"""
    created = 0
    log = []

    def __init__(self, family, X, z, hyp, sig2n):
        type(self).created += 1
        self.set_hyp(hyp, sig2n)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def set_hyp(self, hyp, sig2n):
        assert sig2n >= 0.0                               # the wrappers hand over |sig2_n|
        self.hyp, self.sig2n = np.array(hyp), float(sig2n)

    def run(self):
        if self.hyp[-1] < 0.0:
            raise np.linalg.LinAlgError("not positive definite")
        type(self).log.append(self.hyp.copy())
        return self

    def loo(self, resid=True, cov=False, lpd=True):
        assert not resid and not lpd
        return {"loo": 7.0 * self.hyp[-1], "press": 9.0 * self.hyp[-1]}

    def loo_grad(self, objective="loo"):
        k = 7.0 if objective == "loo" else 9.0
        return k * self.hyp[-1], np.arange(len(self.hyp) + 1) + 1.0


def test_fit_wrapper_slow_path_above_order_256(monkeypatch):
    """order 260: the values from ONE sgpr_fit_batch_nd_loo call, the gradient of each row with info == 0 from a handle"""
    from sympgpr_amd import _lib as L, fit
    rec = _Recorder()
    monkeypatch.setattr(L, "load_library", lambda: rec)
    made = []

    def pairs(family, X, z, hyp, sig2n):
        made.append((np.array(X), np.array(z), np.array(hyp), float(sig2n)))
        return _Handle(family, X, z, hyp, sig2n)

    monkeypatch.setattr(fit.SympFit, "pairs", staticmethod(pairs))
    n_pts, d, B = 65, 2, 3
    X, z, hyp, _ = _data(n_pts, d, B)
    for objective, col in (("loo", 0), ("press", 1)):
        del made[:]
        ncalls = len(rec.calls)
        alpha, nll, value, grad, info = fit.fit_batch_pairs_loo_grad("C", X, z, hyp, [1e-2, 2e-2, 3e-2], objective=objective)
        assert len(rec.calls) == ncalls + 1 and rec.calls[-1]["entry"] == "loo" and rec.calls[-1]["nbatch"] == B
        assert list(info) == [0, 3, 0] and np.isnan(value[1]) and np.all(np.isnan(grad[1])) and np.isnan(nll[1])
        assert value[0] == 1.0 + col and value[2] == 21.0 + col                   # the column of the batched call
        assert [m[3] for m in made] == [1e-2, 3e-2]                               # rows 0 and 2 only
        for m, b in zip(made, (0, 2)):
            assert np.array_equal(m[0], X) and np.array_equal(m[1], z) and np.array_equal(m[2], hyp[b])
            assert np.array_equal(grad[b], np.arange(6) + 1.0)


def test_func_wrappers_conventions(monkeypatch):
    from sympgpr_amd import _lib as L, func
    rec = _Recorder()
    monkeypatch.setattr(L, "load_library", lambda: rec)
    n_pts, d, B = 5, 2, 3
    X, z, hyp, _ = _data(n_pts, d, B)
    func.set_family("C")
    try:
        # the last column is the noise, handed over as |.|; its sign multiplies the last gradient column; a failed row is NaN
        rows = np.column_stack((hyp, [-1e-3, -2e-3, 3e-3]))
        v = func.loo_chol_pairs_batch(rows, X, z)
        c = rec.calls[-1]
        assert c["entry"] == "loo" and np.array_equal(c["hyp"], hyp.ravel()) and list(c["sig2n"]) == [1e-3, 2e-3, 3e-3]
        assert c["alpha"] is None and v.shape == (B,) and v[0] == 1.0 and np.isnan(v[1]) and v[2] == 21.0
        assert func.loo_chol_pairs(rows[0], X, z) == 1.0
        for objective, which in (("loo", 0), ("press", 1)):
            vals, grads = func.loo_chol_pairs_grad_batch(rows, X, z, objective=objective)
            c = rec.calls[-1]
            assert c["entry"] == "loo_grad" and c["which"] == which and list(c["sig2n"]) == [1e-3, 2e-3, 3e-3]
            assert vals[0] == 1.0 + which and np.isnan(vals[1]) and vals[2] == 21.0 + which
            assert np.all(np.isnan(grads[1]))
            assert np.array_equal(grads[0], [1.0, 2.0, 3.0, 4.0, 5.0, -6.0])        # sig2_n < 0: the last entry changes sign
            assert np.array_equal(grads[2], 200.0 + np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]))
            v1, g1 = func.loo_chol_pairs_grad(rows[0], X, z, objective=objective)
            assert v1 == 1.0 + which and np.array_equal(g1, [1.0, 2.0, 3.0, 4.0, 5.0, -6.0])
        rec.fail = 0
        with pytest.raises(np.linalg.LinAlgError):
            func.loo_chol_pairs(rows[0], X, z)
        with pytest.raises(np.linalg.LinAlgError):
            func.loo_chol_pairs_grad(rows[0], X, z)
    finally:
        func.set_family("A")


def test_func_wrappers_switch_paths_above_256_and_2048(monkeypatch):
    from sympgpr_amd import _lib as L, fit, func
    rec = _Recorder()
    rec.fail = 99
    monkeypatch.setattr(L, "load_library", lambda: rec)
    monkeypatch.setattr(fit.SympFit, "pairs", staticmethod(_Handle))
    monkeypatch.setattr(func.SympFit, "pairs", staticmethod(_Handle))
    func.set_family("C")
    try:
        # order 260: values batched, gradients through one handle per row (the fit wrapper's slow path)
        X, z, hyp, _ = _data(65, 2, 3)
        rows = np.column_stack((hyp, [-1e-3, 2e-3, 3e-3]))
        _Handle.created = 0
        n0 = len(rec.calls)
        vals, grads = func.loo_chol_pairs_grad_batch(rows, X, z)
        assert [c["entry"] for c in rec.calls[n0:]] == ["loo"] and _Handle.created == 3
        assert np.array_equal(vals, [1.0, 11.0, 21.0])
        assert np.array_equal(grads[0], [1.0, 2.0, 3.0, 4.0, 5.0, -6.0]) and np.array_equal(grads[1], np.arange(6) + 1.0)
        n0 = len(rec.calls)
        v = func.loo_chol_pairs_batch(rows, X, z)
        assert [c["entry"] for c in rec.calls[n0:]] == ["loo"] and np.array_equal(v, [1.0, 11.0, 21.0])
        # order 2052: no batched call at all, ONE resident handle for the whole population; sig < 0 stands for an indefinite row
        X, z, hyp, _ = _data(513, 2, 3)
        rows = np.column_stack((hyp, [-1e-3, 2e-3, 3e-3]))
        rows[1, -2] = -1.0
        n0 = len(rec.calls)
        _Handle.created = 0
        v = func.loo_chol_pairs_batch(rows, X, z)
        assert len(rec.calls) == n0 and _Handle.created == 1
        assert v[0] == 7.0 * rows[0, -2] and np.isnan(v[1]) and v[2] == 7.0 * rows[2, -2]
        _Handle.created = 0
        vals, grads = func.loo_chol_pairs_grad_batch(rows, X, z, objective="press")
        assert len(rec.calls) == n0 and _Handle.created == 1
        assert vals[0] == 9.0 * rows[0, -2] and np.isnan(vals[1]) and np.all(np.isnan(grads[1]))
        assert np.array_equal(grads[0], [1.0, 2.0, 3.0, 4.0, 5.0, -6.0]) and np.array_equal(grads[2], np.arange(6) + 1.0)
        assert func.loo_chol_pairs(rows[2], X, z) == 7.0 * rows[2, -2]
        v1, g1 = func.loo_chol_pairs_grad(rows[0], X, z)
        assert v1 == 7.0 * rows[0, -2] and np.array_equal(g1, [1.0, 2.0, 3.0, 4.0, 5.0, -6.0])
        with pytest.raises(np.linalg.LinAlgError):
            func.loo_chol_pairs(rows[1], X, z)
        with pytest.raises(np.linalg.LinAlgError):
            func.loo_chol_pairs_grad(rows[1], X, z)
        assert len(rec.calls) == n0
    finally:
        func.set_family("A")
