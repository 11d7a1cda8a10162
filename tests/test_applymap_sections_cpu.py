"""CPU checks of the sectioned map (sgpr_applymap_sections_host, maps.run_map_sections, examples/tokamak_split): the entry is
declared, exported and bound alike, every argument error is answered with SGPR_E_ARG before any device call, the Python
wrapper validates shapes, and the chunk-and-callback bookkeeping of applymap_tok is checked against the reference's
step-by-step double loop with a NumPy stepper.  The numbers are checked on the GPU (tests/test_gpu_applymap_sections.py)."""
import os

import numpy as np
import pytest

from tests import c_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sgpr_applymap_sections_host"


def test_header_ctypes_table_and_library_agree():
    from sympgpr_amd import _lib as L
    c_header.assert_bound_as_declared(NAME, 23)
    assert L.load_library().sgpr_abi_version() == 5


def _args(**over):
    """a valid call (family A, two sections, implicit), as a dict of named arguments in the order of the declaration"""
    from sympgpr_amd import _lib as L
    nsec, n0, n0p, ntest, nm = 2, 4, 5, 3, 3
    keep = dict(hyp=np.array([1.2, 1.5, 1.0, 1.1, 1.4, 0.9]), x=np.zeros(n0 * nsec), y=np.zeros(n0 * nsec),
                alpha=np.zeros(2 * n0 * nsec), hypp=np.array([1.2, 1.5, 1.0, 1.1, 1.4, 0.9]), xp=np.zeros(n0p * nsec),
                yp=np.zeros(n0p * nsec), alphap=np.zeros(n0p * nsec), Q0=np.ones(ntest), P0=np.ones(ntest),
                qmap=np.zeros((nm, ntest)), pmap=np.zeros((nm, ntest)), pdiff=np.zeros((nm, ntest)))
    a = dict(family=0, mode=L.MAP_WRAP_Q | L.MAP_LOSS_NEGP, nsec=nsec, first=1, nm=nm, ntest=ntest, hyp=L.dptr(keep["hyp"]),
             nhyp=3, n0=n0, x=L.dptr(keep["x"]), y=L.dptr(keep["y"]), alpha=L.dptr(keep["alpha"]), hypp=L.dptr(keep["hypp"]),
             nhypp=3, n0p=n0p, xp=L.dptr(keep["xp"]), yp=L.dptr(keep["yp"]), alphap=L.dptr(keep["alphap"]),
             Q0=L.dptr(keep["Q0"]), P0=L.dptr(keep["P0"]), qmap=L.dptr(keep["qmap"]), pmap=L.dptr(keep["pmap"]),
             pdiff=L.dptr(keep["pdiff"]))
    a.update(over)
    return a, keep


BAD = [dict(nsec=0), dict(nsec=-1), dict(first=-1), dict(first=2), dict(nm=0), dict(ntest=-1), dict(n0=-1), dict(n0p=-1),
       dict(mode=16), dict(mode=32 | 1), dict(mode=4 | 8), dict(hyp=None), dict(hypp=None), dict(x=None), dict(y=None),
       dict(alpha=None), dict(xp=None), dict(yp=None), dict(alphap=None), dict(Q0=None), dict(P0=None), dict(qmap=None),
       dict(pmap=None), dict(nhyp=4), dict(nhyp=2), dict(nhypp=4), dict(family=3), dict(family=9), dict(family=-1),
       dict(mode=4, x=None)]


@pytest.mark.parametrize("over", BAD, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_argument_errors_come_before_any_device_call(over):
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    a, keep = _args(**over)
    assert getattr(lib, NAME)(*a.values()) == L.E_ARG
    assert lib.sgpr_last_error() != b""


def test_valid_calls_reach_the_device_check():
    """well-formed calls pass every check: without a GPU they end at SGPR_E_NODEVICE, not SGPR_E_ARG.  With EXPLICIT the guess
    GPs are ignored, null pointers and a wrong nhypp included."""
    import sympgpr_amd
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    want = 0 if sympgpr_amd.device_count() > 0 else L.E_NODEVICE
    for over in ({}, dict(pdiff=None), dict(first=0, nm=1), dict(ntest=0), dict(mode=0),
                 dict(mode=L.MAP_EXPLICIT | L.MAP_WRAP_P, hypp=None, nhypp=0, xp=None, yp=None, alphap=None, n0p=-3),
                 dict(family=3, nhyp=4, nhypp=4, hyp=L.dptr(np.ones(8)), hypp=L.dptr(np.ones(8)))):
        a, keep = _args(**over)
        assert getattr(lib, NAME)(*a.values()) == want, over


def test_run_map_sections_validates_shapes():
    from sympgpr_amd import maps
    nsec, n0, n0p = 3, 4, 5
    good = dict(mode=maps.WRAP_Q, nm=3, Ntest=2, hyp=np.ones((nsec, 3)), xt=np.zeros((n0, nsec)), yt=np.zeros((n0, nsec)),
                alpha=np.zeros((2 * n0, nsec)), Q0=np.ones(2), P0=np.ones(2), hypp=np.ones((nsec, 3)), xp=np.zeros((n0p, nsec)),
                yp=np.zeros((n0p, nsec)), alphap=np.zeros((n0p, nsec)), first=2, family="A")
    bad = [dict(alpha=np.zeros((2 * n0 - 1, nsec))), dict(alpha=np.zeros((n0, nsec))),      # alpha of the wrong length
           dict(alphap=np.zeros((n0p + 1, nsec))), dict(yt=np.zeros((n0 + 1, nsec))),
           dict(xt=np.zeros((n0, nsec - 1))), dict(alpha=np.zeros((2 * n0, nsec + 1))),     # mismatched section counts
           dict(hypp=np.ones((nsec - 1, 3))), dict(xp=np.zeros((n0p, 2))), dict(alpha=np.zeros(2 * n0)),
           dict(hyp=np.ones(3)),
           dict(first=3), dict(first=-1),                                                   # first out of range
           dict(hypp=None), dict(xp=None), dict(yp=None), dict(alphap=None),                # no guess GPs, implicit mode
           dict(nm=0), dict(Q0=np.ones(3))]
    for over in bad:
        with pytest.raises(ValueError):
            maps.run_map_sections(**dict(good, **over))
    assert "fit_batch" in maps.run_map_sections.__doc__ and "gather_sections" in maps.run_map_sections.__doc__


# ---- the chunk-and-callback bookkeeping of examples/tokamak_split.applymap_tok, without a GPU

def _step(m, q, p):
    """a cheap area-preserving map whose step depends on the section index m (a kicked rotor with the kick strength of the
    section); P < 0 loses the orbit like SGPR_MAP_LOSS_NEGP"""
    P = p - (0.05 + 0.02 * m) * np.sin(q + 0.3 * m)
    if not P >= 0.0:
        return np.nan, np.nan
    return np.mod(q + (0.5 + 0.05 * m) * P, 2 * np.pi), P


def _make_stepper(nphmap, calls):
    def run(first, steps, Q0, P0):
        calls.append((first, steps, len(Q0)))
        q, p = np.full((steps + 1, len(Q0)), np.nan), np.full((steps + 1, len(Q0)), np.nan)
        q[0], p[0] = Q0, P0
        for s in range(steps):
            for k in range(len(Q0)):
                if not np.isnan(p[s, k]):
                    q[s + 1, k], p[s + 1, k] = _step((first + s) % nphmap, q[s, k], p[s, k])
        return q, p
    return run


def _compute_r(zk, r0):
    """stand-in for fieldlines.compute_r: depends on all three entries of zk (the momentum, the NEW angle, the section's phi)"""
    assert r0 == 0.3
    return 0.005 + 0.5 * np.sin(37.0 * zk[0] * 1e2 + 3.0 * zk[1] + zk[2]) ** 2


def _reference_loop(nphmap, nm, Ntest, Q0map, P0map, compute_r):
    """Split_SympGPR/func.py:184-219 restated step by step, with _step in place of calcP / calcQ"""
    pmap, qmap = np.zeros([nm, Ntest]), np.zeros([nm, Ntest])
    pmap[0, :], qmap[0, :] = P0map, Q0map
    i = 0
    while i < nm - nphmap:
        for m in range(0, nphmap):
            for k in range(0, Ntest):
                if np.isnan(pmap[i, k]):
                    pmap[i + 1, k] = qmap[i + 1, k] = np.nan
                    continue
                qmap[i + 1, k], pmap[i + 1, k] = _step(m, qmap[i, k], pmap[i, k])
                if np.isnan(pmap[i + 1, k]):
                    continue
                ph = (2 * np.pi) / nphmap * np.mod(i + 1, nphmap)
                zk = np.array([pmap[i + 1, k] * 1e-2, qmap[i + 1, k], ph])
                if compute_r is not None and compute_r(zk, 0.3) > 0.5:
                    pmap[i + 1, k] = qmap[i + 1, k] = np.nan
            i = i + 1
    return qmap, pmap


@pytest.fixture(scope="module")
def start():
    rng = np.random.default_rng(2024)
    Ntest = 12
    return Ntest, rng.uniform(0.0, 2 * np.pi, Ntest), rng.uniform(0.02, 1.0, Ntest)


@pytest.mark.parametrize("chunk", [1, 3, 4, 7])
def test_chunks_with_callback_repeat_the_reference_loop(start, chunk):
    from sympgpr_amd.examples.tokamak_split import map_in_chunks
    nphmap, nm = 4, 23
    Ntest, Q0, P0 = start
    qr, pr = _reference_loop(nphmap, nm, Ntest, Q0, P0, _compute_r)
    steps = 20                                                   # ceil((23 - 4) / 4) * 4
    calls = []
    q, p = map_in_chunks(_make_stepper(nphmap, calls), nphmap, nm, Ntest, Q0, P0, _compute_r, chunk)
    assert np.array_equal(q, qr, equal_nan=True) and np.array_equal(p, pr, equal_nan=True)      # bit for bit
    assert np.array_equal(np.isnan(p), np.isnan(pr)) and np.array_equal(np.isnan(q), np.isnan(p))
    lost = np.isnan(pr[steps])
    assert lost.any() and not lost.all()                         # the rules bite, and not on everything
    assert np.isnan(pr[1:steps + 1]).sum() > np.isnan(_reference_loop(nphmap, nm, Ntest, Q0, P0, None)[1][1:steps + 1]).sum()
    assert np.all(p[steps + 1:] == 0) and np.all(q[steps + 1:] == 0) and steps + 1 < nm
    # every launch starts at the section its first step belongs to, and covers the map exactly once
    assert [c[0] for c in calls] == [(j * chunk) % nphmap for j in range(len(calls))]
    assert sum(c[1] for c in calls) == steps and all(c[1] <= chunk for c in calls)


def test_no_callback_is_one_call(start):
    from sympgpr_amd.examples.tokamak_split import map_in_chunks
    nphmap, nm = 4, 23
    Ntest, Q0, P0 = start
    qr, pr = _reference_loop(nphmap, nm, Ntest, Q0, P0, None)
    calls = []
    q, p = map_in_chunks(_make_stepper(nphmap, calls), nphmap, nm, Ntest, Q0, P0)
    assert calls == [(0, 20, Ntest)]
    assert np.array_equal(q, qr, equal_nan=True) and np.array_equal(p, pr, equal_nan=True)
    assert np.all(p[21:] == 0) and np.all(q[21:] == 0)


@pytest.mark.parametrize("nm", [1, 3, 4])
def test_nm_up_to_nphmap_runs_no_step(start, nm):
    from sympgpr_amd.examples.tokamak_split import map_in_chunks
    Ntest, Q0, P0 = start
    calls = []
    for cr, chunk in ((None, None), (_compute_r, 3)):
        q, p = map_in_chunks(_make_stepper(4, calls), 4, nm, Ntest, Q0, P0, cr, chunk)
        assert calls == []
        assert np.array_equal(q[0], Q0) and np.array_equal(p[0], P0) and np.all(q[1:] == 0) and np.all(p[1:] == 0)
        qr, pr = _reference_loop(4, nm, Ntest, Q0, P0, cr)
        assert np.array_equal(q, qr) and np.array_equal(p, pr)


def test_applymap_tok_routes(monkeypatch, start):
    """applymap_tok itself, with maps.run_map_sections and the host loop replaced: no callback -> ONE call of the sectioned
    map with WRAP_Q | LOSS_NEGP and alpha_m = Kyinv[m] @ ztrain[:, m]; callback + steps_per_launch -> chunks continued at the
    right section; a bare callback -> the host loop of before."""
    from sympgpr_amd import maps
    from sympgpr_amd.examples import tokamak_split as ts
    nph, N, Np, nm = 4, 5, 6, 23
    Ntest, Q0, P0 = start
    rng = np.random.default_rng(3)
    xtrain, ztrain, Kyinv, hyp = rng.normal(size=(2 * N, nph)), rng.normal(size=(2 * N, nph)), rng.normal(size=(nph, 2 * N, 2 * N)), rng.uniform(1, 2, (nph, 3))
    xtrainp, ztrainp, Kyinvp, hypp = rng.normal(size=(2 * Np, nph)), rng.normal(size=(Np, nph)), rng.normal(size=(nph, Np, Np)), rng.uniform(1, 2, (nph, 3))
    seen, calls = [], []
    stepper = _make_stepper(nph, calls)

    def fake(mode, nm_, Ntest_, hyp_, xt, yt, alpha, Q0_, P0_, hypp_=None, xp=None, yp=None, alphap=None, first=0, want_pdiff=False,
             family=None):
        seen.append(dict(mode=mode, family=family, hyp=hyp_, xt=xt, yt=yt, alpha=alpha, hypp=hypp_, xp=xp, yp=yp, alphap=alphap))
        assert Ntest_ == len(Q0_) == len(P0_) and not want_pdiff
        return stepper(first, nm_ - 1, Q0_, P0_)
    monkeypatch.setattr(maps, "run_map_sections", fake)
    monkeypatch.setattr(ts, "_applymap_tok_host", lambda *a: "host loop")
    args = (nph, nm, Ntest, Q0, P0, xtrainp, ztrainp, Kyinvp, hypp, xtrain, ztrain, Kyinv, hyp)
    q, p = ts.applymap_tok(*args)
    assert calls == [(0, 20, Ntest)]
    g = seen[0]
    assert g["mode"] == maps.WRAP_Q | maps.LOSS_NEGP and g["family"] == "A"
    assert np.array_equal(g["xt"], xtrain[:N]) and np.array_equal(g["yt"], xtrain[N:]) and np.array_equal(g["hyp"], hyp)
    assert np.array_equal(g["xp"], xtrainp[:Np]) and np.array_equal(g["yp"], xtrainp[Np:]) and np.array_equal(g["hypp"], hypp)
    for m in range(nph):
        assert np.array_equal(g["alpha"][:, m], Kyinv[m] @ ztrain[:, m]) and np.array_equal(g["alphap"][:, m], Kyinvp[m] @ ztrainp[:, m])
    qr, pr = _reference_loop(nph, nm, Ntest, Q0, P0, None)
    assert np.array_equal(q, qr, equal_nan=True) and np.array_equal(p, pr, equal_nan=True)
    del calls[:]
    q, p = ts.applymap_tok(*args, compute_r=_compute_r, steps_per_launch=7)
    assert [c[:2] for c in calls] == [(0, 7), (3, 7), (2, 6)]
    qr, pr = _reference_loop(nph, nm, Ntest, Q0, P0, _compute_r)
    assert np.array_equal(q, qr, equal_nan=True) and np.array_equal(p, pr, equal_nan=True)
    assert ts.applymap_tok(*args, compute_r=_compute_r) == "host loop"
