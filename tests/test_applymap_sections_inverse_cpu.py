"""CPU checks of the backward sectioned map (sgpr_applymap_sections_inverse_host; maps.run_map_sections_inverse, run_map_inverse,
last_section; examples/tokamak_split.applymap_tok_inverse): declared, exported and bound alike; every argument error answered with
SGPR_E_ARG before any device call; the Python wrappers' ValueErrors; the chunk bookkeeping of the backward tokamak driver with a
NumPy stepper; and the NumPy restatement tests/ref_sections_inverse.py -- the CPU reference of
tests/test_gpu_applymap_sections_inverse.py -- held against the MINPACK forward orbit it undoes and against MINPACK on its own
equation.  The device's numbers are checked on the GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ref_inverse as RI
from tests import ref_sections_inverse as RS
from tests.test_gpu_applymap_sections import _sections, _starts

from tests import c_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sgpr_applymap_sections_inverse_host"
_ip = C.POINTER(C.c_int)


def test_header_exports_map_ctypes_table_and_library_agree():
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    dyn = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True, check=True).stdout
    params, args = c_header.assert_bound_as_declared(NAME, 17), L.SIGNATURES[NAME][1]
    assert args[-1] == _ip and params[-1].startswith("int *")
    assert c_header.in_exports_map(NAME), NAME + " is not covered by exports.map"
    assert re.search(r" T %s$" % NAME, dyn, flags=re.M), NAME + " is not exported"
    # sgpr_applymap_sections_host without the guess GPs and pdiff, with iters: the same leading arguments, position by position
    fwd = L.SIGNATURES["sgpr_applymap_sections_host"][1]
    assert args[:12] == fwd[:12] and args[12:16] == fwd[18:22]
    assert lib.sgpr_abi_version() == 5


def _args(**over):
    """a valid call (family A, two sections), as a dict of named arguments in the order of the declaration"""
    from sympgpr_amd import _lib as L
    nsec, n0, ntest, nm = 2, 4, 3, 3
    keep = dict(hyp=np.array([1.2, 1.5, 1.0, 1.1, 1.4, 0.9]), x=np.zeros(n0 * nsec), y=np.zeros(n0 * nsec),
                alpha=np.zeros(2 * n0 * nsec), Q0=np.ones(ntest), P0=np.ones(ntest), qmap=np.zeros((nm, ntest)),
                pmap=np.zeros((nm, ntest)), iters=np.zeros((nm - 1, ntest), dtype=np.int32), hyp8=np.ones(8))
    a = dict(family=0, mode=L.MAP_WRAP_Q | L.MAP_LOSS_NEGP, nsec=nsec, first=1, nm=nm, ntest=ntest, hyp=L.dptr(keep["hyp"]),
             nhyp=3, n0=n0, x=L.dptr(keep["x"]), y=L.dptr(keep["y"]), alpha=L.dptr(keep["alpha"]), Q0=L.dptr(keep["Q0"]),
             P0=L.dptr(keep["P0"]), qmap=L.dptr(keep["qmap"]), pmap=L.dptr(keep["pmap"]), iters=keep["iters"].ctypes.data_as(_ip))
    for k, v in over.items():
        a[k] = L.dptr(keep[v]) if isinstance(v, str) else v
    return a, keep


# every SGPR_E_ARG case of the header: nsec, first, nm, negative sizes, unknown mode bits, WRAP_P (2), EXPLICIT (4) -- with the sum
# kernel B (1) too --, null required pointers, unknown families, a wrong nhyp
BAD = [dict(nsec=0), dict(nsec=-1), dict(first=-1), dict(first=2), dict(nm=0), dict(nm=-1), dict(ntest=-1), dict(n0=-1),
       dict(mode=16), dict(mode=32 | 1), dict(mode=2), dict(mode=1 | 2), dict(mode=2 | 8), dict(mode=4), dict(mode=4 | 1),
       dict(mode=4 | 8), dict(family=1, mode=4), dict(hyp=None), dict(x=None), dict(y=None), dict(alpha=None), dict(Q0=None),
       dict(P0=None), dict(qmap=None), dict(pmap=None), dict(nhyp=4), dict(nhyp=2), dict(family=3), dict(family=9),
       dict(family=-1)]


@pytest.mark.parametrize("over", BAD, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_argument_errors_come_before_any_device_call(over):
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    a, keep = _args(**over)
    assert getattr(lib, NAME)(*a.values()) == L.E_ARG
    msg = lib.sgpr_last_error()
    assert msg != b"" and (b"applymap_sections_inverse_host" in msg or b"hyp must hold" in msg or b"family" in msg), msg


def test_valid_calls_reach_the_device_check():
    """well-formed calls pass every check: without a GPU they end at SGPR_E_NODEVICE, not SGPR_E_ARG -- no iters, nm = 1,
    ntest = 0, every accepted mode, the sum kernel, family D with its period, no training points at all"""
    import sympgpr_amd
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    want = 0 if sympgpr_amd.device_count() > 0 else L.E_NODEVICE
    for over in ({}, dict(iters=None), dict(first=0, nm=1), dict(ntest=0), dict(mode=0), dict(mode=1), dict(mode=8),
                 dict(family=1, mode=0), dict(family=3, nhyp=4, hyp="hyp8"), dict(n0=0, x=None, y=None, alpha=None)):
        a, keep = _args(**over)
        assert getattr(lib, NAME)(*a.values()) == want, over


def test_python_wrappers_validate_before_the_library_is_asked():
    from sympgpr_amd import maps
    nsec, n0 = 3, 4
    assert list(inspect.signature(maps.run_map_sections_inverse).parameters) == [
        "mode", "nm", "Ntest", "hyp", "xt", "yt", "alpha", "Q0", "P0", "first", "family", "return_iters"]
    assert list(inspect.signature(maps.run_map_inverse).parameters) == [
        "mode", "nm", "Ntest", "l", "Q0", "P0", "xt", "yt", "alpha", "family", "return_iters"]
    good = dict(mode=maps.WRAP_Q | maps.LOSS_NEGP, nm=3, Ntest=2, hyp=np.ones((nsec, 3)), xt=np.zeros((n0, nsec)),
                yt=np.zeros((n0, nsec)), alpha=np.zeros((2 * n0, nsec)), Q0=np.ones(2), P0=np.ones(2), first=2, family="A")
    bad = [dict(alpha=np.zeros((2 * n0 - 1, nsec))), dict(alpha=np.zeros((n0, nsec))), dict(yt=np.zeros((n0 + 1, nsec))),
           dict(xt=np.zeros((n0, nsec - 1))), dict(alpha=np.zeros((2 * n0, nsec + 1))), dict(alpha=np.zeros(2 * n0)),
           dict(hyp=np.ones(3)), dict(hyp=np.ones((0, 3))), dict(first=3), dict(first=-1), dict(nm=0), dict(Ntest=-1),
           dict(Q0=np.ones(3)), dict(P0=np.ones(3)),
           dict(mode=maps.WRAP_P), dict(mode=maps.WRAP_Q | maps.WRAP_P), dict(mode=maps.EXPLICIT), dict(mode=16),
           dict(mode=maps.EXPLICIT, family="B")]
    for over in bad:
        with pytest.raises(ValueError):
            maps.run_map_sections_inverse(**dict(good, **over))
    good1 = dict(mode=maps.WRAP_Q, nm=3, Ntest=2, l=[1.2, 1.5, 1.0], Q0=np.ones(2), P0=np.ones(2), xt=np.zeros(n0), yt=np.zeros(n0),
                 alpha=np.zeros(2 * n0), family="A")
    bad1 = [dict(alpha=np.zeros(n0)), dict(yt=np.zeros(n0 + 1)), dict(xt=np.zeros((n0, 1))), dict(l=np.ones((1, 3))), dict(nm=0),
            dict(Q0=np.ones(3)), dict(mode=maps.WRAP_P), dict(mode=maps.EXPLICIT), dict(mode=64)]
    for over in bad1:
        with pytest.raises(ValueError):
            maps.run_map_inverse(**dict(good1, **over))
    assert "last_section" in maps.run_map_sections_inverse.__doc__


def test_last_section_against_a_brute_force_count():
    from sympgpr_amd import maps
    for nsec in (1, 2, 3, 4, 7):
        for first in range(nsec):
            for nm in range(2, 20):
                used = [(first + i) % nsec for i in range(nm - 1)]          # step i -> i + 1 of a forward run uses this section
                assert maps.last_section(first, nm, nsec) == used[-1]
                # ... and walking back from it, step i of the backward run undoes the forward steps in reverse order
                assert [(used[-1] - i) % nsec for i in range(nm - 1)] == used[::-1]
    for bad in ((0, 3, 0), (3, 3, 3), (-1, 3, 3), (0, 0, 3)):
        with pytest.raises(ValueError):
            maps.last_section(*bad)


# ---- the chunk-and-callback bookkeeping of examples/tokamak_split.applymap_tok_inverse, without a GPU

def _step_back(m, Q, P):
    """the exact inverse of tests/test_applymap_sections_cpu.py's kicked rotor of section m up to rounding; p < 0 loses the orbit"""
    q = np.mod(Q - (0.5 + 0.05 * m) * P, 2 * np.pi)
    p = P + (0.05 + 0.02 * m) * np.sin(q + 0.3 * m)
    if not p >= 0.0:
        return np.nan, np.nan
    return q, p


def _back_stepper(nphmap, calls):
    def run(first, steps, Q0, P0):
        calls.append((first, steps, len(Q0)))
        q, p = np.full((steps + 1, len(Q0)), np.nan), np.full((steps + 1, len(Q0)), np.nan)
        q[0], p[0] = Q0, P0
        for s in range(steps):
            for k in range(len(Q0)):
                if not np.isnan(p[s, k]):
                    q[s + 1, k], p[s + 1, k] = _step_back((first - s) % nphmap, q[s, k], p[s, k])
        return q, p
    return run


def _compute_r(zk, r0):
    assert r0 == 0.3
    return 0.005 + 0.5 * np.sin(37.0 * zk[0] * 1e2 + 3.0 * zk[1] + zk[2]) ** 2


def _backward_loop(nphmap, nm, Ntest, Q0, P0, start, compute_r):
    """the driver's contract step by step: row j sits at section index (start - j) mod nphmap, step j undoes pair
    (start - j - 1) mod nphmap, compute_r sees each new row at its own angle"""
    q, p = np.full((nm, Ntest), np.nan), np.full((nm, Ntest), np.nan)
    q[0], p[0] = Q0, P0
    for j in range(nm - 1):
        for k in range(Ntest):
            if np.isnan(p[j, k]):
                continue
            qq, pp = _step_back((start - j - 1) % nphmap, q[j, k], p[j, k])
            if np.isnan(pp):
                continue
            ph = (2 * np.pi) / nphmap * np.mod(start - (j + 1), nphmap)
            if compute_r is not None and compute_r(np.array([pp * 1e-2, qq, ph]), 0.3) > 0.5:
                continue
            q[j + 1, k], p[j + 1, k] = qq, pp
    return q, p


@pytest.mark.parametrize("start", [0, 1, 3])
def test_backward_chunks_with_callback_repeat_the_step_by_step_loop(start):
    from sympgpr_amd.examples.tokamak_split import map_in_chunks_inverse
    nphmap, nm, Ntest = 4, 23, 12
    rng = np.random.default_rng(2024)
    Q0, P0 = rng.uniform(0.0, 2 * np.pi, Ntest), rng.uniform(0.02, 1.0, Ntest)
    qr, pr = _backward_loop(nphmap, nm, Ntest, Q0, P0, start, _compute_r)
    lost = np.isnan(pr[-1])
    assert lost.any() and not lost.all()
    assert np.isnan(pr).sum() > np.isnan(_backward_loop(nphmap, nm, Ntest, Q0, P0, start, None)[1]).sum()
    for chunk in (1, 3, 4, 7, 22, 50):
        calls = []
        q, p = map_in_chunks_inverse(_back_stepper(nphmap, calls), nphmap, nm, Ntest, Q0, P0, start, _compute_r, chunk)
        assert np.array_equal(q, qr, equal_nan=True) and np.array_equal(p, pr, equal_nan=True)      # bit for bit
        assert [c[0] for c in calls] == [(start - 1 - j * chunk) % nphmap for j in range(len(calls))]
        assert sum(c[1] for c in calls) == nm - 1 and all(c[1] <= chunk for c in calls)
    calls = []
    q, p = map_in_chunks_inverse(_back_stepper(nphmap, calls), nphmap, nm, Ntest, Q0, P0, start)
    assert calls == [((start - 1) % nphmap, nm - 1, Ntest)]                                        # no callback: one call
    qr, pr = _backward_loop(nphmap, nm, Ntest, Q0, P0, start, None)
    assert np.array_equal(q, qr, equal_nan=True) and np.array_equal(p, pr, equal_nan=True)
    q, p = map_in_chunks_inverse(None, nphmap, 1, Ntest, Q0, P0, start, _compute_r, 3)             # nm = 1: no step, no call
    assert np.array_equal(q, Q0[None]) and np.array_equal(p, P0[None])


def test_applymap_tok_inverse_routes(monkeypatch):
    """applymap_tok_inverse itself with maps.run_map_sections_inverse replaced: WRAP_Q | LOSS_NEGP, family A, alpha_m = Kyinv[m] @
    ztrain[:, m], and first = (start - 1) mod nphmap; the forward driver undone by it returns to its start points"""
    from sympgpr_amd import maps
    from sympgpr_amd.examples import tokamak_split as ts
    from tests.test_applymap_sections_cpu import _make_stepper
    nph, N, nm, Ntest = 4, 5, 21, 6
    rng = np.random.default_rng(3)
    xtrain, ztrain, Kyinv, hyp = rng.normal(size=(2 * N, nph)), rng.normal(size=(2 * N, nph)), rng.normal(size=(nph, 2 * N, 2 * N)), rng.uniform(1, 2, (nph, 3))
    Q0, P0 = rng.uniform(0.0, 2 * np.pi, Ntest), rng.uniform(0.3, 1.0, Ntest)
    qf, pf = ts.map_in_chunks(_make_stepper(nph, []), nph, nm, Ntest, Q0, P0)                      # 20 forward steps: rows 0 .. 20
    ok = np.isfinite(pf[-1])
    assert ok.sum() >= 3 and np.isfinite(pf[:, ok]).all()
    seen, calls = [], []
    stepper = _back_stepper(nph, calls)

    def fake(mode, nm_, Ntest_, hyp_, xt, yt, alpha, Q0_, P0_, first=0, family=None, return_iters=False):
        seen.append(dict(mode=mode, family=family, hyp=hyp_, xt=xt, yt=yt, alpha=alpha))
        assert Ntest_ == len(Q0_) == len(P0_) and not return_iters
        return stepper(first, nm_ - 1, Q0_, P0_)
    monkeypatch.setattr(maps, "run_map_sections_inverse", fake)
    q, p = ts.applymap_tok_inverse(nph, nm, Ntest, qf[-1], pf[-1], xtrain, ztrain, Kyinv, hyp, start=(nm - 1) % nph)
    assert calls == [(((nm - 1) % nph - 1) % nph, nm - 1, int(ok.sum()))]     # one call, over the orbits that start alive
    g = seen[0]
    assert g["mode"] == maps.WRAP_Q | maps.LOSS_NEGP and g["family"] == "A"
    assert np.array_equal(g["xt"], xtrain[:N]) and np.array_equal(g["yt"], xtrain[N:]) and np.array_equal(g["hyp"], hyp)
    for m in range(nph):
        assert np.array_equal(g["alpha"][:, m], Kyinv[m] @ ztrain[:, m])
    # a wrong section order would not undo the forward steps (each section has its own kick): 20 steps of a map with |dq/dp| < 1
    assert np.isnan(p[1:, ~ok]).all()                                          # an orbit the forward run lost starts NaN: lost
    assert RI.circle_distance(q[:, ok], qf[::-1][:, ok]).max() <= 1e-12 and np.abs(p[:, ok] - pf[::-1][:, ok]).max() <= 1e-12
    del calls[:]
    ts.applymap_tok_inverse(nph, nm, Ntest, qf[-1], pf[-1], xtrain, ztrain, Kyinv, hyp, start=0, compute_r=lambda z, r: 0.0,
                            steps_per_launch=7)
    assert [c[:2] for c in calls] == [(3, 7), (0, 7), (1, 6)]


# ---- tests/ref_sections_inverse.py ---------------------------------------------------------------------------------------------

NM, NTEST = 8, 8
REF_CASES = [("A", 2, RS.WRAP_Q), ("C", 3, 0), ("D", 3, RS.WRAP_Q)]


@pytest.fixture(scope="module")
def problems(oracle):
    """per case: the sections of tests/test_gpu_applymap_sections.py, the MINPACK forward orbit from _starts(8, 10) and the two
    backward orbits from its last row -- computed once, never changed"""
    from sympgpr_amd import maps
    out = {}
    for fam, nsec, mode in REF_CASES:
        d = _sections(fam, nsec, 40, 43)
        Q0, P0 = _starts(NTEST, 10)
        qf, pf = RS.forward_orbit(oracle, d, mode, NM, Q0, P0)[:2]
        assert np.isfinite(qf).all() and np.isfinite(pf).all()
        first = maps.last_section(0, NM, nsec)
        sec = RS.backward_orbit(oracle, d, mode, NM, qf[-1], pf[-1], first)
        mpk = RS.backward_orbit(oracle, d, mode, NM, qf[-1], pf[-1], first, minpack=True)
        out[fam] = dict(d=d, mode=mode, qf=qf, pf=pf, sec=sec, mpk=mpk)
    return out


def _dist(a, b, mode):
    return RI.circle_distance(a, b) if mode & RS.WRAP_Q else np.abs(a - b)


@pytest.mark.parametrize("fam", [c[0] for c in REF_CASES])
def test_restated_backward_orbit_returns_the_minpack_forward_orbit(problems, fam):
    """NM - 1 forward steps by MINPACK, then NM - 1 backward steps by the secant from the last row: row i is forward row
    NM - 1 - i within 1e-8 (measured: <= 1.1e-12; each solve closes to 1e-13 relative and the maps are gentle, |dQ/dq - 1| < 0.3)"""
    r = problems[fam]
    qb, pb, its, res, _ = r["sec"]
    dq, dp = _dist(qb, r["qf"][::-1], r["mode"]), np.abs(pb - r["pf"][::-1])
    print("family %s: round trip max |dq| = %.3e  max |dp| = %.3e  closing residual %.3e  secant updates %d..%d"
          % (fam, dq.max(), dp.max(), res.max(), its.min(), its.max()))
    assert np.isfinite(qb).all() and np.isfinite(pb).all()
    assert dq.max() <= 1e-8 and dp.max() <= 1e-8
    assert its.min() >= 0 and its.max() <= 12 and res.max() <= 1e-8


@pytest.mark.parametrize("fam", [c[0] for c in REF_CASES])
def test_restated_secant_agrees_with_minpack_backwards(problems, fam):
    r = problems[fam]
    dq, dp = _dist(r["sec"][0], r["mpk"][0], r["mode"]), np.abs(r["sec"][1] - r["mpk"][1])
    print("family %s: secant against MINPACK max |dq| = %.3e  max |dp| = %.3e" % (fam, dq.max(), dp.max()))
    assert np.isfinite(r["mpk"][0]).all()
    assert dq.max() <= 1e-8 and dp.max() <= 1e-8


def test_restated_loss_rules(oracle):
    """LOSS_NEGP loses an orbit whose solved p is negative, from that row on, and only with the bit set; a NaN or infinite start
    value is lost at once (the data of the GPU test's case 5)"""
    d = _sections("A", 2, 40, 43)
    Q0, P0 = _starts(8, 10, 2)
    q, p, its, _, _ = RS.backward_orbit(oracle, d, RS.WRAP_Q | RS.LOSS_NEGP, NM, Q0, P0, first=1)
    q0, p0 = RS.backward_orbit(oracle, d, RS.WRAP_Q, NM, Q0, P0, first=1)[:2]
    lost = np.isnan(p[-1])
    print("LOSS_NEGP: %d of %d orbits lost by the last row" % (lost.sum(), len(lost)))
    assert lost.any() and (~lost).any()
    assert np.isfinite(p0).all() and np.array_equal(np.isnan(q), np.isnan(p))
    for k in range(8):
        neg = np.nonzero(p0[1:, k] < 0.0)[0]
        if len(neg):                                    # NaN from the first negative p on, the rows before it untouched
            i = neg[0] + 1
            assert np.isnan(p[i:, k]).all() and np.array_equal(p[:i, k], p0[:i, k]) and (its[i - 1:, k] == -1).all()
        else:
            assert np.array_equal(p[:, k], p0[:, k]) and np.array_equal(q[:, k], q0[:, k])
    for bad in ((np.nan, 0.5), (1.0, np.inf), (-np.inf, 0.5)):
        q, p, its = RS.backward_orbit(oracle, d, RS.WRAP_Q, 3, [bad[0]], [bad[1]], first=0)[:3]
        assert np.isnan(q[1:]).all() and np.isnan(p[1:]).all() and (its == -1).all()
