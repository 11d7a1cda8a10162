"""GPU tests of the workgroup teams of the d = 1 map (applymap_kernel in sympgpr_amd/csrc/map.hip): S = 1 .. 16 workgroups share
an orbit, each sums its slice of the training points and all add the parts in member order.  Every case runs through
maps.run_map_alpha and is held, step by step from the device's own rows, to the long-double reference of tests/ref_map.py
within bounds derived there (none is measured on the kernel); tests/test_applymap_team_cpu.py asserts the preconditions of
those bounds for every case.  The guess GP cannot be seen in the outputs: its witness is the number of rows calls
(sgpr_probe_map_calls), which the start points are chosen to make comparable with the reference's.

The team sizes are those of 256 CUs (512 workgroup slots); each case asserts its own from the library first, so on another
device it fails instead of quietly testing something else.  SGPR_E_HIP ("did not answer in time") from any case says that
the members of a team were not resident together: a finding about co-residency, not something to retry."""
import functools

import numpy as np
import pytest

from tests import ref_map as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    import sympgpr_amd
    if sympgpr_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need the MI355X")


def _probe():
    from sympgpr_amd import _lib as L
    return L.load_probe_library()


def _assert_team(ntest, n0, S):
    got = _probe().sgpr_probe_map_team(ntest, n0)
    assert got == S, ("%d orbits on %d points run in teams of %d here, not the %d this case is written for (256 CUs, 512 workgroup "
                      "slots): it would test another geometry" % (ntest, n0, got, S))


def _run(d, mode, nm, Q0=None, P0=None, want_pdiff=True):
    """maps.run_map_alpha on the problem d -> qmap, pmap, pdiff (None if not wanted), rows calls of the launch"""
    from sympgpr_amd import maps
    Q0, P0 = d["Q0"] if Q0 is None else Q0, d["P0"] if P0 is None else P0
    g = (None, None, None, None) if mode & R.EXPLICIT else (d["hypp"], d["xp"], d["yp"], d["alphap"])
    try:
        out = maps.run_map_alpha(mode, nm, len(Q0), d["hyp"], Q0, P0, d["xt"], d["yt"], d["alpha"], *g, family=d["fam"],
                                 want_pdiff=want_pdiff)
    except Exception as e:
        if "did not answer in time" in str(e):
            pytest.fail("a team member waited in vain (%s): the workgroups of a team were not resident together" % e)
        raise
    calls = int(_probe().sgpr_probe_map_calls())
    return (out[0], out[1], out[2] if want_pdiff else None, calls)


@functools.lru_cache(maxsize=None)
def _case_run(case_id):
    c = next(c for c in R.CASES + R.PADDING if c.id == case_id)
    d = R.problem(case_id)
    _assert_team(c.ntest, c.n0, c.S)
    out = _run(d, c.mode, c.nm, want_pdiff=c.want_pdiff)
    for a in out[:3]:
        if a is not None:
            a.setflags(write=False)
    return out


def _report(name, worst):
    for k, v in sorted(worst.items()):
        print("MARGIN %-18s %-9s worst |error| / bound = %.3e" % (name, k, v))


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- 1. team geometry, families and modes: every one-step check, and the call count

@pytest.mark.parametrize("c", R.CASES, ids=repr)
def test_case(c):
    d = R.problem(c.id)
    q, p, pd, calls = _case_run(c.id)
    assert q.shape == p.shape == (c.nm, c.ntest)
    _report(c.id, R.check_steps(d, c.mode, q, p, pd))
    if c.mode & R.LOSS_NEGP:
        lost = np.isnan(p)
        first = np.where(lost.any(axis=0), np.argmax(lost, axis=0), c.nm)
        print("orbits lost from row:", np.bincount(first, minlength=c.nm + 1)[:c.nm])
        assert (first[first < c.nm] > 1).any() and 2 * (first == c.nm).sum() >= c.ntest
    else:
        assert np.isfinite(p).all() and np.isfinite(q).all()
    if c.mode & R.WRAP_P:
        assert np.any(np.abs(pd[1:] - p[1:]) > 1.0)                      # P mod 2 pi really wrapped
    # the reference's number of rows calls: a guess that lost or gained a point, or took another GP's weights, changes it
    print("rows calls: device %d, reference %d" % (calls, d["calls"].sum()))
    assert calls == d["calls"].sum()
    if not c.want_pdiff:                                                  # the null pdiff pointer changes no bit
        q3, p3, _, _ = _case_run("s3")
        assert _same(q, q3) and _same(p, p3)


# ---- 2. lost orbits and independence

@pytest.mark.parametrize("cid", ["s3", "s16-one"])
def test_lost_orbits_and_independence(cid):
    c = next(c for c in R.CASES if c.id == cid)
    d = R.problem(cid)
    q, p, pd, calls = _case_run(cid)
    # a repeated call reproduces every bit
    q2, p2, pd2, calls2 = _run(d, c.mode, c.nm)
    assert _same(q2, q) and _same(p2, p) and _same(pd2, pd) and calls2 == calls
    # NaN starts in the middle of the batch stay NaN from row 1; every other orbit keeps the bits of the run without them
    k1, k2 = c.ntest // 2, c.ntest // 2 + 3
    Qn, Pn = d["Q0"].copy(), d["P0"].copy()
    Qn[k1], Pn[k2] = np.nan, np.nan
    qn, pn, pdn, callsn = _run(d, c.mode, c.nm, Qn, Pn)
    for k in (k1, k2):
        assert np.isnan(qn[1:, k]).all() and np.isnan(pn[1:, k]).all() and np.isnan(pdn[1:, k]).all()
    keep = np.array([k for k in range(c.ntest) if k not in (k1, k2)])
    assert _same(qn[:, keep], q[:, keep]) and _same(pn[:, keep], p[:, keep]) and _same(pdn[:, keep], pd[:, keep])
    assert callsn == d["calls"][:, keep].sum()                            # a lost orbit makes no call
    # permuting the orbits permutes the rows
    perm = np.random.default_rng(5).permutation(c.ntest)
    qp, pp, pdp, _ = _run(d, c.mode, c.nm, d["Q0"][perm], d["P0"][perm])
    assert _same(qp, q[:, perm]) and _same(pp, p[:, perm]) and _same(pdp, pd[:, perm])


def test_bits_depend_on_the_start_and_the_team_size_only():
    """20 and 25 orbits on 1500 points both run in teams of 6: the 20 shared orbits have the same bits"""
    d = R.problem("guess-short")
    q, p, pd, _ = _case_run("guess-short")
    Qx, Px = R.starts("plain", 5, 77)
    Q0, P0 = np.hstack((Qx[:2], d["Q0"], Qx[2:])), np.hstack((Px[:2], d["P0"], Px[2:]))
    _assert_team(25, 1500, 6)
    q2, p2, pd2, _ = _run(d, R.WRAP_Q, 4, Q0, P0)
    assert _same(q2[:, 2:22], q) and _same(p2[:, 2:22], p) and _same(pd2[:, 2:22], pd)
    assert np.isfinite(p2).all()


# ---- 3. padding with zero weights: the same mathematics in another geometry

def _padded(d, n0, seed, which="sym"):
    """d with zero-weight training points appended up to n0 points and the order of all points shuffled -- the symplectic GP
    (zeros in both halves of alpha) or the guess GP"""
    rng = np.random.default_rng(seed)
    e = dict(d)
    x, y, a = ("xt", "yt", "alpha") if which == "sym" else ("xp", "yp", "alphap")
    old = len(d[x])
    perm = rng.permutation(n0)
    e[x] = np.hstack((d[x], rng.uniform(0, R.TWO_PI, n0 - old)))[perm]
    e[y] = np.hstack((d[y], rng.uniform(-1, 1, n0 - old)))[perm]
    halves = d[a].reshape(-1, old)
    e[a] = np.hstack([np.hstack((h, np.zeros(n0 - old)))[perm] for h in halves])
    return e


def test_zero_weight_padding_of_the_training_set():
    """explicit map, one step: Praw = p - r1(q, p) and Q = q + r2(q, Praw) of the padded, shuffled problems against the base.
    The elementwise errors are those of identical device products and cancel; only the order of additions differs:
    |difference| <= (n0_a + n0_b) u T, T = |K*| |alpha| at the point of evaluation."""
    from oracle.oracle import Oracle
    c = next(c for c in R.PADDING if c.id == "pad-explicit")
    d = R.problem(c.id)
    q0, p0, pd0, calls0 = _case_run(c.id)
    _report(c.id, R.check_steps(d, c.mode, q0, p0, pd0))
    assert calls0 == 2 * c.ntest == d["calls"].sum()
    absa = np.abs(d["alpha"])
    K = np.abs(Oracle().build_K("A", d["Q0"], d["P0"], d["xt"], d["yt"], d["hyp"]))
    T1 = (K @ absa)[:c.ntest]
    K = np.abs(Oracle().build_K("A", d["Q0"], p0[1], d["xt"], d["yt"], d["hyp"]))
    T2 = (K @ absa)[c.ntest:]
    for n0, S in ((700, 3), (3841, 16), (20481, 16)):
        e = _padded(d, n0, n0)
        _assert_team(c.ntest, n0, S)
        q, p, pd, calls = _run(e, c.mode, c.nm)
        worst = R.check_steps(e, c.mode, q, p, pd)
        bound = (300 + n0) * R.U
        dP, dQ = np.abs(p[1] - p0[1]), np.abs(q[1] - q0[1])
        worst["pad_P"], worst["pad_Q"] = float((dP / (bound * T1)).max()), float((dQ / (bound * T2)).max())
        _report("%s-%d" % (c.id, n0), worst)
        assert np.all(dP <= bound * T1) and np.all(dQ <= bound * T2)
        assert calls == calls0
    assert np.isfinite(p0).all()


def test_zero_weight_padding_and_permutation_of_the_guess():
    """implicit map: a guess GP padded with zero-weight points from 300 to 3000 (which alone ends the staging), and a permuted
    one.  The outputs pass the implicit check; the number of rows calls is the reference's in every variant."""
    c = next(c for c in R.PADDING if c.id == "pad-guess")
    d = R.problem(c.id)
    q0, p0, pd0, calls0 = _case_run(c.id)
    _report(c.id, R.check_steps(d, c.mode, q0, p0, pd0))
    want = d["calls"].sum()
    print("rows calls: base %d, reference %d" % (calls0, want))
    assert calls0 == want
    for name, e in (("padded", _padded(d, 3000, 31, "guess")), ("permuted", _padded(d, 300, 32, "guess"))):
        assert len(e["xp"]) == len(e["alphap"]) == (3000 if name == "padded" else 300) and not _same(e["xp"][:300], d["xp"])
        _assert_team(c.ntest, c.n0, c.S)
        q, p, pd, calls = _run(e, c.mode, c.nm)
        _report("%s-%s" % (c.id, name), R.check_steps(e, c.mode, q, p, pd))
        print("rows calls: %s %d" % (name, calls))
        assert calls == want
