"""GPU tests of the sectioned map (sgpr_applymap_sections_host, maps.run_map_sections, examples/tokamak_split.applymap_tok):
nsec GP pairs applied in turn, every step in one launch.  The yardstick for the bits is the one-section map
(sgpr_applymap_host / maps.run_map_alpha) called once per step with the current section's data -- wherever that kernel runs
one workgroup per orbit a step of the new kernel has its bits; for the values it is the reference's recorded tokamak fixture
and the reference loop restated with the CPU oracle's rows and MINPACK."""
import functools
import os

import numpy as np
import pytest
import scipy.linalg
import scipy.optimize

pytestmark = pytest.mark.gpu

TWO_PI = 2.0 * np.pi
TOL = dict(rtol=1e-8, atol=1e-8)   # the reference's own applymap tolerance (test_sympgpr.py:92-93)


@pytest.fixture(scope="module", autouse=True)
def _device():
    import sympgpr_amd
    if sympgpr_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need the MI355X")


def _oracle():
    from oracle.oracle import Oracle
    return Oracle()


def _solve(K, z):
    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(K, lower=True, check_finite=False), z, check_finite=False)


@functools.lru_cache(maxsize=None)
def _sections(fam, nsec, n0, n0p, seed0=101):
    """Gentle symplectic maps as training data, P' = p - eps sin q, Q = q + eps P', one per section with its own seed, eps and
    hyp; n0 points for the symplectic GP, n0p (its own points) for the regular GP of the first guess.  -> dict of stacked
    arrays, one column (hyp: one row) per section."""
    orc = _oracle()
    noise = 1e-8 if max(n0, n0p) <= 80 else 1e-5        # (a tame alpha for the larger, rank-deficient Gram matrices)
    cols = {k: [] for k in ("hyp", "hypp", "xt", "yt", "alpha", "xp", "yp", "alphap")}
    for s in range(nsec):
        rng = np.random.default_rng(seed0 + 7 * s)
        eps = 0.3 - 0.04 * s
        lx, ly, sig = 1.2 * (1 + 0.05 * s), 1.5 * (1 - 0.04 * s), 1.0 - 0.1 * s
        hyp = np.array([lx, ly, 0.5, sig]) if fam == "D" else np.array([lx, ly, sig])
        hypp = hyp * (1 + 0.02 * s)
        if fam == "D":
            hypp[2] = 0.5

        def pts(n):
            q, pn = rng.uniform(0, TWO_PI, n), rng.uniform(-1, 1, n)
            return q, pn, pn + eps * np.sin(q), q + eps * pn
        q, pn, p_old, Q = pts(n0)
        K = orc.build_K(fam, q, pn, q, pn, hyp, threads=4) + noise * np.eye(2 * n0)
        alpha = _solve(K, np.hstack((p_old - pn, Q - q)))
        qg, png, pg_old, _ = pts(n0p)
        Kp = orc.buildKreg(fam, qg, pg_old, qg, pg_old, hypp, threads=4) + noise * np.eye(n0p)
        alphap = _solve(Kp, png)
        for k, v in zip(cols, (hyp, hypp, q, pn, alpha, qg, pg_old, alphap)):
            cols[k].append(v)
    d = {k: np.stack(v, axis=1) for k, v in cols.items()}
    d["hyp"], d["hypp"] = d["hyp"].T.copy(), d["hypp"].T.copy()
    for v in d.values():
        v.setflags(write=False)
    d["fam"], d["nsec"] = fam, nsec
    return d


def _run(d, mode, nm, Q0, P0, first=0, want_pdiff=False):
    from sympgpr_amd import maps
    return maps.run_map_sections(mode, nm, len(Q0), d["hyp"], d["xt"], d["yt"], d["alpha"], Q0, P0, d["hypp"], d["xp"], d["yp"],
                                 d["alphap"], first=first, want_pdiff=want_pdiff, family=d["fam"])


def _one_section(d, m, mode, nm, Q0, P0):
    """sgpr_applymap_host (the entry behind maps.run_map_alpha, with its pdiff) on section m's data -> qmap, pmap, pdiff"""
    from sympgpr_amd import _lib as L
    from sympgpr_amd import maps
    lib, f = L.load_library(), L.f64
    n = len(Q0)
    xt, yt, al, hyp = f(d["xt"][:, m]), f(d["yt"][:, m]), f(d["alpha"][:, m]), f(d["hyp"][m])
    xp, yp, alp, hp = f(d["xp"][:, m]), f(d["yp"][:, m]), f(d["alphap"][:, m]), f(d["hypp"][m])
    Q0, P0 = f(Q0), f(P0)
    q, p, pd = np.zeros((nm, n)), np.zeros((nm, n)), np.zeros((nm, n))
    L.check(lib.sgpr_applymap_host(L.family_id(d["fam"]), int(mode), nm, n, L.dptr(hyp), len(hyp), len(xt), L.dptr(xt), L.dptr(yt),
                                   L.dptr(al), L.dptr(hp), len(hp), len(xp), L.dptr(xp), L.dptr(yp), L.dptr(alp), L.dptr(Q0),
                                   L.dptr(P0), L.dptr(q), L.dptr(p), L.dptr(pd)), "sgpr_applymap_host")
    q2, p2 = maps.run_map_alpha(mode, nm, n, hyp, Q0, P0, xt, yt, al, hp, xp, yp, alp, family=d["fam"])
    assert np.array_equal(q, q2, equal_nan=True) and np.array_equal(p, p2, equal_nan=True)
    return q, p, pd


def _chain(d, mode, nm, Q0, P0, first=0):
    """the orbit built from single steps of the one-section map: step i with section (first + i) mod nsec on the previous row.
    -> qmap, pmap, and the running sum of the single steps' pdiff increments"""
    n = len(Q0)
    q, p, pd = (np.zeros((nm, n)) for _ in range(3))
    q[0], p[0], pd[0] = Q0, P0, P0
    for i in range(nm - 1):
        qq, pp, dd = _one_section(d, (first + i) % d["nsec"], mode, 2, q[i], p[i])
        q[i + 1], p[i + 1] = qq[1], pp[1]
        pd[i + 1] = pd[i] + (dd[1] - dd[0])
    return q, p, pd


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _starts(n, seed, low_every=0):
    rng = np.random.default_rng(seed)
    Q0, P0 = rng.uniform(0.5, 5.5, n), rng.uniform(0.3, 0.7, n)
    if low_every:
        P0[::low_every] = 0.02           # close to P = 0: SGPR_MAP_LOSS_NEGP bites
    return Q0, P0


def _ntest_without_teams(n0):
    """the chain needs the one-section kernel to run one workgroup per orbit: the first of 520, 1040, 2080 orbits at which it
    does (with that many orbits the device has no workgroups to spare for teams)"""
    from sympgpr_amd import _lib as L
    probe = L.load_probe_library()
    found = [n for n in (520, 1040, 2080) if probe.sgpr_probe_map_team(n, n0) == 1]
    assert found, "the one-section map shares every orbit among workgroups at n0 = %d up to 2080 orbits" % n0
    return found[0]


# ---- 1. one section is the old map

@pytest.mark.parametrize("fam,mode,low", [("A", 1, 0), ("C", 1, 0), ("D", 1, 0), ("A", 1 | 2, 0), ("A", 1 | 8, 2), ("B", 4 | 2, 0)],
                         ids=["A-wrapq", "C-wrapq", "D-wrapq", "A-wrapq-wrapp", "A-wrapq-lossnegp", "B-explicit-wrapp"])
def test_one_section_is_the_one_section_map(fam, mode, low):
    d = _sections(fam, 1, 40, 40)
    Q0, P0 = _starts(8, 5, low)
    if mode & 2:
        P0[1::3] = -P0[1::3]             # negative momenta: P mod 2 pi really wraps
    q, p, pd = _run(d, mode, 7, Q0, P0, want_pdiff=True)
    qr, pr, pdr = _one_section(d, 0, mode, 7, Q0, P0)
    assert _same(q, qr) and _same(p, pr) and _same(pd, pdr)
    assert np.isfinite(p[-1]).any()
    if mode & 8:
        assert np.isnan(p[-1]).any()
    if mode & 2:
        assert np.any(np.abs(pd[1] - p[1]) > 1.0)


# ---- 2. many sections are a chain of single steps

MODE_TOK = 1 | 8                        # WRAP_Q | LOSS_NEGP: the tokamak map


@pytest.fixture(scope="module")
def chain3():
    d = _sections("A", 3, 40, 43)
    Q0, P0 = _starts(8, 6, 2)
    return d, Q0, P0, {first: _chain(d, MODE_TOK, 10, Q0, P0, first) for first in (0, 1, 2)}


@pytest.mark.parametrize("first", [0, 1, 2])
def test_sections_are_a_chain_of_single_steps(chain3, first):
    d, Q0, P0, ref = chain3
    qr, pr, pdr = ref[first]
    q, p, pd = _run(d, MODE_TOK, 10, Q0, P0, first=first, want_pdiff=True)
    assert _same(q, qr) and _same(p, pr)                         # the NaN pattern included
    assert np.array_equal(np.isnan(pd), np.isnan(p))
    ok = np.isfinite(pd)
    err = np.abs(pd[ok] - pdr[ok]).max()
    bound = 4 * np.finfo(float).eps * np.abs(pd[ok]).max()
    print("first %d: max |pdiff - running sum| = %.3e, bound %.3e" % (first, err, bound))
    assert err <= bound
    lost = np.isnan(p[-1])
    assert lost.any() and (~lost).any()
    if first:
        assert not _same(p, ref[0][1])                           # the sections differ: `first` matters


def test_chunks_continue_with_the_right_section(chain3):
    d, Q0, P0, ref = chain3
    for first in (0, 2):
        q, p = np.zeros((10, 8)), np.zeros((10, 8))
        q[0], p[0] = Q0, P0
        for i in range(0, 9, 4):
            kk = min(4, 9 - i)
            qq, pp = _run(d, MODE_TOK, kk + 1, q[i], p[i], first=(first + i) % 3)
            q[i + 1:i + kk + 1], p[i + 1:i + kk + 1] = qq[1:], pp[1:]
        assert _same(q, ref[first][0]) and _same(p, ref[first][1])


# ---- 3. size edges

@pytest.mark.parametrize("n0", [1, 63, 64, 65, 255, 256, 257])
def test_size_edges(n0):
    d = _sections("A", 2, n0, n0 + 3)
    ntest = 3 if n0 <= 256 else _ntest_without_teams(n0)         # n0 <= 256 cannot get a team in the one-section kernel
    Q0, P0 = _starts(ntest, 7)
    q, p, pd = _run(d, 1, 4, Q0, P0, first=1, want_pdiff=True)
    qr, pr, _ = _chain(d, 1, 4, Q0, P0, first=1)
    assert _same(q, qr) and _same(p, pr)
    assert np.isfinite(p[-1]).any()


# ---- 4. both sides of the staging rule

@pytest.mark.parametrize("n0,n0p,nm", [(320, 320, 5), (321, 320, 5), (1300, 1300, 3)], ids=["staged-8960", "unstaged-8964", "unstaged-1300"])
def test_both_sides_of_the_staging_rule(n0, n0p, nm):
    nsec = 4
    assert (nsec * (4 * n0 + 3 * n0p) <= 8960) == (n0 == 320) and (n0 != 320 or nsec * (4 * n0 + 3 * n0p) == 8960)
    d = _sections("A", nsec, n0, n0p)
    ntest = _ntest_without_teams(n0)
    Q0, P0 = _starts(ntest, 8)
    q, p = _run(d, 1, nm, Q0, P0, first=2)
    qr, pr, _ = _chain(d, 1, nm, Q0, P0, first=2)
    assert _same(q, qr) and _same(p, pr)
    assert np.isfinite(p[-1]).any()


# ---- 5. orbits are independent

def test_orbits_are_independent():
    d = _sections("A", 3, 40, 43)
    Q0, P0 = _starts(8, 9, 3)
    q, p, pd = _run(d, MODE_TOK, 6, Q0, P0, first=1, want_pdiff=True)
    for k in range(8):
        q1, p1, pd1 = _run(d, MODE_TOK, 6, Q0[k:k + 1], P0[k:k + 1], first=1, want_pdiff=True)
        assert _same(q1[:, 0], q[:, k]) and _same(p1[:, 0], p[:, k]) and _same(pd1[:, 0], pd[:, k])
    Qn, Pn = Q0.copy(), P0.copy()
    Qn[2], Pn[5] = np.nan, np.nan
    qn, pn, pdn = _run(d, MODE_TOK, 6, Qn, Pn, first=1, want_pdiff=True)
    for k in (2, 5):
        assert np.isnan(qn[1:, k]).all() and np.isnan(pn[1:, k]).all() and np.isnan(pdn[1:, k]).all()
    keep = [k for k in range(8) if k not in (2, 5)]
    assert _same(qn[:, keep], q[:, keep]) and _same(pn[:, keep], p[:, keep]) and _same(pdn[:, keep], pd[:, keep])


# ---- 6. the reference's own fixture

def _compute_r(z, rstart):
    """fieldlines.compute_r (tokamak physics beside the path): 20 Newton steps on p_th = A_th(r, th),
    A_th = B0 (r^2/2 - r^3 cos(th) / (3 R0)) with B0 = R0 = 1"""
    r = rstart
    for _ in range(20):
        y = z[0] - (r * r / 2 - r**3 / 3 * np.cos(z[1]))
        dy = -(r - r * r * np.cos(z[1]))
        r = r - y / dy
    return r


def test_reference_fixture(golden_dir):
    """05_tokamak/Split_SympGPR recorded from the reference's own code (tests/golden/make_flow_golden.py): N = 70 points per
    section, 4 sections, nm = 25, 8 orbits, with the recorded alpha / alphap (Kyinv = I, ztrain = alpha hands them through).
    The reference solves with MINPACK hybrd1 at 1e-13, the device with its secant: 1e-7, as test_tokamak_split_flow has it."""
    from sympgpr_amd.examples import tokamak_split as ts
    g = np.load(os.path.join(golden_dir, "driver_tokamak_split.npz"))
    N, nph, nm, Ntest = int(g["N"]), int(g["nphmap"]), int(g["nm"]), int(g["Ntest"])
    assert (N, nph, nm, Ntest) == (70, 4, 25, 8)
    want_nan = np.zeros((nm, Ntest), dtype=bool)
    want_nan[1:, 5] = True
    assert np.array_equal(np.isnan(g["pmap"]), want_nan) and not (g["pmap"] == 0).all(axis=1).any()     # what the fixture holds
    xtrain, xtrainp = np.vstack((g["q"], g["P"])), np.vstack((g["q"], g["p"]))
    Kyinv, Kyinvp = np.stack([np.eye(2 * N)] * nph), np.stack([np.eye(N)] * nph)
    out = []
    for k in (1, 4, 24):
        q, p = ts.applymap_tok(nph, nm, Ntest, g["Q0map"], g["P0map"], xtrainp, g["alphap"].T, Kyinvp, g["hypp"], xtrain,
                               g["alpha"].T, Kyinv, g["hyp"], compute_r=_compute_r, steps_per_launch=k)
        out.append((q, p))
    q, p = out[0]
    assert np.array_equal(np.isnan(p), want_nan) and np.array_equal(np.isnan(q), want_nan)
    ok = ~want_nan
    rel = np.linalg.norm(p[ok] - g["pmap"][ok]) / np.linalg.norm(g["pmap"][ok])          # the measure of test_tokamak_split_flow
    ang = np.abs(np.mod(q[ok] - g["qmap"][ok] + np.pi, TWO_PI) - np.pi).max()
    print("fixture: pmap rel %.3e, qmap angle %.3e" % (rel, ang))
    assert rel <= 1e-7 and ang <= 1e-7
    for q2, p2 in out[1:]:
        assert _same(q2, q) and _same(p2, p)


# ---- 7. against MINPACK on the oracle's rows

def test_against_minpack_on_the_oracle_rows(oracle):
    d = _sections("A", 2, 40, 43)
    nm, Ntest = 8, 8
    Q0, P0 = _starts(Ntest, 10, 2)
    qr, pr = np.zeros((nm, Ntest)), np.zeros((nm, Ntest))
    qr[0], pr[0] = Q0, P0
    for i in range(nm - 1):                                    # Split_SympGPR/func.py:196-218 without compute_r
        m = i % 2
        rows = lambda q, P: oracle.predict_rows("A", [q], [P], d["xt"][:, m], d["yt"][:, m], d["hyp"][m], d["alpha"][:, m])
        for k in range(Ntest):
            if np.isnan(pr[i, k]):
                qr[i + 1, k] = pr[i + 1, k] = np.nan
                continue
            g0 = oracle.predict_reg("A", [qr[i, k]], [pr[i, k]], d["xp"][:, m], d["yp"][:, m], d["hypp"][m], d["alphap"][:, m])[0]
            f = lambda P: rows(qr[i, k], P[0])[0][0] - pr[i, k] + P[0]
            Pn = scipy.optimize.fsolve(f, [g0], xtol=1e-13)[0]
            if Pn < 0.0:
                qr[i + 1, k] = pr[i + 1, k] = np.nan
                continue
            pr[i + 1, k] = Pn
            qr[i + 1, k] = np.mod(rows(qr[i, k], Pn)[1][0] + qr[i, k], TWO_PI)
    q, p = _run(d, MODE_TOK, nm, Q0, P0)
    alive = ~np.isnan(pr)
    assert np.array_equal(np.isnan(p), ~alive) and np.array_equal(np.isnan(q), ~alive)
    assert alive[-1].any() and (~alive).any()
    np.testing.assert_allclose(p[alive], pr[alive], **TOL)
    np.testing.assert_allclose(q[alive], qr[alive], **TOL)


# ---- 8. trivial calls

def test_trivial_calls():
    d = _sections("A", 3, 40, 43)
    q, p, pd = _run(d, MODE_TOK, 5, np.zeros(0), np.zeros(0), want_pdiff=True)
    assert q.shape == p.shape == pd.shape == (5, 0)
    Q0, P0 = _starts(8, 11)
    q, p, pd = _run(d, MODE_TOK, 1, Q0, P0, first=2, want_pdiff=True)
    assert np.array_equal(q, Q0[None]) and np.array_equal(p, P0[None]) and np.array_equal(pd, P0[None])
