"""GPU tests of the periodic-orbit search of the d-pair map (csrc/periodic_nd.h: periodic_nd_kernel; sgpr_fit_periodic_nd,
sgpr_periodic_nd_host; SympFit.periodic_orbits, maps.run_periodic_nd) on the cases of tests/test_periodic_cpu.py: at most 60
training points, n <= 4, one to six guesses per call.  tol = 1e-12, maxit = 30 throughout; the stateless entry gets the oracle's
alpha, the handle its own.

Reference: tests/ref_periodic.py at the same tol, in the same mode (the data of test_gpu_applymap_nd.py with WRAP_Q for the
families A and D and unwrapped for C; the twist cases wrapped, the d = 1 ones unwrapped as well).

Tolerances, none taken from the device:
  * z: |z - z_ref|_inf <= 4 |(mono_ref - I)^-1|_inf tol max(1, |z_ref|_inf).  Both sides stop at a residual <= tol max(1, |z|),
    which leaves each |(mono - I)^-1| tol max(1, |z|) from the root to first order: a factor 2; another 2 covers second-order terms
    and the rounding difference between the two evaluations of G (n dG <= 5e-13 < tol on the CPU, by permuting the summation).
  * its <= its_ref + 1.
  * mono against ref_tangent.monodromy along the REFERENCE'S OWN converged orbit: per step matrix the bound of
    test_gpu_applymap_tangent.py, 64 D eps kappa_inf(I + B_ref) max(1, |M_ref|_inf), accumulated over the product (each step's
    error times the norms of the other steps) plus that file's n D eps prod |M_i|_inf for the product itself -- and, because
    mono is the monodromy of the RETURNED orbit, which starts z - z_ref away from the reference's, the first-order change of
    the reference's monodromy over that distance, doubled for the second order: 2 sum_j max|d mono_ref / d z_j| |z_j - z_ref,j|,
    the derivative by central differences (h = 1e-6) of one pass of ref_periodic around z_ref.  Without that term the two
    unwrapped d = 1 twist cases lay outside on the device: 1.03e-12 against 6.97e-13 (n = 3, |(mono - I)^-1| = 164) and 2.13e-12
    against 1.88e-12 (n = 4, 324); the other 26 were inside.
  * in addition, mono against the same product along the reference's orbit FROM THE RETURNED POINT (one pass of ref_periodic
    from the device's z), where no such term arises: the accumulated per-step bound alone.
  * the residual recomputed on the host from the existing map's rows: within 4 (2 pi) eps of resid -- the four roundings of
    q_n - q_0 and the reduction at magnitude 2 pi -- and <= tol max(1, |z|) + 4 (2 pi) eps.
  * mono against run_map_nd_tangent's from z: that file's n D eps prod |M_i|_inf.
  * the handle against the stateless entry: 1e-8, the map's own parity tolerance."""
import numpy as np
import pytest

from tests import ref_periodic as RP
from tests import ref_tangent as RT
from tests.test_gpu_applymap_nd import _hyp, _training
from tests.test_periodic_cpu import CASES, IDS, TWO_PI, arg_errors, host_call, model

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TOL, MAXIT = 1e-12, 30
GCASES = [(c, c["data"] == "twist" or c["fam"] != "C") for c in CASES] + [(c, False) for c in CASES if c["d"] == 1]
GIDS = IDS + [i + "-unwrapped" for i, c in zip(IDS, CASES) if c["d"] == 1]


@pytest.fixture(scope="module", autouse=True)
def _device():
    import sympgpr_amd
    if sympgpr_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need the MI355X")


_refs = {}


def ref(oracle, c, wrap):
    """ref_periodic's answer for a case in a mode -- computed once, never changed"""
    key = (c["data"], c["fam"], c["d"], c["n"], c["guess"], wrap)
    if key not in _refs:
        m = model(oracle, c)
        s = RP.solve(c["fam"], c["d"], m["hyp"], m["X"], m["alpha"], c["guess"], c["n"], wind=np.array(c["w"], dtype=np.float64),
                     wrap=wrap, tol=TOL, maxit=MAXIT)
        assert s["converged"] and s["history"][0] >= 1e-2
        w, D, h = np.array(c["w"], dtype=np.float64), 2 * c["d"], 1e-6
        s["dmono"] = np.array([np.abs(RP.one_pass(c["fam"], c["d"], m["hyp"], m["X"], m["alpha"], s["z"] + h * e, c["n"], w, wrap)[1] -
                                      RP.one_pass(c["fam"], c["d"], m["hyp"], m["X"], m["alpha"], s["z"] - h * e, c["n"], w, wrap)[1]).max()
                               / (2 * h) for e in np.eye(D)])                            # max |d mono / d z_j| around z_ref
        for a in (s["z"], s["mono"], s["q"], s["p"], s["M"], s["K"], s["dmono"]):
            a.setflags(write=False)
        _refs[key] = s
    return _refs[key]


def run(oracle, c, wrap, guesses=None, wind=None, **kw):
    from sympgpr_amd import maps
    m, d = model(oracle, c), c["d"]
    g = np.atleast_2d(np.array(c["guess"] if guesses is None else guesses, dtype=np.float64))
    w = np.array(c["w"]) if wind is None else wind
    kw.setdefault("tol", TOL)
    kw.setdefault("maxit", MAXIT)
    return maps.run_periodic_nd(c["fam"], d, maps.WRAP_Q if wrap else 0, c["n"], m["hyp"], m["X"], m["alpha"], g[:, :d], g[:, d:],
                                wind=w, **kw)


def _inf(M):
    return np.abs(M).sum(axis=-1).max(axis=-1)


@pytest.mark.parametrize("c,wrap", GCASES, ids=GIDS)
def test_parity_with_ref_periodic(oracle, c, wrap):
    r, d, n = ref(oracle, c, wrap), c["d"], c["n"]
    D = 2 * d
    out = run(oracle, c, wrap, orbit=True)
    z, zr = out["z"][0], r["z"]
    bound = 4 * r["inv_norm"] * TOL * max(1.0, np.abs(zr).max())
    print("its %d (ref %d)  resid %.3e (ref %.3e)  max |z - z_ref| = %.3e (bound %.3e)  |(mono - I)^-1| = %.3g"
          % (out["its"][0], r["its"], out["resid"][0], r["resid"], np.abs(z - zr).max(), bound, r["inv_norm"]))
    assert out["converged"][0] and out["its"].dtype == np.int32 and out["z"].shape == (1, D)
    assert np.abs(z - zr).max() <= bound
    assert 1 <= out["its"][0] <= r["its"] + 1
    assert out["resid"][0] <= TOL * max(1.0, np.abs(z).max())
    # the monodromy: ref_tangent's step matrices along the reference's own orbit, and what z - z_ref does to them
    nrm = _inf(r["M"])
    per_step = 64 * D * EPS * np.array([np.linalg.cond(r["K"][i], np.inf) for i in range(n)]) * np.maximum(1.0, nrm)
    acc = sum(per_step[i] * np.prod(np.delete(nrm, i)) for i in range(n)) + n * D * EPS * np.prod(nrm)
    moved = 2 * float(r["dmono"] @ np.abs(z - zr))
    want = RT.monodromy(r["M"])
    err = np.abs(out["mono"][0] - want).max()
    print("   along the reference's own orbit: max |mono - mono_ref| = %.3e (bound %.3e = %.3e per step + %.3e for z - z_ref)"
          % (err, acc + moved, acc, moved))
    assert np.abs(want - r["mono"]).max() <= n * D * EPS * np.prod(nrm)
    assert err <= acc + moved
    # ... and along the reference's orbit from the returned point
    m = model(oracle, c)
    _, mono_ref, _, _, Ms, Ks = RP.one_pass(c["fam"], d, m["hyp"], m["X"], m["alpha"], z, n, np.array(c["w"], dtype=np.float64), wrap)
    nrm = _inf(Ms)
    per_step = 64 * D * EPS * np.array([np.linalg.cond(Ks[i], np.inf) for i in range(n)]) * np.maximum(1.0, nrm)
    acc = sum(per_step[i] * np.prod(np.delete(nrm, i)) for i in range(n)) + n * D * EPS * np.prod(nrm)
    want = RT.monodromy(Ms)
    err = np.abs(out["mono"][0] - want).max()
    print("   from the returned point: max |mono - mono_ref| = %.3e (bound %.3e)  |mono|_inf = %.3g" % (err, acc, _inf(want)))
    assert np.abs(want - mono_ref).max() <= n * D * EPS * np.prod(nrm)
    assert err <= acc


@pytest.mark.parametrize("c,wrap", GCASES, ids=GIDS)
def test_it_is_the_existing_map(oracle, c, wrap):
    from sympgpr_amd import maps
    m, d, n, w = model(oracle, c), c["d"], c["n"], np.array(c["w"], dtype=np.float64)
    D = 2 * d
    out = run(oracle, c, wrap, orbit=True)
    assert out["converged"][0] and out["q"].shape == (n, 1, d) and out["p"].shape == (n, 1, d)
    z = out["z"]
    mode = maps.WRAP_Q if wrap else 0
    args = (c["fam"], d, mode, n + 1, m["hyp"], m["X"], m["alpha"], z[:, :d], z[:, d:])
    q, p = maps.run_map_nd(*args)
    assert np.isfinite(q).all() and np.isfinite(p).all()
    assert q[:n].tobytes() == out["q"].tobytes() and p[:n].tobytes() == out["p"].tobytes()
    assert q[0].tobytes() == z[:, :d].tobytes() and p[0].tobytes() == z[:, d:].tobytes()
    # the residual again, on the host, from the existing map's rows: the q part reduced mod 2 pi
    rq = q[n, 0] - q[0, 0] - TWO_PI * w
    rq = rq - TWO_PI * np.round(rq / TWO_PI)
    rhost = max(np.abs(rq).max(), np.abs(p[n, 0] - p[0, 0]).max())
    slack = 4 * TWO_PI * EPS
    print("resid %.3e  on the host %.3e  (tol max(1, |z|) = %.3e)" % (out["resid"][0], rhost, TOL * max(1.0, np.abs(z).max())))
    assert abs(rhost - out["resid"][0]) <= slack
    assert rhost <= TOL * max(1.0, np.abs(z).max()) + slack
    # the winding numbers, from an unwrapped run of the existing entry
    qu, pu = maps.run_map_nd(c["fam"], d, 0, n + 1, m["hyp"], m["X"], m["alpha"], z[:, :d], z[:, d:])
    assert (np.round((qu[n, 0] - qu[0, 0]) / TWO_PI) == w).all()
    # the monodromy, from the tangent entry
    _, _, _, t = maps.run_map_nd_tangent(*args, lyap=False)
    prod = np.prod(_inf(t["jac"][:, 0]))
    err = np.abs(out["mono"][0] - t["mono"][0]).max()
    print("   max |mono - tangent entry's| = %.3e (bound %.3e)" % (err, n * D * EPS * prod))
    assert err <= n * D * EPS * prod


def _batch(oracle, data, fam, d, n):
    """the guesses of one data set, family, d and n as one batch: (case of the first, guesses (k, 2d), wind (k, d))"""
    cs = [c for c in CASES if (c["data"], c["fam"], c["d"], c["n"]) == (data, fam, d, n)]
    return cs, np.array([c["guess"] for c in cs]), np.array([c["w"] for c in cs])


def _same(a, b, ia, ib, names=("z", "resid", "its", "mono", "q", "p")):
    return [k for k in names if k in a and not np.array_equal(a[k][:, ia] if k in "qp" else a[k][ia],
                                                              b[k][:, ib] if k in "qp" else b[k][ib], equal_nan=True)]


def test_independence(oracle):
    """a guess's bits depend on its own inputs only: not on a repeated call, the batch, its index, or the outputs asked for"""
    cs, g, w = _batch(oracle, "twist", "A", 2, 3)
    assert len(cs) == 3
    a = run(oracle, cs[0], True, g, w, orbit=True)
    b = run(oracle, cs[0], True, g, w, orbit=True)
    assert a["converged"].all()
    for k in range(3):
        assert _same(a, b, k, k) == []
    alone = run(oracle, cs[0], True, g[2:3], w[2:3], orbit=True)
    moved = run(oracle, cs[0], True, g[1:3], w[1:3], orbit=True)
    assert _same(alone, a, 0, 2) == [] and _same(moved, a, 1, 2) == [] and _same(moved, a, 0, 1) == []
    bare = run(oracle, cs[0], True, g, w, mono=None, orbit=None)
    assert sorted(bare) == ["converged", "its", "resid", "z"]
    assert all(_same(bare, a, k, k, ("z", "resid", "its")) == [] for k in range(3))


@pytest.mark.parametrize("fam,d,data,n", [("A", 2, "twist", 3), ("D", 3, "fixed", 4), ("C", 2, "fixed", 1)])
def test_handle_entry_agrees_with_the_stateless_one(oracle, fam, d, data, n):
    from sympgpr_amd.fit import SympFit
    cs, g, w = _batch(oracle, data, fam, d, n)
    m, wrap = model(oracle, cs[0]), fam != "C"
    a = run(oracle, cs[0], wrap, g, w, orbit=True)
    with SympFit.pairs(fam, m["X"], m["z"], m["hyp"], m["sig2n"]) as f:
        h = f.run().periodic_orbits(n, g[:, :d], g[:, d:], wind=w, wrap_q=wrap, tol=TOL, maxit=MAXIT, orbit=True)
    assert a["converged"].all() and h["converged"].all()
    for k in ("z", "mono", "q", "p"):
        np.testing.assert_allclose(h[k], a[k], rtol=1e-8, atol=1e-8, err_msg=k)
    assert (h["resid"] <= TOL * np.maximum(1.0, np.abs(h["z"]).max(axis=1))).all()


def test_d1_through_sympfit_and_through_pairs(oracle):
    from sympgpr_amd.fit import SympFit
    cs = [c for c in CASES if c["d"] == 1]
    m = model(oracle, cs[0])
    for c in cs:
        g, w = np.array(c["guess"]), np.array(c["w"])
        with SympFit("A", m["X"][:, 0], m["X"][:, 1], m["z"], m["hyp"], m["sig2n"]) as f:
            a = f.run().periodic_orbits(c["n"], g[:1], g[1:], wind=w, wrap_q=True, tol=TOL, maxit=MAXIT, orbit=True)
        with SympFit.pairs("A", m["X"], m["z"], m["hyp"], m["sig2n"]) as f:
            b = f.run().periodic_orbits(c["n"], g[None, :1], g[None, 1:], wind=w[None, :], wrap_q=True, tol=TOL, maxit=MAXIT, orbit=True)
        assert a["converged"].all() and b["converged"].all() and a["z"].shape == (1, 2) and a["q"].shape == (c["n"], 1, 1)
        for k in ("z", "mono", "q", "p"):
            np.testing.assert_allclose(a[k], b[k], rtol=1e-8, atol=1e-8, err_msg=k)


def test_failure_is_reported_never_faked(oracle):
    cs, g, w = _batch(oracle, "twist", "A", 2, 3)
    n, d = 3, 2
    good = run(oracle, cs[0], True, g, w, orbit=True)
    its_ref = [ref(oracle, c, True)["its"] for c in cs]
    # one pass is never enough from these guesses (the first residual is >= 1e-2: checked where the references are made)
    one = run(oracle, cs[0], True, g, w, orbit=True, maxit=1)
    assert (one["its"] == -1).all() and not one["converged"].any()
    for k in ("z", "resid", "mono", "q", "p"):
        assert np.isnan(one[k]).all(), k
    # a NaN guess fails alone; the others keep their bits
    gn = g.copy()
    gn[1, 3] = np.nan
    out = run(oracle, cs[0], True, gn, w, orbit=True)
    assert out["its"][1] == -1 and not out["converged"][1]
    assert np.isnan(out["z"][1]).all() and np.isnan(out["resid"][1]) and np.isnan(out["mono"][1]).all()
    assert np.isnan(out["q"][:, 1]).all() and np.isnan(out["p"][:, 1]).all()
    assert _same(out, good, 0, 0) == [] and _same(out, good, 2, 2) == []
    # maxit = its_ref + 1 is enough, guess by guess; a batch takes the largest
    for k, c in enumerate(cs):
        o = run(oracle, c, True, maxit=its_ref[k] + 1)
        assert o["converged"][0] and _same(o, good, 0, k, ("z", "resid", "its", "mono")) == []
    # maxit below a guess's need fails that guess only
    short = run(oracle, cs[0], True, g, w, orbit=True, maxit=int(good["its"].max()) - 1)
    lost = good["its"] > good["its"].max() - 1
    assert (short["its"][lost] == -1).all() and np.isnan(short["z"][lost]).all()
    for k in np.flatnonzero(~lost):
        assert _same(short, good, k, k) == []


@pytest.mark.parametrize("what", sorted(arg_errors()))
def test_argument_errors(what):
    from sympgpr_amd import _lib
    assert host_call(**arg_errors()[what]) == _lib.E_ARG, what
    assert host_call() == 0


def test_modes_states_and_empty_calls(oracle):
    from sympgpr_amd import SympGPRError, maps
    from sympgpr_amd.fit import SympFit
    c = [c for c in CASES if (c["data"], c["fam"], c["d"], c["n"]) == ("fixed", "A", 2, 1)][0]
    m, d = model(oracle, c), 2
    g = np.array([c["guess"]])
    with pytest.raises(SympGPRError, match=r"periodic_nd_host.*sum kernels"):
        maps.run_periodic_nd("A", d, maps.EXPLICIT, 1, m["hyp"], m["X"], m["alpha"], g[:, :d], g[:, d:])
    with pytest.raises(ValueError):
        maps.run_periodic_nd("A", d, maps.WRAP_P, 1, m["hyp"], m["X"], m["alpha"], g[:, :d], g[:, d:])
    for bad in (dict(n=0), dict(maxit=0), dict(tol=0.0), dict(tol=float("nan"))):
        kw = dict(n=1, tol=TOL, maxit=MAXIT)
        kw.update(bad)
        with pytest.raises(SympGPRError, match=r"\(-1\)"):
            maps.run_periodic_nd("A", d, 0, kw["n"], m["hyp"], m["X"], m["alpha"], g[:, :d], g[:, d:], tol=kw["tol"], maxit=kw["maxit"])
    # the sum kernel's explicit map is accepted and finds its orbits: its separable data, the fixed point near (pi, pi) and its
    # n = 2 repetition (ref_periodic converges there in 3 and 4 passes: asserted, not assumed)
    Xb, zb = _training(d, c=0.0)
    hb = _hyp("B", d)
    ab = oracle.fit_nd("B", Xb, zb, hb, 1e-8)[0]
    for nb in (1, 2):
        out = maps.run_periodic_nd("B", d, maps.WRAP_Q | maps.EXPLICIT, nb, hb, Xb, ab, g[:, :d], g[:, d:], tol=TOL, maxit=MAXIT)
        rb = RP.solve("B", d, hb, Xb, ab, c["guess"], nb, wrap=True, tol=TOL, maxit=MAXIT, explicit=True)
        assert rb["converged"] and rb["history"][0] >= 1e-2
        assert out["converged"][0] and 1 <= out["its"][0] <= rb["its"] + 1
        assert np.abs(out["z"][0] - rb["z"]).max() <= 4 * rb["inv_norm"] * TOL * max(1.0, np.abs(rb["z"]).max())
    with SympFit.pairs("A", m["X"], m["z"], m["hyp"], 1e-8) as f:
        with pytest.raises(SympGPRError, match=r"\(-5\).*not solved"):
            f.periodic_orbits(1, g[:, :d], g[:, d:])
        with pytest.raises(SympGPRError, match=r"fit_periodic_nd.*sum kernels"):
            f.run().periodic_orbits(1, g[:, :d], g[:, d:], explicit=True)
        e = f.periodic_orbits(2, np.zeros((0, d)), np.zeros((0, d)), orbit=True)
        assert e["z"].shape == (0, 4) and e["its"].shape == (0,) and e["mono"].shape == (0, 4, 4) and e["q"].shape == (2, 0, d)
    x, y = m["X"][:, 0], m["X"][:, 2]
    with SympFit("A", x, y, m["z"][:len(x)], [1.2, 1.5, 1.0], 1e-2, reg=True) as f:
        with pytest.raises(SympGPRError, match=r"\(-5\).*scalar-kernel"):
            f.run().periodic_orbits(1, x[:3], y[:3])
    with SympFit("A", x, y, m["z"][:len(x)], [1.2, 1.5, 1.0], 1e-2, block="qq") as f:
        with pytest.raises(SympGPRError, match=r"\(-5\).*single-block"):
            f.run().periodic_orbits(1, x[:3], y[:3])
    e = maps.run_periodic_nd("A", d, 0, 3, m["hyp"], m["X"], m["alpha"], np.zeros((0, d)), np.zeros((0, d)), orbit=True)
    assert e["z"].shape == (0, 4) and e["resid"].shape == (0,) and e["converged"].shape == (0,) and e["p"].shape == (3, 0, d)
