"""GPU tests of the backward sectioned map (csrc/map.hip: map_step_inverse, applymap_sections_inverse_kernel;
sgpr_applymap_sections_inverse_host; maps.run_map_sections_inverse, maps.run_map_inverse, maps.last_section;
examples/tokamak_split.applymap_tok_inverse) on the data of tests/test_gpu_applymap_sections.py (_sections, _starts).

Reference: the NumPy restatement tests/ref_sections_inverse.py on the CPU oracle's rows (tests/test_applymap_sections_inverse_cpu.py
holds it against MINPACK), run backwards from the last row of the CPU's MINPACK forward orbit.  Tolerance: rtol = atol = 1e-8, the
project's and the reference's map tolerance; a wrapped q is compared by its distance on the circle (ref_inverse.circle_distance),
so that a value at 0 / 2 pi cannot fail.  The secant counts are held against the restatement's plus 2, the margin
tests/test_gpu_applymap_inverse.py gives: the kernel's sums round differently from the oracle's."""
import os

import numpy as np
import pytest

from tests import ref_inverse as RI
from tests import ref_sections_inverse as RS
from tests.test_gpu_applymap_sections import MODE_TOK, _compute_r, _run, _same, _sections, _starts

pytestmark = pytest.mark.gpu

TOL = 1e-8
NM, NTEST = 8, 8


@pytest.fixture(scope="module", autouse=True)
def _device():
    import sympgpr_amd
    if sympgpr_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need the MI355X")


def _inv(d, mode, nm, Q0, P0, first=0, return_iters=False):
    from sympgpr_amd import maps
    return maps.run_map_sections_inverse(mode, nm, len(Q0), d["hyp"], d["xt"], d["yt"], d["alpha"], Q0, P0, first=first,
                                         family=d["fam"], return_iters=return_iters)


def _compare(q, p, qr, pr, wrap, atol=TOL, what=""):
    """|x - ref| <= atol + 1e-8 |ref| for every entry (numpy.testing.assert_allclose's rule), q on the circle where it is wrapped"""
    assert q.shape == qr.shape and p.shape == pr.shape
    assert np.isfinite(q).all() and np.isfinite(p).all() and np.isfinite(qr).all() and np.isfinite(pr).all()
    dq, dp = (RI.circle_distance(q, qr) if wrap else np.abs(q - qr)), np.abs(p - pr)
    print("%smax |dq| = %.3e  max |dp| = %.3e" % (what, dq.max(), dp.max()))
    assert (dp <= atol + TOL * np.abs(pr)).all(), dp.max()
    assert (dq <= atol + TOL * np.abs(qr)).all(), dq.max()


CASES = [("A", RS.WRAP_Q), ("C", 0), ("D", RS.WRAP_Q)]


@pytest.fixture(scope="module")
def refs(oracle):
    """per family: 3 sections of 40 points, the CPU forward orbit (MINPACK) of NM rows from _starts(8, 10), the restatement's
    backward orbit from its last row with first = last_section(0, NM, 3) -- computed once, never changed"""
    from sympgpr_amd import maps
    out = {}
    for fam, mode in CASES:
        d = _sections(fam, 3, 40, 43)
        Q0, P0 = _starts(NTEST, 10)
        qf, pf = RS.forward_orbit(oracle, d, mode, NM, Q0, P0)[:2]
        assert np.isfinite(qf).all() and np.isfinite(pf).all()
        first = maps.last_section(0, NM, 3)
        qb, pb, its, res, _ = RS.backward_orbit(oracle, d, mode, NM, qf[-1], pf[-1], first)
        for a in (qf, pf, qb, pb, its):
            a.setflags(write=False)
        out[fam] = dict(d=d, mode=mode, first=first, qf=qf, pf=pf, Qe=qf[-1], Pe=pf[-1], q=qb, p=pb, its=its)
    return out


# ---- 1. parity with the CPU backward orbit, 2. iteration counts

@pytest.mark.parametrize("fam", [c[0] for c in CASES])
def test_parity_with_the_cpu_backward_orbit_and_iteration_counts(refs, fam):
    r = refs[fam]
    wrap = bool(r["mode"] & RS.WRAP_Q)
    q, p, it = _inv(r["d"], r["mode"], NM, r["Qe"], r["Pe"], first=r["first"], return_iters=True)
    assert np.array_equal(q[0], r["Qe"]) and np.array_equal(p[0], r["Pe"])
    _compare(q, p, r["q"], r["p"], wrap, what="%s against the restatement: " % fam)
    # ... and the backward orbit is the CPU's forward orbit read from its end
    _compare(q, p, r["qf"][::-1], r["pf"][::-1], wrap, what="%s against the CPU forward orbit: " % fam)
    cpu = int(r["its"].max())
    print("secant updates: device %d..%d, restatement %d..%d" % (it.min(), it.max(), r["its"].min(), cpu))
    assert it.shape == (NM - 1, NTEST) and it.dtype == np.int32
    assert cpu <= 12
    assert it.min() >= 0 and it.max() <= cpu + 2, it
    q2, p2 = _inv(r["d"], r["mode"], NM, r["Qe"], r["Pe"], first=r["first"])             # without iters: the same bits
    assert _same(q2, q) and _same(p2, p)


# ---- 3. device round trip

@pytest.mark.parametrize("fam,nsec,n0,mode", [("A", 4, 70, RS.WRAP_Q), ("B", 3, 40, 0)], ids=["A-4x70-wrapq", "B-3x40-mode0"])
def test_round_trip_on_the_device(fam, nsec, n0, mode):
    """run_map_sections forward, run_map_sections_inverse from its last row: row i is forward row nm - 1 - i within 1e-8.  A at
    the drivers' size; B (the sum kernel, whose r2 does not depend on q: the first secant point is the root, one update confirms
    it) with mode 0, the implicit map."""
    from sympgpr_amd import maps
    d = _sections(fam, nsec, n0, n0)
    nm = 10
    Q0, P0 = _starts(NTEST, 12)
    qf, pf = _run(d, mode, nm, Q0, P0, first=1)
    assert np.isfinite(qf).all() and np.isfinite(pf).all()
    q, p, it = _inv(d, mode, nm, qf[-1], pf[-1], first=maps.last_section(1, nm, nsec), return_iters=True)
    assert np.isfinite(q).all() and np.isfinite(p).all()
    dq = RI.circle_distance(q, qf[::-1]) if mode & RS.WRAP_Q else np.abs(q - qf[::-1])
    dp = np.abs(p - pf[::-1])
    print("%s device round trip: max |dq| = %.3e  max |dp| = %.3e  secant updates %d..%d" % (fam, dq.max(), dp.max(), it.min(), it.max()))
    assert dq.max() <= TOL and dp.max() <= TOL
    assert (it >= 0).all()
    if fam == "B":
        assert it.max() <= 1, it


# ---- 4. chain and chunks

@pytest.mark.parametrize("first", [0, 1, 2])
def test_one_launch_is_a_chain_of_single_steps_and_of_chunks(refs, first):
    r = refs["A"]
    d, Qe, Pe = r["d"], r["Qe"], r["Pe"]
    q, p, it = _inv(d, MODE_TOK, NM, Qe, Pe, first=first, return_iters=True)
    assert np.isfinite(p[-1]).any()
    qc, pc, ic = np.zeros_like(q), np.zeros_like(p), np.zeros_like(it)
    qc[0], pc[0] = Qe, Pe
    for i in range(NM - 1):                                     # single steps (nm = 2) chained on the host
        qq, pp, ii = _inv(d, MODE_TOK, 2, qc[i], pc[i], first=(first - i) % 3, return_iters=True)
        assert _same(qq[0], qc[i]) and _same(pp[0], pc[i])
        qc[i + 1], pc[i + 1], ic[i] = qq[1], pp[1], ii[0]
    assert _same(q, qc) and _same(p, pc) and np.array_equal(it, ic)
    qa, pa, ia = _inv(d, MODE_TOK, 4, Qe, Pe, first=first, return_iters=True)            # rows 0 .. 3, then 3 .. 7
    qb, pb, ib = _inv(d, MODE_TOK, NM - 3, qa[-1], pa[-1], first=(first - 3) % 3, return_iters=True)
    assert _same(np.vstack((qa, qb[1:])), q) and _same(np.vstack((pa, pb[1:])), p) and np.array_equal(np.vstack((ia, ib)), it)
    if first != r["first"]:
        assert not _same(p, _inv(d, MODE_TOK, NM, Qe, Pe, first=r["first"])[1])          # the sections differ: `first` matters


# ---- 5. LOSS_NEGP

def test_loss_negp(oracle):
    d = _sections("A", 2, 40, 43)
    Q0, P0 = _starts(8, 10, 2)
    qr, pr, itr = RS.backward_orbit(oracle, d, MODE_TOK, NM, Q0, P0, first=1)[:3]
    lost = np.isnan(pr[-1])
    print("restatement: %d of 8 orbits lost by the last row" % lost.sum())
    assert lost.any() and (~lost).any()
    q, p, it = _inv(d, MODE_TOK, NM, Q0, P0, first=1, return_iters=True)
    assert np.array_equal(np.isnan(p), np.isnan(pr)) and np.array_equal(np.isnan(q), np.isnan(pr))
    assert np.array_equal(it == -1, np.isnan(pr[1:]))
    alive = ~np.isnan(pr)
    dq, dp = RI.circle_distance(q[alive], qr[alive]), np.abs(p[alive] - pr[alive])
    print("alive values: max |dq| = %.3e  max |dp| = %.3e" % (dq.max(), dp.max()))
    assert (dq <= TOL + TOL * np.abs(qr[alive])).all() and (dp <= TOL + TOL * np.abs(pr[alive])).all()
    assert np.array_equal(q[0], Q0) and np.array_equal(p[0], P0)                         # row 0 is not tested: P0 = 0.02 stays


# ---- 6. size edges

@pytest.mark.parametrize("n0", [1, 63, 64, 65, 255, 256, 257])
def test_size_edges(oracle, n0):
    """one section, one backward step from the CPU forward image of the start points, against the CPU backward step; atol scales
    with max |r| met by the reference, as test_kernel_edges of tests/test_gpu_applymap_inverse.py scales with max |G|"""
    d = _sections("A", 1, n0, 5)
    Q0, P0 = _starts(3, 7)
    qf, pf, _, _, r1 = RS.forward_orbit(oracle, d, RS.WRAP_Q, 2, Q0, P0)
    qr, pr, itr, _, r2 = RS.backward_orbit(oracle, d, RS.WRAP_Q, 2, qf[1], pf[1])
    assert np.isfinite(qr).all() and np.isfinite(pr).all()
    q, p, it = _inv(d, RS.WRAP_Q, 2, qf[1], pf[1], return_iters=True)
    atol = TOL * max(1.0, r1, r2)
    _compare(q, p, qr, pr, True, atol=atol, what="n0 = %d  max |r| = %.3g  updates %d..%d  " % (n0, max(r1, r2), it.min(), it.max()))
    _compare(q[1:], p[1:], Q0[None], P0[None], True, atol=atol, what="n0 = %d against the start of the CPU forward step: " % n0)
    assert (it >= 0).all()


# ---- 7. both sides of the staging rule

@pytest.mark.parametrize("nsec,n0", [(7, 320), (7, 321), (2, 1300)], ids=["staged-8960", "unstaged-8988", "unstaged-2x1300"])
def test_both_sides_of_the_staging_rule(oracle, nsec, n0):
    from sympgpr_amd import maps
    assert (nsec * 4 * n0 <= 8960) == (n0 == 320) and (n0 != 320 or nsec * 4 * n0 == 8960)
    d = _sections("A", nsec, n0, 40)
    nm = 4
    Q0, P0 = _starts(4, 8)
    qf, pf, _, _, r1 = RS.forward_orbit(oracle, d, RS.WRAP_Q, nm, Q0, P0, first=2 % nsec)
    first = maps.last_section(2 % nsec, nm, nsec)
    qr, pr, itr, _, r2 = RS.backward_orbit(oracle, d, RS.WRAP_Q, nm, qf[-1], pf[-1], first)
    q, p, it = _inv(d, RS.WRAP_Q, nm, qf[-1], pf[-1], first=first, return_iters=True)
    atol = TOL * max(1.0, r1, r2)
    _compare(q, p, qr, pr, True, atol=atol, what="%d x %d  max |r| = %.3g  updates %d..%d  " % (nsec, n0, max(r1, r2), it.min(), it.max()))
    _compare(q, p, qf[::-1], pf[::-1], True, atol=atol, what="%d x %d against the CPU forward orbit: " % (nsec, n0))
    assert (it >= 0).all()


# ---- 8. orbit independence and lost orbits

def test_orbits_are_independent_and_lost_orbits_stay_alone(refs):
    r = refs["A"]
    d, Qe, Pe, first = r["d"], r["Qe"], r["Pe"], r["first"]
    q0, p0, i0 = _inv(d, RS.WRAP_Q, NM, Qe, Pe, first=first, return_iters=True)
    assert np.isfinite(q0).all() and (i0 >= 0).all()
    Qn, Pn = Qe.copy(), Pe.copy()
    Qn[2], Pn[5] = np.nan, np.inf
    q, p, it = _inv(d, RS.WRAP_Q, NM, Qn, Pn, first=first, return_iters=True)
    for k in (2, 5):
        assert np.isnan(q[1:, k]).all() and np.isnan(p[1:, k]).all() and (it[:, k] == -1).all()
    assert np.isnan(q[0, 2]) and p[0, 2] == Pe[2] and q[0, 5] == Qe[5] and p[0, 5] == np.inf       # row 0 echoes the inputs
    keep = [k for k in range(NTEST) if k not in (2, 5)]
    assert _same(q[:, keep], q0[:, keep]) and _same(p[:, keep], p0[:, keep]) and np.array_equal(it[:, keep], i0[:, keep])
    # a repeated call, another ntest, another index
    q2, p2, i2 = _inv(d, RS.WRAP_Q, NM, Qe, Pe, first=first, return_iters=True)
    assert _same(q2, q0) and _same(p2, p0) and np.array_equal(i2, i0)
    for k in range(NTEST):
        q1, p1, i1 = _inv(d, RS.WRAP_Q, NM, Qe[k:k + 1], Pe[k:k + 1], first=first, return_iters=True)
        assert _same(q1[:, 0], q0[:, k]) and _same(p1[:, 0], p0[:, k]) and np.array_equal(i1[:, 0], i0[:, k])
    q3, p3 = _inv(d, RS.WRAP_Q, NM, Qe[::-1].copy(), Pe[::-1].copy(), first=first)
    assert _same(q3[:, ::-1], q0) and _same(p3[:, ::-1], p0)


# ---- 9. the d = 1 map backwards

def test_run_map_inverse_undoes_the_one_pair_map(oracle):
    """maps.run_map_inverse from the end of the teamed d = 1 kernel's forward orbit (maps.run_map_alpha) on the data of
    test_d1_pairs_fit_undoes_the_one_pair_map: its rows come back within 1e-8; and it agrees within 1e-8 with
    SympFit.pairs(...).applymap_pairs_inverse on the same fit -- another kernel, Newton in place of the secant."""
    from tests.test_gpu_examples import _training as training_d1
    from sympgpr_amd import maps
    from sympgpr_amd.fit import SympFit
    t = training_d1(oracle, "A")
    nm, Ntest = 6, 5
    rng = np.random.default_rng(5)
    Q0, P0 = rng.uniform(0.5, 5.5, Ntest), rng.uniform(-0.6, 0.6, Ntest)
    with SympFit.pairs("A", np.column_stack((t["q"], t["pn"])), t["ztrain"], t["hyp"], 1e-8) as f:
        alpha = f.run().alpha()
        qf, pf = maps.run_map_alpha(maps.WRAP_Q, nm, Ntest, t["hyp"], Q0, P0, t["q"], t["pn"], alpha, hypp=t["hypp"],
                                    xp=t["q"], yp=t["p_old"], alphap=t["alphap"], family="A")
        assert np.isfinite(qf).all() and np.isfinite(pf).all()
        qn, pn = f.applymap_pairs_inverse(nm, qf[-1], pf[-1], wrap_q=True)
    q, p, it = maps.run_map_inverse(maps.WRAP_Q, nm, Ntest, t["hyp"], qf[-1], pf[-1], t["q"], t["pn"], alpha, family="A",
                                    return_iters=True)
    assert q.shape == p.shape == (nm, Ntest) and it.shape == (nm - 1, Ntest) and (it >= 0).all()
    assert np.isfinite(q).all() and np.isfinite(p).all()
    dq, dp = RI.circle_distance(q, qf[::-1]), np.abs(p - pf[::-1])
    print("d = 1 against the one-pair map: max |dq| = %.3e  max |dp| = %.3e  updates %d..%d" % (dq.max(), dp.max(), it.min(), it.max()))
    assert dq.max() <= TOL and dp.max() <= TOL
    dq, dp = RI.circle_distance(q, qn[:, :, 0]), np.abs(p - pn[:, :, 0])
    print("d = 1 against the D = 2 Newton kernel: max |dq| = %.3e  max |dp| = %.3e" % (dq.max(), dp.max()))
    assert dq.max() <= TOL and dp.max() <= TOL


# ---- 10. the tokamak driver backwards

def test_applymap_tok_inverse_on_the_reference_fixture(golden_dir):
    """forward with applymap_tok (no callback, one launch), backward from its last row with the matching start: the alive orbits
    return to the fixture's start points within 1e-7, the tolerance test_reference_fixture uses for this data; with a callback,
    1, 4 and 24 steps per launch give the same bits"""
    from sympgpr_amd.examples import tokamak_split as ts
    g = np.load(os.path.join(golden_dir, "driver_tokamak_split.npz"))
    N, nph, nm, Ntest = int(g["N"]), int(g["nphmap"]), int(g["nm"]), int(g["Ntest"])
    assert (N, nph, nm, Ntest) == (70, 4, 25, 8)
    xtrain, xtrainp = np.vstack((g["q"], g["P"])), np.vstack((g["q"], g["p"]))
    Kyinv, Kyinvp = np.stack([np.eye(2 * N)] * nph), np.stack([np.eye(N)] * nph)
    qf, pf = ts.applymap_tok(nph, nm, Ntest, g["Q0map"], g["P0map"], xtrainp, g["alphap"].T, Kyinvp, g["hypp"], xtrain, g["alpha"].T,
                             Kyinv, g["hyp"])
    assert ts.map_steps(nph, nm) == nm - 1                       # the forward loop fills every row here
    alive = np.isfinite(pf[-1])
    assert alive.sum() >= 4
    start = (nm - 1) % nph
    q, p = ts.applymap_tok_inverse(nph, nm, Ntest, qf[-1], pf[-1], xtrain, g["alpha"].T, Kyinv, g["hyp"], start=start)
    assert q.shape == p.shape == (nm, Ntest)
    assert np.isnan(p[1:, ~alive]).all() and np.isfinite(p[:, alive]).all() and np.isfinite(q[:, alive]).all()
    Q0, P0 = np.broadcast_to(g["Q0map"], (Ntest,)), np.broadcast_to(g["P0map"], (Ntest,))
    ang = RI.circle_distance(q[-1, alive], np.mod(Q0[alive], 2 * np.pi)).max()
    dp = np.abs(p[-1, alive] - P0[alive]).max()
    dall = max(RI.circle_distance(q[:, alive], qf[::-1][:, alive]).max(), np.abs(p[:, alive] - pf[::-1][:, alive]).max())
    print("fixture: back at the start points within %.3e (angle), %.3e (momentum); every row within %.3e" % (ang, dp, dall))
    assert ang <= 1e-7 and dp <= 1e-7 and dall <= 1e-7
    out = [ts.applymap_tok_inverse(nph, nm, Ntest, qf[-1], pf[-1], xtrain, g["alpha"].T, Kyinv, g["hyp"], start=start,
                                   compute_r=_compute_r, steps_per_launch=k) for k in (1, 4, 24)]
    for q2, p2 in out[1:]:
        assert _same(q2, out[0][0]) and _same(p2, out[0][1])
    kept = np.isfinite(out[0][1])                                # what the callback keeps has the bits of the one launch
    assert kept[-1].any() and _same(out[0][0][kept], q[kept]) and _same(out[0][1][kept], p[kept])


# ---- 11. nothing else moved

def test_the_forward_maps_did_not_move(refs):
    from sympgpr_amd import maps
    d = refs["A"]["d"]
    Q0, P0 = _starts(NTEST, 10, 2)
    args = (MODE_TOK, NM, NTEST, d["hyp"], d["xt"], d["yt"], d["alpha"], Q0, P0, d["hypp"], d["xp"], d["yp"], d["alphap"])
    f0 = maps.run_map_sections(*args, first=1, want_pdiff=True, family="A")
    t0 = maps.run_map_sections_tangent(*args, first=1, family="A")
    qb, pb = _inv(d, RS.WRAP_Q, NM, refs["A"]["Qe"], refs["A"]["Pe"], first=refs["A"]["first"])
    assert np.isfinite(qb).all()
    f1 = maps.run_map_sections(*args, first=1, want_pdiff=True, family="A")
    t1 = maps.run_map_sections_tangent(*args, first=1, family="A")
    assert all(_same(a, b) for a, b in zip(f0, f1))
    assert _same(t0[0], t1[0]) and _same(t0[1], t1[1]) and _same(t0[0], f0[0]) and _same(t0[1], f0[1])
    assert sorted(t0[2]) == sorted(t1[2]) == ["jac", "lyap", "mono"] and all(_same(t0[2][k], t1[2][k]) for k in t0[2])


# ---- 12. trivial calls

def test_trivial_calls(refs):
    r = refs["A"]
    q, p, it = _inv(r["d"], MODE_TOK, 5, np.zeros(0), np.zeros(0), return_iters=True)
    assert q.shape == p.shape == (5, 0) and it.shape == (4, 0)
    q, p, it = _inv(r["d"], MODE_TOK, 1, r["Qe"], r["Pe"], first=2, return_iters=True)
    assert np.array_equal(q, r["Qe"][None]) and np.array_equal(p, r["Pe"][None]) and it.shape == (0, NTEST) and it.dtype == np.int32
