"""CPU side of the team tests of the d = 1 map (applymap_kernel in sympgpr_amd/csrc/map.hip; the GPU side is
tests/test_gpu_applymap_team.py): the reference of tests/ref_map.py against the oracle's own rows, the preconditions under
which the GPU cases' tolerances and call counts hold, asserted from the reference for every case, the geometry each case is
there to reach, and the co-residency contract of the teams read from the compiler's resource remarks."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import ref_map as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP_TT, MAP_STAGE = 256, 5              # map.hip: threads of a workgroup, rounds a member keeps in LDS


# ---- the reference

@pytest.mark.parametrize("n0", [7, 300])
@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
def test_sums_against_the_oracle_rows(oracle, fam, n0):
    d = R.training(fam, n0, n0, 7)
    rng = np.random.default_rng(8)
    q, P = rng.uniform(0, R.TWO_PI, 9), rng.uniform(-1, 1, 9)
    r1, r2, B1, B2 = R.sums(fam, d["hyp"], d["xt"], d["yt"], d["alpha"], q, P)
    o1, o2 = oracle.predict_rows(fam, q, P, d["xt"], d["yt"], d["hyp"], d["alpha"])
    assert np.all(B1 > 0) and np.all(B2 > 0) and max(B1.max(), B2.max()) < 1e-11
    assert np.all(np.abs(r1 - o1) <= B1) and np.all(np.abs(r2 - o2) <= B2)
    assert np.abs(r1).max() > 1e-3 and np.abs(r2).max() > 1e-3
    g = R.guess(fam, d["hypp"], d["xp"], d["yp"], d["alphap"], q, P)
    K = oracle.buildKreg(fam, q, P, d["xp"], d["yp"], d["hypp"])
    Bg = (n0 * R.U + 3e-13) * (np.abs(K) @ np.abs(d["alphap"])) + 4e-15 * np.abs(K).max() * np.abs(d["alphap"]).sum()
    assert np.all(np.abs(g - oracle.predict_reg(fam, q, P, d["xp"], d["yp"], d["hypp"], d["alphap"])) <= Bg)


def test_a_zero_weight_point_changes_no_reference_sum():
    d = R.training("A", 300, 300, 7)
    q, P = np.array([1.0, 4.0]), np.array([0.3, -0.2])
    xt, yt = np.hstack((d["xt"], [2.0, 5.0])), np.hstack((d["yt"], [0.1, -0.7]))
    al = np.hstack((d["alpha"][:300], [0, 0], d["alpha"][300:], [0, 0]))
    a, b = R.sums("A", d["hyp"], d["xt"], d["yt"], d["alpha"], q, P), R.sums("A", d["hyp"], xt, yt, al, q, P)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- the preconditions of every GPU case, on the reference's own trajectory

@pytest.mark.parametrize("c", R.CASES + R.PADDING, ids=repr)
def test_case_preconditions(c):
    d = R.problem(c.id)
    o = R.iterate(d, c.mode, c.nm, d["Q0"], d["P0"])
    alive = ~np.isnan(o["p"])
    assert alive[0].all()
    # slope <= 0.5 at every visited point: what the implicit step's tolerance assumes
    assert np.nanmax(o["slope"]) <= 0.5, np.nanmax(o["slope"])
    # no root within 1e-6 of 0: LOSS_NEGP is never ambiguous
    roots = o["root"][alive[:-1]]
    assert not np.isnan(roots).any() and np.abs(roots).min() > 1e-6
    # no test of the stopping rule within a factor 4 of its threshold: the device makes the reference's number of rows calls
    assert R.is_clear(o).all()
    assert np.array_equal(o["calls"], d["calls"])
    if not c.mode & R.EXPLICIT:
        assert (o["calls"][alive[:-1]] >= 3).all() and o["calls"].max() <= 12
    if c.mode & R.LOSS_NEGP:
        first_lost = np.where(alive.all(axis=0), c.nm, np.argmin(alive, axis=0))
        assert (first_lost[first_lost < c.nm] > 1).any(), "no orbit is lost after step 1"
        assert len(set(first_lost[first_lost < c.nm])) >= 2, "the orbits are all lost at the same step"
        assert 2 * alive[-1].sum() >= c.ntest
        # MINPACK (what the GPU case decides a loss with) finds the secant's roots
        for i in range(c.nm - 1):
            for k in np.flatnonzero(alive[i]):
                assert abs(R.root_minpack(d, o["q"][i, k], o["p"][i, k]) - o["root"][i, k]) <= 1e-11
    else:
        assert alive.all()
    if c.mode & R.WRAP_P:
        assert (np.abs(o["p"][1:] - o["Praw"]) > 1.0).sum() >= 5, "P mod 2 pi never wraps"
    if c.kind == "wrapp":
        assert (d["P0"] < 0).sum() >= c.ntest // 4


def _rounds(n, me, S):
    """rounds_of in applymap_kernel: rounds of 256 points member `me` of S sums"""
    return (n - me * MAP_TT + S * MAP_TT - 1) // (S * MAP_TT) if n > me * MAP_TT else 0


def _owned(n, me, S):
    return sum(max(0, min(MAP_TT, n - (me + i * S) * MAP_TT)) for i in range(_rounds(n, me, S)))


def _staged(c, me):
    return _rounds(c.n0, me, c.S) <= MAP_STAGE and _rounds(c.n0p, me, c.S) <= MAP_STAGE


def test_each_geometry_reaches_what_it_is_there_for():
    g = {c.id: c for c in R.CASES}
    for c in R.CASES + R.PADDING:
        assert c.S == max(1, min(512 // c.ntest, -(-c.n0 // MAP_TT), 16))                      # applymap_team at 256 CUs
        assert sum(_owned(c.n0, me, c.S) for me in range(c.S)) == c.n0
    c = g["s1-memory"]
    assert _rounds(c.n0, 0, 1) == 6 and not _staged(c, 0)
    c = g["s2-ragged"]
    assert _rounds(c.n0, 0, 2) == 2 and _owned(c.n0, 0, 2) == 257 and _rounds(c.n0, 1, 2) == 1
    c = g["s2-mixed"]
    assert [_rounds(c.n0, me, 2) for me in (0, 1)] == [6, 5] and [_staged(c, me) for me in (0, 1)] == [False, True]
    c = g["s2-memory"]
    assert [_staged(c, me) for me in (0, 1)] == [False, False]
    c = g["s3"]
    assert _owned(c.n0, 2, 3) == 188 and all(_staged(c, me) for me in range(3))
    c = g["s13-config05"]
    assert c.S * c.ntest == 481 and 16384 // 4 == c.n0
    c = g["s16-one"]
    assert _owned(c.n0, 15, 16) == 1 and all(_staged(c, me) for me in range(16))
    c = g["s16-memory"]
    assert [_staged(c, me) for me in range(16)] == [False] + [True] * 15
    assert [_rounds(c.n0p, me, 16) for me in range(16)] == [1] + [0] * 15
    c = g["guess-short"]
    assert [_rounds(c.n0p, me, 6) for me in range(6)] == [1, 1, 0, 0, 0, 0]
    c = g["guess-one"]
    assert [_owned(c.n0p, me, 6) for me in range(6)] == [1, 0, 0, 0, 0, 0]
    c = g["guess-long"]
    assert [_rounds(c.n0, me, 2) for me in (0, 1)] == [1, 1] and [_rounds(c.n0p, me, 2) for me in (0, 1)] == [6, 6]
    assert not _staged(c, 0) and not _staged(c, 1)


# ---- co-residency: the members of a team wait for each other, so all 2 * CUs workgroups applymap_team hands out must be
# resident at once -- two workgroups of applymap_kernel per CU

LDS_PER_CU = 163840                      # bytes of LDS of a gfx950 compute unit


def resource_remarks():
    """map.hip compiled alone with the Makefile's compiler and flags and -Rpass-analysis=kernel-resource-usage
    -> (the remarks as text, {kernel name: {field: value}})"""
    mk = open(os.path.join(ROOT, "sympgpr_amd", "csrc", "Makefile")).read()
    var = {k: v.strip() for k, v in re.findall(r"^(HIPCC|ARCH|HIPFLAGS)\s*\??=\s*(.*)$", mk, flags=re.M)}
    hipcc = os.environ.get("HIPCC", var["HIPCC"])
    if shutil.which(hipcc) is None:
        pytest.fail("%s not found: the co-residency of the map's teams cannot be checked without the compiler" % hipcc)
    flags = var["HIPFLAGS"].replace("$(ARCH)", os.environ.get("ARCH", var["ARCH"])).replace("$(EXTRA)", "").split()
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", "map.hip", "-o", os.path.join(td, "map.o")],
                           cwd=os.path.join(ROOT, "sympgpr_amd", "csrc"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = kernels.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    text = "\n".join(l for l in r.stderr.splitlines() if "kernel-resource-usage" in l)
    return text, kernels


def test_two_workgroups_of_the_team_kernel_fit_one_cu():
    _, kernels = resource_remarks()
    # _ZN4sgpr...15applymap_kernelILi<family>ELi256EEEvNS0_7MapArgsE
    team = {int(m.group(1)): v for k, v in kernels.items() for m in [re.search(r"15applymap_kernelILi(\d+)ELi%d" % MAP_TT, k)] if m}
    assert sorted(team) == [0, 1, 2, 3, 4], "instances of applymap_kernel<F, 256> found: %s" % sorted(team)      # A - D and USER
    for fam, v in sorted(team.items()):
        lds, occ, scratch = int(v["LDS Size [bytes/block]"]), int(v["Occupancy [waves/SIMD]"]), int(v["ScratchSize [bytes/lane]"])
        print("applymap_kernel<%d, %d>: LDS %d B, %s VGPRs, scratch %d, %d waves/SIMD" % (fam, MAP_TT, lds, v["VGPRs"], scratch, occ))
        assert scratch == 0, "family %d: the team kernel spills to scratch" % fam
        # a 256-thread workgroup is one wave on each of the CU's four SIMDs: two workgroups need two waves per SIMD
        assert occ >= 2, "family %d: %d wave per SIMD -- a second workgroup does not fit the CU's registers" % (fam, occ)
        assert 2 * lds <= LDS_PER_CU, ("family %d: two workgroups need %d B of the CU's %d B of LDS: applymap_team's 2 * CUs "
                                       "slots are not all resident and teams would wait for members that never start" % (fam, 2 * lds, LDS_PER_CU))
