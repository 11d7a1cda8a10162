"""The recursive factorisation with Strassen thresholds of its own (sympgpr_amd/csrc/chol.hip: potrf_rec / trsm_rec give every
product the thresholds strassen_rec_cfg chooses for it), with the recursion's tunables and la_max scaled down by 32 so that an
order of a few thousand runs the whole path: recursion -> per-call thresholds -> short outer k slab -> four-destination launch ->
lower update split around its squares.  At order 4096 (la_max 1024) trsm_rec's 2048 x 1024 x 1024 takes both levels with the long
outer slab, its 2048 x 512 x 512 products both levels with the short one (quarter products 512 x 128 x 128 with four destinations),
the lower update of order 2048 splits twice.  At 4096 + 384 = 35 leaves the halves are 2304 and 2176: products with m = 2176 are no
multiple of the tiles the front end needs and fall through to classical launches beside the ones that qualify.

Every device step is a child process (tools/strassen_rec_check.py) under its own time limit: the library's tunables are read once
per process, and a step that hangs ends alone.  Nothing here provokes a fault; the forced scratch failure is a host-side branch.

Bound: the two-level norm-wise condition of tests/test_gpu_strassen2.py -- each Strassen level multiplies the constant of the
product's error bound by 3 (Higham 23.2.2), so a factorisation through two levels is held to 9 x the residual and 9 x
|L L^T - A| / |A| of a classical factorisation of the same matrix; the classical factorisation here is SciPy's (LAPACK dpotrf).
Measured: profiles/strassen_rec/test_gpu_strassen_rec.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
# the recursion's own values, scaled by 1 / 32 (shipped: 4096 / 8192, slabs 16384 / 32768 / 16384)
REC = {"rec_strassen_min_gemm": 128, "rec_strassen_min_syrk": 128, "rec_strassen2_min_gemm": 256, "rec_strassen2_min_syrk": 256,
       "rec_strassen_kslab": 512, "rec_strassen2_kslab": 1024, "rec_strassen2_kslab_short": 512, "la_max": 1024}
# the library's values scaled the same way (8192 / 16384, slabs 16384 / 32768), and the recursion's set to exactly those
LIB = {"gemm_strassen_min": 256, "gemm_strassen_kslab": 512, "gemm_strassen2_min": 512, "gemm_strassen2_kslab": 1024, "la_max": 1024}
REC_AS_LIB = dict(LIB, rec_strassen_min_gemm=256, rec_strassen_min_syrk=256, rec_strassen2_min_gemm=512, rec_strassen2_min_syrk=512,
                  rec_strassen_kslab=512, rec_strassen2_kslab=1024, rec_strassen2_kslab_short=0)
_runs = {}


def run(tmp_path_factory, name, n, tune, strassen=None):
    """factor + solve in a child process; one run per configuration, shared by the tests"""
    if name not in _runs:
        out = tmp_path_factory.mktemp("rec") / (name + ".npz")
        env = dict(os.environ)
        for k in ("SGPR_GEMM_STRASSEN", "SGPR_GEMM_KMAX", "SGPR_LA_MAX", "SGPR_POTRF"):
            env.pop(k, None)
        env.update({"REC_N": str(n), "REC_TUNE": ",".join("%s=%d" % kv for kv in tune.items())})
        if strassen is not None:
            env["SGPR_GEMM_STRASSEN"] = strassen
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tools", "strassen_rec_check.py"), str(out)]
        r = subprocess.run(cmd, env=env, cwd=ROOT, timeout=300, capture_output=True, text=True)
        assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        _runs[name] = np.load(out)
    return _runs[name]


_refs = {}


def reference(n):
    """the matrix, the right-hand side and the two figures of SciPy's factor of it"""
    if n not in _refs:
        import scipy.linalg as sl
        import strassen_rec_check as chk
        A, z = chk.matrix(n)
        Ls = sl.cholesky(A, lower=True)
        xs = sl.cho_solve((Ls, True), z)
        _refs[n] = (A, z, figures(A, z, Ls, xs))
    return _refs[n]


def figures(A, z, L, x):
    return float(np.linalg.norm(L @ L.T - A) / np.linalg.norm(A)), float(np.linalg.norm(A @ x - z) / np.linalg.norm(z))


def held_to_scipy(name, n, d):
    A, z, (fact_s, res_s) = reference(n)
    fact, res = figures(A, z, d["L"], d["x"])
    print("%s, order %d: |L L^T - A| / |A| = %.3e (SciPy %.3e), residual %.3e (SciPy %.3e)" % (name, n, fact, fact_s, res, res_s))
    assert fact <= 9.0 * fact_s and res <= 9.0 * res_s


@pytest.mark.parametrize("n", [4096, 4096 + 384])
def test_factor_and_solve_with_the_recursions_thresholds(tmp_path_factory, n):
    d = run(tmp_path_factory, "rec%d" % n, n, REC)
    held_to_scipy("recursion's thresholds", n, d)
    if n == 4096:
        # the path was taken: the library's thresholds at the same scale give another factor
        lib = run(tmp_path_factory, "aslib", 4096, REC_AS_LIB)
        assert not np.array_equal(d["L"], lib["L"]), "the recursion's thresholds changed nothing"


def test_strassen_2_is_the_tree_before_bit_for_bit(tmp_path_factory):
    """SGPR_GEMM_STRASSEN=2 (the recursion's tunables are not read) against the recursion's tunables set to the library's values"""
    two = run(tmp_path_factory, "env2", 4096, dict(LIB, rec_strassen_min_gemm=128, rec_strassen2_kslab_short=512), strassen="2")
    lib = run(tmp_path_factory, "aslib", 4096, REC_AS_LIB)
    assert np.array_equal(two["L"].view(np.uint64), lib["L"].view(np.uint64))
    assert np.array_equal(two["x"].view(np.uint64), lib["x"].view(np.uint64))
    held_to_scipy("SGPR_GEMM_STRASSEN=2", 4096, two)


def test_forced_scratch_failure_still_factors(tmp_path_factory):
    d = run(tmp_path_factory, "noscratch", 4096, dict(REC, gemm_strassen_noscratch=1))
    held_to_scipy("no scratch", 4096, d)
    outer = run(tmp_path_factory, "noouter", 4096, dict(REC, gemm_strassen2_noscratch=1))
    held_to_scipy("no scratch for the outer pair", 4096, outer)
    assert not np.array_equal(outer["L"], d["L"]), "one level must still apply without the outer pair"
