"""The top Strassen level of the recursion's largest products on the device (sympgpr_amd/csrc/strassen.hip: strassen_top_gemm),
with everything scaled down by 32 as in tests/test_gpu_strassen_rec.py (library 256 / 512, slabs 512 / 1024; the recursion's own
values 128 / 256, slabs 512 / 1024 / 512; la_max 1024) and the top level at a threshold of 512 with slabs of 2048 / 1024, so that
4096 x 2048 x 2048 takes three levels and an order of 8192 runs the whole path: recursion -> top list -> operand sums, zeroing,
half-size call with its two levels, accumulation on the low-priority stream -> pass-through calls.

Every device step is a child process (tools/strassen_top_check.py) under its own time limit: the library's tunables are read once
per process, and a step that hangs ends alone.  Nothing here provokes a fault; the forced allocation failure is a host-side branch.

Bound of the comparison with the classical kernel on the same operands, the way tests/test_gpu_strassen2.py derives its two-level
bound.  Higham (Accuracy and Stability of Numerical Algorithms, 2nd ed., 23.2.2): Strassen's algorithm over a classical base of
inner dimension k0, k = 2^l k0, has |C - C_hat| <= ((k / k0)^(log2 12) (k0^2 + 5 k0) - 5 k) u max|A| max|B|; three levels,
k0 = k / 8: 1728 (k^2 / 64 + 5 k / 8) - 5 k = 27 k^2 + 1075 k.  The classical result it is compared with carries its own
k^2 u max|A| max|B|.  Each k slab adds its result to C once more than a single pass would, at each of the two levels below: 2
roundings per slab and level, each <= u (max|C0| + k max|A| max|B|), with the finest slab (1024) counted over the whole of k.  The
top level forms every M_i in a temporary and adds it to C in a pass of its own: at most 4 such additions per block and top slab,
each one rounding of a partial sum <= max|C0| + 4 * 2 k max|A| max|B| (an M_i of operand sums is at most (k / 2) * 2 * 2).
    max|C_top - C_classical| <= u max|A| max|B| (28 k^2 + 1075 k) + 4 nslab u (max|C0| + k max|A| max|B|)
                                + 4 nslab3 u (max|C0| + 8 k max|A| max|B|),   u = 2^-53.
Measured differences and the factorisation's ratios: profiles/strassen_top/test_gpu_strassen_top.txt.

The factorisation is held to 27 x SciPy's residual and |L L^T - A| / |A| on the same matrix: 3 per level (Higham 23.2.2), the
factor the two-level tests use as 9 x."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
U = 2.0 ** -53
LIB = {"gemm_strassen_min": 256, "gemm_strassen_kslab": 512, "gemm_strassen2_min": 512, "gemm_strassen2_kslab": 1024, "la_max": 1024}
REC = {"rec_strassen_min_gemm": 128, "rec_strassen_min_syrk": 128, "rec_strassen2_min_gemm": 256, "rec_strassen2_min_syrk": 256,
       "rec_strassen_kslab": 512, "rec_strassen2_kslab": 1024, "rec_strassen2_kslab_short": 512}
TOP = dict(LIB, **REC, rec_strassen3_min=512, rec_strassen3_kslab=2048, rec_strassen3_kslab_short=1024)
OFF = dict(TOP, rec_strassen3_min=0)
RAGGED = 8192 + 128     # halves 4224 / 4096: 4096 x 2048 x 2176 and the 2048 square of the lower update (k = 4224) take the top level
_runs = {}


def run(tmp_path_factory, name, mode, tune, strassen=None, **env_extra):
    """one child process per configuration, shared by the tests"""
    if name not in _runs:
        out = tmp_path_factory.mktemp("top") / (name + (".json" if mode == "front" else ".npz"))
        env = dict(os.environ)
        for k in ("SGPR_GEMM_STRASSEN", "SGPR_GEMM_KMAX", "SGPR_LA_MAX", "SGPR_POTRF"):
            env.pop(k, None)
        env.update({"REC_TUNE": ",".join("%s=%d" % kv for kv in tune.items())})
        env.update({k: str(v) for k, v in env_extra.items()})
        if strassen is not None:
            env["SGPR_GEMM_STRASSEN"] = strassen
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tools", "strassen_top_check.py"), mode, str(out)]
        r = subprocess.run(cmd, env=env, cwd=ROOT, timeout=300, capture_output=True, text=True)
        assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        _runs[name] = json.load(open(out)) if mode == "front" else np.load(out)
    return _runs[name]


def front(tmp_path_factory, name, shape, tune, strassen=None):
    return run(tmp_path_factory, name, "front", tune, strassen, TOP_SHAPE=",".join(str(v) for v in shape))


def bound(r, k):
    ab = r["max_a"] * r["max_b"]
    nslab, nslab3 = -(-k // 1024), max(k // 2048, 1)
    return U * ab * (28.0 * k * k + 1075.0 * k) + 4.0 * nslab * U * (r["max_c0"] + k * ab) + 4.0 * nslab3 * U * (r["max_c0"] + 8.0 * k * ab)


@pytest.mark.parametrize("shape", [(4096, 2048, 2048, 0), (4096, 2048, 2560, 0)])
def test_three_levels_against_the_classical_kernel(tmp_path_factory, shape):
    r = front(tmp_path_factory, "on%d" % shape[2], shape, TOP)
    b = bound(r, shape[2])
    print("three levels %s: max diff to classical %.3e (bound %.3e; classical vs numpy %.3e, three levels vs numpy %.3e, two levels vs numpy %.3e)"
          % (shape, r["max_diff"], b, r["classical_vs_numpy"], r["top_vs_numpy"], r["replaced_vs_numpy"]))
    assert r["operands_untouched"]
    assert not r["same_as_replaced_entry"] and not r["same_as_classical"], "the product was not taken through the top level"
    assert r["max_diff"] <= b
    assert r["top_vs_numpy"] <= b


def test_a_lower_update_through_the_top_level(tmp_path_factory):
    r = front(tmp_path_factory, "lower", (4096, 4096, 2048, 1), TOP)
    b = bound(r, 2048)
    print("lower update of order 4096, k = 2048: max diff to classical %.3e (bound %.3e)" % (r["max_diff"], b))
    assert r["operands_untouched"] and r["again_same"]
    assert not r["same_as_replaced_entry"]
    assert r["max_diff"] <= b and r["top_vs_numpy"] <= b


def test_serial_and_overlapped_passes_give_the_same_bits(tmp_path_factory):
    shape = (4096, 2048, 2560, 0)
    runs = {"two buffer sets on the side stream": front(tmp_path_factory, "on2560", shape, TOP),
            "one buffer set on the side stream": front(tmp_path_factory, "one_set", shape, dict(TOP, rec_strassen3_buffers=1)),
            "serial": front(tmp_path_factory, "serial", shape, dict(TOP, rec_strassen3_overlap=0))}
    for name, r in runs.items():
        assert r["again_same"], name + ": a second run gave other bits"
        assert not r["same_as_replaced_entry"], name
    assert len({r["sha"] for r in runs.values()}) == 1, {k: r["sha"] for k, r in runs.items()}


@pytest.mark.parametrize("name,tune,strassen", [("off", OFF, None), ("env0", TOP, "0"), ("env1", TOP, "1"), ("env2", TOP, "2")])
def test_without_the_top_level_the_call_is_the_one_it_replaced(tmp_path_factory, name, tune, strassen):
    """rec_strassen3_min = 0 with SGPR_GEMM_STRASSEN unset, and SGPR_GEMM_STRASSEN = 0 / 1 / 2 with the top level's tunables set:
    the bits of gemm_nt_strassen_rec, the entry the recursion called before"""
    r = front(tmp_path_factory, name, (4096, 2048, 2048, 0), tune, strassen)
    assert r["same_as_replaced_entry"] and r["again_same"]
    assert r["same_as_classical"] == (strassen == "0")
    on = front(tmp_path_factory, "on2048", (4096, 2048, 2048, 0), TOP)
    assert r["sha"] != on["sha"]


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
    print("%s, order %d: |L L^T - A| / |A| = %.3e (SciPy %.3e, ratio %.2f), residual %.3e (SciPy %.3e, ratio %.2f)"
          % (name, n, fact, fact_s, fact / fact_s, res, res_s, res / res_s))
    assert fact <= 27.0 * fact_s and res <= 27.0 * res_s


@pytest.mark.parametrize("n", [8192, RAGGED])
def test_factor_and_solve_through_the_recursion(tmp_path_factory, n):
    import strassen_top_plan as stp
    # the order was chosen on the CPU from the plan probe: a top-level call occurs in its recursion
    stp.set_tunables({k: v for k, v in TOP.items() if k.startswith("rec_")})
    try:
        took = stp.qualifying_calls(n, la_max=1024, floor=2048)
    finally:
        stp.set_tunables(dict(stp.srp.SHIPPED, **stp.SHIPPED))
    h = n - (n // 2 + 127) // 128 * 128
    assert (h, h // 2, n - h - h // 2, 0) in took and (h, h, n - h, 1) in took, took
    d = run(tmp_path_factory, "potrf%d" % n, "potrf", TOP, REC_N=n)
    held_to_scipy("three levels", n, d)
    if n == 8192:
        off = run(tmp_path_factory, "potrf_off8192", "potrf", OFF, REC_N=n)
        assert not np.array_equal(d["L"], off["L"]), "the recursion did not reach the top level"


def test_forced_allocation_failure_gives_the_bits_without_the_level(tmp_path_factory):
    d = run(tmp_path_factory, "noscratch", "potrf", dict(TOP, rec_strassen3_noscratch=1), REC_N=8192)
    off = run(tmp_path_factory, "potrf_off8192", "potrf", OFF, REC_N=8192)
    assert np.array_equal(d["L"].view(np.uint64), off["L"].view(np.uint64))
    assert np.array_equal(d["x"].view(np.uint64), off["x"].view(np.uint64))
