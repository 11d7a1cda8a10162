"""The outer Strassen level of the fp64 NT product on the device (sympgpr_amd/csrc/strassen.hip) and the product with up to four
destinations it is built on, with both thresholds lowered (inner 256, outer 512, outer k slab 1024) so that orders of a few
thousand take two levels.  With the built-in thresholds no other GPU test reaches the outer level.

Every device step is a child process (tools/strassen2_check.py) under its own time limit: the tunables are read once per
process, and a step that hangs ends alone.  Nothing here provokes a fault; the forced scratch failures are host-side branches.

Bound of the two-level comparison with the classical kernel on the same operands.  Higham (Accuracy and Stability of Numerical
Algorithms, 2nd ed., 23.2.2): Strassen's algorithm over a classical base of inner dimension k0, k = 2^l k0, has
|C - C_hat| <= ((k / k0)^(log2 12) (k0^2 + 5 k0) - 5 k) u max|A| max|B|; two levels, k0 = k / 4: 144 (k^2 / 16 + 5 k / 4) - 5 k =
9 k^2 + 175 k.  The classical result it is compared with carries its own k^2 u max|A| max|B|.  Each k slab adds its result to C
once more than a single pass would, at each of the two levels: 2 roundings per slab and level, each <= u (max|C0| + k max|A| max|B|).
    max|C_two - C_classical| <= u max|A| max|B| (10 k^2 + 175 k) + 4 nslab u (max|C0| + k max|A| max|B|),   u = 2^-53,
with nslab = ceil(k / outer slab).  A k chunk inside a product changes nothing in that count.
Measured differences: see profiles/strassen2/test_gpu_strassen2.txt.

The factorisation is held to 9 x the classical run's residual and |L L^T - A| (3 per level, the accuracy condition of the
full-size step applied twice) and to 3 x the one-level run's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
# (SGPR_GEMM_STRASSEN=2 asks for both levels whatever the library's default is)
TUNE = {"STRASSEN_MIN": "256", "STRASSEN2_MIN": "512", "STRASSEN2_KSLAB": "1024", "SGPR_GEMM_STRASSEN": "2"}


def run_check(mode, out, env_extra, timeout=300):
    env = dict(os.environ)
    for k in ("SGPR_GEMM_STRASSEN", "SGPR_GEMM_KMAX", "SGPR_LA_MAX", "SGPR_POTRF", "STRASSEN2_SAVE"):
        env.pop(k, None)
    env.update(env_extra)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tools", "strassen2_check.py"), mode, str(out)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, timeout=timeout, capture_output=True, text=True)
    assert r.returncode == 0, (mode, r.returncode, r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.parametrize("shapes,kmax", [
    ([(256, 128, 32), (768, 384, 160)], None),     # one tile with two k-steps; 3 x 3 tiles, ten k-steps
    ([(512, 256, 192)], 64),
    # (SGPR_GEMM_KMAX below 128 leaves a product in one launch: the case above runs unchunked.)  Three chunks of 128, each of
    # which adds to every destination; and a shape with edge tiles, which takes the register-staged body
    ([(512, 256, 384), (300, 200, 72)], 128),
])
def test_four_destinations_against_separate_launches(tmp_path, shapes, kmax):
    out = tmp_path / "four.json"
    env = {"STRASSEN2_SHAPES": ",".join("x".join(str(v) for v in s) for s in shapes)}
    if kmax:
        env["SGPR_GEMM_KMAX"] = str(kmax)
    run_check("four", out, env)
    res = json.load(open(out))
    assert len(res) == 4 * len(shapes) and sorted({r["count"] for r in res}) == [2, 3, 4]
    for r in res:
        print("destinations %d of %dx%dx%d kmax %s beta %g: %s" % (r["count"], r["m"], r["n"], r["k"], kmax, r["beta"],
              ", ".join("alpha %g %s (max diff %.3e)" % (b["alpha"], "bitwise" if b["bitwise"] else "differs", b["max_diff"]) for b in r["blocks"])))
        assert r["operands_untouched"] and r["outside_untouched"]
        assert r["blocks"][0]["bitwise"]              # C = beta C + alpha P: the same expression on the same accumulators
        for b in r["blocks"]:
            assert b["changed"]
        for b in r["blocks"][1:]:
            if abs(b["alpha"]) == 1.0:
                assert b["bitwise"]                   # alpha_d P is exact: one rounding either way
            else:
                # fma(alpha_d, P, C_d) against fl(alpha_d P) + C_d: one rounding of alpha_d P apart, plus the final one
                assert b["max_diff"] <= 2.0 * U * b["max"]


def bound(r, k, nslab):
    ab = r["max_a"] * r["max_b"]
    return U * ab * (10.0 * k * k + 175.0 * k) + 4.0 * nslab * U * (r["max_c0"] + k * ab)


@pytest.mark.parametrize("kmax,shapes", [
    (8192, [(2048, 2048, 1024, 0), (4096, 2048, 2048, 0), (4096, 4096, 1024, 1)]),
    # k = 2560 = two outer slabs of 1024 and a remainder of 512 through the inner level; every product in k chunks of <= 256
    (256, [(2048, 2048, 2560, 0)]),
])
def test_two_levels_against_the_classical_kernel(tmp_path, kmax, shapes):
    out = tmp_path / "front.json"
    run_check("front", out, dict(TUNE, SGPR_GEMM_KMAX=str(kmax),
                                 STRASSEN2_SHAPES=",".join("x".join(str(v) for v in s) for s in shapes)))
    res = json.load(open(out))
    assert len(res) == len(shapes)
    for r, (m, n, k, lower) in zip(res, shapes):
        b = bound(r, k, -(-k // 1024))
        print("two levels %s kmax %d: max diff %.3e (bound %.3e; classical vs numpy %.3e, two levels vs numpy %.3e)"
              % ((m, n, k, lower), kmax, r["max_diff"], b, r["classical_vs_numpy"], r["strassen_vs_numpy"]))
        assert r["operands_untouched"]
        assert not r["bitwise"], "the product was not taken through the front end"
        assert r["max_diff"] <= b
        assert r["strassen_vs_numpy"] <= b


def test_below_the_outer_slab_is_the_one_level_call_bit_for_bit(tmp_path):
    """1024 x 1024 x 512: k is shorter than one outer slab, so the call takes one level only"""
    env = dict(TUNE, STRASSEN2_SHAPES="1024x1024x512x0", STRASSEN2_SAVE="1")
    run_check("front", tmp_path / "both.json", env)
    run_check("front", tmp_path / "one.json", dict(env, SGPR_GEMM_STRASSEN="1"))
    both, one = (np.load(str(tmp_path / f) + ".1024x1024x512_0.npy") for f in ("both.json", "one.json"))
    r = json.load(open(tmp_path / "both.json"))[0]
    print("1024x1024x512: max diff to classical %.3e, bitwise equal to the one-level run: %s" % (r["max_diff"], np.array_equal(both, one)))
    assert not r["bitwise"], "one level must still apply"
    assert np.array_equal(both.view(np.uint64), one.view(np.uint64))


def test_factor_and_solve_through_the_recursive_driver(tmp_path):
    """order 4096 with la_max = 1024: potrf_rec splits twice; its first panel solve (2048 x 1024 x 1024) and the square of its
    first SYRK (1024 x 1024 x 2048) take both levels"""
    tune = dict(TUNE, STRASSEN_LA_MAX="1024")
    runs = {"two": tune, "one": dict(tune, SGPR_GEMM_STRASSEN="1"), "off": dict(tune, SGPR_GEMM_STRASSEN="0"),
            "noouter": dict(tune, STRASSEN2_NOSCRATCH="1"), "noscratch": dict(tune, STRASSEN_NOSCRATCH="1")}
    d = {}
    for name, env in runs.items():
        run_check("potrf", tmp_path / (name + ".npz"), env)
        d[name] = np.load(tmp_path / (name + ".npz"))
    A, z = d["off"]["A"], d["off"]["z"]

    def resid(x):
        return float(np.linalg.norm(A @ x["x"] - z) / np.linalg.norm(z))

    def fact(x):
        return float(np.linalg.norm(x["L"] @ x["L"].T - A) / np.linalg.norm(A))
    print("order %d: residual two %.3e one %.3e off %.3e; |L L^T - A| / |A| two %.3e one %.3e off %.3e"
          % (A.shape[0], resid(d["two"]), resid(d["one"]), resid(d["off"]), fact(d["two"]), fact(d["one"]), fact(d["off"])))
    assert resid(d["two"]) <= 9.0 * resid(d["off"]) and fact(d["two"]) <= 9.0 * fact(d["off"])
    assert resid(d["two"]) <= 3.0 * resid(d["one"]) and fact(d["two"]) <= 3.0 * fact(d["one"])
    assert not np.array_equal(d["two"]["L"], d["one"]["L"]), "the recursive driver did not reach the outer level"
    for a, b in (("noouter", "one"), ("noscratch", "off")):
        assert np.array_equal(d[a]["L"].view(np.uint64), d[b]["L"].view(np.uint64)), (a, b)
        assert np.array_equal(d[a]["x"].view(np.uint64), d[b]["x"].view(np.uint64)), (a, b)
