"""The Strassen front end of the fp64 NT product on the device (sympgpr_amd/csrc/strassen.hip), with the threshold tunable
`gemm_strassen_min` lowered so that orders of a few thousand qualify.  With the built-in threshold (half-sizes >= 8192) NO
other GPU test of this suite reaches a qualifying product: they cover the classical path, this file covers the new one.

Every device step is a child process (tools/strassen_check.py) under its own time limit: the tunables are read once per
process, and a step that hangs ends alone.  Nothing here provokes a fault; the forced scratch failure is a host-side branch.

Bound of (a): the front end is compared with the classical kernel on the same operands,
    max|C_strassen - C_classical| <= 3 k u max|A| max|B| c,     u = 2^-53,   c = (4 k + 25) / 3 + 2 nslab.
Higham (Accuracy and Stability of Numerical Algorithms, 2nd ed., 23.2.2) bounds one level of Strassen over a classical base of
inner dimension k / 2 by (12 ((k/2)^2 + 5 k/2) - 5 k) u max|A| max|B| = (3 k^2 + 25 k) u max|A| max|B| = 3 k u max|A| max|B|
(k + 25/3); the classical result it is compared with carries its own k^2 u max|A| max|B| (+ k/3 in c); and each of the nslab
k slabs adds its result to C once more than a single pass would: <= u (|C0| + k max|A| max|B|) each, covered by 2 nslab in c
for |C0| <= 1 <= k max|A| max|B|.  A k chunk inside a product changes nothing in that count (the partial sums of one
element are still added in k order).  Measured differences: 1.2e-13 ... 4.2e-13 at k = 1024 ... 2560 (profiles/strassen/test_gpu_strassen.txt), against bounds of 5e-10 ... 3e-9."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def run_check(mode, out, env_extra, timeout=300):
    env = dict(os.environ)
    for k in ("SGPR_GEMM_STRASSEN", "SGPR_GEMM_KMAX", "SGPR_LA_MAX", "SGPR_POTRF"):
        env.pop(k, None)
    env.update(env_extra)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tools", "strassen_check.py"), mode, str(out)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, timeout=timeout, capture_output=True, text=True)
    assert r.returncode == 0, (mode, r.returncode, r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.parametrize("kslab,kmax,shapes", [
    # half-sizes >= 512 (k: 256) qualify.  (m, n, k, lower); the last shape of each set does not qualify
    (16384, 8192, [(2048, 2048, 1024, 0), (4096, 2048, 2048, 0), (2048, 3072, 1536, 0), (4096, 4096, 1024, 1), (1280, 2048, 1024, 0)]),
    # k in slabs of at most 1024 (k = 2560: 864 + 864 + 832), every product cut into k chunks of at most 256
    (1024, 256, [(2048, 2048, 2560, 0), (2048, 1024, 2048, 0), (4096, 4096, 2048, 1), (2048, 2048, 384, 0)]),
])
def test_front_end_against_the_classical_kernel(tmp_path, kslab, kmax, shapes):
    out = tmp_path / "front.json"
    run_check("front", out, {"STRASSEN_MIN": "512", "STRASSEN_KSLAB": str(kslab), "SGPR_GEMM_KMAX": str(kmax),
                             "STRASSEN_SHAPES": ",".join("x".join(str(v) for v in s) for s in shapes)})
    res = json.load(open(out))
    assert len(res) == len(shapes)
    for r, s in zip(res, shapes):
        m, n, k, lower = s
        print("front end %s kslab %d kmax %d: max diff %.3e (classical vs numpy %.3e, strassen vs numpy %.3e) bitwise %s"
              % (s, kslab, kmax, r["max_diff"], r["classical_vs_numpy"], r["strassen_vs_numpy"], r["bitwise"]))
        assert r["operands_untouched"]
        if s is shapes[-1]:
            assert r["bitwise"], "a product that does not qualify must be the classical launch, bit for bit"
            continue
        nslab = -(-k // kslab)
        c = (4.0 * k + 25.0) / 3.0 + 2.0 * nslab
        assert r["max_diff"] <= 3.0 * k * U * r["max_a"] * r["max_b"] * c
        assert not r["bitwise"], "the qualifying product was not taken through the seven products"
        assert r["strassen_vs_numpy"] <= 3.0 * k * U * r["max_a"] * r["max_b"] * c


def test_two_destination_epilogue_against_two_launches(tmp_path):
    out = tmp_path / "two.json"
    run_check("two", out, {})
    for r in json.load(open(out)):
        print("two destinations %dx%dx%d alpha2 %g: first bitwise %s, second bitwise %s (max diff %.3e)"
              % (r["m"], r["n"], r["k"], r["alpha2"], r["first_bitwise"], r["second_bitwise"], r["second_max_diff"]))
        assert r["first_bitwise"]                 # C = beta C + alpha P: the same expression on the same accumulators
        if abs(r["alpha2"]) == 1.0:
            assert r["second_bitwise"]            # alpha2 P is exact: one rounding either way
        else:
            # fma(alpha2, P, C2) against fl(alpha2 P) + C2: one rounding of alpha2 P apart, plus the final one
            assert r["second_max_diff"] <= 2.0 * U * r["second_max"]


def test_factor_and_solve_through_the_recursive_driver(tmp_path):
    """order 4096 with la_max = 1024: potrf_rec splits twice, its panel solves and SYRKs take the front end (half-sizes >= 256);
    against the same run with SGPR_GEMM_STRASSEN=0, and with the scratch allocation reported as failed"""
    tune = {"STRASSEN_MIN": "256", "STRASSEN_LA_MAX": "1024"}
    run_check("potrf", tmp_path / "on.npz", tune)
    run_check("potrf", tmp_path / "off.npz", dict(tune, SGPR_GEMM_STRASSEN="0"))
    run_check("potrf", tmp_path / "noscratch.npz", dict(tune, STRASSEN_NOSCRATCH="1"))
    on, off, ns = (np.load(tmp_path / f) for f in ("on.npz", "off.npz", "noscratch.npz"))
    A, z = off["A"], off["z"]
    n = A.shape[0]

    def resid(d):
        return float(np.linalg.norm(A @ d["x"] - z) / np.linalg.norm(z))

    def fact(d):
        return float(np.linalg.norm(d["L"] @ d["L"].T - A) / np.linalg.norm(A))
    dx = float(np.linalg.norm(on["x"] - off["x"]) / np.linalg.norm(off["x"]))
    print("order %d: |x_on - x_off| / |x_off| = %.3e; residual on %.3e off %.3e; |L L^T - A| / |A| on %.3e off %.3e"
          % (n, dx, resid(on), resid(off), fact(on), fact(off)))
    assert not np.array_equal(on["L"], off["L"]), "the recursive driver did not reach the front end"
    # one level: the constant of the error bound grows by at most 3 (the accuracy condition of the full-size step)
    assert resid(on) <= 3.0 * resid(off)
    assert fact(on) <= 3.0 * fact(off)
    # cond(A) ~ 10 here: the two solutions agree to a small multiple of cond * n * u
    assert dx <= 100.0 * n * U
    # (d) no scratch: every product runs classically and the factor is the classical one, bit for bit
    assert np.array_equal(ns["L"].view(np.uint64), off["L"].view(np.uint64))
    assert np.array_equal(ns["x"].view(np.uint64), off["x"].view(np.uint64))
