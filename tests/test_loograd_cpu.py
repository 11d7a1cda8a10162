"""CPU checks of the gradient of the leave-one-point-out objectives (sgpr_fit_loo_grad, SympFit.loo_grad, func.loo_chol_grad).

(a) tests/ref_loograd.py's restatement of the formulas against central differences of the DEFINITION, ref_loo.loo_by_deletion
    (every point's rows and columns deleted, a refit on the rest), on the project's own kernels: relative step 1e-5, agreement
    1e-6 relative to max(|g_k|, 1e-3 max|g|), the scaling of test_gpu_nll_grad_full._fd_check.
(b) the restatement in float64 against the same formulas at 40 digits (mpmath) on the smallest pair fixture: the ratio
    err / (cond eps S) must stay <= 10, one tenth of the device tolerance 100 cond eps S of tests/test_gpu_loo_grad.py, so
    that the reference's own error cannot decide a device comparison.  SGPR_RECORD=1 writes the ratios to
    profiles/loograd/reference_margin.txt.
(c) the boundary: the symbol declared, bound and exported; argument errors answered before any device is touched."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ref_loo as R
from tests import ref_loograd as G
from tests import c_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FD_CASES = [("A", 1, 14), ("D", 1, 14), ("A", "reg", 20), ("A", 2, 10)]


def _objective(oracle, fam, kind, p, objective):
    build = G.builder(oracle, fam, kind, p["X"])
    n = p["N"] * p["D"]

    def f(theta):
        Ky = build(theta[:-1]) + abs(theta[-1]) * np.eye(n)
        return R.loo_by_deletion(0.5 * (Ky + Ky.T), p["z"], p["N"], p["D"])[objective]
    return f


@pytest.mark.parametrize("objective", ["loo", "press"])
@pytest.mark.parametrize("fam,kind,N", FD_CASES)
def test_formulas_against_differences_of_the_definition(oracle, fam, kind, N, objective):
    p = R.problem(oracle, fam, kind, N, 700 + N)
    ref = G.reference(oracle, fam, kind, p, objective)
    f = _objective(oracle, fam, kind, p, objective)
    theta = np.append(p["hyp"], p["s2"])
    assert f(theta) == pytest.approx(ref["value"], rel=R.tolerance(p["cond"]))
    g, gscale = ref["g"], np.abs(ref["g"]).max()
    for k in range(len(theta)):
        h = 1e-5 * abs(theta[k])
        tp, tm = theta.copy(), theta.copy()
        tp[k] += h
        tm[k] -= h
        fd = (f(tp) - f(tm)) / (2 * h)
        rel = abs(fd - g[k]) / max(abs(g[k]), 1e-3 * gscale)
        print("%s %s N=%d %s: component %d  formula %.12g  fd %.12g  rel %.3g" % (fam, kind, N, objective, k, g[k], fd, rel))
        assert rel <= 1e-6, (fam, kind, N, objective, k, g[k], fd)


def test_negative_noise_flips_the_last_component_only(oracle):
    p = R.problem(oracle, "A", 1, 14, 714)
    pos = G.reference(oracle, "A", 1, p, "loo")
    neg = G.reference(oracle, "A", 1, p, "loo", s2_sign=-1.0)
    assert np.array_equal(pos["g"][:-1], neg["g"][:-1]) and neg["g"][-1] == -pos["g"][-1]
    f = _objective(oracle, "A", 1, p, "loo")
    theta = np.append(p["hyp"], -p["s2"])
    h = 1e-5 * p["s2"]
    tp, tm = theta.copy(), theta.copy()
    tp[-1] += h
    tm[-1] -= h
    fd = (f(tp) - f(tm)) / (2 * h)
    assert abs(fd - neg["g"][-1]) <= 1e-6 * max(abs(neg["g"][-1]), 1e-3 * np.abs(neg["g"]).max())


def test_float64_restatement_against_40_digits(oracle):
    import mpmath as mp
    fam, kind, N = "A", 1, 14
    p = R.problem(oracle, fam, kind, N, 700 + N)
    dKs, _ = G.dKy(oracle, fam, kind, p)
    n = p["N"] * p["D"]
    lines, worst = [], 0.0
    for objective in ("loo", "press"):
        W64, _ = G.weights(p["Ky"], p["z"], N, p["D"], objective)
        g64, S = G.contract(W64, dKs, 1.0)
        _, Wmp = G.weights_mp(p["Ky"], p["z"], N, p["D"], objective)
        with mp.workdps(40):
            gmp = [0.5 * mp.fsum(Wmp[j, k] * mp.mpf(float(dK[j, k])) for j in range(n) for k in range(n)) for dK in dKs]
            gmp.append(0.5 * mp.fsum(Wmp[j, j] for j in range(n)))
            err = np.array([float(abs(mp.mpf(float(a)) - b)) for a, b in zip(g64, gmp)])
        ratio = err / (p["cond"] * G.EPS * S)
        worst = max(worst, ratio.max())
        line = "pairs A N=%d %-5s cond %.3g  err / (cond eps S) per component: %s" % (N, objective, p["cond"],
                                                                                       " ".join("%.3g" % v for v in ratio))
        print(line)
        lines.append(line)
    if os.environ.get("SGPR_RECORD") == "1":
        os.makedirs(os.path.join(ROOT, "profiles", "loograd"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "loograd", "reference_margin.txt"), "w") as fh:
            fh.write("tests/test_loograd_cpu.py::test_float64_restatement_against_40_digits (SGPR_RECORD=1)\n"
                     "the float64 restatement of tests/ref_loograd.py against the same formulas at 40 digits; bound 10\n")
            fh.write("\n".join(lines) + "\nworst %.3g\n" % worst)
    assert worst <= 10.0, worst


# ---------------------------------------------------------------------------------------------------------- the boundary

def _lib():
    from sympgpr_amd import _lib as L
    return L, L.load_library()


def test_symbol_in_header_dynamic_table_and_signatures():
    L, lib = _lib()
    name = "sgpr_fit_loo_grad"
    c_header.assert_bound_as_declared(name, 5)
    nm = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT %s$" % name, nm, re.M)
    assert lib.sgpr_abi_version() == 5
    hdr = open(c_header.HEADER).read()
    assert re.search(r"enum\s*\{\s*SGPR_LOO_LPD\s*=\s*0\s*,\s*SGPR_LOO_PRESS\s*=\s*1\s*\}", hdr)
    assert (L.LOO_LPD, L.LOO_PRESS) == (0, 1)
    assert re.search(r"needs solved:.*?loo_grad", hdr, re.S), "no row in the header's state table"


def test_handle_entry_rejects_a_null_handle_and_null_outputs():
    L, lib = _lib()
    v, g = np.zeros(1), np.zeros(4)
    assert lib.sgpr_fit_loo_grad(None, 0, L.dptr(v), L.dptr(g), 4) == L.E_ARG
    assert b"fit_loo_grad" in lib.sgpr_last_error()


def test_python_argument_errors_and_calls_without_a_device():
    import sympgpr_amd
    from sympgpr_amd import fit, func
    x = np.linspace(0.1, 3.0, 8)
    xx, hyp = np.concatenate([x, x[::-1]]), np.array([1.0, 1.0, 1.0, 1e-3])
    with pytest.raises(ValueError):
        func.loo_chol_grad(hyp, xx, np.ones(16), 16, objective="nll")
    with pytest.raises(ValueError):
        func.loo_chol_grad(hyp, xx, np.ones(16), 0)
    with pytest.raises(ValueError):
        func.loo_chol_grad(hyp, np.zeros(8), np.zeros(8), 12)            # x holds four points only
    with pytest.raises(ValueError):
        func.loo_chol_grad(hyp, xx, np.ones(5), 8, reg=True)             # too few targets
    assert callable(fit.SympFit.loo_grad)
    calls = [lambda: func.loo_chol_grad(hyp, xx, np.ones(16), 16),
             lambda: func.loo_chol_grad(hyp, xx, np.ones(8), 8, reg=True, objective="press")]
    for call in calls:
        if sympgpr_amd.device_count() > 0:
            value, grad = call()                     # with a device the same calls go through
            assert np.isfinite(value) and grad.shape == (4,)
        else:
            with pytest.raises(sympgpr_amd.NoDeviceError):
                call()
