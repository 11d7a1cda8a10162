"""The fp64 oracle against tests/golden/range.npz (50-digit values over lengths 1e-2 .. 1e2, make_range_golden.py) under
the error model of tests/ref_range.py.  This is where the model's constants are MEASURED: the worst ratio
(|got - v| - F)+ / (eps T) per site is C_REF, the device is held to 4 * C_REF (test_gpu_range.py).  Conditions, not
measurements: every C_REF <= 16, every entry of every combination is compared, and the only entries not compared through
the bound are those whose S is identically 0 (a zero polynomial: family B's mixed block, kxy at coincident points), which
must be exactly 0.  An S that is 0 only because exp underflowed in fp64 is NOT skipped: the entry is held to F alone.

    python tests/test_range_cpu.py        prints the table kept in profiles/range/errors.txt"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_range as R  # noqa: E402

DL_WHICH = {"k_dlx": 4, "k_dly": 5, "kxx_dlx": 6, "kyy_dlx": 7, "kxy_dlx": 8, "kxx_dly": 9, "kyy_dly": 10, "kxy_dly": 11}
WHICH = {"k": 0, "kxx": 1, "kyy": 2, "kxy": 3}


@pytest.fixture(scope="module")
def g():
    return R.load()


class Tally:
    """worst ratio and entry counts per (site, family)"""

    def __init__(self):
        self.worst, self.count, self.zeros = {}, {}, {}

    def add(self, site, fam, got, v, model, extra=None):
        S, T, F, Z = model
        if extra is not None:
            F = F + extra
        r, nb, nz = R.ratio(got, v, S, T, F, Z)
        k = (site, fam)
        self.worst[k] = max(self.worst.get(k, 0.0), r)
        self.count[k] = self.count.get(k, 0) + nb
        self.zeros[k] = self.zeros.get(k, 0) + nz
        return r

    def site_worst(self, site):
        return max([v for (s, _), v in self.worst.items() if s == site], default=0.0)


def measure_pairs(oracle, g, tally):
    for key in g["pair_cases"]:
        fam = str(key)[0]
        c = R.case(g, str(key))
        x, y, x0, y0, hyp = c["x"], c["y"], c["x0"], c["y0"], c["hyp"]
        n, n0 = len(x), len(x0)
        m = R.pair_model(fam, x, y, x0, y0, hyp)
        K = oracle.build_K(fam, x, y, x0, y0, hyp)
        for site, blk in (("kxx", K[:n, :n0]), ("kxy", K[n:, :n0]), ("kxy", K[:n, n0:]), ("kyy", K[n:, n0:])):
            tally.add(site, fam, blk, c[site], m[site])
        tally.add("k", fam, oracle.buildKreg(fam, x, y, x0, y0, hyp), c["k"], m["k"])
        # the scalar functions return the entry without sig: multiplying adds one rounding, eps |v|
        sig, p = hyp[-1], (hyp[2] if fam == "D" else 0.0)
        for site, w in WHICH.items():
            got = np.array([[sig * oracle.scalar(fam, w, x0[j], y0[j], x[i], y[i], hyp[0], hyp[1], p) for j in range(n0)]
                            for i in range(n)])
            tally.add(site, fam, got, c[site], m[site], extra=R.EPS * np.abs(got))
        if fam == "D":
            continue                                         # the oracle restates no length derivative of family D
        dK = oracle.build_dK(fam, x, y, x0, y0, hyp)
        dKr = oracle.build_dKreg(fam, x, y, x0, y0, hyp)
        for w, sfx in enumerate(("_dlx", "_dly")):
            D = dK[w]
            for e, blk in (("kxx", D[:n0, :n]), ("kxy", D[n0:, :n]), ("kxy", D[:n0, n:]), ("kyy", D[n0:, n:])):
                tally.add(e + sfx, fam, blk.T, c[e + sfx], m[e + sfx])
            tally.add("k" + sfx, fam, dKr[w], c["k" + sfx], m["k" + sfx])
        for site, w in DL_WHICH.items():
            got = np.array([[sig * oracle.scalar_dl(fam, w, x0[j], y0[j], x[i], y[i], hyp[0], hyp[1]) for j in range(n0)]
                            for i in range(n)])
            tally.add(site, fam, got, c[site], m[site], extra=R.EPS * np.abs(got))


def measure_nd(oracle, g, tally):
    for key in g["nd_cases"]:
        fam, d = str(key)[3], int(str(key)[4])
        c = R.case(g, str(key))
        S, T, F, Z, diag = R.nd_model(fam, d, c["X"], c["X0"], c["hyp"])
        K = oracle.build_K_nd(fam, c["X"], c["X0"], c["hyp"])
        for site, sel in (("nd_diag", diag), ("nd_off", ~diag)):
            tally.add(site, fam, K[sel], c["K"][sel], (S[sel], T[sel], F[sel], Z[sel]))


def grad_ratios(oracle, g):
    """{case: worst |g - g_exact| / (eps cond sum|W||dK|)} of two fp64 numpy gradients built from the oracle's K, dK"""
    import scipy.linalg
    out = {}
    for key in g["fit_cases"]:
        key = str(key)
        fam, d, reg = key[4], int(key[5]), key[6] == "r"
        if d != 1 or fam not in "AC":
            continue                                         # no dK in the oracle for family D and for d > 1
        c = R.case(g, key)
        x, y, hyp = c["X"][:, 0], c["X"][:, 1], c["hyp"]
        if reg:
            K, dK = oracle.buildKreg(fam, x, y, x, y, hyp), oracle.build_dKreg(fam, x, y, x, y, hyp)
        else:
            K, dK = oracle.build_K(fam, x, y, x, y, hyp), oracle.build_dK(fam, x, y, x, y, hyp)
        N = K.shape[0]
        Ky = K + float(c["sig2n"]) * np.eye(N)
        dKs = [dK[0], dK[1], K / hyp[-1], np.eye(N)]
        worst = 0.0
        for how in ("inv", "chol"):
            if how == "inv":
                Kinv = np.linalg.inv(Ky)
            else:
                Kinv = scipy.linalg.cho_solve(scipy.linalg.cho_factor(Ky, lower=True), np.eye(N))
            alpha = Kinv @ c["z"]
            W = Kinv - np.outer(alpha, alpha)
            got = np.array([0.5 * np.sum(W * d_) for d_ in dKs])
            worst = max(worst, float((np.abs(got - c["grad"]) / (R.EPS * float(c["cond"]) * c["absum"])).max()))
        out[key] = worst
    return out


@pytest.fixture(scope="module")
def tally(oracle, g):
    t = Tally()
    measure_pairs(oracle, g, t)
    measure_nd(oracle, g, t)
    return t


def test_every_entry_is_compared(g, tally):
    """no case left out: per family and site, bound-compared + exact-zero entries == every entry of the fixture"""
    for fam in "ABCD":
        ncase = sum(1 for k in g["pair_cases"] if str(k)[0] == fam)
        assert ncase == 9
        per = ncase * 12 * 8
        for site in R.ENTRIES + (R.DERIVS if fam != "D" else ()):
            mult = 3 if site.startswith("kxy") else 2   # the matrix builder (kxy fills two blocks) + the scalar function
            assert tally.count[(site, fam)] + tally.zeros[(site, fam)] == mult * per, (site, fam)
    total = sum(g[str(k) + "_K"].size for k in g["nd_cases"])
    got = sum(tally.count[k] + tally.zeros[k] for k in tally.count if k[0].startswith("nd_"))
    assert got == total
    assert len(g["nd_cases"]) == 18


def test_fixture_has_the_edges(g):
    """coincident points, a denormal exp per combination, an exponent below -800, both zeros, |dx| ~ pi"""
    deep = 0
    for key in g["pair_cases"]:
        c = R.case(g, str(key))
        fam = str(key)[0]
        assert c["x"][0] == c["x0"][0] and c["y"][0] == c["y0"][0]
        lx, ly = c["hyp"][0], c["hyp"][1]
        assert abs(abs(c["y"][1] - c["y0"][1]) - ly) <= 2.0 ** -24 and abs(abs(c["y"][2] - c["y0"][2]) - ly) <= 2.0 ** -24
        ay = (c["y"][6] - c["y0"][6]) ** 2 / (2 * ly * ly)
        assert 708 <= ay <= 745 and c["x"][6] == c["x0"][6]
        dx = c["x0"][None, :] - c["x"][:, None]
        dy = c["y0"][None, :] - c["y"][:, None]
        u = dx * dx if fam == "C" else np.sin((c["hyp"][2] if fam == "D" else 0.5) * dx) ** 2
        deep += int(np.sum(u / (2 * lx * lx) + dy * dy / (2 * ly * ly) > 800))
        # the stored kxx at the placed root is far below the size of its two cancelling terms
        # (one grid step moves lx^2 cos 2h by 2^-24 * 2 hs lx^2, against terms of size min(lx^2, 1/4))
        m = R.pair_model(fam, c["x"], c["y"], c["x0"], c["y0"], c["hyp"])
        hs = 1.0 if fam == "C" else (c["hyp"][2] if fam == "D" else 0.5)
        assert abs(c["kxx"][1, 1]) <= 2.0 ** -23 * hs * (lx * lx + 1.0) / min(lx * lx, 0.25) * m["kxx"][0][1, 1]
        assert abs(c["kyy"][1, 1]) <= 1e-5 * m["kyy"][0][1, 1]
    assert deep >= 1


@pytest.mark.parametrize("site", R.SITES)
def test_oracle_within_model(tally, site):
    """C_REF <= 16 and the constant in ref_range.py covers what the oracle does today"""
    worst = tally.site_worst(site)
    print("%-8s oracle worst ratio %.3f  C_REF %.2f" % (site, worst, R.C_REF[site]))
    assert R.C_REF[site] <= R.C_REF_MAX
    assert worst <= R.C_REF[site]
    assert R.C[site] == 4.0 * R.C_REF[site]


def test_gradient_constant(oracle, g):
    r = grad_ratios(oracle, g)
    assert len(r) == 9
    worst = max(r.values())
    print("gradient: oracle-based worst ratio %.3g  C_G_REF %.3g" % (worst, R.C_G_REF))
    assert worst <= R.C_G_REF and R.C_G == min(4.0 * R.C_G_REF, 64.0)


def test_host_cos_fast_is_relative():
    """devmath.h's cos_fast (the cos 2h of the Gram kernels) compiled for the host: within 2 ulp of ITS OWN size next to
    its zeros, which is what lx^2 cos 2h - (sin h cos h)^2 needs at lx = 100 and what 1 - 2 sin^2 h does not give"""
    import subprocess
    import tempfile
    src = r"""
#define SGPR_HOST_MATH_TEST
#include "devmath.h"
#include <cstdio>
#include <random>
int main(){ std::mt19937_64 g(7); std::uniform_real_distribution<double> ue(-12,0), uh(-1e4,1e4); std::uniform_int_distribution<int> uk(-3000,3000);
 double mr=0, ma=0;
 for(int i=0;i<400000;i++){ double x;
  if(i%2){ long double z=(2*uk(g)+1)*1.57079632679489661923132169163975144L; x=(double)z+((i%4==1)?1:-1)*std::pow(10.0,ue(g)); }
  else x=uh(g);
  double c=sgpr::cos_fast(x); long double cl=cosl((long double)x);
  double a=std::fabs((double)(c-cl)), r=a/std::fabs((double)cl); if(r>mr)mr=r; if(a>ma)ma=a; }
 printf("%.3e %.3e\n",mr,ma); }
"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.cpp"), "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.run(["g++", "-O2", "-mfma", "-I", os.path.join(root, "sympgpr_amd", "csrc"), os.path.join(td, "t.cpp"),
                        "-o", exe], check=True)
        mr, ma = map(float, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    print("cos_fast: worst relative %.3e, worst absolute %.3e" % (mr, ma))
    assert mr <= 2.0 ** -51 and ma < 1.5e-16


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from oracle.oracle import Oracle
    o, gg = Oracle(), R.load()
    t = Tally()
    measure_pairs(o, gg, t)
    measure_nd(o, gg, t)
    print("site       fam  oracle_worst  compared  exact_zero")
    for (site, fam) in sorted(t.worst):
        print("%-10s %-3s  %12.4f  %8d  %10d" % (site, fam, t.worst[(site, fam)], t.count[(site, fam)], t.zeros[(site, fam)]))
    print()
    print("site       C_ref(measured)  C_REF  C=4*C_REF")
    for site in R.SITES:
        print("%-10s %15.4f  %5.2f  %9.2f" % (site, t.site_worst(site), R.C_REF[site], R.C[site]))
    print()
    for k, v in grad_ratios(o, gg).items():
        print("gradient %-12s oracle-based ratio %.4g" % (k, v))
    print("C_G_REF %.4g  C_G %.4g" % (R.C_G_REF, R.C_G))


if __name__ == "__main__":
    main()
