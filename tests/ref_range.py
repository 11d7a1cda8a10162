"""The error model of tests/golden/range.npz (make_range_golden.py), in plain numpy: shared by test_range_cpu.py
(the fp64 oracle against the fixture, which MEASURES the constants below) and test_gpu_range.py (the device against
the same fixture and the same bound).

For a stored entry v (the exact value rounded once to fp64) a computed `got` is accepted when

    |got - v| <= C * eps * T + F,      eps = 2^-53,
    T = sum_t S_t (1 + A_t),           F = 4 (1 + M) 2^-1074.

Every entry is a sum of terms  sig * poly * exp(-a) / (lx^kx ly^ky):
  * S_t is the term with every cancelling piece of `poly` replaced by its magnitude (lx^2 |cos 2h| + (sin h cos h)^2
    for kxx, 2 l^4 + 5 l^2 v + v^2 for d kyy / d ly, ...), computed here in fp64 from the inputs; S = sum_t S_t;
  * A_t is the sum of the magnitudes of the exponent's terms as the family writes them: s^2 / 2 lx^2 + dy^2 / 2 ly^2
    (A, C, D), and (0.5 ya^2 + |ya yb| + 0.5 yb^2) / ly^2 for the expanded P exponent of family B.  An fp64 exponent
    carries A_t * eps absolute error, which exp turns into that relative error;
  * where a derivative of family B is written with (ya - yb)^2 expanded, ya^2 + 2 |ya yb| + yb^2 stands in for it.
F covers results and intermediates on the denormal grid: exp(-a) below 2^-1022 is only known to 2^-1074 absolute,
and whatever factors multiply it afterwards multiply that error; M = max(1, sig) max(1, poly) max(1, lx^-kx)
max(1, ly^-ky) bounds their product in any order of evaluation.  With M <= 1 this is the plain 4 * 2^-1074.  In the
normal range F is far below eps * S and changes nothing.

C is measured, not chosen: C_REF[site] is the worst ratio (|got - v| - F)+ / (eps T) of the fp64 ORACLE over every
entry of every combination of the fixture (test_range_cpu.py asserts it is reproduced and <= 16), and
C[site] = 4 * C_REF[site]; the factor 4 allows for FMA contraction and x * (1 / l^2) against x / l^2.  Family D has no
length derivatives in the oracle and shares the constants of A, whose forms it shares."""
import os

import numpy as np

EPS = 2.0 ** -53
TINY = 2.0 ** -1074
HERE = os.path.dirname(os.path.abspath(__file__))
ENTRIES = ("k", "kxx", "kxy", "kyy")
DERIVS = tuple(e + s for s in ("_dlx", "_dly") for e in ENTRIES)
SITES = ENTRIES + DERIVS + ("nd_diag", "nd_off")

# measured by test_range_cpu.py (profiles/range/errors.txt): worst oracle ratio per site, rounded up to one decimal
C_REF = {
    "k": 3.5, "kxx": 3.9, "kxy": 4.5, "kyy": 3.0,
    "k_dlx": 3.7, "kxx_dlx": 4.8, "kxy_dlx": 4.8, "kyy_dlx": 4.1,
    "k_dly": 3.4, "kxx_dly": 5.5, "kxy_dly": 4.9, "kyy_dly": 4.0,
    "nd_diag": 3.3, "nd_off": 4.0,
}
C = {s: 4.0 * v for s, v in C_REF.items()}
C_REF_MAX = 16.0
# NLL gradient: |g - g_exact| <= C_G * eps * cond(Ky) * sum_ij |W_ij| |dK_ij|; C_G_REF is the worst ratio of fp64 numpy
# gradients built from the oracle's K and dK (explicit inverse, and Cholesky solves); margin 4, cap 64
C_G_REF = 1.3
C_G = min(4.0 * C_G_REF, 64.0)


def load():
    return np.load(os.path.join(HERE, "golden", "range.npz"))


def case(g, key):
    n = len(key) + 1
    return {k[n:]: g[k] for k in g.files if k.startswith(key + "_")}


def _term(sig, P, a, A, lx, kx, ly, ky):
    """-> (S_t, T_t, M_t, Z_t) of one term sig * P * exp(-a) / (lx^kx ly^ky); Z_t: the term is zero whatever exp gives"""
    pre = (1.0 / lx ** kx) * (1.0 / ly ** ky)
    with np.errstate(under="ignore"):
        S = sig * P * pre * np.exp(-a)
    M = max(1.0, sig) * np.maximum(1.0, P) * max(1.0, 1.0 / lx ** kx) * max(1.0, 1.0 / ly ** ky)
    return S, S * (1.0 + A), M, (sig * P * pre) == 0


def pair_model(fam, x, y, x0, y0, hyp):
    """{entry: (S, T, F, Z)}, each (n, n0): row point i against column point j, for the 12 entries of a family"""
    hyp = np.asarray(hyp, dtype=np.float64)
    lx, ly, sig = abs(hyp[0]), abs(hyp[1]), abs(hyp[-1])
    x, y, x0, y0 = (np.asarray(v, dtype=np.float64) for v in (x, y, x0, y0))
    dx = x0[None, :] - x[:, None]
    dy = y0[None, :] - y[:, None]
    v = dy * dy
    lx2, ly2 = lx * lx, ly * ly
    if fam == "C":
        hs, u, cd = 1.0, dx * dx, np.ones_like(dx)
        q2, q = dx * dx, np.abs(dx)
    else:
        hs = hyp[2] if fam == "D" else 0.5
        s, c = np.sin(hs * dx), np.cos(hs * dx)
        u, cd = s * s, np.abs(np.cos(2.0 * hs * dx))
        q2, q = (s * c) ** 2, np.abs(s * c)
    pp = hs * hs
    ax, ay = u / (2.0 * lx2), v / (2.0 * ly2)
    ady = np.abs(dy)
    Pxx = pp * (lx2 * cd + q2)
    Pxx_dlx = pp * (2.0 * lx2 * lx2 * cd + lx2 * (3.0 * cd + 2.0) * u + u * q2)
    zero = (np.zeros_like(dx), np.zeros_like(dx), np.ones_like(dx), np.ones(dx.shape, dtype=bool))
    if fam == "B":
        Ay = (0.5 * y0[None, :] ** 2 + np.abs(y0[None, :] * y[:, None]) + 0.5 * y[:, None] ** 2) / ly2
        vexp = y0[None, :] ** 2 + 2.0 * np.abs(y0[None, :] * y[:, None]) + y[:, None] ** 2
        tx = lambda P, kx: _term(sig, P, ax, ax, lx, kx, ly, 0)
        ty = lambda P, ky: _term(sig, P, ay, Ay, lx, 0, ly, ky)
        one = np.ones_like(dx)
        kx_, ky_ = tx(one, 0), ty(one, 0)
        terms = {
            "k": (kx_[0] + ky_[0], kx_[1] + ky_[1], np.maximum(kx_[2], ky_[2]), kx_[3] & ky_[3]),
            "kxx": tx(Pxx, 4), "kyy": ty(ly2 + v, 4), "kxy": zero,
            "k_dlx": tx(u, 3), "k_dly": ty(vexp, 3),
            "kxx_dlx": tx(Pxx_dlx, 7), "kyy_dlx": zero, "kxy_dlx": zero,
            "kxx_dly": zero, "kxy_dly": zero,
            "kyy_dly": ty(2.0 * ly2 * ly2 + ly2 * (vexp + 4.0 * v) + v * vexp, 7),
        }
    else:
        a = ax + ay
        t = lambda P, kx, ky: _term(sig, P, a, a, lx, kx, ly, ky)
        Pxy = hs * ady * q
        terms = {
            "k": t(np.ones_like(dx), 0, 0),
            "kxx": t(Pxx, 4, 0), "kyy": t(ly2 + v, 0, 4), "kxy": t(Pxy, 2, 2),
            "k_dlx": t(u, 3, 0), "k_dly": t(v, 0, 3),
            "kxx_dlx": t(Pxx_dlx, 7, 0), "kyy_dlx": t((ly2 + v) * u, 3, 4), "kxy_dlx": t(Pxy * (u + 2.0 * lx2), 5, 2),
            "kxx_dly": t(Pxx * v, 4, 3), "kyy_dly": t(2.0 * ly2 * ly2 + 5.0 * ly2 * v + v * v, 0, 7),
            "kxy_dly": t(Pxy * (v + 2.0 * ly2), 2, 5),
        }
    return {k: (S, T, 4.0 * (1.0 + M) * TINY, Z) for k, (S, T, M, Z) in terms.items()}


def nd_model(fam, d, X, X0, hyp):
    """(S, T, F, Z, diag) in build_k_nd's layout (2d n x 2d n0): block (a, b) at rows a n, columns b n0; diag marks a == b"""
    X, X0, hyp = (np.asarray(v, dtype=np.float64) for v in (X, X0, hyp))
    D = 2 * d
    n, n0 = X.shape[0], X0.shape[0]
    sig = abs(hyp[-1])
    aa, gn, nhn, il2 = [], [], [], []
    for m in range(D):
        l2 = hyp[m] ** 2
        dx = X0[None, :, m] - X[:, None, m]
        if m < d and fam != "C":
            hs = hyp[D + m] if fam == "D" else 0.5
            s, c = np.sin(hs * dx), np.cos(hs * dx)
            aa.append(s * s / (2.0 * l2))
            gn.append(hs * np.abs(s * c))
            nhn.append(hs * hs * (l2 * np.abs(np.cos(2.0 * hs * dx)) + (s * c) ** 2))
        else:
            aa.append(dx * dx / (2.0 * l2))
            gn.append(np.abs(dx))
            nhn.append(l2 + dx * dx)
        il2.append(1.0 / l2)
    atot = sum(aa)
    S = np.zeros((D * n, D * n0))
    T, M = np.zeros_like(S), np.ones_like(S)
    Z = np.ones(S.shape, dtype=bool)
    diag = np.zeros(S.shape, dtype=bool)
    for a in range(D):
        for b in range(D):
            blk = (slice(a * n, (a + 1) * n), slice(b * n0, (b + 1) * n0))
            diag[blk] = a == b
            if fam == "B" and a != b:
                continue
            P = nhn[a] if a == b else gn[a] * gn[b]
            ex = aa[a] if fam == "B" else atot
            pre = il2[a] * il2[b]
            with np.errstate(under="ignore"):
                s_ = sig * P * pre * np.exp(-ex)
            S[blk], T[blk] = s_, s_ * (1.0 + ex)
            Z[blk] = (sig * P * pre) == 0
            M[blk] = max(1.0, sig) * np.maximum(1.0, P) * max(1.0, il2[a]) * max(1.0, il2[b])
    return S, T, 4.0 * (1.0 + M) * TINY, Z, diag


def ratio(got, v, S, T, F, Z):
    """worst (|got - v| - F)+ / (eps T) over the entries that are not identically zero (Z); where Z, got must be exactly 0.
    An entry whose model term underflows (T == 0) is held to F alone.
    -> (ratio, number of entries compared through the bound, number compared as exact zeros)"""
    got, v = np.asarray(got, dtype=np.float64), np.asarray(v, dtype=np.float64)
    assert got.shape == v.shape == S.shape, (got.shape, v.shape, S.shape)
    assert np.all(np.isfinite(got)), "non-finite entry"
    assert np.all(got[Z] == 0.0) and np.all(v[Z] == 0.0), "an identically zero entry is not 0"
    if Z.all():
        return 0.0, 0, int(Z.sum())
    err = np.maximum(np.abs(got - v)[~Z] - F[~Z], 0.0)
    t = EPS * T[~Z]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / t)
    return float(r.max()), int((~Z).sum()), int(Z.sum())
