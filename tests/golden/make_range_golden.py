#!/usr/bin/env python3
"""tests/golden/range.npz: every kernel-formula site at 50 digits over the optimiser's range of lengths.

Each family's scalar kernel k(xa, ya, xb, yb) is written ONCE below from its mathematical definition; the Hessian
entries, the length derivatives, the d-pair blocks and the NLL gradients all come from sympy.diff of that one
expression, are lambdified to mpmath (50 digits) and rounded ONCE to the nearest fp64.  Nothing here reads
tools/gen_kernels.py, csrc/, the oracle or the reference: the fixture is independent of all of them.

Inputs (all stored in the file):
  * coordinates are multiples of 2^-24, so xa - xb, ya - yb, 0.5 (xa - xb) and p (xa - xb) (p in 0.5, 0.75, 2) are
    exact in fp64 and the rounding of the difference is not charged to the kernels;
  * lengths are nominal * 1.37 (not round): lx = ly in 1e-2 .. 1e2, the corners (1e-2, 1e2), (1e2, 1e-2), two seeded
    log-uniform pairs; sig cycles through 1e-2, 1, 1e2;
  * per combination 12 row points x 8 column points: 5 uniform rows (q in [0, 2 pi), P in [-3, 3]) and 7 rows placed
    relative to a column point (see placed_rows): coincident, dy = +-ly, the zero of kxx, |dx| ~ pi, separations
    l * (2^-10, 0.5, 2, 6, 30) and a pair whose exponent is -726 (a denormal exp);
  * d-pair cases: d = 2, 3 (A, C), d = 2 (B, D), per-coordinate lengths nominal * FACT[m], 6 x 5 points;
  * 8-point fits (the column points of a combination): NLL, cond(Ky) and the exact gradient 1/2 tr(W dK) in every
    hyperparameter, with sum |W_ij| |dK_ij| for the error bound.

Usage:  python tests/golden/make_range_golden.py      (about two minutes; regenerates range.npz byte for byte)"""
import io
import os
import zipfile
from fractions import Fraction

import mpmath as mp
import numpy as np
import sympy as sp

HERE = os.path.dirname(os.path.abspath(__file__))
mp.mp.dps = 50
GRID = 2.0 ** -24
LFAC = 1.37
FACT = (1.37, 0.83, 1.19, 0.71, 1.53, 0.94)
SIGS = (1e-2, 1.0, 1e2)
PVALS = (0.5, 0.75, 2.0)
N_ROW, N_COL = 12, 8
ND_ROW, ND_COL = 6, 5
ENTRIES = ("k", "kxx", "kxy", "kyy")

xa, ya, xb, yb = sp.symbols("xa ya xb yb", real=True)
lx, ly, p, sig = sp.symbols("lx ly p sig", positive=True)


def kernel(fam):
    """the four one-line definitions"""
    se_y = sp.exp(-(ya - yb) ** 2 / (2 * ly ** 2))
    if fam == "A":
        return sp.exp(-sp.sin((xa - xb) / 2) ** 2 / (2 * lx ** 2)) * se_y
    if fam == "B":
        return sp.exp(-sp.sin((xa - xb) / 2) ** 2 / (2 * lx ** 2)) + se_y
    if fam == "C":
        return sp.exp(-(xa - xb) ** 2 / (2 * lx ** 2)) * se_y
    return sp.exp(-sp.sin(p * (xa - xb)) ** 2 / (2 * lx ** 2)) * se_y


def pair_exprs(fam):
    k = kernel(fam)
    e = {"k": k, "kxx": sp.diff(k, xa, xb), "kxy": sp.diff(k, xa, yb), "kyy": sp.diff(k, ya, yb)}
    for name in ENTRIES:
        e[name + "_dlx"] = sp.diff(e[name], lx)
        e[name + "_dly"] = sp.diff(e[name], ly)
    return e


def to_f64(v):
    """nearest fp64 of an mpf, one rounding, denormals included"""
    v = mp.mpf(v)
    if v == 0:
        return 0.0
    s, man, ex, _ = v._mpf_
    fr = Fraction(int(man)) * (Fraction(2) ** int(ex))
    if fr < Fraction(1, 2 ** 1200):
        return 0.0
    out = fr.numerator / fr.denominator
    return -out if s else out


def grid(v):
    return np.round(np.asarray(v, dtype=np.float64) / GRID) * GRID


def mpf(v):
    return mp.mpf(float(v))


def kxx_root(fam, lxv, pv):
    """dx > 0 nearest the smallest root of lx^2 cos 2h = (sin h cos h)^2 (C: dx = lx)"""
    if fam == "C":
        return float(lxv)
    hs = mpf(pv) if fam == "D" else mp.mpf("0.5")
    L2 = mpf(lxv) ** 2
    f = lambda h: L2 * mp.cos(2 * h) - (mp.sin(h) * mp.cos(h)) ** 2
    h = mp.findroot(f, (mp.mpf(0), mp.pi / 4), solver="anderson")
    return float(h / hs)


def placed_rows(fam, x0, y0, lxv, lyv, pv):
    """(dx, dy) of seven rows relative to the column points 0..6"""
    dpi = np.pi / (2 * pv) if fam == "D" else np.pi          # |h| ~ pi/2: |dx| ~ pi for A, B (C: just a separation)
    sep = [(0.0, 0.0),
           (kxx_root(fam, lxv, pv), lyv),
           (dpi, -lyv),
           (lxv * 2.0 ** -10, 0.5 * lyv),
           (2.0 * lxv, -6.0 * lyv),
           (-30.0 * lxv, lyv * 2.0 ** -10),
           (0.0, lyv * np.sqrt(2.0 * 726.0))]
    xs = [x0[j] + grid(dx) for j, (dx, _) in enumerate(sep)]
    ys = [y0[j] + grid(dy) for j, (_, dy) in enumerate(sep)]
    return np.array(xs), np.array(ys)


def combos(rng):
    """(lx, ly) nominal: the star design"""
    out = [(v, v) for v in (1e-2, 1e-1, 1.0, 10.0, 100.0)] + [(1e-2, 100.0), (100.0, 1e-2)]
    out += [tuple(10.0 ** rng.uniform(-2, 2, 2)) for _ in range(2)]
    return out


def eval_pairs(fns, x, y, x0, y0, hyp_args, sigv):
    n, n0 = len(x), len(x0)
    out = {name: np.zeros((n, n0)) for name in fns}
    for i in range(n):
        for j in range(n0):
            a = (mpf(x0[j]), mpf(y0[j]), mpf(x[i]), mpf(y[i])) + hyp_args      # a = column ("0") point, b = row point
            for name, f in fns.items():
                out[name][i, j] = to_f64(mpf(sigv) * f(*a))
    return out


def nd_kernel(fam, d):
    D = 2 * d
    A = sp.symbols("a0:%d" % D, real=True)
    B = sp.symbols("b0:%d" % D, real=True)
    ls = sp.symbols("l0:%d" % D, positive=True)
    ps = sp.symbols("p0:%d" % d, positive=True)
    fac = []
    for m in range(D):
        t = A[m] - B[m]
        if m < d and fam in "AB":
            fac.append(sp.exp(-sp.sin(t / 2) ** 2 / (2 * ls[m] ** 2)))
        elif m < d and fam == "D":
            fac.append(sp.exp(-sp.sin(ps[m] * t) ** 2 / (2 * ls[m] ** 2)))
        else:
            fac.append(sp.exp(-t ** 2 / (2 * ls[m] ** 2)))
    k = sum(fac) if fam == "B" else sp.prod(fac)
    hyp = ls + (ps if fam == "D" else ()) + (sig,)
    return sig * k, A, B, hyp


def nd_case(fam, d, nominal, rng):
    D = 2 * d
    k, A, B, hyp = nd_kernel(fam, d)
    args = A + B + hyp
    H = [[sp.lambdify(args, sp.diff(k, A[a], B[b]), "mpmath") for b in range(D)] for a in range(D)]
    l = np.array([nominal * FACT[m] for m in range(D)])
    X0 = np.column_stack([grid(rng.uniform(0, 2 * np.pi, ND_COL)) for _ in range(d)] +
                         [grid(rng.uniform(-3, 3, ND_COL)) for _ in range(d)])
    X = np.column_stack([grid(rng.uniform(0, 2 * np.pi, ND_ROW)) for _ in range(d)] +
                        [grid(rng.uniform(-3, 3, ND_ROW)) for _ in range(d)])
    seps = [np.zeros(6), np.array([0.5, 1, 2, 0.5, 1, 2]), np.array([2.0 ** -10, 6, 1, 2, 0.5, -1]), -np.ones(6)]
    for r, s in enumerate(seps):
        # row r sits at column point r + l_m * s_m: q's first, then P's
        sm = np.concatenate((s[:d], s[3:3 + d]))
        X[r] = X0[r] + grid(l * sm)
    pv = np.array(PVALS[:d])
    sigv = SIGS[(d + ord(fam)) % 3]
    hv = np.concatenate((l, pv, [sigv])) if fam == "D" else np.append(l, sigv)
    hm = tuple(mpf(v) for v in hv)
    K = np.zeros((D * ND_ROW, D * ND_COL))
    for i in range(ND_ROW):
        for j in range(ND_COL):
            pt = tuple(mpf(v) for v in X0[j]) + tuple(mpf(v) for v in X[i]) + hm
            for a in range(D):
                for b in range(D):
                    K[a * ND_ROW + i, b * ND_COL + j] = to_f64(H[a][b](*pt))
    return {"X": X, "X0": X0, "hyp": hv, "K": K}


def fit_case(fam, d, X, hv, reg, rng):
    """8-point fit on the points X (n x 2d): NLL, cond and 1/2 tr(W dK/dtheta) for every theta in (hyp, sig2n)"""
    D = 2 * d
    n = X.shape[0]
    k, A, B, hyp = nd_kernel(fam, d)
    args = A + B + hyp
    nb = 1 if reg else D
    ent = [[k if reg else sp.diff(k, A[a], B[b]) for b in range(nb)] for a in range(nb)]
    fK = [[sp.lambdify(args, e, "mpmath") for e in row] for row in ent]
    fdK = [[[sp.lambdify(args, sp.diff(e, th), "mpmath") for e in row] for row in ent] for th in hyp]
    hm = tuple(mpf(v) for v in hv)
    N = nb * n
    nl = D                                                   # lengths come first in hyp
    lmin = min(hv[:nl])
    sig2n = float(1e-2 * hv[-1] / lmin ** 2)
    z = grid(rng.standard_normal(N)) * float(np.sqrt(hv[-1]) / (2 * lmin))
    Km = mp.zeros(N, N)
    dKm = [mp.zeros(N, N) for _ in hyp]
    for i in range(n):
        for j in range(n):
            pt = tuple(mpf(v) for v in X[j]) + tuple(mpf(v) for v in X[i]) + hm
            for a in range(nb):
                for b in range(nb):
                    Km[a * n + i, b * n + j] = fK[a][b](*pt)
                    for t in range(len(hyp)):
                        dKm[t][a * n + i, b * n + j] = fdK[t][a][b](*pt)
    Ky = Km + mpf(sig2n) * mp.eye(N)
    Lc = mp.cholesky(Ky)
    zm = mp.matrix([mpf(v) for v in z])
    alpha = mp.cholesky_solve(Ky, zm)
    nll = mp.fdot(zm, alpha) / 2 + mp.fsum(mp.log(Lc[i, i]) for i in range(N))
    ev = mp.eigsy(Ky, eigvals_only=True)
    cond = max(ev) / min(ev)
    W = mp.inverse(Ky) - alpha * alpha.T
    dKm.append(mp.eye(N))                                    # d Ky / d sig2n, sig2n > 0
    grad, absum = [], []
    for dK in dKm:
        grad.append(to_f64(mp.fsum(W[i, j] * dK[i, j] for i in range(N) for j in range(N)) / 2))
        absum.append(to_f64(mp.fsum(abs(W[i, j]) * abs(dK[i, j]) for i in range(N) for j in range(N))))
    return {"X": X, "hyp": hv, "sig2n": np.array(sig2n), "z": z, "nll": np.array(to_f64(nll)),
            "cond": np.array(to_f64(cond)), "grad": np.array(grad), "absum": np.array(absum)}


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps, so the file is reproducible byte for byte"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    out = {}
    names = []
    for fam in "ABCD":
        ex = pair_exprs(fam)
        sy = (xa, ya, xb, yb, lx, ly) + ((p,) if fam == "D" else ())
        fns = {name: sp.lambdify(sy, e, "mpmath") for name, e in ex.items()}
        rng = np.random.default_rng(1000 + ord(fam))
        for c, (lxn, lyn) in enumerate(combos(rng)):
            lxv, lyv = float(lxn * LFAC), float(lyn * LFAC)
            sigv, pv = SIGS[c % 3], PVALS[c % 3]
            x0 = grid(rng.uniform(0, 2 * np.pi, N_COL))
            y0 = grid(rng.uniform(-3, 3, N_COL))
            xp, yp = placed_rows(fam, x0, y0, lxv, lyv, pv)
            x = np.concatenate((xp, grid(rng.uniform(0, 2 * np.pi, N_ROW - len(xp)))))
            y = np.concatenate((yp, grid(rng.uniform(-3, 3, N_ROW - len(yp)))))
            hv = np.array([lxv, lyv, pv, sigv] if fam == "D" else [lxv, lyv, sigv])
            vals = eval_pairs(fns, x, y, x0, y0, tuple(mpf(v) for v in hv[:-1]), sigv)
            key = "%s%d" % (fam, c)
            names.append(key)
            for nm, v in (("x", x), ("y", y), ("x0", x0), ("y0", y0), ("hyp", hv)):
                out["%s_%s" % (key, nm)] = v
            for nm, v in vals.items():
                out["%s_%s" % (key, nm)] = v
            print(key, hv, flush=True)
    out["pair_cases"] = np.array(names)

    nd_names = []
    for fam, d in (("A", 2), ("A", 3), ("C", 2), ("C", 3), ("B", 2), ("D", 2)):
        rng = np.random.default_rng(2000 + 10 * d + ord(fam))
        for c, nominal in enumerate((1e-2, 1.0, 100.0)):
            key = "nd_%s%d_%d" % (fam, d, c)
            nd_names.append(key)
            for nm, v in nd_case(fam, d, nominal, rng).items():
                out["%s_%s" % (key, nm)] = v
            print(key, flush=True)
    out["nd_cases"] = np.array(nd_names)

    fit_names = []
    for fam, d, reg in (("A", 1, False), ("C", 1, False), ("D", 1, False), ("B", 1, False), ("A", 2, False), ("A", 1, True)):
        rng = np.random.default_rng(3000 + 10 * d + ord(fam) + (100 if reg else 0))
        for c in (0, 2, 4):                                 # lx = ly = 1e-2, 1, 1e2 (times 1.37)
            if d == 1:
                pk = "%s%d" % (fam, c)
                X = np.column_stack((out[pk + "_x0"], out[pk + "_y0"]))
                hv = out[pk + "_hyp"]
            else:
                nominal = (1e-2, 1.0, 100.0)[c // 2]
                X = np.column_stack([grid(rng.uniform(0, 2 * np.pi, N_COL)) for _ in range(d)] +
                                    [grid(rng.uniform(-3, 3, N_COL)) for _ in range(d)])
                for r in range(1, 4):                         # three near neighbours, or every block is diagonal at 1e-2
                    X[r] = X[0] + grid(nominal * np.array(FACT[:2 * d]) * rng.uniform(-1.5, 1.5, 2 * d))
                hv = np.append(nominal * np.array(FACT[:2 * d]), SIGS[c % 3])
            if d == 1 and c == 0:
                X = X.copy()
                for r in range(1, 4):
                    X[r] = X[0] + grid(hv[:2] * rng.uniform(-1.5, 1.5, 2))
            key = "fit_%s%d%s_%d" % (fam, d, "r" if reg else "", c)
            fit_names.append(key)
            for nm, v in fit_case(fam, d, X, hv, reg, rng).items():
                out["%s_%s" % (key, nm)] = v
            print(key, flush=True)
    out["fit_cases"] = np.array(fit_names)

    path = os.path.join(HERE, "range.npz")
    write_npz(path, out)
    print("wrote range.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
