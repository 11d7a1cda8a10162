"""NumPy restatement of leave-one-point-out cross-validation (sgpr_fit_loo, sgpr_fit_batch_loo) and the fixtures its tests share.

Point i of N owns the D rows B_i = {c N + i, c = 0 .. D-1} of Ky.  `loo_blocks` is the formula the device uses, from the D x D
diagonal blocks of an explicit inverse; `loo_by_deletion` is the definition: delete the point's rows and columns, refit on
the rest, predict the left-out rows."""
import numpy as np

EPS = np.finfo(np.float64).eps
LOG_2PI = float(np.log(2.0 * np.pi))


def rows_of(i, N, D):
    return np.arange(D) * N + i


def loo_blocks(Ky, z, N, D):
    """-> dict(resid (N, D), cov (N, D, D), lpd (N,), loo, press) through C_i = (Ky^-1)[B_i, B_i], a_i = alpha[B_i]"""
    Kinv = np.linalg.inv(Ky)
    Kinv = 0.5 * (Kinv + Kinv.T)
    alpha = np.linalg.solve(Ky, z)
    r, S, lpd = np.empty((N, D)), np.empty((N, D, D)), np.empty(N)
    for i in range(N):
        B = rows_of(i, N, D)
        C, a = Kinv[np.ix_(B, B)], alpha[B]
        S[i] = np.linalg.inv(C)
        S[i] = 0.5 * (S[i] + S[i].T)
        r[i] = np.linalg.solve(C, a)
        lpd[i] = -0.5 * a @ r[i] + 0.5 * np.linalg.slogdet(C)[1] - 0.5 * D * LOG_2PI
    return {"resid": r, "cov": S, "lpd": lpd, "loo": float(-lpd.sum()), "press": float(np.sum(r * r))}


def loo_by_deletion(Ky, z, N, D):
    """the same quantities from N refits without one point each"""
    n = N * D
    r, S, lpd = np.empty((N, D)), np.empty((N, D, D)), np.empty(N)
    for i in range(N):
        B = rows_of(i, N, D)
        keep = np.setdiff1d(np.arange(n), B)
        Koo, Kio = Ky[np.ix_(keep, keep)], Ky[np.ix_(B, keep)]
        mu = Kio @ np.linalg.solve(Koo, z[keep])
        S[i] = Ky[np.ix_(B, B)] - Kio @ np.linalg.solve(Koo, Kio.T)      # Ky's diagonal holds the noise
        S[i] = 0.5 * (S[i] + S[i].T)
        r[i] = z[B] - mu
        lpd[i] = -0.5 * r[i] @ np.linalg.solve(S[i], r[i]) - 0.5 * np.linalg.slogdet(S[i])[1] - 0.5 * D * LOG_2PI
    return {"resid": r, "cov": S, "lpd": lpd, "loo": float(-lpd.sum()), "press": float(np.sum(r * r))}


def tolerance(cond):
    """the project's rule for ill-conditioned fixtures, relative to the max-norm of each array"""
    return max(1e-10, 50.0 * cond * EPS)


def compare(got, ref, cond, what, keys=("resid", "cov", "lpd", "loo", "press")):
    """every requested quantity within tolerance(cond) of the max-norm of the reference array (loo and press: of their own
    magnitude); prints each figure before it asserts"""
    tol = tolerance(cond)
    errs = {k: float(np.max(np.abs(np.asarray(got[k]) - np.asarray(ref[k]))) / np.max(np.abs(ref[k]))) for k in keys}
    print("%s: cond %.3g tol %.3g  %s" % (what, cond, tol, "  ".join("%s %.3g" % kv for kv in errs.items())))
    for k in keys:
        assert np.all(np.isfinite(got[k])), (what, k)
        assert errs[k] <= tol, (what, k, errs[k], tol)


# ---- fixtures: seeded points and hyperparameters in the ranges of the batch-gradient tests --------------------------------

def _ell(n, d=1):
    return 2.0 * np.sqrt(12 * np.pi) * n ** (-1.0 / (2 * d))


def pair_hyp(fam, n):
    """(hyp, sig2n) of a d = 1 or reg problem of order n, as tests/test_gpu_nll_grad_full.py draws them"""
    l = _ell(n)
    return np.array([0.9 * l, 1.1 * l, 0.45, 1.3] if fam == "D" else [0.9 * l, 1.1 * l, 1.3]), 1e-2 / l ** 2


def nd_hyp(fam, N, d):
    l = _ell(N, d) * np.linspace(0.9, 1.15, 2 * d)
    h = list(l) + ([0.45 + 0.05 * m for m in range(d)] if fam == "D" else []) + [1.2]
    return np.array(h), 1e-2 / l.mean() ** 2


def problem(oracle, fam, kind, N, seed, ofam=None):
    """kind "reg" | 1 | 2 | 3 (pairs per point) -> dict(X (N, 2d), z, hyp, s2, D, N, Ky, cond).  hyp is jittered by up to 10 %
    like the batch-gradient problems; Ky = K + s2 I from the oracle's Gram builders."""
    ofam = ofam or fam
    rng = np.random.default_rng(seed)
    d = 1 if kind == "reg" else int(kind)
    D = 1 if kind == "reg" else 2 * d
    X = np.column_stack([rng.uniform(0, 2 * np.pi, (N, d)), rng.uniform(-3, 3, (N, d))])
    z = rng.standard_normal(D * N)
    if d == 1:
        hyp, s2 = pair_hyp(fam, D * N)
    else:
        hyp, s2 = nd_hyp(fam, N, d)
    hyp = hyp * rng.uniform(0.9, 1.1, len(hyp))
    if kind == "reg":
        K = oracle.buildKreg(ofam, X[:, 0], X[:, 1], X[:, 0], X[:, 1], hyp, threads=8)
    elif d == 1:
        K = oracle.build_K(ofam, X[:, 0], X[:, 1], X[:, 0], X[:, 1], hyp, threads=8)
    else:
        K = oracle.build_K_nd(ofam, X, X, hyp)
    Ky = np.array(K) + s2 * np.eye(D * N)
    Ky = 0.5 * (Ky + Ky.T)
    return {"X": X, "z": z, "hyp": hyp, "s2": float(s2), "D": D, "N": N, "Ky": Ky, "cond": float(np.linalg.cond(Ky))}
