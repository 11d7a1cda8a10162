"""NumPy restatement of the gradient of the leave-one-point-out objectives (sgpr_fit_loo_grad) and what its tests share.

Notation of tests/ref_loo.py: point i owns the rows B_i = {c N + i}; C_i = (Ky^-1)[B_i, B_i], a_i = alpha[B_i], S_i = C_i^-1,
r_i = S_i a_i, loo = -sum lpd_i, press = sum |r_i|^2.  Then

    d obj / d theta = 1/2 sum_jk W'_jk dKy_jk / d theta,   W' = M - beta alpha^T - alpha beta^T,
    M = Ky^-1 W~ Ky^-1,  beta = Ky^-1 v,
    loo:    W~[B_i, B_i] = r_i r_i^T + S_i,              v[B_i] = r_i
    press:  W~[B_i, B_i] = 2 (r_i s_i^T + s_i r_i^T),    v[B_i] = 2 s_i,  s_i = S_i r_i

and the noise component is sign(sig2n) 1/2 tr W'.  `weights` is that formula in float64, `weights_mp` the same at 40 digits;
`reference` contracts W' with dKy obtained the way tests/test_gpu_nll_grad_full.py::_reference obtains it: the oracle's exact
forms where they exist (lx, ly of the families without a period; sig), central differences of the oracle's builders otherwise."""
import numpy as np

from tests import ref_loo as R

EPS = R.EPS


def weights(Ky, z, N, D, objective):
    """-> (W' (n x n), value)"""
    n = N * D
    Kinv = np.linalg.inv(Ky)
    Kinv = 0.5 * (Kinv + Kinv.T)
    alpha = np.linalg.solve(Ky, z)
    Wt, v = np.zeros((n, n)), np.zeros(n)
    value = 0.0
    for i in range(N):
        B = R.rows_of(i, N, D)
        C, a = Kinv[np.ix_(B, B)], alpha[B]
        S = np.linalg.inv(C)
        S = 0.5 * (S + S.T)
        r = S @ a
        if objective == "loo":
            Wt[np.ix_(B, B)] = np.outer(r, r) + S
            v[B] = r
            value -= -0.5 * a @ r + 0.5 * np.linalg.slogdet(C)[1] - 0.5 * D * R.LOG_2PI
        else:
            s = S @ r
            Wt[np.ix_(B, B)] = 2.0 * (np.outer(r, s) + np.outer(s, r))
            v[B] = 2.0 * s
            value += r @ r
    M = Kinv @ Wt @ Kinv
    beta = Kinv @ v
    Wp = M - np.outer(beta, alpha) - np.outer(alpha, beta)
    return 0.5 * (Wp + Wp.T), float(value)


def weights_mp(Ky, z, N, D, objective, digits=40):
    """the same formulas in mpmath at `digits` digits, from the same float64 Ky and z -> W' as a float64 array of the rounded
    high-precision entries, and the matrix of mpmath numbers itself"""
    import mpmath as mp
    with mp.workdps(digits):
        n = N * D
        K = mp.matrix(Ky.tolist())
        Kinv = K ** -1
        alpha = Kinv * mp.matrix(z.tolist())
        Wt, v = mp.zeros(n, n), mp.zeros(n, 1)
        for i in range(N):
            B = [int(b) for b in R.rows_of(i, N, D)]
            C = mp.matrix(D, D)
            for e in range(D):
                for c in range(D):
                    C[e, c] = Kinv[B[e], B[c]]
            S = C ** -1
            a = mp.matrix([alpha[b] for b in B])
            r = S * a
            s = S * r
            for e in range(D):
                for c in range(D):
                    Wt[B[e], B[c]] = r[e] * r[c] + S[e, c] if objective == "loo" else 2 * (r[e] * s[c] + s[e] * r[c])
                v[B[e]] = r[e] if objective == "loo" else 2 * s[e]
        M = Kinv * Wt * Kinv
        beta = Kinv * v
        Wp = M - beta * alpha.T - alpha * beta.T
        return np.array([[float(Wp[j, k]) for k in range(n)] for j in range(n)]), Wp


def builder(oracle, fam, kind, X, ofam=None):
    """build(hyp) = K without noise, from the oracle's Gram builders"""
    ofam = ofam or fam
    if kind == "reg":
        return lambda h: np.array(oracle.buildKreg(ofam, X[:, 0], X[:, 1], X[:, 0], X[:, 1], np.asarray(h, float), threads=8))
    if int(kind) == 1:
        return lambda h: np.array(oracle.build_K(ofam, X[:, 0], X[:, 1], X[:, 0], X[:, 1], np.asarray(h, float), threads=8))
    return lambda h: np.array(oracle.build_K_nd(ofam, X, X, np.asarray(h, float)))


def _central(build, hyp, k, rel=1e-5):
    h = np.array(hyp, dtype=float)
    step = rel * abs(h[k])
    hp, hm = h.copy(), h.copy()
    hp[k] += step
    hm[k] -= step
    return (build(hp) - build(hm)) / (2 * step)


def dKy(oracle, fam, kind, p, ofam=None):
    """-> (list of dKy / d hyp[k], mask of the exact ones), as test_gpu_nll_grad_full._reference"""
    ofam = ofam or fam
    X, hyp = p["X"], np.asarray(p["hyp"], float)
    build = builder(oracle, fam, kind, X, ofam)
    exact = {}
    if ofam != "D" and kind == "reg":
        exact = dict(enumerate(oracle.build_dKreg(ofam, X[:, 0], X[:, 1], X[:, 0], X[:, 1], hyp)))
    elif ofam != "D" and int(kind) == 1:
        exact = dict(enumerate(oracle.build_dK(ofam, X[:, 0], X[:, 1], X[:, 0], X[:, 1], hyp)))
    K = build(hyp)
    out, ex = [], np.zeros(len(hyp) + 1, bool)
    for k in range(len(hyp)):
        if k == len(hyp) - 1:
            out.append(K / hyp[-1])
            ex[k] = True
        elif k in exact:
            out.append(np.array(exact[k]))
            ex[k] = True
        else:
            out.append(_central(build, hyp, k))
    ex[len(hyp)] = True
    return out, ex


def contract(Wp, dKs, sgn):
    """-> (g, S): g_k = 1/2 sum W' dKy_k and its scale S_k = 1/2 sum |W' dKy_k|; the last component is the noise's"""
    g = [0.5 * np.sum(Wp * dK) for dK in dKs] + [sgn * 0.5 * np.trace(Wp)]
    S = [0.5 * np.sum(np.abs(Wp * dK)) for dK in dKs] + [0.5 * np.sum(np.abs(np.diag(Wp)))]
    return np.array(g), np.array(S)


def reference(oracle, fam, kind, p, objective, s2_sign=1.0, ofam=None):
    """-> dict(g, S, exact, value, cond) for the problem p of ref_loo.problem (its Ky holds |s2|)"""
    dKs, ex = dKy(oracle, fam, kind, p, ofam)
    Wp, value = weights(p["Ky"], p["z"], p["N"], p["D"], objective)
    g, S = contract(Wp, dKs, s2_sign)
    return {"g": g, "S": S, "exact": ex, "value": value, "cond": p["cond"]}


def compare(g, ref, what):
    """the NLL gradient's rule: |g - g_ref| <= max(1e-9, 100 cond eps) S per exact component, 1e-6 in place of 1e-9 for the
    difference-based ones; prints the figures before it asserts"""
    g = np.asarray(g)
    assert g.shape == ref["g"].shape and np.all(np.isfinite(g)), (what, g)
    tol = np.where(ref["exact"], max(1e-9, 100 * ref["cond"] * EPS), max(1e-6, 100 * ref["cond"] * EPS)) * ref["S"]
    err = np.abs(g - ref["g"])
    print("%s: cond %.3g  max err/S %.3g  max err/tol %.3g  (exact %s)" % (
        what, ref["cond"], (err / np.maximum(ref["S"], 1e-300)).max(), (err / tol).max(), ref["exact"].astype(int)))
    assert np.all(err <= tol), (what, g, ref["g"], err / ref["S"])
