"""NumPy restatement of the generating function F of a fit, its cross-covariance vectors and its prior (test infrastructure).

The observations of a fit are (dF/dq, dF/dP), so with alpha = Ky^-1 z
    F(x*) = sig sum_j [dk/dx(x_j; x*) alpha_j + dk/dy(x_j; x*) alpha_{N+j}],
the derivatives taken in the TRAINING point: dkdx_num / dkdy_num of the reference's kernels*.f90 (Oracle.scalar_x, ids 16 and
17).  d = 1 goes through those; d pairs through the per-coordinate forms of genfun_nd.hip (dx = x_train - x_test, g = f'/f,
E = sig k for the product families and sig f_c per coordinate for the sum family B).  Both return a dict:
    F (m,), T (m,) = sum_j sum_c |term| (the scale of F's rounding error), v (m, n) the cross vectors (F = v alpha),
    kappa (m, m) the prior sig k between the test points.
"""
import numpy as np


def _split_d1(fam, hyp):
    hyp = [float(h) for h in hyp]
    return (hyp[0], hyp[1], hyp[2], hyp[3]) if fam == "D" else (hyp[0], hyp[1], 0.0, hyp[2])


def genfun_d1(oracle, fam, x, y, hyp, alpha, q, P):
    """d = 1: x, y (N,) training points, hyp = (lx, ly, [p,] sig), alpha (2N,), test points q, P (m,)"""
    lx, ly, p, sig = _split_d1(fam, hyp)
    x, y, q, P = (np.asarray(a, dtype=np.float64) for a in (x, y, q, P))
    N, m = len(x), len(q)
    v = np.empty((m, 2 * N))
    for t in range(m):
        for j in range(N):
            v[t, j] = sig * oracle.scalar_x(fam, 16, x[j], y[j], q[t], P[t], lx, ly, p)
            v[t, N + j] = sig * oracle.scalar_x(fam, 17, x[j], y[j], q[t], P[t], lx, ly, p)
    kappa = np.array([[sig * oracle.scalar(fam, 0, q[t], P[t], q[s], P[s], lx, ly, p) for s in range(m)] for t in range(m)])
    terms = v * np.asarray(alpha, dtype=np.float64)[None, :]
    return {"F": terms.sum(axis=1), "T": np.abs(terms).sum(axis=1), "v": v, "kappa": kappa.reshape(m, m)}


def _factors(fam, hyp, Xa, Xb):
    """per coordinate and per pair (a of Xa, b of Xb): log f and g = f'/f at dx = Xa - Xb -> (arg, g), each (na, nb, D); sig"""
    Xa, Xb, hyp = (np.asarray(a, dtype=np.float64) for a in (Xa, Xb, hyp))
    D = Xa.shape[1]
    d = D // 2
    l = hyp[:D]
    hs = hyp[D:D + d] if fam == "D" else np.full(d, 0.5)
    dx = Xa[:, None, :] - Xb[None, :, :]
    arg = -0.5 * dx**2 / l**2
    g = -dx / l**2
    if fam != "C":                                     # the q's are periodic: f = exp(-sin(hs dx)^2 / (2 l^2))
        s, c = np.sin(hs * dx[..., :d]), np.cos(hs * dx[..., :d])
        arg[..., :d] = -0.5 * s * s / l[:d]**2
        g[..., :d] = -hs * s * c / l[:d]**2
    return arg, g, float(hyp[-1])


def kappa_nd(fam, hyp, Xa, Xb):
    """sig k(Xa_a, Xb_b) -> (na, nb): the product of the factors, their sum for family B"""
    arg, _, sig = _factors(fam, hyp, Xa, Xb)
    return sig * (np.exp(arg).sum(axis=2) if fam == "B" else np.exp(arg.sum(axis=2)))


def genfun_nd(fam, X, hyp, alpha, Xt):
    """d pairs: X (N, 2d) training points, hyp = (lq.., lP.., [p..,] sig), alpha (2 d N,), test points Xt (m, 2d)"""
    X, Xt = np.asarray(X, dtype=np.float64), np.asarray(Xt, dtype=np.float64)
    N, D = X.shape
    m = Xt.shape[0]
    arg, g, sig = _factors(fam, hyp, Xt, X)            # (m, N, D); dx = x_test - x_train here ...
    g = -g                                             # ... and g is odd in dx: this is g at dx = x_train - x_test
    E = sig * np.exp(arg) if fam == "B" else np.repeat(sig * np.exp(arg.sum(axis=2))[..., None], D, axis=2)
    v = np.transpose(E * g, (0, 2, 1)).reshape(m, D * N)      # entry c N + j
    terms = v * np.asarray(alpha, dtype=np.float64)[None, :]
    return {"F": terms.sum(axis=1), "T": np.abs(terms).sum(axis=1), "v": v, "kappa": kappa_nd(fam, hyp, Xt, Xt)}


def host_variance(res, Ky, ref=None):
    """var_t = kappa(t, t) - |L^-1 v_t|^2 from a genfun_* result and Ky = K + |sig2n| I (SciPy's Cholesky); ref: the index of
    the test point that serves as the reference -> the variance of F(x_t) - F(x_ref).  -> (var (m,), the priors (m,))"""
    import scipy.linalg
    v, kap = res["v"], res["kappa"]
    prior = np.diag(kap).copy()
    if ref is not None:
        v = v - v[ref][None, :]
        prior = prior - 2.0 * kap[:, ref] + kap[ref, ref]
    Lf = scipy.linalg.cholesky(Ky, lower=True)
    W = scipy.linalg.solve_triangular(Lf, v.T, lower=True)
    return prior - (W * W).sum(axis=0), prior
