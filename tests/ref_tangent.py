"""NumPy restatement of the tangent map of the d-pair symplectic map (csrc/maptan.h), the CPU reference of
tests/test_gpu_applymap_tangent.py.  Written from the mathematics, not from the kernel: every coordinate's factor is
f = exp(a) with a, a', a'', a''' in closed form, and g = f'/f = a', nh = -f''/f = -(a'' + a'^2), th = f'''/f = a''' + 3 a' a'' + a'^3;
T = (I + B)^-1 by numpy.linalg.solve.  tests/test_applymap_tangent_cpu.py holds the Hessian against sympy's own third
derivatives of the kernels tools/gen_kernels.py defines, and the step matrix against central differences of a CPU step.

x = (q_1..q_d, P_1..P_d); X (n0, D) training points; alpha (D n0,) block by block; hyp = (lq.., lP.., [p..,] sig).
Families: A, B periodic q-factors exp(-sin^2(dx / 2) / (2 l^2)), D exp(-sin^2(p dx) / (2 l^2)), C squared exponential; every
P-factor squared exponential; B is the sum kernel, the others products.  (USER as shipped is C.)"""
import numpy as np


def factor_terms(fam, d, hyp, dx):
    """dx (n, D) = x_train - x  ->  a, g, nh, th, each (n, D)"""
    hyp = np.asarray(hyp, dtype=np.float64)
    D = 2 * d
    l2 = hyp[:D] ** 2
    a, a1, a2, a3 = (np.empty_like(dx) for _ in range(4))
    for m in range(D):
        x = dx[:, m]
        if m < d and fam in "ABD":
            h = hyp[D + m] if fam == "D" else 0.5
            a[:, m] = -np.sin(h * x) ** 2 / (2 * l2[m])
            a1[:, m] = -h * np.sin(2 * h * x) / (2 * l2[m])
            a2[:, m] = -h * h * np.cos(2 * h * x) / l2[m]
            a3[:, m] = 2 * h ** 3 * np.sin(2 * h * x) / l2[m]
        else:
            a[:, m] = -x * x / (2 * l2[m])
            a1[:, m] = -x / l2[m]
            a2[:, m] = -1.0 / l2[m]
            a3[:, m] = 0.0
    return a, a1, -(a2 + a1 * a1), a3 + 3 * a1 * a2 + a1 ** 3


def _terms(fam, d, hyp, X, alpha, x):
    X = np.asarray(X, dtype=np.float64).reshape(-1, 2 * d)
    n0 = X.shape[0]
    al = np.asarray(alpha, dtype=np.float64).reshape(2 * d, n0).T
    a, g, nh, th = factor_terms(fam, d, hyp, X - np.asarray(x, dtype=np.float64)[None, :])
    sig = float(np.asarray(hyp)[-1])
    return al, a, g, nh, th, sig


def gradient(fam, d, hyp, X, alpha, x):
    """G(x) = K*(x) alpha (D,)"""
    al, a, g, nh, th, sig = _terms(fam, d, hyp, X, alpha, x)
    if fam == "B":
        return (sig * np.exp(a) * nh * al).sum(axis=0)
    E = sig * np.exp(a.sum(axis=1))[:, None]
    S = (g * al).sum(axis=1)[:, None]
    return (E * (nh * al - g * (S - g * al))).sum(axis=0)


def hessian(fam, d, hyp, X, alpha, x):
    """H = dG/dx (D, D), symmetric"""
    D = 2 * d
    al, a, g, nh, th, sig = _terms(fam, d, hyp, X, alpha, x)
    H = np.zeros((D, D))
    if fam == "B":
        H[np.arange(D), np.arange(D)] = (sig * np.exp(a) * al * th).sum(axis=0)
        return H
    E = sig * np.exp(a.sum(axis=1))
    S = (g * al).sum(axis=1)
    for c in range(D):
        H[c, c] = (E * (al[:, c] * th[:, c] - nh[:, c] * (S - g[:, c] * al[:, c]))).sum()
        for e in range(c + 1, D):
            rest = S - g[:, c] * al[:, c] - g[:, e] * al[:, e]
            H[c, e] = H[e, c] = -(E * (g[:, e] * nh[:, c] * al[:, c] + g[:, c] * nh[:, e] * al[:, e] - g[:, c] * g[:, e] * rest)).sum()
    return H


def step_matrix(H, d):
    """M (D, D) of one step from the Hessian at the accepted (q, P), rows (Q, P), columns (q, p); also I + B"""
    A, B, C = H[:d, :d], H[:d, d:], H[d:, d:]
    K = np.eye(d) + B
    T = np.linalg.solve(K, np.eye(d))
    TA = T @ A
    return np.block([[np.eye(d) + B.T - C @ TA, C @ T], [-TA, T]]), K


def jacobians(fam, d, hyp, X, alpha, q, p):
    """along an orbit q, p (nm, Ntest, d) (unwrapped or wrapped alike): M (nm - 1, Ntest, D, D) and I + B (nm - 1, Ntest, d, d);
    step i is evaluated at (q_i, P_{i+1})"""
    nm, Ntest = q.shape[:2]
    M = np.empty((nm - 1, Ntest, 2 * d, 2 * d))
    K = np.empty((nm - 1, Ntest, d, d))
    for i in range(nm - 1):
        for k in range(Ntest):
            M[i, k], K[i, k] = step_matrix(hessian(fam, d, hyp, X, alpha, np.concatenate((q[i, k], p[i + 1, k]))), d)
    return M, K


def gram_schmidt(Z):
    """modified Gram-Schmidt on the columns of Z in column order -> Q (orthonormal columns), diag(R)"""
    Z = np.array(Z, dtype=np.float64)
    D = Z.shape[1]
    r = np.empty(D)
    for c in range(D):
        r[c] = np.sqrt(Z[:, c] @ Z[:, c])
        Z[:, c] /= r[c]
        for e in range(c + 1, D):
            Z[:, e] -= (Z[:, c] @ Z[:, e]) * Z[:, c]
    return Z, r


def benettin(Ms, orth=gram_schmidt):
    """Ms (steps, D, D) in order -> sum of log |r_cc| per column divided by the number of steps"""
    D = Ms.shape[-1]
    Q, s = np.eye(D), np.zeros(D)
    for M in Ms:
        Q, r = orth(M @ Q)
        s += np.log(np.abs(r))
    return s / len(Ms)


def qr_orth(Z):
    Q, R = np.linalg.qr(Z)
    return Q, np.diag(R)


def monodromy(Ms):
    out = np.eye(Ms.shape[-1])
    for M in Ms:
        out = M @ out
    return out
