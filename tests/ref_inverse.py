"""NumPy restatement of the backward step of the d-pair symplectic map (csrc/map_nd.hip: applymap_nd_inverse_kernel), on top of
tests/ref_tangent.py (gradient, hessian).  Written from the mathematics: G = K*(x) alpha is the gradient of the generating function
F(q, P), G_q = p - P and G_P = Q - q, H = dG/dx symmetric with blocks A = H_qq, B = H_qP, C = H_PP.

    forward   solve  G_q(q, P) - p + P = 0  for P  (Jacobian I + B),    then  Q = q + G_P(q, P)
    backward  solve  q + G_P(q, P) - Q = 0  for q  (Jacobian I + B^T),  then  p = P + G_q(q, P)

Both pass through the same point x = (q, P).  Newton from q = Q (from P = p forward), stopping when max|step| <= tol max(1, max|unknown|)
or after maxiter iterations, as the kernel does; no wrapping inside a step (the callers wrap)."""
import numpy as np

from tests import ref_tangent as RT

TWO_PI = 2.0 * np.pi


def backward_jacobian(fam, d, hyp, X, alpha, q, P):
    """I + dG_P/dq = I + B^T at (q, P), (d, d)"""
    H = RT.hessian(fam, d, hyp, X, alpha, np.concatenate((q, P)))
    return np.eye(d) + H[:d, d:].T


def backward_step(fam, d, hyp, X, alpha, Q, P, tol=1e-13, maxiter=60):
    """(Q, P) -> (q, p, Newton iterations, closing residual max|q + G_P(q, P) - Q|)"""
    Q, P = np.asarray(Q, dtype=np.float64), np.asarray(P, dtype=np.float64)
    q, its = Q.copy(), 0
    for _ in range(maxiter):
        G = RT.gradient(fam, d, hyp, X, alpha, np.concatenate((q, P)))
        dq = np.linalg.solve(backward_jacobian(fam, d, hyp, X, alpha, q, P), -(q + G[d:] - Q))
        q = q + dq
        its += 1
        if np.abs(dq).max() <= tol * max(1.0, np.abs(q).max()):
            break
    G = RT.gradient(fam, d, hyp, X, alpha, np.concatenate((q, P)))
    return q, P + G[:d], its, float(np.abs(q + G[d:] - Q).max())


def forward_step(fam, d, hyp, X, alpha, q, p, tol=1e-13, maxiter=60):
    """(q, p) -> (Q, P, Newton iterations, closing residual max|G_q(q, P) - p + P|), the forward twin with I + B"""
    q, p = np.asarray(q, dtype=np.float64), np.asarray(p, dtype=np.float64)
    P, its = p.copy(), 0
    for _ in range(maxiter):
        x = np.concatenate((q, P))
        G = RT.gradient(fam, d, hyp, X, alpha, x)
        dP = np.linalg.solve(np.eye(d) + RT.hessian(fam, d, hyp, X, alpha, x)[:d, d:], -(G[:d] - p + P))
        P = P + dP
        its += 1
        if np.abs(dP).max() <= tol * max(1.0, np.abs(P).max()):
            break
    G = RT.gradient(fam, d, hyp, X, alpha, np.concatenate((q, P)))
    return q + G[d:], P, its, float(np.abs(G[:d] - p + P).max())


def _orbit(step, fam, d, hyp, X, alpha, nm, A0, B0, wrap_q):
    A0, B0 = np.asarray(A0, dtype=np.float64).reshape(-1, d), np.asarray(B0, dtype=np.float64).reshape(-1, d)
    Ntest = A0.shape[0]
    qm, pm = np.zeros((nm, Ntest, d)), np.zeros((nm, Ntest, d))
    its, res = np.zeros((nm - 1, Ntest), dtype=np.int32), np.zeros((nm - 1, Ntest))
    qm[0], pm[0] = A0, B0
    for i in range(nm - 1):
        for k in range(Ntest):
            qn, pn, its[i, k], res[i, k] = step(fam, d, hyp, X, alpha, qm[i, k], pm[i, k])
            qm[i + 1, k], pm[i + 1, k] = (np.mod(qn, TWO_PI) if wrap_q else qn), pn
    return qm, pm, its, res


def backward_orbit(fam, d, hyp, X, alpha, nm, Q0, P0, wrap_q=False):
    """row 0 = (Q0, P0) (Ntest, d), row i the i-th preimage -> qmap, pmap (nm, Ntest, d), iters and residuals (nm - 1, Ntest)"""
    return _orbit(backward_step, fam, d, hyp, X, alpha, nm, Q0, P0, wrap_q)


def forward_orbit(fam, d, hyp, X, alpha, nm, Q0, P0, wrap_q=False):
    return _orbit(forward_step, fam, d, hyp, X, alpha, nm, Q0, P0, wrap_q)


def circle_distance(a, b):
    """|a - b| mod 2 pi: the distance on the circle, so that a value at 0 / 2 pi compares equal to its neighbour across the seam"""
    diff = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return np.abs(diff - TWO_PI * np.round(diff / TWO_PI))      # (a small difference is kept exactly: no sum with pi)
