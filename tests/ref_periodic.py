"""NumPy restatement of the periodic-orbit search of the d-pair symplectic map (csrc/periodic_nd.h), the CPU reference of
tests/test_gpu_periodic_nd.py, on top of tests/ref_tangent.py (gradient, hessian, step_matrix).  Written from the algorithm, not
from the kernel:

  * one step (q, p) -> (Q, P): Newton in P on f(P) = G_q(q, P) - p + P with the Jacobian I + H_qP from ref_tangent.hessian, to a
    step <= 1e-15 relative (or 60 iterations), then Q = q + G_P(q, P) in lifted coordinates; with `wrap` Q is reduced by
    floor(Q / 2 pi) turns, which are counted.  explicit: P = p - G_q(q, p), no solve (sum kernels).
  * one pass from z = (q, p): n steps, mono = M_n ... M_1 (ref_tangent.step_matrix at every accepted (q, P)), the residual
    r = ((Q_n - q_0) + 2 pi (turns - w), P_n - p_0) -- the small difference first; without `wrap` turns = 0 and Q_n is lifted.
  * the outer Newton: converged when the pass that started from z has max|r| <= tol max(1, max|z|), and that z is returned;
    otherwise z <- z + solve(mono - I, -r) (numpy.linalg.solve: LU with partial pivoting), with `wrap` the new q mod 2 pi.

x = (q_1..q_d, P_1..P_d); X (n0, D) training points; alpha (D n0,) block by block; hyp = (lq.., lP.., [p..,] sig)."""
import numpy as np

from tests import ref_tangent as RT

TWO_PI = 2.0 * np.pi


def step(fam, d, hyp, X, alpha, q, p, explicit=False):
    """-> Q (lifted), P, M (the step matrix at (q, P)), I + B there"""
    q, p = np.asarray(q, dtype=np.float64), np.asarray(p, dtype=np.float64)
    if explicit:
        P = p - RT.gradient(fam, d, hyp, X, alpha, np.concatenate((q, p)))[:d]
    else:
        P = p.copy()
        for _ in range(60):
            x = np.concatenate((q, P))
            f = RT.gradient(fam, d, hyp, X, alpha, x)[:d] - p + P
            dP = -np.linalg.solve(np.eye(d) + RT.hessian(fam, d, hyp, X, alpha, x)[:d, d:], f)
            P = P + dP
            if np.abs(dP).max() <= 1e-15 * max(1.0, np.abs(P).max()):
                break
    x = np.concatenate((q, P))
    Q = q + RT.gradient(fam, d, hyp, X, alpha, x)[d:]
    M, K = RT.step_matrix(RT.hessian(fam, d, hyp, X, alpha, x), d)
    return Q, P, M, K


def one_pass(fam, d, hyp, X, alpha, z, n, wind, wrap, explicit=False):
    """n steps from z -> r (D,), mono (D, D), the orbit rows q, p (n, d) (wrapped with `wrap`), the steps' M (n, D, D), I + B (n, d, d)"""
    z = np.asarray(z, dtype=np.float64)
    q, p = z[:d].copy(), z[d:].copy()
    turns = np.zeros(d)
    mono = np.eye(2 * d)
    qs, ps, Ms, Ks = [], [], [], []
    for _ in range(n):
        qs.append(q)
        ps.append(p)
        Q, P, M, K = step(fam, d, hyp, X, alpha, q, p, explicit)
        if wrap:
            t = np.floor(Q / TWO_PI)
            Q = Q - TWO_PI * t
            turns += t
        mono = M @ mono
        Ms.append(M)
        Ks.append(K)
        q, p = Q, P
    r = np.concatenate(((q - z[:d]) + TWO_PI * (turns - wind), p - z[d:]))
    return r, mono, np.array(qs), np.array(ps), np.array(Ms), np.array(Ks)


def solve(fam, d, hyp, X, alpha, z, n, wind=None, wrap=False, tol=1e-12, maxit=30, explicit=False):
    """-> dict: converged, z, resid, its (passes run, the converged one included; -1 failed), mono, q, p (n, d), M (n, D, D) and K (n, d, d), the
    step matrices and I + B of the returned orbit, inv_norm = |(mono - I)^-1|_inf, history (max|r| of every pass)"""
    D = 2 * d
    z = np.array(z, dtype=np.float64)
    wind = np.zeros(d) if wind is None else np.asarray(wind, dtype=np.float64)
    history = []
    fail = dict(converged=False, z=np.full(D, np.nan), resid=np.nan, its=-1, mono=np.full((D, D), np.nan), history=history)
    for it in range(1, maxit + 1):
        with np.errstate(all="ignore"):
            try:
                r, mono, qs, ps, Ms, Ks = one_pass(fam, d, hyp, X, alpha, z, n, wind, wrap, explicit)
            except np.linalg.LinAlgError:
                return fail
        rmax = np.abs(r).max()
        history.append(rmax)
        if not (np.isfinite(r).all() and np.isfinite(mono).all()):
            return fail
        if rmax <= tol * max(1.0, np.abs(z).max()):
            inv = np.linalg.inv(mono - np.eye(D))
            return dict(converged=True, z=z, resid=rmax, its=it, mono=mono, q=qs, p=ps, M=Ms, K=Ks,
                        inv_norm=np.abs(inv).sum(axis=1).max(), history=history)
        if it == maxit:
            break
        try:
            z = z + np.linalg.solve(mono - np.eye(D), -r)
        except np.linalg.LinAlgError:
            return fail
        if not np.isfinite(z).all():
            return fail
        if wrap:
            z[:d] -= TWO_PI * np.floor(z[:d] / TWO_PI)
    return fail
