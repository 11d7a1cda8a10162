"""NumPy restatement of the sectioned d = 1 map, forwards and BACKWARDS (csrc/map.hip: map_step_inverse,
applymap_sections_inverse_kernel), on the CPU oracle's rows: r1, r2 = K*(1,:).alpha, K*(2,:).alpha at (q, P) from
oracle.predict_rows with one section's data.  `d` is the dict of tests.test_gpu_applymap_sections._sections.

    forward   solve  P + r1(q, P) - p = 0  for P  (MINPACK from P = p),  then  Q = q + r2(q, P)
    backward  solve  q + r2(q, P) - Q = 0  for q,                        then  p = P + r1(q, P)

Both pass through the same point (q, P).  The backward solve is the kernel's secant, statement by statement: q0 = Q, f0 = r2(q0, P),
q1 = q0 - f0, at most maxiter updates, stopped when |q1 - q0| <= tol max(1, |q1|), when f1 is not finite or when f1 == f0; accepted
when f1 is finite and |f1| <= 1e-8 max(1, |Q|); `iters` counts the updates (-1 for a lost step).  backward_step_minpack solves the
same equation with MINPACK hybrd (scipy.optimize.fsolve, xtol 1e-13).  Step i of a backward orbit undoes section (first - i) mod
nsec, step i of a forward orbit uses section (first + i) mod nsec.  WRAP_Q = 1 wraps the new q, LOSS_NEGP = 8 loses an orbit whose
new momentum is negative."""
import numpy as np
import scipy.optimize

TWO_PI = 2.0 * np.pi
WRAP_Q, LOSS_NEGP = 1, 8


class Rows:
    """rows(q, P) -> (r1, r2) of section m; remembers the largest |r| it met (the scale of the sums' rounding)"""

    def __init__(self, oracle, d, m):
        self.args = (d["fam"], d["xt"][:, m], d["yt"][:, m], d["hyp"][m], d["alpha"][:, m])
        self.oracle, self.rmax = oracle, 0.0

    def __call__(self, q, P):
        fam, xt, yt, hyp, alpha = self.args
        r1, r2 = self.oracle.predict_rows(fam, [q], [P], xt, yt, hyp, alpha)
        r1, r2 = float(r1[0]), float(r2[0])
        if np.isfinite(r1) and np.isfinite(r2):
            self.rmax = max(self.rmax, abs(r1), abs(r2))
        return r1, r2


def _finish(q, p, mode):
    """the new point, or NaN if the new momentum is negative with LOSS_NEGP; q wrapped with WRAP_Q"""
    if not (np.isfinite(q) and np.isfinite(p)) or ((mode & LOSS_NEGP) and p < 0.0):
        return np.nan, np.nan
    return (q - TWO_PI * np.floor(q / TWO_PI) if mode & WRAP_Q else q), p


def backward_step(rows, Q, P, mode=0, tol=1e-13, maxiter=60):
    """(Q, P) -> (q, p, secant updates, closing residual |q + r2(q, P) - Q|); lost: (nan, nan, -1, nan)"""
    lost = (np.nan, np.nan, -1, np.nan)
    if not (np.isfinite(Q) and np.isfinite(P)):
        return lost
    q0 = Q
    r1, r2 = rows(q0, P)
    f0 = r2
    q1 = q0 - f0
    r1, r2 = rows(q1, P)
    f1 = q1 + r2 - Q
    it = 0
    while it < maxiter:
        if not (abs(q1 - q0) > tol * max(1.0, abs(q1))) or not np.isfinite(f1):
            break
        dd = f1 - f0
        if dd == 0.0:
            break
        qs = q1 - f1 * (q1 - q0) / dd
        q0, f0, q1 = q1, f1, qs
        r1, r2 = rows(q1, P)
        f1 = q1 + r2 - Q
        it += 1
    if not (np.isfinite(f1) and abs(f1) <= 1e-8 * max(1.0, abs(Q))):
        return lost
    q, p = _finish(q1, P + r1, mode)
    return (q, p, it, abs(f1)) if np.isfinite(p) else lost


def _fsolve(f, x0):
    """MINPACK hybrd at xtol 1e-13.  Its progress test can fire at the rounding floor of the residual although it stands on the
    root (ier = 5); the point is taken only if a second run of the same solver from it ends with ier = 1 without moving
    (tests/test_gpu_applymap_inverse.py: _ref_inverse_nd)."""
    x, _, ier, msg = scipy.optimize.fsolve(f, [x0], xtol=1e-13, full_output=True)
    if ier != 1:
        x2, _, ier, msg = scipy.optimize.fsolve(f, x, xtol=1e-13, full_output=True)
        assert ier == 1 and abs(x2[0] - x[0]) <= 1e-13 * max(1.0, abs(x[0])), msg
        x = x2
    return float(x[0])


def backward_step_minpack(rows, Q, P, mode=0):
    """the same step with MINPACK on g(q) = q + r2(q, P) - Q from q = Q -> (q, p, 0, closing residual)"""
    if not (np.isfinite(Q) and np.isfinite(P)):
        return np.nan, np.nan, -1, np.nan
    qs = _fsolve(lambda q: q[0] + rows(q[0], P)[1] - Q, Q)
    r1, r2 = rows(qs, P)
    q, p = _finish(qs, P + r1, mode)
    return (q, p, 0, abs(qs + r2 - Q)) if np.isfinite(p) else (np.nan, np.nan, -1, np.nan)


def forward_step_minpack(rows, q, p, mode=0):
    """(q, p) -> (Q, P, 0, closing residual |P + r1(q, P) - p|) with MINPACK on f(P) from P = p"""
    if not (np.isfinite(q) and np.isfinite(p)):
        return np.nan, np.nan, -1, np.nan
    Pn = _fsolve(lambda P: P[0] + rows(q, P[0])[0] - p, p)
    r1, r2 = rows(q, Pn)
    Q, Pn2 = _finish(q + r2, Pn, mode)
    return (Q, Pn2, 0, abs(Pn + r1 - p)) if np.isfinite(Pn2) else (np.nan, np.nan, -1, np.nan)


def _orbit(oracle, d, step, direction, mode, nm, A0, B0, first):
    A0, B0 = np.asarray(A0, dtype=np.float64), np.asarray(B0, dtype=np.float64)
    Ntest, nsec = len(A0), d["nsec"]
    rows = [Rows(oracle, d, m) for m in range(nsec)]
    qm, pm = np.full((nm, Ntest), np.nan), np.full((nm, Ntest), np.nan)
    its, res = np.full((max(nm - 1, 0), Ntest), -1, dtype=np.int32), np.full((max(nm - 1, 0), Ntest), np.nan)
    qm[0], pm[0] = A0, B0
    for i in range(nm - 1):
        m = (first + direction * i) % nsec
        for k in range(Ntest):
            qm[i + 1, k], pm[i + 1, k], its[i, k], res[i, k] = step(rows[m], qm[i, k], pm[i, k], mode)
    return qm, pm, its, res, max(r.rmax for r in rows)


def backward_orbit(oracle, d, mode, nm, Q0, P0, first=0, minpack=False):
    """row 0 = (Q0, P0), row i the i-th preimage; step i undoes section (first - i) mod nsec
    -> qmap, pmap (nm, Ntest), iters, residuals (nm - 1, Ntest), max |r| met"""
    return _orbit(oracle, d, backward_step_minpack if minpack else backward_step, -1, mode, nm, Q0, P0, first)


def forward_orbit(oracle, d, mode, nm, Q0, P0, first=0):
    """the forward orbit by MINPACK; step i uses section (first + i) mod nsec -> as backward_orbit"""
    return _orbit(oracle, d, forward_step_minpack, +1, mode, nm, Q0, P0, first)
