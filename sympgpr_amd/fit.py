"""Device-resident fit: Gram build + Cholesky + alpha without K ever leaving HBM.

Host-side owner of a ``sgpr_fit_t`` handle (include/sympgpr_hip.h); the same sequence the
reference runs in ``nll_chol`` / ``gpsolve`` (python/functions/func.py:165-171,189-196).
"""
import ctypes as C

import numpy as np

from . import _lib as L


class SympFit:
    def __init__(self, family, x, y, z, hyp, sig2n, lower_only=True, stream=None, reg=False, block=None):
        """reg=True: the scalar-kernel GP of buildKreg / nll_chol_reg (order n = len(x)).
        block="qq" | "PP": only that diagonal block of build_K (order n = len(x)), the systems
        nll_expl factors (04_standard_map/func.py:126-141)."""
        self._lib = L.load_library()
        self._h = C.c_void_p()
        x, y, hyp = L.f64(x), L.f64(y), L.f64(hyp)
        if x.shape != y.shape or x.ndim != 1:
            raise ValueError("x and y must be 1-D arrays of equal length")
        self.n_pts = len(x)
        self.d, self.reg = 1, bool(reg)
        if block not in (None, "qq", "PP") or (block and reg):
            raise ValueError("block must be None, 'qq' or 'PP' (and excludes reg)")
        self.n = self.n_pts if (reg or block) else 2 * self.n_pts
        self.nhyp = len(hyp)
        z = L.f64(z) if z is not None else np.zeros(self.n)
        if z.shape != (self.n,):
            raise ValueError("z must have length %d" % self.n)
        flags = (L.FIT_LOWER_ONLY if lower_only else 0) | (L.FIT_REG if reg else 0)
        flags |= {None: 0, "qq": L.FIT_BLOCK_QQ, "PP": L.FIT_BLOCK_PP}[block]
        L.check(self._lib.sgpr_fit_create(L.family_id(family), self.n_pts, L.dptr(x), L.dptr(y), L.dptr(z),
                                          L.dptr(hyp), len(hyp), float(sig2n), flags,
                                          C.c_void_p(stream or 0), C.byref(self._h)), "sgpr_fit_create")

    @classmethod
    def pairs(cls, family, X, z, hyp, sig2n, stream=None):
        """d canonical pairs per point (BASELINE configs d = 2, 3): X is (n_pts, 2d) with columns
        (q_1..q_d, P_1..P_d), hyp = (lq_1..lq_d, lP_1..lP_d, sig), z has 2*d*n_pts entries ordered
        block by block like the rows of K.  d = 1 is the reference's layout."""
        self = cls.__new__(cls)
        self._lib = L.load_library()
        self._h = C.c_void_p()
        X = np.asfortranarray(X, dtype=np.float64)
        if X.ndim != 2 or X.shape[1] % 2:
            raise ValueError("X must be (n_pts, 2d)")
        self.n_pts, D = X.shape
        self.d, self.reg = D // 2, False
        self.n = D * self.n_pts
        hyp = L.f64(hyp)
        self.nhyp = len(hyp)
        z = L.f64(z) if z is not None else np.zeros(self.n)
        if z.shape != (self.n,):
            raise ValueError("z must have length %d" % self.n)
        L.check(self._lib.sgpr_fit_create_nd(L.family_id(family), self.d, self.n_pts, L.dptr(X), max(self.n_pts, 1),
                                             L.dptr(z), L.dptr(hyp), len(hyp), float(sig2n), 0,
                                             C.c_void_p(stream or 0), C.byref(self._h)), "sgpr_fit_create_nd")
        return self

    def predict_pairs(self, Xt):
        """K* . alpha for test points Xt (m, 2d) -> (m, 2d): column a = predicted dF/dx_a.  Needs a solved fit (run()); not
        defined for reg=True and block="qq" / "PP" fits (SympGPRError, SGPR_E_STATE): predict_rows serves a reg=True fit."""
        Xt = np.asfortranarray(np.atleast_2d(Xt), dtype=np.float64)
        m = Xt.shape[0]
        out = np.empty((m, Xt.shape[1]), order="F")
        L.check(self._lib.sgpr_fit_predict_nd(self._h, m, L.dptr(Xt), max(m, 1), L.dptr(out)), "sgpr_fit_predict_nd")
        return out

    def predict_pairs_cov(self, Xt):
        """Posterior mean and covariance at test points Xt (m, 2d) of a create_nd / pairs fit, D = 2d outputs per point.
        -> (mean (m, D), cov (m, D, D)).  Column / index a is dF/dx_a, as in predict_pairs; for d > 1 `mean` has the bits of
        predict_pairs(Xt) (for d = 1 those of predict_rows, the same numbers to rounding).  cov[t] = K**_t - K*_t Ky^-1 K*_t^T
        with K**_t the latent prior (no |sig2n| added): the covariance of the noise-free map, not of a new noisy observation.
        Exactly symmetric; the values are returned as computed, so next to a training point rounding can leave a diagonal
        entry slightly negative.  Needs a solved fit (run())."""
        Xt = np.asfortranarray(np.atleast_2d(Xt), dtype=np.float64)
        if Xt.ndim != 2 or Xt.shape[1] != 2 * self.d:
            raise ValueError("Xt must be (m, %d)" % (2 * self.d))
        return self._predict_cov(Xt)

    def predict_cov(self, q, P):
        """Posterior mean and covariance at the test points (q, P) of a d = 1 pair fit (D = 2) or a reg=True fit (D = 1).
        -> (mean (m, D), cov (m, D, D)).  Pair fit: index 0 is predict_rows' out_p, index 1 its out_q, and `mean` has their
        bits; reg fit: mean[:, 0] is predict_rows' out_p.  cov[t] = K**_t - K*_t Ky^-1 K*_t^T with K**_t the latent prior (no
        |sig2n| added).  Exactly symmetric; the values are returned as computed, so next to a training point rounding can leave
        a diagonal entry slightly negative.  Needs a solved fit (run()); not defined for block="qq" / "PP" fits."""
        if self.d != 1:
            raise ValueError("predict_cov is for d = 1 fits: use predict_pairs_cov")
        q, P = L.f64(np.atleast_1d(q)), L.f64(np.atleast_1d(P))
        if q.shape != P.shape or q.ndim != 1:
            raise ValueError("q and P must be 1-D arrays of equal length")
        return self._predict_cov(np.asfortranarray(np.column_stack((q, P)).reshape(len(q), 2)))

    def _predict_cov(self, Xt):
        m, D = Xt.shape[0], 1 if self.reg else 2 * self.d
        mean = np.empty((m, D), order="F")
        cov = np.empty((m, D, D))       # C order: point t's D x D block contiguous; symmetric, so its order does not matter
        L.check(self._lib.sgpr_fit_predict_cov(self._h, m, L.dptr(Xt), max(m, 1), L.dptr(mean), L.dptr(cov)),
                "sgpr_fit_predict_cov")
        return mean, cov

    def predict_genfun(self, q, P, ref=None, var=False):
        """The learned generating function F itself at the test points (q, P) of a d = 1 pair fit -> F (m,), or (F, var) with
        var=True.  Every other prediction returns derivatives of this F: dF/dq = predict_rows' out_p and dF/dP = its out_q.
        ref = (q0, P0): F(q, P) - F(q0, P0) and the variance of that difference; at a point equal to ref, F is exactly 0.0.
        The variance is that of the latent posterior (no |sig2n| added) and is returned as computed, so rounding can leave it
        slightly negative.  Derivative observations do not fix the constant of F: without ref the variance is dominated by the
        undetermined constant and does not vanish with data, while the variance of a difference does.  A NaN coordinate gives
        NaN for that point only.  Needs a solved fit (run()); not defined for reg=True (there predict_rows returns F) and
        block="qq" / "PP" fits."""
        if self.d != 1:
            raise ValueError("predict_genfun is for d = 1 fits: use predict_pairs_genfun")
        if self.reg:
            raise ValueError("predict_genfun is not defined for a reg=True fit: predict_rows returns its F")
        q, P = L.f64(np.atleast_1d(q)), L.f64(np.atleast_1d(P))
        if q.shape != P.shape or q.ndim != 1:
            raise ValueError("q and P must be 1-D arrays of equal length")
        return self._predict_genfun(np.asfortranarray(np.column_stack((q, P)).reshape(len(q), 2)), ref, var)

    def predict_pairs_genfun(self, Xt, ref=None, var=False):
        """The learned generating function F itself at test points Xt (m, 2d) of a create_nd / pairs fit -> F (m,), or (F, var)
        with var=True.  predict_pairs returns its gradient: column a is dF/dx_a (for d = 1: dF/dq = predict_rows' out_p and
        dF/dP = its out_q).  ref (2d,): F(x) - F(ref) and the variance of that difference; at a point equal to ref, F is exactly
        0.0.  The variance is that of the latent posterior (no |sig2n| added) and is returned as computed, so rounding can
        leave it slightly negative.  Derivative observations do not fix the constant of F: without ref the variance is
        dominated by the undetermined constant and does not vanish with data, while the variance of a difference does.  A NaN
        coordinate gives NaN for that point only.  Needs a solved fit (run()); not defined for reg=True fits."""
        if self.reg:
            raise ValueError("predict_pairs_genfun is not defined for a reg=True fit: predict_rows returns its F")
        Xt = np.asfortranarray(np.atleast_2d(Xt), dtype=np.float64)
        if Xt.ndim != 2 or Xt.shape[1] != 2 * self.d:
            raise ValueError("Xt must be (m, %d)" % (2 * self.d))
        return self._predict_genfun(Xt, ref, var)

    def _predict_genfun(self, Xt, ref, var):
        m = Xt.shape[0]
        if ref is not None:
            ref = L.f64(np.ravel(ref))
            if ref.shape != (2 * self.d,):
                raise ValueError("ref must hold %d coordinates" % (2 * self.d))
        F = np.empty(m)
        v = np.empty(m) if var else None
        L.check(self._lib.sgpr_fit_predict_genfun(self._h, m, L.dptr(Xt), max(m, 1), L.dptr(ref) if ref is not None else None,
                                                  L.dptr(F), L.dptr(v) if var else None), "sgpr_fit_predict_genfun")
        return (F, v) if var else F

    def applymap_pairs(self, nm, Q0, P0, wrap_q=False, explicit=False, return_iters=False):
        """nm - 1 steps of the fit's symplectic map for the start points Q0, P0 (Ntest, d) -- for d = 1 also (Ntest,) --, every
        step on the device: per step the implicit equation G_q(q, P) - p + P = 0 is solved for P by Newton with the analytic
        Jacobian (G = predict_pairs), then Q = q + G_P(q, P).  wrap_q: every q_i mod 2 pi; explicit: P = p - G_q(q, p), no
        solve.  -> qmap, pmap (nm, Ntest, d), row 0 the start points, NaN from the step at which an orbit is lost; with
        return_iters also iters (nm - 1, Ntest): Newton iterations per solve, 0 in explicit mode, -1 for a lost orbit.
        Needs a solved fit (run()); not defined for reg=True and block="qq" / "PP" fits."""
        from . import maps
        mode = (maps.WRAP_Q if wrap_q else 0) | (maps.EXPLICIT if explicit else 0)
        qmap, pmap, iters, _ = maps._map_call_nd("sgpr_fit_applymap_nd", (self._h,), self.d, mode, nm, Q0, P0)
        return (qmap, pmap, iters) if return_iters else (qmap, pmap)

    def applymap_pairs_tangent(self, nm, Q0, P0, wrap_q=False, explicit=False, jac=True, mono=True, lyap=True):
        """applymap_pairs with the tangent map -> (qmap, pmap, iters, out): the same orbits bit for bit, and in the dict `out`
        the requested arrays jac (nm - 1, Ntest, D, D), mono (Ntest, D, D), lyap (Ntest, D) with D = 2 d -- see
        maps.run_map_nd_tangent; maps.symplectic_defect and maps.greene_residue (d = 1) read them.  explicit: sum kernels only."""
        from . import maps
        mode = (maps.WRAP_Q if wrap_q else 0) | (maps.EXPLICIT if explicit else 0)
        return maps._map_call_nd("sgpr_fit_applymap_nd_tangent", (self._h,), self.d, mode, nm, Q0, P0, tangent=(jac, mono, lyap))

    def applymap_pairs_inverse(self, nm, Q0, P0, wrap_q=False, return_iters=False):
        """applymap_pairs backwards: Q0, P0 (Ntest, d) -- for d = 1 also (Ntest,) -- are points (Q, P), and row i of qmap, pmap
        (nm, Ntest, d) is their i-th preimage under the fit's (implicit) map, row 0 the start points: per step
        q + G_P(q, P) - Q = 0 is solved for q by Newton from q = Q with the transposed Jacobian block of the forward solve, then
        p = P + G_q(q, P).  wrap_q: every solved q_i mod 2 pi.  There is no explicit mode: the explicit product-family map has
        another inverse, and for the sum kernels the two maps coincide.  NaN from the step at which an orbit is lost; with
        return_iters also iters (nm - 1, Ntest), -1 for a lost orbit.  The tangent map of a backward orbit:
        maps.symplectic_inverse.  Needs a solved fit (run()); not defined for reg=True and block="qq" / "PP" fits."""
        from . import maps
        mode = maps.WRAP_Q if wrap_q else 0
        qmap, pmap, iters, _ = maps._map_call_nd("sgpr_fit_applymap_nd_inverse", (self._h,), self.d, mode, nm, Q0, P0)
        return (qmap, pmap, iters) if return_iters else (qmap, pmap)

    def periodic_orbits(self, n, Q0, P0, wind=None, wrap_q=False, explicit=False, tol=1e-12, maxit=30, mono=True, orbit=False):
        """Periodic orbits of the fit's symplectic map (the map of applymap_pairs; d = 1 fits too): for every guess (Q0, P0)
        (Ntest, d) -- for d = 1 also (Ntest,) -- Newton on the n-fold map with the winding numbers wind, all passes in one
        device launch, one workgroup per guess.  -> dict with z, resid, its, converged and, as asked, mono, q, p: see
        maps.run_periodic_nd, whose hazard applies here as well -- far from the training data the learned map is the identity,
        every point there is a "fixed point" with mono = I, and results whose mono - I is negligible are to be discarded.
        maps.multipliers and maps.greene_residue (d = 1) classify the orbits.  explicit: sum kernels only.
        Needs a solved fit (run()); not defined for reg=True and block="qq" / "PP" fits."""
        from . import maps
        mode = (maps.WRAP_Q if wrap_q else 0) | (maps.EXPLICIT if explicit else 0)
        return maps._periodic_call_nd("sgpr_fit_periodic_nd", (self._h,), self.d, mode, n, Q0, P0, wind, tol, maxit, mono, orbit)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.sgpr_fit_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_hyp(self, hyp, sig2n):
        hyp = L.f64(hyp)
        L.check(self._lib.sgpr_fit_set_hyp(self._h, L.dptr(hyp), len(hyp), float(sig2n)), "sgpr_fit_set_hyp")

    def set_targets(self, z):
        z = L.f64(z)
        if z.shape != (self.n,):
            raise ValueError("z must have length 2*n_pts")
        L.check(self._lib.sgpr_fit_set_targets(self._h, L.dptr(z)), "sgpr_fit_set_targets")

    def build(self):
        L.check(self._lib.sgpr_fit_build(self._h), "sgpr_fit_build")

    def factor(self):
        L.check(self._lib.sgpr_fit_factor(self._h), "sgpr_fit_factor")

    def solve(self):
        L.check(self._lib.sgpr_fit_solve(self._h), "sgpr_fit_solve")

    def run(self):
        L.check(self._lib.sgpr_fit_run(self._h), "sgpr_fit_run")
        return self

    def alpha(self):
        out = np.empty(self.n)
        L.check(self._lib.sgpr_fit_alpha(self._h, L.dptr(out)), "sgpr_fit_alpha")
        return out

    def nll(self):
        v = C.c_double()
        L.check(self._lib.sgpr_fit_nll(self._h, C.cast(C.byref(v), L._dp)), "sgpr_fit_nll")
        return v.value

    def nll_grad(self):
        """d nll / d(lx, ly) (functions/func.py:132-162: nlp_grad) on a solved fit."""
        g = np.empty(2)
        L.check(self._lib.sgpr_fit_nll_grad(self._h, L.dptr(g)), "sgpr_fit_nll_grad")
        return g

    def nll_grad_full(self):
        """Gradient of the fit's NLL (1/2 z^T alpha + sum log L_ii) in every hyperparameter, on a solved fit: an ndarray of
        shape (nhyp + 1,).  Entries 0 .. nhyp-1 follow the fit's hyp order -- (lx, ly, [p,] sig) for SympFit(...) and
        SympFit(..., reg=True), (lq_1..lq_d, lP_1..lP_d, [p_1..p_d,] sig) for SympFit.pairs --, the last entry is d/dsig2n.
        Ky holds |sig2n|, so that entry is sign(sig2n) * 1/2 (tr Ky^-1 - alpha^T alpha), with sign(0) = +1.  Exact (no
        finite differences), deterministic, and the factor, alpha and nll() are left as they are.  Not defined for
        block="qq" / "PP" fits.  With SciPy's L-BFGS-B over (hyp, sig2n):

            def fun(h):
                f.set_hyp(h[:-1], h[-1]); f.run()
                return f.nll(), f.nll_grad_full()
            res = scipy.optimize.minimize(fun, np.append(hyp, sig2n), jac=True, method="L-BFGS-B")
        """
        g = np.empty(self.nhyp + 1)
        L.check(self._lib.sgpr_fit_nll_grad_full(self._h, L.dptr(g), len(g)), "sgpr_fit_nll_grad_full")
        return g

    def loo(self, resid=True, cov=False, lpd=True):
        """Leave-one-point-out cross-validation of a solved fit -> dict with "loo", "press" and the requested arrays.
        Point i owns D rows of Ky (D = 2d; 1 with reg=True), and leaving it out removes them together.  "resid" (N, D): column c
        is part c of the observed rows minus their prediction from the fit without point i; "cov" (N, D, D): the covariance of
        that prediction, noise included, indexed as predict_cov's and exactly symmetric; "lpd" (N,): the log predictive density
        of the left-out rows.  loo = -sum lpd is an objective to minimise like nll(); press = sum |resid_i|^2.  A point whose
        block of Ky^-1 is not positive definite to rounding gives NaN in its entries and in loo and press.  Exact (Ky^-1 from
        the cached factor by row panels, 2 n^3 / 3 flop), deterministic, and the factor, alpha and nll() are left as they are.
        Not defined for block="qq" / "PP" fits."""
        N, D = self.n_pts, 1 if self.reg else 2 * self.d
        two = np.empty(2)
        r = np.empty(self.n) if resid else None
        c = np.empty((N, D, D)) if cov else None
        l = np.empty(N) if lpd else None
        opt = lambda a: L.dptr(a) if a is not None else None
        L.check(self._lib.sgpr_fit_loo(self._h, L.dptr(two), opt(r), opt(c), opt(l)), "sgpr_fit_loo")
        out = {"loo": float(two[0]), "press": float(two[1])}
        if resid:
            out["resid"] = np.ascontiguousarray(r.reshape(D, N).T)
        if cov:
            out["cov"] = c
        if lpd:
            out["lpd"] = l
        return out

    def loo_grad(self, objective="loo"):
        """One of loo()'s objectives and its exact gradient in every hyperparameter, on a solved fit -> (value, grad).
        objective "loo" (-sum lpd) or "press"; grad has shape (nhyp + 1,) in nll_grad_full's order, the last entry d/dsig2n with
        the sign of sig2n.  One weight matrix M = Ky^-1 W Ky^-1 serves all hyperparameters (about 5 n^3 / 3 flop, two n x n
        blocks of device scratch that release_scratch() gives back); deterministic, and the factor, alpha and nll() are left as
        they are.  A point whose block of Ky^-1 is not positive definite to rounding gives NaN in the value and the whole
        gradient.  Not defined for block="qq" / "PP" fits.  With SciPy's L-BFGS-B over (hyp, sig2n):

            def fun(h):
                f.set_hyp(h[:-1], h[-1]); f.run()
                return f.loo_grad()
            res = scipy.optimize.minimize(fun, np.append(hyp, sig2n), jac=True, method="L-BFGS-B")
        """
        if objective not in ("loo", "press"):
            raise ValueError('loo_grad: objective is "loo" or "press"')
        v = C.c_double()
        g = np.empty(self.nhyp + 1)
        L.check(self._lib.sgpr_fit_loo_grad(self._h, L.LOO_PRESS if objective == "press" else L.LOO_LPD,
                                            C.cast(C.byref(v), L._dp), L.dptr(g), len(g)), "sgpr_fit_loo_grad")
        return v.value, g

    def nll_grad_terms(self):
        """[alpha^T dK_lx alpha, tr(Ky^-1 dK_lx), alpha^T dK_ly alpha, tr(Ky^-1 dK_ly), tr(Ky^-1)]: the
        pieces of Rasmussen (5.9) the per-example nll_grad variants recombine."""
        t = np.empty(5)
        L.check(self._lib.sgpr_fit_nll_grad_terms(self._h, L.dptr(t)), "sgpr_fit_nll_grad_terms")
        return t

    def eig(self):
        """-> (w, c): eigenvalues of Ky = K + |sig2n| I (ascending) and c = Q^T z, computed on the
        device (parallel Jacobi).  The failure path of the drivers' nll_chol: their
        `except: eigsh(Ky, neig, ...)` branch (02_pert_pendulum/func.py:194-203).  The handle has to
        be run() again before other queries."""
        w, c = np.empty(self.n), np.empty(self.n)
        rc = self._lib.sgpr_fit_eig(self._h, L.dptr(w), L.dptr(c))
        if rc > 0:
            raise np.linalg.LinAlgError("Jacobi eigen-solver did not converge")
        L.check(rc, "sgpr_fit_eig")
        return w, c

    def inverse(self):
        """Ky^-1 as an F-ordered host array (the drivers' scipy.linalg.inv(K + sig2n I))."""
        A = np.empty((self.n, self.n), order="F")
        L.check(self._lib.sgpr_fit_inverse(self._h, L.dptr(A), self.n), "sgpr_fit_inverse")
        return A

    def ldiag(self):
        out = np.empty(self.n)
        L.check(self._lib.sgpr_fit_ldiag(self._h, L.dptr(out)), "sgpr_fit_ldiag")
        return out

    def matrix(self):
        """The factor L (after factor()) or Ky (after build()), as an F-ordered host array."""
        A = np.empty((self.n, self.n), order="F")
        L.check(self._lib.sgpr_fit_get_matrix(self._h, L.dptr(A), self.n), "sgpr_fit_get_matrix")
        return A

    def solve_rhs(self, B):
        B = np.array(B, dtype=np.float64, order="F")
        nrhs = 1 if B.ndim == 1 else B.shape[1]
        if B.shape[0] != self.n:
            raise ValueError("B must have 2*n_pts rows")
        L.check(self._lib.sgpr_fit_solve_rhs(self._h, L.dptr(B), self.n, nrhs), "sgpr_fit_solve_rhs")
        return B

    def solve_rhs_dev(self, dptr, nrhs, ldb=None):
        """solve_rhs for right-hand sides that are already on the fit's device: `dptr` = device address (int) of an n x nrhs
        column-major block of doubles -- e.g. `t.data_ptr()` of a contiguous torch.float64 tensor of shape (nrhs, n) --,
        overwritten with the solution.  No host copies; returns when the solve has finished.

        The solve runs on the FIT'S OWN stream and is not ordered against the stream that produced the block: the caller makes
        sure B is complete on the device before the call (e.g. `torch.cuda.current_stream().synchronize()`, as bench.py does).
        The scratch of the block solves (~0.8 GB at n = 98 304) stays with the handle until `release_scratch()` or close."""
        L.check(self._lib.sgpr_fit_solve_rhs_dev(self._h, C.c_void_p(int(dptr)), self.n if ldb is None else int(ldb), int(nrhs)),
                "sgpr_fit_solve_rhs_dev")

    def release_scratch(self):
        """give the block solves' device scratch back (it is allocated again by the next solve_rhs that needs it)"""
        L.check(self._lib.sgpr_fit_trim(self._h), "sgpr_fit_trim")

    def solve_rhs_ms(self):
        """Device time (ms) of the last solve_rhs: the triangular solves without the host copies of B."""
        v = C.c_double()
        L.check(self._lib.sgpr_fit_solve_rhs_ms(self._h, C.cast(C.byref(v), L._dp)), "sgpr_fit_solve_rhs_ms")
        return v.value

    def predict_rows(self, q, P):
        q, P = L.f64(np.atleast_1d(q)), L.f64(np.atleast_1d(P))
        m = len(q)
        op, oq = np.empty(m), np.empty(m)
        L.check(self._lib.sgpr_fit_predict_rows(self._h, m, L.dptr(q), L.dptr(P), L.dptr(op), L.dptr(oq)),
                "sgpr_fit_predict_rows")
        return op, oq

    def cond_estimate(self, iters=30):
        """cond_2(Ky) from below: power iteration for lambda_max (Ky v through the prediction kernel), inverse iteration with
        the cached factor for lambda_min.  Returns dict(lambda_max, lambda_min, cond, last_change, iters).  Not part of the
        reference's call surface (it never computes a condition number); the parity tolerances are multiples of cond * eps."""
        o = np.zeros(4)
        L.check(self._lib.sgpr_fit_cond_estimate(self._h, int(iters), L.dptr(o)), "sgpr_fit_cond_estimate")
        return {"lambda_max": float(o[0]), "lambda_min": float(o[1]), "cond": float(o[2]), "last_change": float(o[3]),
                "iters": int(iters), "method": "power iteration on Ky v (rows re-evaluated by the prediction kernel) / inverse "
                                                "iteration with the cached factor; Rayleigh quotients: a lower bound of cond_2"}

    def stage_ms(self):
        b, f, s = C.c_double(), C.c_double(), C.c_double()
        c = lambda v: C.cast(C.byref(v), L._dp)
        L.check(self._lib.sgpr_fit_stage_ms(self._h, c(b), c(f), c(s)), "sgpr_fit_stage_ms")
        return b.value, f.value, s.value

    def device_ptrs(self):
        dA, lda, dal = C.c_void_p(), C.c_size_t(), C.c_void_p()
        L.check(self._lib.sgpr_fit_device_ptrs(self._h, C.byref(dA), C.byref(lda), C.byref(dal)))
        return dA.value, lda.value, dal.value


def batch_max_order():
    """largest matrix order per problem sgpr_fit_batch takes (256)"""
    return L.load_library().sgpr_fit_batch_max_order()


def _batch_inputs(name, x, y, z, hyp, sig2n, reg):
    """The inputs of the wrappers that take points as x | y: contiguous float64 (B, .) arrays, sig2n broadcast to (B,), the shapes
    checked (the ValueError names the wrapper).  -> (x, y, z, hyp, s2), B, n_pts, n, nhyp"""
    x, y, z, hyp = (np.ascontiguousarray(np.atleast_2d(np.asarray(v, dtype=np.float64))) for v in (x, y, z, hyp))
    B, n_pts = x.shape
    n = n_pts if reg else 2 * n_pts
    if y.shape != (B, n_pts) or z.shape != (B, n) or hyp.shape[0] != B:
        raise ValueError("%s: x, y (B, n_pts), z (B, n), hyp (B, nhyp)" % name)
    s2 = np.ascontiguousarray(np.broadcast_to(np.asarray(sig2n, dtype=np.float64), (B,)))
    return (x, y, z, hyp, s2), B, n_pts, n, hyp.shape[1]


def _batch_lead(family, arrays, B, n_pts, reg):
    """the arguments every x | y entry starts with: family, nbatch, n_pts, x, y, z, hyp, nhyp, sig2n, flags"""
    x, y, z, hyp, s2 = arrays
    return (L.family_id(family), B, n_pts, L.dptr(x), L.dptr(y), L.dptr(z), L.dptr(hyp), hyp.shape[1], L.dptr(s2),
            L.FIT_REG if reg else 0)


def _batch_run(entry, lead, B, n, want_alpha, extra=(), which=None):
    """Allocate alpha (B, n) or None, nll (B,), info (B,) and call entry(*lead [, which], alpha, nll, *extra, info)."""
    alpha = np.empty((B, n)) if want_alpha else None
    nll = np.empty(B)
    info = np.zeros(B, dtype=np.int32)
    args = list(lead) + ([] if which is None else [which]) + [L.dptr(alpha) if want_alpha else None, L.dptr(nll)]
    args += [L.dptr(e) for e in extra] + [info.ctypes.data_as(C.POINTER(C.c_int))]
    L.check(getattr(L.load_library(), entry)(*args), entry)
    return alpha, nll, info


def fit_batch(family, x, y, z, hyp, sig2n, reg=False, want_alpha=True):
    """Many small independent fits in ONE launch (one workgroup per problem): the body of nll_chol
    (python/functions/func.py:189-196; reg=True: nll_chol_reg) for every row b of
        x, y (B, n_pts);  z (B, n), n = 2 n_pts (n_pts with reg);  hyp (B, nhyp);  sig2n (B,) or scalar.
    -> (alpha (B, n) or None, nll (B,), info (B,)): info[b] > 0 where Ky_b is not positive definite
    (nll[b] is NaN there, like the LinAlgError scipy raises for that problem)."""
    arrays, B, n_pts, n, _ = _batch_inputs("fit_batch", x, y, z, hyp, sig2n, reg)
    alpha, nll, info = _batch_run("sgpr_fit_batch", _batch_lead(family, arrays, B, n_pts, reg), B, n, want_alpha)
    nll[info != 0] = np.nan
    return alpha, nll, info


def _pairs_inputs(name, family, X, z, hyp, sig2n):
    """The inputs of the wrappers for d canonical pairs per point: X (B, n_pts, 2d) or (n_pts, 2d) and z (B, n) or (n,) broadcast
    over the rows of hyp, sig2n to (B,), the shapes checked (the ValueError names the wrapper), X in the library's layout.
    -> lead (the arguments every d-pair entry starts with), the arrays behind its pointers, B, n, nhyp"""
    X = np.asarray(X, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    hyp = np.asarray(hyp, dtype=np.float64)
    if hyp.ndim != 2:
        raise ValueError("%s: hyp (B, nhyp)" % name)
    B = hyp.shape[0]
    if X.ndim == 2:
        X = np.broadcast_to(X, (B,) + X.shape)
    if X.ndim != 3 or X.shape[0] != B or X.shape[2] % 2 or X.shape[2] == 0:
        raise ValueError("%s: X (B, n_pts, 2d) or (n_pts, 2d), B the rows of hyp" % name)
    n_pts, D = X.shape[1], X.shape[2]
    n = D * n_pts
    if z.ndim == 1:
        z = np.broadcast_to(z, (B,) + z.shape)
    if z.shape != (B, n):
        raise ValueError("%s: z (B, n) or (n,), n = 2 d n_pts" % name)
    if np.ndim(sig2n) > 1 or (np.ndim(sig2n) == 1 and np.shape(sig2n) != (B,)):
        raise ValueError("%s: sig2n scalar or (B,)" % name)
    # the library's layout: coordinate m of point i of problem b at (b 2d + m) n_pts + i
    Xl = np.ascontiguousarray(np.swapaxes(X, 1, 2))
    z = np.ascontiguousarray(z)
    hyp = np.ascontiguousarray(hyp)
    s2 = np.ascontiguousarray(np.broadcast_to(np.asarray(sig2n, dtype=np.float64), (B,)))
    lead = (L.family_id(family), D // 2, B, n_pts, L.dptr(Xl), L.dptr(z), L.dptr(hyp), hyp.shape[1], L.dptr(s2), 0)
    return lead, (Xl, z, hyp, s2), B, n, hyp.shape[1]


def fit_batch_pairs(family, X, z, hyp, sig2n, want_alpha=True):
    """fit_batch for problems with d canonical pairs per point (SympFit.pairs' kernels and layouts), every order
    n = 2 d n_pts up to batch_max_order(): one launch up to order 256, the mid path above it.
        X (B, n_pts, 2d), columns (q_1..q_d, P_1..P_d) -- or (n_pts, 2d), broadcast over the rows of hyp: one data set,
        a population of hyper-parameters;  z (B, n) or (n,), block by block like the rows of K;
        hyp (B, nhyp), rows as SympFit.pairs takes them;  sig2n (B,) or scalar.
    -> (alpha (B, n) or None, nll (B,), info (B,)): info[b] > 0 where Ky_b is not positive definite (nll[b] is NaN there)."""
    lead, _keep, B, n, _ = _pairs_inputs("fit_batch_pairs", family, X, z, hyp, sig2n)
    alpha, nll, info = _batch_run("sgpr_fit_batch_nd", lead, B, n, want_alpha)
    nll[info != 0] = np.nan
    return alpha, nll, info


def fit_batch_pairs_grad(family, X, z, hyp, sig2n, want_alpha=False):
    """fit_batch_pairs plus the exact gradient of every problem's nll in (hyp, sig2n), every order up to batch_max_order() on the
    device (sgpr_fit_batch_nd_grad): one launch up to order 256, the mid path with its gradient phase above.  Shapes and
    broadcasting as fit_batch_pairs.
    -> (alpha (B, n) or None, nll (B,), grad (B, nhyp + 1), info (B,)).  Row b of grad is (d/dlq_1..d/dlq_d, d/dlP_1..d/dlP_d,
    [d/dp_1..d/dp_d,] d/dsig, d/dsig2n), SympFit.pairs(...).nll_grad_full()'s order; Ky holds |sig2n[b]|, so the last entry carries
    sign(sig2n[b]) (sign(0) = +1).  Rows with info > 0 are NaN (nll and the whole gradient row).  nll, alpha and info are the same
    bits fit_batch_pairs returns; a row's gradient bits do not depend on the batch."""
    lead, _keep, B, n, nhyp = _pairs_inputs("fit_batch_pairs_grad", family, X, z, hyp, sig2n)
    grad = np.empty((B, nhyp + 1))
    alpha, nll, info = _batch_run("sgpr_fit_batch_nd_grad", lead, B, n, want_alpha, (grad,))
    bad = info != 0
    nll[bad] = np.nan
    grad[bad] = np.nan
    return alpha, nll, grad, info


def fit_batch_pairs_loo(family, X, z, hyp, sig2n, want_alpha=False):
    """fit_batch_pairs plus leave-one-point-out cross-validation of every problem (SympFit.pairs(...).loo()'s definitions: a point
    owns its 2d rows), every order up to batch_max_order() on the device (sgpr_fit_batch_nd_loo): one launch up to order 256, the
    mid path with its loo phase above.  Shapes and broadcasting as fit_batch_pairs.
    -> (alpha (B, n) or None, nll (B,), loo (B, 2), info (B,)).  Row b of loo is (loo, press).  Rows with info > 0 are NaN (nll and
    the loo row).  nll, alpha and info are the same bits fit_batch_pairs returns; a row's loo bits do not depend on the batch."""
    lead, _keep, B, n, _ = _pairs_inputs("fit_batch_pairs_loo", family, X, z, hyp, sig2n)
    loo = np.empty((B, 2))
    alpha, nll, info = _batch_run("sgpr_fit_batch_nd_loo", lead, B, n, want_alpha, (loo,))
    bad = info != 0
    nll[bad] = np.nan
    loo[bad] = np.nan
    return alpha, nll, loo, info


def fit_batch_pairs_loo_grad(family, X, z, hyp, sig2n, objective="loo", want_alpha=False):
    """fit_batch_pairs plus one leave-one-point-out objective of every problem and its exact gradient in (hyp, sig2n):
    objective="loo" (minus the summed log predictive densities) or "press" (the summed squared residuals),
    SympFit.pairs(...).loo_grad's definitions.  Shapes and broadcasting as fit_batch_pairs.
    -> (alpha (B, n) or None, nll (B,), value (B,), grad (B, nhyp + 1), info (B,)).  Row b of grad is in fit_batch_pairs_grad's
    order; Ky holds |sig2n[b]|, so the last entry carries sign(sig2n[b]) (sign(0) = +1).  Rows with info > 0 are NaN (nll, value and
    the whole gradient row).  nll, alpha and info are the same bits fit_batch_pairs returns, value the bits of
    fit_batch_pairs_loo's column.
    n <= 256: ONE launch (sgpr_fit_batch_nd_loo_grad), one workgroup per problem.
    256 < n <= 2048 (the slow path): nll, alpha, info and value from one fit_batch_pairs_loo call, and the gradient of every
    positive-definite row from SympFit.pairs(...).run().loo_grad(objective), one device-resident fit per row.  Every gradient of
    that range on the device: fit_batch_pairs_loo_grad_mid."""
    if objective not in ("loo", "press"):
        raise ValueError('fit_batch_pairs_loo_grad: objective is "loo" or "press"')
    which = L.LOO_PRESS if objective == "press" else L.LOO_LPD
    lead, keep, B, n, nhyp = _pairs_inputs("fit_batch_pairs_loo_grad", family, X, z, hyp, sig2n)
    if n > batch_grad_max_order():
        Xl, zl, hl, s2 = keep
        alpha, nll, loo, info = fit_batch_pairs_loo(family, np.swapaxes(Xl, 1, 2), zl, hl, s2, want_alpha=want_alpha)
        grad = np.full((B, nhyp + 1), np.nan)
        for b in np.flatnonzero(info == 0):
            with SympFit.pairs(family, Xl[b].T, zl[b], hl[b], s2[b]) as f:
                grad[b] = f.run().loo_grad(objective)[1]
        return alpha, nll, loo[:, which].copy(), grad, info
    value = np.empty(B)
    grad = np.empty((B, nhyp + 1))
    alpha, nll, info = _batch_run("sgpr_fit_batch_nd_loo_grad", lead, B, n, want_alpha, (value, grad), which)
    bad = info != 0
    nll[bad] = np.nan
    value[bad] = np.nan
    grad[bad] = np.nan
    return alpha, nll, value, grad, info


def fit_batch_pairs_loo_grad_mid(family, X, z, hyp, sig2n, objective="loo", want_alpha=False):
    """fit_batch_pairs_loo_grad for 256 < n <= batch_max_order(), every gradient on the device (sgpr_fit_batch_nd_loo_grad_mid): shapes,
    broadcasting, the returned (alpha or None, nll, value, grad, info) and the NaN rows for info > 0 as fit_batch_pairs_loo_grad; nll,
    alpha and info are the bits fit_batch_pairs returns, value the bits of fit_batch_pairs_loo's column.  Per chunk of problems, behind
    the mid path's Ky^-1 stage: one thread per point, M = Ky^-1 W~ Ky^-1 on the matrix cores, one contraction launch.  ValueError for
    n <= 256: fit_batch_pairs_loo_grad serves that range in one launch."""
    if objective not in ("loo", "press"):
        raise ValueError('fit_batch_pairs_loo_grad_mid: objective is "loo" or "press"')
    which = L.LOO_PRESS if objective == "press" else L.LOO_LPD
    lead, _keep, B, n, nhyp = _pairs_inputs("fit_batch_pairs_loo_grad_mid", family, X, z, hyp, sig2n)
    if n <= batch_grad_max_order():
        raise ValueError("fit_batch_pairs_loo_grad_mid: order %d <= %d is fit_batch_pairs_loo_grad's range" % (n, batch_grad_max_order()))
    value = np.empty(B)
    grad = np.empty((B, nhyp + 1))
    alpha, nll, info = _batch_run("sgpr_fit_batch_nd_loo_grad_mid", lead, B, n, want_alpha, (value, grad), which)
    bad = info != 0
    nll[bad] = np.nan
    value[bad] = np.nan
    grad[bad] = np.nan
    return alpha, nll, value, grad, info


def batch_grad_max_order():
    """largest matrix order per problem sgpr_fit_batch_grad takes on the device (256)"""
    return 256


def fit_batch_grad(family, x, y, z, hyp, sig2n, reg=False, want_alpha=False):
    """fit_batch plus the exact gradient of every problem's nll in (hyp, sig2n).  Shapes as fit_batch:
        x, y (B, n_pts);  z (B, n), n = 2 n_pts (n_pts with reg);  hyp (B, nhyp);  sig2n (B,) or scalar.
    -> (alpha (B, n) or None, nll (B,), grad (B, nhyp + 1), info (B,)).  Row b of grad is (d/dhyp_0 .. d/dhyp_{nhyp-1},
    d/dsig2n); Ky holds |sig2n[b]|, so the last entry carries sign(sig2n[b]) (sign(0) = +1).  Rows with info > 0 are NaN
    (nll and the whole gradient row).  nll, alpha and info are the same bits fit_batch returns.
    n <= 256: ONE launch (sgpr_fit_batch_grad), one workgroup per problem.
    256 < n <= 2048 (the slow path): nll, alpha and info from one fit_batch call, and the gradient of every positive-definite
    row from SympFit(...).run().nll_grad_full(), one device-resident fit per row."""
    arrays, B, n_pts, n, nhyp = _batch_inputs("fit_batch_grad", x, y, z, hyp, sig2n, reg)
    x, y, z, hyp, s2 = arrays
    if n > batch_grad_max_order():
        alpha, nll, info = fit_batch(family, x, y, z, hyp, s2, reg=reg, want_alpha=want_alpha)
        grad = np.full((B, nhyp + 1), np.nan)
        for b in np.flatnonzero(info == 0):
            with SympFit(family, x[b], y[b], z[b], hyp[b], s2[b], reg=reg) as f:
                grad[b] = f.run().nll_grad_full()
        return alpha, nll, grad, info
    grad = np.empty((B, nhyp + 1))
    alpha, nll, info = _batch_run("sgpr_fit_batch_grad", _batch_lead(family, arrays, B, n_pts, reg), B, n, want_alpha, (grad,))
    return alpha, nll, grad, info


def batch_grad_mid_max_order():
    """largest matrix order per problem sgpr_fit_batch_grad_mid takes (sgpr_fit_batch_max_order(): 2048)"""
    return L.load_library().sgpr_fit_batch_max_order()


def fit_batch_grad_mid(family, x, y, z, hyp, sig2n, reg=False, want_alpha=False):
    """fit_batch_grad for 256 < n <= batch_grad_mid_max_order(), every gradient on the device (sgpr_fit_batch_grad_mid): shapes,
    the returned (alpha or None, nll, grad, info) and the NaN rows for info > 0 as fit_batch_grad; nll, alpha and info are the
    bits fit_batch returns.  Per chunk of problems: L^-T from the leaf inverses by block doubling, Ky^-1 = L^-T L^-1 on the
    matrix cores, one contraction launch.  ValueError for n <= 256: fit_batch_grad serves that range in one launch."""
    arrays, B, n_pts, n, nhyp = _batch_inputs("fit_batch_grad_mid", x, y, z, hyp, sig2n, reg)
    if n <= batch_grad_max_order():
        raise ValueError("fit_batch_grad_mid: order %d <= %d is fit_batch_grad's range" % (n, batch_grad_max_order()))
    grad = np.empty((B, nhyp + 1))
    alpha, nll, info = _batch_run("sgpr_fit_batch_grad_mid", _batch_lead(family, arrays, B, n_pts, reg), B, n, want_alpha, (grad,))
    return alpha, nll, grad, info


def fit_batch_loo(family, x, y, z, hyp, sig2n, reg=False, want_alpha=False):
    """fit_batch plus leave-one-point-out cross-validation of every problem (SympFit.loo's definitions, D = 2; 1 with reg), for
    every order up to batch_max_order().  Shapes as fit_batch:
        x, y (B, n_pts);  z (B, n), n = 2 n_pts (n_pts with reg);  hyp (B, nhyp);  sig2n (B,) or scalar.
    -> (alpha (B, n) or None, nll (B,), loo (B, 2), info (B,)).  Row b of loo is (loo, press).  Rows with info > 0 are NaN (nll
    and the loo row).  nll, alpha and info are the same bits fit_batch returns; a row's loo bits do not depend on the batch."""
    arrays, B, n_pts, n, _ = _batch_inputs("fit_batch_loo", x, y, z, hyp, sig2n, reg)
    loo = np.empty((B, 2))
    alpha, nll, info = _batch_run("sgpr_fit_batch_loo", _batch_lead(family, arrays, B, n_pts, reg), B, n, want_alpha, (loo,))
    return alpha, nll, loo, info


def fit_batch_loo_grad(family, x, y, z, hyp, sig2n, reg=False, objective="loo", want_alpha=False):
    """fit_batch plus one leave-one-point-out objective of every problem and its exact gradient in (hyp, sig2n): objective="loo"
    (minus the summed log predictive densities) or "press" (the summed squared residuals), SympFit.loo_grad's definitions.
    Shapes as fit_batch:
        x, y (B, n_pts);  z (B, n), n = 2 n_pts (n_pts with reg);  hyp (B, nhyp);  sig2n (B,) or scalar.
    -> (alpha (B, n) or None, nll (B,), value (B,), grad (B, nhyp + 1), info (B,)).  Row b of grad is (d/dhyp_0 ..
    d/dhyp_{nhyp-1}, d/dsig2n) of value[b]; Ky holds |sig2n[b]|, so the last entry carries sign(sig2n[b]) (sign(0) = +1).  Rows
    with info > 0 are NaN (nll, value and the whole gradient row).  nll, alpha and info are the same bits fit_batch returns,
    value the bits of fit_batch_loo's column.
    n <= 256: ONE launch (sgpr_fit_batch_loo_grad), one workgroup per problem.
    256 < n <= 2048 (the slow path): nll, alpha, info and value from one fit_batch_loo call, and the gradient of every
    positive-definite row from SympFit(...).run().loo_grad(objective), one device-resident fit per row.  Every gradient of that
    range on the device: fit_batch_loo_grad_mid."""
    if objective not in ("loo", "press"):
        raise ValueError('fit_batch_loo_grad: objective is "loo" or "press"')
    which = L.LOO_PRESS if objective == "press" else L.LOO_LPD
    arrays, B, n_pts, n, nhyp = _batch_inputs("fit_batch_loo_grad", x, y, z, hyp, sig2n, reg)
    x, y, z, hyp, s2 = arrays
    if n > batch_grad_max_order():
        alpha, nll, loo, info = fit_batch_loo(family, x, y, z, hyp, s2, reg=reg, want_alpha=want_alpha)
        grad = np.full((B, nhyp + 1), np.nan)
        for b in np.flatnonzero(info == 0):
            with SympFit(family, x[b], y[b], z[b], hyp[b], s2[b], reg=reg) as f:
                grad[b] = f.run().loo_grad(objective)[1]
        return alpha, nll, loo[:, which].copy(), grad, info
    value = np.empty(B)
    grad = np.empty((B, nhyp + 1))
    alpha, nll, info = _batch_run("sgpr_fit_batch_loo_grad", _batch_lead(family, arrays, B, n_pts, reg), B, n, want_alpha,
                                  (value, grad), which)
    return alpha, nll, value, grad, info


def fit_batch_loo_grad_mid(family, x, y, z, hyp, sig2n, reg=False, objective="loo", want_alpha=False):
    """fit_batch_loo_grad for 256 < n <= batch_grad_mid_max_order(), every gradient on the device (sgpr_fit_batch_loo_grad_mid): shapes,
    the returned (alpha or None, nll, value, grad, info) and the NaN rows for info > 0 as fit_batch_loo_grad; nll, alpha and info are
    the bits fit_batch returns, value the bits of fit_batch_loo's column.  Per chunk of problems, behind fit_batch_grad_mid's Ky^-1
    stage: one thread per point, M = Ky^-1 W~ Ky^-1 on the matrix cores, one contraction launch.  ValueError for n <= 256:
    fit_batch_loo_grad serves that range in one launch."""
    if objective not in ("loo", "press"):
        raise ValueError('fit_batch_loo_grad_mid: objective is "loo" or "press"')
    which = L.LOO_PRESS if objective == "press" else L.LOO_LPD
    arrays, B, n_pts, n, nhyp = _batch_inputs("fit_batch_loo_grad_mid", x, y, z, hyp, sig2n, reg)
    if n <= batch_grad_max_order():
        raise ValueError("fit_batch_loo_grad_mid: order %d <= %d is fit_batch_loo_grad's range" % (n, batch_grad_max_order()))
    value = np.empty(B)
    grad = np.empty((B, nhyp + 1))
    alpha, nll, info = _batch_run("sgpr_fit_batch_loo_grad_mid", _batch_lead(family, arrays, B, n_pts, reg), B, n, want_alpha,
                                  (value, grad), which)
    return alpha, nll, value, grad, info
