"""Mirror of the reference's GP library python/functions/func.py -- same names, positional
order, in-place semantics and error behaviour -- with the hot path on the MI355X.

    reference                               here
    ------------------------------------    -----------------------------------------------
    sympgpr.build_k / buildkreg (f2py)      sgpr_build_k_host / sgpr_buildkreg_host
    scipy.linalg.cholesky(lower=True)       sgpr_potrf_host          (LinAlgError if not PD)
    solve_triangular x 2                    sgpr_potrs_host
    nll_chol / nll_chol_reg                 one device-resident sgpr_fit_* pass (K stays in HBM)
    guessP / calcQ / calcP / applymap       K* rows . alpha on the device, alpha cached

Select the kernel family (which kernels*.f90 the reference would have compiled) with
`set_family("A"|"B"|"C"|"D")`; default "A" (python/05_tokamak/SympGPR/kernels.f90).
build_dK / build_dKreg / nll_grad / nll_grad_reg are available for the product kernels (A, C, D).
"""
import numpy as np

from . import kernels as _kernels
from .fit import SympFit
from .fortran.sympgpr import sympgpr
from .kernels import *  # noqa: F401,F403  (kern_num, d2kdxdx0_num, ... like `from kernels import *`, func.py:15)
from . import ops as _ops
from .ops import cholesky as _cholesky
from .ops import get_family, set_family, solve_cholesky as _solve_cholesky  # noqa: F401
from .predict import Predictor, solve_implicit_P


_SMALL_ORDER = 256      # sgpr_fit_batch_max_order(): up to here one objective call is one single-workgroup launch


def _l(l):
    return tuple(float(v) for v in l)


def f_kern(x, y, x0, y0, l):            # functions/func.py:17-18
    return _kernels.kern_num(x, y, x0, y0, *_l(l))


def d2kdxdx0(x, y, x0, y0, l):          # :20-21
    return _kernels.d2kdxdx0_num(x, y, x0, y0, *_l(l))


def d2kdydy0(x, y, x0, y0, l):          # :23-24
    return _kernels.d2kdydy0_num(x, y, x0, y0, *_l(l))


def d2kdxdy0(x, y, x0, y0, l):          # :26-27
    return _kernels.d2kdxdy0_num(x, y, x0, y0, *_l(l))


def d2kdydx0(x, y, x0, y0, l):          # :29-30
    return d2kdxdy0(x, y, x0, y0, l)


def build_K(xin, x0in, hyp, K):
    """functions/func.py:32-40: covariance with derivative observations, Eq. (38); K in place."""
    N = K.shape[0] // 2
    N0 = K.shape[1] // 2
    x0 = x0in[0:N0]
    x = xin[0:N]
    y0 = x0in[N0:2 * N0]
    y = xin[N:2 * N]
    sympgpr.build_k(x, y, x0, y0, hyp, K)


def buildKreg(xin, x0in, hyp, K):
    """functions/func.py:42-50: scalar-kernel covariance on the regular (q,p) grid; K in place."""
    N = K.shape[0]
    N0 = K.shape[1]
    x0 = x0in[0:N0]
    x = xin[0:N]
    y0 = x0in[N0:2 * N0]
    y = xin[N:2 * N]
    sympgpr.buildkreg(x, y, x0, y0, hyp, K)


def gpsolve(Ky, ft):
    """functions/func.py:165-171 -> (L, alpha)."""
    Lf = _cholesky(Ky, lower=True)
    return Lf, _solve_cholesky(Lf, ft)


def solve_cholesky(L, b):
    """functions/func.py:174-177."""
    return _solve_cholesky(L, b)


def _nll_small(hyp, x, y, N, reg):
    """One objective value at the drivers' own sizes (matrix order <= 256): the whole body runs in ONE launch of
    one workgroup (sgpr_fit_batch with a batch of one) -- a device-resident handle costs five launches, an
    allocation per buffer and 230-390 us at these orders, more than the reference's CPU path needs at order 80."""
    from .fit import fit_batch
    npts = N if reg else N // 2
    _, nll, info = fit_batch(get_family(), x[None, 0:npts], x[None, npts:2 * npts], y[None, :N if reg else 2 * npts],
                             hyp[None, :-1], np.abs(hyp[-1:]), reg=reg, want_alpha=False)
    if info[0]:
        raise np.linalg.LinAlgError("%d-th leading minor of the array is not positive definite" % int(info[0]))
    return float(nll[0])


def nll_chol_reg(hyp, x, y, N):
    """functions/func.py:180-187: negative log-posterior of the scalar-kernel GP.  N = matrix
    order; x holds (q || p) and is sliced exactly as buildKreg does."""
    hyp = np.asarray(hyp, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if 0 < N <= _SMALL_ORDER:
        return _nll_small(hyp, x, y, N, True)
    with SympFit(get_family(), x[0:N], x[N:2 * N], y[:N], hyp[:-1],
                 np.abs(hyp[-1]), reg=True) as f:
        return f.run().nll()


def nll_chol(hyp, x, y, N):
    """functions/func.py:189-196: negative log-posterior of the symplectic GP.  N = matrix order
    (twice the number of points build_K slices out of x)."""
    hyp = np.asarray(hyp, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if 0 < N <= _SMALL_ORDER and N % 2 == 0:
        return _nll_small(hyp, x, y, N, False)
    npts = N // 2
    with SympFit(get_family(), x[0:npts], x[npts:2 * npts], y[:2 * npts],
                 hyp[:-1], np.abs(hyp[-1])) as f:
        return f.run().nll()


def nll_chol_batch(hyps, x, y, N, reg=False):
    """nll_chol (reg=True: nll_chol_reg) for a whole POPULATION of hyper-parameter vectors over the same
    data in one launch: what a CMA-ES generation costs the Split_SympGPR driver one call at a time
    (python/05_tokamak/Split_SympGPR/main.py:36-41,63-66: `cma.fmin(nll_transform, ...)`).
    hyps (B, nhyp + 1) rows like nll_chol's hyp (the last entry is sig2_n); N = matrix order, at most
    fit.batch_max_order() (larger orders: loop over nll_chol).  Rows whose Ky is not positive
    definite come back as +inf (an optimiser's usual penalty for an exception)."""
    from .fit import batch_max_order, fit_batch
    hyps = np.atleast_2d(np.asarray(hyps, dtype=np.float64))
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if N > batch_max_order():
        f = nll_chol_reg if reg else nll_chol
        out = np.empty(len(hyps))
        for b, h in enumerate(hyps):
            try:
                out[b] = f(h, x, y, N)
            except np.linalg.LinAlgError:
                out[b] = np.inf
        return out
    npts = N if reg else N // 2
    B = len(hyps)
    X = np.broadcast_to(x[0:npts], (B, npts))
    Y = np.broadcast_to(x[npts:2 * npts], (B, npts))
    Z = np.broadcast_to(y[:N if reg else 2 * npts], (B, N if reg else 2 * npts))
    _, nll, info = fit_batch(get_family(), X, Y, Z, hyps[:, :-1], np.abs(hyps[:, -1]), reg=reg, want_alpha=False)
    nll[info != 0] = np.inf
    return nll


def _pairs_check(name, hyps, X, z):
    """hyps (B, nhyp + 1), X (n_pts, 2d), z (n,) as float64 arrays, the shapes checked -> hyps, X, z, n"""
    hyps = np.atleast_2d(np.asarray(hyps, dtype=np.float64))
    X = np.asarray(X, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] % 2 or X.shape[1] == 0:
        raise ValueError("%s: X must be (n_pts, 2d)" % name)
    n = X.shape[0] * X.shape[1]
    if z.shape != (n,):
        raise ValueError("%s: z must have length %d" % (name, n))
    if hyps.ndim != 2 or hyps.shape[1] < 2:
        raise ValueError("%s: rows (lq.., lP.., [p..,] sig, sig2_n)" % name)
    return hyps, X, z, n


def nll_chol_pairs_batch(hyps, X, z):
    """nll_chol_batch for a fit with d canonical pairs per point: the negative log-posterior of SympFit.pairs(family, X, z, ...)
    for a whole POPULATION of hyper-parameter vectors over one data set.  X (n_pts, 2d), columns (q_1..q_d, P_1..P_d); z the
    2 d n_pts targets, block by block; hyps (B, nhyp + 1), rows (lq_1..lq_d, lP_1..lP_d, [p_1..p_d,] sig, sig2_n) -- the
    d-pair counterpart of nll_chol's hyp.  Up to order fit.batch_max_order() (2048) one batched call (fit.fit_batch_pairs);
    above it a loop over ONE device-resident handle (set_hyp / run).  Rows whose Ky is not positive definite come back
    as +inf."""
    from .fit import batch_max_order, fit_batch_pairs
    hyps, X, z, n = _pairs_check("nll_chol_pairs", hyps, X, z)
    if n <= batch_max_order():
        _, nll, info = fit_batch_pairs(get_family(), X, z, hyps[:, :-1], np.abs(hyps[:, -1]), want_alpha=False)
        nll[info != 0] = np.inf
        return nll
    out = np.empty(len(hyps))
    if len(hyps) == 0:
        return out
    with SympFit.pairs(get_family(), X, z, hyps[0, :-1], np.abs(hyps[0, -1])) as f:
        for b, h in enumerate(hyps):
            try:
                f.set_hyp(h[:-1], np.abs(h[-1]))
                out[b] = f.run().nll()
            except np.linalg.LinAlgError:
                out[b] = np.inf
    return out


def nll_chol_pairs(hyp, X, z):
    """nll_chol for a fit with d canonical pairs per point: one row of nll_chol_pairs_batch (+inf where Ky is not positive
    definite) -- the objective of an optimiser over (lq.., lP.., [p..,] sig, sig2_n)."""
    hyp = np.asarray(hyp, dtype=np.float64)
    if hyp.ndim != 1:
        raise ValueError("nll_chol_pairs: hyp is one row (lq.., lP.., [p..,] sig, sig2_n)")
    return float(nll_chol_pairs_batch(hyp[None], X, z)[0])


def nll_chol_pairs_grad_batch(hyps, X, z):
    """nll_chol_pairs_batch with gradients: hyps (B, nhyp + 1), rows (lq_1..lq_d, lP_1..lP_d, [p_1..p_d,] sig, sig2_n) ->
    (nlls (B,), grads (B, nhyp + 1)), grads[b, k] = d nll[b] / d hyps[b, k].  The noise enters as |hyps[b, -1]|, so the last column
    carries its sign (sign(0) = +1).  Rows whose Ky is not positive definite give nll = +inf and a NaN gradient row.  Up to order
    fit.batch_max_order() (2048) one batched call (fit.fit_batch_pairs_grad); above it a loop over ONE device-resident handle
    (set_hyp / run / nll_grad_full)."""
    from .fit import batch_max_order, fit_batch_pairs_grad
    hyps, X, z, n = _pairs_check("nll_chol_pairs_grad", hyps, X, z)
    sign = np.where(hyps[:, -1] < 0.0, -1.0, 1.0)
    if n <= batch_max_order():
        _, nll, grad, info = fit_batch_pairs_grad(get_family(), X, z, hyps[:, :-1], np.abs(hyps[:, -1]), want_alpha=False)
        bad = info != 0
        nll[bad] = np.inf
        grad[bad] = np.nan
        grad[:, -1] *= sign
        return nll, grad
    nll = np.empty(len(hyps))
    grad = np.full(hyps.shape, np.nan)
    if len(hyps) == 0:
        return nll, grad
    with SympFit.pairs(get_family(), X, z, hyps[0, :-1], np.abs(hyps[0, -1])) as f:
        for b, h in enumerate(hyps):
            try:
                f.set_hyp(h[:-1], np.abs(h[-1]))
                nll[b] = f.run().nll()
                grad[b] = f.nll_grad_full()
                grad[b, -1] *= sign[b]
            except np.linalg.LinAlgError:
                nll[b] = np.inf
                grad[b] = np.nan
    return nll, grad


def nll_chol_pairs_grad(hyp, X, z):
    """nll_chol_pairs and its exact gradient -> (nll, grad), grad[k] = d nll / d hyp[k] for every entry of hyp = (lq.., lP..,
    [p..,] sig, sig2_n): the objective for scipy.optimize.minimize(..., jac=True) on a fit with d canonical pairs per point.
    One row of nll_chol_pairs_grad_batch; raises LinAlgError where Ky is not positive definite, as nll_chol_grad does."""
    hyp = np.asarray(hyp, dtype=np.float64)
    if hyp.ndim != 1:
        raise ValueError("nll_chol_pairs_grad: hyp is one row (lq.., lP.., [p..,] sig, sig2_n)")
    nll, grad = nll_chol_pairs_grad_batch(hyp[None], X, z)
    if nll[0] == np.inf:
        raise np.linalg.LinAlgError("a leading minor of Ky is not positive definite")
    return float(nll[0]), grad[0]


def loo_chol_pairs_batch(hyps, X, z):
    """loo_chol_batch for a fit with d canonical pairs per point: the leave-one-point-out objective (minus the summed log predictive
    densities of each point's 2d rows given all other points, SympFit.pairs(...).loo()) for a whole population of hyper-parameter
    vectors over one data set.  Arguments as nll_chol_pairs_batch.  Rows whose Ky is not positive definite come back as NaN, as in
    loo_chol_batch.  Up to order fit.batch_max_order() (2048) one batched call (fit.fit_batch_pairs_loo); above it a loop over ONE
    device-resident handle (set_hyp / run / loo)."""
    from .fit import batch_max_order, fit_batch_pairs_loo
    hyps, X, z, n = _pairs_check("loo_chol_pairs", hyps, X, z)
    if n <= batch_max_order():
        _, _, loo, info = fit_batch_pairs_loo(get_family(), X, z, hyps[:, :-1], np.abs(hyps[:, -1]))
        out = loo[:, 0].copy()
        out[info != 0] = np.nan
        return out
    out = np.empty(len(hyps))
    if len(hyps) == 0:
        return out
    with SympFit.pairs(get_family(), X, z, hyps[0, :-1], np.abs(hyps[0, -1])) as f:
        for b, h in enumerate(hyps):
            try:
                f.set_hyp(h[:-1], np.abs(h[-1]))
                out[b] = f.run().loo(resid=False, lpd=False)["loo"]
            except np.linalg.LinAlgError:
                out[b] = np.nan
    return out


def loo_chol_pairs(hyp, X, z):
    """loo_chol for a fit with d canonical pairs per point: one row of loo_chol_pairs_batch -- the cross-validation objective of
    an optimiser over (lq.., lP.., [p..,] sig, sig2_n).  Raises LinAlgError where Ky is not positive definite, as loo_chol does."""
    from .fit import batch_max_order, fit_batch_pairs_loo
    hyp = np.asarray(hyp, dtype=np.float64)
    if hyp.ndim != 1:
        raise ValueError("loo_chol_pairs: hyp is one row (lq.., lP.., [p..,] sig, sig2_n)")
    hyps, X, z, n = _pairs_check("loo_chol_pairs", hyp[None], X, z)
    if n <= batch_max_order():
        _, _, loo, info = fit_batch_pairs_loo(get_family(), X, z, hyps[:, :-1], np.abs(hyps[:, -1]))
        if info[0]:
            raise np.linalg.LinAlgError("%d-th leading minor of the array is not positive definite" % int(info[0]))
        return float(loo[0, 0])
    with SympFit.pairs(get_family(), X, z, hyp[:-1], np.abs(hyp[-1])) as f:
        return f.run().loo(resid=False, lpd=False)["loo"]


def loo_chol_pairs_grad_batch(hyps, X, z, objective="loo", mid=None):
    """loo_chol_pairs_batch with gradients: hyps (B, nhyp + 1), rows (lq_1..lq_d, lP_1..lP_d, [p_1..p_d,] sig, sig2_n) -> (value
    (B,), grad (B, nhyp + 1)), grad[b, k] = d value[b] / d hyps[b, k].  objective="press": the sum of squared leave-one-point-out
    residuals instead.  The noise enters as |hyps[b, -1]|, so the last column carries its sign (sign(0) = +1).  Rows whose Ky is not
    positive definite give NaN in the value and the whole gradient row, as in loo_chol_grad_batch.  Up to order 256 one launch
    (fit.fit_batch_pairs_loo_grad); up to fit.batch_max_order() (2048) the values from one batched call and the gradients row by
    row (that wrapper's slow path); above it a loop over ONE device-resident handle (set_hyp / run / loo_grad).
    mid="device": orders 256 < n <= 2048 go through fit.fit_batch_pairs_loo_grad_mid instead, every gradient on the device in a few
    launches per chunk, with the same conventions (the gradients agree with the slow path to rounding, not bit for bit).  mid=None
    (the default) is the behaviour described first."""
    from .fit import batch_grad_max_order, batch_max_order, fit_batch_pairs_loo_grad, fit_batch_pairs_loo_grad_mid
    if objective not in ("loo", "press"):
        raise ValueError('loo_chol_pairs_grad: objective is "loo" or "press"')
    if mid not in (None, "device"):
        raise ValueError('loo_chol_pairs_grad_batch: mid is None or "device"')
    hyps, X, z, n = _pairs_check("loo_chol_pairs_grad", hyps, X, z)
    sign = np.where(hyps[:, -1] < 0.0, -1.0, 1.0)
    if n <= batch_max_order():
        fn = fit_batch_pairs_loo_grad_mid if mid == "device" and n > batch_grad_max_order() else fit_batch_pairs_loo_grad
        _, _, value, grad, info = fn(get_family(), X, z, hyps[:, :-1], np.abs(hyps[:, -1]), objective=objective)
        bad = info != 0
        value[bad] = np.nan
        grad[bad] = np.nan
        grad[:, -1] *= sign
        return value, grad
    value = np.full(len(hyps), np.nan)
    grad = np.full(hyps.shape, np.nan)
    if len(hyps) == 0:
        return value, grad
    with SympFit.pairs(get_family(), X, z, hyps[0, :-1], np.abs(hyps[0, -1])) as f:
        for b, h in enumerate(hyps):
            try:
                f.set_hyp(h[:-1], np.abs(h[-1]))
                value[b], grad[b] = f.run().loo_grad(objective)
                grad[b, -1] *= sign[b]
            except np.linalg.LinAlgError:
                value[b] = np.nan
                grad[b] = np.nan
    return value, grad


def loo_chol_pairs_grad(hyp, X, z, objective="loo"):
    """loo_chol_pairs and its exact gradient -> (value, grad), grad[k] = d value / d hyp[k] for every entry of hyp = (lq.., lP..,
    [p..,] sig, sig2_n): the objective for scipy.optimize.minimize(..., jac=True) on the cross-validation objective of a fit with
    d canonical pairs per point.  One row of loo_chol_pairs_grad_batch; raises LinAlgError where Ky is not positive definite."""
    from .fit import batch_max_order, fit_batch_pairs_loo_grad
    if objective not in ("loo", "press"):
        raise ValueError('loo_chol_pairs_grad: objective is "loo" or "press"')
    hyp = np.asarray(hyp, dtype=np.float64)
    if hyp.ndim != 1:
        raise ValueError("loo_chol_pairs_grad: hyp is one row (lq.., lP.., [p..,] sig, sig2_n)")
    hyps, X, z, n = _pairs_check("loo_chol_pairs_grad", hyp[None], X, z)
    sign = -1.0 if hyp[-1] < 0.0 else 1.0
    if n <= batch_max_order():
        _, _, value, grad, info = fit_batch_pairs_loo_grad(get_family(), X, z, hyps[:, :-1], np.abs(hyps[:, -1]), objective=objective)
        if info[0]:
            raise np.linalg.LinAlgError("%d-th leading minor of the array is not positive definite" % int(info[0]))
        grad[0, -1] *= sign
        return float(value[0]), grad[0]
    with SympFit.pairs(get_family(), X, z, hyp[:-1], np.abs(hyp[-1])) as f:
        value, grad = f.run().loo_grad(objective)
        grad[-1] *= sign
        return value, grad


def _batch_data(x, y, N, reg):
    npts = N if reg else N // 2
    return x[0:npts], x[npts:2 * npts], y[:N if reg else 2 * npts]


def nll_chol_grad(hyp, x, y, N, reg=False):
    """nll_chol (reg=True: nll_chol_reg) and its exact gradient -> (nll, grad), grad[k] = d nll / d hyp[k] for every entry
    of hyp, the last being sig2_n (Ky holds |hyp[-1]|, so that entry carries its sign).  Sliced exactly like nll_chol /
    nll_chol_reg; raises LinAlgError where they do.  The objective for scipy.optimize.minimize(..., jac=True).  Up to order
    256 one launch (sgpr_fit_batch_grad with a batch of one); above, a device-resident fit and SympFit.nll_grad_full."""
    from .fit import batch_grad_max_order, fit_batch_grad
    hyp = np.asarray(hyp, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if N <= 0:
        raise ValueError("nll_chol_grad: N must be positive")
    X, Y, Z = _batch_data(x, y, N, reg)
    if len(X) != (N if reg else N // 2) or len(Y) != len(X) or len(Z) != (N if reg else 2 * len(X)):
        raise ValueError("nll_chol_grad: x holds 2 * n_pts coordinates and y the n targets of order N")
    if N <= batch_grad_max_order():
        _, nll, grad, info = fit_batch_grad(get_family(), X[None], Y[None], Z[None], hyp[None, :-1], hyp[-1:], reg=reg)
        if info[0]:
            raise np.linalg.LinAlgError("%d-th leading minor of the array is not positive definite" % int(info[0]))
        return float(nll[0]), grad[0]
    with SympFit(get_family(), X, Y, Z, hyp[:-1], hyp[-1], reg=reg) as f:
        f.run()
        return f.nll(), f.nll_grad_full()


def nll_chol_grad_batch(hyps, x, y, N, reg=False, mid=None):
    """nll_chol_batch with gradients: hyps (B, nhyp + 1) rows like nll_chol's hyp -> (nll (B,), grad (B, nhyp + 1)).  Rows
    whose Ky is not positive definite give nll = +inf and a NaN gradient row.  Up to order 256 one launch; above it, the
    nll of every row from one fit_batch call and the gradients row by row (fit.fit_batch_grad's slow path).
    mid="device": orders 256 < N <= 2048 go through fit.fit_batch_grad_mid instead, every gradient on the device in a few
    launches per chunk, with the same conventions (the values agree with the slow path to rounding, not bit for bit).
    mid=None (the default) is the behaviour described first; making "device" the default is a later one-line change, once
    that path has a measured record."""
    from .fit import batch_grad_max_order, batch_grad_mid_max_order, fit_batch_grad, fit_batch_grad_mid
    if mid not in (None, "device"):
        raise ValueError('nll_chol_grad_batch: mid is None or "device"')
    hyps = np.atleast_2d(np.asarray(hyps, dtype=np.float64))
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if hyps.ndim != 2 or hyps.shape[1] < 2:
        raise ValueError("nll_chol_grad_batch: hyps (B, nhyp + 1)")
    if N <= 0:
        raise ValueError("nll_chol_grad_batch: N must be positive")
    X, Y, Z = _batch_data(x, y, N, reg)
    if len(X) != (N if reg else N // 2) or len(Y) != len(X) or len(Z) != (N if reg else 2 * len(X)):
        raise ValueError("nll_chol_grad_batch: x holds 2 * n_pts coordinates and y the n targets of order N")
    B = len(hyps)
    fn = fit_batch_grad
    if mid == "device" and batch_grad_max_order() < N <= batch_grad_mid_max_order():
        fn = fit_batch_grad_mid
    _, nll, grad, info = fn(get_family(), np.broadcast_to(X, (B, len(X))), np.broadcast_to(Y, (B, len(Y))),
                            np.broadcast_to(Z, (B, len(Z))), hyps[:, :-1], hyps[:, -1], reg=reg)
    nll[info != 0] = np.inf
    return nll, grad


def _loo_one(hyp, x, y, N, reg):
    from .fit import batch_max_order, fit_batch_loo
    hyp = np.asarray(hyp, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if N <= 0:
        raise ValueError("loo_chol: N must be positive")
    X, Y, Z = _batch_data(x, y, N, reg)
    if len(X) != (N if reg else N // 2) or len(Y) != len(X) or len(Z) != (N if reg else 2 * len(X)):
        raise ValueError("loo_chol: x holds 2 * n_pts coordinates and y the n targets of order N")
    if len(Z) <= batch_max_order():
        _, _, loo, info = fit_batch_loo(get_family(), X[None], Y[None], Z[None], hyp[None, :-1], np.abs(hyp[-1:]), reg=reg)
        if info[0]:
            raise np.linalg.LinAlgError("%d-th leading minor of the array is not positive definite" % int(info[0]))
        return float(loo[0, 0])
    with SympFit(get_family(), X, Y, Z, hyp[:-1], np.abs(hyp[-1]), reg=reg) as f:
        return f.run().loo(resid=False, lpd=False)["loo"]


def loo_chol(hyp, x, y, N):
    """The leave-one-point-out objective of the symplectic GP, with nll_chol's arguments: minus the sum over the training points
    of the log predictive density of a point's two observed rows given all other points (SympFit.loo).  Minimised like
    nll_chol.  Up to order fit.batch_max_order() one batched call with a batch of one, above it a device-resident fit;
    raises LinAlgError where nll_chol does."""
    return _loo_one(hyp, x, y, N, False)


def loo_chol_reg(hyp, x, y, N):
    """loo_chol for the scalar-kernel GP, with nll_chol_reg's arguments (one row per point)."""
    return _loo_one(hyp, x, y, N, True)


def loo_chol_grad(hyp, x, y, N, reg=False, objective="loo"):
    """loo_chol (reg=True: loo_chol_reg) and its exact gradient -> (value, grad), grad[k] = d value / d hyp[k] for every entry
    of hyp, the last being sig2_n (Ky holds |hyp[-1]|, so that entry carries its sign).  objective="press": the sum of squared
    leave-one-point-out residuals instead.  Arguments checked and sliced like nll_chol_grad; raises LinAlgError where loo_chol
    does.  The objective for scipy.optimize.minimize(..., jac=True).  Every order goes through a device-resident fit and
    SympFit.loo_grad; a population's gradients in one launch: loo_chol_grad_batch."""
    if objective not in ("loo", "press"):
        raise ValueError('loo_chol_grad: objective is "loo" or "press"')
    hyp = np.asarray(hyp, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if N <= 0:
        raise ValueError("loo_chol_grad: N must be positive")
    X, Y, Z = _batch_data(x, y, N, reg)
    if len(X) != (N if reg else N // 2) or len(Y) != len(X) or len(Z) != (N if reg else 2 * len(X)):
        raise ValueError("loo_chol_grad: x holds 2 * n_pts coordinates and y the n targets of order N")
    with SympFit(get_family(), X, Y, Z, hyp[:-1], hyp[-1], reg=reg) as f:
        return f.run().loo_grad(objective)


def loo_chol_batch(hyps, x, y, N, reg=False):
    """loo_chol (reg=True: loo_chol_reg) for a whole population of hyper-parameter vectors over the same data, the counterpart
    of nll_chol_batch: hyps (B, nhyp + 1) -> the vector of objectives (B,).  Rows whose Ky is not positive definite come back
    as NaN.  Orders above fit.batch_max_order(): a loop over the scalar call."""
    from .fit import batch_max_order, fit_batch_loo
    hyps = np.atleast_2d(np.asarray(hyps, dtype=np.float64))
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if N > batch_max_order():
        out = np.empty(len(hyps))
        for b, h in enumerate(hyps):
            try:
                out[b] = _loo_one(h, x, y, N, reg)
            except np.linalg.LinAlgError:
                out[b] = np.nan
        return out
    if N <= 0:
        raise ValueError("loo_chol_batch: N must be positive")
    X, Y, Z = _batch_data(x, y, N, reg)
    B = len(hyps)
    _, _, loo, _ = fit_batch_loo(get_family(), np.broadcast_to(X, (B, len(X))), np.broadcast_to(Y, (B, len(Y))),
                                 np.broadcast_to(Z, (B, len(Z))), hyps[:, :-1], np.abs(hyps[:, -1]), reg=reg)
    return loo[:, 0].copy()


def loo_chol_grad_batch(hyps, x, y, N, reg=False, objective="loo", mid=None):
    """loo_chol_batch with gradients: hyps (B, nhyp + 1) rows like loo_chol's hyp -> (value (B,), grad (B, nhyp + 1)), grad[b, k]
    = d value[b] / d hyps[b, k]; the last column is sig2_n, which enters as |hyps[b, -1]| and gives that entry its sign.
    objective="press": the sum of squared leave-one-point-out residuals instead.  Sliced and checked like nll_chol_grad_batch.
    Rows whose Ky is not positive definite give NaN in the value and the whole gradient row, as in loo_chol_batch.  Up to order
    256 one launch (fit.fit_batch_loo_grad); above it the values from one fit_batch_loo call and the gradients row by row.
    mid="device": orders 256 < N <= 2048 go through fit.fit_batch_loo_grad_mid instead, every gradient on the device in a few
    launches per chunk, with the same conventions (the gradients agree with the slow path to rounding, not bit for bit).  mid=None
    (the default) is the behaviour described first."""
    from .fit import batch_grad_max_order, batch_grad_mid_max_order, fit_batch_loo_grad, fit_batch_loo_grad_mid
    if objective not in ("loo", "press"):
        raise ValueError('loo_chol_grad_batch: objective is "loo" or "press"')
    if mid not in (None, "device"):
        raise ValueError('loo_chol_grad_batch: mid is None or "device"')
    hyps = np.atleast_2d(np.asarray(hyps, dtype=np.float64))
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if hyps.ndim != 2 or hyps.shape[1] < 2:
        raise ValueError("loo_chol_grad_batch: hyps (B, nhyp + 1)")
    if N <= 0:
        raise ValueError("loo_chol_grad_batch: N must be positive")
    X, Y, Z = _batch_data(x, y, N, reg)
    if len(X) != (N if reg else N // 2) or len(Y) != len(X) or len(Z) != (N if reg else 2 * len(X)):
        raise ValueError("loo_chol_grad_batch: x holds 2 * n_pts coordinates and y the n targets of order N")
    B = len(hyps)
    fn = fit_batch_loo_grad
    if mid == "device" and batch_grad_max_order() < N <= batch_grad_mid_max_order():
        fn = fit_batch_loo_grad_mid
    _, _, value, grad, _ = fn(get_family(), np.broadcast_to(X, (B, len(X))), np.broadcast_to(Y, (B, len(Y))),
                              np.broadcast_to(Z, (B, len(Z))), hyps[:, :-1], hyps[:, -1], reg=reg, objective=objective)
    return value, grad


def guessP(x, y, hypp, xtrainp, ztrainp, Kyinvp):
    """functions/func.py:198-201."""
    Ntrain = len(xtrainp) // 2
    return sympgpr.guessp(x, y, hypp, xtrainp[0:Ntrain], xtrainp[Ntrain:], ztrainp, Kyinvp)


def calcQ(x, y, xtrain, l, Kyinv, ztrain):
    """functions/func.py:204-207."""
    Ntrain = len(xtrain) // 2
    return sympgpr.calcq(x, y, xtrain[:Ntrain], xtrain[Ntrain:], l, Kyinv, ztrain)


def calcP(x, y, l, hypp, xtrainp, ztrainp, Kyinvp, xtrain, ztrain, Kyinv):
    """functions/func.py:209-213."""
    Ntrain = len(xtrain) // 2
    Ntrainp = len(xtrainp) // 2
    return sympgpr.calcp(x, y, l, hypp, xtrainp[:Ntrainp], xtrainp[Ntrainp:], ztrainp, Kyinvp,
                         xtrain[:Ntrain], xtrain[Ntrain:], ztrain, Kyinv)


def _applymap(nm, Ntest, l, hypp, Q0map, P0map, xtrainp, ztrainp, Kyinvp, xtrain, ztrain, Kyinv, wrap):
    """The recurrences of the reference's double loop (functions/func.py:216-237) with all nm steps
    of all Ntest orbits inside one device launch (sgpr_applymap_host): alpha = Kyinv ztrain is
    formed once instead of inside every calcP / calcQ call."""
    from .maps import WRAP_Q, run_map
    return run_map(WRAP_Q if wrap else 0, nm, Ntest, l, Q0map, P0map, xtrain, ztrain, Kyinv, hypp, xtrainp,
                   ztrainp, Kyinvp)


def applymap(nm, Ntest, l, hypp, Q0map, P0map, xtrainp, ztrainp, Kyinvp, xtrain, ztrain, Kyinv):
    """functions/func.py:216-237 (q taken mod 2 pi)."""
    return _applymap(nm, Ntest, l, hypp, Q0map, P0map, xtrainp, ztrainp, Kyinvp, xtrain, ztrain, Kyinv, True)


def applymap_henon(nm, Ntest, l, hypp, Q0map, P0map, xtrainp, ztrainp, Kyinvp, xtrain, ztrain, Kyinv):
    """functions/func.py:239-260 (no wrap of q)."""
    return _applymap(nm, Ntest, l, hypp, Q0map, P0map, xtrainp, ztrainp, Kyinvp, xtrain, ztrain, Kyinv, False)


def quality(qmap, pmap, H, ysint, Ntest, Nm):
    """Diagnostics the drivers print after applying the map (same name, arguments and return values as
    functions/func.py:262-272; host arithmetic on [nm, Ntest] arrays, outside the accelerated path):
    gd[k]   mean squared distance between the first mapped point (q_1, p_1) of orbit k and the reference
            orbit ysint[Nm, :, k];  stdgd = its standard deviation over the orbits;
    Eosc[k] relative energy oscillation std(H[:, k]) / mean(H[:, k])."""
    first = np.stack((np.asarray(qmap)[1, :Ntest], np.asarray(pmap)[1, :Ntest]))          # (2, Ntest)
    gd = np.mean((first - np.asarray(ysint)[Nm, :, :Ntest]) ** 2, axis=0)
    Hk = np.asarray(H)[:, :Ntest]
    return np.std(Hk, axis=0) / np.mean(Hk, axis=0), gd, np.std(gd)


def build_dKreg(xin, x0in, hyp):
    """functions/func.py:52-78 -> [dK/dlx, dK/dly], each (N x N0)."""
    N = len(xin) // 2
    N0 = len(x0in) // 2
    return _ops.build_dkreg(xin[0:N], xin[N:2 * N], x0in[0:N0], x0in[N0:2 * N0], hyp)


def build_dK(xin, x0in, hyp):
    """functions/func.py:80-129 -> [dK/dlx, dK/dly], each (2 N0 x 2 N), rows over the "0" points."""
    N = len(xin) // 2
    N0 = len(x0in) // 2
    return _ops.build_dk(xin[0:N], xin[N:2 * N], x0in[0:N0], x0in[N0:2 * N0], hyp)


def nll_grad_reg(hyp, x, y, N):
    """functions/func.py:132-146 -> (nlp_val, nlp_grad[2]).  The reference inverts Ky and takes
    slogdet; 0.5 slogdet(Ky) = sum log diag L, so the value is the one nll_chol_reg returns."""
    hyp = np.asarray(hyp, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    with SympFit(get_family(), x[0:N], x[N:2 * N], np.asarray(y, dtype=np.float64)[:N], hyp[:-1],
                 np.abs(hyp[-1]), reg=True, lower_only=False) as f:
        f.run()
        return f.nll(), f.nll_grad()


def nll_grad(hyp, x, y, N):
    """functions/func.py:148-162 -> (nlp_val, nlp_grad[2])."""
    hyp = np.asarray(hyp, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    npts = N // 2
    with SympFit(get_family(), x[0:npts], x[npts:2 * npts], np.asarray(y, dtype=np.float64)[:2 * npts],
                 hyp[:-1], np.abs(hyp[-1]), lower_only=False) as f:
        f.run()
        return f.nll(), f.nll_grad()
