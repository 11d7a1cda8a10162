"""Symplectic-map application: every time step of every orbit inside one device launch.

One recurrence, the variants the reference's drivers carry in their own func.py copies:

    applymap          functions/func.py:216-237           implicit, q mod 2 pi
    applymap_henon    functions/func.py:239-260           implicit, no wrap
    applymap          04_standard_map/func.py:218-254     implicit, q and P mod 2 pi, + pdiff
    applymap_expl     04_standard_map/func.py:256-285     explicit, P mod 2 pi, + pdiff
    applymap          01_pendulum/explicit/func_expl.py:113-128   explicit, q mod 2 pi
    applymap_tok      05_tokamak/SympGPR/func.py:182-211  implicit, q mod 2 pi, an orbit with P < 0 is lost (LOSS_NEGP)
    applymap_tok      05_tokamak/Split_SympGPR/func.py:184-219   the same with one GP pair per toroidal section, applied in
                                                                 turn: run_map_sections (sgpr_applymap_sections_host);
                                                                 run_map_sections_tangent adds the step matrices, their
                                                                 product and Lyapunov exponents, tangent_from_jac rebuilds the
                                                                 last two on the host from the jac of a run split into chunks;
                                                                 run_map_sections_inverse iterates it BACKWARDS
                                                                 (sgpr_applymap_sections_inverse_host), run_map_inverse the
                                                                 one-pair map of run_map_alpha: one section of the same entry

For fits with d canonical pairs (d = 1, 2, 3) the map is run_map_nd / SympFit.applymap_pairs: Newton with the analytic
Jacobian on the d unknowns P, one workgroup per orbit (include/sympgpr_hip.h: sgpr_applymap_nd_host).
run_map_nd_tangent / SympFit.applymap_pairs_tangent return the same orbits with the Jacobian of every step, their product and
finite-time Lyapunov exponents (sgpr_applymap_nd_tangent_host); symplectic_defect and greene_residue read them.
run_map_nd_inverse / SympFit.applymap_pairs_inverse iterate the same map backwards (sgpr_applymap_nd_inverse_host): Newton on the
d unknowns q with the transposed Jacobian; symplectic_inverse turns a forward step matrix into the backward step's.
run_periodic_nd / SympFit.periodic_orbits find periodic orbits of that map: Newton on the n-fold map with winding numbers, every
pass of every guess in one launch (sgpr_periodic_nd_host); multipliers reads the monodromy at any d.
genfun_along evaluates the learned generating function itself along computed orbits (sgpr_fit_predict_genfun).

alpha = Kyinv ztrain is formed once (the reference re-multiplies Kyinv inside every calcP / calcQ
call); a residual of the implicit equation is one block-wide reduction over the training points.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .ops import get_family

WRAP_Q, WRAP_P, EXPLICIT, LOSS_NEGP = L.MAP_WRAP_Q, L.MAP_WRAP_P, L.MAP_EXPLICIT, L.MAP_LOSS_NEGP


def run_map_alpha(mode, nm, Ntest, l, Q0map, P0map, xt, yt, alpha, hypp=None, xp=None, yp=None, alphap=None, family=None,
                  want_pdiff=False):
    """The same iteration from the posterior weights themselves (alpha = Ky^-1 ztrain, 2 N0; alphap, N0p) instead of the explicit
    inverses the drivers carry around: for training sets where Kyinv (8 (2 N0)^2 bytes) is not something to form.
    -> (qmap, pmap) or (qmap, pmap, pdiff), each [nm, Ntest]."""
    lib = L.load_library()
    f = L.f64
    family = get_family() if family is None else family
    xt, yt, alpha, hyp = f(xt), f(yt), f(alpha), f(l)
    if mode & EXPLICIT:
        xp, yp, alphap, hp = f([]), f([]), f([]), f([])
    else:
        xp, yp, alphap, hp = f(xp), f(yp), f(alphap), f(hypp)
    Q0, P0 = f(np.broadcast_to(Q0map, (Ntest,))), f(np.broadcast_to(P0map, (Ntest,)))
    pmap, qmap = np.zeros([nm, Ntest]), np.zeros([nm, Ntest])
    pdiff = np.zeros([nm, Ntest]) if want_pdiff else None
    L.check(lib.sgpr_applymap_host(L.family_id(family), int(mode), nm, Ntest, L.dptr(hyp), len(hyp), len(xt),
                                   L.dptr(xt), L.dptr(yt), L.dptr(alpha), L.dptr(hp), len(hp), len(xp), L.dptr(xp),
                                   L.dptr(yp), L.dptr(alphap), L.dptr(Q0), L.dptr(P0), L.dptr(qmap), L.dptr(pmap),
                                   L.dptr(pdiff) if want_pdiff else None), "sgpr_applymap_host")
    return (qmap, pmap, pdiff) if want_pdiff else (qmap, pmap)


def run_map(mode, nm, Ntest, l, Q0map, P0map, xtrain, ztrain, Kyinv, hypp=None, xtrainp=None, ztrainp=None,
            Kyinvp=None, want_pdiff=False, family=None):
    """-> (qmap, pmap) or (qmap, pmap, pdiff), each [nm, Ntest].  `l` = (lx, ly, sig) of the
    symplectic GP, xtrain = (q || P), alpha = Kyinv @ ztrain; the *p arguments describe the
    regular GP that supplies the first guess of the implicit solve (unused with EXPLICIT)."""
    Ntrain = len(xtrain) // 2
    alpha = np.asarray(Kyinv, dtype=np.float64) @ np.asarray(ztrain, dtype=np.float64)
    xp = yp = alphap = None
    if not mode & EXPLICIT:
        Ntrainp = len(xtrainp) // 2
        xp, yp = xtrainp[:Ntrainp], xtrainp[Ntrainp:2 * Ntrainp]
        alphap = np.asarray(Kyinvp, dtype=np.float64) @ np.asarray(ztrainp, dtype=np.float64)
    return run_map_alpha(mode, nm, Ntest, l, Q0map, P0map, xtrain[:Ntrain], xtrain[Ntrain:2 * Ntrain], alpha, hypp, xp, yp,
                         alphap, family=family, want_pdiff=want_pdiff)


def _section_columns(name, a, rows, nsec):
    """`a` as a float64 array with one tight column per section: (rows, nsec), F-ordered"""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != nsec:
        raise ValueError("%s must have one column per section: (%s, %d)" % (name, "rows" if rows is None else rows, nsec))
    if rows is not None and a.shape[0] != rows:
        raise ValueError("%s must be (%d, %d), not %s" % (name, rows, nsec, a.shape))
    return np.asfortranarray(a)


def _sections_model(mode, nm, Ntest, hyp, xt, yt, alpha, first, family):
    """What every sectioned entry, forwards and backwards, asks of the symplectic GPs and the call's sizes: -> (family, mode, nm,
    Ntest, first, nsec, N0, hyp (nsec, nhyp), xt, yt, alpha as tight columns).  Shape errors are ValueError."""
    family = get_family() if family is None else family
    mode, nm, Ntest, first = int(mode), int(nm), int(Ntest), int(first)
    hyp = np.asarray(hyp, dtype=np.float64)
    if hyp.ndim != 2 or hyp.shape[0] < 1:
        raise ValueError("hyp must be (nsec, nhyp) with at least one section")
    nsec = hyp.shape[0]
    if not 0 <= first < nsec:
        raise ValueError("first must lie in [0, nsec = %d)" % nsec)
    if nm < 1 or Ntest < 0:
        raise ValueError("nm must be at least 1 and Ntest non-negative")
    xt = _section_columns("xt", xt, None, nsec)
    N0 = xt.shape[0]
    yt = _section_columns("yt", yt, N0, nsec)
    alpha = _section_columns("alpha", alpha, 2 * N0, nsec)
    return family, mode, nm, Ntest, first, nsec, N0, hyp, xt, yt, alpha


def _sections_call(mode, nm, Ntest, hyp, xt, yt, alpha, Q0, P0, first, family, guess=None, want_pdiff=False):
    """What the sectioned wrappers share: the checked, laid-out arguments of their C entries as a list, the arrays its pointers
    point into, and the output arrays (qmap, pmap, pdiff or None).  guess = (hypp, xp, yp, alphap): the forward entries, whose
    list runs up to and including pdiff; guess = None: the backward entry, whose list has neither the guess GPs nor pdiff and
    ends with pmap.  Shape errors are ValueError."""
    family, mode, nm, Ntest, first, nsec, N0, hyp, xt, yt, alpha = _sections_model(mode, nm, Ntest, hyp, xt, yt, alpha, first, family)
    hyp = L.f64(hyp)                                    # C order: section s at hyp + s * nhyp
    keep, mid = [hyp, xt, yt, alpha], []
    if guess is not None:
        hypp, xp, yp, alphap = guess
        if mode & EXPLICIT:
            N0p, hp = 0, np.zeros((nsec, 0))
            xp = yp = alphap = np.zeros((0, nsec), order="F")
        else:
            if hypp is None or xp is None or yp is None or alphap is None:
                raise ValueError("the implicit map needs the guess GPs: hypp, xp, yp and alphap")
            hp = np.asarray(hypp, dtype=np.float64)
            if hp.ndim != 2 or hp.shape[0] != nsec:
                raise ValueError("hypp must be (nsec = %d, nhyp)" % nsec)
            xp = _section_columns("xp", xp, None, nsec)
            N0p = xp.shape[0]
            yp = _section_columns("yp", yp, N0p, nsec)
            alphap = _section_columns("alphap", alphap, N0p, nsec)
        hp = L.f64(hp)
        keep += [hp, xp, yp, alphap]
        mid = [L.dptr(hp), hp.shape[1], N0p, L.dptr(xp), L.dptr(yp), L.dptr(alphap)]
    Q0, P0 = L.f64(np.broadcast_to(Q0, (Ntest,))), L.f64(np.broadcast_to(P0, (Ntest,)))
    qmap, pmap = np.zeros([nm, Ntest]), np.zeros([nm, Ntest])
    pdiff = np.zeros([nm, Ntest]) if want_pdiff else None
    keep += [Q0, P0]
    args = [L.family_id(family), mode, nsec, first, nm, Ntest, L.dptr(hyp), hyp.shape[1], N0, L.dptr(xt), L.dptr(yt), L.dptr(alpha),
            *mid, L.dptr(Q0), L.dptr(P0), L.dptr(qmap), L.dptr(pmap)]
    if guess is not None:
        args.append(L.dptr(pdiff) if want_pdiff else None)
    return args, keep, (qmap, pmap, pdiff)


def run_map_sections(mode, nm, Ntest, hyp, xt, yt, alpha, Q0, P0, hypp=None, xp=None, yp=None, alphap=None, first=0,
                     want_pdiff=False, family=None):
    """The sectioned map of 05_tokamak/Split_SympGPR/func.py:184-219 in ONE launch: nsec independent GP pairs of one size,
    applied in turn -- step i -> i + 1 uses section (first + i) mod nsec (sgpr_applymap_sections_host).

    hyp (nsec, nhyp), row s = section s's (lx, ly, sig) -- (lx, ly, p, sig) for family D; xt, yt (N0, nsec) and alpha
    (2 N0, nsec), one column per section; hypp (nsec, nhyp), xp, yp, alphap (N0p, nsec) the regular GPs of the first guess
    (not needed with EXPLICIT).  alpha and alphap are the posterior weights Ky^-1 z of the sections' fits: what fit.fit_batch
    returns for them or sections.gather_sections collects, stacked as columns (np.stack(alphas, axis=1)).
    -> (qmap, pmap) or (qmap, pmap, pdiff), each [nm, Ntest]; NaN from the step at which an orbit is lost.  A map continued
    from row i with first = (first + i) mod nsec has the bits of the uninterrupted one.  Shape errors are ValueError before
    any device call."""
    args, keep, (qmap, pmap, pdiff) = _sections_call(mode, nm, Ntest, hyp, xt, yt, alpha, Q0, P0, first, family,
                                                     (hypp, xp, yp, alphap), want_pdiff)
    lib = L.load_library()
    L.check(lib.sgpr_applymap_sections_host(*args), "sgpr_applymap_sections_host")
    return (qmap, pmap, pdiff) if want_pdiff else (qmap, pmap)


def run_map_sections_tangent(mode, nm, Ntest, hyp, xt, yt, alpha, Q0, P0, hypp=None, xp=None, yp=None, alphap=None, first=0,
                             want_pdiff=False, family=None, jac=True, mono=True, lyap=True):
    """run_map_sections with the tangent map (sgpr_applymap_sections_tangent_host): -> (qmap, pmap[, pdiff], t).  The orbits
    have the bits of run_map_sections; `t` is a dict of the requested arrays: t["jac"] (nm - 1, Ntest, 2, 2), the Jacobian M of
    every step with rows (Q, P) and columns (q, p) -- step i belongs to section (first + i) mod nsec; t["mono"] (Ntest, 2, 2) =
    M_{nm-1} ... M_1 (greene_residue reads it); t["lyap"] (Ntest, 2), finite-time Lyapunov exponents per step of the map by
    Benettin's method.  All NaN from the step at which an orbit is lost.  WRAP_P has no tangent map; EXPLICIT only with the sum
    kernels (family B); lyap needs nm >= 2: ValueError before any device call, like the shape errors.  A run split into several
    calls keeps the calls' jac and takes mono and lyap from tangent_from_jac."""
    if int(mode) & WRAP_P:
        raise ValueError("the sectioned map's tangent knows no WRAP_P (it would need two Hessians per step)")
    fam = get_family() if family is None else family
    if int(mode) & EXPLICIT and not L.family_id(fam) == L.family_id("B"):
        raise ValueError("EXPLICIT has a tangent map for the sum kernels only (family B)")
    args, keep, (qmap, pmap, pdiff) = _sections_call(mode, nm, Ntest, hyp, xt, yt, alpha, Q0, P0, first, family,
                                                     (hypp, xp, yp, alphap), want_pdiff)
    t = tangent_outputs_nd(int(nm), int(Ntest), 1, jac, mono, lyap)
    lib = L.load_library()
    L.check(lib.sgpr_applymap_sections_tangent_host(*args, _optr(t, "jac"), _optr(t, "mono"), _optr(t, "lyap")),
            "sgpr_applymap_sections_tangent_host")
    return (qmap, pmap, pdiff, t) if want_pdiff else (qmap, pmap, t)


def last_section(first, nm, nsec):
    """The section whose step produced the LAST row of a forward run of nm rows that began with section `first`:
    (first + nm - 2) mod nsec -- the `first` to hand to run_map_sections_inverse with that row as start points.  (nm = 1, a run
    of no step: the section before `first`, whose step a longer run would have ended with.)"""
    first, nm, nsec = int(first), int(nm), int(nsec)
    if nsec < 1 or nm < 1 or not 0 <= first < nsec:
        raise ValueError("last_section needs nsec >= 1, nm >= 1 and first in [0, nsec)")
    return (first + nm - 2) % nsec


def map_mode_sections_inverse(mode):
    mode = int(mode)
    if mode & ~(WRAP_Q | WRAP_P | EXPLICIT | LOSS_NEGP):
        raise ValueError("unknown mode bit")
    if mode & WRAP_P:
        raise ValueError("the backward sectioned map knows no WRAP_P (the two halves of a wrapped step sit at different P)")
    if mode & EXPLICIT:
        raise ValueError("the backward sectioned map inverts the implicit map only: EXPLICIT has no backward step "
                         "(for the sum kernels the two maps coincide, use the implicit mode)")
    return mode


def run_map_sections_inverse(mode, nm, Ntest, hyp, xt, yt, alpha, Q0, P0, first=0, family=None, return_iters=False):
    """run_map_sections BACKWARDS in one launch (sgpr_applymap_sections_inverse_host): Q0, P0 are points (Q, P) and row i of
    qmap, pmap [nm, Ntest] is their i-th preimage (row 0 the start points).  Step i undoes section (first - i) mod nsec: `first`
    is the section whose forward step produced the start points -- last_section(first_forward, nm, nsec) from the last row of a
    forward run.  A step solves q + r2(q, P) - Q = 0 for q by the forward map's secant from q = Q (no guess GPs are needed),
    then p = P + r1(q, P).  hyp, xt, yt, alpha as run_map_sections takes them; mode = WRAP_Q (the solved q mod 2 pi) |
    LOSS_NEGP (a step whose solved p < 0 loses the orbit); WRAP_P and EXPLICIT have no backward step.
    -> (qmap, pmap) or with return_iters (qmap, pmap, iters): iters (nm - 1, Ntest) int32, the secant updates of each step, -1
    for a lost one.  NaN from the step at which an orbit is lost.  A run continued from row i with first = (first - i) mod nsec
    has the bits of the uninterrupted one.  Shape and mode errors are ValueError before any device call."""
    mode = map_mode_sections_inverse(mode)
    args, keep, (qmap, pmap, _) = _sections_call(mode, nm, Ntest, hyp, xt, yt, alpha, Q0, P0, first, family)
    iters = np.zeros((qmap.shape[0] - 1, qmap.shape[1]), dtype=np.int32)
    lib = L.load_library()
    L.check(lib.sgpr_applymap_sections_inverse_host(*args, iters.ctypes.data_as(C.POINTER(C.c_int))),
            "sgpr_applymap_sections_inverse_host")
    return (qmap, pmap, iters) if return_iters else (qmap, pmap)


def run_map_inverse(mode, nm, Ntest, l, Q0, P0, xt, yt, alpha, family=None, return_iters=False):
    """The one-pair (d = 1) map of run_map_alpha BACKWARDS: Q0, P0 are points (Q, P), row i of qmap, pmap [nm, Ntest] their i-th
    preimage under the map with the same l = (lx, ly, sig), xt, yt (N0) and alpha (2 N0).  The sectioned backward map with one
    section (run_map_sections_inverse): mode = WRAP_Q | LOSS_NEGP bits, no guess GP.  -> (qmap, pmap[, iters])."""
    def vec(name, a):
        a = np.asarray(a, dtype=np.float64)
        if a.ndim != 1:
            raise ValueError("%s must be a vector" % name)
        return a
    xt, yt, alpha, l = vec("xt", xt), vec("yt", yt), vec("alpha", alpha), vec("l", l)
    return run_map_sections_inverse(mode, nm, Ntest, l[None, :], xt[:, None], yt[:, None], alpha[:, None], Q0, P0, first=0,
                                    family=family, return_iters=return_iters)


def tangent_from_jac(jac):
    """mono, lyap on the host from the step matrices jac (steps, Ntest, D, D) of one or several calls, concatenated in step order:
    mono (Ntest, D, D) = M_steps ... M_1 and lyap (Ntest, D) by Benettin's method with the kernels' Gram-Schmidt order (modified,
    in column order, log |r_cc| summed per column, divided by the number of steps).  An orbit with a NaN step has NaN mono and
    lyap.  For runs split into several launches: Benettin's basis does not survive a relaunch, the step matrices do."""
    jac = np.asarray(jac, dtype=np.float64)
    if jac.ndim != 4 or jac.shape[2] != jac.shape[3] or jac.shape[0] < 1:
        raise ValueError("jac must be (steps >= 1, Ntest, D, D)")
    steps, Ntest, D = jac.shape[:3]
    mono = np.broadcast_to(np.eye(D), (Ntest, D, D)).copy()
    Q = mono.copy()
    s = np.zeros((Ntest, D))
    with np.errstate(invalid="ignore", divide="ignore"):
        for M in jac:
            mono = M @ mono
            Z = M @ Q
            for c in range(D):
                r = np.sqrt(np.einsum("kr,kr->k", Z[:, :, c], Z[:, :, c]))
                Z[:, :, c] /= r[:, None]
                for e in range(c + 1, D):
                    Z[:, :, e] -= np.einsum("kr,kr->k", Z[:, :, c], Z[:, :, e])[:, None] * Z[:, :, c]
                s[:, c] += np.log(np.abs(r))
            Q = Z
    bad = ~np.isfinite(jac).all(axis=(0, 2, 3))
    mono[bad] = np.nan
    lyap = s / steps
    lyap[bad] = np.nan
    return mono, lyap


def start_points_nd(Q0, P0, d):
    """Q0, P0 as (Ntest, d) F-ordered float64 arrays; for d = 1 a vector (Ntest,) is accepted too."""
    out = []
    for name, v in (("Q0", Q0), ("P0", P0)):
        v = np.asarray(v, dtype=np.float64)
        if d == 1 and v.ndim == 1:
            v = v.reshape(-1, 1)
        if v.ndim != 2 or v.shape[1] != d:
            raise ValueError("%s must be (Ntest, %d)%s" % (name, d, " or (Ntest,)" if d == 1 else ""))
        out.append(np.asfortranarray(v))
    if out[0].shape != out[1].shape:
        raise ValueError("Q0 and P0 must have the same shape")
    return out


def map_mode_nd(mode):
    mode = int(mode)
    if mode & ~(WRAP_Q | EXPLICIT):
        raise ValueError("the d-pair map knows WRAP_Q and EXPLICIT only")
    return mode


def map_outputs_nd(nm, Ntest, d):
    nm = int(nm)
    if nm < 1:
        raise ValueError("nm must be at least 1")
    return nm, np.zeros((nm, Ntest, d)), np.zeros((nm, Ntest, d)), np.zeros((nm - 1, Ntest), dtype=np.int32)


def run_map_nd(family, d, mode, nm, hyp, X, alpha, Q0, P0, return_iters=False):
    """The d-pair symplectic map from the posterior weights themselves: X (N0, 2d) training points with columns
    (q_1..q_d, P_1..P_d), alpha = Ky^-1 z (2 d N0, block by block like the rows of K), hyp = (lq.., lP.., [p..,] sig),
    Q0, P0 (Ntest, d) start points; mode = WRAP_Q | EXPLICIT bits.  -> qmap, pmap of shape (nm, Ntest, d), row 0 the start
    points, NaN from the step at which an orbit is lost; with return_iters also iters (nm - 1, Ntest): Newton iterations of
    each solve, 0 in explicit mode, -1 for a lost orbit.  Every step runs on the device, one workgroup per orbit."""
    qmap, pmap, iters, _ = _run_map_nd("sgpr_applymap_nd_host", family, d, map_mode_nd, mode, nm, hyp, X, alpha, Q0, P0)
    return (qmap, pmap, iters) if return_iters else (qmap, pmap)


def _nd_inputs(d, X, alpha, hyp):
    d = int(d)
    if d not in (1, 2, 3):
        raise ValueError("d must be 1, 2 or 3")
    X = np.asfortranarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != 2 * d:
        raise ValueError("X must be (N0, %d)" % (2 * d))
    alpha, hyp = L.f64(alpha), L.f64(hyp)
    if alpha.shape != (2 * d * X.shape[0],):
        raise ValueError("alpha must have length 2 d N0 = %d" % (2 * d * X.shape[0]))
    return d, X, alpha, hyp


def tangent_outputs_nd(nm, Ntest, d, jac=True, mono=True, lyap=True):
    """the arrays a tangent entry fills, by name, for those that are wanted"""
    D = 2 * d
    out = {}
    if jac:
        out["jac"] = np.zeros((nm - 1, Ntest, D, D))
    if mono:
        out["mono"] = np.zeros((Ntest, D, D))
    if lyap:
        if nm < 2:
            raise ValueError("lyap needs nm >= 2")
        out["lyap"] = np.zeros((Ntest, D))
    return out


def _optr(out, name):
    return L.dptr(out[name]) if name in out else None


def _map_call_nd(entry_name, lead_args, d, mode, nm, Q0, P0, model_args=(), tangent=None):
    """The one call behind the six d-pair map wrappers: the C entry `entry_name` with the arguments
    (*lead_args, mode, nm, Ntest, *model_args, Q0, ldq, P0, ldp, qmap, pmap, iters[, jac, mono, lyap]) -- a fit's entries lead
    with the handle, the _host entries with (family, d) and carry the model (hyp .. alpha) in model_args.
    tangent = (jac, mono, lyap): which tangent arrays are wanted.  -> (qmap, pmap, iters, out or None).  Shape errors are
    ValueError before the library is loaded."""
    Q0, P0 = start_points_nd(Q0, P0, d)
    Ntest = Q0.shape[0]
    nm, qmap, pmap, iters = map_outputs_nd(nm, Ntest, d)
    out = None if tangent is None else tangent_outputs_nd(nm, Ntest, d, *tangent)
    opt = () if tangent is None else (_optr(out, "jac"), _optr(out, "mono"), _optr(out, "lyap"))
    entry = getattr(L.load_library(), entry_name)
    L.check(entry(*lead_args, mode, nm, Ntest, *model_args, L.dptr(Q0), max(Ntest, 1), L.dptr(P0), max(Ntest, 1), L.dptr(qmap),
                  L.dptr(pmap), iters.ctypes.data_as(C.POINTER(C.c_int)), *opt), entry_name)
    return qmap, pmap, iters, out


def _run_map_nd(entry_name, family, d, check_mode, mode, nm, hyp, X, alpha, Q0, P0, tangent=None):
    """run_map_nd, run_map_nd_tangent and run_map_nd_inverse: the model's checks, then the mode's, then _map_call_nd"""
    d, X, alpha, hyp = _nd_inputs(d, X, alpha, hyp)
    N0 = X.shape[0]
    mode = check_mode(mode)
    model = (L.dptr(hyp), len(hyp), N0, L.dptr(X), max(N0, 1), L.dptr(alpha))
    return _map_call_nd(entry_name, (L.family_id(family), d), d, mode, nm, Q0, P0, model, tangent)


def run_map_nd_tangent(family, d, mode, nm, hyp, X, alpha, Q0, P0, jac=True, mono=True, lyap=True):
    """run_map_nd with the tangent map: -> (qmap, pmap, iters, out).  qmap, pmap, iters have the bits of run_map_nd; `out` is a
    dict of the requested arrays: jac (nm - 1, Ntest, D, D), the Jacobian M of every step with rows (Q_1..Q_d, P_1..P_d) and
    columns (q_1..q_d, p_1..p_d), D = 2 d; mono (Ntest, D, D) = M_{nm-1} ... M_1; lyap (Ntest, D), finite-time Lyapunov exponents
    per step of the map by Benettin's method, in Gram-Schmidt column order.  All NaN from the step at which an orbit is lost.
    EXPLICIT is accepted for the sum kernels only (family B)."""
    return _run_map_nd("sgpr_applymap_nd_tangent_host", family, d, map_mode_nd, mode, nm, hyp, X, alpha, Q0, P0,
                       (jac, mono, lyap))


def map_mode_nd_inverse(mode):
    mode = map_mode_nd(mode)
    if mode & EXPLICIT:
        raise ValueError("the backward d-pair map inverts the implicit map only: EXPLICIT has no backward step "
                         "(for the sum kernels the two maps coincide, use mode 0)")
    return mode


def run_map_nd_inverse(family, d, mode, nm, hyp, X, alpha, Q0, P0, return_iters=False):
    """run_map_nd backwards: Q0, P0 (Ntest, d) are points (Q, P) and row i of qmap, pmap (nm, Ntest, d) is their i-th preimage
    under the map of run_map_nd with the same X, alpha, hyp (row 0 the start points).  A step solves q + G_P(q, P) - Q = 0 for q
    by Newton from q = Q with the transposed Jacobian block of the forward solve, then p = P + G_q(q, P); mode = WRAP_Q (the
    solved q mod 2 pi) or 0 -- EXPLICIT raises ValueError (the explicit product-family map has another inverse).  NaN from the
    step at which an orbit is lost; with return_iters also iters (nm - 1, Ntest): Newton iterations, -1 for a lost orbit.  Every
    step runs on the device, one workgroup per orbit (sgpr_applymap_nd_inverse_host)."""
    qmap, pmap, iters, _ = _run_map_nd("sgpr_applymap_nd_inverse_host", family, d, map_mode_nd_inverse, mode, nm, hyp, X, alpha,
                                       Q0, P0)
    return (qmap, pmap, iters) if return_iters else (qmap, pmap)


def _periodic_call_nd(entry_name, lead_args, d, mode, n, Q0, P0, wind, tol, maxit, mono, orbit, model_args=()):
    """The one call behind run_periodic_nd and SympFit.periodic_orbits: the C entry `entry_name` with the arguments
    (*lead_args, mode, n, Ntest, *model_args, wind, Q0, ldq, P0, ldp, tol, maxit, z, resid, its, mono, qorb, porb).  Shape errors
    are ValueError before the library is loaded; n, tol and maxit are the library's to refuse (SympGPRError, SGPR_E_ARG)."""
    Q0, P0 = start_points_nd(Q0, P0, d)
    Ntest, D, n = Q0.shape[0], 2 * d, int(n)
    wptr = None
    if wind is not None:
        w = np.asarray(wind)
        if w.ndim <= 1 and w.size == d:
            w = np.broadcast_to(w.reshape(1, d), (Ntest, d))                           # one winding vector for every guess
        elif d == 1 and w.ndim == 1:
            w = w.reshape(-1, 1)
        if w.shape != (Ntest, d) or not np.array_equal(w, np.round(w)):
            raise ValueError("wind must hold integers, (Ntest, %d) or (%d,)" % (d, d))
        w = np.asfortranarray(w, dtype=np.int32)
        wptr = w.ctypes.data_as(C.POINTER(C.c_int))
    rows = max(n, 0)
    out = {"z": np.zeros((Ntest, D)), "resid": np.zeros(Ntest), "its": np.zeros(Ntest, dtype=np.int32)}
    if mono:
        out["mono"] = np.zeros((Ntest, D, D))
    if orbit:
        out["q"], out["p"] = np.zeros((rows, Ntest, d)), np.zeros((rows, Ntest, d))
    entry = getattr(L.load_library(), entry_name)
    L.check(entry(*lead_args, mode, n, Ntest, *model_args, wptr, L.dptr(Q0), max(Ntest, 1), L.dptr(P0), max(Ntest, 1), float(tol),
                  int(maxit), L.dptr(out["z"]), L.dptr(out["resid"]), out["its"].ctypes.data_as(C.POINTER(C.c_int)),
                  _optr(out, "mono"), _optr(out, "q"), _optr(out, "p")), entry_name)
    out["converged"] = out["its"] > 0
    return out


def run_periodic_nd(family, d, mode, n, hyp, X, alpha, Q0, P0, wind=None, tol=1e-12, maxit=30, mono=True, orbit=False):
    """Periodic orbits of the map of run_map_nd (same family, d, hyp, X, alpha, mode = WRAP_Q | EXPLICIT bits, EXPLICIT for the
    sum kernels only): for every guess z = (q, p) = row of Q0, P0 (Ntest, d) find z* with
        r(z) = (q_n - q_0 - 2 pi w, p_n - p_0) = 0,      (q_n, p_n) the n-th image of z in lifted (unwrapped) coordinates,
    for the period n >= 1 and the integer winding numbers wind ((Ntest, d), or (d,) for all guesses, default 0), by plain Newton
    on the n-fold map, z <- z - (mono(z) - I)^-1 r(z): no damping, no line search.  Every pass of a guess -- n steps of the map
    with its tangent map, the 2d x 2d solve -- runs on the device inside ONE launch, one workgroup per guess
    (sgpr_periodic_nd_host).  A guess has converged when the pass that started from z has max|r| <= tol max(1, max|z|).
    -> dict: z (Ntest, 2d) the points (q*, p*); resid (Ntest,) max|r| evaluated at z; its (Ntest,) int32, the passes run, the
    converged one included; converged (Ntest,) bool; with mono=True mono (Ntest, 2d, 2d), the monodromy of the returned orbit
    (multipliers and greene_residue read it); with orbit=True q, p (n, Ntest, d), the returned orbit, row 0 = z, bit for bit what
    run_map_nd gives from z.  A guess that fails -- maxit passes without convergence, a lost orbit, a singular I + B or mono - I,
    a non-finite update or start -- has its = -1 and NaN in z, resid, mono, q and p; the others keep their bits.  With WRAP_Q
    the q of an updated guess is wrapped into [0, 2 pi).
    HAZARD: far from the training data the GP returns its prior mean, the learned map is the identity, and EVERY far point is a
    "fixed point" with mono = I to rounding.  Newton can walk there from a poor guess (on the CPU, family C at d = 3 went from
    (0.1, ...) to such a point with |(mono - I)^-1| = 1e13) and report convergence: discard results whose mono - I is negligible."""
    d, X, alpha, hyp = _nd_inputs(d, X, alpha, hyp)
    N0 = X.shape[0]
    model = (L.dptr(hyp), len(hyp), N0, L.dptr(X), max(N0, 1), L.dptr(alpha))
    return _periodic_call_nd("sgpr_periodic_nd_host", (L.family_id(family), d), d, map_mode_nd(mode), n, Q0, P0, wind, tol, maxit,
                             mono, orbit, model)


def multipliers(mono):
    """Floquet multipliers of symplectic monodromy matrices mono (..., D, D) as reciprocal pairs -> complex (..., D / 2, 2):
    [..., i, 0] and [..., i, 1] are lambda_i and its partner closest to 1 / lambda_i, the pairs ordered by |lambda_i| descending
    (|lambda| >= 1 first in each pair).  Classifies an orbit at any d (greene_residue is for d = 1): every pair on the unit circle
    is elliptic, a real pair (lambda, 1 / lambda) hyperbolic, a quadruple off both is complex unstable.  NaN input gives NaN.
    Mind the hazard named in run_periodic_nd: where the learned map is the identity every multiplier is 1 and means nothing."""
    mono = np.asarray(mono, dtype=np.float64)
    if mono.ndim < 2 or mono.shape[-1] != mono.shape[-2] or mono.shape[-1] % 2:
        raise ValueError("mono must be (..., D, D) with D even")
    D = mono.shape[-1]
    flat = mono.reshape(-1, D, D)
    out = np.full((flat.shape[0], D // 2, 2), np.nan + 0j)
    for k, M in enumerate(flat):
        if not np.isfinite(M).all():
            continue
        left = list(np.linalg.eigvals(M))
        left.sort(key=lambda v: -abs(v))
        for i in range(D // 2):
            lam = left.pop(0)
            j = int(np.argmin([abs(v - 1.0 / lam) for v in left]))
            out[k, i] = lam, left.pop(j)
    return out.reshape(mono.shape[:-2] + (D // 2, 2))


def genfun_along(fit, qmap, pmap, ref=None):
    """The fit's learned generating function along computed orbits: F(q_k, P_{k+1}) for k = 0 .. nm-2 -> (nm - 1, Ntest), an
    energy-like diagnostic that needs no analytic H.  qmap, pmap: (nm, Ntest) or (nm, Ntest, d) as applymap / applymap_pairs
    return them; ref as SympFit.predict_genfun / predict_pairs_genfun take it.  One device call over all steps and orbits, the
    bits of predict_genfun / predict_pairs_genfun on the stacked points; a lost (NaN) orbit stays NaN."""
    qmap, pmap = np.asarray(qmap, dtype=np.float64), np.asarray(pmap, dtype=np.float64)
    if qmap.shape != pmap.shape or qmap.ndim not in (2, 3) or qmap.shape[0] < 1:
        raise ValueError("qmap and pmap must both be (nm, Ntest) or (nm, Ntest, d)")
    nm, Ntest = qmap.shape[:2]
    d = 1 if qmap.ndim == 2 else qmap.shape[2]
    if d != fit.d:
        raise ValueError("the orbits have d = %d, the fit d = %d" % (d, fit.d))
    Xt = np.asfortranarray(np.hstack((qmap[:-1].reshape(-1, d), pmap[1:].reshape(-1, d))))
    F = fit.predict_genfun(Xt[:, 0], Xt[:, 1], ref=ref) if qmap.ndim == 2 else fit.predict_pairs_genfun(Xt, ref=ref)
    return F.reshape(nm - 1, Ntest)


def symplectic_defect(M):
    """max |M^T J M - J| over the last two axes of M (..., D, D), J = [[0, I], [-I, 0]] in the order (q_1..q_d, p_1..p_d)"""
    M = np.asarray(M, dtype=np.float64)
    if M.ndim < 2 or M.shape[-1] != M.shape[-2] or M.shape[-1] % 2:
        raise ValueError("M must be (..., D, D) with D even")
    d = M.shape[-1] // 2
    J = np.zeros((2 * d, 2 * d))
    J[:d, d:], J[d:, :d] = np.eye(d), -np.eye(d)
    return np.abs(np.swapaxes(M, -1, -2) @ J @ M - J).max(axis=(-2, -1))


def symplectic_inverse(M):
    """-J M^T J over the last two axes of M (..., D, D), J as in symplectic_defect: the inverse of a symplectic M, exact (the
    blocks [[a, b], [c, e]] are rearranged to [[e^T, -b^T], [-c^T, a^T]], no arithmetic).
    This is how the tangent map of a BACKWARD orbit is obtained without a kernel of its own: the Jacobian of backward step i,
    (Q, P) -> (q, p), is the symplectic inverse of the forward step matrix at the same (q, P).  Run run_map_nd_tangent /
    SympFit.applymap_pairs_tangent for one step (nm = 2) from each row i + 1 of the backward orbit and apply this to jac[0]."""
    M = np.asarray(M, dtype=np.float64)
    if M.ndim < 2 or M.shape[-1] != M.shape[-2] or M.shape[-1] % 2:
        raise ValueError("M must be (..., D, D) with D even")
    d = M.shape[-1] // 2
    T = np.swapaxes(M, -1, -2)
    out = np.empty_like(T)
    out[..., :d, :d], out[..., :d, d:] = T[..., d:, d:], -T[..., d:, :d]      # T = M^T holds [[a^T, c^T], [b^T, e^T]]
    out[..., d:, :d], out[..., d:, d:] = -T[..., :d, d:], T[..., :d, :d]
    return out


def greene_residue(mono):
    """Greene's residue (2 - tr M) / 4 of the monodromy matrices mono (..., 2, 2) of a one-pair map"""
    mono = np.asarray(mono, dtype=np.float64)
    if mono.ndim < 2 or mono.shape[-2:] != (2, 2):
        raise ValueError("greene_residue is defined for D = 2: mono must be (..., 2, 2)")
    return (2.0 - np.trace(mono, axis1=-2, axis2=-1)) / 4.0
