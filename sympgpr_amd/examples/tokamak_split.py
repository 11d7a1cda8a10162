"""python/05_tokamak/Split_SympGPR/func.py -- kernel family A; nphmap independent GPs, one per
toroidal section, applied in turn (the sections are independent fits: "replicas only" across
GPUs, see sympgpr_amd/sections.py)."""
import numpy as np

from . import _common as _c
from ..func import calcP, calcQ, guessP  # noqa: F401  (func.py:167-182)

FAMILY = "A"
_c.python_surface(FAMILY, globals())
for _n in ("calcP", "calcQ", "guessP"):
    globals()[_n] = _c.with_family(FAMILY)(globals()[_n])


def build_dK(xin, x0in, hyp):
    """func.py:47-111 -> [dK/dlx, dK/dly, K/sig]"""
    return _c.build_dK3(FAMILY, xin, x0in, hyp)


def nll_chol_reg(hyp, x, y, N):
    """func.py:128-146: eigen fallback with neig = len(x)//2"""
    return _c.nll_fit(FAMILY, hyp, x, y, N, reg=True, neig=len(x) // 2)


def nll_chol(hyp, x, y, N):
    """func.py:148-166: eigen fallback with neig = len(x)//2"""
    return _c.nll_fit(FAMILY, hyp, x, y, N, neig=len(x) // 2)


def map_steps(nphmap, nm):
    """the steps applymap_tok runs: the reference's while loop advances nphmap steps at a time (func.py:196-197)"""
    return -(-(nm - nphmap) // nphmap) * nphmap if nm > nphmap else 0


def map_in_chunks(run, nphmap, nm, Ntest, Q0map, P0map, compute_r=None, steps_per_launch=None, jac_out=None):
    """The bookkeeping of applymap_tok around a stepper `run(first, steps, Q0, P0) -> (q, p)`, each [steps + 1, len(Q0)] with
    row 0 the start points and NaN from the step at which an orbit is lost: `steps` steps of the sectioned map whose first
    step uses section `first`.  The reference's loop quirk is kept (func.py:196-197: the while loop advances nphmap steps at
    a time): ceil((nm - nphmap) / nphmap) nphmap steps are run and the rows beyond them stay 0.  Without a callback the
    whole map is one call of `run`; with one, `steps_per_launch` steps per call, each continued with first = i mod nphmap from
    the orbits still alive, and compute_r is applied to the new rows step by step and orbit by orbit in the reference's
    order (func.py:212-217).  What a chunk computed for an orbit beyond the step that lost it is dropped.
    jac_out (map_steps(nphmap, nm), Ntest, 2, 2), filled with NaN by the caller: `run` then returns (q, p, jac) with jac
    [steps, len(Q0), 2, 2] the step matrices, and row i of jac_out receives the matrix of step i -> i + 1 of every orbit whose
    row i + 1 is kept."""
    pmap = np.zeros([nm, Ntest])
    qmap = np.zeros([nm, Ntest])
    pmap[0, :] = P0map
    qmap[0, :] = Q0map
    steps = map_steps(nphmap, nm)
    if steps == 0:
        return qmap, pmap
    k = steps if compute_r is None else max(1, int(steps_per_launch or 1))
    pmap[1:steps + 1, :] = np.nan
    qmap[1:steps + 1, :] = np.nan
    i = 0
    while i < steps:
        kk = min(k, steps - i)
        idx = np.nonzero(~np.isnan(pmap[i, :]))[0]
        if len(idx):
            out = run(i % nphmap, kk, qmap[i, idx], pmap[i, idx])
            qq, pp = out[0], out[1]
            jj = out[2] if jac_out is not None else None
            if compute_r is None:
                pmap[i + 1:i + kk + 1, idx], qmap[i + 1:i + kk + 1, idx] = pp[1:], qq[1:]
                if jj is not None:
                    jac_out[i:i + kk, idx] = jj
            else:
                alive = np.ones(len(idx), dtype=bool)
                for s in range(1, kk + 1):
                    ph = (2 * np.pi) / nphmap * np.mod(i + s, nphmap)
                    for j, orbit in enumerate(idx):
                        if not alive[j]:
                            continue
                        if np.isnan(pp[s, j]):                  # the solve failed or P < 0: lost inside the kernel
                            alive[j] = False
                            continue
                        if compute_r(np.array([pp[s, j] * 1e-2, qq[s, j], ph]), 0.3) > 0.5:
                            alive[j] = False
                            continue
                        pmap[i + s, orbit], qmap[i + s, orbit] = pp[s, j], qq[s, j]
                        if jj is not None:
                            jac_out[i + s - 1, orbit] = jj[s - 1, j]
        i += kk
    return qmap, pmap


def applymap_tok(nphmap, nm, Ntest, Q0map, P0map, xtrainp, ztrainp, Kyinvp, hypp, xtrain, ztrain, Kyinv, hyp,
                 compute_r=None, steps_per_launch=None):
    """func.py:184-219: section m's GP pair maps step i -> i+1 for i = m (mod nphmap).
    xtrainp (2N x nphmap), ztrainp (N x nphmap), Kyinvp (nphmap x N x N), hypp (nphmap x 3) and the
    same for the symplectic GP.  `compute_r(zk, r_gss)`: the reference's fieldlines.compute_r; an
    orbit with compute_r > 0.5 or P < 0 is lost (without it only P < 0).
    Every time step runs on the device (maps.run_map_sections: the implicit P, the P < 0 test and the q update of all
    sections inside one kernel): without a callback the whole map is ONE launch; with a callback and steps_per_launch = k,
    k steps per launch with the callback applied to the new rows on the host (map_in_chunks).  With a callback and
    steps_per_launch = None every step is driven from the host (one batched device call per residual of the secant)."""
    if compute_r is not None and steps_per_launch is None:
        return _applymap_tok_host(nphmap, nm, Ntest, Q0map, P0map, xtrainp, ztrainp, Kyinvp, hypp, xtrain, ztrain, Kyinv, hyp,
                                  compute_r)
    run = _sections_stepper(nphmap, xtrainp, ztrainp, Kyinvp, hypp, xtrain, ztrain, Kyinv, hyp)
    return map_in_chunks(run, nphmap, nm, Ntest, np.broadcast_to(Q0map, (Ntest,)), np.broadcast_to(P0map, (Ntest,)), compute_r,
                         steps_per_launch)


def _sections_stepper(nphmap, xtrainp, ztrainp, Kyinvp, hypp, xtrain, ztrain, Kyinv, hyp, tangent=None):
    """map_in_chunks's `run` for the drivers' arrays: maps.run_map_sections, or with `tangent` (a dict of
    maps.run_map_sections_tangent's jac / mono / lyap switches) that entry; its last result's dict is kept in tangent["last"]"""
    from .. import maps
    f = lambda a: np.asarray(a, dtype=np.float64)
    xtrain, ztrain, xtrainp, ztrainp, hyp, hypp = (f(a) for a in (xtrain, ztrain, xtrainp, ztrainp, hyp, hypp))
    N, Np = xtrain.shape[0] // 2, xtrainp.shape[0] // 2
    sec = range(nphmap)
    alpha = np.stack([f(Kyinv[m]) @ ztrain[:, m] for m in sec], axis=1)           # once per section, not per step
    alphap = np.stack([f(Kyinvp[m]) @ ztrainp[:, m] for m in sec], axis=1)
    mode = maps.WRAP_Q | maps.LOSS_NEGP

    def run(first, steps, Q0, P0):
        args = (mode, steps + 1, len(Q0), hyp[:nphmap], xtrain[:N, :nphmap], xtrain[N:2 * N, :nphmap], alpha, Q0, P0, hypp[:nphmap],
                xtrainp[:Np, :nphmap], xtrainp[Np:2 * Np, :nphmap], alphap)
        if tangent is None:
            return maps.run_map_sections(*args, first=first, family=FAMILY)
        q, p, t = maps.run_map_sections_tangent(*args, first=first, family=FAMILY, jac=tangent["jac"], mono=tangent["mono"],
                                                lyap=tangent["lyap"])
        tangent["last"] = t
        return q, p, t.get("jac")
    return run


def applymap_tok_tangent(nphmap, nm, Ntest, Q0map, P0map, xtrainp, ztrainp, Kyinvp, hypp, xtrain, ztrain, Kyinv, hyp,
                         compute_r=None, steps_per_launch=None):
    """applymap_tok with the tangent map (maps.run_map_sections_tangent): -> (qmap, pmap, t), the orbits as applymap_tok returns
    them from the device and t["jac"] (steps, Ntest, 2, 2), t["mono"] (Ntest, 2, 2), t["lyap"] (Ntest, 2) over the
    steps = map_steps(nphmap, nm) steps that are run; NaN from the step at which an orbit is lost.  Without a callback ONE
    launch, mono and lyap from the device.  With compute_r, steps_per_launch = k steps per launch (1 if not given: every step
    runs on the device here), the chunks' jac collected by map_in_chunks's bookkeeping and mono, lyap taken from them on the
    host (maps.tangent_from_jac): Benettin's basis does not survive a relaunch."""
    from .. import maps
    steps = map_steps(nphmap, nm)
    Q0, P0 = np.broadcast_to(Q0map, (Ntest,)), np.broadcast_to(P0map, (Ntest,))
    t = {"jac": np.full((steps, Ntest, 2, 2), np.nan), "mono": np.broadcast_to(np.eye(2), (Ntest, 2, 2)).copy(),
         "lyap": np.full((Ntest, 2), np.nan)}
    if steps == 0:
        qmap, pmap = map_in_chunks(None, nphmap, nm, Ntest, Q0, P0)
        return qmap, pmap, t
    one = compute_r is None
    sw = {"jac": True, "mono": one, "lyap": one}
    run = _sections_stepper(nphmap, xtrainp, ztrainp, Kyinvp, hypp, xtrain, ztrain, Kyinv, hyp, tangent=sw)
    qmap, pmap = map_in_chunks(run, nphmap, nm, Ntest, Q0, P0, compute_r, steps_per_launch, jac_out=t["jac"])
    if one and "last" in sw:                  # one launch over all Ntest orbits (a NaN start is an orbit like any other there)
        alive = ~np.isnan(P0)
        t["mono"][:], t["lyap"][:] = np.nan, np.nan
        t["mono"][alive], t["lyap"][alive] = sw["last"]["mono"], sw["last"]["lyap"]
    else:
        t["mono"], t["lyap"] = maps.tangent_from_jac(t["jac"])
    return qmap, pmap, t


def map_in_chunks_inverse(run, nphmap, nm, Ntest, Q0map, P0map, start=0, compute_r=None, steps_per_launch=None):
    """map_in_chunks's backward twin, around a stepper `run(first, steps, Q0, P0) -> (q, p)`, each [steps + 1, len(Q0)] with row
    0 the start points and NaN from the step at which an orbit is lost: `steps` BACKWARD steps of the sectioned map whose first
    step undoes section `first`.  The start points sit at toroidal section index `start`; row j sits at index (start - j) mod
    nphmap and step j -> j + 1 undoes GP pair (start - j - 1) mod nphmap.  All nm - 1 steps are run (the forward loop's quirk of
    whole turns belongs to the reference's forward loop only).  Without a callback one call of `run`; with one,
    `steps_per_launch` steps per call, each continued at its section from the orbits still alive, and compute_r is applied to the
    new rows step by step and orbit by orbit at the row's own angle.  What a chunk computed for an orbit beyond the step that
    lost it is dropped."""
    pmap = np.zeros([nm, Ntest])
    qmap = np.zeros([nm, Ntest])
    pmap[0, :] = P0map
    qmap[0, :] = Q0map
    steps = nm - 1
    if steps <= 0:
        return qmap, pmap
    k = steps if compute_r is None else max(1, int(steps_per_launch or 1))
    pmap[1:, :] = np.nan
    qmap[1:, :] = np.nan
    i = 0
    while i < steps:
        kk = min(k, steps - i)
        idx = np.nonzero(~np.isnan(pmap[i, :]))[0]
        if len(idx):
            qq, pp = run((start - i - 1) % nphmap, kk, qmap[i, idx], pmap[i, idx])[:2]
            if compute_r is None:
                pmap[i + 1:i + kk + 1, idx], qmap[i + 1:i + kk + 1, idx] = pp[1:], qq[1:]
            else:
                alive = np.ones(len(idx), dtype=bool)
                for s in range(1, kk + 1):
                    ph = (2 * np.pi) / nphmap * np.mod(start - (i + s), nphmap)
                    for j, orbit in enumerate(idx):
                        if not alive[j]:
                            continue
                        if np.isnan(pp[s, j]):                  # the solve failed or p < 0: lost inside the kernel
                            alive[j] = False
                            continue
                        if compute_r(np.array([pp[s, j] * 1e-2, qq[s, j], ph]), 0.3) > 0.5:
                            alive[j] = False
                            continue
                        pmap[i + s, orbit], qmap[i + s, orbit] = pp[s, j], qq[s, j]
        i += kk
    return qmap, pmap


def applymap_tok_inverse(nphmap, nm, Ntest, Q0map, P0map, xtrain, ztrain, Kyinv, hyp, start=0, compute_r=None,
                         steps_per_launch=None):
    """applymap_tok BACKWARDS (maps.run_map_sections_inverse): Q0map, P0map are points at toroidal section index `start`, row j
    of (qmap, pmap) [nm, Ntest] their j-th preimage, at section index (start - j) mod nphmap; step j uses GP pair
    (start - j - 1) mod nphmap.  From the last row i of a forward applymap_tok run, start = i mod nphmap.  xtrain (2N x nphmap),
    ztrain (2N x nphmap), Kyinv (nphmap x 2N x 2N), hyp (nphmap x 3): the symplectic GPs alone, the backward solve needs no
    guess.  An orbit whose preimage has p < 0 -- or compute_r > 0.5, with a callback -- is lost: NaN from that row on.  All nm - 1
    steps run on the device: without a callback in ONE launch; with compute_r, steps_per_launch = k steps per launch (1 if not
    given) with the callback applied on the host to each new row at that row's own angle (map_in_chunks_inverse)."""
    from .. import maps
    f = lambda a: np.asarray(a, dtype=np.float64)
    xtrain, ztrain, hyp = f(xtrain), f(ztrain), f(hyp)
    nphmap, start = int(nphmap), int(start)
    N = xtrain.shape[0] // 2
    alpha = np.stack([f(Kyinv[m]) @ ztrain[:, m] for m in range(nphmap)], axis=1)           # once per section, not per step
    mode = maps.WRAP_Q | maps.LOSS_NEGP

    def run(first, steps, Q0, P0):
        return maps.run_map_sections_inverse(mode, steps + 1, len(Q0), hyp[:nphmap], xtrain[:N, :nphmap], xtrain[N:2 * N, :nphmap],
                                             alpha, Q0, P0, first=first, family=FAMILY)
    return map_in_chunks_inverse(run, nphmap, nm, Ntest, np.broadcast_to(Q0map, (Ntest,)), np.broadcast_to(P0map, (Ntest,)),
                                 start % nphmap, compute_r, steps_per_launch)


def _applymap_tok_host(nphmap, nm, Ntest, Q0map, P0map, xtrainp, ztrainp, Kyinvp, hypp, xtrain, ztrain, Kyinv, hyp, compute_r):
    """the host-driven form of applymap_tok: a Python loop over the time steps"""
    preds = [_c.predictor_pair(FAMILY, hyp[m, :], hypp[m, :], xtrainp[:, m], ztrainp[:, m], Kyinvp[m], xtrain[:, m],
                               ztrain[:, m], Kyinv[m]) for m in range(nphmap)]
    pmap = np.zeros([nm, Ntest])
    qmap = np.zeros([nm, Ntest])
    pmap[0, :] = P0map
    qmap[0, :] = Q0map
    i = 0
    r_gss = 0.3
    r_cut = 0.5
    while i < nm - nphmap:
        for m in range(0, nphmap):
            pr, prp = preds[m]
            pmap[i + 1, :] = np.nan
            qmap[i + 1, :] = np.nan
            ok = ~np.isnan(pmap[i, :])
            if ok.any():
                pmap[i + 1, ok] = _c.solve_implicit_P(pr, prp, qmap[i, ok], pmap[i, ok])
            ok2 = ~np.isnan(pmap[i + 1, :])
            if ok2.any():
                dq = pr(qmap[i, ok2], pmap[i + 1, ok2])[1]
                qmap[i + 1, ok2] = np.mod(dq + qmap[i, ok2], 2 * np.pi)
                ph = (2 * np.pi) / nphmap * np.mod(i + 1, nphmap)
                for k in np.nonzero(ok2)[0]:
                    lost = pmap[i + 1, k] < 0.0
                    if compute_r is not None and not lost:
                        lost = compute_r(np.array([pmap[i + 1, k] * 1e-2, qmap[i + 1, k], ph]), r_gss) > r_cut
                    if lost:
                        pmap[i + 1, k] = np.nan
                        qmap[i + 1, k] = np.nan
            i = i + 1
    return qmap, pmap


def quality(qmap, pmap, H, ysint, Ntest, Nm):
    """Diagnostics of Split_SympGPR/func.py:221-233 (host arithmetic): (p, q) against ysint[Nm, 0:2, k], H indexed
    [orbit, step]; like the reference it wraps ysint[:, 1] mod 2 pi IN PLACE."""
    ysint[:, 1] = np.mod(ysint[:, 1], 2 * np.pi)
    first = np.stack((np.asarray(pmap)[1, :Ntest], np.asarray(qmap)[1, :Ntest]))
    gd = np.mean((first - np.asarray(ysint)[Nm, 0:2, :Ntest]) ** 2, axis=0)
    Hk = np.asarray(H)[:Ntest, :]
    return np.std(Hk, axis=1) / np.mean(Hk, axis=1), gd, np.std(gd)
