"""The sectioned map (05_tokamak/Split_SympGPR: nsec GP pairs applied in turn) in one launch -- maps.run_map_sections,
sgpr_applymap_sections_host -- against the routes there were before it.  Family A, host clock around whole calls, the routes
alternately in one process, median of --reps.  One JSON line per case, appended to profiles/mapsec/mapsec_speed.jsonl.
    python tools/mapsec_speed.py [--reps R] [--n0 N] [--nsec S] [--ntest T] [--nm M] [--host-steps H] [--out FILE]
  case a  the driver's size (70 points per section, 4 sections, 30 orbits): the new entry at nm = 4001 against the host loop of
          examples/tokamak_split.applymap_tok (compute_r given, steps_per_launch=None: a Python loop over the steps, one device
          call per residual of a vectorised secant) over --host-steps steps; per step.
  case b  what cycling through sections costs: the new entry with nsec sections against sgpr_applymap_host (maps.run_map_alpha)
          on one of them, same n0, Ntest and nm.
Training data: per section a gentle symplectic map P' = p - eps sin q, Q = q + eps P' with its own eps, points and hyp, fitted on
the device (sections.fit_sections: one batched launch); start points on rotating orbits (P stays positive, inside the training
box), so that no orbit is lost and every step costs a full solve.  The JSON says how many were lost all the same."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FAMILY, SIG2N = "A", 1e-8


def training(nsec, n0, seed=7):
    """-> xtrain (2 n0, nsec), ztrain (2 n0, nsec), xtrainp (2 n0, nsec), ztrainp (n0, nsec), hyp (nsec, 3), hypp (nsec, 3)"""
    xt, zt, xp, zp, hyp = [], [], [], [], []
    for s in range(nsec):
        rng = np.random.default_rng(seed + s)
        eps = 0.2 - 0.02 * s
        q, pn = rng.uniform(0, 2 * np.pi, n0), rng.uniform(0.3, 4.3, n0)
        p_old, Q = pn + eps * np.sin(q), q + eps * pn
        xt.append(np.hstack((q, pn)))
        zt.append(np.hstack((p_old - pn, Q - q)))
        xp.append(np.hstack((q, p_old)))
        zp.append(pn)
        hyp.append([1.2 * (1 + 0.03 * s), 1.5 * (1 - 0.03 * s), 1.0])
    st = lambda a: np.stack(a, axis=1)
    return st(xt), st(zt), st(xp), st(zp), np.array(hyp), np.array(hyp)


def start_points(ntest, seed=5):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 5.5, ntest), rng.uniform(2.5, 3.0, ntest)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n0", type=int, default=70)
    ap.add_argument("--nsec", type=int, default=4)
    ap.add_argument("--ntest", type=int, default=30)
    ap.add_argument("--nm", type=int, default=4001)
    ap.add_argument("--host-steps", type=int, default=200, help="steps of the host loop per timing (it is slow); a multiple of nsec")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapsec", "mapsec_speed.jsonl"))
    a = ap.parse_args()
    from sympgpr_amd import maps, sections
    from sympgpr_amd.examples import tokamak_split as ts
    n0, nsec, Ntest, nm = a.n0, a.nsec, a.ntest, a.nm
    xtrain, ztrain, xtrainp, ztrainp, hyp, hypp = training(nsec, n0)
    fits = sections.fit_sections(FAMILY, xtrain, ztrain, hyp, SIG2N)
    fitsp = sections.fit_sections(FAMILY, xtrainp, ztrainp, hypp, SIG2N, reg=True)
    alpha = np.stack([fits[m][0] for m in range(nsec)], axis=1)
    alphap = np.stack([fitsp[m][0] for m in range(nsec)], axis=1)
    Q0, P0 = start_points(Ntest)
    mode = maps.WRAP_Q | maps.LOSS_NEGP
    xt, yt, xp, yp = xtrain[:n0], xtrain[n0:], xtrainp[:n0], xtrainp[n0:]
    new = lambda steps: maps.run_map_sections(mode, steps + 1, Ntest, hyp, xt, yt, alpha, Q0, P0, hypp, xp, yp, alphap, family=FAMILY)
    one = lambda steps: maps.run_map_alpha(mode, steps + 1, Ntest, hyp[0], Q0, P0, xt[:, 0], yt[:, 0], alpha[:, 0], hypp[0], xp[:, 0],
                                           yp[:, 0], alphap[:, 0], family=FAMILY)
    # the host loop takes Kyinv and ztrain and forms alpha = Kyinv ztrain itself: the identity hands the fitted alpha through
    eye, eyep = np.stack([np.eye(2 * n0)] * nsec), np.stack([np.eye(n0)] * nsec)
    hs = max(nsec, a.host_steps // nsec * nsec)
    host = lambda steps: ts.applymap_tok(nsec, steps + nsec, Ntest, Q0, P0, xtrainp, alphap, eyep, hypp, xtrain, alpha, eye, hyp,
                                         compute_r=lambda *z: 0.0)
    new(nsec), one(nsec), host(nsec)                      # warm-up of every route (code object load, first allocations)
    t_new, t_host, t_one = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        qn, pn = new(nm - 1)
        t_new.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        qh, ph = host(hs)
        t_host.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        qo, po = one(nm - 1)
        t_one.append(time.perf_counter() - t0)
    assert qh.shape[0] == hs + nsec and not np.any(ph[hs] == 0)          # the host loop ran exactly hs steps
    med = lambda t: float(np.median(t))
    ms = lambda t: [round(v * 1e3, 3) for v in t]
    new_step, host_step, one_step = med(t_new) / (nm - 1), med(t_host) / hs, med(t_one) / (nm - 1)
    common = {"tool": "mapsec_speed", "family": FAMILY, "n0": n0, "n0p": n0, "nsec": nsec, "Ntest": Ntest, "reps": a.reps}
    rows = [dict(common, case="a", nm=nm, new_ms_per_call=round(med(t_new) * 1e3, 3), new_ms_calls=ms(t_new),
                 new_us_per_step=round(new_step * 1e6, 3), lost_orbits_new=int(np.isnan(pn[-1]).sum()),
                 host_steps_timed=hs, host_ms_calls=ms(t_host), host_us_per_step=round(host_step * 1e6, 1),
                 lost_orbits_host=int(np.isnan(ph[hs]).sum()), host_over_new_per_step=round(host_step / new_step, 1),
                 max_abs_diff_first_steps=float(max(np.nanmax(np.abs(qn[:hs + 1] - qh[:hs + 1])),
                                                    np.nanmax(np.abs(pn[:hs + 1] - ph[:hs + 1]))))),
            dict(common, case="b", nm=nm, new_ms_calls=ms(t_new), new_us_per_step=round(new_step * 1e6, 3),
                 one_section_ms_calls=ms(t_one), one_section_us_per_step=round(one_step * 1e6, 3),
                 lost_orbits_one_section=int(np.isnan(po[-1]).sum()), new_over_one_section=round(new_step / one_step, 3))]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
