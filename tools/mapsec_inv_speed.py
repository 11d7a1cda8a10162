"""What the backward sectioned map costs beside the forward one: maps.run_map_sections_inverse
(sgpr_applymap_sections_inverse_host) against maps.run_map_sections (sgpr_applymap_sections_host) on the same data, alternately in
one process.  Family A, 37 orbits, host clock around whole calls, median of --reps.  One JSON line per size, appended to
profiles/mapsec_inv/speed.jsonl.
    python tools/mapsec_inv_speed.py [--reps R] [--out FILE]
  size a  the driver's: 4 sections of 70 points, nm = 1001 (the sections staged in LDS, in both directions)
  size b  one unstaged size: 4 sections of 1300 points, nm = 101 (the points read from memory on every pass)
The backward call starts from the last row of the forward call, with first = last_section(0, nm, nsec), and walks the same orbit
the other way: row i is forward row nm - 1 - i (the JSON says how far off it is after 10 steps and at the end -- a chaotic orbit
forgets its end point --, and the backward passes: two starting residuals and the secant updates per step; a forward step is one
guess pass, two starting residuals, its secant updates and at most one more pass for q, and the forward entry does not count them).
The model: the passes per secant update are the same and there is no guess pass, so at or below the forward call's time.  Training data and start points as in tools/mapsec_speed.py (mode WRAP_Q | LOSS_NEGP; the JSON
says how many orbits were lost)."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FAMILY = "A"


def one_size(n0, nsec, Ntest, nm, reps, sig2n):
    from mapsec_speed import start_points, training
    from sympgpr_amd import maps, sections
    xtrain, ztrain, xtrainp, ztrainp, hyp, hypp = training(nsec, n0)
    fits = sections.fit_sections(FAMILY, xtrain, ztrain, hyp, sig2n)
    fitsp = sections.fit_sections(FAMILY, xtrainp, ztrainp, hypp, sig2n, reg=True)
    alpha = np.stack([fits[m][0] for m in range(nsec)], axis=1)
    alphap = np.stack([fitsp[m][0] for m in range(nsec)], axis=1)
    Q0, P0 = start_points(Ntest)
    mode = maps.WRAP_Q | maps.LOSS_NEGP
    xt, yt, xp, yp = xtrain[:n0], xtrain[n0:], xtrainp[:n0], xtrainp[n0:]
    fwd = lambda rows: maps.run_map_sections(mode, rows, Ntest, hyp, xt, yt, alpha, Q0, P0, hypp, xp, yp, alphap, family=FAMILY)
    bwd = lambda rows, Q, P: maps.run_map_sections_inverse(mode, rows, Ntest, hyp, xt, yt, alpha, Q, P,
                                                           first=maps.last_section(0, rows, nsec), family=FAMILY, return_iters=True)
    qw, pw = fwd(nsec + 1)                                # warm-up of both routes (code object load, first allocations)
    bwd(nsec + 1, qw[-1], pw[-1])
    t_fwd, t_bwd = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        qf, pf = fwd(nm)
        t_fwd.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        qb, pb, it = bwd(nm, qf[-1], pf[-1])
        t_bwd.append(time.perf_counter() - t0)
    med = lambda v: float(np.median(v))
    ms = lambda v: [round(x * 1e3, 3) for x in v]
    alive = np.isfinite(pf[-1]) & np.isfinite(pb[-1])
    dq = np.abs(qb - qf[::-1])
    dq = np.minimum(dq, 2 * np.pi - dq)
    dist = lambda rows: float(max(np.nanmax(dq[rows][:, alive]), np.nanmax(np.abs(pb - pf[::-1])[rows][:, alive]))) if alive.any() else None
    ok = it >= 0
    return {"tool": "mapsec_inv_speed", "family": FAMILY, "n0": n0, "nsec": nsec, "Ntest": Ntest, "nm": nm, "reps": reps,
            "staged_forward": bool(nsec * 7 * n0 <= 8960), "staged_backward": bool(nsec * 4 * n0 <= 8960), "sig2n": sig2n,
            "forward_ms_calls": ms(t_fwd), "backward_ms_calls": ms(t_bwd),
            "forward_us_per_step": round(med(t_fwd) / (nm - 1) * 1e6, 3), "backward_us_per_step": round(med(t_bwd) / (nm - 1) * 1e6, 3),
            "backward_over_forward": round(med(t_bwd) / med(t_fwd), 3),
            "lost_forward": int((~np.isfinite(pf[-1])).sum()), "lost_backward": int((~np.isfinite(pb[-1])).sum()),
            "backward_updates_min_mean_max": [int(it[ok].min()), round(float(it[ok].mean()), 3), int(it[ok].max())] if ok.any() else None,
            "backward_passes_slowest_orbit": int((np.where(ok, it, 0) + 2 * ok).sum(axis=0).max()),
            "distance_after_10_steps": dist(slice(0, 11)), "distance_at_end": dist(slice(0, nm))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapsec_inv", "speed.jsonl"))
    a = ap.parse_args()
    rows = [one_size(70, 4, 37, 1001, a.reps, 1e-8), one_size(1300, 4, 37, 101, a.reps, 1e-5)]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
