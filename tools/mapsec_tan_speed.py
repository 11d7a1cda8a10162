"""What the tangent map costs the sectioned map: maps.run_map_sections_tangent (sgpr_applymap_sections_tangent_host, all three
outputs) against maps.run_map_sections (sgpr_applymap_sections_host) on the same data, alternately in one process.  Family A,
host clock around whole calls, median of --reps.  One JSON line per size, appended to profiles/mapsec_tan/speed.jsonl.
    python tools/mapsec_tan_speed.py [--reps R] [--out FILE]
  size a  the driver's: 4 sections of 70 points, 37 orbits, nm = 1001 (the sections staged in LDS)
  size b  one unstaged size: 4 sections of 1300 points, 37 orbits, nm = 101 (the points read from memory on every pass)
The yardstick is the plain entry on the same box.  The model: one extra pass of roughly twice a rows pass's flops on top of the
guess and 3 - 6 rows passes per step, so about 1.2 - 1.5 x the plain time.  Training data and start points as in
tools/mapsec_speed.py (no orbit is lost, every step costs a full solve; the JSON says how many were lost all the same)."""
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
    args = lambda steps: (mode, steps + 1, Ntest, hyp, xt, yt, alpha, Q0, P0, hypp, xp, yp, alphap)
    plain = lambda steps: maps.run_map_sections(*args(steps), family=FAMILY)
    tang = lambda steps: maps.run_map_sections_tangent(*args(steps), family=FAMILY)
    plain(nsec), tang(nsec)                               # warm-up of both routes (code object load, first allocations)
    t_plain, t_tan = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        qp, pp = plain(nm - 1)
        t_plain.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        qt, pt, t = tang(nm - 1)
        t_tan.append(time.perf_counter() - t0)
    assert np.array_equal(qp, qt, equal_nan=True) and np.array_equal(pp, pt, equal_nan=True)
    med = lambda v: float(np.median(v))
    ms = lambda v: [round(x * 1e3, 3) for x in v]
    alive = np.isfinite(pt[-1])
    return {"tool": "mapsec_tan_speed", "family": FAMILY, "n0": n0, "n0p": n0, "nsec": nsec, "Ntest": Ntest, "nm": nm, "reps": reps,
            "staged": bool(nsec * 7 * n0 <= 8960), "sig2n": sig2n, "plain_ms_calls": ms(t_plain), "tangent_ms_calls": ms(t_tan),
            "plain_us_per_step": round(med(t_plain) / (nm - 1) * 1e6, 3), "tangent_us_per_step": round(med(t_tan) / (nm - 1) * 1e6, 3),
            "tangent_over_plain": round(med(t_tan) / med(t_plain), 3), "lost_orbits": int((~alive).sum()),
            "max_abs_det_minus_1": float(np.nanmax(np.abs(np.linalg.det(t["jac"][:, alive]) - 1.0))) if alive.any() else None,
            "lyap_max": float(np.nanmax(t["lyap"][:, 0])) if alive.any() else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapsec_tan", "speed.jsonl"))
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
