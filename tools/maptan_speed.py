"""What the tangent map costs: SympFit.applymap_pairs_tangent (sgpr_fit_applymap_nd_tangent, all three outputs) against
SympFit.applymap_pairs (sgpr_fit_applymap_nd) on the cases and data of tools/mapnd_speed.py.  Host clock around whole calls,
the two entries alternately in one process, median of --reps.  One JSON line per case.
    python tools/maptan_speed.py [--reps R] [CASE ...]       CASE = n0:d:Ntest:nm, default 64:2:37:1000 16384:3:37:20
A pass is one sweep of an orbit over the n0 training points; the plain map takes one per Newton iteration and one closing pass
per accepted step, the tangent map one more per accepted step (the Hessian sums)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sympgpr_amd import maps
from sympgpr_amd.fit import SympFit
from bench import synth_pairs

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("cases", nargs="*", default=["64:2:37:1000", "16384:3:37:20"])
a = ap.parse_args()


def training(n0, d, eps=0.25, c=0.4):      # as tools/mapnd_speed.py
    X, _, hyp, s2 = synth_pairs(n0, d)
    q, P = X[:, :d], X[:, d:] / 3.0
    s, h = q.sum(axis=1), 1.0 + 0.5 * (P * P).sum(axis=1)
    Fq = -eps * np.sin(q) - (c * eps * np.sin(s) * h)[:, None]
    FP = eps * P + (c * eps * np.cos(s))[:, None] * P
    return np.hstack((q, P)), np.concatenate((Fq.T.ravel(), FP.T.ravel())), hyp, s2


for case in a.cases:
    n0, d, Ntest, nm = (int(v) for v in case.split(":"))
    X, z, hyp, s2 = training(n0, d)
    rng = np.random.default_rng(5)
    Q0, P0 = rng.uniform(0.5, 5.5, (Ntest, d)), rng.uniform(-0.6, 0.6, (Ntest, d))
    with SympFit.pairs("A", X, z, hyp, s2) as f:
        f.run()
        f.applymap_pairs(2, Q0, P0)                       # warm-up of both entries (code object load, first allocations)
        f.applymap_pairs_tangent(2, Q0, P0)
        t_plain, t_tan = [], []
        for r in range(a.reps):
            t0 = time.perf_counter()
            q0, p0, it0 = f.applymap_pairs(nm, Q0, P0, return_iters=True)
            t_plain.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            q, p, it, out = f.applymap_pairs_tangent(nm, Q0, P0)
            t_tan.append(time.perf_counter() - t0)
    same = q.tobytes() == q0.tobytes() and p.tobytes() == p0.tobytes() and it.tobytes() == it0.tobytes()
    accepted = int((it >= 0).sum())
    passes = int(it[it > 0].sum()) + accepted
    plain_s, tan_s = float(np.median(t_plain)), float(np.median(t_tan))
    good = np.isfinite(out["lyap"]).all(axis=1)
    print(json.dumps({"tool": "maptan_speed", "family": "A", "n0": n0, "d": d, "Ntest": Ntest, "nm": nm,
                      "lost_orbits": int((it[-1] < 0).sum()), "orbit_bits_equal": bool(same),
                      "newton_iters_max": int(it.max()), "newton_iters_mean": round(float(it[it > 0].mean()), 2),
                      "passes_plain": passes, "passes_tangent": passes + accepted,
                      "pass_ratio": round((passes + accepted) / passes, 3),
                      "plain_ms_per_call": round(plain_s * 1e3, 3), "plain_ms_calls": [round(v * 1e3, 3) for v in t_plain],
                      "tangent_ms_per_call": round(tan_s * 1e3, 3), "tangent_ms_calls": [round(v * 1e3, 3) for v in t_tan],
                      "tangent_over_plain": round(tan_s / plain_s, 3),
                      "max_symplectic_defect": float(np.nanmax(maps.symplectic_defect(out["jac"]))),
                      "max_abs_lyap": float(np.abs(out["lyap"][good]).max()) if good.any() else None,
                      "max_abs_sum_lyap": float(np.abs(out["lyap"][good].sum(axis=1)).max()) if good.any() else None}),
          flush=True)
