"""The d-pair symplectic map forwards (maps.run_map_nd: sgpr_applymap_nd_host) and backwards (maps.run_map_nd_inverse:
sgpr_applymap_nd_inverse_host) on the same data in one process: nm - 1 steps forward from the start points, then nm - 1 steps
backward from the end of that orbit.  Host clock around whole calls, the two directions alternately, median of --reps.  One JSON
line per case.
    python tools/mapinv_speed.py [--reps R] [CASE ...]       CASE = n0:d:Ntest:nm
    default: n0 = 20, 40, 80 (the drivers' sizes) with 1000 rows, 1024 and 1025 (the last staged size, the first from memory) with
             200, 16384 with 20, each at d = 1, 2, 3 and 37 orbits
The model: a backward step runs the passes of a forward step -- the same x = (q, P), the same sums, the transposed d x d solve --
so with equal iteration counts the ratio backward / forward is 1.0 within run-to-run noise.  The line reports the measured ratio
beside the counts and the passes of both directions (a pass is one sweep of an orbit over the n0 training points), the ratio per
pass of the slowest orbit -- the orbits run side by side, so that orbit sets the time of the call --, and how far the backward
orbit is from the forward one after 10 steps and at its end.  The latter measures the orbits, not the kernel: over hundreds of
steps a chaotic orbit of the learned map amplifies the last bit of its end point to order 1 in either direction.  No threshold:
a record, not a test.
Training data: up to n0 = 2048 the smooth generating function of tests/test_gpu_applymap_nd.py on bench.py's synthetic points
and length scales, alpha from the fit (SympFit.pairs); above, random alpha ~ 0.1 / sqrt(n0) on the same points with the lengths
1.2 / 1.5 (the recipe of that file's test_kernel_edges), which needs no factorisation of order 2 d n0."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sympgpr_amd import maps
from sympgpr_amd.fit import SympFit
from bench import synth_pairs

DEFAULT = ["%d:%d:37:%d" % (n0, d, nm) for n0, nm in ((20, 1000), (40, 1000), (80, 1000), (1024, 200), (1025, 200), (16384, 20))
           for d in (1, 2, 3)]
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("cases", nargs="*", default=DEFAULT)
a = ap.parse_args()
FIT_MAX = 2048


def training(n0, d, eps=0.25, c=0.4):
    X, _, hyp, s2 = synth_pairs(n0, d)
    q, P = X[:, :d], X[:, d:] / 3.0
    s, h = q.sum(axis=1), 1.0 + 0.5 * (P * P).sum(axis=1)
    Fq = -eps * np.sin(q) - (c * eps * np.sin(s) * h)[:, None]
    FP = eps * P + (c * eps * np.cos(s))[:, None] * P
    return np.hstack((q, P)), np.concatenate((Fq.T.ravel(), FP.T.ravel())), hyp, s2


def passes(it):
    """Newton passes + the closing pass of every accepted step -> (all orbits together, the orbit with the most).  The orbits
    run side by side, one workgroup each on a CU of its own (Ntest = 37 of 256), so a call lasts as long as its slowest orbit."""
    per_orbit = np.where(it > 0, it, 0).sum(axis=0) + (it >= 0).sum(axis=0)
    return int(per_orbit.sum()), int(per_orbit.max())


for case in a.cases:
    n0, d, Ntest, nm = (int(v) for v in case.split(":"))
    X, z, hyp, s2 = training(n0, d)
    if n0 > FIT_MAX:                                      # test_kernel_edges' lengths with its alpha: G stays small, every orbit converges
        hyp = np.array((1.2,) * d + (1.5,) * d + (1.0,))
    if n0 <= FIT_MAX:
        with SympFit.pairs("A", X, z, hyp, s2) as f:
            alpha = f.run().alpha()
    else:
        alpha = np.random.default_rng(100 + n0).standard_normal(2 * d * n0) * 0.1 / np.sqrt(n0)
    rng = np.random.default_rng(5)
    Q0, P0 = rng.uniform(0.5, 5.5, (Ntest, d)), rng.uniform(-0.6, 0.6, (Ntest, d))
    args = ("A", d, 0, nm, hyp, X, alpha)
    qf, pf = maps.run_map_nd(*args, Q0, P0)               # warm-up of both directions (code object load, first allocations)
    maps.run_map_nd_inverse("A", d, 0, 2, hyp, X, alpha, qf[-1], pf[-1])
    t_f, t_b = [], []
    for r in range(a.reps):
        t0 = time.perf_counter()
        qf, pf, itf = maps.run_map_nd(*args, Q0, P0, return_iters=True)
        t_f.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        qb, pb, itb = maps.run_map_nd_inverse(*args, qf[-1], pf[-1], return_iters=True)
        t_b.append(time.perf_counter() - t0)
    ok = (itf[-1] >= 0) & (itb[-1] >= 0)                   # orbits neither direction lost
    back = float(max(np.abs(qb[-1][ok] - Q0[ok]).max(), np.abs(pb[-1][ok] - P0[ok]).max())) if ok.any() else None
    k = min(10, nm - 1)                                   # ... and after the first k backward steps: row k against forward row nm - 1 - k
    back_k = float(max(np.abs(qb[k][ok] - qf[nm - 1 - k][ok]).max(), np.abs(pb[k][ok] - pf[nm - 1 - k][ok]).max())) if ok.any() else None
    f_s, b_s, (pf_, sf_), (pb_, sb_) = float(np.median(t_f)), float(np.median(t_b)), passes(itf), passes(itb)
    print(json.dumps({"tool": "mapinv_speed", "family": "A", "n0": n0, "d": d, "Ntest": Ntest, "nm": nm,
                      "alpha": "fit" if n0 <= FIT_MAX else "random",
                      "forward_lost": int((itf[-1] < 0).sum()), "backward_lost": int((itb[-1] < 0).sum()),
                      "forward_iters_mean": round(float(itf[itf > 0].mean()), 2), "forward_iters_max": int(itf.max()),
                      "backward_iters_mean": round(float(itb[itb > 0].mean()), 2), "backward_iters_max": int(itb.max()),
                      "forward_passes": pf_, "backward_passes": pb_,
                      "forward_passes_slowest_orbit": sf_, "backward_passes_slowest_orbit": sb_,
                      "forward_ms_per_call": round(f_s * 1e3, 3), "backward_ms_per_call": round(b_s * 1e3, 3),
                      "forward_ms_calls": [round(v * 1e3, 3) for v in t_f], "backward_ms_calls": [round(v * 1e3, 3) for v in t_b],
                      "backward_over_forward": round(b_s / f_s, 3),
                      "backward_over_forward_per_pass_of_slowest_orbit": round((b_s / sb_) / (f_s / sf_), 3) if sf_ and sb_ else None,
                      "round_trip_steps": k, "round_trip_max_abs": back_k, "round_trip_whole_orbit_max_abs": back}), flush=True)
