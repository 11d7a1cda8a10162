"""Predictive covariance (sgpr_fit_predict_cov) after one factorisation: host clock around whole calls (each ends in a stream
synchronise), per forward pass of 64 right-hand-side columns, against the same process's 64-column forward + backward block
solve (sgpr_fit_solve_rhs, its device time).  One JSON line per matrix order.
    python tools/predcov_speed.py [--d D] [--m M] [--reg] N [N ...]        N = matrix order: N / (2 d) points, N with --reg
A pass reads the lower triangle of L once (4 n^2 bytes); l_read_GBps is that over the measured time per pass, which also
carries the chunk's Gram builds, the reduction and the mean."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sympgpr_amd.fit import SympFit
from bench import synth, synth_pairs
ap = argparse.ArgumentParser()
ap.add_argument("--d", type=int, default=1)
ap.add_argument("--m", type=int, default=320, help="test points per call")
ap.add_argument("--reg", action="store_true", help="the scalar-kernel GP (D = 1 output per point; d = 1 only)")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("n", type=int, nargs="+", help="matrix orders")
a = ap.parse_args()
if a.reg and a.d != 1:
    sys.exit("--reg needs d = 1")
D = 1 if a.reg else 2 * a.d
for n in a.n:
    npts = n if a.reg else n // (2 * a.d)
    rng = np.random.default_rng(77)
    if a.d == 1:
        q, P, z, hyp, s2 = synth(npts)
        f = SympFit("A", q, P, z[:npts] if a.reg else z, hyp, s2, reg=a.reg)
        Xt = np.column_stack((rng.uniform(0, 2 * np.pi, a.m), rng.uniform(-3, 3, a.m)))
    else:
        X, z, hyp, s2 = synth_pairs(npts, a.d)
        f = SympFit.pairs("A", X, z, hyp, s2)
        Xt = np.column_stack([rng.uniform(0, 2 * np.pi, (a.m, a.d)), rng.uniform(-3, 3, (a.m, a.d))])
    call = (lambda: f.predict_pairs_cov(Xt)) if a.d > 1 else (lambda: f.predict_cov(Xt[:, 0], Xt[:, 1]))
    with f:
        f.run()
        ts = []
        for r in range(2 + a.reps):
            t0 = time.perf_counter()
            mean, cov = call()
            if r >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)
        B = rng.standard_normal((f.n, 64))
        rhs = []
        for r in range(1 + a.reps):
            f.solve_rhs(B)
            if r:
                rhs.append(f.solve_rhs_ms())
        nn = f.n
    mc = 256 // D
    chunks = [min(mc, a.m - c0) for c0 in range(0, a.m, mc)]
    passes = sum((D * c + 63) // 64 for c in chunks)
    ms = float(np.median(ts))
    ms_pass = ms / passes
    rhs_ms = float(np.median(rhs))
    print(json.dumps({"tool": "predcov_speed", "n": nn, "d": a.d, "reg": a.reg, "m": a.m, "D": D, "chunks": len(chunks),
                      "passes": passes, "ms_per_call": round(ms, 3), "ms_calls": [round(v, 3) for v in ts],
                      "ms_per_pass": round(ms_pass, 3), "solve_rhs64_ms": round(rhs_ms, 3),
                      "pass_over_solve_rhs64": round(ms_pass / rhs_ms, 4),
                      "l_read_GBps_per_pass": round(4.0 * nn * nn / (ms_pass * 1e-3) / 1e9, 1),
                      "min_diag_var": float(np.diagonal(cov, axis1=1, axis2=2).min())}), flush=True)
