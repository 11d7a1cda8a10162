"""The d-pair symplectic map on the device (SympFit.applymap_pairs: sgpr_fit_applymap_nd, one launch for all steps) against
the only route there was before it: the same Newton iteration driven from the host through SympFit.predict_pairs -- one call
per residual for all orbits at once, a forward-difference Jacobian (1 + d residuals per iteration), one more call for the Q
update.  Host clock around whole calls, the two routes alternately in one process, median of --reps.  One JSON line per case.
    python tools/mapnd_speed.py [--reps R] [--host-steps S] [CASE ...]       CASE = n0:d:Ntest:nm, default 64:2:37:1000 16384:3:37:20
Training data: the smooth generating function of tests/test_gpu_applymap_nd.py on bench.py's synthetic points and length
scales, so every orbit converges.  A pass is one sweep of an orbit over the n0 training points (one K* row block times alpha,
with or without the Jacobian sums): pair evaluations = n0 x passes, counted from the returned iteration counts."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sympgpr_amd.fit import SympFit
from bench import synth_pairs

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--host-steps", type=int, default=20, help="steps of the host-driven route per timing (it is slow)")
ap.add_argument("cases", nargs="*", default=["64:2:37:1000", "16384:3:37:20"])
a = ap.parse_args()


def training(n0, d, eps=0.25, c=0.4):
    X, _, hyp, s2 = synth_pairs(n0, d)
    q, P = X[:, :d], X[:, d:] / 3.0
    s, h = q.sum(axis=1), 1.0 + 0.5 * (P * P).sum(axis=1)
    Fq = -eps * np.sin(q) - (c * eps * np.sin(s) * h)[:, None]
    FP = eps * P + (c * eps * np.cos(s))[:, None] * P
    return np.hstack((q, P)), np.concatenate((Fq.T.ravel(), FP.T.ravel())), hyp, s2


def host_map(f, d, nm, Q0, P0, tol=1e-13, maxiter=60, h=1e-7):
    """-> (qmap, pmap, predict_pairs calls, Newton iterations of every step): Newton on G_q(q, P) - p + P = 0 for all orbits together, from P = p"""
    q, p = Q0.copy(), P0.copy()
    qs, ps, calls, its = [q.copy()], [p.copy()], 0, []
    for _ in range(nm - 1):
        P = p.copy()
        for it in range(maxiter):
            f0 = f.predict_pairs(np.hstack((q, P)))[:, :d] - p + P
            calls += 1
            J = np.empty((len(q), d, d))
            for e in range(d):
                Ph = P.copy()
                Ph[:, e] += h
                J[:, :, e] = ((f.predict_pairs(np.hstack((q, Ph)))[:, :d] - p + Ph) - f0) / h
                calls += 1
            dP = -np.linalg.solve(J, f0[:, :, None])[:, :, 0]
            P += dP
            if np.abs(dP).max() <= tol * max(1.0, np.abs(P).max()) or it >= 8:     # (a forward-difference Jacobian stalls near 1e-13)
                break
        its.append(it + 1)
        q = q + f.predict_pairs(np.hstack((q, P)))[:, d:]
        calls += 1
        p = P
        qs.append(q.copy())
        ps.append(p.copy())
    return np.array(qs), np.array(ps), calls, its


for case in a.cases:
    n0, d, Ntest, nm = (int(v) for v in case.split(":"))
    X, z, hyp, s2 = training(n0, d)
    rng = np.random.default_rng(5)
    Q0, P0 = rng.uniform(0.5, 5.5, (Ntest, d)), rng.uniform(-0.6, 0.6, (Ntest, d))
    hs = min(a.host_steps, nm - 1)
    with SympFit.pairs("A", X, z, hyp, s2) as f:
        f.run()
        f.applymap_pairs(2, Q0, P0)                       # warm-up of both routes (code object load, first allocations)
        host_map(f, d, 2, Q0, P0)
        t_dev, t_host = [], []
        for r in range(a.reps):
            t0 = time.perf_counter()
            qd, pd, it = f.applymap_pairs(nm, Q0, P0, return_iters=True)
            t_dev.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            qh, ph, calls, hits = host_map(f, d, hs + 1, Q0, P0)
            t_host.append(time.perf_counter() - t0)
    lost = int((it[-1] < 0).sum()) if nm > 1 else 0
    passes = int(it[it > 0].sum() + (it >= 0).sum())     # Newton passes + the closing pass of every accepted step
    dev_s, host_s = float(np.median(t_dev)), float(np.median(t_host))
    dev_step, host_step = dev_s / (nm - 1), host_s / hs
    print(json.dumps({"tool": "mapnd_speed", "family": "A", "n0": n0, "d": d, "Ntest": Ntest, "nm": nm, "lost_orbits": lost,
                      "newton_iters_max": int(it.max()), "newton_iters_mean": round(float(it[it > 0].mean()), 2),
                      "passes": passes, "device_ms_per_call": round(dev_s * 1e3, 3),
                      "device_ms_calls": [round(v * 1e3, 3) for v in t_dev], "device_ms_per_step": round(dev_step * 1e3, 5),
                      "device_G_pair_evals_per_s": round(n0 * passes / dev_s / 1e9, 3),
                      "host_steps_timed": hs, "host_predict_calls": calls, "host_newton_iters_min": min(hits),
                      "host_newton_iters_max": max(hits), "host_newton_iters_cap": 9, "host_ms_per_step": round(host_step * 1e3, 3),
                      "host_ms_calls": [round(v * 1e3, 3) for v in t_host],
                      "host_over_device_per_step": round(host_step / dev_step, 1),
                      "max_abs_diff_first_steps": float(max(np.abs(qd[:hs + 1] - qh).max(), np.abs(pd[:hs + 1] - ph).max()))}),
          flush=True)
