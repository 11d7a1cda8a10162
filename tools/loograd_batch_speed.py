"""Whole-call time of the batched leave-one-point-out gradient (sgpr_fit_batch_loo_grad) beside the same process's
sgpr_fit_batch_loo and sgpr_fit_batch_grad, and the per-row func.loo_chol_grad loop (a device-resident handle per row) it replaces:
    python tools/loograd_batch_speed.py [--orders 80,140] [--batch 1024] [--loop 64] [--fam C] [--reps 5] [--out FILE]
Pair fits; host clock around whole calls after one warm-up, median of --reps, the three batched calls measured alternately.  The
handle loop is timed on at most --loop rows and scaled to the batch; the line says so.  One JSON line per order is printed and,
with --out, appended to FILE (profiles/loograd_batch/)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sympgpr_amd import func
from sympgpr_amd.fit import fit_batch_grad, fit_batch_loo, fit_batch_loo_grad

ap = argparse.ArgumentParser()
ap.add_argument("--orders", default="80,140")
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--loop", type=int, default=64, help="rows of the per-row loo_chol_grad loop (at most)")
ap.add_argument("--fam", default="C")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()

rng = np.random.default_rng(5)
func.set_family(a.fam)
B = a.batch
for n in (int(v) for v in a.orders.split(",")):
    npts = n // 2
    X, Y = rng.uniform(0, 2 * np.pi, (B, npts)), rng.uniform(-3, 3, (B, npts))
    Z = rng.standard_normal((B, n))
    l = 2.0 * np.sqrt(12 * np.pi) * n ** -0.5
    H = np.array([0.9 * l, 1.1 * l, 1.3]) * rng.uniform(0.9, 1.1, (B, 3))
    S2 = np.full(B, 1e-2 / l**2)
    calls = {"loo_grad": lambda: fit_batch_loo_grad(a.fam, X, Y, Z, H, S2),
             "loo": lambda: fit_batch_loo(a.fam, X, Y, Z, H, S2),
             "grad": lambda: fit_batch_grad(a.fam, X, Y, Z, H, S2)}
    k = min(a.loop, B)

    def loop():
        for b in range(k):
            func.loo_chol_grad(np.append(H[b], S2[b]), np.concatenate([X[b], Y[b]]), Z[b], n)
    calls["loop"] = loop
    for f in calls.values():
        f()                                   # warm-up: arena growth, handle pools
    ts = {name: [] for name in calls}
    for _ in range(a.reps):
        for name, f in calls.items():
            t0 = time.perf_counter()
            f()
            ts[name].append(time.perf_counter() - t0)
    t = {name: float(np.median(v)) for name, v in ts.items()}
    t_loop = t["loop"] / k * B
    r = {"order": n, "kind": "pair", "family": a.fam, "batch": B, "reps": a.reps,
         "call_ms_loo_grad": t["loo_grad"] * 1e3, "call_ms_loo": t["loo"] * 1e3, "call_ms_grad": t["grad"] * 1e3,
         "loop_rows": k, "loop_ms_per_problem": t["loop"] / k * 1e3, "loop_ms_scaled_to_batch": t_loop * 1e3,
         "loop_note": "timed on %d rows, scaled to %d" % (k, B),
         "loo_grad_per_s": B / t["loo_grad"], "loo_grad_over_grad": t["loo_grad"] / t["grad"],
         "speedup_vs_loop": t_loop / t["loo_grad"]}
    line = json.dumps(r)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
