"""Whole-call time of the mid-order batched NLL gradient (sgpr_fit_batch_grad_mid) beside the same process's sgpr_fit_batch and
the handle-per-row slow path of fit.fit_batch_grad it replaces:
    python tools/batchgrad_mid_speed.py [--orders 512,1024,2048] [--batch 64] [--reps 3] [--fam C] [--no-slow] [--out FILE]
Pair fits; host clock around whole calls; after one warm-up of each, the three are measured alternately (grad_mid, fit_batch,
slow path, grad_mid, ...) and the median of --reps is kept.  One JSON line per order is printed and, with --out, appended to FILE
(profiles/batchgrad_mid/).  --no-slow leaves the slow path out (a kernel trace of the new path alone)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sympgpr_amd.fit import fit_batch, fit_batch_grad, fit_batch_grad_mid

ap = argparse.ArgumentParser()
ap.add_argument("--orders", default="512,1024,2048")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--fam", default="C")
ap.add_argument("--no-slow", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()

rng = np.random.default_rng(5)
B = a.batch
for n in (int(v) for v in a.orders.split(",")):
    npts = n // 2
    X, Y = rng.uniform(0, 2 * np.pi, (B, npts)), rng.uniform(-3, 3, (B, npts))
    Z = rng.standard_normal((B, n))
    l = 2.0 * np.sqrt(12 * np.pi) * n ** -0.5
    H = np.array([0.9 * l, 1.1 * l, 1.3]) * rng.uniform(0.9, 1.1, (B, 3))
    S2 = np.full(B, 1e-2 / l**2)
    calls = {"grad_mid": lambda: fit_batch_grad_mid(a.fam, X, Y, Z, H, S2),
             "fit": lambda: fit_batch(a.fam, X, Y, Z, H, S2, want_alpha=False)}
    if not a.no_slow:
        calls["slow"] = lambda: fit_batch_grad(a.fam, X, Y, Z, H, S2)
    ts = {k: [] for k in calls}
    for f in calls.values():
        f()
    for _ in range(a.reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            ts[k].append(time.perf_counter() - t0)
    t = {k: float(np.median(v)) for k, v in ts.items()}
    r = {"order": n, "kind": "pair", "family": a.fam, "batch": B, "reps": a.reps,
         "call_ms_grad_mid": t["grad_mid"] * 1e3, "call_ms_fit": t["fit"] * 1e3, "grad_mid_over_fit": t["grad_mid"] / t["fit"],
         "grad_mid_per_s": B / t["grad_mid"]}
    if "slow" in t:
        r.update(call_ms_slow=t["slow"] * 1e3, slow_over_grad_mid=t["slow"] / t["grad_mid"])
    line = json.dumps(r)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
