"""Problems per second of the batched NLL gradient (sgpr_fit_batch_grad) beside the same process's sgpr_fit_batch, and ms per
problem of the per-row SympFit(...).run().nll_grad_full() loop it replaces:
    python tools/batchgrad_speed.py [--orders 80,140,160,256] [--batches 64,1024] [--loop 16] [--fam C] [--out FILE]
Pair fits and reg fits at every order; host clock around whole calls after one warm-up, median of 5.  One JSON line per
(order, kind, batch) is printed and, with --out, appended to FILE (profiles/batchgrad/)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sympgpr_amd.fit import SympFit, fit_batch, fit_batch_grad

ap = argparse.ArgumentParser()
ap.add_argument("--orders", default="80,140,160,256")
ap.add_argument("--batches", default="64,1024")
ap.add_argument("--loop", type=int, default=16, help="rows of the per-row nll_grad_full loop")
ap.add_argument("--fam", default="C")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()


def median_s(f):
    f()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


rng = np.random.default_rng(5)
for n in (int(v) for v in a.orders.split(",")):
    for reg in (False, True):
        npts = n if reg else n // 2
        Bmax = max(int(v) for v in a.batches.split(","))
        X, Y = rng.uniform(0, 2 * np.pi, (Bmax, npts)), rng.uniform(-3, 3, (Bmax, npts))
        Z = rng.standard_normal((Bmax, n))
        l = 2.0 * np.sqrt(12 * np.pi) * n ** -0.5
        H = np.array([0.9 * l, 1.1 * l, 1.3]) * rng.uniform(0.9, 1.1, (Bmax, 3))
        S2 = np.full(Bmax, 1e-2 / l**2)
        rec = {"order": n, "kind": "reg" if reg else "pair", "family": a.fam}
        k = a.loop

        def loop():
            for b in range(k):
                with SympFit(a.fam, X[b], Y[b], Z[b], H[b], S2[b], reg=reg) as f:
                    f.run().nll_grad_full()
        t_loop = median_s(loop)
        for B in (int(v) for v in a.batches.split(",")):
            t_fit = median_s(lambda: fit_batch(a.fam, X[:B], Y[:B], Z[:B], H[:B], S2[:B], reg=reg, want_alpha=False))
            t_grad = median_s(lambda: fit_batch_grad(a.fam, X[:B], Y[:B], Z[:B], H[:B], S2[:B], reg=reg))
            r = dict(rec, batch=B, fit_batch_per_s=B / t_fit, fit_batch_grad_per_s=B / t_grad,
                     grad_over_fit=t_fit / t_grad, call_ms_fit=t_fit * 1e3, call_ms_grad=t_grad * 1e3,
                     loop_rows=k, loop_ms_per_problem=t_loop / k * 1e3,
                     speedup_vs_loop=(t_loop / k) / (t_grad / B))
            line = json.dumps(r)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as fh:
                    fh.write(line + "\n")
