"""The batched d-pair NLL gradient (sgpr_fit_batch_nd_grad) against its yardsticks, in one process: the loop its users had before --
one resident SympFit.pairs handle, set_hyp / run / nll / nll_grad_full per row (--loop-rows rows timed, scaled to the batch) --
and fit_batch_pairs at the same shape (the fit alone: what the gradient phase costs on top).  A case with d = 1 also times
fit_batch_grad (order <= 256) or fit_batch_grad_mid on the same problems given as x | y: the d = 1 contraction beside the d-pair
one.  Host clock around whole calls (each ends in a stream synchronise), --warmup calls first, then --reps timed calls with the
compared entries alternating; median, minimum and maximum.  One JSON line per case, appended to
profiles/batch_nd_grad/batch_nd_grad_speed.jsonl (--out).
    python tools/batch_nd_grad_speed.py [--fam A] [--batch B] D:N [D:N ...]
        e.g. --batch 1024 2:20 2:40 2:64 3:13 3:27 3:42 1:40 1:128      and      --batch 64 2:128 2:256 2:512 3:171 3:341 1:512"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sympgpr_amd.fit import SympFit, fit_batch_grad, fit_batch_grad_mid, fit_batch_pairs, fit_batch_pairs_grad
ap = argparse.ArgumentParser()
ap.add_argument("--fam", default="A")
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--loop-rows", type=int, default=64)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_nd_grad", "batch_nd_grad_speed.jsonl"))
ap.add_argument("cases", nargs="+", help="d:N -- pairs per point and points per problem (order 2 d N)")
a = ap.parse_args()


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


for case in a.cases:
    d, N = (int(v) for v in case.split(":"))
    n, B = 2 * d * N, a.batch
    rng = np.random.default_rng(77)
    X = np.concatenate([rng.uniform(0, 2 * np.pi, (B, N, d)), rng.uniform(-3, 3, (B, N, d))], axis=2)
    z = rng.standard_normal((B, n))
    l = 1.2 * (12 * np.pi / N) ** (1.0 / (2 * d)) * rng.uniform(0.8, 1.25, B)
    hyp = np.hstack([np.tile(l[:, None], (1, 2 * d))] + ([np.full((B, d), 0.5)] if a.fam == "D" else []) + [np.ones((B, 1))])
    s2 = 1e-2 / l**2
    calls = {"grad": lambda: fit_batch_pairs_grad(a.fam, X, z, hyp, s2)[1:],
             "fit": lambda: fit_batch_pairs(a.fam, X, z, hyp, s2, want_alpha=False)[1:]}
    if d == 1:
        x1, y1 = np.ascontiguousarray(X[:, :, 0]), np.ascontiguousarray(X[:, :, 1])
        xy = fit_batch_grad if n <= 256 else fit_batch_grad_mid
        calls["xy"] = lambda: xy(a.fam, x1, y1, z, hyp, s2)[1:]
    t = {name: [] for name in calls}
    for r in range(a.warmup + a.reps):
        for name, call in calls.items():
            t0 = time.perf_counter()
            out = call()
            if r >= a.warmup:
                t[name].append((time.perf_counter() - t0) * 1e3)
            if np.count_nonzero(out[-1]):
                raise SystemExit("%s: a problem of the benchmark is not positive definite" % name)
    rows = min(a.loop_rows, B)
    with SympFit.pairs(a.fam, X[0], z[0], hyp[0], s2[0]) as f:
        f.run().nll()                                  # warm-up: allocations, first launches
        f.nll_grad_full()
        loop = []
        for r in range(3):
            t0 = time.perf_counter()
            for b in range(rows):
                f.set_hyp(hyp[b], s2[b])
                f.run().nll()
                f.nll_grad_full()
            loop.append((time.perf_counter() - t0) * 1e3 * B / rows)
    g, ft, lp = stats(t["grad"]), stats(t["fit"]), stats(loop)
    rec = {"tool": "batch_nd_grad_speed", "fam": a.fam, "d": d, "n_pts": N, "n": n, "batch": B,
           "path": "one launch" if n <= 256 else "mid", "warmup": a.warmup, "reps": a.reps,
           "fit_batch_nd_grad": g, "fit_batch_nd": ft, "handle_loop_scaled": dict(lp, rows_timed=rows, reps=3),
           "handle_loop_over_grad": round(lp["median_ms"] / g["median_ms"], 2),
           "grad_rate_over_fit_rate": round(ft["median_ms"] / g["median_ms"], 3),
           "grad_over_fit_time": round(g["median_ms"] / ft["median_ms"], 2),
           "grads_per_s": round(B / g["median_ms"] * 1e3, 1)}
    if d == 1:
        xs = stats(t["xy"])
        rec["fit_batch_grad_xy"] = dict(xs, entry=xy.__name__)
        rec["nd_grad_over_xy_grad"] = round(g["median_ms"] / xs["median_ms"], 3)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")
