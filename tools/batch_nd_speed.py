"""The batched d-pair fit (sgpr_fit_batch_nd) against its two yardsticks, in one process: sgpr_fit_batch at the same matrix order
and batch (d = 1: the factorisation and solves are the same code, so the difference is the Gram stage and the input copy), and
the loop its users had before -- one resident SympFit.pairs handle, set_hyp / run / nll per row (--loop-rows rows timed, scaled
to the batch).  Host clock around whole calls (each ends in a stream synchronise), --warmup calls first, then --reps timed calls
with the compared entries alternating; median, minimum and maximum.  One JSON line per case, appended to
profiles/batch_nd/batch_nd_speed.jsonl (--out).
    python tools/batch_nd_speed.py [--fam A] [--batch B] D:N [D:N ...]      e.g. 2:20 2:40 2:64 3:13 3:27 3:42 --batch 1024"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sympgpr_amd.fit import SympFit, fit_batch, fit_batch_pairs
ap = argparse.ArgumentParser()
ap.add_argument("--fam", default="A")
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--loop-rows", type=int, default=64)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_nd", "batch_nd_speed.jsonl"))
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
    # the d = 1 yardstick: the same order and batch, n / 2 points per problem
    x1, y1 = rng.uniform(0, 2 * np.pi, (B, n // 2)), rng.uniform(-3, 3, (B, n // 2))
    l1 = 1.2 * (12 * np.pi / (n // 2)) ** 0.5 * rng.uniform(0.8, 1.25, B)
    hyp1 = np.column_stack([l1, l1] + ([np.full(B, 0.5)] if a.fam == "D" else []) + [np.ones(B)])
    calls = {"nd": lambda: fit_batch_pairs(a.fam, X, z, hyp, s2, want_alpha=False),
             "d1": lambda: fit_batch(a.fam, x1, y1, z, hyp1, 1e-2 / l1**2, want_alpha=False)}
    t = {"nd": [], "d1": []}
    for r in range(a.warmup + a.reps):
        for name, call in calls.items():
            t0 = time.perf_counter()
            _, nll, info = call()
            if r >= a.warmup:
                t[name].append((time.perf_counter() - t0) * 1e3)
            if np.count_nonzero(info):
                raise SystemExit("%s: a problem of the benchmark is not positive definite" % name)
    rows = min(a.loop_rows, B)
    with SympFit.pairs(a.fam, X[0], z[0], hyp[0], s2[0]) as f:
        f.run().nll()                                  # warm-up: allocations, first launches
        loop = []
        for r in range(3):
            t0 = time.perf_counter()
            for b in range(rows):
                f.set_hyp(hyp[b], s2[b])
                f.run().nll()
            loop.append((time.perf_counter() - t0) * 1e3 * B / rows)
    nd, d1, lp = stats(t["nd"]), stats(t["d1"]), stats(loop)
    rec = {"tool": "batch_nd_speed", "fam": a.fam, "d": d, "n_pts": N, "n": n, "batch": B, "path": "one launch" if n <= 256 else "mid",
           "warmup": a.warmup, "reps": a.reps, "fit_batch_nd": nd, "fit_batch_same_order": d1,
           "handle_loop_scaled": dict(lp, rows_timed=rows, reps=3),
           "nd_over_fit_batch": round(nd["median_ms"] / d1["median_ms"], 3),
           "handle_loop_over_nd": round(lp["median_ms"] / nd["median_ms"], 2),
           "fits_per_s": round(B / nd["median_ms"] * 1e3, 1)}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")
