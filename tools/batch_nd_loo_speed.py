"""The batched d-pair leave-one-point-out entries (sgpr_fit_batch_nd_loo, sgpr_fit_batch_nd_loo_grad) against their yardsticks, in
one process: fit_batch_pairs at the same shape (the fit alone), the d = 1 entries fit_batch_loo / fit_batch_loo_grad on problems of
the SAME ORDER given as x | y (d N points), and the loop its users had before -- one resident SympFit.pairs handle, set_hyp / run /
loo [/ loo_grad] per row (--loop-rows rows timed, scaled to the batch).  The gradient entries are timed up to order 256 (above it
both are row-by-row slow paths).  Host clock around whole calls (each ends in a stream synchronise), --warmup calls first, then
--reps timed calls with the compared entries alternating; median, minimum and maximum.  One JSON line per case, appended to
profiles/batch_nd_loo/batch_nd_loo_speed.jsonl (--out).
    python tools/batch_nd_loo_speed.py [--fam A] [--batch B] D:N [D:N ...]
        e.g. --batch 1024 2:20 2:40 2:64 3:13 3:27 3:42      and      --batch 64 2:128 2:256 2:512 3:171 3:341"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sympgpr_amd.fit import (SympFit, fit_batch_loo, fit_batch_loo_grad, fit_batch_pairs, fit_batch_pairs_loo,
                             fit_batch_pairs_loo_grad)
ap = argparse.ArgumentParser()
ap.add_argument("--fam", default="A")
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--loop-rows", type=int, default=64)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_nd_loo", "batch_nd_loo_speed.jsonl"))
ap.add_argument("cases", nargs="+", help="d:N -- pairs per point and points per problem (order 2 d N)")
a = ap.parse_args()


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def draw(rng, B, N, d):
    """B problems with d pairs per point: X (B, N, 2d), z, hyp, s2"""
    X = np.concatenate([rng.uniform(0, 2 * np.pi, (B, N, d)), rng.uniform(-3, 3, (B, N, d))], axis=2)
    z = rng.standard_normal((B, 2 * d * N))
    l = 1.2 * (12 * np.pi / N) ** (1.0 / (2 * d)) * rng.uniform(0.8, 1.25, B)
    hyp = np.hstack([np.tile(l[:, None], (1, 2 * d))] + ([np.full((B, d), 0.5)] if a.fam == "D" else []) + [np.ones((B, 1))])
    return X, z, hyp, 1e-2 / l**2


for case in a.cases:
    d, N = (int(v) for v in case.split(":"))
    n, B = 2 * d * N, a.batch
    small = n <= 256
    X, z, hyp, s2 = draw(np.random.default_rng(77), B, N, d)
    X1, z1, hyp1, s21 = draw(np.random.default_rng(78), B, d * N, 1)          # d = 1 at the same order
    x1, y1 = np.ascontiguousarray(X1[:, :, 0]), np.ascontiguousarray(X1[:, :, 1])
    calls = {"fit": lambda: fit_batch_pairs(a.fam, X, z, hyp, s2, want_alpha=False)[1:],
             "loo": lambda: fit_batch_pairs_loo(a.fam, X, z, hyp, s2)[1:],
             "loo_d1": lambda: fit_batch_loo(a.fam, x1, y1, z1, hyp1, s21)[1:]}
    if small:
        calls["loo_grad"] = lambda: fit_batch_pairs_loo_grad(a.fam, X, z, hyp, s2)[1:]
        calls["loo_grad_d1"] = lambda: fit_batch_loo_grad(a.fam, x1, y1, z1, hyp1, s21)[1:]
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
    loops = {"loo": [], "loo_grad": []}
    with SympFit.pairs(a.fam, X[0], z[0], hyp[0], s2[0]) as f:
        f.run().loo(resid=False, lpd=False)            # warm-up: allocations, first launches
        f.loo_grad()
        for r in range(3):
            t0 = time.perf_counter()
            for b in range(rows):
                f.set_hyp(hyp[b], s2[b])
                f.run().loo(resid=False, lpd=False)
            loops["loo"].append((time.perf_counter() - t0) * 1e3 * B / rows)
        for r in range(3 if small else 0):
            t0 = time.perf_counter()
            for b in range(rows):
                f.set_hyp(hyp[b], s2[b])
                f.run().loo_grad()
            loops["loo_grad"].append((time.perf_counter() - t0) * 1e3 * B / rows)
    st = {name: stats(ts) for name, ts in t.items()}
    lp = stats(loops["loo"])
    rec = {"tool": "batch_nd_loo_speed", "fam": a.fam, "d": d, "n_pts": N, "n": n, "batch": B,
           "path": "one launch" if small else "mid", "warmup": a.warmup, "reps": a.reps,
           "fit_batch_nd": st["fit"], "fit_batch_nd_loo": st["loo"], "fit_batch_loo_d1_same_order": dict(st["loo_d1"], n_pts=d * N),
           "handle_loop_loo_scaled": dict(lp, rows_timed=rows, reps=3),
           "loo_over_fit_time": round(st["loo"]["median_ms"] / st["fit"]["median_ms"], 2),
           "nd_loo_over_d1_loo": round(st["loo"]["median_ms"] / st["loo_d1"]["median_ms"], 3),
           "handle_loop_over_loo": round(lp["median_ms"] / st["loo"]["median_ms"], 2)}
    if small:
        lg = stats(loops["loo_grad"])
        rec.update({"fit_batch_nd_loo_grad": st["loo_grad"],
                    "fit_batch_loo_grad_d1_same_order": dict(st["loo_grad_d1"], n_pts=d * N),
                    "handle_loop_loo_grad_scaled": dict(lg, rows_timed=rows, reps=3),
                    "loo_grad_over_fit_time": round(st["loo_grad"]["median_ms"] / st["fit"]["median_ms"], 2),
                    "nd_loo_grad_over_d1_loo_grad": round(st["loo_grad"]["median_ms"] / st["loo_grad_d1"]["median_ms"], 3),
                    "handle_loop_over_loo_grad": round(lg["median_ms"] / st["loo_grad"]["median_ms"], 2)})
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")
