"""Whole-call time of the mid-order batched leave-one-point-out gradient (sgpr_fit_batch_loo_grad_mid and
sgpr_fit_batch_nd_loo_grad_mid) beside, in the same process and at the same shape, the batched loo values, the batched NLL gradient
and the handle loop the new entries replace:
    python tools/loograd_mid_speed.py [--orders 512,1024,2048] [--batch 64] [--reps 7] [--warm 2] [--rows 16] [--kinds pair,d2]
                                      [--only-new] [--out FILE]
kind pair: family C, points as x | y; kind d2: family A, d = 2 canonical pairs per point.  Host clock around whole calls, each ended
by a device synchronise; after --warm calls of each, the calls are measured alternately (new, loo, nll gradient, handle loop, new,
...) and the median of --reps is kept.  The handle loop is set_hyp / run / loo_grad over ONE resident handle for --rows rows,
scaled to the batch.  One JSON line per kind and order is printed and, with --out, appended to FILE (profiles/loograd_mid/).
--only-new leaves everything but the new entry out (a kernel trace of the new path alone)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sympgpr_amd.fit import (SympFit, fit_batch_grad_mid, fit_batch_loo, fit_batch_loo_grad_mid, fit_batch_pairs_grad,
                             fit_batch_pairs_loo, fit_batch_pairs_loo_grad_mid)

ap = argparse.ArgumentParser()
ap.add_argument("--orders", default="512,1024,2048")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--rows", type=int, default=16)
ap.add_argument("--kinds", default="pair,d2")
ap.add_argument("--only-new", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()

rng = np.random.default_rng(5)
B = a.batch


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


for kind in a.kinds.split(","):
    for n in (int(v) for v in a.orders.split(",")):
        if kind == "pair":
            fam, npts = "C", n // 2
            X, Y = rng.uniform(0, 2 * np.pi, (B, npts)), rng.uniform(-3, 3, (B, npts))
            Z = rng.standard_normal((B, n))
            l = 2.0 * np.sqrt(12 * np.pi) * n ** -0.5
            H = np.array([0.9 * l, 1.1 * l, 1.3]) * rng.uniform(0.9, 1.1, (B, 3))
            S2 = np.full(B, 1e-2 / l**2)
            calls = {"new": lambda: fit_batch_loo_grad_mid(fam, X, Y, Z, H, S2),
                     "loo": lambda: fit_batch_loo(fam, X, Y, Z, H, S2),
                     "nllgrad": lambda: fit_batch_grad_mid(fam, X, Y, Z, H, S2)}
            handle = lambda: SympFit(fam, X[0], Y[0], Z[0], H[0], S2[0])
        else:
            fam, d = "A", 2
            npts = n // (2 * d)
            X = np.concatenate([rng.uniform(0, 2 * np.pi, (B, npts, d)), rng.uniform(-3, 3, (B, npts, d))], axis=2)
            Z = rng.standard_normal((B, n))
            l = 2.0 * np.sqrt(12 * np.pi) * npts ** (-1.0 / (2 * d)) * np.linspace(0.9, 1.15, 2 * d)
            H = np.append(l, 1.2) * rng.uniform(0.9, 1.1, (B, 2 * d + 1))
            S2 = np.full(B, 1e-2 / l.mean()**2)
            calls = {"new": lambda: fit_batch_pairs_loo_grad_mid(fam, X, Z, H, S2),
                     "loo": lambda: fit_batch_pairs_loo(fam, X, Z, H, S2),
                     "nllgrad": lambda: fit_batch_pairs_grad(fam, X, Z, H, S2)}
            handle = lambda: SympFit.pairs(fam, X[0], Z[0], H[0], S2[0])
        if a.only_new:
            calls = {"new": calls["new"]}
        f = None
        if not a.only_new:
            f = handle()
            rows = min(a.rows, B)

            def loop():
                for b in range(rows):
                    f.set_hyp(H[b], S2[b])
                    f.run().loo_grad("loo")
            calls["handle"] = loop
        ts = {k: [] for k in calls}
        for _ in range(a.warm):
            for c in calls.values():
                c()
        for _ in range(a.reps):
            for k, c in calls.items():
                ts[k].append(timed(c))
        if f is not None:
            f.close()
        t = {k: float(np.median(v)) for k, v in ts.items()}
        r = {"order": n, "kind": kind, "family": fam, "batch": B, "reps": a.reps, "warm": a.warm, "call_ms_loo_grad_mid": t["new"] * 1e3,
             "loo_grad_mid_per_s": B / t["new"]}
        if not a.only_new:
            t_handle = t["handle"] * B / rows
            r.update(call_ms_loo=t["loo"] * 1e3, call_ms_nll_grad=t["nllgrad"] * 1e3, handle_rows=rows,
                     handle_loop_ms_scaled_to_batch=t_handle * 1e3, loo_grad_mid_over_nll_grad=t["new"] / t["nllgrad"],
                     loo_grad_mid_over_loo=t["new"] / t["loo"], handle_loop_over_loo_grad_mid=t_handle / t["new"])
        line = json.dumps(r)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
