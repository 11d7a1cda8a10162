"""The gradient of the leave-one-point-out objective beside the calls it is measured against, alternately in one process:
    python tools/loograd_speed.py [--reg] [--fam F] [--reps R] [--objective loo|press] [--out FILE] N [N ...]     N = matrix order
SympFit.loo_grad (sgpr_fit_loo_grad) against nll_grad_full and the factor stage (device events of a run()) of the same handle;
host clock around whole calls, each ending in a stream synchronise, median of --reps rounds after one warm-up round.  Flop
model: n^3 / 3 (L^-T) + n^3 / 3 (Ky^-1) + n^3 (M) against nll_grad_full's 2 n^3 / 3 -- 2.5 x --, the factor's n^3 / 3.
One JSON line per size is printed and, with --out, appended to FILE (profiles/loograd/loograd_speed.jsonl)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sympgpr_amd.fit import SympFit

ap = argparse.ArgumentParser()
ap.add_argument("--reg", action="store_true", help="the scalar-kernel GP")
ap.add_argument("--fam", default="C")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--objective", default="loo", choices=["loo", "press"])
ap.add_argument("--out", default=None)
ap.add_argument("n", type=int, nargs="+", help="matrix orders")
a = ap.parse_args()

from bench import synth
for n in a.n:
    npts = n if a.reg else n // 2
    q, P, z, hyp, s2 = synth(npts)
    with SympFit(a.fam, q, P, z[:npts] if a.reg else z, hyp, s2, reg=a.reg) as f:
        f.run()
        ts = {"loo_grad": [], "nll_grad_full": [], "factor": []}
        value = grad = None
        for r in range(1 + a.reps):
            t0 = time.perf_counter()
            value, grad = f.loo_grad(a.objective)
            t1 = time.perf_counter()
            f.nll_grad_full()
            t2 = time.perf_counter()
            f.run()
            fac = f.stage_ms()[1]
            if r:
                ts["loo_grad"].append((t1 - t0) * 1e3)
                ts["nll_grad_full"].append((t2 - t1) * 1e3)
                ts["factor"].append(fac)
        med = {k: float(np.median(v)) for k, v in ts.items()}
        rec = {"tool": "loograd_speed", "n": f.n, "fam": a.fam, "reg": a.reg, "objective": a.objective, "reps": a.reps,
               "loo_grad_ms": round(med["loo_grad"], 2), "nll_grad_full_ms": round(med["nll_grad_full"], 2),
               "factor_ms": round(med["factor"], 2), "loo_grad_over_nll_grad_full": round(med["loo_grad"] / med["nll_grad_full"], 3),
               "loo_grad_over_factor": round(med["loo_grad"] / med["factor"], 3), "flop_model_over_nll_grad_full": 2.5,
               "tflops_model": round(5.0 * f.n ** 3 / 3 / (med["loo_grad"] * 1e-3) / 1e12, 2),
               "loo_grad_ms_calls": [round(v, 2) for v in ts["loo_grad"]],
               "nll_grad_full_ms_calls": [round(v, 2) for v in ts["nll_grad_full"]],
               "factor_ms_calls": [round(v, 2) for v in ts["factor"]], "value": value, "grad": [float(v) for v in grad]}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
