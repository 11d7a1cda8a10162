"""Leave-one-point-out cross-validation beside the calls it shares its work with, alternately in one process:
    python tools/loo_speed.py handle [--reg] [--fam F] [--reps R] [--out FILE] N [N ...]      N = matrix order
        SympFit.loo (sgpr_fit_loo) against nll_grad_full and the factor stage (device events) of the same handle; host clock
        around whole calls, each ending in a stream synchronise.  Both form Ky^-1 by the same row panels (2 n^3 / 3 flop);
        loo copies the blocks out where the gradient contracts the panel, so the model says loo <= nll_grad_full.
    python tools/loo_speed.py batch [--orders 80,140,256,512,1024] [--fam F] [--reps R] [--out FILE]
        fit_batch_loo against fit_batch and fit_batch_grad (fit_batch_grad_mid above order 256); B = 1024 up to order 256, 64
        above.  The model says loo lies between the two.
One JSON line per size is printed and, with --out, appended to FILE (profiles/loo/loo_speed.jsonl)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sympgpr_amd.fit import SympFit, fit_batch, fit_batch_grad, fit_batch_grad_mid, fit_batch_loo

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["handle", "batch"])
ap.add_argument("--reg", action="store_true", help="handle: the scalar-kernel GP")
ap.add_argument("--fam", default="C")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--orders", default="80,140,256,512,1024")
ap.add_argument("--out", default=None)
ap.add_argument("n", type=int, nargs="*", help="handle: matrix orders")
a = ap.parse_args()


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


def alternately(fns, reps):
    """one warm-up of each, then reps rounds in which every function runs once: -> median ms per function"""
    ts = [[] for _ in fns]
    for r in range(1 + reps):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            if r:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(t)) for t in ts], ts


if a.mode == "handle":
    from bench import synth
    for n in a.n:
        npts = n if a.reg else n // 2
        q, P, z, hyp, s2 = synth(npts)
        with SympFit(a.fam, q, P, z[:npts] if a.reg else z, hyp, s2, reg=a.reg) as f:
            fac = []
            for r in range(2):
                f.run()
                fac.append(f.stage_ms()[1])
            (ms_loo, ms_grad), ts = alternately([lambda: f.loo(resid=False, lpd=False), f.nll_grad_full], a.reps)
            full = alternately([lambda: f.loo(resid=True, cov=True, lpd=True)], 1)[0][0]
            o = f.loo(resid=False, lpd=False)
            emit({"tool": "loo_speed", "mode": "handle", "n": f.n, "fam": a.fam, "reg": a.reg, "loo_ms": round(ms_loo, 2),
                  "nll_grad_full_ms": round(ms_grad, 2), "factor_ms": round(fac[-1], 2),
                  "loo_over_grad": round(ms_loo / ms_grad, 4), "loo_over_factor": round(ms_loo / fac[-1], 3),
                  "loo_all_outputs_ms": round(full, 2), "loo_ms_calls": [round(v, 2) for v in ts[0]],
                  "grad_ms_calls": [round(v, 2) for v in ts[1]],
                  "tf_panel_solves": round(2.0 * f.n ** 3 / 3 / (ms_loo * 1e-3) / 1e12, 2), "loo": o["loo"], "press": o["press"]})
else:
    rng = np.random.default_rng(5)
    for n in (int(v) for v in a.orders.split(",")):
        B, npts = (1024 if n <= 256 else 64), n // 2
        X, Y = rng.uniform(0, 2 * np.pi, (B, npts)), rng.uniform(-3, 3, (B, npts))
        Z = rng.standard_normal((B, 2 * npts))
        l = 2.0 * np.sqrt(12 * np.pi) * n ** -0.5
        H = np.array([0.9 * l, 1.1 * l, 1.3]) * rng.uniform(0.9, 1.1, (B, 3))
        S2 = np.full(B, 1e-2 / l**2)
        grad = fit_batch_grad if n <= 256 else fit_batch_grad_mid
        (t_fit, t_loo, t_grad), _ = alternately([lambda: fit_batch(a.fam, X, Y, Z, H, S2, want_alpha=False),
                                                 lambda: fit_batch_loo(a.fam, X, Y, Z, H, S2),
                                                 lambda: grad(a.fam, X, Y, Z, H, S2)], a.reps)
        emit({"tool": "loo_speed", "mode": "batch", "order": 2 * npts, "family": a.fam, "batch": B,
              "call_ms_fit": round(t_fit, 3), "call_ms_loo": round(t_loo, 3), "call_ms_grad": round(t_grad, 3),
              "loo_over_fit": round(t_loo / t_fit, 3), "loo_over_grad": round(t_loo / t_grad, 3),
              "between": bool(t_fit <= t_loo <= t_grad), "loo_per_s": round(B / (t_loo * 1e-3), 1)})
