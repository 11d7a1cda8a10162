"""The full NLL gradient (sgpr_fit_nll_grad_full) after one factorisation: host clock around whole calls (each ends in a
stream synchronise), against the same process's factorisation (sgpr_fit_factor's stage time, device events) and, at d = 1,
against the old two-length-scale sgpr_fit_nll_grad (whole calls).  One JSON line per matrix order, also appended to --out.
    python tools/nllgrad_speed.py [--d D] [--fam F] [--reg] [--old] [--out FILE] N [N ...]    N = matrix order
The panel solves cost 2 n^3 / 3 flop; tf_panel_solves is that over the measured whole-call time (the contraction, the
panel set-up and the fold included)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sympgpr_amd.fit import SympFit
from bench import synth, synth_pairs
ap = argparse.ArgumentParser()
ap.add_argument("--d", type=int, default=1)
ap.add_argument("--fam", default="A")
ap.add_argument("--reg", action="store_true", help="the scalar-kernel GP (d = 1 only)")
ap.add_argument("--old", action="store_true", help="also time the old sgpr_fit_nll_grad (d = 1; two n x n scratch matrices)")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None, help="append the JSON lines to this file")
ap.add_argument("--tune", action="append", default=[], help="name=value of an experiment knob (libsympgpr_probe.so)")
ap.add_argument("n", type=int, nargs="+", help="matrix orders")
a = ap.parse_args()
if a.tune:
    from sympgpr_amd import _lib as L
    for kv in a.tune:
        L.check(L.load_probe_library().sgpr_probe_tune(kv.split("=")[0].encode(), float(kv.split("=")[1])))
if a.reg and a.d != 1:
    sys.exit("--reg needs d = 1")


def timed(fn, reps):
    ts, out = [], None
    for r in range(1 + reps):
        t0 = time.perf_counter()
        out = fn()
        if r:
            ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


for n in a.n:
    npts = n if a.reg else n // (2 * a.d)
    if a.d == 1:
        q, P, z, hyp, s2 = synth(npts)
        if a.fam == "D":
            hyp = np.array([hyp[0], hyp[1], 0.45, hyp[2]])
        f = SympFit(a.fam, q, P, z[:npts] if a.reg else z, hyp, s2, reg=a.reg)
    else:
        X, z, hyp, s2 = synth_pairs(npts, a.d)
        if a.fam == "D":
            hyp = np.concatenate((hyp[:2 * a.d], np.full(a.d, 0.45), hyp[-1:]))
        f = SympFit.pairs(a.fam, X, z, hyp, s2)
    with f:
        fac = []
        for r in range(2):
            f.run()
            fac.append(f.stage_ms()[1])
        g, ts = timed(f.nll_grad_full, a.reps)
        old_ts = None
        if a.old and a.d == 1:
            go, old_ts = timed(f.nll_grad, a.reps)
        nn = f.n
    ms = float(np.median(ts))
    rec = {"tool": "nllgrad_speed", "n": nn, "tune": a.tune, "d": a.d, "fam": a.fam, "reg": a.reg, "nhyp": len(hyp),
           "ms_per_call": round(ms, 2), "ms_calls": [round(v, 2) for v in ts], "factor_ms": round(fac[-1], 2),
           "over_factor": round(ms / fac[-1], 3), "tf_panel_solves": round(2.0 * nn ** 3 / 3 / (ms * 1e-3) / 1e12, 2),
           "grad": [float(v) for v in g]}
    if old_ts:
        om = float(np.median(old_ts))
        rec.update(old_nll_grad_ms=round(om, 2), over_old_nll_grad=round(ms / om, 4),
                   old_grad_rel_diff=float(np.abs(go - g[:2]).max() / np.abs(go).max()))
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
