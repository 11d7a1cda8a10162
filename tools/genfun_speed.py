"""The generating function (sgpr_fit_predict_genfun) against the entries it should cost no more than, after one factorisation:
host clock around whole calls (each ends in a stream synchronise), 1 warm-up each, median of 3, the compared entries
alternating in one process.  One JSON line per case, appended to profiles/genfun/genfun_speed.jsonl (--out).
    python tools/genfun_speed.py mean [--d D] [--m M] N0 [N0 ...]   F at M points against predict_pairs / predict_rows on them
    python tools/genfun_speed.py var  [--d D] [--m M] N0 [N0 ...]   F and its variance against predict_cov, per forward pass
N0 = training points (matrix order 2 d N0).  A forward pass is 64 right-hand-side columns: the variance takes ceil(c / 64) per
chunk of c <= 256 points, predict_cov ceil(2 d c / 64) per chunk of c <= 256 / (2 d)."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sympgpr_amd.fit import SympFit
from bench import synth, synth_pairs
ap = argparse.ArgumentParser()
ap.add_argument("what", choices=("mean", "var"))
ap.add_argument("--d", type=int, default=1)
ap.add_argument("--m", type=int, default=320, help="test points per call")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "genfun", "genfun_speed.jsonl"))
ap.add_argument("n0", type=int, nargs="+", help="training points")
a = ap.parse_args()
d, D, m = a.d, 2 * a.d, a.m


def passes(cols_per_point, chunk):
    return sum((cols_per_point * min(chunk, m - c0) + 63) // 64 for c0 in range(0, m, chunk))


for n0 in a.n0:
    rng = np.random.default_rng(77)
    Xt = np.asfortranarray(np.column_stack([rng.uniform(0, 2 * np.pi, (m, d)), rng.uniform(-3, 3, (m, d))]))
    if d == 1:
        q, P, z, hyp, s2 = synth(n0)
        f = SympFit("A", q, P, z, hyp, s2)
        qt, Pt = np.ascontiguousarray(Xt[:, 0]), np.ascontiguousarray(Xt[:, 1])
        grad, gname = (lambda: f.predict_rows(qt, Pt)), "predict_rows"
        cov = lambda: f.predict_cov(qt, Pt)
        gen = lambda var: f.predict_genfun(qt, Pt, var=var)
    else:
        X, z, hyp, s2 = synth_pairs(n0, d)
        f = SympFit.pairs("A", X, z, hyp, s2)
        grad, gname = (lambda: f.predict_pairs(Xt)), "predict_pairs"
        cov = lambda: f.predict_pairs_cov(Xt)
        gen = lambda var: f.predict_pairs_genfun(Xt, var=var)
    new, old = ((lambda: gen(False)), grad) if a.what == "mean" else ((lambda: gen(True)), cov)
    with f:
        f.run()
        t = {"new": [], "old": []}
        for r in range(1 + a.reps):
            for name, call in (("old", old), ("new", new)):
                t0 = time.perf_counter()
                call()
                if r:
                    t[name].append((time.perf_counter() - t0) * 1e3)
        nn = f.n
    ms_new, ms_old = float(np.median(t["new"])), float(np.median(t["old"]))
    rec = {"tool": "genfun_speed", "what": a.what, "n0": n0, "d": d, "n": nn, "m": m,
           "genfun_ms": round(ms_new, 3), "genfun_ms_calls": [round(v, 3) for v in t["new"]]}
    if a.what == "mean":
        rec.update({"against": gname, "against_ms": round(ms_old, 3), "against_ms_calls": [round(v, 3) for v in t["old"]],
                    "genfun_over_against": round(ms_new / ms_old, 4)})
    else:
        p_new, p_old = passes(1, 256), passes(D, 256 // D)
        rec.update({"against": "predict_cov", "against_ms": round(ms_old, 3), "against_ms_calls": [round(v, 3) for v in t["old"]],
                    "genfun_passes": p_new, "against_passes": p_old, "genfun_ms_per_pass": round(ms_new / p_new, 3),
                    "against_ms_per_pass": round(ms_old / p_old, 3),
                    "per_pass_genfun_over_against": round((ms_new / p_new) / (ms_old / p_old), 4)})
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")
