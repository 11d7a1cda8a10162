"""What finding periodic orbits on the device saves: maps.run_periodic_nd (sgpr_periodic_nd_host: every Newton pass of every
guess inside one launch) against the loop it replaces, on the same guesses in one process: per Newton iteration one
maps.run_map_nd_tangent call (nm = n + 1, jac=False, lyap=False) on the guesses still running, the residual and a NumPy solve of
(mono - I) dz = -r per guess on the host, the next guesses uploaded by the next call.  Host clock around whole calls / whole
loops, alternately, median of --reps.  One JSON line per case, appended to profiles/periodic_nd/speed.jsonl.
    python tools/periodic_nd_speed.py [--reps R] [--out FILE] [CASE ...]     CASE = d:Nt:Ntest:n:w, default 1:40:2048:3:1 2:60:2048:3:1
Data: the twist map of tests/test_periodic_cpu.py (F_q = -0.3 sin q_c - 0.09 sin(sum q), F_P = P, family A, sig2n 1e-6); guesses
scattered around that file's guess (pi + 0.1, .., 2.1, ..) of the period-3 orbit with winding number 1 per pair; WRAP_Q,
tol 1e-12, maxit 30 on both sides.
The model: one Newton pass costs one tangent orbit of n steps, so the launch should take about max(its) x the tangent call's
kernel time, and the host loop that plus a launch, two copies and a Python-side solve per iteration."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sympgpr_amd import maps
from sympgpr_amd.fit import SympFit
from tests.test_periodic_cpu import twist_training

TWO_PI, TOL, MAXIT, FAMILY = 2.0 * np.pi, 1e-12, 30, "A"


def host_loop(d, n, w, hyp, X, alpha, Q0, P0):
    """the loop a user writes today -> z (Ntest, 2d) (NaN where it failed), its, the tangent calls made"""
    Ntest, D = Q0.shape[0], 2 * d
    z = np.hstack((Q0, P0))
    out, its = np.full((Ntest, D), np.nan), np.full(Ntest, -1)
    run = np.arange(Ntest)
    calls = 0
    for it in range(1, MAXIT + 1):
        if run.size == 0:
            break
        zr = z[run]
        q, p, _, t = maps.run_map_nd_tangent(FAMILY, d, 0, n + 1, hyp, X, alpha, zr[:, :d], zr[:, d:], jac=False, lyap=False)
        calls += 1
        r = np.hstack((q[n] - zr[:, :d] - TWO_PI * w, p[n] - zr[:, d:]))         # the unwrapped map: q_n is lifted
        ok = np.isfinite(r).all(axis=1) & np.isfinite(t["mono"]).all(axis=(1, 2))
        done = ok & (np.abs(r).max(axis=1) <= TOL * np.maximum(1.0, np.abs(zr).max(axis=1)))
        out[run[done]], its[run[done]] = zr[done], it
        go = ok & ~done
        with np.errstate(all="ignore"):
            det = np.linalg.det(t["mono"] - np.eye(D))
        go &= np.isfinite(det) & (det != 0.0)                                   # a singular mono - I fails that guess only
        dz = np.linalg.solve(t["mono"][go] - np.eye(D), -r[go][:, :, None])[:, :, 0]
        z[run[go]] = zr[go] + dz
        z[run[go], :d] = np.mod(z[run[go], :d], TWO_PI)
        run = run[go]
    return out, its, calls


def one_case(d, Nt, Ntest, n, wind, reps):
    X, ztr = twist_training(d, Nt)
    hyp = np.array((1.2,) * d + (1.5,) * d + (1.0,))
    with SympFit.pairs(FAMILY, X, ztr, hyp, 1e-6) as f:
        alpha = f.run().alpha()
    rng = np.random.default_rng(7)
    Q0 = np.pi + 0.1 + rng.uniform(-0.05, 0.05, (Ntest, d))
    P0 = 2.1 + rng.uniform(-0.03, 0.03, (Ntest, d))
    w = np.full(d, wind)
    dev = lambda: maps.run_periodic_nd(FAMILY, d, maps.WRAP_Q, n, hyp, X, alpha, Q0, P0, wind=w, tol=TOL, maxit=MAXIT)
    tan = lambda: maps.run_map_nd_tangent(FAMILY, d, 0, n + 1, hyp, X, alpha, Q0, P0, jac=False, lyap=False)
    dev(), tan(), host_loop(d, n, w, hyp, X, alpha, Q0[:4], P0[:4])       # warm-up: code object load, first allocations
    t_dev, t_host, t_tan = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter(); o = dev(); t_dev.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); zh, ih, calls = host_loop(d, n, w, hyp, X, alpha, Q0, P0); t_host.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); tan(); t_tan.append(time.perf_counter() - t0)
    both = o["converged"] & (ih > 0)
    dq = np.abs(np.mod(o["z"][both, :d] - zh[both, :d] + np.pi, TWO_PI) - np.pi)
    med = lambda v: float(np.median(v))
    ms = lambda v: [round(x * 1e3, 3) for x in v]
    return {"tool": "periodic_nd_speed", "family": FAMILY, "d": d, "n0": Nt, "Ntest": Ntest, "n": n, "wind": wind, "reps": reps,
            "tol": TOL, "maxit": MAXIT, "device_converged": int(o["converged"].sum()), "host_converged": int((ih > 0).sum()),
            "device_its_max": int(o["its"].max()), "device_its_mean": round(float(o["its"][o["converged"]].mean()), 2),
            "host_tangent_calls": calls, "device_ms_calls": ms(t_dev), "host_loop_ms_calls": ms(t_host), "tangent_call_ms_calls": ms(t_tan),
            "device_ms": round(med(t_dev) * 1e3, 3), "host_loop_ms": round(med(t_host) * 1e3, 3),
            "tangent_call_ms": round(med(t_tan) * 1e3, 3), "host_loop_over_device": round(med(t_host) / med(t_dev), 2),
            "device_over_its_max_tangent_calls": round(med(t_dev) / (int(o["its"].max()) * med(t_tan)), 3),
            "median_abs_dz_both_converged": float(np.median(np.maximum(dq.max(axis=1), np.abs(o["z"][both, d:] - zh[both, d:]).max(axis=1))))
                                            if both.any() else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "periodic_nd", "speed.jsonl"))
    ap.add_argument("cases", nargs="*", default=["1:40:2048:3:1", "2:60:2048:3:1"])
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for case in a.cases:
            line = json.dumps(one_case(*(int(v) for v in case.split(":")), a.reps))
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
