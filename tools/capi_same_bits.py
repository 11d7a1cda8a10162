"""Every output of the entries behind capi.hip / capi_fit.hip / batch.hip's host tail on small fixed-seed cases, for a
byte-for-byte comparison of two builds (profiles/capi_paths/same_bits.txt):
    python tools/capi_same_bits.py run --root TREE --out A.npz        (TREE: a checkout with its own built library)
    python tools/capi_same_bits.py run --out B.npz                    (this tree)
    python tools/capi_same_bits.py compare A.npz B.npz
Families A and D (D carries the periods, so nhyp differs).  Single fits: a pair fit, a scalar-kernel (reg) fit and a d = 2 fit,
each with sig2n > 0 and < 0, and the pair fit at the orders on either side of the strip solves' threshold (n = 512: no strips,
n = 640: strips) -- nll_grad_full, loo with every optional output, loo_grad for both objectives; predict_cov at one point and
at two chunks; predict_genfun with var at one point and at 257, with and without ref; the d-pair maps (forward, tangent,
inverse, periodic search) through the handle and through the _host entries; every batched entry with three problems, one not
positive definite and one with sig2n < 0, in one launch and on the mid path, the latter also in chunks of two."""
import argparse
import os
import sys

import numpy as np


def model(fam, kind, N, seed):
    """(points, z, hyp, sig2n) of one problem: kind "pair" / "reg" (x | y points) or "d2" (X (N, 4))"""
    rng = np.random.default_rng(seed)
    d = 2 if kind == "d2" else 1
    q, P = rng.uniform(0, 2 * np.pi, (N, d)), rng.uniform(-3, 3, (N, d))
    n = N if kind == "reg" else 2 * d * N
    z = rng.standard_normal(n)
    l = min(2.0, 2.0 * np.sqrt(12 * np.pi) * N ** (-1.0 / (2 * d)))
    hyp = [l] * (2 * d) + ([0.5] * d if fam == "D" else []) + [1.0]
    return np.hstack((q, P)), z, np.array(hyp), 1e-2 / l ** 2


def make_fit(F, fam, kind, X, z, hyp, s2):
    if kind == "d2":
        return F.SympFit.pairs(fam, X, z, hyp, s2)
    return F.SympFit(fam, X[:, 0], X[:, 1], z, hyp, s2, reg=(kind == "reg"))


def single_fits(F, maps, out):
    for fam in "AD":
        for kind, N, tag in (("pair", 40, ""), ("reg", 40, ""), ("d2", 20, ""), ("pair", 256, "_nostrips"), ("pair", 320, "_strips")):
            X, z, hyp, s2 = model(fam, kind, N, 11)
            for sign in ((1, -1) if not tag else (1,)):
                key = "%s_%s%s_%s" % (fam, kind, tag, "pos" if sign > 0 else "neg")
                with make_fit(F, fam, kind, X, z, hyp, sign * s2) as f:
                    f.run()
                    out[key + "_alpha"], out[key + "_nll"] = f.alpha(), np.array(f.nll())
                    out[key + "_nll_grad_full"] = f.nll_grad_full()
                    for name, v in f.loo(resid=True, cov=True, lpd=True).items():
                        out[key + "_loo_" + name] = np.asarray(v)
                    for obj in ("loo", "press"):
                        v, g = f.loo_grad(obj)
                        out[key + "_loo_grad_%s_value" % obj], out[key + "_loo_grad_%s" % obj] = np.array(v), g
                    if sign < 0 or tag:
                        continue
                    D = 1 if kind == "reg" else X.shape[1]
                    rng = np.random.default_rng(5)
                    for m in (1, 256 // D + 1):
                        Xt = np.hstack((rng.uniform(0, 2 * np.pi, (m, X.shape[1] // 2)), rng.uniform(-3, 3, (m, X.shape[1] // 2))))
                        mean, cov = f.predict_pairs_cov(Xt) if kind == "d2" else f.predict_cov(Xt[:, 0], Xt[:, 1])
                        out[key + "_cov%d_mean" % m], out[key + "_cov%d_cov" % m] = mean, cov
                    if kind == "reg":
                        continue
                    for m in (1, 257):
                        Xt = np.hstack((rng.uniform(0, 2 * np.pi, (m, D // 2)), rng.uniform(-3, 3, (m, D // 2))))
                        for ref in (None, X[0]):
                            Fv, var = f.predict_pairs_genfun(Xt, ref=ref, var=True)
                            r = "ref" if ref is not None else "noref"
                            out[key + "_genfun%d_%s_F" % (m, r)], out[key + "_genfun%d_%s_var" % (m, r)] = Fv, var


def pair_maps(F, maps, out):
    """d = 2, 20 training points, three orbits, nm = 4; the periodic search with n = 2"""
    for fam in "AD":
        X, z, hyp, s2 = model(fam, "d2", 20, 23)
        Q0, P0 = X[:3, :2] + 0.01, X[:3, 2:] - 0.01
        with F.SympFit.pairs(fam, X, z, hyp, s2) as f:
            f.run()
            alpha = f.alpha()
            calls = {"fit": (lambda: f.applymap_pairs(4, Q0, P0, return_iters=True),
                             lambda: f.applymap_pairs_tangent(4, Q0, P0),
                             lambda: f.applymap_pairs_inverse(4, Q0, P0, return_iters=True),
                             lambda: f.periodic_orbits(2, Q0, P0, mono=True, orbit=True)),
                     "host": (lambda: maps.run_map_nd(fam, 2, 0, 4, hyp, X, alpha, Q0, P0, return_iters=True),
                              lambda: maps.run_map_nd_tangent(fam, 2, 0, 4, hyp, X, alpha, Q0, P0),
                              lambda: maps.run_map_nd_inverse(fam, 2, 0, 4, hyp, X, alpha, Q0, P0, return_iters=True),
                              lambda: maps.run_periodic_nd(fam, 2, 0, 2, hyp, X, alpha, Q0, P0, mono=True, orbit=True))}
            for via, (fwd, tan, inv, per) in calls.items():
                key = "%s_map_%s" % (fam, via)
                for name, res in (("fwd", fwd()), ("inv", inv())):
                    out[key + "_%s_q" % name], out[key + "_%s_p" % name], out[key + "_%s_iters" % name] = res
                q, p, it, t = tan()
                out[key + "_tan_q"], out[key + "_tan_p"], out[key + "_tan_iters"] = q, p, it
                for name, v in list(t.items()) + [("periodic_" + k, v) for k, v in per().items()]:
                    out[key + "_" + name] = np.asarray(v)


def batches(F, L, out):
    """three problems each: row 1 not positive definite (sig < 0), row 2 with sig2n < 0"""
    out["batch_max_order"] = np.array(F.batch_max_order())

    def problems(fam, kind, N):
        rows = [model(fam, kind, N, 31 + b) for b in range(3)]
        hyp = np.array([r[2] for r in rows])
        hyp[1, -1] = -1.0
        s2 = np.array([r[3] for r in rows]) * (1, 1, -1)
        return np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), hyp, s2

    def keep(key, names, res):
        for name, v in zip(names, res):
            if v is not None:
                out[key + "_" + name] = np.asarray(v)

    for chunk in (0, 2):
        L.check(L.load_probe_library().sgpr_probe_tune(b"batch_gradmid_chunk", float(chunk)))
        for fam in "AD":
            for n in ((40, 320) if chunk == 0 else (320,)):
                X, z, hyp, s2 = problems(fam, "pair", n // 2)
                x, y = X[:, :, 0], X[:, :, 1]
                key = "%s_batch_xy%d%s" % (fam, n, "_chunk2" if chunk else "")
                mid = n > 256
                if chunk == 0:
                    keep(key + "_fit", ("alpha", "nll", "info"), F.fit_batch(fam, x, y, z, hyp, s2))
                keep(key + "_loo", ("alpha", "nll", "loo", "info"), F.fit_batch_loo(fam, x, y, z, hyp, s2, want_alpha=True))
                grad = F.fit_batch_grad_mid if mid else F.fit_batch_grad
                keep(key + "_grad", ("alpha", "nll", "grad", "info"), grad(fam, x, y, z, hyp, s2, want_alpha=True))
                loo_grad = F.fit_batch_loo_grad_mid if mid else F.fit_batch_loo_grad
                for obj in ("loo", "press"):
                    keep(key + "_loo_grad_" + obj, ("alpha", "nll", "value", "grad", "info"),
                         loo_grad(fam, x, y, z, hyp, s2, objective=obj, want_alpha=True))
            for n in ((40, 260) if chunk == 0 else (260,)):
                X, z, hyp, s2 = problems(fam, "d2", n // 4)
                key = "%s_batch_nd%d%s" % (fam, n, "_chunk2" if chunk else "")
                if chunk == 0:
                    keep(key + "_fit", ("alpha", "nll", "info"), F.fit_batch_pairs(fam, X, z, hyp, s2))
                keep(key + "_grad", ("alpha", "nll", "grad", "info"), F.fit_batch_pairs_grad(fam, X, z, hyp, s2, want_alpha=True))
                keep(key + "_loo", ("alpha", "nll", "loo", "info"), F.fit_batch_pairs_loo(fam, X, z, hyp, s2, want_alpha=True))
                loo_grad = F.fit_batch_pairs_loo_grad_mid if n > 256 else F.fit_batch_pairs_loo_grad
                for obj in ("loo", "press"):
                    keep(key + "_loo_grad_" + obj, ("alpha", "nll", "value", "grad", "info"),
                         loo_grad(fam, X, z, hyp, s2, objective=obj, want_alpha=True))
    L.check(L.load_probe_library().sgpr_probe_tune(b"batch_gradmid_chunk", 0.0))


def run(args):
    root = os.path.abspath(args.root or os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    sys.path.insert(0, root)
    import sympgpr_amd
    from sympgpr_amd import _lib as L, fit as F, maps
    assert os.path.abspath(sympgpr_amd.__file__).startswith(root), sympgpr_amd.__file__
    out = {}
    single_fits(F, maps, out)
    pair_maps(F, maps, out)
    batches(F, L, out)
    np.savez(args.out, **out)
    print("%d arrays from %s -> %s" % (len(out), L.lib_path(), args.out))


def compare(args):
    a, b = np.load(args.a), np.load(args.b)
    assert sorted(a.files) == sorted(b.files), sorted(set(a.files) ^ set(b.files))
    print("%-44s %-12s %-10s parent vs this tree" % ("array", "shape", "non-finite"))
    differ = 0
    for k in sorted(a.files):
        same = a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
        differ += not same
        print("%-44s %-12s %-10d %s" % (k, "x".join(map(str, a[k].shape)) or "scalar", int(np.sum(~np.isfinite(a[k]))),
                                        "identical" if same else "DIFFER"))
    print("%d arrays, %d differ" % (len(a.files), differ))
    return 1 if differ else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--root", default=None)
    r.add_argument("--out", required=True)
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    args = ap.parse_args()
    sys.exit(run(args) if args.cmd == "run" else compare(args))
