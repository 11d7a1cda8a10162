"""The exact gradient of the leave-one-point-out objectives on the device (sgpr_fit_loo_grad, SympFit.loo_grad, func.loo_chol_grad).

Reference: tests/ref_loograd.py's NumPy restatement on the oracle's Ky, which tests/test_loograd_cpu.py pins to central differences
of the definition by deletion and to the same formulas at 40 digits (its own error stays below a tenth of the tolerance here).
Tolerance: the NLL gradient's rule, |g - g_ref| <= max(1e-9, 100 cond eps) S per exact component, 1e-6 in place of 1e-9 for
difference-based ones, S = 1/2 sum |W' dKy| the size of the component's own sum, cond from NumPy on the host Ky.
Shapes: pairs N = 83 (n = 166: no multiple of 64 or 128) in families A, B (the sum kernel), C, D (periods); pairs N = 330 with
panels of 256 rows (n = 660: three panels, the last ragged, J > 0); reg N = 257 (odd order: the apply kernel's 8-byte path);
d = 2, N = 90 (D = 4); d = 3, N = 50 in family D (D = 6, 10 hyperparameters)."""
import numpy as np
import pytest

from tests import ref_loo as R
from tests import ref_loograd as G

pytestmark = pytest.mark.gpu

_cache = {}


def _case(oracle, fam, kind, N, objective="loo"):
    """one problem with its host reference: computed once, shared, never written to"""
    if (fam, kind, N) not in _cache:
        p = R.problem(oracle, fam, kind, N, 900 + N)
        for a in p.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[(fam, kind, N)] = p
    p = _cache[(fam, kind, N)]
    if (fam, kind, N, objective) not in _cache:
        ref = G.reference(oracle, fam, kind, p, objective)
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[(fam, kind, N, objective)] = ref
    return p, _cache[(fam, kind, N, objective)]


def _fit(fam, kind, p, s2=None, hyp=None):
    from sympgpr_amd.fit import SympFit
    X = p["X"]
    s2 = p["s2"] if s2 is None else s2
    hyp = p["hyp"] if hyp is None else hyp
    if kind == "reg":
        return SympFit(fam, X[:, 0], X[:, 1], p["z"], hyp, s2, reg=True)
    if kind == 1:
        return SympFit(fam, X[:, 0], X[:, 1], p["z"], hyp, s2)
    return SympFit.pairs(fam, X, p["z"], hyp, s2)


def _bits(a):
    return np.ascontiguousarray(np.atleast_1d(a)).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


class _panel_width:
    """the loograd_nb knob for the calls inside the block; 0 = the default rule (the library reads the knob at every call)"""

    def __init__(self, nb):
        self.nb = nb

    def __enter__(self):
        from sympgpr_amd import _lib as L
        L.check(L.load_probe_library().sgpr_probe_tune(b"loograd_nb", float(self.nb)))

    def __exit__(self, *a):
        from sympgpr_amd import _lib as L
        L.check(L.load_probe_library().sgpr_probe_tune(b"loograd_nb", 0.0))


def _check_value(value, f, p, objective, what):
    ref = f.loo(resid=False, lpd=False)[objective]
    tol = R.tolerance(p["cond"])
    print("%s: value %.15g  f.loo() %.15g  rel %.3g  tol %.3g" % (what, value, ref, abs(value - ref) / abs(ref), tol))
    assert abs(value - ref) <= tol * abs(ref)


@pytest.mark.parametrize("fam,kind,N,objective", [("A", 1, 83, "loo"), ("B", 1, 83, "loo"), ("C", 1, 83, "loo"), ("D", 1, 83, "loo"),
                                                  ("A", "reg", 257, "loo"), ("D", "reg", 257, "loo"),
                                                  ("A", 2, 90, "loo"), ("D", 3, 50, "loo"),
                                                  ("C", 1, 83, "press"), ("A", "reg", 257, "press")])
def test_against_the_host(oracle, fam, kind, N, objective):
    p, ref = _case(oracle, fam, kind, N, objective)
    assert p["cond"] <= 1e8
    what = "%s %s N=%d %s" % (fam, kind, N, objective)
    with _fit(fam, kind, p) as f:
        f.run()
        value, g = f.loo_grad(objective)
        assert g.shape == (len(p["hyp"]) + 1,)
        G.compare(g, ref, what)
        _check_value(value, f, p, objective, what)
        assert abs(value - ref["value"]) <= R.tolerance(p["cond"]) * abs(ref["value"])


def test_three_panels_and_every_panel_width(oracle):
    """n = 660 with panels of 256 rows (256 + 256 + 148), of 128 rows (six panels) and the default (one panel): each within the
    tolerance of the host reference and of one another (the order of the sums changes: equal bits are not asked)"""
    fam, kind, N = "A", 1, 330
    p, ref = _case(oracle, fam, kind, N)
    got = {}
    with _fit(fam, kind, p) as f:
        f.run()
        for nb in (256, 128, 0):
            with _panel_width(nb):
                value, g = f.loo_grad()
            G.compare(g, ref, "A pairs N=330, loograd_nb=%d" % nb)
            _check_value(value, f, p, "loo", "loograd_nb=%d" % nb)
            got[nb] = g
    tol = np.where(ref["exact"], max(1e-9, 100 * ref["cond"] * G.EPS), max(1e-6, 100 * ref["cond"] * G.EPS)) * ref["S"]
    for nb in (256, 128):
        assert np.all(np.abs(got[nb] - got[0]) <= tol), (nb, got[nb], got[0])


def test_negative_noise_flips_the_last_entry_only(oracle):
    p, ref = _case(oracle, "A", 1, 83)
    with _fit("A", 1, p) as f:
        _, gp = f.run().loo_grad()
    with _fit("A", 1, p, s2=-p["s2"]) as f:
        vn, gn = f.run().loo_grad()
    assert _same(gp[:-1], gn[:-1]) and gn[-1] == -gp[-1] and gp[-1] != 0.0
    neg = dict(ref, g=np.append(ref["g"][:-1], -ref["g"][-1]))
    G.compare(gn, neg, "A pairs N=83, sig2n < 0")


@pytest.mark.parametrize("fam,kind,N", [("A", 1, 83), ("A", "reg", 257), ("A", 2, 90)])
def test_differences_of_the_device_objective(oracle, fam, kind, N):
    """central differences of f.loo()["loo"] over refits with set_hyp, relative step 1e-4, against loo_grad: the rule of
    test_gpu_nll_grad_full._fd_check, |fd - g_k| <= 1e-5 max(|g_k|, 1e-3 max|g|)"""
    p, _ = _case(oracle, fam, kind, N)
    hyp, s2 = np.array(p["hyp"]), p["s2"]
    with _fit(fam, kind, p) as f:
        _, g = f.run().loo_grad()
        gscale = np.abs(g).max()
        for k in range(len(hyp) + 1):
            h = 1e-4 * abs(hyp[k] if k < len(hyp) else s2)
            vals = []
            for sgn in (1.0, -1.0):
                hp, sp = hyp.copy(), s2
                if k < len(hyp):
                    hp[k] += sgn * h
                else:
                    sp += sgn * h
                f.set_hyp(hp, sp)
                vals.append(f.run().loo(resid=False, lpd=False)["loo"])
            fd = (vals[0] - vals[1]) / (2 * h)
            rel = abs(fd - g[k]) / max(abs(g[k]), 1e-3 * gscale)
            print("%s %s N=%d: component %d  grad %.12g  fd %.12g  rel %.3g" % (fam, kind, N, k, g[k], fd, rel))
            assert rel <= 1e-5, (fam, kind, N, k, g[k], fd)


@pytest.mark.parametrize("fam,kind,N", [("A", 1, 330), ("A", "reg", 257), ("A", 2, 90)])
def test_purity_and_determinism(oracle, fam, kind, N):
    p, _ = _case(oracle, fam, kind, N)
    with _fit(fam, kind, p) as f:
        f.run()
        held = lambda: [f.alpha(), f.nll(), f.nll_grad_full()] + [f.loo(cov=True)[k] for k in ("loo", "press", "resid", "cov", "lpd")]
        before = held()
        v1, g1 = f.loo_grad()
        after = held()
        assert all(_same(a, b) for a, b in zip(before, after)), "loo_grad changed what the handle holds"
        v2, g2 = f.loo_grad()
        assert _same(g1, g2) and _same(v1, v2), "two calls differ"
        vp, gpress = f.loo_grad("press")
        f.release_scratch()
        v3, g3 = f.loo_grad()
        assert _same(g1, g3) and _same(v1, v3), "the call after sgpr_fit_trim differs"
        assert all(_same(a, b) for a, b in zip(before, held()))
        assert not _same(g1, gpress)


def test_refusals_leave_the_handle_alone(oracle):
    import sympgpr_amd
    from sympgpr_amd import _lib as L
    from sympgpr_amd.fit import SympFit
    p, _ = _case(oracle, "A", 1, 83)
    lib = L.load_library()
    nh = len(p["hyp"])
    v, g = np.zeros(1), np.zeros(nh + 2)

    def refused(f, which, ngrad, code, word, vp=None, gp=None):
        rc = lib.sgpr_fit_loo_grad(f._h, which, L.dptr(v) if vp is None else vp, L.dptr(g) if gp is None else gp, ngrad)
        msg = lib.sgpr_last_error()
        assert rc == code, (rc, msg)
        assert msg.startswith(b"fit_loo_grad:") and word in msg, msg

    with _fit("A", 1, p) as f:
        refused(f, 0, nh, L.E_ARG, b"ngrad")                      # argument errors come before the state
        refused(f, 0, nh + 1, L.E_STATE, b"not solved")
        with pytest.raises(sympgpr_amd.SympGPRError, match="not solved"):
            f.loo_grad()
        f.build()
        f.factor()
        refused(f, 0, nh + 1, L.E_STATE, b"not solved")
        f.solve()
        before = [f.alpha(), f.nll()] + list(f.loo_grad())
        refused(f, 0, nh, L.E_ARG, b"ngrad")
        refused(f, 0, nh + 2, L.E_ARG, b"ngrad")
        refused(f, 2, nh + 1, L.E_ARG, b"which")
        refused(f, -1, nh + 1, L.E_ARG, b"which")
        assert lib.sgpr_fit_loo_grad(f._h, 0, None, L.dptr(g), nh + 1) == L.E_ARG
        assert lib.sgpr_fit_loo_grad(f._h, 0, L.dptr(v), None, nh + 1) == L.E_ARG
        with pytest.raises(ValueError):
            f.loo_grad("nll")
        after = [f.alpha(), f.nll()] + list(f.loo_grad())
        assert all(_same(a, b) for a, b in zip(before, after))
    with SympFit("A", p["X"][:, 0], p["X"][:, 1], p["z"][:83], p["hyp"], p["s2"], block="qq") as f:
        f.run()
        before = [f.alpha(), f.nll()]
        refused(f, 0, nh + 1, L.E_STATE, b"single-block")
        with pytest.raises(sympgpr_amd.SympGPRError, match="single-block"):
            f.loo_grad()
        assert all(_same(a, b) for a, b in zip(before, [f.alpha(), f.nll()]))


def test_func_route_and_lbfgs(oracle):
    """func.loo_chol_grad at order 166 is the handle route; L-BFGS-B with jac=True lowers loo_chol from a perturbed start
    within five iterations"""
    from scipy.optimize import minimize
    from sympgpr_amd import func
    p, _ = _case(oracle, "A", 1, 83)
    x = np.concatenate([p["X"][:, 0], p["X"][:, 1]])
    theta = np.append(p["hyp"], p["s2"])
    old = func.get_family()
    func.set_family("A")
    try:
        value, grad = func.loo_chol_grad(theta, x, p["z"], 166)
        with _fit("A", 1, p) as f:
            v2, g2 = f.run().loo_grad()
        assert _same(value, v2) and _same(grad, g2)
        vneg, gneg = func.loo_chol_grad(np.append(p["hyp"], -p["s2"]), x, p["z"], 166)
        assert _same(vneg, value) and gneg[-1] == -grad[-1]
        vpress, _ = func.loo_chol_grad(theta, x, p["z"], 166, objective="press")
        assert vpress > 0 and vpress != value
        start = theta * np.array([1.25, 0.8, 1.2, 3.0])
        res = minimize(lambda t: func.loo_chol_grad(t, x, p["z"], 166), start, jac=True, method="L-BFGS-B",
                       bounds=[(1e-3 * t, 1e3 * t) for t in theta], options={"maxiter": 5})
        f0, f1 = func.loo_chol(start, x, p["z"], 166), func.loo_chol(res.x, x, p["z"], 166)
        print("L-BFGS-B: loo_chol %.6g -> %.6g in %d iterations (%d evaluations); at the fixture's own hyp %.6g" % (
            f0, f1, res.nit, res.nfev, value))
        assert res.nit <= 5 and f1 < f0
    finally:
        func.set_family(old)
