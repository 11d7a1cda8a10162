"""The gradient of the leave-one-point-out objectives of every problem of a batch in one launch (sgpr_fit_batch_loo_grad,
fit.fit_batch_loo_grad, func.loo_chol_grad_batch).

Fixtures as tests/test_gpu_batch_loo.py: ref_loo.problem(oracle, fam, kind, npts, 7000 + 11 npts + k), k = 0 .. 4, batches of five.
Reference and tolerance as tests/test_gpu_loo_grad.py: tests/ref_loograd.py's NumPy restatement on the oracle's Ky under
ref_loograd.compare's rule, |g - g_ref| <= max(1e-9, 100 cond eps) S per exact component, 1e-6 in place of 1e-9 for the
difference-based ones.  Where |g| / S is small and a component is difference-based that comparison is weak, so every row is also
held to SympFit(...).run().loo_grad(objective) under the exact-component rule on EVERY component: both are exact device
computations.  The largest condition number of a batch here is 4.0e3 (measured on the host with the oracle), every test asserts
cond <= 1e8, so the 1e-9 floor is what applies.

Shapes, the smallest at which each piece of the kernel can go wrong: pairs N = 37 (n = 74: one leaf, P rows in the q rows' leaf)
and N = 128 (n = 256, the maximum: a point's two rows lie in different leaves) in families A, B, C, D; C pairs N = 70 (n = 140:
the P rows straddle the leaf boundary) and N = 5 (n = 10: most lanes idle in every fold); C reg N = 129 (a second leaf of order 1)
and N = 256; n = 258 for the slow path."""
import numpy as np
import pytest

from tests import ref_loo as R
from tests import ref_loograd as G

pytestmark = pytest.mark.gpu

WHICH = {"loo": 0, "press": 1}
_cache = {}


def _batch(oracle, fam, npts, reg, objective="loo"):
    """five problems of one shape with their host references: computed once, shared, never written to"""
    kind = "reg" if reg else 1
    key = (fam, npts, reg)
    if key not in _cache:
        probs = [R.problem(oracle, fam, kind, npts, 7000 + 11 * npts + k) for k in range(5)]
        data = (np.array([p["X"][:, 0] for p in probs]), np.array([p["X"][:, 1] for p in probs]), np.array([p["z"] for p in probs]),
                np.array([p["hyp"] for p in probs]), np.array([p["s2"] for p in probs]))
        for a in data:
            a.setflags(write=False)
        _cache[key] = (data, probs)
    data, probs = _cache[key]
    if key + (objective,) not in _cache:
        refs = [G.reference(oracle, fam, kind, p, objective) for p in probs]
        for ref in refs:
            for a in ref.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _cache[key + (objective,)] = refs
    return data, probs, _cache[key + (objective,)]


def _bits(a):
    return np.ascontiguousarray(np.atleast_1d(a)).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _against_the_handle(g, gfit, ref, what):
    """the exact-component rule on every component"""
    tol = max(1e-9, 100 * ref["cond"] * G.EPS) * ref["S"]
    err = np.abs(np.asarray(g) - np.asarray(gfit))
    print("%s: max err/S %.3g  max err/tol %.3g" % (what, (err / np.maximum(ref["S"], 1e-300)).max(), (err / tol).max()))
    assert np.all(err <= tol), (what, g, gfit, err / ref["S"])


def _check_rows(oracle, fam, npts, reg, objective):
    from sympgpr_amd.fit import SympFit, fit_batch, fit_batch_loo, fit_batch_loo_grad
    (X, Y, Z, H, S2), probs, refs = _batch(oracle, fam, npts, reg, objective)
    call = lambda sel=slice(None): fit_batch_loo_grad(fam, X[sel], Y[sel], Z[sel], H[sel], S2[sel], reg=reg, objective=objective,
                                                      want_alpha=True)
    al, nll, value, grad, info = call()
    assert value.shape == (5,) and grad.shape == (5, H.shape[1] + 1)
    assert np.all(info == 0) and np.all(np.isfinite(nll))
    # 1. the rows against the host and against the handle; the value against the host and fit_batch_loo's column
    for b in range(5):
        what = "%s reg=%s npts=%d %s row %d" % (fam, reg, npts, objective, b)
        assert probs[b]["cond"] <= 1e8
        G.compare(grad[b], refs[b], what + " vs host")
        with SympFit(fam, X[b], Y[b], Z[b], H[b], S2[b], reg=reg) as f:
            vfit, gfit = f.run().loo_grad(objective)
        _against_the_handle(grad[b], gfit, refs[b], what + " vs SympFit.loo_grad")
        tol = R.tolerance(probs[b]["cond"])
        print("%s: value %.15g  host %.15g  handle %.15g  tol %.3g" % (what, value[b], refs[b]["value"], vfit, tol))
        assert abs(value[b] - refs[b]["value"]) <= tol * abs(refs[b]["value"])
    _, _, loo, info_l = fit_batch_loo(fam, X, Y, Z, H, S2, reg=reg)
    assert _same(value, loo[:, WHICH[objective]]) and np.array_equal(info, info_l)
    # 2. nll, alpha and info are fit_batch's
    al0, nll0, info0 = fit_batch(fam, X, Y, Z, H, S2, reg=reg, want_alpha=True)
    assert np.array_equal(info, info0) and _same(nll, nll0) and _same(al, al0)
    # 3. the bits do not depend on a repetition, the place in the batch or the batch size
    _, _, v2, g2, _ = call()
    assert _same(v2, value) and _same(g2, grad)
    perm = [4, 1, 2, 3, 0]
    _, _, vp, gp, _ = call(perm)
    assert _same(vp, value[perm]) and _same(gp, grad[perm])
    for b in (0, 4):
        _, n1, v1, g1, _ = call(slice(b, b + 1))
        assert _same(v1[0], value[b]) and _same(g1[0], grad[b]) and _same(n1[0], nll[b])


@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
@pytest.mark.parametrize("npts", [37, 128])                                  # n = 74, 256
def test_pairs_all_families(oracle, fam, npts):
    _check_rows(oracle, fam, npts, False, "loo")


@pytest.mark.parametrize("npts,reg,objective", [(70, False, "loo"), (70, False, "press"), (5, False, "loo"),
                                                (129, True, "loo"), (129, True, "press"), (256, True, "loo")])
def test_family_c_other_shapes(oracle, npts, reg, objective):
    _check_rows(oracle, "C", npts, reg, objective)


def test_grid_stride_and_scratch_reuse(oracle):
    """1030 problems (206 copies of the five): more than the 1024 workgroups of the grid, so some workgroups run a second problem
    in the scratch of their first; rows b and b mod 5 agree bit for bit"""
    from sympgpr_amd.fit import fit_batch_loo_grad
    (X, Y, Z, H, S2), _, _ = _batch(oracle, "C", 37, False)
    _, nll, value, grad, info = fit_batch_loo_grad("C", X, Y, Z, H, S2)
    rep = lambda a: np.tile(a, (206,) + (1,) * (a.ndim - 1))
    _, nllb, vb, gb, infob = fit_batch_loo_grad("C", rep(X), rep(Y), rep(Z), rep(H), rep(S2))
    assert vb.shape == (1030,) and gb.shape == (1030, 4) and not infob.any()
    assert _same(vb, rep(value)) and _same(gb, rep(grad)) and _same(nllb, rep(nll))


def test_the_other_batched_calls_keep_their_bits(oracle):
    """fit_batch, fit_batch_grad and fit_batch_loo before and after a fit_batch_loo_grad call on the same data: the arena grew,
    nothing else changed"""
    from sympgpr_amd.fit import fit_batch, fit_batch_grad, fit_batch_loo, fit_batch_loo_grad
    (X, Y, Z, H, S2), _, _ = _batch(oracle, "C", 37, False)

    def others():
        a, n, i = fit_batch("C", X, Y, Z, H, S2)
        _, n2, g, _ = fit_batch_grad("C", X, Y, Z, H, S2)
        _, n3, l, _ = fit_batch_loo("C", X, Y, Z, H, S2)
        return [a, n, i.astype(np.float64), n2, g, n3, l]
    before = others()
    _, _, value, grad, _ = fit_batch_loo_grad("C", X, Y, Z, H, S2)
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad))
    after = others()
    assert all(_same(a, b) for a, b in zip(before, after))


@pytest.mark.parametrize("npts,reg", [(70, False), (129, True)])
def test_indefinite_row(oracle, npts, reg):
    from sympgpr_amd.fit import fit_batch, fit_batch_loo_grad
    (X, Y, Z, H, S2), _, _ = _batch(oracle, "C", npts, reg)
    _, nll, value, grad, info = fit_batch_loo_grad("C", X, Y, Z, H, S2, reg=reg)
    Hb = H.copy()
    Hb[1, -1] = -1.0                                                         # sig < 0: Ky is negative definite but for the noise
    _, nllb, vb, gb, infob = fit_batch_loo_grad("C", X, Y, Z, Hb, S2, reg=reg)
    _, _, info0 = fit_batch("C", X, Y, Z, Hb, S2, reg=reg)
    assert infob[1] > 0 and np.array_equal(infob, info0)
    assert np.isnan(nllb[1]) and np.isnan(vb[1]) and np.all(np.isnan(gb[1]))
    keep = [0, 2, 3, 4]
    assert _same(vb[keep], value[keep]) and _same(gb[keep], grad[keep]) and _same(nllb[keep], nll[keep])


def test_negative_noise_flips_the_last_entry_only(oracle):
    from sympgpr_amd.fit import fit_batch_loo_grad
    (X, Y, Z, H, S2), _, _ = _batch(oracle, "C", 37, False)
    _, nll, value, grad, _ = fit_batch_loo_grad("C", X, Y, Z, H, S2)
    _, nlln, vn, gn, _ = fit_batch_loo_grad("C", X, Y, Z, H, -S2)
    assert _same(vn, value) and _same(nlln, nll) and _same(gn[:, :-1], grad[:, :-1])
    assert np.array_equal(gn[:, -1], -grad[:, -1]) and np.all(grad[:, -1] != 0.0)


def test_press_and_loo_differ(oracle):
    """each objective matches its own reference (test_family_c_other_shapes); here: they are two different gradients and values"""
    from sympgpr_amd.fit import fit_batch_loo_grad
    (X, Y, Z, H, S2), _, refl = _batch(oracle, "C", 70, False, "loo")
    _, _, refp = _batch(oracle, "C", 70, False, "press")
    _, _, vl, gl, _ = fit_batch_loo_grad("C", X, Y, Z, H, S2, objective="loo")
    _, _, vp, gp, _ = fit_batch_loo_grad("C", X, Y, Z, H, S2, objective="press")
    for b in range(5):
        G.compare(gl[b], refl[b], "C npts=70 loo row %d" % b)
        G.compare(gp[b], refp[b], "C npts=70 press row %d" % b)
        assert not _same(gl[b], gp[b]) and vl[b] != vp[b] and vp[b] > 0


def test_differences_of_the_batched_objective(oracle):
    """central differences of fit_batch_loo's own loo, relative step 1e-4 in each of the four entries of row 0 (one batched call
    of eight perturbed rows), against the gradient: |fd - g_k| <= 1e-5 max(|g_k|, 1e-3 max|g|), tests/test_gpu_loo_grad.py's rule"""
    from sympgpr_amd.fit import fit_batch_loo, fit_batch_loo_grad
    (X, Y, Z, H, S2), _, _ = _batch(oracle, "C", 37, False)
    _, _, _, grad, _ = fit_batch_loo_grad("C", X[:1], Y[:1], Z[:1], H[:1], S2[:1])
    g = grad[0]
    theta = np.append(H[0], S2[0])
    rows = np.tile(theta, (8, 1))
    steps = 1e-4 * np.abs(theta)
    for k in range(4):
        rows[2 * k, k] += steps[k]
        rows[2 * k + 1, k] -= steps[k]
    rep = lambda a: np.tile(a[:1], (8,) + (1,) * (a.ndim - 1))
    _, _, loo, info = fit_batch_loo("C", rep(X), rep(Y), rep(Z), rows[:, :-1], rows[:, -1])
    assert not info.any()
    gscale = np.abs(g).max()
    for k in range(4):
        fd = (loo[2 * k, 0] - loo[2 * k + 1, 0]) / (2 * steps[k])
        rel = abs(fd - g[k]) / max(abs(g[k]), 1e-3 * gscale)
        print("component %d  grad %.12g  fd %.12g  rel %.3g" % (k, g[k], fd, rel))
        assert rel <= 1e-5, (k, g[k], fd)


def test_slow_path_above_order_256(oracle):
    """n = 258: the gradient rows are SympFit.loo_grad's, the value fit_batch_loo's, nll fit_batch's, bit for bit"""
    from sympgpr_amd.fit import SympFit, fit_batch, fit_batch_loo, fit_batch_loo_grad
    (X, Y, Z, H, S2), probs, _ = _batch(oracle, "C", 129, False)
    sel = slice(0, 2)
    assert max(p["cond"] for p in probs[:2]) <= 1e8
    _, nll, value, grad, info = fit_batch_loo_grad("C", X[sel], Y[sel], Z[sel], H[sel], S2[sel])
    assert grad.shape == (2, 4) and not info.any()
    for b in range(2):
        with SympFit("C", X[b], Y[b], Z[b], H[b], S2[b]) as f:
            _, gfit = f.run().loo_grad("loo")
        assert _same(grad[b], gfit)
    _, _, loo, _ = fit_batch_loo("C", X[sel], Y[sel], Z[sel], H[sel], S2[sel])
    _, nll0, _ = fit_batch("C", X[sel], Y[sel], Z[sel], H[sel], S2[sel])
    assert _same(value, loo[:, 0]) and _same(nll, nll0)


def test_func_wrapper_and_lbfgs(oracle):
    from scipy.optimize import minimize
    from sympgpr_amd import func
    npts, N = 70, 140
    (X, Y, Z, H, S2), probs, refs = _batch(oracle, "C", npts, False)
    old = func.get_family()
    func.set_family("C")
    try:
        xx = np.concatenate([X[0], Y[0]])
        hyps = np.column_stack([H, S2])
        hyps[:, :-1] = H[0] * np.linspace(0.9, 1.1, 5)[:, None]
        hyps[0, :-1] = H[0]
        values, grads = func.loo_chol_grad_batch(hyps, xx, Z[0], N)
        assert values.shape == (5,) and grads.shape == (5, 4)
        assert _same(values, func.loo_chol_batch(hyps, xx, Z[0], N))
        G.compare(grads[0], refs[0], "loo_chol_grad_batch C N=140 row 0")
        assert abs(values[0] - refs[0]["value"]) <= R.tolerance(probs[0]["cond"]) * abs(refs[0]["value"])
        bad = hyps.copy()
        bad[2, -2] = -1.0
        vb, gb = func.loo_chol_grad_batch(bad, xx, Z[0], N)
        assert np.isnan(vb[2]) and np.all(np.isnan(gb[2]))
        keep = [0, 1, 3, 4]
        assert _same(vb[keep], values[keep]) and _same(gb[keep], grads[keep])
        theta = hyps[0]
        start = theta * np.array([1.25, 0.8, 1.2, 3.0])

        def one(t):
            v, g = func.loo_chol_grad_batch(t[None], xx, Z[0], N)
            return float(v[0]), g[0]
        res = minimize(one, start, jac=True, method="L-BFGS-B", bounds=[(1e-3 * t, 1e3 * t) for t in theta],
                       options={"maxiter": 3})
        f0, f1 = func.loo_chol(start, xx, Z[0], N), func.loo_chol(res.x, xx, Z[0], N)
        print("L-BFGS-B: loo_chol %.6g -> %.6g in %d iterations (%d evaluations); at the fixture's own hyp %.6g" % (
            f0, f1, res.nit, res.nfev, values[0]))
        assert res.nit <= 3 and f1 < f0
    finally:
        func.set_family(old)
