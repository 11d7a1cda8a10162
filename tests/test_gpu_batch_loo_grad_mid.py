"""One leave-one-point-out objective and its exact gradient for every problem of a batch of mid-order fits, 256 < n <= 2048, on
the device (sgpr_fit_batch_loo_grad_mid, fit.fit_batch_loo_grad_mid, func.loo_chol_grad_batch(mid="device")); both objectives.

Fixtures as the order <= 256 tests draw them: ref_loo.problem(oracle, fam, kind, N, 7000 + 11 N + k), k = 0, 1, 2.  Values against
ref_loo.loo_blocks under ref_loo.compare.  Gradients against ref_loograd.reference under ref_loograd.compare: |g - g_ref| <=
max(1e-9, 100 cond eps) S for the exact components, 1e-6 in place of 1e-9 for the difference-based ones, S = 1/2 sum |W' dKy|; and
against SympFit(...).run().loo_grad(objective) under the exact rule on EVERY component (both are analytic; min |g| / S of these
fixtures is about 1e-7, so the host's difference-based components alone would not pin small gradients).  Every case asserts
cond <= 1e6 and prints cond and err / tol before asserting.

Shapes, the smallest at which each piece can go wrong: pairs N = 129 (n = 258: W = 3 tiles, 126 padding rows, ragged doubling) and
N = 300 (n = 600: W = 5, two-panel factor) in families A - D; reg N = 257 (odd order) in A - D and N = 600 in B; family C at N = 192
(n = 384, no padding), 256 (n = 512) and 550 (n = 1100: W = 9, several row blocks of the contraction); n = 2048 once, against the
handle alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ref_loo as R
from tests import ref_loograd as G
from tests.test_gpu_nll_grad_full import _user_is_c

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COND_MAX = 1e6
OBJECTIVES = ("loo", "press")
_cache = {}


def _batch(oracle, fam, npts, reg):
    """three problems of one shape: the inputs, the problems themselves (for the gradient reference) and the value references"""
    kind = "reg" if reg else 1
    key = (fam, npts, reg)
    if key not in _cache:
        ofam = "C" if fam == "USER" else fam
        probs = [R.problem(oracle, fam, kind, npts, 7000 + 11 * npts + k, ofam=ofam) for k in range(3)]
        vals = [R.loo_blocks(p["Ky"], p["z"], npts, 1 if reg else 2) for p in probs]
        data = (np.array([p["X"][:, 0] for p in probs]), np.array([p["X"][:, 1] for p in probs]), np.array([p["z"] for p in probs]),
                np.array([p["hyp"] for p in probs]), np.array([p["s2"] for p in probs]))
        for a in data:
            a.setflags(write=False)
        _cache[key] = (data, probs, vals)
    return _cache[key]


def _gref(oracle, fam, npts, reg, b, objective):
    """the host gradient reference of problem b: computed once, never modified"""
    key = (fam, npts, reg, b, objective)
    if key not in _cache:
        _, probs, _ = _batch(oracle, fam, npts, reg)
        _cache[key] = G.reference(oracle, fam, "reg" if reg else 1, probs[b], objective, ofam="C" if fam == "USER" else fam)
    return _cache[key]


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(np.atleast_1d(a)).view(np.uint64), np.ascontiguousarray(np.atleast_1d(b)).view(np.uint64))


def _exact(ref):
    """the reference with every component under the exact rule (for analytic against analytic)"""
    return dict(ref, exact=np.ones_like(ref["exact"]))


def _handle(fam, x, y, z, hyp, s2, reg, objective):
    from sympgpr_amd.fit import SympFit
    with SympFit(fam, x, y, z, hyp, s2, reg=reg) as f:
        return f.run().loo_grad(objective)


def _population(fam, npts, reg, B, seed):
    rng = np.random.default_rng(seed)
    X, Y = rng.uniform(0, 2 * np.pi, (B, npts)), rng.uniform(-3, 3, (B, npts))
    Z = rng.standard_normal((B, npts if reg else 2 * npts))
    h, s2 = R.pair_hyp(fam, npts if reg else 2 * npts)
    H = h * rng.uniform(0.9, 1.1, (B, len(h)))
    return X, Y, Z, H, s2 * rng.uniform(0.5, 2.0, B)


def _check_rows(oracle, fam, npts, reg, objective, rows=3):
    from sympgpr_amd.fit import fit_batch_loo_grad_mid
    (X, Y, Z, H, S2), probs, vals = _batch(oracle, fam, npts, reg)
    sel = slice(0, rows)
    _, nll, value, g, info = fit_batch_loo_grad_mid(fam, X[sel], Y[sel], Z[sel], H[sel], S2[sel], reg=reg, objective=objective)
    assert g.shape == (rows, H.shape[1] + 1) and value.shape == (rows,) and np.all(info == 0) and np.all(np.isfinite(nll))
    for b in range(rows):
        what = "%s reg=%s N=%d %s row %d" % (fam, reg, npts, objective, b)
        ref = _gref(oracle, fam, npts, reg, b, objective)
        assert ref["cond"] <= COND_MAX, (what, ref["cond"])
        R.compare({objective: value[b]}, vals[b], ref["cond"], what + " value vs host", (objective,))
        G.compare(g[b], ref, what + " vs host")
        vh, gh = _handle(fam, X[b], Y[b], Z[b], H[b], S2[b], reg, objective)
        G.compare(g[b], dict(_exact(ref), g=gh), what + " vs SympFit.loo_grad")
        R.compare({objective: value[b]}, {objective: vh}, ref["cond"], what + " value vs SympFit.loo_grad", (objective,))


# ---- 1. rows against the host and the handle, both objectives
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
@pytest.mark.parametrize("npts", [129, 300])                                 # n = 258, 600
def test_pairs_all_families(oracle, fam, npts, objective):
    _check_rows(oracle, fam, npts, False, objective)


@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
def test_reg_all_families(oracle, fam, objective):
    _check_rows(oracle, fam, 257, True, objective)


@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("fam,npts,reg", [("B", 600, True), ("C", 192, False), ("C", 256, False), ("C", 550, False)])
def test_other_orders(oracle, fam, npts, reg, objective):
    _check_rows(oracle, fam, npts, reg, objective, rows=2 if npts == 550 else 3)


# ---- 2. the maximum order, against the handle alone
def test_maximum_order_vs_loo_grad(oracle):
    """n = 2048: two problems against SympFit.loo_grad alone.  The tolerance keeps compare's form; its scale S comes from the host's
    W' and dK (no host gradient is compared), its cond from the fit's own estimate, a lower bound of cond_2: the bound is at most the
    one a host reference would give."""
    from sympgpr_amd.fit import SympFit, fit_batch_loo_grad_mid
    npts, fam, objective = 1024, "C", "loo"
    X, Y, Z, H, S2 = _population(fam, npts, False, 2, 2048)
    _, nll, value, g, info = fit_batch_loo_grad_mid(fam, X, Y, Z, H, S2, objective=objective)
    assert np.all(info == 0) and np.all(np.isfinite(nll))
    for b in range(2):
        K = np.array(oracle.build_K(fam, X[b], Y[b], X[b], Y[b], H[b], threads=16))
        Wp, _ = G.weights(K + S2[b] * np.eye(2 * npts), Z[b], npts, 2, objective)
        dKs = list(oracle.build_dK(fam, X[b], Y[b], X[b], Y[b], H[b])) + [K / H[b, -1]]
        _, S = G.contract(Wp, dKs, 1.0)
        with SympFit(fam, X[b], Y[b], Z[b], H[b], S2[b]) as f:
            f.run()
            (vh, gh), cond = f.loo_grad(objective), f.cond_estimate()["cond"]
        assert cond <= COND_MAX
        G.compare(g[b], {"g": gh, "S": S, "exact": np.ones(len(S), bool), "cond": cond}, "n=2048 row %d vs SympFit.loo_grad" % b)
        R.compare({objective: value[b]}, {objective: vh}, cond, "n=2048 row %d value vs SympFit.loo_grad" % b, (objective,))


# ---- 3. the bits
@pytest.mark.parametrize("fam,npts,reg,objective", [("A", 129, False, "loo"), ("D", 300, False, "press"), ("B", 257, True, "loo")])
def test_bits(fam, npts, reg, objective):
    from sympgpr_amd.fit import fit_batch, fit_batch_loo, fit_batch_loo_grad_mid
    X, Y, Z, H, S2 = _population(fam, npts, reg, 4, 50 + npts)
    call = lambda sel=slice(None): fit_batch_loo_grad_mid(fam, X[sel], Y[sel], Z[sel], H[sel], S2[sel], reg=reg, objective=objective,
                                                          want_alpha=True)
    al, nll, value, g, info = call()
    assert np.all(info == 0) and np.all(np.isfinite(g))
    _, nlll, loo, infol = fit_batch_loo(fam, X, Y, Z, H, S2, reg=reg)
    assert _same(value, loo[:, OBJECTIVES.index(objective)]) and _same(nll, nlll) and np.array_equal(info, infol)
    al0, nll0, info0 = fit_batch(fam, X, Y, Z, H, S2, reg=reg, want_alpha=True)
    assert np.array_equal(info, info0) and _same(nll, nll0) and _same(al, al0)
    _, nll2, v2, g2, _ = call()                                              # a repeated call
    assert _same(g2, g) and _same(v2, value) and _same(nll2, nll)
    perm = [3, 1, 2, 0]
    _, _, vp, gp, _ = call(perm)
    assert _same(gp, g[perm]) and _same(vp, value[perm])
    for b in (0, 3):
        _, n1, v1, g1, _ = call(slice(b, b + 1))
        assert _same(g1[0], g[b]) and _same(v1[0], value[b]) and _same(n1[0], nll[b])


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from sympgpr_amd import _lib as L
from sympgpr_amd.fit import fit_batch_loo_grad_mid
L.check(L.load_probe_library().sgpr_probe_tune(b"batch_gradmid_chunk", 2.0))
d = np.load(sys.argv[2])
_, nll, v, g, info = fit_batch_loo_grad_mid("C", d["X"], d["Y"], d["Z"], d["H"], d["S2"], objective="press")
np.savez(sys.argv[3], nll=nll, v=v, g=g, info=info)
"""


def test_bits_across_chunks(tmp_path):
    """five problems of order 384 in chunks of two (three chunks, the last of one problem), in a fresh process that sets the
    batch_gradmid_chunk knob before its first call: the same bits as this process's single chunk"""
    from sympgpr_amd.fit import fit_batch_loo_grad_mid
    X, Y, Z, H, S2 = _population("C", 192, False, 5, 384)
    _, nll, v, g, info = fit_batch_loo_grad_mid("C", X, Y, Z, H, S2, objective="press")
    assert np.all(info == 0)
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, X=X, Y=Y, Z=Z, H=H, S2=S2)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    o = np.load(fout)
    assert np.array_equal(o["info"], info)
    assert _same(o["nll"], nll) and _same(o["v"], v) and _same(o["g"], g)


# ---- 4. an indefinite row, and the sign of sig2n
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_indefinite_row_and_negative_noise(objective):
    from sympgpr_amd.fit import fit_batch, fit_batch_loo_grad_mid
    X, Y, Z, H, S2 = _population("C", 300, False, 3, 600)                    # n = 600
    _, nll, v, g, info = fit_batch_loo_grad_mid("C", X, Y, Z, H, S2, objective=objective)
    assert np.all(info == 0) and np.all(np.isfinite(g))
    Hb = H.copy()
    Hb[1, -1] = -1.0                                                         # sig < 0: Ky indefinite
    _, nllb, vb, gb, infob = fit_batch_loo_grad_mid("C", X, Y, Z, Hb, S2, objective=objective)
    _, _, info0 = fit_batch("C", X, Y, Z, Hb, S2)
    assert infob[1] > 0 and np.array_equal(infob, info0)
    assert np.isnan(nllb[1]) and np.isnan(vb[1]) and np.all(np.isnan(gb[1]))
    keep = [0, 2]
    assert _same(gb[keep], g[keep]) and _same(vb[keep], v[keep]) and _same(nllb[keep], nll[keep])
    S2n = S2.copy()
    S2n[[0, 2]] *= -1.0
    _, nlln, vn, gn, _ = fit_batch_loo_grad_mid("C", X, Y, Z, H, S2n, objective=objective)
    assert _same(nlln, nll) and _same(vn, v) and _same(gn[:, :-1], g[:, :-1])
    assert np.array_equal(gn[:, -1], np.where(S2n < 0, -g[:, -1], g[:, -1])) and np.all(g[:, -1] != 0.0)


# ---- 5. central differences (relative step 1e-5) of fit_batch_loo's own values
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_central_differences_of_the_batch_values(oracle, objective):
    from sympgpr_amd.fit import fit_batch_loo, fit_batch_loo_grad_mid
    fam, npts = "D", 129
    (X, Y, Z, H, S2), _, _ = _batch(oracle, fam, npts, False)
    S = _gref(oracle, fam, npts, False, 0, objective)["S"]
    _, _, _, g, info = fit_batch_loo_grad_mid(fam, X[:1], Y[:1], Z[:1], H[:1], S2[:1], objective=objective)
    assert info[0] == 0
    full = np.append(H[0], S2[0])
    rel = 1e-5
    rows = []
    for k in range(len(full)):
        for sgn in (1, -1):
            h = full.copy()
            h[k] += sgn * rel * abs(full[k])
            rows.append(h)
    rows = np.array(rows)
    rep = lambda a: np.repeat(a[:1], len(rows), 0)
    _, _, loo, info = fit_batch_loo(fam, rep(X), rep(Y), rep(Z), rows[:, :-1], rows[:, -1])
    assert np.all(info == 0)
    v = loo[:, OBJECTIVES.index(objective)]
    fd = (v[0::2] - v[1::2]) / (2 * rel * np.abs(full))
    print("fd %s N=%d %s: max |fd - g| / S %.3g" % (fam, npts, objective, (np.abs(fd - g[0]) / S).max()))
    assert np.all(np.abs(fd - g[0]) <= 1e-5 * S + 1e-6 * np.abs(g[0])), (fd, g[0], np.abs(fd - g[0]) / S)


# ---- 6. the user's family against family C's references
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_user_family_vs_family_c(oracle, golden_dir, objective):
    if not _user_is_c(golden_dir):
        pytest.skip("USER_FAMILY has been edited: no hand-written twin to compare with")
    _check_rows(oracle, "USER", 129, False, objective)


# ---- 7. the wrapper of func
def test_func_wrapper_mid_device(oracle):
    from sympgpr_amd import func
    from sympgpr_amd.fit import fit_batch_loo_grad, fit_batch_loo_grad_mid
    npts, N = 129, 258
    (X, Y, Z, H, S2), _, _ = _batch(oracle, "D", npts, False)
    old = func.get_family()
    func.set_family("D")
    try:
        xx = np.concatenate([X[0], Y[0]])
        Hs = H[0] * np.linspace(0.95, 1.05, 3)[:, None]
        hyps = np.column_stack([Hs, [S2[0], -S2[0], S2[0]]])
        rep = lambda a: np.repeat(a[:1], 3, 0)
        for objective in OBJECTIVES:
            v, g = func.loo_chol_grad_batch(hyps, xx, Z[0], N, objective=objective, mid="device")
            _, _, vb, gb, _ = fit_batch_loo_grad_mid("D", rep(X), rep(Y), rep(Z), hyps[:, :-1], hyps[:, -1], objective=objective)
            assert _same(v, vb) and _same(g, gb)
            # mid=None: still the slow path's bits
            v0, g0 = func.loo_chol_grad_batch(hyps, xx, Z[0], N, objective=objective)
            _, _, vs, gs, _ = fit_batch_loo_grad("D", rep(X), rep(Y), rep(Z), hyps[:, :-1], hyps[:, -1], objective=objective)
            assert _same(v0, vs) and _same(g0, gs) and _same(v0, v)
        bad = hyps.copy()
        bad[1, -2] = -1.0
        vbad, gbad = func.loo_chol_grad_batch(bad, xx, Z[0], N, objective="press", mid="device")
        assert np.isnan(vbad[1]) and np.all(np.isnan(gbad[1])) and _same(vbad[[0, 2]], v[[0, 2]]) and _same(gbad[[0, 2]], g[[0, 2]])
        # at or below order 256 the switch changes nothing
        sub = np.r_[0:50, npts:npts + 50]
        v1, g1 = func.loo_chol_grad_batch(hyps, xx[sub], Z[0][sub], 100, mid="device")
        v2, g2 = func.loo_chol_grad_batch(hyps, xx[sub], Z[0][sub], 100)
        assert _same(v1, v2) and _same(g1, g2)
    finally:
        func.set_family(old)
