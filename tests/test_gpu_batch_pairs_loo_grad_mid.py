"""One leave-one-point-out objective and its exact gradient for every problem of a batch of mid-order fits with d canonical pairs
per point, 256 < n = 2 d N <= 2048, on the device (sgpr_fit_batch_nd_loo_grad_mid, fit.fit_batch_pairs_loo_grad_mid,
func.loo_chol_pairs_grad_batch(mid="device")); both objectives.

Fixtures, references and tolerances as tests/test_gpu_batch_pairs_loo_grad.py: ref_loo.problem(oracle, fam, d, N, 7000 + 11 N + k),
k = 0, 1, 2; values against ref_loo.loo_blocks under ref_loo.compare; gradients against ref_loograd.reference under
ref_loograd.compare (max(1e-9, 100 cond eps) S on exact components, 1e-6 on difference-based ones) and against
SympFit.pairs(...).run().loo_grad(objective) under the exact rule on EVERY component.  Every case asserts cond <= 1e6 and prints
cond and err / tol before asserting.

Shapes: (d, N) = (3, 43) (n = 258: W = 3 tiles, 126 padding rows) and (2, 150) (n = 600: W = 5, two-panel factor) in families
A - D; family A at (2, 275) (n = 1100) and (3, 184) (n = 1104: W = 9, several row blocks of the contraction); (2, 512) (n = 2048)
once, against the handle alone."""
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


def _batch(oracle, fam, d, N):
    """three problems of one shape: the inputs, the problems themselves (for the gradient reference) and the value references"""
    key = (fam, d, N)
    if key not in _cache:
        ofam = "C" if fam == "USER" else fam
        probs = [R.problem(oracle, fam, d, N, 7000 + 11 * N + k, ofam=ofam) for k in range(3)]
        vals = [R.loo_blocks(p["Ky"], p["z"], N, 2 * d) for p in probs]
        data = (np.array([p["X"] for p in probs]), np.array([p["z"] for p in probs]), np.array([p["hyp"] for p in probs]),
                np.array([p["s2"] for p in probs]))
        for a in data:
            a.setflags(write=False)
        _cache[key] = (data, probs, vals)
    return _cache[key]


def _gref(oracle, fam, d, N, b, objective):
    """the host gradient reference of problem b: computed once, never modified"""
    key = (fam, d, N, b, objective)
    if key not in _cache:
        _, probs, _ = _batch(oracle, fam, d, N)
        _cache[key] = G.reference(oracle, fam, d, probs[b], objective, ofam="C" if fam == "USER" else fam)
    return _cache[key]


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(np.atleast_1d(a)).view(np.uint64), np.ascontiguousarray(np.atleast_1d(b)).view(np.uint64))


def _handle(fam, X, z, hyp, s2, objective):
    from sympgpr_amd.fit import SympFit
    with SympFit.pairs(fam, X, z, hyp, s2) as f:
        return f.run().loo_grad(objective)


def _exact(ref):
    """the reference with every component under the exact rule (for analytic against analytic)"""
    return dict(ref, exact=np.ones_like(ref["exact"]))


def _population(fam, d, N, B, seed):
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.uniform(0, 2 * np.pi, (B, N, d)), rng.uniform(-3, 3, (B, N, d))], axis=2)
    Z = rng.standard_normal((B, 2 * d * N))
    h, s2 = R.nd_hyp(fam, N, d)
    H = h * rng.uniform(0.9, 1.1, (B, len(h)))
    return X, Z, H, s2 * rng.uniform(0.5, 2.0, B)


def _check_rows(oracle, fam, d, N, objective, rows=3):
    from sympgpr_amd.fit import fit_batch_pairs_loo_grad_mid
    (X, Z, H, S2), probs, vals = _batch(oracle, fam, d, N)
    sel = slice(0, rows)
    _, nll, value, g, info = fit_batch_pairs_loo_grad_mid(fam, X[sel], Z[sel], H[sel], S2[sel], objective=objective)
    assert g.shape == (rows, H.shape[1] + 1) and value.shape == (rows,) and np.all(info == 0) and np.all(np.isfinite(nll))
    for b in range(rows):
        what = "%s d=%d N=%d (n=%d) %s row %d" % (fam, d, N, 2 * d * N, objective, b)
        ref = _gref(oracle, fam, d, N, b, objective)
        assert ref["cond"] <= COND_MAX, (what, ref["cond"])
        R.compare({objective: value[b]}, vals[b], ref["cond"], what + " value vs host", (objective,))
        G.compare(g[b], ref, what + " vs host")
        vh, gh = _handle(fam, X[b], Z[b], H[b], S2[b], objective)
        G.compare(g[b], dict(_exact(ref), g=gh), what + " vs SympFit.loo_grad")
        R.compare({objective: value[b]}, {objective: vh}, ref["cond"], what + " value vs SympFit.loo_grad", (objective,))


# ---- 1. rows against the host and the handle, both objectives
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
@pytest.mark.parametrize("d,N", [(3, 43), (2, 150)])                         # n = 258, 600
def test_rows_vs_host_and_handle(oracle, fam, d, N, objective):
    _check_rows(oracle, fam, d, N, objective)


@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("d,N", [(2, 275), (3, 184)])                        # n = 1100, 1104
def test_family_a_order_1100(oracle, d, N, objective):
    _check_rows(oracle, "A", d, N, objective, rows=2)


# ---- 2. the maximum order, against the handle alone
def test_maximum_order_vs_loo_grad(oracle):
    """n = 2048 (d = 2, N = 512): two problems against SympFit.pairs(...).loo_grad alone.  The tolerance keeps compare's form; its
    scale S comes from the host's W' and dK (no host gradient is compared; all of family A's d-pair components but sig are
    difference-based on the host), its cond from the fit's own estimate, a lower bound of cond_2."""
    from sympgpr_amd.fit import SympFit, fit_batch_pairs_loo_grad_mid
    fam, d, N, objective = "A", 2, 512, "press"
    X, Z, H, S2 = _population(fam, d, N, 2, 2048)
    _, nll, value, g, info = fit_batch_pairs_loo_grad_mid(fam, X, Z, H, S2, objective=objective)
    assert np.all(info == 0) and np.all(np.isfinite(nll))
    for b in range(2):
        p = {"X": X[b], "hyp": H[b]}
        K = G.builder(oracle, fam, d, X[b])(H[b])
        Wp, _ = G.weights(K + S2[b] * np.eye(2 * d * N), Z[b], N, 2 * d, objective)
        dKs, _ = G.dKy(oracle, fam, d, p)
        _, S = G.contract(Wp, dKs, 1.0)
        with SympFit.pairs(fam, X[b], Z[b], H[b], S2[b]) as f:
            f.run()
            (vh, gh), cond = f.loo_grad(objective), f.cond_estimate()["cond"]
        assert cond <= COND_MAX
        G.compare(g[b], {"g": gh, "S": S, "exact": np.ones(len(S), bool), "cond": cond}, "d=2 n=2048 row %d vs SympFit.loo_grad" % b)
        R.compare({objective: value[b]}, {objective: vh}, cond, "d=2 n=2048 row %d value vs SympFit.loo_grad" % b, (objective,))


# ---- 3. the bits
@pytest.mark.parametrize("fam,d,N,objective", [("A", 3, 43, "press"), ("D", 2, 150, "loo")])
def test_bits(fam, d, N, objective):
    from sympgpr_amd.fit import fit_batch_pairs, fit_batch_pairs_loo, fit_batch_pairs_loo_grad_mid
    X, Z, H, S2 = _population(fam, d, N, 4, 50 + N)
    call = lambda sel=slice(None): fit_batch_pairs_loo_grad_mid(fam, X[sel], Z[sel], H[sel], S2[sel], objective=objective, want_alpha=True)
    al, nll, value, g, info = call()
    assert np.all(info == 0) and np.all(np.isfinite(g))
    _, nlll, loo, infol = fit_batch_pairs_loo(fam, X, Z, H, S2)
    assert _same(value, loo[:, OBJECTIVES.index(objective)]) and _same(nll, nlll) and np.array_equal(info, infol)
    al0, nll0, info0 = fit_batch_pairs(fam, X, Z, H, S2, want_alpha=True)
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
from sympgpr_amd.fit import fit_batch_pairs_loo_grad_mid
L.check(L.load_probe_library().sgpr_probe_tune(b"batch_gradmid_chunk", 2.0))
d = np.load(sys.argv[2])
_, nll, v, g, info = fit_batch_pairs_loo_grad_mid("C", d["X"], d["Z"], d["H"], d["S2"])
np.savez(sys.argv[3], nll=nll, v=v, g=g, info=info)
"""


def test_bits_across_chunks(tmp_path):
    """five problems of order 384 (d = 2, N = 96) in chunks of two (three chunks, the last of one problem), in a fresh process that
    sets the batch_gradmid_chunk knob before its first call: the same bits as this process's single chunk"""
    from sympgpr_amd.fit import fit_batch_pairs_loo_grad_mid
    X, Z, H, S2 = _population("C", 2, 96, 5, 384)
    _, nll, v, g, info = fit_batch_pairs_loo_grad_mid("C", X, Z, H, S2)
    assert np.all(info == 0)
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, X=X, Z=Z, H=H, S2=S2)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    o = np.load(fout)
    assert np.array_equal(o["info"], info)
    assert _same(o["nll"], nll) and _same(o["v"], v) and _same(o["g"], g)


# ---- 4. an indefinite row, and the sign of sig2n
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_indefinite_row_and_negative_noise(objective):
    from sympgpr_amd.fit import fit_batch_pairs, fit_batch_pairs_loo_grad_mid
    X, Z, H, S2 = _population("C", 2, 150, 3, 29)                            # n = 600
    _, nll, v, g, info = fit_batch_pairs_loo_grad_mid("C", X, Z, H, S2, objective=objective)
    assert np.all(info == 0) and np.all(np.isfinite(g))
    Hb = H.copy()
    Hb[1, -1] = -1.3                                                         # sig < 0: Ky indefinite
    _, nllb, vb, gb, infob = fit_batch_pairs_loo_grad_mid("C", X, Z, Hb, S2, objective=objective)
    _, _, info0 = fit_batch_pairs("C", X, Z, Hb, S2)
    assert infob[1] > 0 and np.array_equal(infob, info0)
    assert np.isnan(nllb[1]) and np.isnan(vb[1]) and np.all(np.isnan(gb[1]))
    keep = [0, 2]
    assert _same(gb[keep], g[keep]) and _same(vb[keep], v[keep]) and _same(nllb[keep], nll[keep])
    S2n = S2.copy()
    S2n[[0, 2]] *= -1.0
    _, nlln, vn, gn, _ = fit_batch_pairs_loo_grad_mid("C", X, Z, H, S2n, objective=objective)
    assert _same(nlln, nll) and _same(vn, v) and _same(gn[:, :-1], g[:, :-1])
    assert np.array_equal(gn[:, -1], np.where(S2n < 0, -g[:, -1], g[:, -1])) and np.all(g[:, -1] != 0.0)


# ---- 5. central differences (relative step 1e-5) of fit_batch_pairs_loo's own values
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_central_differences_of_the_batch_values(oracle, objective):
    from sympgpr_amd.fit import fit_batch_pairs_loo, fit_batch_pairs_loo_grad_mid
    fam, d, N = "D", 3, 43
    (X, Z, H, S2), _, _ = _batch(oracle, fam, d, N)
    S = _gref(oracle, fam, d, N, 0, objective)["S"]
    _, _, _, g, info = fit_batch_pairs_loo_grad_mid(fam, X[:1], Z[:1], H[:1], S2[:1], objective=objective)
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
    _, _, loo, info = fit_batch_pairs_loo(fam, X[0], Z[0], rows[:, :-1], rows[:, -1])
    assert np.all(info == 0)
    v = loo[:, OBJECTIVES.index(objective)]
    fd = (v[0::2] - v[1::2]) / (2 * rel * np.abs(full))
    print("fd %s d=%d N=%d %s: max |fd - g| / S %.3g" % (fam, d, N, objective, (np.abs(fd - g[0]) / S).max()))
    assert np.all(np.abs(fd - g[0]) <= 1e-5 * S + 1e-6 * np.abs(g[0])), (fd, g[0], np.abs(fd - g[0]) / S)


# ---- 6. the user's family against family C's references
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_user_family_vs_family_c(oracle, golden_dir, objective):
    if not _user_is_c(golden_dir):
        pytest.skip("USER_FAMILY has been edited: no hand-written twin to compare with")
    _check_rows(oracle, "USER", 3, 43, objective)


# ---- 7. d = 1 through the d-pair entry against the x | y entry: another Gram stage, so the tolerance rule, not the bits
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("fam", ["A", "D"])
def test_d1_against_fit_batch_loo_grad_mid(oracle, fam, objective):
    from sympgpr_amd.fit import fit_batch_loo_grad_mid, fit_batch_pairs_loo_grad_mid
    N = 129
    (X, Z, H, S2), _, vals = _batch(oracle, fam, 1, N)
    _, nll, v, g, info = fit_batch_pairs_loo_grad_mid(fam, X, Z, H, S2, objective=objective)
    _, nll1, v1, g1, info1 = fit_batch_loo_grad_mid(fam, np.ascontiguousarray(X[:, :, 0]), np.ascontiguousarray(X[:, :, 1]), Z, H, S2,
                                                    objective=objective)
    assert np.all(info == 0) and np.all(info1 == 0)
    for b in range(3):
        what = "%s d=1 N=%d %s row %d" % (fam, N, objective, b)
        ref = _gref(oracle, fam, 1, N, b, objective)
        assert ref["cond"] <= COND_MAX
        G.compare(g[b], ref, what + " vs host")
        G.compare(g[b], dict(_exact(ref), g=g1[b]), what + " vs fit_batch_loo_grad_mid")
        R.compare({objective: v[b]}, {objective: v1[b]}, ref["cond"], what + " value vs fit_batch_loo_grad_mid", (objective,))
        assert abs(nll[b] - nll1[b]) <= 1e-10 * abs(nll1[b])


# ---- 8. the wrapper of func
def test_func_wrapper_mid_device():
    from sympgpr_amd import func
    from sympgpr_amd.fit import fit_batch_pairs_loo_grad, fit_batch_pairs_loo_grad_mid
    func.set_family("D")
    try:
        X, Z, H, S2 = _population("D", 2, 65, 3, 12)                         # n = 260
        hyps = np.column_stack([H, [S2[0], -S2[1], S2[2]]])
        for objective in OBJECTIVES:
            v, g = func.loo_chol_pairs_grad_batch(hyps, X[0], Z[0], objective=objective, mid="device")
            assert g.shape == hyps.shape
            _, _, vb, gb, _ = fit_batch_pairs_loo_grad_mid("D", X[0], Z[0], H, np.abs(hyps[:, -1]), objective=objective)
            assert _same(v, vb) and _same(g[:, :-1], gb[:, :-1])
            assert np.array_equal(g[:, -1], np.where(hyps[:, -1] < 0, -gb[:, -1], gb[:, -1]))
            # mid=None: still the slow path's bits
            v0, g0 = func.loo_chol_pairs_grad_batch(hyps, X[0], Z[0], objective=objective)
            _, _, vs, gs, _ = fit_batch_pairs_loo_grad("D", X[0], Z[0], H, np.abs(hyps[:, -1]), objective=objective)
            assert _same(v0, vs) and _same(g0[:, :-1], gs[:, :-1]) and _same(v0, v)
        bad = hyps.copy()
        bad[1, -2] = -1.0
        vbad, gbad = func.loo_chol_pairs_grad_batch(bad, X[0], Z[0], objective="press", mid="device")
        assert np.isnan(vbad[1]) and np.all(np.isnan(gbad[1])) and _same(vbad[[0, 2]], v[[0, 2]]) and _same(gbad[[0, 2]], g[[0, 2]])
        # at or below order 256 the switch changes nothing
        v1, g1 = func.loo_chol_pairs_grad_batch(hyps, X[0][:30], Z[0][np.r_[0:30, 65:95, 130:160, 195:225]], mid="device")
        v2, g2 = func.loo_chol_pairs_grad_batch(hyps, X[0][:30], Z[0][np.r_[0:30, 65:95, 130:160, 195:225]])
        assert _same(v1, v2) and _same(g1, g2)
    finally:
        func.set_family("A")
