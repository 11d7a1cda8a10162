"""Leave-one-point-out cross-validation of every problem of a batch (sgpr_fit_batch_loo, fit.fit_batch_loo, func.loo_chol,
loo_chol_reg, loo_chol_batch).

Reference and tolerance as tests/test_gpu_loo.py: tests/ref_loo.py's block formulas on the oracle's Ky, max(1e-10, 50 cond eps)
relative to each quantity's magnitude, cond from the fixture; every row also against SympFit(...).run().loo().  Orders: 74 (one
leaf), 140 (two leaves), 256 (the one-launch kernel's maximum), 258 (the mid path's minimum: npad = 384, W = 3, ragged
doubling), reg 257 and reg 600; every family at 74 and 258, C elsewhere; batches of five."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ref_loo as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("loo", "press")
_cache = {}


def _batch(oracle, fam, npts, reg):
    """five problems of one shape with their host references: computed once, shared, never written to"""
    key = (fam, npts, reg)
    if key not in _cache:
        probs = [R.problem(oracle, fam, "reg" if reg else 1, npts, 7000 + 11 * npts + k) for k in range(5)]
        refs = [R.loo_blocks(p["Ky"], p["z"], npts, p["D"]) for p in probs]
        data = (np.array([p["X"][:, 0] for p in probs]), np.array([p["X"][:, 1] for p in probs]), np.array([p["z"] for p in probs]),
                np.array([p["hyp"] for p in probs]), np.array([p["s2"] for p in probs]))
        for a in data:
            a.setflags(write=False)
        _cache[key] = (data, refs, [p["cond"] for p in probs])
    return _cache[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_rows(oracle, fam, npts, reg):
    from sympgpr_amd.fit import SympFit, fit_batch, fit_batch_loo
    (X, Y, Z, H, S2), refs, conds = _batch(oracle, fam, npts, reg)
    al, nll, loo, info = fit_batch_loo(fam, X, Y, Z, H, S2, reg=reg, want_alpha=True)
    assert loo.shape == (5, 2) and np.all(info == 0) and np.all(np.isfinite(nll))
    for b in range(5):
        what = "%s reg=%s npts=%d row %d" % (fam, reg, npts, b)
        assert conds[b] <= 1e8
        got = {"loo": loo[b, 0], "press": loo[b, 1]}
        R.compare(got, refs[b], conds[b], what + " vs host", KEYS)
        with SympFit(fam, X[b], Y[b], Z[b], H[b], S2[b], reg=reg) as f:
            R.compare(got, f.run().loo(resid=False, lpd=False), conds[b], what + " vs SympFit.loo", KEYS)
    al0, nll0, info0 = fit_batch(fam, X, Y, Z, H, S2, reg=reg, want_alpha=True)
    assert np.array_equal(info, info0)
    assert np.array_equal(_bits(nll), _bits(nll0)) and np.array_equal(_bits(al), _bits(al0))
    _, _, again, _ = fit_batch_loo(fam, X, Y, Z, H, S2, reg=reg)                         # a repeated call
    assert np.array_equal(_bits(again), _bits(loo))
    perm = [4, 1, 2, 3, 0]                                                              # positions 0 and 4 swapped
    _, _, lp, _ = fit_batch_loo(fam, X[perm], Y[perm], Z[perm], H[perm], S2[perm], reg=reg)
    assert np.array_equal(_bits(lp), _bits(loo[perm]))
    for b in (0, 4):                                                                    # a batch of one
        _, n1, l1, _ = fit_batch_loo(fam, X[b:b + 1], Y[b:b + 1], Z[b:b + 1], H[b:b + 1], S2[b:b + 1], reg=reg)
        assert np.array_equal(_bits(l1[0]), _bits(loo[b])) and n1[0] == nll[b]


@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
@pytest.mark.parametrize("npts", [37, 129])                                  # n = 74, 258
def test_pairs_all_families(oracle, fam, npts):
    _check_rows(oracle, fam, npts, False)


@pytest.mark.parametrize("npts,reg", [(70, False), (128, False), (257, True), (600, True)])    # n = 140, 256; reg 257, 600
def test_family_c_other_orders(oracle, npts, reg):
    _check_rows(oracle, "C", npts, reg)


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from sympgpr_amd import _lib as L
from sympgpr_amd.fit import fit_batch_loo
L.check(L.load_probe_library().sgpr_probe_tune(b"batch_gradmid_chunk", 2.0))
d = np.load(sys.argv[2])
_, nll, loo, info = fit_batch_loo("C", d["X"], d["Y"], d["Z"], d["H"], d["S2"])
np.savez(sys.argv[3], nll=nll, loo=loo, info=info)
"""


def test_bits_across_chunks(oracle, tmp_path):
    """five problems of order 384 in chunks of two (three chunks, the last of one problem), in a fresh process that sets the
    batch_gradmid_chunk knob before its first call: the same bits as this process's single chunk"""
    from sympgpr_amd.fit import fit_batch_loo
    (X, Y, Z, H, S2), refs, conds = _batch(oracle, "C", 192, False)
    _, nll, loo, info = fit_batch_loo("C", X, Y, Z, H, S2)
    assert np.all(info == 0)
    for b in range(5):
        R.compare({"loo": loo[b, 0], "press": loo[b, 1]}, refs[b], conds[b], "C n=384 row %d" % b, KEYS)
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, X=X, Y=Y, Z=Z, H=H, S2=S2)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    o = np.load(fout)
    assert np.array_equal(o["info"], info)
    assert np.array_equal(_bits(o["nll"]), _bits(nll))
    assert np.array_equal(_bits(o["loo"]), _bits(loo))


@pytest.mark.parametrize("npts", [70, 129])                                  # the one-launch kernel and the mid path
def test_indefinite_row(oracle, npts):
    from sympgpr_amd.fit import fit_batch, fit_batch_loo
    (X, Y, Z, H, S2), _, _ = _batch(oracle, "C", npts, False)
    _, nll, loo, info = fit_batch_loo("C", X, Y, Z, H, S2)
    Hb = H.copy()
    Hb[1, -1] = -1.0                                                         # sig < 0: Ky is negative definite but for the noise
    _, nllb, loob, infob = fit_batch_loo("C", X, Y, Z, Hb, S2)
    _, _, info0 = fit_batch("C", X, Y, Z, Hb, S2)
    assert infob[1] > 0 and np.array_equal(infob, info0)
    assert np.isnan(nllb[1]) and np.all(np.isnan(loob[1]))
    keep = [0, 2, 3, 4]
    assert np.array_equal(_bits(loob[keep]), _bits(loo[keep])) and np.array_equal(_bits(nllb[keep]), _bits(nll[keep]))
    S2n = -S2                                                                # the noise enters as |sig2n|
    _, nlln, loon, _ = fit_batch_loo("C", X, Y, Z, H, S2n)
    assert np.array_equal(_bits(loon), _bits(loo)) and np.array_equal(_bits(nlln), _bits(nll))


def test_func_wrappers(oracle):
    from sympgpr_amd import func
    func.set_family("C")
    try:
        for npts, reg in ((70, False), (129, False), (257, True)):
            (X, Y, Z, H, S2), refs, conds = _batch(oracle, "C", npts, reg)
            N = npts if reg else 2 * npts
            xx = np.concatenate([X[0], Y[0]])
            hyps = np.column_stack([H, S2])
            hyps[:, :-1] = H[0] * np.linspace(0.9, 1.1, 5)[:, None]
            hyps[0, :-1] = H[0]
            v = func.loo_chol_batch(hyps, xx, Z[0], N, reg=reg)
            assert v.shape == (5,)
            R.compare({"loo": v[0]}, refs[0], conds[0], "loo_chol_batch C N=%d" % N, ("loo",))
            one = func.loo_chol_reg if reg else func.loo_chol
            for b in (0, 3):
                assert _bits(np.array([one(hyps[b], xx, Z[0], N)]))[0] == _bits(v[b:b + 1])[0]
            bad = hyps.copy()
            bad[2, -2] = -1.0
            vb = func.loo_chol_batch(bad, xx, Z[0], N, reg=reg)
            assert np.isnan(vb[2]) and np.array_equal(_bits(vb[[0, 1, 3, 4]]), _bits(v[[0, 1, 3, 4]]))
            with pytest.raises(np.linalg.LinAlgError):
                one(bad[2], xx, Z[0], N)
    finally:
        func.set_family("A")


def test_order_above_the_batch_maximum_goes_through_a_handle(oracle):
    from sympgpr_amd import func
    npts = 1025                                                              # n = 2050
    p = R.problem(oracle, "C", 1, npts, 31)
    assert p["cond"] <= 1e8
    ref = R.loo_blocks(p["Ky"], p["z"], npts, 2)
    func.set_family("C")
    try:
        xx = np.concatenate([p["X"][:, 0], p["X"][:, 1]])
        hyp = np.append(p["hyp"], p["s2"])
        v = func.loo_chol(hyp, xx, p["z"], 2 * npts)
        R.compare({"loo": v}, ref, p["cond"], "loo_chol n=2050", ("loo",))
        vb = func.loo_chol_batch(hyp[None], xx, p["z"], 2 * npts)
        assert vb.shape == (1,) and vb[0] == v
    finally:
        func.set_family("A")
