"""The NLL gradient of every problem of a batch of mid-order fits, 256 < n <= 2048, on the device (sgpr_fit_batch_grad_mid,
fit.fit_batch_grad_mid, func.nll_chol_grad_batch(mid="device")).

Reference and tolerance are those of tests/test_gpu_batch_grad.py: the host gradient from the oracle's Gram builders and every
row against SympFit.nll_grad_full, each component within max(1e-9, 100 cond eps) S (1e-6 for difference-based components).
Orders: 258 (W = 3 tiles, 126 padding rows, ragged doubling), 384 (no padding), 512 (the one-panel limit, a power of two),
600 (two-panel factor, W = 5), 1100 (W = 9, first panel of 5), reg 257 (odd) and 1025, and 2048 (W = 16, the maximum).  Also:
nll / alpha / info bits against fit_batch, gradient bits independent of repetition, position, batch and chunking, an
indefinite row, the sign of sig2n, central differences of the batch's own nll, and the func wrapper."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_batch_grad import _batch, _compare, _population, _problem
from tests.test_gpu_nll_grad_full import EPS, _pair_hyp, _reference, _user_is_c

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def _shared_batch(oracle, fam, npts, reg, ofam=None):
    """two problems of one shape with their host references: computed once, shared, never written to"""
    key = (fam, npts, reg, ofam)
    if key not in _cache:
        _cache[key] = _batch(oracle, fam, npts, reg, [4000 + 3 * npts + k for k in range(2)], ofam)
        for a in _cache[key][0]:
            a.setflags(write=False)
    return _cache[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_rows(fam, data, refs, reg, what):
    from sympgpr_amd.fit import SympFit, fit_batch_grad_mid
    X, Y, Z, H, S2 = data
    _, nll, g, info = fit_batch_grad_mid(fam, X, Y, Z, H, S2, reg=reg)
    assert g.shape == (len(X), H.shape[1] + 1) and np.all(info == 0) and np.all(np.isfinite(nll))
    for b in range(len(X)):
        _compare(g[b], refs[b], "%s row %d vs host" % (what, b))
        with SympFit(fam, X[b], Y[b], Z[b], H[b], S2[b], reg=reg) as f:
            _compare(g[b], (f.run().nll_grad_full(),) + refs[b][1:], "%s row %d vs nll_grad_full" % (what, b))


@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
@pytest.mark.parametrize("npts", [129, 300])                              # n = 258, 600
def test_pairs_all_families(oracle, fam, npts):
    data, refs = _shared_batch(oracle, fam, npts, False)
    _check_rows(fam, data, refs, False, "pairs %s n=%d" % (fam, 2 * npts))


@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
def test_reg_all_families(oracle, fam):
    data, refs = _shared_batch(oracle, fam, 257, True)
    _check_rows(fam, data, refs, True, "reg %s n=257" % fam)


@pytest.mark.parametrize("npts,reg", [(192, False), (256, False), (550, False), (1025, True)])    # n = 384, 512, 1100; reg 1025
def test_family_c_other_orders(oracle, npts, reg):
    data, refs = _shared_batch(oracle, "C", npts, reg)
    _check_rows("C", data, refs, reg, "C reg=%s npts=%d" % (reg, npts))


def test_user_family_vs_family_c(oracle, golden_dir):
    if not _user_is_c(golden_dir):
        pytest.skip("USER_FAMILY has been edited: no hand-written twin to compare with")
    from sympgpr_amd.fit import fit_batch_grad_mid
    (X, Y, Z, H, S2), refs = _shared_batch(oracle, "USER", 129, False, ofam="C")
    _, _, g, info = fit_batch_grad_mid("USER", X, Y, Z, H, S2)
    assert np.all(info == 0)
    for b in range(2):
        _compare(g[b], refs[b], "USER (= C) n=258")


def test_maximum_order_vs_nll_grad_full(oracle):
    """n = 2048: two problems against SympFit.nll_grad_full alone.  The tolerance keeps _compare's form; its scale S comes from
    the host's W and dK (no host gradient is compared), its cond from the fit's own estimate, a lower bound of cond_2: the
    bound is at most the one a host reference would give."""
    from sympgpr_amd.fit import SympFit, fit_batch_grad_mid
    npts, fam = 1024, "C"
    X, Y, Z, H, S2 = _population(fam, npts, False, 2, 2048)
    _, nll, g, info = fit_batch_grad_mid(fam, X, Y, Z, H, S2)
    assert np.all(info == 0) and np.all(np.isfinite(nll))
    for b in range(2):
        K = oracle.build_K(fam, X[b], Y[b], X[b], Y[b], H[b], threads=16)
        Kinv = np.linalg.inv(K + S2[b] * np.eye(2 * npts))
        al = Kinv @ Z[b]
        Wm = np.abs(0.5 * (Kinv + Kinv.T) - np.outer(al, al))
        dKs = list(oracle.build_dK(fam, X[b], Y[b], X[b], Y[b], H[b])) + [K / H[b, -1]]
        S = np.array([0.5 * np.sum(Wm * np.abs(d)) for d in dKs] + [0.5 * (np.trace(np.abs(Kinv)) + al @ al)])
        with SympFit(fam, X[b], Y[b], Z[b], H[b], S2[b]) as f:
            f.run()
            gf, cond = f.nll_grad_full(), f.cond_estimate()["cond"]
        print("n=2048 row %d: cond >= %.3e, |g - g_full| / S = %s" % (b, cond, np.abs(g[b] - gf) / S))
        _compare(g[b], (gf, S, cond, np.ones(len(S), bool)), "n=2048 row %d vs nll_grad_full" % b)


@pytest.mark.parametrize("fam,npts,reg", [("A", 129, False), ("D", 300, False), ("C", 550, False), ("B", 257, True)])
def test_bits(fam, npts, reg):
    from sympgpr_amd.fit import fit_batch, fit_batch_grad_mid
    X, Y, Z, H, S2 = _population(fam, npts, reg, 4, 50 + npts)
    al, nll, g, info = fit_batch_grad_mid(fam, X, Y, Z, H, S2, reg=reg, want_alpha=True)
    assert np.all(info == 0)
    al0, nll0, info0 = fit_batch(fam, X, Y, Z, H, S2, reg=reg, want_alpha=True)
    assert np.array_equal(info, info0)
    assert np.array_equal(_bits(nll), _bits(nll0))
    assert np.array_equal(_bits(al), _bits(al0))
    _, nll2, g2, _ = fit_batch_grad_mid(fam, X, Y, Z, H, S2, reg=reg)       # a repeated call
    assert np.array_equal(_bits(g), _bits(g2)) and np.array_equal(_bits(nll2), _bits(nll))
    for b in (0, 3):                                                        # alone, and at another position of a permuted batch
        _, n1, g1, _ = fit_batch_grad_mid(fam, X[b:b + 1], Y[b:b + 1], Z[b:b + 1], H[b:b + 1], S2[b:b + 1], reg=reg)
        assert np.array_equal(_bits(g1[0]), _bits(g[b])) and n1[0] == nll[b]
        perm = [2, b, 1]
        _, _, g3, _ = fit_batch_grad_mid(fam, X[perm], Y[perm], Z[perm], H[perm], S2[perm], reg=reg)
        assert np.array_equal(_bits(g3[1]), _bits(g[b]))


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from sympgpr_amd import _lib as L
from sympgpr_amd.fit import fit_batch_grad_mid
L.check(L.load_probe_library().sgpr_probe_tune(b"batch_gradmid_chunk", 2.0))
d = np.load(sys.argv[2])
_, nll, g, info = fit_batch_grad_mid("C", d["X"], d["Y"], d["Z"], d["H"], d["S2"])
np.savez(sys.argv[3], nll=nll, g=g, info=info)
"""


def test_bits_across_chunks(tmp_path):
    """five problems of order 384 in chunks of two (three chunks, the last of one problem), in a fresh process that sets the
    batch_gradmid_chunk knob before its first call: the same bits as this process's single chunk"""
    from sympgpr_amd.fit import fit_batch_grad_mid
    X, Y, Z, H, S2 = _population("C", 192, False, 5, 384)
    _, nll, g, info = fit_batch_grad_mid("C", X, Y, Z, H, S2)
    assert np.all(info == 0)
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, X=X, Y=Y, Z=Z, H=H, S2=S2)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    o = np.load(fout)
    assert np.array_equal(o["info"], info)
    assert np.array_equal(_bits(o["nll"]), _bits(nll))
    assert np.array_equal(_bits(o["g"]), _bits(g))


def test_indefinite_row_and_negative_noise():
    from sympgpr_amd.fit import fit_batch, fit_batch_grad_mid
    X, Y, Z, H, S2 = _population("C", 300, False, 3, 600)                  # n = 600
    _, nll, g, info = fit_batch_grad_mid("C", X, Y, Z, H, S2)
    assert np.all(info == 0)
    Hb = H.copy()
    Hb[1, -1] = -1.0                                                        # sig < 0: Ky indefinite
    _, nllb, gb, infob = fit_batch_grad_mid("C", X, Y, Z, Hb, S2)
    _, nll0, info0 = fit_batch("C", X, Y, Z, Hb, S2)
    assert infob[1] > 0 and np.array_equal(infob, info0)
    assert np.isnan(nllb[1]) and np.all(np.isnan(gb[1]))
    keep = [0, 2]
    _, nllk, gk, _ = fit_batch_grad_mid("C", X[keep], Y[keep], Z[keep], H[keep], S2[keep])      # the batch without the bad row
    assert np.array_equal(_bits(gb[keep]), _bits(gk)) and np.array_equal(_bits(gb[keep]), _bits(g[keep]))
    assert np.array_equal(_bits(nllb[keep]), _bits(nllk))
    S2n = S2.copy()
    S2n[[0, 2]] *= -1.0
    _, nlln, gn, _ = fit_batch_grad_mid("C", X, Y, Z, H, S2n)
    assert np.array_equal(_bits(nlln), _bits(nll))
    assert np.array_equal(_bits(gn[:, :-1]), _bits(g[:, :-1]))
    assert np.array_equal(gn[:, -1], np.where(S2n < 0, -g[:, -1], g[:, -1]))


@pytest.mark.parametrize("fam,npts,reg", [("D", 129, False), ("A", 257, True)])
def test_central_differences_of_batch_nll(oracle, fam, npts, reg):
    from sympgpr_amd.fit import fit_batch, fit_batch_grad_mid
    (x, y, z, hyp, s2), ref = _problem(oracle, fam, npts, reg, 77 + npts)
    _, _, g, _ = fit_batch_grad_mid(fam, x[None], y[None], z[None], hyp[None], s2, reg=reg)
    full = np.append(hyp, s2)
    rel = 1e-5
    rows = []
    for k in range(len(full)):
        for sgn in (1, -1):
            h = full.copy()
            h[k] += sgn * rel * abs(full[k])
            rows.append(h)
    rows = np.array(rows)
    B = len(rows)
    _, nll, info = fit_batch(fam, np.repeat(x[None], B, 0), np.repeat(y[None], B, 0), np.repeat(z[None], B, 0), rows[:, :-1],
                             rows[:, -1], reg=reg)
    assert np.all(info == 0)
    fd = (nll[0::2] - nll[1::2]) / (2 * rel * np.abs(full))
    S = ref[1]
    assert np.all(np.abs(fd - g[0]) <= 1e-5 * S + 1e-6 * np.abs(g[0])), (fd, g[0], np.abs(fd - g[0]) / S)


def test_func_wrapper_mid_device(oracle):
    from sympgpr_amd import func
    from sympgpr_amd.fit import SympFit
    func.set_family("C")
    try:
        (x, y, z, hyp, s2), ref0 = _problem(oracle, "C", 150, False, 300)  # N = 300
        hyp1 = hyp * np.array([1.07, 0.94, 1.1])
        build = lambda h: oracle.build_K("C", x, y, x, y, h, threads=16)
        ref1 = _reference(build, hyp1, s2, z, dict(enumerate(oracle.build_dK("C", x, y, x, y, hyp1))))
        hyps = np.array([np.append(hyp, s2), np.append(hyp1, s2)])
        xx = np.concatenate([x, y])
        nll_d, g_d = func.nll_chol_grad_batch(hyps, xx, z, 300, mid="device")
        nll_h, g_h = func.nll_chol_grad_batch(hyps, xx, z, 300)
        assert np.array_equal(_bits(nll_d), _bits(nll_h))
        for b, ref in enumerate((ref0, ref1)):
            _compare(g_d[b], (g_h[b],) + ref[1:], "mid=device vs mid=None row %d" % b)
            _compare(g_d[b], ref, "mid=device vs host row %d" % b)
            with SympFit("C", x, y, z, hyps[b, :-1], hyps[b, -1]) as f:
                assert np.array_equal(f.run().nll_grad_full(), g_h[b])     # mid=None: still the slow path's bits
        bad = hyps.copy()
        bad[1, -2] = -1.0
        for mid in (None, "device"):
            nb, gbad = func.nll_chol_grad_batch(bad, xx, z, 300, mid=mid)
            assert nb[1] == np.inf and np.all(np.isnan(gbad[1])) and nb[0] == nll_h[0]
            assert np.array_equal(_bits(gbad[0]), _bits((g_h if mid is None else g_d)[0]))
        # at or below order 256 the switch changes nothing
        n1, g1 = func.nll_chol_grad_batch(hyps, xx[np.r_[0:50, 150:200]], z[np.r_[0:50, 150:200]], 100, mid="device")
        n0, g0 = func.nll_chol_grad_batch(hyps, xx[np.r_[0:50, 150:200]], z[np.r_[0:50, 150:200]], 100)
        assert np.array_equal(_bits(n1), _bits(n0)) and np.array_equal(_bits(g1), _bits(g0))
    finally:
        func.set_family("A")
