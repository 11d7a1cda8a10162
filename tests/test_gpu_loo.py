"""Leave-one-point-out cross-validation of a device-resident fit (sgpr_fit_loo, SympFit.loo).

Reference: tests/ref_loo.py's block formulas on the oracle's Ky (NumPy, explicit inverse), which tests/test_loo_cpu.py pins to
the definition by deletion.  Tolerance: max(1e-10, 50 cond eps) relative to the max-norm of each array, cond from the fixture.
Shapes: d = 1, N = 37 (one leaf) in every family; reg N = 130 (crosses the 128 leaf); d = 2, N = 40 and d = 3, N = 50 (D = 4, 6:
strided blocks); d = 1, N = 1100 (n = 2200: two default panels, the last of 152 rows, every point's partner row in the other
panel); d = 3, N = 100 with panels of 128 rows (five panels, a point's six rows in up to five of them) in a child process."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ref_loo as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def _case(oracle, fam, kind, N):
    """one problem with its host reference: computed once, shared, never written to"""
    key = (fam, kind, N)
    if key not in _cache:
        p = R.problem(oracle, fam, kind, N, 500 + N)
        ref = R.loo_blocks(p["Ky"], p["z"], N, p["D"])
        for a in list(p.values()) + list(ref.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = (p, ref)
    return _cache[key]


def _fit(fam, kind, p):
    from sympgpr_amd.fit import SympFit
    X = p["X"]
    if kind == "reg":
        return SympFit(fam, X[:, 0], X[:, 1], p["z"], p["hyp"], p["s2"], reg=True)
    if kind == 1:
        return SympFit(fam, X[:, 0], X[:, 1], p["z"], p["hyp"], p["s2"])
    return SympFit.pairs(fam, X, p["z"], p["hyp"], p["s2"])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check(got, ref, p, what):
    N, D = p["N"], p["D"]
    assert got["resid"].shape == (N, D) and got["cov"].shape == (N, D, D) and got["lpd"].shape == (N,)
    R.compare(got, ref, p["cond"], what)
    assert np.array_equal(_bits(got["cov"]), _bits(np.swapaxes(got["cov"], 1, 2)))      # symmetric bit for bit


@pytest.mark.parametrize("fam,kind,N", [("A", 1, 37), ("B", 1, 37), ("C", 1, 37), ("D", 1, 37),
                                        ("C", "reg", 130), ("A", 2, 40), ("C", 3, 50), ("C", 1, 1100)])
def test_against_the_host(oracle, fam, kind, N):
    p, ref = _case(oracle, fam, kind, N)
    assert p["cond"] <= 1e8
    with _fit(fam, kind, p) as f:
        f.run()
        got = f.loo(resid=True, cov=True, lpd=True)
        _check(got, ref, p, "%s %s N=%d" % (fam, kind, N))
        again = f.loo(resid=True, cov=True, lpd=True)
    for k in ("resid", "cov", "lpd"):
        assert np.array_equal(_bits(got[k]), _bits(again[k])), k
    assert _bits(np.array([got["loo"], got["press"]])).tolist() == _bits(np.array([again["loo"], again["press"]])).tolist()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from sympgpr_amd import _lib as L
from sympgpr_amd.fit import SympFit
L.check(L.load_probe_library().sgpr_probe_tune(b"loo_nb", 128.0))
d = np.load(sys.argv[2])
with SympFit.pairs("C", d["X"], d["z"], d["hyp"], float(d["s2"])) as f:
    o = f.run().loo(resid=True, cov=True, lpd=True)
np.savez(sys.argv[3], **o)
"""


def test_five_panels_of_128_rows(oracle, tmp_path):
    """d = 3, N = 100 (n = 600) in a fresh process that sets the loo_nb knob to 128 before its first call"""
    p, ref = _case(oracle, "C", 3, 100)
    assert p["cond"] <= 1e8
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, X=p["X"], z=p["z"], hyp=p["hyp"], s2=p["s2"])
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    o = np.load(fout)
    got = {k: (float(o[k]) if o[k].ndim == 0 else o[k]) for k in o.files}
    _check(got, ref, p, "C d=3 N=100, panels of 128")
    with _fit("C", 3, p) as f:                         # one default panel here: the same numbers to the tolerance
        one = f.run().loo(resid=True, cov=True, lpd=True)
    R.compare(got, one, p["cond"], "panels of 128 vs one panel")


@pytest.mark.parametrize("fam,kind,N", [("C", 1, 1100), ("A", 2, 40), ("C", "reg", 130)])
def test_state_is_left_alone(oracle, fam, kind, N):
    p, _ = _case(oracle, fam, kind, N)
    with _fit(fam, kind, p) as f:
        f.run()
        before = (f.alpha(), np.array([f.nll()]), f.nll_grad_full())
        pr = f.predict_rows(p["X"][:5, 0], p["X"][:5, 1]) if kind == 1 else None
        f.loo(cov=True)
        after = (f.alpha(), np.array([f.nll()]), f.nll_grad_full())
        for a, b in zip(before, after):
            assert np.array_equal(_bits(a), _bits(b))
        if pr is not None:
            pr2 = f.predict_rows(p["X"][:5, 0], p["X"][:5, 1])
            assert np.array_equal(_bits(pr[0]), _bits(pr2[0])) and np.array_equal(_bits(pr[1]), _bits(pr2[1]))


def test_null_outputs_in_every_combination(oracle):
    p, ref = _case(oracle, "A", 2, 40)
    with _fit("A", 2, p) as f:
        f.run()
        full = f.loo(resid=True, cov=True, lpd=True)
        for resid, cov, lpd in itertools.product((False, True), repeat=3):
            o = f.loo(resid=resid, cov=cov, lpd=lpd)
            assert set(o) == {"loo", "press"} | {k for k, on in (("resid", resid), ("cov", cov), ("lpd", lpd)) if on}
            assert o["loo"] == full["loo"] and o["press"] == full["press"]
            for k in set(o) - {"loo", "press"}:
                assert np.array_equal(_bits(o[k]), _bits(full[k]))


def test_unsolved_handle_errors_like_nll_grad_full(oracle):
    import sympgpr_amd
    p, _ = _case(oracle, "A", 1, 37)
    with _fit("A", 1, p) as f:
        with pytest.raises(sympgpr_amd.SympGPRError) as e1:
            f.nll_grad_full()
        with pytest.raises(sympgpr_amd.SympGPRError) as e2:
            f.loo()
        assert type(e1.value) is type(e2.value)
        assert "(%d)" % sympgpr_amd._lib.E_STATE in str(e1.value) and "(%d)" % sympgpr_amd._lib.E_STATE in str(e2.value)
        f.build()
        f.factor()
        with pytest.raises(sympgpr_amd.SympGPRError, match="not solved"):
            f.loo()
    from sympgpr_amd.fit import SympFit
    with SympFit("A", p["X"][:, 0], p["X"][:, 1], p["z"][:37], p["hyp"], p["s2"], block="qq") as f:
        f.run()
        with pytest.raises(sympgpr_amd.SympGPRError, match="single-block"):
            f.loo()
