"""GPU parity of the batched fits with d canonical pairs per point (sgpr_fit_batch_nd / fit.fit_batch_pairs: one launch up to
order 256, the mid path up to 2048) against the CPU oracle's fit_nd, problem by problem.  Inputs as test_fit_pairs_vs_oracle:
q ~ U(0, 2 pi), P ~ U(-3, 3), l = 1.2 (12 pi / N)^(1 / 2d) times a per-problem factor in U(0.8, 1.25), s2 = 1e-2 / l^2, periods
0.5 for family D.  Acceptance as test_gpu_batch.py: alpha within max(1e-10, 50 cond eps) (cond of the oracle's Ky), nll rel 1e-10,
abs 1e-10."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.2e-16


def _problems(rng, B, N, d, has_p=False):
    X = np.concatenate([rng.uniform(0, 2 * np.pi, (B, N, d)), rng.uniform(-3, 3, (B, N, d))], axis=2)
    l = 1.2 * (12 * np.pi / N) ** (1.0 / (2 * d)) * rng.uniform(0.8, 1.25, B)
    cols = [np.tile(l[:, None], (1, 2 * d))]
    if has_p:
        cols.append(np.full((B, d), 0.5))
    cols.append(np.ones((B, 1)))
    return X, rng.standard_normal((B, 2 * d * N)), np.hstack(cols), 1e-2 / l**2


def _check(oracle, fam, X, z, hyp, s2, al, nll, rows=None):
    for b in (range(len(hyp)) if rows is None else rows):
        a_o, nll_o, _ = oracle.fit_nd(fam, X[b], z[b], hyp[b], s2[b])
        Ky = oracle.build_K_nd(fam, X[b], X[b], hyp[b]) + s2[b] * np.eye(z.shape[1])
        rel, bound = np.linalg.norm(al[b] - a_o) / np.linalg.norm(a_o), max(1e-10, 50 * np.linalg.cond(Ky) * EPS)
        print("fam %s n %d problem %d: alpha rel %.3e (bound %.3e)  nll %.15g (oracle %.15g)" % (fam, z.shape[1], b, rel, bound,
                                                                                              nll[b], nll_o))
        assert rel < bound
        assert nll[b] == pytest.approx(nll_o, rel=1e-10, abs=1e-10)


@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
@pytest.mark.parametrize("d,N", [(2, 1), (2, 7), (2, 32), (2, 33), (2, 64), (3, 21), (3, 22), (3, 42)])
def test_one_launch_path_vs_oracle(oracle, fam, d, N):
    """orders 4 ... 256: one leaf (d = 2: n = 128 exactly; d = 3: 126), the first two-leaf orders (132) and BMAX = 256 / 252;
    family B has all-zero off-diagonal blocks"""
    from sympgpr_amd.fit import fit_batch_pairs
    rng = np.random.default_rng(1000 * d + 10 * N + ord(fam))
    X, z, hyp, s2 = _problems(rng, 5, N, d, fam == "D")
    al, nll, info = fit_batch_pairs(fam, X, z, hyp, s2)
    assert np.all(info == 0)
    _check(oracle, fam, X, z, hyp, s2, al, nll)


@pytest.mark.parametrize("fam,d,N,B", [("A", 3, 43, 4), ("C", 2, 128, 4), ("D", 2, 160, 4), ("B", 3, 171, 4), ("A", 3, 341, 3),
                                       ("C", 2, 512, 3)])
def test_mid_path_vs_oracle(oracle, fam, d, N, B):
    """n = 258 (padded to 384), 512 (the last one-panel order), 640 (two panels), 1026, 2046 (padded to 2048), 2048"""
    from sympgpr_amd.fit import fit_batch_pairs
    rng = np.random.default_rng(1000 * d + N)
    X, z, hyp, s2 = _problems(rng, B, N, d, fam == "D")
    al, nll, info = fit_batch_pairs(fam, X, z, hyp, s2)
    assert np.all(info == 0)
    _check(oracle, fam, X, z, hyp, s2, al, nll)


@pytest.mark.parametrize("d,N", [(2, 20), (3, 22), (2, 70)])
def test_user_family(oracle, d, N):
    """Family USER: the oracle has no d-pair form of the user's kernel (build_K_nd raises), so this is device against device --
    every row against a SympFit.pairs("USER", ...) handle on the same problem, alpha 1e-10, nll rel 1e-10."""
    from sympgpr_amd import _lib as L
    from sympgpr_amd.fit import SympFit, fit_batch_pairs
    rng = np.random.default_rng(77 * d + N)
    X, z, hyp, s2 = _problems(rng, 4, N, d, L.family_has_p("USER"))
    try:
        oracle.build_K_nd("USER", X[0], X[0], hyp[0])
        have_oracle = True
    except (KeyError, ValueError):
        have_oracle = False
    al, nll, info = fit_batch_pairs("USER", X, z, hyp, s2)
    assert np.all(info == 0)
    if have_oracle:
        _check(oracle, "USER", X, z, hyp, s2, al, nll)
        return
    for b in range(4):
        with SympFit.pairs("USER", X[b], z[b], hyp[b], s2[b]) as f:
            f.run()
            a_h, nll_h = f.alpha(), f.nll()
        assert np.linalg.norm(al[b] - a_h) / np.linalg.norm(a_h) < 1e-10
        assert nll[b] == pytest.approx(nll_h, rel=1e-10)


@pytest.mark.parametrize("fam", ["A", "D"])
@pytest.mark.parametrize("N", [40, 128, 200])
def test_d1_through_the_new_entry_agrees_with_fit_batch(oracle, fam, N):
    """d = 1 is sgpr_fit_batch's problem with the d-pair entry formulas: a different evaluation order of the same Gram matrix, so
    not the same bits.  Both Gram matrices carry relative rounding errors of a few eps per entry; two solves of systems that
    differ by that much differ by at most ~cond eps in alpha: the oracle tests' bound max(1e-10, 50 cond eps)."""
    from sympgpr_amd.fit import fit_batch, fit_batch_pairs
    rng = np.random.default_rng(N + ord(fam))
    X, z, hyp, s2 = _problems(rng, 4, N, 1, fam == "D")
    a1, nll1, info1 = fit_batch(fam, X[:, :, 0], X[:, :, 1], z, hyp, s2)
    a2, nll2, info2 = fit_batch_pairs(fam, X, z, hyp, s2)
    assert np.all(info1 == 0) and np.all(info2 == 0)
    for b in range(4):
        Ky = oracle.build_K(fam, X[b, :, 0], X[b, :, 1], X[b, :, 0], X[b, :, 1], hyp[b]) + s2[b] * np.eye(2 * N)
        assert np.linalg.norm(a2[b] - a1[b]) / np.linalg.norm(a1[b]) < max(1e-10, 50 * np.linalg.cond(Ky) * EPS)
        assert nll2[b] == pytest.approx(nll1[b], rel=1e-12)


def test_population_over_one_data_set(oracle):
    """a CMA-ES generation of a d = 2 fit: 12 hyper-parameter rows over one data set; one row with sig < 0 is not positive
    definite -- +inf, info the index LAPACK's dpotrf reports for the oracle's Ky -- and leaves its neighbours alone"""
    import scipy.linalg
    from sympgpr_amd import func
    from sympgpr_amd.fit import fit_batch_pairs
    rng = np.random.default_rng(21)
    d, N = 2, 20
    X, z, _, _ = _problems(rng, 1, N, d)
    X, z = X[0], z[0]
    rows = np.column_stack((rng.uniform(1.2, 2.2, (12, 2 * d)), rng.uniform(0.5, 2.0, 12), rng.uniform(1e-3, 1e-2, 12)))
    rows[5, 2 * d] = -3.0
    rows[5, 2 * d + 1] = 0.1
    func.set_family("A")
    got = func.nll_chol_pairs_batch(rows, X, z)
    _, _, info = fit_batch_pairs("A", X, z, rows[:, :-1], rows[:, -1])
    for b, h in enumerate(rows):
        one = func.nll_chol_pairs(h, X, z)
        if b == 5:
            Ky = oracle.build_K_nd("A", X, X, h[:-1]) + h[-1] * np.eye(2 * d * N)
            expect = scipy.linalg.lapack.dpotrf(Ky, lower=1)[1]
            assert expect > 0 and info[b] == expect and got[b] == np.inf and one == np.inf
            continue
        assert info[b] == 0
        _, nll_o, _ = oracle.fit_nd("A", X, z, h[:-1], h[-1])
        assert got[b] == pytest.approx(nll_o, rel=1e-10, abs=1e-10)
        assert got[b] == one                                   # the same problem alone: the same bits


def test_more_problems_than_workgroups(oracle):
    from sympgpr_amd.fit import fit_batch_pairs
    rng = np.random.default_rng(22)
    B, d, N = 1500, 2, 10
    X, z, hyp, s2 = _problems(rng, B, N, d)
    al, nll, info = fit_batch_pairs("A", X, z, hyp, s2)
    assert np.count_nonzero(info) == 0 and np.all(np.isfinite(nll))
    _check(oracle, "A", X, z, hyp, s2, al, nll, rows=(0, 1, 1023, 1024, 1499))


@pytest.mark.parametrize("d,N", [(2, 20), (3, 30), (2, 70)])
def test_bits_do_not_depend_on_the_place_in_the_batch(d, N):
    """the same problem first in a batch of 4 and last in a batch of 6, on the one-launch path (n = 80, 180) and the mid path (280)"""
    from sympgpr_amd.fit import fit_batch_pairs
    rng = np.random.default_rng(23 + N)
    X, z, hyp, s2 = _problems(rng, 10, N, d)
    first = [0, 1, 2, 3]
    last = [4, 5, 6, 7, 8, 0]
    a1, n1, i1 = fit_batch_pairs("A", X[first], z[first], hyp[first], s2[first])
    a2, n2, i2 = fit_batch_pairs("A", X[last], z[last], hyp[last], s2[last])
    assert i1[0] == 0 and i2[-1] == 0
    assert a1[0].tobytes() == a2[-1].tobytes() and n1[0].tobytes() == n2[-1].tobytes()


def test_edges():
    """an empty batch; an order above the batched maximum is refused by fit_batch_pairs and looped over one resident handle by
    nll_chol_pairs_batch; a NaN target stays in its problem (both paths)"""
    import sympgpr_amd
    from sympgpr_amd import _lib as L, func
    from sympgpr_amd.fit import SympFit, fit_batch_pairs
    al, nll, info = fit_batch_pairs("A", np.zeros((0, 5, 4)), np.zeros((0, 20)), np.zeros((0, 5)), 1e-2)
    assert al.shape == (0, 20) and nll.shape == (0,) and info.shape == (0,)
    rng = np.random.default_rng(24)
    X, z, hyp, s2 = _problems(rng, 2, 513, 2)
    with pytest.raises(sympgpr_amd.SympGPRError) as e:
        fit_batch_pairs("A", X[0], z[0], hyp, s2)
    assert e.value.code == L.E_ARG
    func.set_family("A")
    got = func.nll_chol_pairs_batch(np.column_stack((hyp, s2)), X[0], z[0])
    for b in range(2):
        with SympFit.pairs("A", X[0], z[0], hyp[b], s2[b]) as f:
            assert got[b] == f.run().nll()
    for d, N in ((2, 12), (2, 70)):
        X, z, hyp, s2 = _problems(rng, 4, N, d)
        a0, n0, _ = fit_batch_pairs("A", X, z, hyp, s2)
        z[2, 3] = np.nan
        a1, n1, i1 = fit_batch_pairs("A", X, z, hyp, s2)
        assert np.all(i1 == 0) and np.isnan(n1[2])
        keep = [0, 1, 3]
        assert a1[keep].tobytes() == a0[keep].tobytes() and n1[keep].tobytes() == n0[keep].tobytes()
