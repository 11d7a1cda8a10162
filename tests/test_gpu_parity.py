"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI
(ctypes -> libsympgpr_hip.so), against the CPU oracle, the golden vectors generated from the
reference's own Fortran + SciPy, and size-independent properties at BASELINE sizes."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAMS = "ABCD"
HYP = {"A": [0.5, 2.0, 0.4], "B": [0.5, 2.0, 0.4], "C": [0.5, 2.0, 0.4], "D": [0.5, 2.0, 0.7, 0.4]}
# Gram tolerance: the HIP kernels evaluate the same formulas with one exp + one sincos per
# pair and reciprocal constants; entries agree with the Fortran to a few ulp of the largest
# entry.  4e-15 * max|K| absolute (the reference's own Python==Fortran check uses 1e-12).
GRAM_RTOL = 4e-15


def gram_close(K, Kref):
    """|dK| <= 4e-15 max|K| + 3e-13 |K| elementwise: entries deep in the exp tail (argument
    ~ -80) carry |arg| * ulp relative differences between x * (1/l^2) and x / l^2."""
    return bool(np.all(np.abs(K - Kref) <= GRAM_RTOL * np.abs(Kref).max() + 3e-13 * np.abs(Kref)))


@pytest.fixture(scope="module")
def ops():
    import sympgpr_amd
    from sympgpr_amd import ops
    if sympgpr_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need the MI355X")
    return ops


@pytest.fixture(scope="module")
def gram(golden_dir):
    return np.load(os.path.join(golden_dir, "gram.npz"))


@pytest.fixture(scope="module")
def fits(golden_dir):
    return np.load(os.path.join(golden_dir, "fits.npz"))


@pytest.fixture(scope="module")
def ka(golden_dir):
    return json.load(open(os.path.join(golden_dir, "known_answer.json")))


def test_known_answer_build_K(ops, ka):
    """The reference's own test inputs (05_tokamak/SympGPR/test_sympgpr.py:7-10,19-45), its
    tolerance (rtol = atol = 1e-12)."""
    x, y, x0, y0, hyp = (np.array(ka[k]) for k in ("x", "y", "x0", "y0", "hyp"))
    K = np.empty((6, 4), order="F")
    ops.build_k(x, y, x0, y0, hyp, K, family="A")
    np.testing.assert_allclose(K, np.array(ka["build_K_6x4"]), rtol=1e-12, atol=1e-12)
    G = np.empty((3, 2), order="F")
    ops.buildkreg(x, y, x0, y0, hyp, G, family="A")
    np.testing.assert_allclose(G, np.array(ka["buildKreg_3x2"]), rtol=1e-12, atol=1e-12)
    G1 = np.zeros((1, 2), order="F")
    ops.buildkreg(x[:1], y[:1], x0, y0, hyp, G1, family="A")
    np.testing.assert_allclose(G1, np.array(ka["buildKreg_1x2"]), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("tag", ["sq8", "sq64", "rect5x7", "row1x9", "col9x1"])
def test_gram_golden(ops, gram, fam, tag):
    g = lambda k: gram[f"{fam}_{tag}_{k}"]
    n, n0 = len(g("x")), len(g("x0"))
    K = np.full((2 * n, 2 * n0), np.nan, order="F")
    ops.build_k(g("x"), g("y"), g("x0"), g("y0"), g("hyp"), K, family=fam)
    assert gram_close(K, g("K"))
    G = np.full((n, n0), np.nan, order="F")
    ops.buildkreg(g("x"), g("y"), g("x0"), g("y0"), g("hyp"), G, family=fam)
    assert gram_close(G, g("Kreg"))


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("shape", [(1, 1), (3, 1200), (513, 33), (1025, 700), (1024, 1024)])
def test_gram_vs_oracle(ops, oracle, fam, shape):
    """ragged / odd / multi-tile shapes (vector and scalar store paths) against the oracle."""
    n, n0 = shape
    rng = np.random.default_rng(n * 7919 + n0)
    x, y = rng.uniform(0, 2 * np.pi, n), rng.uniform(-3, 3, n)
    x0, y0 = rng.uniform(0, 2 * np.pi, n0), rng.uniform(-3, 3, n0)
    hyp = np.array(HYP[fam]); hyp[0] = 0.21; hyp[1] = 0.43
    K = np.full((2 * n, 2 * n0), np.nan, order="F")
    ops.build_k(x, y, x0, y0, hyp, K, family=fam)
    Ko = oracle.build_K(fam, x, y, x0, y0, hyp, threads=8)
    assert gram_close(K, Ko)
    G = np.full((n, n0), np.nan, order="F")
    ops.buildkreg(x, y, x0, y0, hyp, G, family=fam)
    Go = oracle.buildKreg(fam, x, y, x0, y0, hyp, threads=8)
    assert gram_close(G, Go)


def test_gram_nan_and_large_args(ops, oracle):
    """NaN marks a lost orbit and must propagate (functions/func.py:231-232); huge
    coordinates take the wide range-reduction path."""
    x = np.array([1.0, np.nan, 3.0e12, -2.5e7]); y = np.array([0.0, 1.0, np.nan, 2.0])
    x0 = np.array([0.5, 1.0e11]); y0 = np.array([0.1, -0.3])
    hyp = [0.8, 1.1, 1.0]
    K = np.empty((8, 4), order="F")
    ops.build_k(x, y, x0, y0, hyp, K, family="A")
    Ko = oracle.build_K("A", x, y, x0, y0, hyp)
    assert np.array_equal(np.isnan(K), np.isnan(Ko))
    m = ~np.isnan(Ko)
    assert np.abs(K[m] - Ko[m]).max() <= 1e-9  # sin of a 1e12 argument: ulp(1e12) = 1e-4 rad matters equally in both


def test_kernel_eval(ops, oracle):
    rng = np.random.default_rng(3)
    a = rng.uniform(-3, 3, (4, 50))
    for fam in FAMS:
        l = HYP[fam][:-1]
        p = l[2] if fam == "D" else 0.0
        for which in range(4):
            got = ops.kernel_eval(which, a[0], a[1], a[2], a[3], l, family=fam)
            ref = np.array([oracle.scalar(fam, which, *a[:, i], l[0], l[1], p) for i in range(50)])
            assert np.abs(got - ref).max() <= 1e-14 * max(1.0, np.abs(ref).max())
    assert isinstance(ops.kernel_eval(0, 1.0, 0.0, 2.0, 3.0, [0.5, 2.0], family="A"), float)


def test_f2py_inout_semantics(ops):
    K = np.empty((6, 4))  # C-ordered: f2py refuses intent(inout) (SURVEY 8b error conventions)
    with pytest.raises(ValueError):
        ops.build_k([1, 2, 3.0], [0, 3, 2.0], [1, 2.0], [0, 3.0], [0.5, 2.0, 0.4], K)


# ---------------------------------------------------------------- dense kernels
def _torch():
    import torch
    return torch


def _dev(a):
    t = _torch()
    return t.from_numpy(np.asfortranarray(a).T.copy()).cuda()  # column-major image as a C-ordered (cols, rows) tensor


@pytest.mark.parametrize("shape", [(256, 128, 64), (300, 200, 37), (128, 128, 128), (1000, 1000, 500),
                                   (64, 17, 3), (2048, 2048, 256),
                                   # squares whose tile counts are not multiples of the super-tile:
                                   # the triangular enumeration with a partial last column group
                                   (1536, 1536, 48), (2560, 2560, 32), (5000, 5000, 16), (6656, 6656, 16)])
@pytest.mark.parametrize("lower", [0, 1])
def test_gemm_nt(shape, lower):
    """C = beta C + alpha A B^T with asymmetric random operands (catches a transposed
    accumulator map), ragged edges, and the SYRK-style lower mode."""
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    t = _torch()
    m, n, k = shape
    rng = np.random.default_rng(m + 3 * n + 7 * k)
    A = rng.standard_normal((m, k)); B = rng.standard_normal((n, k)); Cm = rng.standard_normal((m, n))
    dA, dB, dC = _dev(A), _dev(B), _dev(Cm)
    alpha, beta = -0.75, 1.25
    L.check(lib.sgpr_gemm_nt_dev(m, n, k, alpha, dA.data_ptr(), m, dB.data_ptr(), n, beta, dC.data_ptr(), m,
                                 lower, 0, None))
    t.cuda.synchronize()
    got = dC.cpu().numpy().T
    ref = beta * Cm + alpha * A @ B.T
    err = np.abs(got - ref)
    if lower:
        i, j = np.indices((m, n))
        # everything on/below the diagonal must be updated; tiles wholly above stay untouched
        assert err[i >= j].max() <= 1e-12 * k
        untouched = np.abs(got - Cm) == 0
        assert untouched[(i // 256 * 256 + 255 < j // 128 * 128)].all()
    else:
        assert err.max() <= 1e-12 * k


@pytest.mark.parametrize("n", [1, 2, 40, 127, 128, 129, 300, 513, 1000, 2304])
def test_potrf_potrs_host(ops, oracle, n):
    rng = np.random.default_rng(n)
    M = rng.standard_normal((n, n))
    A = M @ M.T / n + np.eye(n) * 0.5
    Lh = ops.cholesky(A)
    assert Lh.flags.f_contiguous and np.all(np.triu(Lh, 1) == 0.0)
    import scipy.linalg
    Ls = scipy.linalg.cholesky(A, lower=True)
    assert np.abs(Lh - Ls).max() <= 1e-13 * np.abs(Ls).max() * max(1, n / 100)
    if n <= 300:
        Lo = oracle.cholesky(A)
        assert np.abs(Lh - Lo).max() <= 1e-13 * np.abs(Lo).max()
    b = rng.standard_normal(n)
    xh = ops.solve_cholesky(Lh, b)
    xo = oracle.solve_cholesky(Ls, b)
    assert np.linalg.norm(xh - xo) <= 1e-12 * np.linalg.norm(xo)
    B = rng.standard_normal((n, 3))
    Xh = ops.solve_cholesky(Lh, B)
    assert np.linalg.norm(A @ Xh - B) <= 1e-11 * np.linalg.norm(B)


def test_not_positive_definite(ops):
    A = np.eye(300)
    A[200, 200] = -1.0
    with pytest.raises(np.linalg.LinAlgError) as e:
        ops.cholesky(A)
    assert "201" in str(e.value)  # LAPACK-style 1-based index of the failing minor
    with pytest.raises(np.linalg.LinAlgError):
        ops.cholesky(np.array([[1.0, 2.0], [2.0, 1.0]]))


# ---------------------------------------------------------------- the fit (alpha, nll)
@pytest.mark.parametrize("tag", ["A_N32", "A_N128", "A_N512", "C_N32", "C_N128", "C_N512", "A_driver20"])
@pytest.mark.parametrize("lower_only", [True, False])
def test_fit_golden(fits, tag, lower_only):
    """posterior weights within 1e-10 relative of the reference CPU solve (north_star) at
    bounded condition number; conditioning-aware budget for the driver-like case."""
    from sympgpr_amd.fit import SympFit
    g = lambda k: fits[f"{tag}_{k}"]
    with SympFit(tag[0], g("q"), g("P"), g("z"), g("hyp"), float(g("sig2n")), lower_only=lower_only) as f:
        f.run()
        alpha, nll, ld = f.alpha(), f.nll(), f.ldiag()
    cond = float(g("cond"))
    tol = max(1e-10, 50 * cond * 2.2e-16)
    assert np.linalg.norm(alpha - g("alpha")) / np.linalg.norm(g("alpha")) < tol
    assert np.linalg.norm(alpha - g("alpha_hp")) / np.linalg.norm(g("alpha_hp")) < tol
    assert nll == pytest.approx(float(g("nll")), rel=max(1e-11, tol))
    np.testing.assert_allclose(ld, g("Ldiag"), rtol=max(1e-11, tol))


def test_known_answer_fit(ka):
    from sympgpr_amd.fit import SympFit
    f6 = ka["fit6"]
    with SympFit("A", ka["x"], ka["y"], f6["z"], ka["hyp"], f6["sig2n"]) as f:
        f.run()
        np.testing.assert_allclose(f.alpha(), f6["alpha"], rtol=1e-12)
        assert f.nll() == pytest.approx(f6["nll"], rel=1e-13)
        # rows of K* . alpha (calcq / target of calcP with alpha cached, sympgpr.f90:75-86,112-124)
        op, oq = f.predict_rows(ka["x"], ka["y"])
        Kalpha = np.concatenate([op, oq])
        z = np.array(f6["z"])
        np.testing.assert_allclose(Kalpha + f6["sig2n"] * f.alpha(), z, atol=1e-12)


@pytest.mark.parametrize("fam,N", [("A", 700), ("C", 1025), ("D", 384), ("B", 300)])
def test_fit_vs_oracle(oracle, fam, N):
    from sympgpr_amd.fit import SympFit
    rng = np.random.default_rng(1234 + N)
    q, P, z = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N), rng.standard_normal(2 * N)
    l = 2.0 * np.sqrt(12 * np.pi / N)
    hyp = [l, l, 0.5, 1.0] if fam == "D" else [l, l, 1.0]
    s2 = 1e-2 / l**2
    a_o, nll_o, L_o = oracle.fit(fam, q, P, z, hyp, s2, threads=8)
    with SympFit(fam, q, P, z, hyp, s2) as f:
        f.run()
        a, nll = f.alpha(), f.nll()
        Lh = f.matrix()
    assert np.linalg.norm(a - a_o) / np.linalg.norm(a_o) < 1e-10
    assert nll == pytest.approx(nll_o, rel=1e-11)
    assert np.all(np.triu(Lh, 1) == 0.0)
    assert np.abs(Lh - L_o).max() <= 1e-11 * np.abs(L_o).max()


@pytest.mark.parametrize("fam,d,N", [("A", 1, 700), ("C", 1, 500), ("A", 2, 160), ("C", 3, 90)])
def test_cond_estimate_vs_eigenvalues(oracle, fam, d, N):
    """sgpr_fit_cond_estimate (power iteration through the prediction kernel + inverse iteration with the factor) against the
    eigenvalues of the oracle's Ky: both quotients are one-sided bounds, so the estimate must not exceed the true condition
    number, and with 80 steps it is within a few per cent of it at these sizes."""
    from sympgpr_amd.fit import SympFit
    rng = np.random.default_rng(99 + N)
    if d == 1:
        q, P, z = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N), rng.standard_normal(2 * N)
        l = 2.0 * np.sqrt(12 * np.pi / N)
        hyp, s2 = [l, l, 1.0], 1e-2 / l**2
        K = oracle.build_K(fam, q, P, q, P, hyp, threads=4)
        fit = SympFit(fam, q, P, z, hyp, s2)
    else:
        X = np.column_stack([rng.uniform(0, 2 * np.pi, (N, d)), rng.uniform(-3, 3, (N, d))])
        z = rng.standard_normal(2 * d * N)
        l = 2.0 * np.sqrt(12 * np.pi) * N ** (-1.0 / (2 * d))
        hyp, s2 = np.append(np.full(2 * d, l), 1.0), 1e-2 / l**2
        K = oracle.build_K_nd(fam, X, X, hyp)
        fit = SympFit.pairs(fam, X, z, hyp, s2)
    w = np.linalg.eigvalsh(K + s2 * np.eye(K.shape[0]))
    with fit as f:
        f.run()
        c = f.cond_estimate(80)
    assert c["lambda_max"] <= w[-1] * (1 + 1e-10) and c["lambda_max"] >= 0.98 * w[-1], (c, w[-1])
    assert c["lambda_min"] >= w[0] * (1 - 1e-8) and c["lambda_min"] <= 1.3 * w[0], (c, w[0])
    assert c["cond"] <= (w[-1] / w[0]) * (1 + 1e-8)


def test_fit_refit_and_errors():
    """the optimiser loop re-runs the path with new hyper-parameters on a resident handle
    (01_pendulum/implicit/main.py:146-151); a non-PD Ky raises LinAlgError like SciPy."""
    from sympgpr_amd.fit import SympFit
    from sympgpr_amd import SympGPRError
    rng = np.random.default_rng(5)
    N = 200
    q, P, z = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N), rng.standard_normal(2 * N)
    with SympFit("A", q, P, z, [0.5, 0.5, 1.0], 1e-2) as f:
        n1 = f.run().nll()
        f.set_hyp([0.7, 0.4, 2.0], 3e-2)
        with pytest.raises(SympGPRError):
            f.alpha()  # stale until re-run
        n2 = f.run().nll()
        assert n1 != n2
        f.set_hyp([0.5, 0.5, 1.0], 1e-2)
        assert f.run().nll() == pytest.approx(n1, rel=1e-12)
        f.set_hyp([3.0, 3.0, 1.0], -0.0)  # numerically singular at sig2n = 0
        with pytest.raises(np.linalg.LinAlgError):
            f.run()


@pytest.mark.parametrize("N", [8192])
def test_fit_property_config2(N):
    """BASELINE config `04_standard_map: N=8192` (n = 16384) -- too big for the scalar oracle in
    test time, so parity is checked through size-independent properties:
      (1) Ky alpha == z, with K alpha recomputed by the independent K*-row kernel;
      (2) nll == 0.5 z.alpha + sum log diag L recomputed on the host from alpha and diag L;
      (3) agreement with SciPy's LAPACK dpotrf/dtrtrs (the calls of func.py:193-194) on the
          same Ky downloaded from the device."""
    from sympgpr_amd.fit import SympFit
    import scipy.linalg
    rng = np.random.default_rng(1234)
    q, P, z = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N), rng.standard_normal(2 * N)
    l = 2.0 * np.sqrt(12 * np.pi / N)
    hyp, s2 = [l, l, 1.0], 1e-2 / l**2
    with SympFit("A", q, P, z, hyp, s2) as f:
        f.build()
        Ky = f.matrix()
        f.factor()
        f.solve()
        a, nll, ld = f.alpha(), f.nll(), f.ldiag()
        op, oq = f.predict_rows(q, P)
    assert np.abs(Ky - Ky.T).max() == 0.0
    r = np.concatenate([op, oq]) + s2 * a - z
    assert np.linalg.norm(r) / np.linalg.norm(z) < 1e-11
    assert nll == pytest.approx(0.5 * z @ a + np.sum(np.log(ld)), rel=1e-12)
    Ls = scipy.linalg.cholesky(Ky, lower=True, check_finite=False, overwrite_a=True)
    a_s = scipy.linalg.solve_triangular(Ls.T, scipy.linalg.solve_triangular(Ls, z, lower=True, check_finite=False),
                                        lower=False, check_finite=False)
    assert np.linalg.norm(a - a_s) / np.linalg.norm(a_s) < 1e-10
    np.testing.assert_allclose(ld, Ls.diagonal(), rtol=1e-11)


# ---------------------------------------------------------------- block-cyclic driver on the GPU
def _dist_worker(rank, world, port, backend, N, nb, out):
    import os, sys
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    kw = {"device_id": torch.device("cuda", 0)} if backend == "nccl" else {}
    dist.init_process_group(backend, rank=rank, world_size=world, **kw)
    try:
        from sympgpr_amd.dist import DistFit, HipOps
        rng = np.random.default_rng(1234)
        q, P, z = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N), rng.standard_normal(2 * N)
        l = 2.0 * np.sqrt(12 * np.pi / N)
        f = DistFit(HipOps(torch.device("cuda", 0)), "A", q, P, z, [l, l, 1.0], 1e-2 / l**2, nb=nb)
        a = f.run().cpu().numpy().copy()
        Bm = np.random.default_rng(77).standard_normal((2 * N, 9))
        Bm[:, 0] = z
        Xs = f.solve_rhs(Bm).cpu().numpy().copy()            # a block of right-hand sides against the distributed factor
        out[rank] = (a, f.nll, Xs)
    finally:
        dist.destroy_process_group()


_DIST_ORACLE = {}


@pytest.mark.parametrize("world,backend,N,nb", [(1, "nccl", 2048, 256), (2, "gloo", 1024, 128),
                                                (4, "gloo", 2048, 256)])
def test_block_cyclic_hip_ops(oracle, world, backend, N, nb):
    """The distributed driver with the HIP block backend.  One GPU is all this box has: world 1
    runs over RCCL; worlds 2 and 4 put several ranks on the one card and exchange the panels
    through gloo (host-staged), which exercises the same driver + kernels + index arithmetic
    the 8-GPU run uses."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_dist_worker, args=(world, port, backend, N, nb, out), nprocs=world, join=True)
    rng = np.random.default_rng(1234)
    q, P, z = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N), rng.standard_normal(2 * N)
    l = 2.0 * np.sqrt(12 * np.pi / N)
    from sympgpr_amd.fit import SympFit
    Bm = np.random.default_rng(77).standard_normal((2 * N, 9))
    Bm[:, 0] = z
    with SympFit("A", q, P, z, [l, l, 1.0], 1e-2 / l**2) as f:
        a_ref, nll_ref = f.run().alpha(), f.nll()
        X_ref = f.solve_rhs(Bm)
    if N not in _DIST_ORACLE:          # (two of the cases share N)
        _DIST_ORACLE[N] = oracle.fit("A", q, P, z, [l, l, 1.0], 1e-2 / l**2, threads=8)[:2]
    a_o, nll_o = _DIST_ORACLE[N]
    for r in range(world):
        a, nll, Xs = out[r]
        assert np.linalg.norm(a - a_ref) / np.linalg.norm(a_ref) < 1e-10
        assert nll == pytest.approx(nll_ref, rel=1e-11)
        assert np.linalg.norm(a - a_o) / np.linalg.norm(a_o) < 1e-10       # and against the CPU oracle: not HIP against HIP alone
        assert nll == pytest.approx(nll_o, rel=1e-11)
        assert np.linalg.norm(Xs - X_ref) <= 1e-10 * np.linalg.norm(X_ref)
        assert np.linalg.norm(Xs[:, 0] - a) <= 1e-12 * np.linalg.norm(a)


# ---------------------------------------------------------------- the func.py mirror
def test_mirror_reference_equivalence_checks(ka):
    """The reference's own test (05_tokamak/SympGPR/test_sympgpr.py:19-75) asserts
    func.py == Fortran to 1e-12 for buildKreg, build_K, guessP, calcQ, calcP on fixed inputs;
    the mirror is held to the values the reference's Fortran returns for them."""
    from sympgpr_amd import func
    from sympgpr_amd.fortran.sympgpr import sympgpr
    func.set_family("A")
    x, y, x0, y0 = (np.array(ka[k]) for k in ("x", "y", "x0", "y0"))
    hyp, hypp = np.array(ka["hyp"]), np.array(ka["hypp"])
    N, N0 = 3, 2
    K = np.empty([N, N0], order="F")
    func.buildKreg(np.hstack((x, y)), np.hstack((x0, y0)), hyp, K)
    Kf = np.empty([N, N0], order="F")
    sympgpr.buildkreg(x, y, x0, y0, hyp, Kf)
    assert np.allclose(K, Kf, rtol=1e-12, atol=1e-12)
    assert np.allclose(K, np.array(ka["buildKreg_3x2"]), rtol=1e-12, atol=1e-12)
    K = np.empty([2 * N, 2 * N0], order="F")
    func.build_K(np.hstack((x, y)), np.hstack((x0, y0)), hyp, K)
    assert np.allclose(K, np.array(ka["build_K_6x4"]), rtol=1e-12, atol=1e-12)
    Kyinvp = np.array(ka["Kyinvp"], order="F"); ztrainp = np.array(ka["ztrainp"])
    Kyinv = np.array(ka["Kyinv"], order="F"); ztrain = np.array(ka["ztrain"])
    pg = func.guessP(x[0], y[0], hypp, np.hstack((x0, y0)), ztrainp, Kyinvp)
    assert np.allclose(pg, ka["guessP"], rtol=1e-12, atol=1e-12)
    assert np.allclose(sympgpr.guessp(x[0], y[0], hypp, x0, y0, ztrainp, Kyinvp), ka["guessP"], rtol=1e-12, atol=1e-12)
    qq = func.calcQ(x[0], y[0], np.hstack((x0, y0)), hyp, Kyinv, ztrain)
    assert np.allclose(qq, ka["calcQ"], rtol=1e-12, atol=1e-12)
    pp = func.calcP(x[0], y[0], hyp, hypp, np.hstack((x0, y0)), ztrainp, Kyinvp, np.hstack((x0, y0)), ztrain, Kyinv)
    # hybrd1 stops at tol 1e-13 (sympgpr.f90:107); the secant root agrees far inside 1e-10
    assert np.allclose(pp, ka["calcP"], rtol=1e-10, atol=1e-10)
    # scalar kernel wrappers
    assert func.f_kern(x0[0], y0[0], x[1], y[1], hyp[:2]) * hyp[2] == pytest.approx(ka["buildKreg_3x2"][1][0], rel=1e-13)
    assert func.d2kdydx0(1.0, 0.0, 2.0, 3.0, hyp[:2]) == func.d2kdxdy0(1.0, 0.0, 2.0, 3.0, hyp[:2])


def test_mirror_gpsolve_nll(fits, oracle):
    from sympgpr_amd import func
    func.set_family("A")
    g = lambda k: fits[f"A_N128_{k}"]
    N = 256
    x = np.hstack((g("q"), g("P")))
    hyp4 = np.append(g("hyp"), -float(g("sig2n")))  # nll_chol takes abs(hyp[-1]) (func.py:192)
    assert func.nll_chol(hyp4, x, g("z"), N) == pytest.approx(float(g("nll")), rel=1e-11)
    K = np.empty((N, N), order="F")
    func.build_K(x, x, g("hyp"), K)
    Ky = K + float(g("sig2n")) * np.eye(N)
    Lf, alpha = func.gpsolve(Ky, g("z"))
    assert np.linalg.norm(alpha - g("alpha")) / np.linalg.norm(g("alpha")) < 1e-10
    assert np.all(np.triu(Lf, 1) == 0)
    np.testing.assert_allclose(func.solve_cholesky(Lf, g("z")), alpha, rtol=0, atol=0)
    # the regular GP tuned with the symplectic nll on an N x N matrix whose
    # build_K slices N/2 "points" out of a longer x
    assert func.nll_chol(hyp4, x, g("z")[:128], 128) == pytest.approx(
        oracle.fit("A", x[:64], x[64:128], g("z")[:128], g("hyp"), float(g("sig2n")))[1], rel=1e-11)
    # scalar-kernel GP
    Kr = oracle.buildKreg("A", g("q"), g("P"), g("q"), g("P"), g("hyp")) + float(g("sig2n")) * np.eye(128)
    Lr = oracle.cholesky(Kr)
    ar = oracle.solve_cholesky(Lr, g("z")[:128])
    assert func.nll_chol_reg(hyp4, x, g("z")[:128], 128) == pytest.approx(oracle.nll(Lr, g("z")[:128], ar), rel=1e-11)


def test_mirror_applymap_vs_pointwise_reference(oracle):
    """applymap (functions/func.py:216-237) against the reference recurrences written out with
    the oracle's K*-rows and MINPACK hybrd (scipy.optimize.fsolve, the solver behind hybrd1)."""
    import scipy.optimize
    from sympgpr_amd import func
    func.set_family("A")
    rng = np.random.default_rng(11)
    Nt = 40
    q, P = rng.uniform(0, 2 * np.pi, Nt), rng.uniform(-1, 1, Nt)
    # a gentle symplectic map as training data: Q = q + 0.3 P', P' = p - 0.3 sin q
    pn = P; p_old = pn + 0.3 * np.sin(q); Q = q + 0.3 * pn
    xtrain = np.hstack((q, pn)); ztrain = np.hstack((p_old - pn, Q - q))
    xtrainp = np.hstack((q, p_old)); ztrainp = pn
    hyp = np.array([1.2, 1.5, 1.0]); hypp = np.array([1.2, 1.5, 1.0])
    K = oracle.build_K("A", q, pn, q, pn, hyp) + 1e-8 * np.eye(2 * Nt)
    Kp = oracle.buildKreg("A", q, p_old, q, p_old, hypp) + 1e-8 * np.eye(Nt)
    Kyinv, Kyinvp = np.linalg.inv(K), np.linalg.inv(Kp)
    Ntest, nm = 5, 6
    Q0, P0 = rng.uniform(0.5, 5.5, Ntest), rng.uniform(-0.5, 0.5, Ntest)
    qmap, pmap = func.applymap(nm, Ntest, hyp, hypp, Q0, P0, xtrainp, ztrainp, Kyinvp, xtrain, ztrain, Kyinv)
    alpha, alphap = Kyinv @ ztrain, Kyinvp @ ztrainp
    qr, pr = np.zeros((nm, Ntest)), np.zeros((nm, Ntest))
    qr[0], pr[0] = Q0, P0
    for i in range(nm - 1):
        for k in range(Ntest):
            g0 = oracle.predict_reg("A", [qr[i, k]], [pr[i, k]], q, p_old, hypp, alphap)[0]
            f = lambda Pn: oracle.predict_rows("A", [qr[i, k]], [Pn[0]], q, pn, hyp, alpha)[0][0] - pr[i, k] + Pn[0]
            pr[i + 1, k] = scipy.optimize.fsolve(f, [g0], xtol=1e-13)[0]
            dq = oracle.predict_rows("A", [qr[i, k]], [pr[i + 1, k]], q, pn, hyp, alpha)[1][0]
            qr[i + 1, k] = np.mod(dq + qr[i, k], 2 * np.pi)
    np.testing.assert_allclose(pmap, pr, rtol=1e-8, atol=1e-8)   # the reference's applymap tolerance (test_sympgpr.py:92-93)
    np.testing.assert_allclose(qmap, qr, rtol=1e-8, atol=1e-8)
    # NaN start = lost orbit stays lost, the others are unaffected (functions/func.py:231-232)
    P0n = P0.copy(); P0n[2] = np.nan
    q2, p2 = func.applymap(3, Ntest, hyp, hypp, Q0, P0n, xtrainp, ztrainp, Kyinvp, xtrain, ztrain, Kyinv)
    assert np.all(np.isnan(p2[1:, 2])) and np.all(np.isnan(q2[1:, 2]))
    np.testing.assert_allclose(np.delete(p2, 2, axis=1), np.delete(pmap[:3], 2, axis=1), rtol=1e-12)


def test_applymap_orbit_shared_by_several_workgroups(oracle):
    """Large training sets: the residuals of one orbit are summed by a TEAM of workgroups (3 here: 20 orbits on 1500 points) that
    exchange their parts through memory and all take the same branches.  Against the recurrences of functions/func.py:204-237
    written out on the host with the oracle's K*-rows and MINPACK hybrd, from posterior weights fitted on the device."""
    import scipy.optimize
    from sympgpr_amd import _lib as L, maps
    from sympgpr_amd.fit import SympFit
    rng = np.random.default_rng(21)
    Nt, Ntest, nm = 1500, 20, 4
    assert L.load_probe_library().sgpr_probe_map_team(Ntest, Nt) == 6      # ceil(1500 / 256) members per orbit
    q, pn = rng.uniform(0, 2 * np.pi, Nt), rng.uniform(-1, 1, Nt)
    p_old = pn + 0.3 * np.sin(q); Q = q + 0.3 * pn               # a gentle symplectic map as training data
    ztrain = np.hstack((p_old - pn, Q - q))
    hyp, hypp, s2 = np.array([0.9, 1.1, 1.0]), np.array([0.9, 1.1, 1.0]), 1e-6
    with SympFit("A", q, pn, ztrain, hyp, s2) as f:
        alpha = f.run().alpha()
    with SympFit("A", q, p_old, pn, hypp, s2, reg=True) as f:
        alphap = f.run().alpha()
    Q0, P0 = rng.uniform(0.5, 5.5, Ntest), rng.uniform(-0.5, 0.5, Ntest)
    P0[7] = np.nan                                                 # a lost orbit in the middle of the teams
    qmap, pmap = maps.run_map_alpha(maps.WRAP_Q, nm, Ntest, hyp, Q0, P0, q, pn, alpha, hypp, q, p_old, alphap, family="A")
    qr, pr = np.zeros((nm, Ntest)), np.zeros((nm, Ntest))
    qr[0], pr[0] = Q0, P0
    for i in range(nm - 1):
        for k in range(Ntest):
            if np.isnan(pr[i, k]):
                qr[i + 1, k] = pr[i + 1, k] = np.nan
                continue
            g0 = oracle.predict_reg("A", [qr[i, k]], [pr[i, k]], q, p_old, hypp, alphap)[0]
            fres = lambda Pn: oracle.predict_rows("A", [qr[i, k]], [Pn[0]], q, pn, hyp, alpha)[0][0] - pr[i, k] + Pn[0]
            pr[i + 1, k] = scipy.optimize.fsolve(fres, [g0], xtol=1e-13)[0]
            dq = oracle.predict_rows("A", [qr[i, k]], [pr[i + 1, k]], q, pn, hyp, alpha)[1][0]
            qr[i + 1, k] = np.mod(dq + qr[i, k], 2 * np.pi)
    ok = ~np.isnan(pr)
    assert np.array_equal(np.isnan(pmap), np.isnan(pr)) and np.array_equal(np.isnan(qmap), np.isnan(qr))
    np.testing.assert_allclose(pmap[ok], pr[ok], rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(qmap[ok], qr[ok], rtol=1e-8, atol=1e-8)
    # and run to run the teams reproduce themselves bit for bit (every member adds the parts in member order)
    q2, p2 = maps.run_map_alpha(maps.WRAP_Q, nm, Ntest, hyp, Q0, P0, q, pn, alpha, hypp, q, p_old, alphap, family="A")
    assert np.array_equal(q2[ok], qmap[ok]) and np.array_equal(p2[ok], pmap[ok])


# ---------------------------------------------------------------- hyper-parameter gradients
@pytest.mark.parametrize("fam", ["A", "B", "C", "D"])
def test_build_dK_vs_oracle(oracle, fam):
    from sympgpr_amd import func
    func.set_family(fam)
    try:
        rng = np.random.default_rng(21)
        N, N0 = 37, 29
        xin = np.hstack((rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N)))
        x0in = np.hstack((rng.uniform(0, 2 * np.pi, N0), rng.uniform(-3, 3, N0)))
        hyp = np.array([0.6, 0.9, 0.4, 1.3]) if fam == "D" else np.array([0.6, 0.9, 1.3])
        dK = func.build_dK(xin, x0in, hyp)
        dKr = func.build_dKreg(xin, x0in, hyp)
        assert dK[0].shape == (2 * N0, 2 * N) and dKr[0].shape == (N, N0)
        if fam != "D":
            dKo = oracle.build_dK(fam, xin[:N], xin[N:], x0in[:N0], x0in[N0:], hyp)
            dKro = oracle.build_dKreg(fam, xin[:N], xin[N:], x0in[:N0], x0in[N0:], hyp)
            for a, b in zip(dK + dKr, dKo + dKro):
                assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max()
        else:
            # no generated reference for the driver-less family D gradient: check against central
            # differences of the (parity-checked) build_K in lx and ly
            for i in (0, 1):
                h = 1e-6
                hp, hm = hyp.copy(), hyp.copy()
                hp[i] += h; hm[i] -= h
                Kp = np.empty((2 * N0, 2 * N), order="F"); Km = np.empty((2 * N0, 2 * N), order="F")
                func.build_K(x0in, xin, hp, Kp); func.build_K(x0in, xin, hm, Km)
                fd = (Kp - Km) / (2 * h)
                assert np.abs(dK[i] - fd).max() <= 1e-6 * max(1.0, np.abs(fd).max())
    finally:
        func.set_family("A")


@pytest.mark.parametrize("fam,Np", [("A", 40), ("C", 150), ("A", 700), ("B", 60)])
def test_nll_grad_vs_oracle(oracle, fam, Np):
    """nll_grad / nll_grad_reg (functions/func.py:132-162) through the device path (two panel
    solves + a transpose instead of the explicit inverse) against the restated reference."""
    from sympgpr_amd import func
    func.set_family(fam)
    try:
        rng = np.random.default_rng(1234 + Np)
        x = np.hstack((rng.uniform(0, 2 * np.pi, Np), rng.uniform(-3, 3, Np)))
        y = rng.standard_normal(2 * Np)
        l = 2.0 * np.sqrt(12 * np.pi / Np)
        hyp = np.array([l, 1.3 * l, 0.8, 1e-2 / l**2])
        val, g = func.nll_grad(hyp, x, y, 2 * Np)
        val_o, g_o = oracle.nll_grad(fam, hyp, x, y, 2 * Np)
        assert val == pytest.approx(val_o, rel=1e-11)
        np.testing.assert_allclose(g, g_o, rtol=1e-9)
        valr, gr = func.nll_grad_reg(hyp, x, y[:Np], Np)
        valr_o, gr_o = oracle.nll_grad(fam, hyp, x, y[:Np], Np, reg=True)
        assert valr == pytest.approx(valr_o, rel=1e-11)
        np.testing.assert_allclose(gr, gr_o, rtol=1e-9)
    finally:
        func.set_family("A")


# ---------------------------------------------------------------- inverse, edge cases
@pytest.mark.parametrize("N", [20, 300, 1000])
def test_fit_inverse(oracle, N):
    """Kyinv = scipy.linalg.inv(K + sig2n I) as the drivers form it (01_pendulum/implicit/main.py:161)."""
    from sympgpr_amd.fit import SympFit
    rng = np.random.default_rng(N)
    q, P, z = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N), rng.standard_normal(2 * N)
    l = 2.0 * np.sqrt(12 * np.pi / N)
    hyp, s2 = [l, l, 1.0], 1e-2 / l**2
    Ky = oracle.build_K("A", q, P, q, P, hyp) + s2 * np.eye(2 * N)
    with SympFit("A", q, P, z, hyp, s2) as f:
        f.run()
        Ki = f.inverse()
        a = f.alpha()
    assert np.abs(Ki - Ki.T).max() == 0.0
    assert np.abs(Ki @ Ky - np.eye(2 * N)).max() < 1e-9
    assert np.linalg.norm(Ki @ z - a) / np.linalg.norm(a) < 1e-10


def test_edge_shapes(ops, oracle):
    """empty and one-point inputs (the reference builds a 2 x 2N0 K* row block with N = 1 on every
    prediction, sympgpr.f90:82-84)."""
    from sympgpr_amd.fit import SympFit
    K = np.empty((0, 0), order="F")
    ops.build_k([], [], [], [], [0.5, 2.0, 0.4], K)
    K = np.empty((0, 8), order="F")
    ops.build_k([], [], [1.0, 2, 3, 4], [0.0, 1, 2, 3], [0.5, 2.0, 0.4], K)
    K = np.full((2, 6), np.nan, order="F")
    ops.build_k([1.5], [0.2], [1.0, 2.0, 3.0], [0.0, 3.0, 2.0], [0.5, 2.0, 0.4], K)
    assert gram_close(K, oracle.build_K("A", [1.5], [0.2], [1.0, 2.0, 3.0], [0.0, 3.0, 2.0], [0.5, 2.0, 0.4]))
    with SympFit("A", [1.0], [0.5], [0.3, -0.2], [0.5, 2.0, 0.4], 1e-3) as f:   # one training point: n = 2
        a = f.run().alpha()
    a_o, _, _ = oracle.fit("A", [1.0], [0.5], [0.3, -0.2], [0.5, 2.0, 0.4], 1e-3)
    np.testing.assert_allclose(a, a_o, rtol=1e-13)
    assert ops.cholesky(np.zeros((0, 0))).shape == (0, 0)
    with pytest.raises(ValueError):
        ops.cholesky(np.ones((2, 3)))


def test_fit_matrix_roundtrip(oracle):
    """get_matrix after build returns the full symmetric Ky (also from a lower-only build),
    after factor the SciPy-shaped L."""
    from sympgpr_amd.fit import SympFit
    rng = np.random.default_rng(2)
    N = 150
    q, P = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N)
    hyp, s2 = [0.4, 0.6, 1.2], 5e-2
    Ko = oracle.build_K("A", q, P, q, P, hyp) + s2 * np.eye(2 * N)
    for lower_only in (True, False):
        with SympFit("A", q, P, None, hyp, s2, lower_only=lower_only) as f:
            f.build()
            assert gram_close(f.matrix(), Ko)
            f.factor()
            Lh = f.matrix()
            assert np.all(np.triu(Lh, 1) == 0) and np.abs(Lh @ Lh.T - Ko).max() < 1e-12
            X = f.solve_rhs(np.eye(2 * N)[:, :3])
            assert np.abs(Ko @ X - np.eye(2 * N)[:, :3]).max() < 1e-10


@pytest.mark.parametrize("n,nrhs", [(40, 8), (129, 17), (1000, 64), (2304, 300)])
def test_multi_rhs_solve_on_mfma(ops, n, nrhs):
    """solve_cholesky with many right-hand sides (>= 8) runs as GEMM-shaped panel solves (rows =
    right-hand sides, 'NT' forward and 'NN' backward products) instead of per-vector TRSVs."""
    rng = np.random.default_rng(n + nrhs)
    M = rng.standard_normal((n, n))
    A = M @ M.T / n + np.eye(n) * 0.5
    import scipy.linalg
    Lf = scipy.linalg.cholesky(A, lower=True)
    B = rng.standard_normal((n, nrhs))
    X = ops.solve_cholesky(Lf, B)
    Xr = scipy.linalg.cho_solve((Lf, True), B)
    assert np.linalg.norm(X - Xr) / np.linalg.norm(Xr) < 1e-12
    x1 = ops.solve_cholesky(Lf, B[:, 0])
    assert np.linalg.norm(x1 - Xr[:, 0]) / np.linalg.norm(Xr[:, 0]) < 1e-12


@pytest.mark.parametrize("n,nrhs", [(640, 2), (640, 64), (1024, 3), (1280, 64), (2304, 17), (4096, 65), (8192, 130),
                                    (33 * 128, 64), (16384, 256)])
def test_block_rhs_strip_solve(ops, n, nrhs):
    """2 .. 256 right-hand sides at orders that are multiples of 128 above 512: the one-launch strip solves of trsm.hip (L streamed
    once per 64 columns, segments handed from strip to strip), every strip count from 5 (all strips folded or nearly) to 128,
    column counts that are not multiples of 64, several 64-column passes; against LAPACK, residual and per-column."""
    import scipy.linalg
    rng = np.random.default_rng(n + nrhs)
    # a banded-dominant SPD matrix built without an n^3 host product: L0 well conditioned, A = L0 L0^T
    L0 = np.tril(rng.standard_normal((n, n))) / np.sqrt(n)
    L0[np.diag_indices(n)] = 1.0 + rng.uniform(0, 1, n)
    B = rng.standard_normal((n, nrhs))
    B[:, -1] = 0.0
    B[n // 3, -1] = 1.0                                     # a unit vector among the right-hand sides
    X = ops.solve_cholesky(np.asfortranarray(L0), B)
    Xr = scipy.linalg.solve_triangular(L0.T, scipy.linalg.solve_triangular(L0, B, lower=True, check_finite=False),
                                       lower=False, check_finite=False)
    assert X.shape == Xr.shape
    err = np.linalg.norm(X - Xr, axis=0) / np.linalg.norm(Xr, axis=0)
    assert err.max() < 1e-11, (n, nrhs, err.max(), int(err.argmax()))


@pytest.mark.parametrize("n,nrhs,piece", [(2304, 64, 4), (4096, 65, 8), (8192, 3, 16), (8192, 64, 7)])
def test_block_rhs_strips_streamed_in_pieces(ops, n, nrhs, piece):
    """Strips that stream more than `trsm_piece` tiles (16 up to order 16 384, 128 above) go out as several tickets whose
    partial sums the last one adds up; here with a small cap, so that strips of 2 .. 15 pieces occur at test sizes.  Same
    answer as LAPACK, and bit-identical from call to call (the pieces are added in a fixed order)."""
    import scipy.linalg
    from sympgpr_amd import _lib as L
    probe = L.load_probe_library()
    rng = np.random.default_rng(n + nrhs + piece)
    L0 = np.tril(rng.standard_normal((n, n))) / np.sqrt(n)
    L0[np.diag_indices(n)] = 1.0 + rng.uniform(0, 1, n)
    B = rng.standard_normal((n, nrhs))
    L.check(probe.sgpr_probe_tune(b"trsm_piece", float(piece)))
    try:
        X = ops.solve_cholesky(np.asfortranarray(L0), B)
        X2 = ops.solve_cholesky(np.asfortranarray(L0), B)
    finally:
        L.check(probe.sgpr_probe_tune(b"trsm_piece", 0.0))
    Xr = scipy.linalg.solve_triangular(L0.T, scipy.linalg.solve_triangular(L0, B, lower=True, check_finite=False),
                                       lower=False, check_finite=False)
    err = np.linalg.norm(X - Xr, axis=0) / np.linalg.norm(Xr, axis=0)
    assert err.max() < 1e-11, (n, nrhs, piece, err.max(), int(err.argmax()))
    assert np.array_equal(X, X2)


@pytest.mark.parametrize("bad_pass", [0, 1])
def test_block_rhs_give_up_in_an_earlier_pass_is_reported(ops, bad_pass):
    """130 right-hand sides = three 64-column passes through the strip solves.  A hand-off that gives up in the first or second
    pass (forced: the tunable raises the forward solve's give-up word in front of that pass) must still be on record when the
    status is read after the LAST pass: the call fails, it does not return 0 with NaN columns (round-4 advice: every pass used
    to clear the give-up words)."""
    from sympgpr_amd import _lib as L
    probe = L.load_probe_library()
    n, nrhs = 1280, 130
    rng = np.random.default_rng(7)
    L0 = np.tril(rng.standard_normal((n, n))) / np.sqrt(n)
    L0[np.diag_indices(n)] = 1.0 + rng.uniform(0, 1, n)
    B = rng.standard_normal((n, nrhs))
    L.check(probe.sgpr_probe_tune(b"trsm_force_giveup_pass", float(bad_pass)))
    try:
        with pytest.raises(L.SympGPRError):
            ops.solve_cholesky(np.asfortranarray(L0), B)
    finally:
        L.check(probe.sgpr_probe_tune(b"trsm_force_giveup_pass", -1.0))
    X = ops.solve_cholesky(np.asfortranarray(L0), B)          # and the next call is clean again
    assert np.all(np.isfinite(X))


# ---------------------------------------------------------------- d canonical pairs (BASELINE d = 2, 3)
@pytest.mark.parametrize("fam,d,n,n0", [("A", 1, 37, 21), ("A", 2, 600, 70), ("C", 2, 33, 1025), ("A", 3, 130, 64),
                                        ("C", 3, 1, 5), ("B", 2, 100, 31), ("D", 2, 65, 130), ("D", 3, 20, 20),
                                        ("B", 1, 40, 9), ("D", 1, 40, 9)])
def test_build_k_nd_vs_oracle(ops, oracle, fam, d, n, n0):
    rng = np.random.default_rng(1000 * d + n)
    X = np.column_stack([rng.uniform(0, 2 * np.pi, (n, d)), rng.uniform(-3, 3, (n, d))])
    X0 = np.column_stack([rng.uniform(0, 2 * np.pi, (n0, d)), rng.uniform(-3, 3, (n0, d))])
    hyp = np.append(rng.uniform(0.5, 1.5, 2 * d), 0.8)
    if fam == "D":   # free period per q: (lq.., lP.., p_1..p_d, sig)
        hyp = np.concatenate((hyp[:-1], rng.uniform(0.4, 0.9, d), hyp[-1:]))
    K = ops.build_k_nd(X, X0, hyp, family=fam)
    Ko = oracle.build_K_nd(fam, X, X0, hyp)
    assert gram_close(K, Ko)
    if d == 1:   # one pair: exactly the reference's build_K
        K1 = np.empty((2 * n, 2 * n0), order="F")
        ops.build_k(X[:, 0], X[:, 1], X0[:, 0], X0[:, 1], hyp, K1, family=fam)
        assert gram_close(K, K1)


@pytest.mark.parametrize("fam,d,N", [("A", 2, 300), ("C", 2, 260), ("C", 3, 200), ("A", 1, 150), ("D", 2, 220), ("B", 2, 180)])
def test_fit_pairs_vs_oracle(oracle, fam, d, N):
    from sympgpr_amd.fit import SympFit
    rng = np.random.default_rng(7 * d + N)
    X = np.column_stack([rng.uniform(0, 2 * np.pi, (N, d)), rng.uniform(-3, 3, (N, d))])
    z = rng.standard_normal(2 * d * N)
    l = 1.2 * (12 * np.pi / N) ** (1.0 / (2 * d))
    hyp = np.append(np.full(2 * d, l), 1.0)
    if fam == "D":
        hyp = np.concatenate((hyp[:-1], np.full(d, 0.5), hyp[-1:]))
    s2 = 1e-2 / l**2
    a_o, nll_o, _ = oracle.fit_nd(fam, X, z, hyp, s2)
    with SympFit.pairs(fam, X, z, hyp, s2) as f:
        f.run()
        a, nll = f.alpha(), f.nll()
        pred = f.predict_pairs(X[:17])
    assert np.linalg.norm(a - a_o) / np.linalg.norm(a_o) < 1e-10
    assert nll == pytest.approx(nll_o, rel=1e-11)
    # K alpha at training points = z - sig2n alpha
    Kalpha = (z - s2 * a).reshape(2 * d, N).T[:17]
    np.testing.assert_allclose(pred, Kalpha, atol=1e-9)


def test_fit_duplicate_points(oracle):
    """collisions: repeated training points make K itself singular; with the noise term the fit
    must still agree with the reference path."""
    from sympgpr_amd.fit import SympFit
    rng = np.random.default_rng(8)
    N = 120
    q, P = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N)
    q[10:20] = q[0:10]; P[10:20] = P[0:10]          # ten exact duplicates
    z = rng.standard_normal(2 * N)
    hyp, s2 = [0.7, 0.9, 1.0], 1e-3
    a_o, nll_o, _ = oracle.fit("A", q, P, z, hyp, s2)
    with SympFit("A", q, P, z, hyp, s2) as f:
        a, nll = f.run().alpha(), f.nll()
    cond = 2 * 40.0 / s2  # crude bound: duplicated pairs leave eigenvalues at the noise floor
    assert np.linalg.norm(a - a_o) / np.linalg.norm(a_o) < max(1e-10, 50 * cond * 2.2e-16)
    assert nll == pytest.approx(nll_o, rel=1e-10)


def _oracle_row_residual(oracle, fam, X, idx, hyp, s2, V, B):
    """|Ky V - B| / |B| on the rows of the sampled training points `idx`, with those rows of K
    re-evaluated ON THE HOST by the oracle's build_K / build_K_nd (the restated Fortran formulas) --
    independent of every device formula.  X (N x 2d), V and B (n) or (n x nrhs)."""
    N, D = X.shape
    if D == 2:
        Krows = oracle.build_K(fam, X[idx, 0], X[idx, 1], X[:, 0], X[:, 1], hyp, threads=8)
    else:
        Krows = oracle.build_K_nd(fam, X[idx], X, hyp)
    rows = np.concatenate([a * N + idx for a in range(D)])      # row order of build_K(x = sample, x0 = all)
    R = Krows @ V + s2 * V[rows] - B[rows]
    return float(np.linalg.norm(R) / np.linalg.norm(B[rows]))


def test_fit_full_size_properties(oracle):
    """BASELINE's headline size (N = 65536 points, matrix order n = 131072, 137 GB in place): no CPU
    reference is feasible (7.5e14 flop), so parity is checked through size-independent properties:
    Ky alpha = z on sampled rows with those rows of K recomputed on the host by the oracle, the nll
    recomputed on the host from alpha and diag L, positivity of diag L, info == 0."""
    import torch
    from sympgpr_amd.fit import SympFit
    free, _ = torch.cuda.mem_get_info()
    if free < 150e9:
        pytest.skip("needs ~140 GB of free HBM")
    N = 65536
    rng = np.random.default_rng(1234)
    q, P, z = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N), rng.standard_normal(2 * N)
    l = 2.0 * np.sqrt(12 * np.pi / N)
    hyp, s2 = [l, l, 1.0], 1e-2 / l**2
    with SympFit("A", q, P, z, hyp, s2, lower_only=False) as f:
        f.run()
        a, nll, ld = f.alpha(), f.nll(), f.ldiag()
        idx = rng.choice(N, 1024, replace=False)
        op, oq = f.predict_rows(q[idx], P[idx])
    r = np.concatenate([op + s2 * a[idx] - z[idx], oq + s2 * a[N + idx] - z[N + idx]])
    assert np.linalg.norm(r) / np.linalg.norm(np.concatenate([z[idx], z[N + idx]])) < 1e-10
    assert _oracle_row_residual(oracle, "A", np.column_stack((q, P)), idx[:192], hyp, s2, a, z) < 1e-10
    assert np.all(ld > 0) and np.all(np.isfinite(a))
    assert nll == pytest.approx(0.5 * z @ a + np.sum(np.log(ld)), rel=1e-12)


@pytest.mark.parametrize("fam,d,N,nrhs", [("C", 2, 32768, 0), ("A", 3, 16384, 64)])
def test_fit_pairs_full_size_configs(oracle, fam, d, N, nrhs):
    """BASELINE configs at their stated sizes: `03_henon_heiles` (family C, N = 32768, d = 2 canonical
    pairs: n = 131072 through gram_nd_kernel) and `05_tokamak` (d = 3, N = 16384: n = 98304, with the
    config's multi-right-hand-side solve: 64 columns through the MFMA panel solves).  Same
    size-independent properties as above; every residual uses rows of K recomputed on the host by the
    oracle (build_K_nd), not a device kernel."""
    import torch
    from sympgpr_amd.fit import SympFit
    n = 2 * d * N
    free, _ = torch.cuda.mem_get_info()
    if free < 8.0 * n * n + 8e9:
        pytest.skip("needs %.0f GB of free HBM" % (8.0 * n * n / 1e9 + 8))
    rng = np.random.default_rng(1234)
    X = np.column_stack([rng.uniform(0, 2 * np.pi, (N, d)), rng.uniform(-3, 3, (N, d))])
    z = rng.standard_normal(n)
    l = 2.0 * np.sqrt(12 * np.pi) * N ** (-1.0 / (2 * d))
    hyp = np.append(np.full(2 * d, l), 1.0)
    s2 = 1e-2 / l**2
    idx = rng.choice(N, 96, replace=False)
    with SympFit.pairs(fam, X, z, hyp, s2) as f:
        f.run()
        a, nll, ld = f.alpha(), f.nll(), f.ldiag()
        pred = f.predict_pairs(X[idx])
        if nrhs:
            B = rng.standard_normal((n, nrhs))
            Xs = f.solve_rhs(B)
    assert np.all(ld > 0) and np.all(np.isfinite(a))
    assert nll == pytest.approx(0.5 * z @ a + np.sum(np.log(ld)), rel=1e-12)
    assert _oracle_row_residual(oracle, fam, X, idx, hyp, s2, a, z) < 1e-10
    # the device's own K* rows agree with the same identity (K alpha = z - sig2n alpha)
    Kalpha = (z - s2 * a).reshape(2 * d, N).T[idx]
    assert np.linalg.norm(pred - Kalpha) / np.linalg.norm(Kalpha) < 1e-9
    if nrhs:
        assert np.all(np.isfinite(Xs))
        assert _oracle_row_residual(oracle, fam, X, idx, hyp, s2, Xs, B) < 1e-10


@pytest.mark.parametrize("n,bad", [(1024, 1), (1024, 130), (1024, 257), (1024, 640), (1024, 1024), (2048, 1500), (4096, 3970)])
def test_not_positive_definite_in_the_panel_kernel(ops, n, bad):
    """LAPACK's info out of the persistent panel kernel: the first non-positive pivot sits in the first leaf of a
    panel, in a leaf on the fused chain (solve -> update -> leaf in LDS) and in the last leaf; orders that are
    multiples of 128, so the look-ahead driver and its panel kernel take them (chol.hip)."""
    import scipy.linalg.lapack as lp
    rng = np.random.default_rng(n + bad)
    B = rng.standard_normal((n, 64))
    A = B @ B.T + n * np.eye(n)
    A[bad - 1, bad - 1] = -1.0                 # 1-based minor `bad` is the first that is not positive definite
    _, info_ref = lp.dpotrf(A, lower=1)
    assert info_ref == bad
    with pytest.raises(np.linalg.LinAlgError) as e:
        ops.cholesky(A)
    import re
    assert int(re.search(r"\d+", str(e.value)).group()) == bad


@pytest.mark.gpu
@pytest.mark.parametrize("n_pts,nrhs", [(300, 5), (640, 64), (1024, 70)])
def test_solve_rhs_device_resident(n_pts, nrhs):
    """sgpr_fit_solve_rhs_dev: the right-hand sides stay on the device (a torch tensor here), the solve's scratch stays with the
    fit; same answer as the host-buffer entry, call after call, and column z gives alpha."""
    import torch
    from sympgpr_amd.fit import SympFit
    rng = np.random.default_rng(n_pts + nrhs)
    q, P = rng.uniform(0, 2 * np.pi, n_pts), rng.uniform(-3, 3, n_pts)
    z = rng.standard_normal(2 * n_pts)
    hyp, s2 = np.array([0.7, 0.9, 1.0]), 1e-2
    with SympFit("A", q, P, z, hyp, s2) as f:
        f.run()
        n = f.n
        B = rng.standard_normal((n, nrhs))
        B[:, 0] = z
        Xh = f.solve_rhs(B.copy())
        dev = torch.device("cuda", torch.cuda.current_device())
        B0 = torch.from_numpy(np.ascontiguousarray(B.T)).to(dev)
        for _ in range(2):
            Bd = B0.clone()
            torch.cuda.synchronize()
            f.solve_rhs_dev(Bd.data_ptr(), nrhs)
            Xd = Bd.cpu().numpy().T
            assert np.array_equal(Xd, Xh)
        al = f.alpha()
        assert np.linalg.norm(Xd[:, 0] - al) / np.linalg.norm(al) < 1e-10
        # a wider leading dimension: the block sits inside a larger allocation
        big = torch.zeros((nrhs, n + 24), dtype=torch.float64, device=dev)
        big[:, :n] = B0
        torch.cuda.synchronize()
        f.solve_rhs_dev(big.data_ptr(), nrhs, ldb=n + 24)
        assert np.array_equal(big[:, :n].cpu().numpy().T, Xh) and float(big[:, n:].abs().max()) == 0.0
