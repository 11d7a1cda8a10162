"""The block-cyclic driver with the HIP block backend (DistFit(HipOps)) against the CPU oracle, on one card: every stage of it
-- the Gram blocks each rank builds, the factor blocks, alpha, nll, blocks of right-hand sides, the info of a matrix that is
not positive definite -- on grids where N / nb is NOT a multiple of the grid dimensions, pr != pc, ranks without a diagonal
block or without any rows, block sizes that are no multiple of the 128-row leaf, families A to D, d = 1, 2, 3, serial and
overlapped mode.  The parent computes every reference with the oracle alone (no SympFit: an error the two HIP paths share
would cancel); the gates are the single-GPU ones of tests/test_gpu_parity.py.  All ranks of a case share cuda:0 and exchange
through gloo (world 1: RCCL); at most 8 ranks per case."""
import datetime
import os
import socket
import sys
from collections import namedtuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "world d fam N nb nrhs modes")
Case.__new__.__defaults__ = ((9,), (False,))
BOTH = (False, True)                 # overlapped (the default), then serial=True

# world (grid) | d | family | N | nb | N / nb: what the case crosses
CASES = {
    "2x1-A": Case(2, 1, "A", 640, 128),                     # 5: a selection of points of its own for every part
    "2x1-B": Case(2, 1, "B", 640, 128),                     #    (B: the mixed parts are zeros the kernel has to WRITE)
    "2x1-C": Case(2, 1, "C", 640, 128),
    "2x1-D": Case(2, 1, "D", 640, 128),
    "3x1-A": Case(3, 1, "A", 896, 128),                     # 7: ragged, pc = 1 (no row broadcast)
    "2x2-A": Case(4, 1, "A", 640, 128),                     # 5: ragged both ways, gcd 2, period 1
    "3x2-A": Case(6, 1, "A", 1280, 128, (9,), BOTH),        # 10: pr != pc, gcd 1, period 3
    "4x2-A": Case(8, 1, "A", 640, 128),                     # 5: gcd 2, period 2; four ranks own no diagonal block
    "3x2-A-norows": Case(6, 1, "A", 128, 128),              # 1: two block rows on three process rows
    "2x1-A-nb96": Case(2, 1, "A", 480, 96),                 # 5: a block below one leaf
    "2x2-C-nb200": Case(4, 1, "C", 1000, 200, (9, 1, 65), BOTH),   # 5: 1.56 leaves: the inverses message ends in a partial leaf
    "3x2-A-nb256": Case(6, 1, "A", 1792, 256),              # 7: two leaves per block, ragged
    "3x1-A-d2": Case(3, 2, "A", 640, 128),                  # 5: gram_nd_sel over distinct selections
    "3x2-C-d2": Case(6, 2, "C", 640, 128, (9, 1, 65)),      # 5: the same with pr != pc
    "2x2-D-d3": Case(4, 3, "D", 384, 128),                  # 3: d = 3, periods in hyp
    "2x1-B-d2": Case(2, 2, "B", 384, 128),                  # 3: sum kernel, d > 1
    "1x1-A-d2": Case(1, 2, "A", 640, 128),                  # 5: world 1 over RCCL
}


def _inputs(d, fam, N, notpd=False):
    """the recipes of test_fit_vs_oracle (d = 1) and test_fit_pairs_vs_oracle (d > 1), seed 1234 -> (X or None, q, P, z, hyp, s2)"""
    rng = np.random.default_rng(1234)
    if d == 1:
        q, P, z = rng.uniform(0, 2 * np.pi, N), rng.uniform(-3, 3, N), rng.standard_normal(2 * N)
        l = 2.0 * np.sqrt(12 * np.pi / N)
        hyp = [l, l, 0.5, 1.0] if fam == "D" else [l, l, 1.0]
        if notpd:                      # sig < 0 flips the sign of K: a pivot turns negative early (tests/test_dist_cpu.py)
            return None, q, P, z, [l, l, -4.0], 2.0 / l**2
        return None, q, P, z, hyp, 1e-2 / l**2
    X = np.column_stack([rng.uniform(0, 2 * np.pi, (N, d)), rng.uniform(-3, 3, (N, d))])
    z = rng.standard_normal(2 * d * N)
    l = 1.2 * (12 * np.pi / N) ** (1.0 / (2 * d))
    hyp = np.append(np.full(2 * d, l), 1.0)
    if fam == "D":
        hyp = np.concatenate((hyp[:-1], np.full(d, 0.5), hyp[-1:]))
    return X, None, None, z, hyp, 1e-2 / l**2


def _rhs(z, nrhs):
    B = np.random.default_rng(77).standard_normal((len(z), nrhs))
    B[:, 0] = z
    return B


def _snapshot(f):
    """the blocks this rank holds, {(I, J): nb x nb array, rows = matrix rows} (DistFit._blk is a [column, row] view)"""
    return {(f.rows[li], J): f._blk(li, lj).cpu().numpy().T.copy()
            for lj, J in enumerate(f.cols) for li in range(f.lifirst[lj], len(f.rows))}


def _worker(rank, world, port, d, fam, N, nb, nrhs, modes, notpd, poisons, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    backend = "nccl" if world == 1 else "gloo"
    kw = {"device_id": torch.device("cuda", 0)} if backend == "nccl" else {}
    # the timeout: a rank that dies makes its peers raise instead of waiting for it
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120), **kw)
    try:
        from sympgpr_amd.dist import DistFit, HipOps
        X, q, P, z, hyp, s2 = _inputs(d, fam, N, notpd)
        ops = HipOps(torch.device("cuda", 0))
        res = []
        for serial in modes:
            for poison in poisons:
                f = DistFit(ops, fam, q, P, z, hyp, s2, nb=nb, X=X, serial=serial)
                assert f.nb == nb and f.serial == serial
                f.A.fill_(float("nan"))          # whatever build() does not write is seen
                f.build()
                for (K, j) in poison:            # entry j of the diagonal of diagonal block K, by its owner
                    if K in f.owned:
                        f._blk(K // f.pr, K // f.pc).diagonal()[j] = -1.0
                r = {"serial": serial, "poison": poison, "K": None if (notpd or poison) else _snapshot(f)}
                r["info"] = f.factor()
                if r["info"] == 0:
                    r["L"] = _snapshot(f)
                    r["alpha"] = f.solve().cpu().numpy().copy()
                    r["nll"] = f.nll
                    r["X"] = {m: f.solve_rhs(_rhs(z, m)).cpu().numpy().copy() for m in nrhs}
                res.append(r)
        out[rank] = res
    finally:
        dist.destroy_process_group()


def _spawn(world, d, fam, N, nb, nrhs=(9,), modes=(False,), notpd=False, poisons=((),), meanwhile=lambda: None):
    """run the workers; `meanwhile` (the oracle's part) runs in this process while they do -> (per-rank results, its value)"""
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    with mp.Manager() as mgr:
        out = mgr.dict()
        ctx = mp.spawn(_worker, args=(world, port, d, fam, N, nb, tuple(nrhs), tuple(modes), notpd, tuple(poisons), out),
                       nprocs=world, join=False)
        try:
            ref = meanwhile()
        finally:
            while not ctx.join():
                pass
        res = dict(out)
    assert sorted(res) == list(range(world))
    return res, ref


_REF = {}


def _reference(oracle, d, fam, N):
    """Ky, alpha, nll, L of the oracle for one (d, family, N) -- computed once, shared by the cases, never written to"""
    key = (d, fam, N)
    if key not in _REF:
        X, q, P, z, hyp, s2 = _inputs(d, fam, N)
        if d == 1:
            K = oracle.build_K(fam, q, P, q, P, hyp, threads=8)
            a, nll, Lo = oracle.fit(fam, q, P, z, hyp, s2, threads=8)
        else:
            K = oracle.build_K_nd(fam, X, X, hyp)
            a, nll, Lo = oracle.fit_nd(fam, X, z, hyp, s2)
        Ky = K + s2 * np.eye(K.shape[0])
        for arr in (Ky, a, Lo):
            arr.setflags(write=False)
        _REF[key] = {"Ky": Ky, "alpha": a, "nll": nll, "L": Lo, "z": z, "X": {}}
    return _REF[key]


def _rhs_reference(ref, nrhs):
    import scipy.linalg
    if nrhs not in ref["X"]:
        if "cho" not in ref:
            ref["cho"] = scipy.linalg.cho_factor(ref["Ky"], lower=True)
        ref["X"][nrhs] = scipy.linalg.cho_solve(ref["cho"], _rhs(ref["z"], nrhs))
    return ref["X"][nrhs]


def _assemble(res, which, nb, nbk, mode):
    """the ranks' blocks of result `mode` put together; the union must be exactly the blocks I >= J, each held once"""
    held = [key for r in sorted(res) for key in res[r][mode][which]]
    assert sorted(held) == [(I, J) for I in range(nbk) for J in range(I + 1)], "the ranks' blocks are not the lower block triangle, each once"
    M = np.zeros((nbk * nb, nbk * nb))
    for r in res:
        for (I, J), blk in res[r][mode][which].items():
            assert blk.shape == (nb, nb)
            M[I * nb:(I + 1) * nb, J * nb:(J + 1) * nb] = blk
    return M


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", list(CASES))
def test_dist_hip_vs_oracle(oracle, name):
    """build(), factor(), solve() and solve_rhs() of DistFit(HipOps), stage by stage against the oracle.

    Serial and overlapped mode issue the same kernels on the same operands in the same order and gloo reduces in the same
    order, so the two alphas are compared bit for bit."""
    from tests.test_gpu_parity import GRAM_RTOL, gram_close
    c = CASES[name]
    n = 2 * c.d * c.N
    nbk = n // c.nb
    res, ref = _spawn(c.world, c.d, c.fam, c.N, c.nb, c.nrhs, c.modes, meanwhile=lambda: _reference(oracle, c.d, c.fam, c.N))
    Ky, a_o, nll_o, L_o = ref["Ky"], ref["alpha"], ref["nll"], ref["L"]
    low = np.tril(np.ones((n, n), dtype=bool))               # the lower triangle: all that the packed storage defines
    for mode, serial in enumerate(c.modes):
        tag = "DISTPARITY %s%s:" % (name, " serial" if serial else "")
        assert all(res[r][mode]["serial"] == serial for r in res)
        # 1. the Gram blocks
        Kh = _assemble(res, "K", c.nb, nbk, mode)
        gate = GRAM_RTOL * np.abs(Ky).max() + 3e-13 * np.abs(Ky[low])
        with np.errstate(invalid="ignore"):
            print(tag, "worst Gram error / gate = %.3f" % np.nan_to_num(np.abs(Kh[low] - Ky[low]) / gate, nan=np.inf).max())
        assert gram_close(Kh[low], Ky[low])
        # 2. the factor
        assert [res[r][mode]["info"] for r in sorted(res)] == [0] * c.world
        Lh = _assemble(res, "L", c.nb, nbk, mode)
        eL = np.nan_to_num(np.abs(Lh[low] - L_o[low]), nan=np.inf).max() / np.abs(L_o).max()
        print(tag, "max |L - L_o| / max |L_o| = %.3e (gate 1e-11)" % eL)
        assert eL <= 1e-11
        # 3. alpha, nll
        a0 = res[0][mode]["alpha"]
        ea = np.linalg.norm(a0 - a_o) / np.linalg.norm(a_o)
        print(tag, "|alpha - alpha_o| / |alpha_o| = %.3e (gate 1e-10), nll rel %.3e (gate 1e-11)"
              % (ea, max(abs(res[r][mode]["nll"] - nll_o) for r in res) / abs(nll_o)))
        assert ea < 1e-10
        for r in sorted(res):
            assert _same_bits(res[r][mode]["alpha"], a0), "alpha of rank %d differs from rank 0's" % r
            assert res[r][mode]["nll"] == pytest.approx(nll_o, rel=1e-11)
        # 4. blocks of right-hand sides
        for m in c.nrhs:
            X_o = _rhs_reference(ref, m)
            X0 = res[0][mode]["X"][m]
            assert X0.shape == X_o.shape == (n, m)
            print(tag, "nrhs %d: |X - X_o| / |X_o| = %.3e (gate 1e-10), |X[:,0] - alpha| / |alpha| = %.3e (gate 1e-12)"
                  % (m, np.linalg.norm(X0 - X_o) / np.linalg.norm(X_o), np.linalg.norm(X0[:, 0] - a0) / np.linalg.norm(a0)))
            assert np.linalg.norm(X0 - X_o) <= 1e-10 * np.linalg.norm(X_o)
            assert np.linalg.norm(X0[:, 0] - a0) <= 1e-12 * np.linalg.norm(a0)
            for r in sorted(res):
                assert _same_bits(res[r][mode]["X"][m], X0), "X (nrhs %d) of rank %d differs from rank 0's" % (m, r)
    # 5. the two modes
    if len(c.modes) == 2:
        assert _same_bits(res[0][0]["alpha"], res[0][1]["alpha"]), "serial and overlapped mode give different alpha"


@pytest.mark.parametrize("world", [4, 6])
def test_dist_hip_not_pd_info(oracle, world):
    """Ky indefinite from its eighth row on (sig < 0): every rank's factor() returns LAPACK's info for the oracle's Ky; the
    index is tracked on the device and agreed by one reduction."""
    import scipy.linalg
    N, nb = 640, 128

    def expect():
        _, q, P, _, hyp, s2 = _inputs(1, "A", N, notpd=True)
        Ky = oracle.build_K("A", q, P, q, P, hyp, threads=8) + s2 * np.eye(2 * N)
        return scipy.linalg.lapack.dpotrf(Ky, lower=1)[1]

    res, info_o = _spawn(world, 1, "A", N, nb, notpd=True, meanwhile=expect)
    assert info_o == 8
    assert [res[r][0]["info"] for r in sorted(res)] == [info_o] * world


def test_dist_hip_not_pd_where_rank0_is_not_the_owner(oracle):
    """A pivot made negative in a diagonal block that rank 0 does not own (as test_potrf_not_pd does on one matrix: entry j
    of the diagonal of block K := -1 after build(), every earlier leading minor stays positive definite): info is K nb + j + 1
    on every rank, and of two such blocks the earlier one's.  A failed pivot leaves NaN from its column on (leaf.h) and the
    blocks after it report their own first column; no kernel of this path waits for another (blocks of <= 4 leaves are factored
    and solved by the plain recursion), so NaN cannot keep anything waiting."""
    import scipy.linalg
    N, nb, world = 1280, 128, 6
    nbk = 2 * N // nb
    poisons = (((nbk - 1, nb - 1),), ((3, 17), (7, 0)))

    def expect():
        Ky = _reference(oracle, 1, "A", N)["Ky"]
        infos = []
        for poison in poisons:
            M = Ky.copy()
            for (K, j) in poison:
                M[K * nb + j, K * nb + j] = -1.0
            infos.append(scipy.linalg.lapack.dpotrf(M, lower=1)[1])
        return infos

    res, infos_o = _spawn(world, 1, "A", N, nb, poisons=poisons, meanwhile=expect)
    assert infos_o == [(nbk - 1) * nb + nb, 3 * nb + 17 + 1]
    for i, info_o in enumerate(infos_o):
        assert [res[r][i]["info"] for r in sorted(res)] == [info_o] * world
