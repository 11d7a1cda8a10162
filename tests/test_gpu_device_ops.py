"""The device-pointer primitives of include/sympgpr_hip.h, called directly through the C ABI (ctypes) on torch
buffers and a non-default stream, each against a plain host reference.

Every output lives in a guarded buffer: a sentinel NaN with a recognisable payload fills the guard regions before
and after it and the padding rows between the extent and the leading dimension, and must be bit-identical after the
call.  Operands that are only read must come back bit-identical.  Operands sit either 16-byte aligned with an even
leading dimension or one double further on with an odd one: the two reach the fast and the general bodies.

Products (GEMM, GEMV) and copies use small integer operands, so every partial sum is exact in fp64 and the device
result must equal numpy whatever the order of summation.  Random operands are held to a componentwise bound
|C - C_ref| <= 2 (k + 2) u (|alpha| |A| |B|^T + |beta| |C0|), u = 2^-53.  Solves are held to the normwise backward
error ||X L^T - B||_F / (||L||_F ||X||_F) <= 4 n u plus a forward error against SciPy on well-conditioned factors
(cond(L) < 2)."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GUARD = 64                                       # doubles before and after every buffer (keeps the base 16-byte aligned)
SENT_BITS = np.uint64(0x7FF8DEADBEEF0001)        # quiet NaN, payload 0xdeadbeef0001
SENT = np.array([SENT_BITS], dtype=np.uint64).view(np.float64)[0]
GRAM_RTOL = 4e-15                                # tests/test_gpu_parity.py
HYP = {"A": [0.5, 2.0, 0.4], "B": [0.5, 2.0, 0.4], "C": [0.5, 2.0, 0.4], "D": [0.5, 2.0, 0.7, 0.4]}


def gram_close(K, Kref):
    """the tolerance of test_gram_vs_oracle: |dK| <= 4e-15 max|K| + 3e-13 |K| elementwise"""
    return bool(np.all(np.abs(K - Kref) <= GRAM_RTOL * np.abs(Kref).max() + 3e-13 * np.abs(Kref)))


@pytest.fixture(scope="module")
def dev():
    import torch
    from sympgpr_amd import _lib as L
    lib = L.load_library()
    if lib.sgpr_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need the MI355X")
    L.check(lib.sgpr_set_device(0))
    stream = torch.cuda.Stream()
    return Dev(torch, L, lib, stream)


class Dev:
    def __init__(self, torch, L, lib, stream):
        self.torch, self.L, self.lib, self.stream = torch, L, lib, stream
        self.sp = C.c_void_p(stream.cuda_stream)

    def call(self, name, *args):
        """run one entry on the test's stream and wait for that stream; returns the entry's return value"""
        self.torch.cuda.synchronize()               # uploads (default stream) are complete
        rc = getattr(self.lib, name)(*args)
        self.stream.synchronize()
        return rc

    def ok(self, name, *args):
        rc = self.call(name, *args)
        assert rc == 0, (name, rc, self.lib.sgpr_last_error())

    def buf(self, rows, cols, ld, odd=False, fill=None):
        return GBuf(self, rows, cols, ld, odd, fill)

    def work(self, n):
        """a factor workspace, NaN-filled"""
        nd = (self.lib.sgpr_potrf_workspace(n) + 7) // 8
        return self.torch.full((nd,), float("nan"), dtype=self.torch.float64, device="cuda")


class GBuf:
    """column-major rows x cols at leading dimension ld inside a sentinel-filled allocation with guards"""

    def __init__(self, d, rows, cols, ld, odd, fill):
        assert ld >= max(rows, 1)
        self.d, self.rows, self.cols, self.ld = d, rows, cols, ld
        self.base = GUARD + (1 if odd else 0)
        n = self.base + ld * max(cols, 1) + GUARD
        h = np.full(n, SENT)
        if fill is not None:
            self.view(h)[:, :] = fill
        self.h0 = h
        self.t = d.torch.from_numpy(h.copy()).to("cuda")

    def view(self, h):
        return h[self.base:self.base + self.ld * self.cols].reshape(self.cols, self.ld).T[:self.rows]

    @property
    def p(self):
        return C.c_void_p(self.t.data_ptr() + 8 * self.base)

    def host(self):
        return self.t.cpu().numpy()

    def get(self):
        """the matrix; asserts every byte outside it (guards, padding rows) is as it was"""
        h = self.host()
        inside = np.zeros(h.shape, bool)
        self.view(inside)[:, :] = True
        assert np.array_equal(h.view(np.uint64)[~inside], self.h0.view(np.uint64)[~inside]), "write outside the extent"
        return self.view(h).copy()

    def rebase(self):
        """take the current device contents as the reference of later checks"""
        self.h0 = self.host().copy()

    def unchanged(self):
        return np.array_equal(self.host().view(np.uint64), self.h0.view(np.uint64))


def ldp(rows, odd, extra=0):
    """a leading dimension >= rows + extra: even for the aligned placement, odd for the one-double offset"""
    ld = max(rows + extra, 1)
    return ld + 1 if (ld & 1) != int(odd) else ld


def ints(rng, *shape):
    """small non-zero integers: products and partial sums stay exact in fp64"""
    v = rng.integers(1, 5, size=shape).astype(np.float64)
    return v * rng.choice([-1.0, 1.0], size=shape)


# ---------------------------------------------------------------------------------------------- GEMM (NT / NN)
# (m, n, k, alpha, beta): the branch each reaches in gemm_launch / gemm_nt_bc (csrc/gemm_f64.hip)
GEMM_EXACT = [
    (1, 128, 16, 1.0, 1.0),          # 64x128 tiles (n <= 128, m <= 32768)
    (63, 100, 17, -1.0, -0.5),
    (64, 128, 16, 0.37, 0.0),
    (65, 128, 15, 0.0, -0.5),
    (32768, 128, 16, 1.0, 1.0),      # last m of the 64-row tiles
    (32769, 128, 16, -1.0, 0.0),     # n = 128, m > 32768: 256x128
    (40000, 100, 16, 0.37, 1.0),     # n < 128, m > 32768: 128x128
    (300, 200, 1, 1.0, -0.5),        # 128x128, small grid
    (300, 200, 0, 0.37, -0.5),       # k = 0: C := beta C
    (300, 200, 0, 1.0, 0.0),         # k = 0, beta = 0: C := 0 over NaN
    (4096, 2048, 16, -1.0, 1.0),     # 256x128, 256 workgroups
    (512, 128, 64, 0.37, -0.5),      # 256x128, m >= 256 and n = 128
    (256, 128, 8192, 1.0, -0.5),     # deepest single launch
    (200, 130, 8193, -1.0, 0.0),     # two k-chunks, beta = 0 over NaN only in the first
    (130, 64, 16500, 1.0, 1.0),      # three k-chunks
]


def _gemm_case(dev, m, n, k, alpha, beta, odd, nn, seed):
    rng = np.random.default_rng(seed)
    A = ints(rng, m, k)
    Bm = ints(rng, k, n) if nn else ints(rng, n, k)
    C0 = np.full((m, n), np.nan) if beta == 0.0 else ints(rng, m, n)
    ga = dev.buf(m, k, ldp(m, odd, 1), odd, A)
    gb = dev.buf(*Bm.shape, ldp(Bm.shape[0], odd, 3 if nn else 1), odd, Bm)   # NN: ldb > k
    gc = dev.buf(m, n, ldp(m, odd, 4), odd, C0)
    if nn:
        dev.ok("sgpr_gemm_nn_dev", m, n, k, alpha, ga.p, ga.ld, gb.p, gb.ld, beta, gc.p, gc.ld, dev.sp)
    else:
        dev.ok("sgpr_gemm_nt_dev", m, n, k, alpha, ga.p, ga.ld, gb.p, gb.ld, beta, gc.p, gc.ld, 0, 0, dev.sp)
    P = A @ (Bm if nn else Bm.T)
    ref = alpha * P if beta == 0.0 else beta * C0 + alpha * P
    return gc.get(), ref, ga, gb


def _exact_ok(alpha, k):
    # alpha * P is one rounding; more than one k-chunk adds the rounded chunk products one by one, which is
    # exact only for alpha = +-1, 0
    return k <= 8192 or alpha in (1.0, -1.0, 0.0)


@pytest.mark.parametrize("nn", [False, True], ids=["nt", "nn"])
@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd"])
@pytest.mark.parametrize("case", GEMM_EXACT, ids=lambda c: "m%d_n%d_k%d_a%g_b%g" % c)
def test_gemm_exact(dev, case, odd, nn):
    """integer operands: the device result equals numpy exactly; guards, padding and the operands are untouched;
    beta = 0 overwrites a NaN-filled C"""
    m, n, k, alpha, beta = case
    if not _exact_ok(alpha, k):
        alpha = 1.0
    got, ref, ga, gb = _gemm_case(dev, m, n, k, alpha, beta, odd, nn, m + 7 * n + 13 * k)
    assert ga.unchanged() and gb.unchanged()
    assert not np.isnan(got).any()
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]


@pytest.mark.parametrize("nn", [False, True], ids=["nt", "nn"])
@pytest.mark.parametrize("case", [(300, 200, 200, 0.37, -0.5, True), (129, 77, 8193, 0.37, 1.0, True),
                                  (1000, 1000, 16500, 0.37, 0.0, False), (2048, 4096, 512, -1.0, 1.0, False)],
                         ids=lambda c: "m%d_n%d_k%d" % c[:3])
def test_gemm_random_bound(dev, case, nn):
    """random operands, alpha = 0.37 over k-chunks: componentwise bound against long double (small) or fp64 BLAS"""
    m, n, k, alpha, beta, longd = case
    rng = np.random.default_rng(m * 31 + k)
    A = rng.standard_normal((m, k))
    Bm = rng.standard_normal((k, n) if nn else (n, k))
    C0 = rng.standard_normal((m, n)) if beta != 0.0 else np.full((m, n), np.nan)
    ga = dev.buf(m, k, m + 1, True, A)
    gb = dev.buf(*Bm.shape, Bm.shape[0] + 1, True, Bm)
    gc = dev.buf(m, n, m + 3, True, C0)
    if nn:
        dev.ok("sgpr_gemm_nn_dev", m, n, k, alpha, ga.p, ga.ld, gb.p, gb.ld, beta, gc.p, gc.ld, dev.sp)
    else:
        dev.ok("sgpr_gemm_nt_dev", m, n, k, alpha, ga.p, ga.ld, gb.p, gb.ld, beta, gc.p, gc.ld, 0, 0, dev.sp)
    got = gc.get()
    Bt = Bm if nn else Bm.T
    C0z = np.zeros_like(C0) if beta == 0.0 else C0
    if longd:
        ref = (np.longdouble(alpha) * (A.astype(np.longdouble) @ Bt.astype(np.longdouble))
               + np.longdouble(beta) * C0z.astype(np.longdouble))
    else:
        ref = alpha * (A @ Bt) + beta * C0z
    bound = 2 * (k + 2) * U * (abs(alpha) * (np.abs(A) @ np.abs(Bt)) + abs(beta) * np.abs(C0z))
    err = np.abs(got - ref).astype(np.float64)
    assert np.all(err <= bound), float((err / bound).max())


@pytest.mark.parametrize("case", [(500, 300, 32, -70), (500, 300, 32, 45), (300, 500, 17, 200), (1000, 130, 16, -300),
                                  (333, 333, 16, 0)], ids=lambda c: "m%d_n%d_k%d_d%d" % c)
@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd"])
def test_gemm_lower_diag_off(dev, case, odd):
    """lower mode: every element with row + diag_off >= col is updated; any other element is either updated
    correctly or bit-identical to its input"""
    m, n, k, doff = case
    rng = np.random.default_rng(m + n + doff)
    A, Bm, C0 = ints(rng, m, k), ints(rng, n, k), ints(rng, m, n)
    ga, gb = dev.buf(m, k, ldp(m, odd), odd, A), dev.buf(n, k, ldp(n, odd, 2), odd, Bm)
    gc = dev.buf(m, n, m + 5, odd, C0)
    dev.ok("sgpr_gemm_nt_dev", m, n, k, -1.0, ga.p, ga.ld, gb.p, gb.ld, 1.0, gc.p, gc.ld, 1, doff, dev.sp)
    got = gc.get()
    ref = C0 - A @ Bm.T
    i, j = np.indices((m, n))
    need = i + doff >= j
    assert np.array_equal(got[need], ref[need])
    assert np.all((got[~need] == ref[~need]) | (got[~need].view(np.uint64) == C0[~need].view(np.uint64)))
    assert ga.unchanged() and gb.unchanged()


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd"])
@pytest.mark.parametrize("m,n", [(1000, 128), (1000, 100), (40000, 128), (40000, 100)])
def test_gemm_in_place_leaf(dev, m, n, odd):
    """C == A with k = n <= 128 (the leaf step of trsm_rlt / trsm_rl): equals the out-of-place product bit for
    bit, on the fast (aligned, even ld) and the general body"""
    rng = np.random.default_rng(m + n)
    X = rng.standard_normal((m, n))
    inv = np.tril(rng.standard_normal((n, n)))
    gi = dev.buf(n, n, 128, False, inv)
    gx = dev.buf(m, n, ldp(m, odd, 2), odd, X)
    go = dev.buf(m, n, ldp(m, odd, 2), odd, np.zeros((m, n)))
    dev.ok("sgpr_gemm_nt_dev", m, n, n, 1.0, gx.p, gx.ld, gi.p, gi.ld, 0.0, go.p, go.ld, 0, 0, dev.sp)
    dev.ok("sgpr_gemm_nt_dev", m, n, n, 1.0, gx.p, gx.ld, gi.p, gi.ld, 0.0, gx.p, gx.ld, 0, 0, dev.sp)
    out, inplace = go.get(), gx.get()
    assert np.array_equal(out.view(np.uint64), inplace.view(np.uint64))
    ref = X @ inv.T
    assert np.all(np.abs(out - ref) <= 2 * (n + 2) * U * (np.abs(X) @ np.abs(inv).T))
    # the NN leaf of trsm_rl: B := B inv
    gx2 = dev.buf(m, n, ldp(m, odd, 2), odd, X)
    go2 = dev.buf(m, n, ldp(m, odd, 2), odd, np.zeros((m, n)))
    dev.ok("sgpr_gemm_nn_dev", m, n, n, 1.0, gx2.p, gx2.ld, gi.p, gi.ld, 0.0, go2.p, go2.ld, dev.sp)
    dev.ok("sgpr_gemm_nn_dev", m, n, n, 1.0, gx2.p, gx2.ld, gi.p, gi.ld, 0.0, gx2.p, gx2.ld, dev.sp)
    assert np.array_equal(go2.get().view(np.uint64), gx2.get().view(np.uint64))


def _bc_needed(m, n, blk, pr, pi, pc, pj):
    i, j = np.indices((m, n))
    rbg, cbg = (i // blk) * pr + pi, (j // blk) * pc + pj
    return (rbg > cbg) | ((rbg == cbg) & (i % blk >= j % blk))


@pytest.mark.parametrize("blk", [64, 100, 128, 300])
@pytest.mark.parametrize("grid", [(1, 1), (2, 1), (2, 2), (3, 2), (2, 4)], ids=lambda g: "%dx%d" % g)
def test_gemm_nt_bc(dev, grid, blk):
    """block-cyclic lower update at every (pi, pj) of the grid: on/below the global diagonal updated correctly,
    everything else correct or untouched"""
    pr, pc = grid
    m, n, k = 3 * blk + 17, 2 * blk + 5, 16
    rng = np.random.default_rng(blk * 10 + pr * 3 + pc)
    A, Bm = ints(rng, m, k), ints(rng, n, k)
    ref_prod = A @ Bm.T
    ga, gb = dev.buf(m, k, m + 1, True, A), dev.buf(n, k, n, False, Bm)
    for pi in range(pr):
        for pj in range(pc):
            C0 = ints(rng, m, n)
            gc = dev.buf(m, n, m + 2, False, C0)
            dev.ok("sgpr_gemm_nt_bc_dev", m, n, k, -1.0, ga.p, ga.ld, gb.p, gb.ld, 1.0, gc.p, gc.ld, blk, pr, pi, pc, pj,
                   dev.sp)
            got, ref = gc.get(), C0 - ref_prod
            need = _bc_needed(m, n, blk, pr, pi, pc, pj)
            assert np.array_equal(got[need], ref[need]), (pi, pj)
            other = ~need
            assert np.all((got[other] == ref[other]) | (got[other].view(np.uint64) == C0[other].view(np.uint64))), (pi, pj)
    assert ga.unchanged() and gb.unchanged()


def test_gemm_profile_flop(dev):
    """the algorithmic flop count of lower and block-cyclic launches: 2k x the on-or-below-diagonal elements"""
    m, n, k, doff = 300, 200, 16, 37
    rng = np.random.default_rng(5)
    ga, gb = dev.buf(m, k, m, False, rng.standard_normal((m, k))), dev.buf(n, k, n, False, rng.standard_normal((n, k)))
    gc = dev.buf(m, n, m, False, np.zeros((m, n)))
    blk, pr, pi, pc, pj = 64, 2, 1, 3, 1
    out = (C.c_double * 12)()
    assert dev.lib.sgpr_profile_begin() == 0
    try:
        dev.ok("sgpr_gemm_nt_dev", m, n, k, 1.0, ga.p, ga.ld, gb.p, gb.ld, 1.0, gc.p, gc.ld, 1, doff, dev.sp)
        dev.ok("sgpr_gemm_nt_bc_dev", m, n, k, 1.0, ga.p, ga.ld, gb.p, gb.ld, 1.0, gc.p, gc.ld, blk, pr, pi, pc, pj, dev.sp)
    finally:
        assert dev.lib.sgpr_profile_end(out) == 0
    i, j = np.indices((m, n))
    elems = int((i + doff >= j).sum()) + int(_bc_needed(m, n, blk, pr, pi, pc, pj).sum())
    assert out[0] + out[3] + out[8] == 2
    assert out[1] + out[4] + out[9] == 2.0 * k * elems


# ---------------------------------------------------------------------------------------------- GEMV
@pytest.mark.parametrize("lda_pad", [0, 1])
@pytest.mark.parametrize("trans", [0, 1])
def test_gemv_sub(dev, trans, lda_pad):
    """y -= A x / y -= A^T x, integer operands: exact; guards of y; A and x untouched"""
    rng = np.random.default_rng(trans * 2 + lda_pad)
    sizes = [0, 1, 63, 64, 65, 1000, 4097]
    for m in sizes:
        for k in sizes:
            A = ints(rng, m, k)
            x = ints(rng, k if trans == 0 else m, 1)
            y = ints(rng, m if trans == 0 else k, 1)
            odd = bool(lda_pad)
            ga = dev.buf(m, k, max(m + lda_pad, 1), odd, A)
            gx = dev.buf(x.shape[0], 1, max(x.shape[0], 1), odd, x)
            gy = dev.buf(y.shape[0], 1, max(y.shape[0], 1), odd, y)
            dev.ok("sgpr_gemv_sub_dev", trans, m, k, ga.p, ga.ld, gx.p, gy.p, dev.sp)
            ref = y - (A @ x if trans == 0 else A.T @ x)
            assert np.array_equal(gy.get(), ref), (m, k)
            assert ga.unchanged() and gx.unchanged()


# ---------------------------------------------------------------------------------------------- copy_blocks
COPY_CASES = [(1, 1, 1), (255, 1023, 3), (256, 1024, 1), (257, 1025, 3), (1000, 3000, 1), (1, 3000, 70),
              (257, 1, 70), (256, 5, 70), (1000, 1024, 3), (255, 1025, 1)]


@pytest.mark.parametrize("case", COPY_CASES, ids=lambda c: "r%d_c%d_n%d" % c)
def test_copy_blocks(dev, case):
    """bitwise copy of cnt blocks (NaN payloads, -0.0, infinities, subnormals) with ld > rows and
    non-contiguous steps; nothing between the blocks is written"""
    rows, cols, cnt = case
    rng = np.random.default_rng(rows * 7 + cols + cnt)
    lds, ldd = rows + 3, rows + 1
    sstep, dstep = lds * cols + 5, ldd * cols + 9
    src = rng.standard_normal(sstep * cnt)
    special = np.array([0x7FF0000000000001, 0x7FF8000000000123, 0xFFF4000000000ABC, 0x8000000000000000,
                        0x7FF0000000000000, 0x0000000000000001], dtype=np.uint64)
    idx = rng.integers(0, src.size, size=min(src.size, 64))
    gs = dev.buf(src.size, 1, src.size, True, src[:, None])
    gs.h0.view(np.uint64)[gs.base + idx] = special[np.arange(idx.size) % special.size]
    gs.t.copy_(dev.torch.from_numpy(gs.h0))
    bits = gs.h0[gs.base:gs.base + src.size].view(np.uint64)
    gd = dev.buf(dstep * cnt, 1, dstep * cnt, False, None)
    dev.ok("sgpr_copy_blocks_dev", rows, cols, cnt, gs.p, lds, sstep, gd.p, ldd, dstep, dev.sp)
    got = gd.get()[:, 0].view(np.uint64)
    want = np.full(dstep * cnt, SENT_BITS, dtype=np.uint64)
    for b in range(cnt):
        s = bits[b * sstep:b * sstep + lds * cols].reshape(cols, lds)[:, :rows]
        want[b * dstep:b * dstep + ldd * cols].reshape(cols, ldd)[:, :rows] = s
    assert np.array_equal(got, want)
    assert gs.unchanged()


def test_copy_blocks_edges(dev):
    """a zero extent is a no-op; more than 65535 blocks is an argument error (buffers cover the call either way)"""
    gs = dev.buf(64, 1, 64, False, np.arange(64.0)[:, None])
    gd = dev.buf(64, 1, 64, False, None)
    for r, c, n in [(0, 4, 2), (4, 0, 2), (4, 4, 0)]:
        dev.ok("sgpr_copy_blocks_dev", r, c, n, gs.p, 4, 16, gd.p, 4, 16, dev.sp)
        assert gd.unchanged()
    rc = dev.call("sgpr_copy_blocks_dev", 1, 1, 65536, gs.p, 1, 0, gd.p, 1, 0, dev.sp)
    assert rc == dev.L.E_ARG and gd.unchanged()


# ---------------------------------------------------------------------------------------------- factor + solves
POTRF_ORDERS = [100, 128, 129, 512, 1000, 1024, 1280, 1536, 2048]


def spd(n, seed):
    """well-conditioned SPD: eigenvalues in [2, ~6] (cond(L) < 2)"""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    return M @ M.T / n + 2.0 * np.eye(n)


def factor(dev, n, ld, odd, seed):
    """sgpr_potrf_dev on a guarded copy of spd(n) whose strict upper triangle holds the sentinel"""
    A = spd(n, seed)
    Au = np.tril(A) + np.triu(np.full((n, n), SENT), 1)
    ga = dev.buf(n, n, ld, odd, Au)
    work = dev.work(n)
    info = dev.torch.full((1,), -7, dtype=dev.torch.int32, device="cuda")
    dev.ok("sgpr_potrf_dev", n, ga.p, ga.ld, C.c_void_p(work.data_ptr()), 8 * work.numel(),
           C.c_void_p(info.data_ptr()), dev.sp)
    assert dev.lib.sgpr_potrf_info_dev(int(info.item()), dev.sp) == 0
    return A, ga, work


def factored(dev, n, ld, odd, seed):
    """factor(), with the factor itself as the reference of the buffer's later checks (solves only read L)"""
    A, ga, work = factor(dev, n, ld, odd, seed)
    ga.rebase()
    return A, ga, work


@pytest.mark.parametrize("lda_pad", [0, 1])
@pytest.mark.parametrize("n", POTRF_ORDERS)
def test_potrf(dev, n, lda_pad):
    """L against SciPy; the strict upper triangle (sentinel NaN), padding rows and guards are untouched"""
    A, ga, _ = factor(dev, n, n + lda_pad, bool(lda_pad), n)
    got = ga.get()
    iu = np.triu_indices(n, 1)
    assert np.all(got[iu].view(np.uint64) == SENT_BITS), "strict upper triangle written"
    Lg = np.tril(got)
    Ls = scipy.linalg.cholesky(A, lower=True)
    assert np.linalg.norm(Lg @ Lg.T - A) <= 4 * n * U * np.linalg.norm(A)
    assert np.linalg.norm(Lg - Ls) <= 4 * n * U * np.linalg.norm(Ls)


@pytest.mark.parametrize("n,j", [(100, 0), (129, 128), (1000, 127), (1000, 700), (1536, 1300), (2048, 2047)])
def test_potrf_not_pd(dev, n, j):
    """a matrix that stops being positive definite at column j reports the minor j + 1"""
    A = spd(n, n + j)
    A[j, j] = -1.0
    ga = dev.buf(n, n, n, False, A)
    work = dev.work(n)
    info = dev.torch.full((1,), -7, dtype=dev.torch.int32, device="cuda")
    dev.ok("sgpr_potrf_dev", n, ga.p, ga.ld, C.c_void_p(work.data_ptr()), 8 * work.numel(),
           C.c_void_p(info.data_ptr()), dev.sp)
    assert dev.lib.sgpr_potrf_info_dev(int(info.item()), dev.sp) == j + 1
    ga.get()


def _inverses_only(dev, n, work):
    """a fresh workspace holding only the first sgpr_potrf_inverses_bytes(n) bytes of `work`, NaN behind them"""
    w2 = dev.torch.full_like(work, float("nan"))
    ni = dev.lib.sgpr_potrf_inverses_bytes(n) // 8
    w2[:ni] = work[:ni]
    dev.torch.cuda.synchronize()
    return w2


# (n, m, ldb pad, B odd, ldl pad): every order of POTRF_ORDERS, every m, ldb pad and alignment at least once
TRSM_CASES = [(100, 1, 0, False, 0), (128, 7, 1, True, 1), (129, 64, 3, False, 0), (512, 65, 0, True, 1),
              (1000, 1000, 1, False, 1), (1024, 65, 3, True, 0), (1280, 1000, 0, False, 0), (1536, 7, 3, True, 1),
              (2048, 64, 1, True, 0), (129, 33000, 0, False, 1), (256, 33000, 1, True, 0)]


@pytest.mark.parametrize("case", TRSM_CASES, ids=lambda c: "n%d_m%d_ldb+%d_%s_ldl+%d" % (c[0], c[1], c[2],
                                                                                        "odd" if c[3] else "al", c[4]))
def test_trsm_rlt_rl(dev, case):
    """B := B L^-T (rlt) then B L^-1 (rl) = B (L L^T)^-1, backward and forward error; the solve against an
    inverses-only workspace is bit-identical"""
    n, m, ldb_pad, odd, ldl_pad = case
    A, gl, work = factored(dev, n, n + ldl_pad, False, n + 1)
    Lh = np.tril(gl.get())
    rng = np.random.default_rng(n + m)
    B = rng.standard_normal((m, n))
    gb = dev.buf(m, n, m + ldb_pad, odd, B)
    wp = C.c_void_p(work.data_ptr())
    dev.ok("sgpr_trsm_rlt_dev", m, n, gl.p, gl.ld, gb.p, gb.ld, wp, dev.sp)
    Y = gb.get()
    dev.ok("sgpr_trsm_rl_dev", m, n, gl.p, gl.ld, gb.p, gb.ld, wp, dev.sp)
    X = gb.get()
    nL = np.linalg.norm(Lh)
    assert np.linalg.norm(Y @ Lh.T - B) <= 4 * n * U * nL * np.linalg.norm(Y)
    assert np.linalg.norm(X @ Lh - Y) <= 4 * n * U * nL * np.linalg.norm(X)
    Yref = scipy.linalg.solve_triangular(Lh, B.T, lower=True).T
    Xref = scipy.linalg.solve_triangular(Lh, Yref.T, lower=True, trans="T").T
    assert np.linalg.norm(Y - Yref) <= 8 * n * U * np.linalg.norm(Yref)
    assert np.linalg.norm(X - Xref) <= 16 * n * U * np.linalg.norm(Xref)
    assert gl.unchanged()
    # workspace contract: L and the leaf inverses are all the solves read
    w2 = _inverses_only(dev, n, work)
    gb2 = dev.buf(m, n, m + ldb_pad, odd, B)
    dev.ok("sgpr_trsm_rlt_dev", m, n, gl.p, gl.ld, gb2.p, gb2.ld, C.c_void_p(w2.data_ptr()), dev.sp)
    assert np.array_equal(gb2.get().view(np.uint64), Y.view(np.uint64))
    dev.ok("sgpr_trsm_rl_dev", m, n, gl.p, gl.ld, gb2.p, gb2.ld, C.c_void_p(w2.data_ptr()), dev.sp)
    assert np.array_equal(gb2.get().view(np.uint64), X.view(np.uint64))


TRSV_ORDERS = [1, 127, 128, 129, 512, 513, 640, 1024, 2048, 2304]


def _vec_solves(dev, n, gl, work, b):
    """trsv(0), trsv(1), potrs_vec, each followed by solve_status; the vectors after each step"""
    wp = C.c_void_p(work.data_ptr())
    out = []
    for step in ("n", "t", "potrs"):
        gv = dev.buf(n, 1, n, False, b[:, None])
        if step == "potrs":
            dev.ok("sgpr_potrs_vec_dev", n, gl.p, gl.ld, wp, gv.p, dev.sp)
        else:
            dev.ok("sgpr_trsv_dev", n, gl.p, gl.ld, wp, gv.p, 1 if step == "t" else 0, dev.sp)
        assert dev.call("sgpr_solve_status_dev", n, gl.p, gl.ld, wp, dev.sp) == 0
        out.append(gv.get()[:, 0])
    return out


def _check_vec(n, Lh, b, xs):
    xn, xt, xp = xs
    nL = np.linalg.norm(Lh)
    assert np.linalg.norm(Lh @ xn - b) <= 4 * n * U * nL * np.linalg.norm(xn)
    assert np.linalg.norm(Lh.T @ xt - b) <= 4 * n * U * nL * np.linalg.norm(xt)
    for x, ref in ((xn, scipy.linalg.solve_triangular(Lh, b, lower=True)),
                   (xt, scipy.linalg.solve_triangular(Lh, b, lower=True, trans="T")),
                   (xp, scipy.linalg.cho_solve((Lh, True), b))):
        assert np.linalg.norm(x - ref) <= 16 * max(n, 8) * U * np.linalg.norm(ref)


@pytest.mark.parametrize("n", TRSV_ORDERS)
def test_trsv_potrs_vec(dev, n):
    """trsv (both directions), potrs_vec, solve_status: against SciPy, twice on one workspace, and bit-identical
    against an inverses-only workspace"""
    A, gl, work = factored(dev, n, n, False, 3 * n)
    Lh = np.tril(gl.get())
    b = np.random.default_rng(n).standard_normal(n)
    xs = _vec_solves(dev, n, gl, work, b)
    _check_vec(n, Lh, b, xs)
    again = _vec_solves(dev, n, gl, work, b)
    for x, y in zip(xs, again):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    w2 = _inverses_only(dev, n, work)
    for x, y in zip(xs, _vec_solves(dev, n, gl, w2, b)):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    assert gl.unchanged()


@pytest.mark.parametrize("n", [1024, 2304])
def test_trsv_strip_and_recursion_agree(dev, n):
    """one order, three paths: strips (ldl = n, aligned), recursion by ldl = n + 1, recursion by L one double off"""
    res = []
    b = np.random.default_rng(n + 1).standard_normal(n)
    for ld, odd in ((n, False), (n + 1, False), (n, True)):
        A, gl, work = factored(dev, n, ld, odd, 11)
        Lh = np.tril(gl.get())
        xs = _vec_solves(dev, n, gl, work, b)
        _check_vec(n, Lh, b, xs)
        res.append((Lh, xs))
    for Lh, xs in res[1:]:
        for x, y in zip(xs, res[0][1]):
            assert np.linalg.norm(x - y) <= 32 * n * U * np.linalg.norm(y)


# ---------------------------------------------------------------------------------------------- Gram builds
def _pts(rng, n):
    return rng.uniform(0, 2 * np.pi, n), rng.uniform(-3, 3, n)


def _dvec(dev, v):
    return dev.torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to("cuda")


def _hypc(h):
    h = np.ascontiguousarray(h, dtype=np.float64)
    return h.ctypes.data_as(C.POINTER(C.c_double)), len(h), h


@pytest.mark.parametrize("fam", "ABCD")
def test_gram_pairs_parts(dev, oracle, fam):
    """every subset of the four parts: selected parts match build_K, unselected (flag clear or null pointer) are
    never written; SGPR_G_OCML agrees with the default"""
    from sympgpr_amd import _lib as L
    mi, mj = 37, 29
    rng = np.random.default_rng(ord(fam))
    xb, yb = _pts(rng, mi)
    xa, ya = _pts(rng, mj)
    hp, nh, _keep = _hypc(HYP[fam])
    K = oracle.build_K(fam, xb, yb, xa, ya, HYP[fam])
    parts = [K[:mi, :mj], K[mi:, :mj], K[:mi, mj:], K[mi:, mj:]]
    dxb, dyb, dxa, dya = (_dvec(dev, v) for v in (xb, yb, xa, ya))
    P = [C.c_void_p(t.data_ptr()) for t in (dxb, dyb, dxa, dya)]
    for sub in range(1, 16):
        for nulls in (False, True):
            bufs = [dev.buf(mi, mj, mi + 3, bool(q & 1), None) for q in range(4)]
            ptr = [b.p if (sub >> q) & 1 or not nulls else None for q, b in enumerate(bufs)]
            flags = L.G_ALL if nulls else sub
            dev.ok("sgpr_gram_pairs_dev", L.family_id(fam), mi, mj, *P, hp, nh, *ptr, mi + 3, 0, 0.0, flags, dev.sp)
            for q, b in enumerate(bufs):
                if (sub >> q) & 1:
                    assert gram_close(b.get(), parts[q]), (sub, q)
                else:
                    assert b.unchanged(), (sub, q)
    bufs = [dev.buf(mi, mj, mi, False, None) for _ in range(4)]
    dev.ok("sgpr_gram_pairs_dev", L.family_id(fam), mi, mj, *P, hp, nh, *[b.p for b in bufs], mi, 0, 0.0,
           L.G_ALL | L.G_OCML, dev.sp)
    for q, b in enumerate(bufs):
        assert gram_close(b.get(), parts[q])


@pytest.mark.parametrize("doff", [-50, 0, 120])
@pytest.mark.parametrize("fam", "ABCD")
def test_gram_pairs_lower_noise(dev, oracle, fam, doff):
    """SGPR_G_LOWER with diag_off: on qq / PP every row + diag_off >= col is correct, the rest correct or untouched;
    Pq is written whole and qP not at all.  |noise| lands on qq and PP exactly where i + diag_off == j and nowhere
    else"""
    from sympgpr_amd import _lib as L
    mi, mj, noise = 300, 200, -0.75
    rng = np.random.default_rng(doff + 1000 + ord(fam))
    xb, yb = _pts(rng, mi)
    xa, ya = _pts(rng, mj)
    hp, nh, _keep = _hypc(HYP[fam])
    K = oracle.build_K(fam, xb, yb, xa, ya, HYP[fam])
    parts = [K[:mi, :mj], K[mi:, :mj], K[:mi, mj:], K[mi:, mj:]]
    keep = [_dvec(dev, v) for v in (xb, yb, xa, ya)]
    P = [C.c_void_p(t.data_ptr()) for t in keep]
    i, j = np.indices((mi, mj))
    need, diag = i + doff >= j, i + doff == j
    for lower in (False, True):
        out = []
        for nz in (0.0, noise):
            bufs = [dev.buf(mi, mj, mi + 1, True, None) for _ in range(4)]
            dev.ok("sgpr_gram_pairs_dev", L.family_id(fam), mi, mj, *P, hp, nh, *[b.p for b in bufs], mi + 1, doff, nz,
                   L.G_ALL | (L.G_LOWER if lower else 0), dev.sp)
            out.append([b.get() for b in bufs])
        for q in range(4):
            plain, noisy = out[0][q], out[1][q]
            ref = parts[q] + (abs(noise) * diag if q in (0, 3) else 0.0)
            upd = ~np.isnan(noisy)
            assert np.array_equal(upd, ~np.isnan(plain))
            if lower and q == 2:
                assert not upd.any()
                continue
            if lower and q in (0, 3):
                assert upd[need].all()
            else:
                assert upd.all()
            assert gram_close(np.where(upd, noisy, ref), ref)
            dlt = np.where(upd, noisy - plain, 0.0)
            if q in (0, 3):
                assert np.all(dlt[~diag] == 0.0)
                dd = dlt[diag & upd]
                assert np.all(np.abs(dd - abs(noise)) <= 4 * U * (abs(noise) + np.abs(parts[q][diag & upd]).max(initial=0)))
            else:
                assert np.all(dlt == 0.0)


@pytest.mark.parametrize("fam", "AC")
def test_gram_pairs_dl(dev, oracle, fam):
    """SGPR_G_DLX / SGPR_G_DLY against build_dK (rows = the tile's row points); the oracle's build_dK knows the
    three-parameter families"""
    from sympgpr_amd import _lib as L
    mi, mj = 41, 23
    rng = np.random.default_rng(7 + ord(fam))
    xb, yb = _pts(rng, mi)
    xa, ya = _pts(rng, mj)
    hp, nh, _keep = _hypc(HYP[fam])
    dK = oracle.build_dK(fam, xa, ya, xb, yb, HYP[fam])
    keep = [_dvec(dev, v) for v in (xb, yb, xa, ya)]
    P = [C.c_void_p(t.data_ptr()) for t in keep]
    for w, flag in ((0, L.G_DLX), (1, L.G_DLY)):
        D = dK[w]
        parts = [D[:mi, :mj], D[mi:, :mj], D[:mi, mj:], D[mi:, mj:]]
        bufs = [dev.buf(mi, mj, mi + 2, False, None) for _ in range(4)]
        dev.ok("sgpr_gram_pairs_dev", L.family_id(fam), mi, mj, *P, hp, nh, *[b.p for b in bufs], mi + 2, 0, 0.0,
               L.G_ALL | flag, dev.sp)
        for q, b in enumerate(bufs):
            assert gram_close(b.get(), parts[q]), (w, q)


@pytest.mark.parametrize("fam", "ABCD")
@pytest.mark.parametrize("mi,mj,doff", [(1, 1, 0), (37, 300, -3), (301, 17, 12), (256, 256, 0)])
def test_gram_reg(dev, oracle, fam, mi, mj, doff):
    """the scalar-kernel tile against buildKreg: ragged, ld > mi, diag_off / noise, guards"""
    from sympgpr_amd import _lib as L
    rng = np.random.default_rng(mi * 3 + mj + ord(fam))
    xb, yb = _pts(rng, mi)
    xa, ya = _pts(rng, mj)
    hp, nh, _keep = _hypc(HYP[fam])
    G = oracle.buildKreg(fam, xb, yb, xa, ya, HYP[fam])
    keep = [_dvec(dev, v) for v in (xb, yb, xa, ya)]
    P = [C.c_void_p(t.data_ptr()) for t in keep]
    i, j = np.indices((mi, mj))
    diag = i + doff == j
    noise = 0.3
    for odd in (False, True):
        gp, gn = dev.buf(mi, mj, mi + 3, odd, None), dev.buf(mi, mj, mi + 3, odd, None)
        dev.ok("sgpr_gram_reg_dev", L.family_id(fam), mi, mj, *P, hp, nh, gp.p, gp.ld, doff, 0.0, dev.sp)
        dev.ok("sgpr_gram_reg_dev", L.family_id(fam), mi, mj, *P, hp, nh, gn.p, gn.ld, doff, -noise, dev.sp)
        plain, noisy = gp.get(), gn.get()
        assert gram_close(plain, G)
        dlt = noisy - plain
        assert np.all(dlt[~diag] == 0.0)
        assert np.all(np.abs(dlt[diag] - noise) <= 4 * U * (noise + np.abs(G).max()))


def _nd_hyp(fam, d):
    h = [0.6 + 0.1 * c for c in range(d)] + [1.5 + 0.2 * c for c in range(d)]
    if fam == "D":
        h += [0.8 + 0.1 * c for c in range(d)]
    return h + [0.4]


def _nd_pts(rng, n, d):
    return np.hstack([rng.uniform(0, 2 * np.pi, (n, d)), rng.uniform(-2, 2, (n, d))])


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("fam", "ABCD")
def test_gram_nd(dev, oracle, fam, d):
    """blocks placed apart by rstride / cstride, NaN-padded coordinates (ldxb > mi, ldxa > mj), noise on the
    diagonal of the diagonal blocks only; gaps between the blocks untouched"""
    from sympgpr_amd import _lib as L
    D = 2 * d
    mi, mj, doff, noise = 45, 33, 5, 0.6
    rng = np.random.default_rng(d * 100 + ord(fam))
    Xb, Xa = _nd_pts(rng, mi, d), _nd_pts(rng, mj, d)
    hyp = _nd_hyp(fam, d)
    hp, nh, _keep = _hypc(hyp)
    K = oracle.build_K_nd(fam, Xb, Xa, hyp)
    gxb, gxa = dev.buf(mi, D, mi + 3, True, Xb), dev.buf(mj, D, mj + 2, False, Xa)
    rs, cs = mi + 5, mj + 3
    ld = D * rs + 1
    out = []
    for nz in (0.0, noise):
        gk = dev.buf(ld, D * cs, ld, False, None)
        dev.ok("sgpr_gram_nd_dev", L.family_id(fam), d, mi, mj, gxb.p, gxb.ld, gxa.p, gxa.ld, hp, nh, gk.p, ld, rs, cs,
               doff, nz, dev.sp)
        out.append(gk.get())
    assert gxb.unchanged() and gxa.unchanged()
    i, j = np.indices((mi, mj))
    diag = i + doff == j
    for nz, M in zip((0.0, noise), out):
        written = np.zeros(M.shape, bool)
        for a in range(D):
            for b in range(D):
                blk = M[a * rs:a * rs + mi, b * cs:b * cs + mj]
                ref = K[a * mi:(a + 1) * mi, b * mj:(b + 1) * mj] + (nz * diag if a == b else 0.0)
                assert gram_close(blk, ref), (nz, a, b)
                written[a * rs:a * rs + mi, b * cs:b * cs + mj] = True
        assert np.all(M[~written].view(np.uint64) == SENT_BITS)
    dlt = out[1] - out[0]
    for a in range(D):
        for b in range(D):
            blk = dlt[a * rs:a * rs + mi, b * cs:b * cs + mj]
            if a == b:
                assert np.all(blk[~diag] == 0.0)
                assert np.all(np.abs(blk[diag] - noise) <= 4 * U * (noise + np.abs(K).max()))
            else:
                assert np.all(blk == 0.0)


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("fam", "AD")
def test_gram_nd_sel(dev, oracle, fam, d):
    """only the blocks whose row and column offsets are >= 0 are written, each where its offsets say"""
    from sympgpr_amd import _lib as L
    D = 2 * d
    mi, mj = 40, 31
    rng = np.random.default_rng(d * 7 + ord(fam))
    Xb, Xa = _nd_pts(rng, mi, d), _nd_pts(rng, mj, d)
    hyp = _nd_hyp(fam, d)
    hp, nh, _keep = _hypc(hyp)
    K = oracle.build_K_nd(fam, Xb, Xa, hyp)
    gxb, gxa = dev.buf(mi, D, mi + 1, False, Xb), dev.buf(mj, D, mj + 4, True, Xa)
    # rows: blocks in reverse order, one left out; columns: every other block, one left out
    roff = [(D - 1 - a) * (mi + 2) + 1 for a in range(D)]
    roff[D // 2] = -1
    coff = [b * (mj + 1) for b in range(D)]
    coff[0] = -1
    ld = D * (mi + 2) + 3
    gk = dev.buf(ld, D * (mj + 1), ld, True, None)
    ro, co = (C.c_long * D)(*roff), (C.c_long * D)(*coff)
    dev.ok("sgpr_gram_nd_sel_dev", L.family_id(fam), d, mi, mj, gxb.p, gxb.ld, gxa.p, gxa.ld, hp, nh, gk.p, ld, ro, co,
           dev.sp)
    M = gk.get()
    written = np.zeros(M.shape, bool)
    for a in range(D):
        for b in range(D):
            if roff[a] < 0 or coff[b] < 0:
                continue
            blk = M[roff[a]:roff[a] + mi, coff[b]:coff[b] + mj]
            assert gram_close(blk, K[a * mi:(a + 1) * mi, b * mj:(b + 1) * mj]), (a, b)
            written[roff[a]:roff[a] + mi, coff[b]:coff[b] + mj] = True
    assert np.all(M[~written].view(np.uint64) == SENT_BITS)


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("fam", "ABCD")
def test_predict_nd(dev, oracle, fam, d):
    """K*(Xt, Xtr) alpha with padded leading dimensions, against build_K_nd @ alpha in long double"""
    from sympgpr_amd import _lib as L
    D = 2 * d
    m, n0 = 57, 300
    rng = np.random.default_rng(d + ord(fam))
    Xt, Xtr = _nd_pts(rng, m, d), _nd_pts(rng, n0, d)
    hyp = _nd_hyp(fam, d)
    hp, nh, _keep = _hypc(hyp)
    alpha = rng.standard_normal(D * n0)
    K = oracle.build_K_nd(fam, Xt, Xtr, hyp)
    ref = (K.astype(np.longdouble) @ alpha.astype(np.longdouble)).astype(np.float64)
    gxt, gxr = dev.buf(m, D, m + 3, True, Xt), dev.buf(n0, D, n0 + 1, False, Xtr)
    ga = dev.buf(D * n0, 1, D * n0, False, alpha[:, None])
    go = dev.buf(m, D, m, False, None)
    dev.ok("sgpr_predict_nd_dev", L.family_id(fam), d, m, gxt.p, gxt.ld, n0, gxr.p, gxr.ld, hp, nh, ga.p, go.p, dev.sp)
    got = go.get().reshape(-1, order="F")     # out (m x D) column-major = the D m rows of K*
    bound = GRAM_RTOL * np.abs(K).max() * np.abs(alpha).sum() + 2 * (D * n0 + 2) * U * (np.abs(K) @ np.abs(alpha))
    assert np.all(np.abs(got - ref) <= bound), float((np.abs(got - ref) / bound).max())
    assert gxt.unchanged() and gxr.unchanged() and ga.unchanged()
