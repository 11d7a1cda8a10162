"""The arena layout of the batched fits (sympgpr_amd/csrc/batch.hip: batch_layout, host arithmetic) against the formulas, restated
here independently.  Every batched entry cuts one device allocation and one pinned block by these offsets, so a wrong one is an
out-of-bounds access on the device; this check needs no GPU (sgpr_probe_batch_layout makes no device call).

Only the two struct sizes (KConst, NdConst) and the panel's flag bytes for a chunk are taken from the probe; the rest is computed
from the shape.  For every shape: each region starts on a 256-byte boundary, the regions are in order and disjoint, each is at
least as large as what is stored there, and the chunk and the three totals equal the restated values."""
import ctypes as C

import pytest

from sympgpr_amd import _lib as L

LEAF, BMAX, PER_WG = 128, 256, 98816          # leaf order, largest one-launch order, scratch doubles per workgroup of a plain fit
GT, GCJ, GPART = 256, 64, 8                   # mid gradient: rows / column points per workgroup, doubles per partial
FIT, GRAD, LOO, LOOGRAD = 0, 1, 2, 3


def up256(b):
    return (b + 255) // 256 * 256


def probe(path, mode, d, reg, nbatch, npts, nhyp):
    out = (C.c_ulonglong * 24)()
    L.check(L.load_probe_library().sgpr_probe_batch_layout(path, mode, d, reg, nbatch, npts, nhyp, out))
    v = [int(t) for t in out]
    names = ("chunk nacc o_x o_y o_z o_kc o_no in_bytes o_al o_nll o_info out_bytes o_A o_inv o_fl o_fl2 o_r o_pub o_st o_part "
             "scr_bytes kconst ndconst flag_bytes").split()
    return dict(zip(names, v))


def regions(starts, needs, total):
    """(start, need) in order -> the checks of one block"""
    for s in starts:
        assert s % 256 == 0
    ends = list(starts[1:]) + [total]
    for s, e, need in zip(starts, ends, needs):
        assert s <= e                    # in order
        assert e - s >= need             # disjoint from the next one, and large enough
    assert total % 256 == 0


def check(path, mode, d, reg, nbatch, npts, nhyp, cap=0):
    got = probe(path, mode, d, reg, nbatch, npts, nhyp)
    n = 2 * d * npts if d else (npts if reg else 2 * npts)
    xb = 2 * d * npts * 8 if d else npts * 8
    yb = 0 if d else npts * 8
    const = got["ndconst"] if d else got["kconst"]
    kinv = mode != FIT
    if path == 0:
        chunk = nbatch
        nacc = {FIT: 0, GRAD: nhyp + 1, LOO: 2, LOOGRAD: nhyp + 3}[mode]
    else:
        npad = -(-n // LEAF) * LEAF
        W = npad // LEAF
        nimg = 2 if kinv else 1
        img = npad * npad * 8
        chunk = min(nbatch, max(-(-256 // W), (2 << 30) // (nimg * img)), 16384)
        if kinv and cap > 0:
            chunk = min(chunk, cap)
        nacc = {FIT: 0, GRAD: nhyp + 1, LOO: 2}[mode]
    c = chunk
    assert got["chunk"] == chunk and got["nacc"] == nacc
    # input block: x | y | z | consts | noise
    needs_in = [c * xb, c * yb, c * n * 8, c * const, c * 8]
    in_bytes = sum(up256(b) for b in needs_in)
    regions([got[k] for k in ("o_x", "o_y", "o_z", "o_kc", "o_no")], needs_in, got["in_bytes"])
    assert got["o_x"] == 0 and got["in_bytes"] == in_bytes
    # output block: alpha | nll + sums | info
    needs_out = [c * n * 8, c * (1 + nacc) * 8, c * 4]
    out_bytes = sum(up256(b) for b in needs_out)
    regions([got[k] for k in ("o_al", "o_nll", "o_info")], needs_out, got["out_bytes"])
    assert got["o_al"] == 0 and got["out_bytes"] == out_bytes
    if path == 0:
        per_wg = PER_WG + (BMAX * BMAX if mode != FIT else 0) + (BMAX * BMAX if mode == LOOGRAD else 0)
        assert got["scr_bytes"] == min(nbatch, 1024) * per_wg * 8
        assert got["flag_bytes"] == 0
        return
    flag = got["flag_bytes"]
    assert flag >= 4 * c                 # at least one word per problem
    gnwg = -(-n // GT) * -(-npts // GCJ)
    lnwg = -(-npts // GT)
    part = c * gnwg * GPART * 8 if mode == GRAD else c * lnwg * 2 * 8 if mode == LOO else 0
    # images (L, then U directly behind it) | leaf inverses | flags of panel 1 | of panel 2 | r | pub | state | partials
    needs_scr = [nimg * c * img, c * W * LEAF * LEAF * 8, flag, flag, c * npad * 8, 2 * c * npad * 8, c * 8 * 4, part]
    scr_bytes = nimg * up256(c * img) + sum(up256(b) for b in needs_scr[1:])
    regions([got[k] for k in ("o_A", "o_inv", "o_fl", "o_fl2", "o_r", "o_pub", "o_st", "o_part")], needs_scr, got["scr_bytes"])
    assert got["o_A"] == 0 and got["scr_bytes"] == scr_bytes
    assert (c * img) % 256 == 0          # the U images start at image c of the L images


SMALL = [(npts, reg) for npts, reg in ((1, 0), (40, 0), (128, 0), (129, 1))]       # n = 2, 80, 256; reg at n = 129


@pytest.mark.parametrize("mode", [FIT, GRAD, LOO, LOOGRAD])
@pytest.mark.parametrize("nbatch", [1, 1024, 1500])
@pytest.mark.parametrize("npts,reg", SMALL)
def test_small_path(npts, reg, nbatch, mode):
    for nhyp in (3, 4):
        check(0, mode, 0, reg, nbatch, npts, nhyp)


@pytest.mark.parametrize("d,npts", [(2, 64), (3, 42)])
@pytest.mark.parametrize("nbatch", [1, 1024, 1500])
def test_small_path_pairs(d, npts, nbatch):
    check(0, FIT, d, 0, nbatch, npts, 3 * d + 1)


@pytest.fixture(params=[0, 2])
def chunk_cap(request):
    """the batch_gradmid_chunk tunable at 0 (none, the built-in value) and 2; back to 0 afterwards"""
    tune = L.load_probe_library().sgpr_probe_tune
    L.check(tune(b"batch_gradmid_chunk", float(request.param)))
    yield request.param
    L.check(tune(b"batch_gradmid_chunk", 0.0))


@pytest.mark.parametrize("mode", [FIT, GRAD, LOO])
@pytest.mark.parametrize("nbatch", [1, 3, 70])
@pytest.mark.parametrize("npts,reg", [(129, 0), (320, 0), (1024, 0), (257, 1)])       # n = 258, 640, 2048; reg at n = 257
def test_mid_path(npts, reg, nbatch, mode, chunk_cap):
    for nhyp in (3, 4):
        check(1, mode, 0, reg, nbatch, npts, nhyp, chunk_cap)


@pytest.mark.parametrize("d,npts", [(3, 43), (2, 512)])
@pytest.mark.parametrize("nbatch", [1, 3, 70])
def test_mid_path_pairs(d, npts, nbatch, chunk_cap):
    check(1, FIT, d, 0, nbatch, npts, 2 * d + 1, chunk_cap)


def test_probe_rejects_shapes_outside_a_path():
    out = (C.c_ulonglong * 24)()
    lib = L.load_probe_library()
    assert lib.sgpr_probe_batch_layout(0, FIT, 0, 0, 4, 129, 3, out) != 0       # order 258 on the one-launch path
    assert lib.sgpr_probe_batch_layout(1, FIT, 0, 0, 4, 128, 3, out) != 0       # order 256 on the mid path
    assert lib.sgpr_probe_batch_layout(1, LOOGRAD, 0, 0, 4, 200, 3, out) != 0   # no loo gradient above order 256
