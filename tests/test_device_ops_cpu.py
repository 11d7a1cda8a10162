"""Argument checks of the device-pointer primitives (the *_dev entries of include/sympgpr_hip.h).

Every rule is answered with SGPR_E_ARG before any device is looked for, and sgpr_last_error() names the entry
point, so these run on a machine without a GPU.  There, well-formed calls still return SGPR_E_NODEVICE.  With a
device present, a call that would pass a null pointer is not made: should a check go missing it would reach a
kernel.  Every other bad call gets real device buffers, large enough that even a call whose check had gone missing
would stay in bounds."""
import ctypes as C

import pytest

from sympgpr_amd import _lib as L

N = 256          # order / extents of the calls below
BUF = 4 * N * N  # doubles per buffer: covers every call below at its largest leading dimension


@pytest.fixture(scope="module")
def env():
    lib = L.load_library()
    has_dev = lib.sgpr_device_count() > 0
    if has_dev:
        import torch
        bufs = [torch.zeros(BUF, dtype=torch.float64, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        ptrs = [C.c_void_p(b.data_ptr()) for b in bufs]
    else:
        bufs = [(C.c_double * 16)() for _ in range(4)]
        ptrs = [C.cast(b, C.c_void_p) for b in bufs]
    return lib, has_dev, ptrs, bufs


def _hyp(d=1):
    h = (C.c_double * (2 * d + 1))(*([0.5] * (2 * d) + [1.0]))
    return h, 2 * d + 1


# (entry, uses a null pointer, call) -- every call breaks exactly one rule of its entry
def _bad_calls(p):
    A, B, Cm, W = p
    nul = None
    big = L.load_library().sgpr_potrf_workspace(N)
    h1, nh1 = _hyp(1)
    off = (C.c_long * 2)(0, N)
    return [
        # triangular solves with the rows of B as right-hand sides
        ("sgpr_trsm_rlt_dev", False, lambda l: l.sgpr_trsm_rlt_dev(-1, N, A, N, B, N, W, nul)),
        ("sgpr_trsm_rlt_dev", False, lambda l: l.sgpr_trsm_rlt_dev(N, -1, A, N, B, N, W, nul)),
        ("sgpr_trsm_rlt_dev", False, lambda l: l.sgpr_trsm_rlt_dev(N, N, A, N - 1, B, N, W, nul)),
        ("sgpr_trsm_rlt_dev", False, lambda l: l.sgpr_trsm_rlt_dev(N, N, A, N, B, N - 1, W, nul)),
        ("sgpr_trsm_rlt_dev", True, lambda l: l.sgpr_trsm_rlt_dev(N, N, nul, N, B, N, W, nul)),
        ("sgpr_trsm_rlt_dev", True, lambda l: l.sgpr_trsm_rlt_dev(N, N, A, N, nul, N, W, nul)),
        ("sgpr_trsm_rlt_dev", True, lambda l: l.sgpr_trsm_rlt_dev(N, N, A, N, B, N, nul, nul)),
        ("sgpr_trsm_rl_dev", False, lambda l: l.sgpr_trsm_rl_dev(-1, N, A, N, B, N, W, nul)),
        ("sgpr_trsm_rl_dev", False, lambda l: l.sgpr_trsm_rl_dev(N, -1, A, N, B, N, W, nul)),
        ("sgpr_trsm_rl_dev", False, lambda l: l.sgpr_trsm_rl_dev(N, N, A, N - 1, B, N, W, nul)),
        ("sgpr_trsm_rl_dev", False, lambda l: l.sgpr_trsm_rl_dev(N, N, A, N, B, N - 1, W, nul)),
        ("sgpr_trsm_rl_dev", True, lambda l: l.sgpr_trsm_rl_dev(N, N, nul, N, B, N, W, nul)),
        ("sgpr_trsm_rl_dev", True, lambda l: l.sgpr_trsm_rl_dev(N, N, A, N, nul, N, W, nul)),
        ("sgpr_trsm_rl_dev", True, lambda l: l.sgpr_trsm_rl_dev(N, N, A, N, B, N, nul, nul)),
        # vector solves
        ("sgpr_trsv_dev", False, lambda l: l.sgpr_trsv_dev(-1, A, N, W, B, 0, nul)),
        ("sgpr_trsv_dev", False, lambda l: l.sgpr_trsv_dev(N, A, N - 1, W, B, 1, nul)),
        ("sgpr_trsv_dev", True, lambda l: l.sgpr_trsv_dev(N, nul, N, W, B, 0, nul)),
        ("sgpr_trsv_dev", True, lambda l: l.sgpr_trsv_dev(N, A, N, nul, B, 0, nul)),
        ("sgpr_trsv_dev", True, lambda l: l.sgpr_trsv_dev(N, A, N, W, nul, 0, nul)),
        ("sgpr_potrs_vec_dev", False, lambda l: l.sgpr_potrs_vec_dev(-1, A, N, W, B, nul)),
        ("sgpr_potrs_vec_dev", False, lambda l: l.sgpr_potrs_vec_dev(N, A, N - 1, W, B, nul)),
        ("sgpr_potrs_vec_dev", True, lambda l: l.sgpr_potrs_vec_dev(N, nul, N, W, B, nul)),
        ("sgpr_potrs_vec_dev", True, lambda l: l.sgpr_potrs_vec_dev(N, A, N, nul, B, nul)),
        ("sgpr_potrs_vec_dev", True, lambda l: l.sgpr_potrs_vec_dev(N, A, N, W, nul, nul)),
        ("sgpr_solve_status_dev", False, lambda l: l.sgpr_solve_status_dev(-1, A, N, W, nul)),
        ("sgpr_solve_status_dev", False, lambda l: l.sgpr_solve_status_dev(N, A, N - 1, W, nul)),
        ("sgpr_solve_status_dev", True, lambda l: l.sgpr_solve_status_dev(N, nul, N, W, nul)),
        ("sgpr_solve_status_dev", True, lambda l: l.sgpr_solve_status_dev(N, A, N, nul, nul)),
        # products
        ("sgpr_gemm_nt_dev", False, lambda l: l.sgpr_gemm_nt_dev(-1, N, N, 1.0, A, N, B, N, 0.0, Cm, N, 0, 0, nul)),
        ("sgpr_gemm_nt_dev", False, lambda l: l.sgpr_gemm_nt_dev(N, N, -1, 1.0, A, N, B, N, 0.0, Cm, N, 0, 0, nul)),
        ("sgpr_gemm_nt_dev", False, lambda l: l.sgpr_gemm_nt_dev(N, N, N, 1.0, A, N - 1, B, N, 0.0, Cm, N, 0, 0, nul)),
        ("sgpr_gemm_nt_dev", False, lambda l: l.sgpr_gemm_nt_dev(N, N, N, 1.0, A, N, B, N - 1, 0.0, Cm, N, 0, 0, nul)),
        ("sgpr_gemm_nt_dev", False, lambda l: l.sgpr_gemm_nt_dev(N, N, N, 1.0, A, N, B, N, 0.0, Cm, N - 1, 1, 3, nul)),
        ("sgpr_gemm_nn_dev", False, lambda l: l.sgpr_gemm_nn_dev(N, -1, N, 1.0, A, N, B, N, 0.0, Cm, N, nul)),
        ("sgpr_gemm_nn_dev", False, lambda l: l.sgpr_gemm_nn_dev(N, N, N, 1.0, A, N - 1, B, N, 0.0, Cm, N, nul)),
        # NN: B is (k x n), so ldb >= k -- here k = 2N with ldb = 2N - 1 >= n
        ("sgpr_gemm_nn_dev", False, lambda l: l.sgpr_gemm_nn_dev(N, N, 2 * N, 1.0, A, N, B, 2 * N - 1, 0.0, Cm, N, nul)),
        ("sgpr_gemm_nn_dev", False, lambda l: l.sgpr_gemm_nn_dev(N, N, N, 1.0, A, N, B, N, 0.0, Cm, N - 1, nul)),
        ("sgpr_gemm_nt_bc_dev", False,
         lambda l: l.sgpr_gemm_nt_bc_dev(N, N, N, 1.0, A, N, B, N, 0.0, Cm, N, 0, 1, 0, 1, 0, nul)),
        ("sgpr_gemm_nt_bc_dev", False,
         lambda l: l.sgpr_gemm_nt_bc_dev(N, N, N, 1.0, A, N, B, N, 0.0, Cm, N, 64, 0, 0, 1, 0, nul)),
        ("sgpr_gemm_nt_bc_dev", False,
         lambda l: l.sgpr_gemm_nt_bc_dev(N, N, N, 1.0, A, N, B, N, 0.0, Cm, N, 64, 1, 0, 0, 0, nul)),
        ("sgpr_gemm_nt_bc_dev", False,
         lambda l: l.sgpr_gemm_nt_bc_dev(N, N, N, 1.0, A, N, B, N - 1, 0.0, Cm, N, 64, 2, 1, 2, 0, nul)),
        ("sgpr_gemm_nt_bc_dev", False,
         lambda l: l.sgpr_gemm_nt_bc_dev(N, N, -2, 1.0, A, N, B, N, 0.0, Cm, N, 64, 2, 1, 2, 0, nul)),
        ("sgpr_gemv_sub_dev", False, lambda l: l.sgpr_gemv_sub_dev(0, -1, N, A, N, B, Cm, nul)),
        ("sgpr_gemv_sub_dev", False, lambda l: l.sgpr_gemv_sub_dev(1, N, N, A, N - 1, B, Cm, nul)),
        ("sgpr_gemv_sub_dev", True, lambda l: l.sgpr_gemv_sub_dev(0, N, N, A, N, nul, Cm, nul)),
        # copies
        ("sgpr_copy_blocks_dev", False, lambda l: l.sgpr_copy_blocks_dev(N, 4, 2, A, N - 1, N * 4, B, N, N * 4, nul)),
        ("sgpr_copy_blocks_dev", False, lambda l: l.sgpr_copy_blocks_dev(N, 4, 2, A, N, N * 4, B, N - 1, N * 4, nul)),
        ("sgpr_copy_blocks_dev", False, lambda l: l.sgpr_copy_blocks_dev(-1, 4, 2, A, N, N * 4, B, N, N * 4, nul)),
        ("sgpr_copy_blocks_dev", False, lambda l: l.sgpr_copy_blocks_dev(1, 1, 65536, A, 1, 0, B, 1, 0, nul)),
        ("sgpr_copy_blocks_dev", True, lambda l: l.sgpr_copy_blocks_dev(N, 4, 2, nul, N, N * 4, B, N, N * 4, nul)),
        # factorisation
        ("sgpr_potrf_dev", False, lambda l: l.sgpr_potrf_dev(-1, A, N, W, big, Cm, nul)),
        ("sgpr_potrf_dev", False, lambda l: l.sgpr_potrf_dev(N, A, N - 1, W, big, Cm, nul)),
        ("sgpr_potrf_dev", False, lambda l: l.sgpr_potrf_dev(N, A, N, W, big - 8, Cm, nul)),
        ("sgpr_potrf_dev", True, lambda l: l.sgpr_potrf_dev(N, A, N, W, big, nul, nul)),
        # Gram builds for d pairs per point: output and coordinate leading dimensions
        ("sgpr_gram_nd_dev", False,
         lambda l: l.sgpr_gram_nd_dev(0, 1, 64, 32, A, 64, B, 32, h1, nh1, Cm, 63, 64, 32, 0, 0.0, nul)),
        ("sgpr_gram_nd_dev", False,
         lambda l: l.sgpr_gram_nd_dev(0, 1, 64, 32, A, 63, B, 32, h1, nh1, Cm, 128, 64, 32, 0, 0.0, nul)),
        ("sgpr_gram_nd_dev", False,
         lambda l: l.sgpr_gram_nd_dev(0, 1, 64, 32, A, 64, B, 31, h1, nh1, Cm, 128, 64, 32, 0, 0.0, nul)),
        ("sgpr_gram_nd_sel_dev", False,
         lambda l: l.sgpr_gram_nd_sel_dev(0, 1, 64, 32, A, 64, B, 32, h1, nh1, Cm, 63, off, off, nul)),
        ("sgpr_gram_nd_sel_dev", False,
         lambda l: l.sgpr_gram_nd_sel_dev(0, 1, 64, 32, A, 63, B, 32, h1, nh1, Cm, 128, off, off, nul)),
        ("sgpr_gram_nd_sel_dev", False,
         lambda l: l.sgpr_gram_nd_sel_dev(0, 1, 64, 32, A, 64, B, 31, h1, nh1, Cm, 128, off, off, nul)),
        ("sgpr_predict_nd_dev", False,
         lambda l: l.sgpr_predict_nd_dev(0, 1, 64, A, 63, 32, B, 32, h1, nh1, W, Cm, nul)),
        ("sgpr_predict_nd_dev", False,
         lambda l: l.sgpr_predict_nd_dev(0, 1, 64, A, 64, 32, B, 31, h1, nh1, W, Cm, nul)),
    ]


def _good_calls(p):
    A, B, Cm, W = p
    nul = None
    big = L.load_library().sgpr_potrf_workspace(N)
    h1, nh1 = _hyp(1)
    off = (C.c_long * 2)(0, N)
    return [
        lambda l: l.sgpr_trsm_rlt_dev(N, N, A, N, B, N, W, nul),
        lambda l: l.sgpr_trsm_rl_dev(N, N, A, N, B, N, W, nul),
        lambda l: l.sgpr_trsv_dev(N, A, N, W, B, 0, nul),
        lambda l: l.sgpr_potrs_vec_dev(N, A, N, W, B, nul),
        lambda l: l.sgpr_solve_status_dev(N, A, N, W, nul),
        lambda l: l.sgpr_gemm_nt_dev(N, N, N, 1.0, A, N, B, N, 0.0, Cm, N, 1, 3, nul),
        lambda l: l.sgpr_gemm_nn_dev(N, N, 2 * N, 1.0, A, N, B, 2 * N, 0.0, Cm, N, nul),
        lambda l: l.sgpr_gemm_nt_bc_dev(N, N, N, 1.0, A, N, B, N, 0.0, Cm, N, 64, 2, 1, 2, 0, nul),
        lambda l: l.sgpr_gemv_sub_dev(1, N, N, A, N, B, Cm, nul),
        lambda l: l.sgpr_copy_blocks_dev(N, 4, 2, A, N, N * 4, B, N, N * 4, nul),
        lambda l: l.sgpr_copy_blocks_dev(0, 4, 70000, A, N, N * 4, B, N, N * 4, nul),
        lambda l: l.sgpr_potrf_dev(N, A, N, W, big, Cm, nul),
        lambda l: l.sgpr_gram_nd_dev(0, 1, 64, 32, A, 64, B, 32, h1, nh1, Cm, 128, 64, 32, 0, 0.0, nul),
        lambda l: l.sgpr_gram_nd_sel_dev(0, 1, 64, 32, A, 64, B, 32, h1, nh1, Cm, 128, off, off, nul),
        lambda l: l.sgpr_predict_nd_dev(0, 1, 64, A, 64, 32, B, 32, h1, nh1, W, Cm, nul),
    ]


def test_argument_errors_name_the_entry(env):
    """each rule: E_ARG, and the message starts with the entry point's name"""
    lib, has_dev, ptrs, _ = env
    ran = 0
    for entry, uses_null, call in _bad_calls(ptrs):
        if uses_null and has_dev:
            continue
        rc = call(lib)
        msg = lib.sgpr_last_error().decode()
        assert rc == L.E_ARG, (entry, rc, msg)
        assert msg.startswith(entry + ":"), (entry, msg)
        ran += 1
    assert ran >= (45 if has_dev else 60)
    if has_dev:
        import torch
        torch.cuda.synchronize()   # nothing was enqueued: a missing check would show up here at the latest


def test_valid_calls_reach_the_device_check(env):
    """without a device, well-formed calls get past the argument checks and return E_NODEVICE"""
    lib, has_dev, ptrs, _ = env
    if has_dev:
        # on a GPU machine these calls would run on zero-filled buffers; the GPU suite covers them
        assert lib.sgpr_device_count() > 0
        return
    for call in _good_calls(ptrs):
        rc = call(lib)
        assert rc == L.E_NODEVICE, (rc, lib.sgpr_last_error())
