// capi_util.h -- what more than one of the C API units (capi.hip, capi_fit.hip, capi_dev.hip) needs: host code only
#pragma once
#include "common.h"

namespace sgpr {

int need_device();   // capi.hip: SGPR_E_NODEVICE (and the message) when there is no HIP device

// small RAII device buffer for the host-pointer calls
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) { SGPR_HIP(hipMalloc(&p, bytes ? bytes : 8)); return 0; }
    template <typename T> T *as() { return static_cast<T *>(p); }
};

inline int upload(DevBuf &b, const double *h, size_t n, hipStream_t st)
{
    int rc = b.alloc(n * sizeof(double));
    if (rc) return rc;
    if (n) SGPR_HIP(hipMemcpyAsync(b.p, h, n * sizeof(double), hipMemcpyHostToDevice, st));
    return 0;
}

// column-major (rows x cols) copies between host and device on `st`; extents and leading dimensions in doubles
inline int copy_2d(double *dst, size_t ldd, const double *src, size_t lds, size_t rows, size_t cols, hipMemcpyKind kind,
                   hipStream_t st)
{
    SGPR_HIP(hipMemcpy2DAsync(dst, ldd * sizeof(double), src, lds * sizeof(double), rows * sizeof(double), cols, kind, st));
    return 0;
}
inline int copy_in(void *dev, size_t ldd, const double *host, size_t ldh, size_t rows, size_t cols, hipStream_t st)
{
    return copy_2d(static_cast<double *>(dev), ldd, host, ldh, rows, cols, hipMemcpyHostToDevice, st);
}
inline int copy_out(double *host, size_t ldh, const void *dev, size_t ldd, size_t rows, size_t cols, hipStream_t st)
{
    return copy_2d(host, ldh, static_cast<const double *>(dev), ldd, rows, cols, hipMemcpyDeviceToHost, st);
}

// Factor (factor() enqueues one attempt on st and leaves its status in *dinfo), wait, read *info.  When the task-queue driver
// gave up (a hand-off between its persistent kernels ran into its time limit) the matrix is half overwritten: restore() puts
// it back and the look-ahead driver, which this device uses from now on, factors it.  Once: a second give-up is an error.
template <typename Factor, typename Restore>
int factor_with_retry(Factor factor, const int *dinfo, int *info, hipStream_t st, Restore restore)
{
    for (int attempt = 0;; ++attempt) {
        int rc = factor();
        if (rc) return rc;
        SGPR_HIP(hipMemcpyAsync(info, dinfo, sizeof(int), hipMemcpyDeviceToHost, st));
        SGPR_HIP(hipStreamSynchronize(st));
        if (*info != POTRF_HANDOFF_TIMEOUT || attempt || !potrf_queue_mark_failed(st)) return 0;
        if ((rc = restore())) return rc;
    }
}

// a block of right-hand sides goes to the matrix cores (potrs_mat, which needs potrs_mat_scratch bytes), fewer go one by one
inline bool potrs_blocked(int n, int nrhs, const double *L, size_t ldl)
{
    return nrhs >= 8 || potrs_mat_uses_strips(n, nrhs, L, ldl);
}

// B (n x nrhs) := L^-T L^-1 B by the path potrs_blocked names (scratch is read on the block path only); waits for the solves.
// `solved`, if given, is recorded behind the last solve: ahead of the block path's status wait, after the per-column ones.
inline int potrs_dispatch(int n, const double *L, size_t ldl, void *work, double *B, size_t ldb, int nrhs, double *scratch,
                          hipStream_t st, hipEvent_t solved = nullptr)
{
    int rc;
    if (potrs_blocked(n, nrhs, L, ldl)) {
        if ((rc = potrs_mat(n, L, ldl, work, B, ldb, nrhs, scratch, st))) return rc;
        if (solved) SGPR_HIP(hipEventRecord(solved, st));
        return solve_status(n, L, ldl, work, st);
    }
    for (int r = 0; r < nrhs; ++r) {
        if ((rc = potrs_vec(n, L, ldl, work, B + (size_t)r * ldb, st))) return rc;
        if ((rc = solve_status(n, L, ldl, work, st))) return rc;   // the next solve reuses the hand-off words
    }
    if (solved) SGPR_HIP(hipEventRecord(solved, st));
    return 0;
}

}  // namespace sgpr
