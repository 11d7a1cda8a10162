// capi_util.h -- what more than one of the C API units (capi.hip, capi_fit.hip, capi_dev.hip) needs: host code only.  Device
// buffers and copies (DevBuf, upload, copy_2d); the factorisation's one retry; the choice of a solve path (potrs_blocked,
// potrs_dispatch); and the d-pair map entries of a fit handle and of the _host calls: their argument checks, their model
// (MapModel) and the device traffic of one call (applymap_nd_io, periodic_nd_io).
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

// What sgpr_fit_applymap_nd and sgpr_applymap_nd_host share.  The checks need no device: an argument error is SGPR_E_ARG on any
// machine.  The shape of the call (both entries) ...
inline int applymap_nd_call_check(const char *entry, int mode, int nm, int ntest, const double *Q0, size_t ldq, const double *P0,
                                  size_t ldp, const double *qmap, const double *pmap)
{
    auto E = [&](const char *what) { set_error(std::string(entry) + ": " + what); return SGPR_E_ARG; };
    if (mode & ~(SGPR_MAP_WRAP_Q | SGPR_MAP_EXPLICIT)) return E("unknown mode bit (only SGPR_MAP_WRAP_Q and SGPR_MAP_EXPLICIT)");
    if (nm < 1) return E("nm < 1");
    if (ntest < 0) return E("ntest < 0");
    if (!Q0 || !P0 || !qmap || !pmap) return E("null Q0, P0, qmap or pmap");
    if (ldq < (size_t)ntest || ldp < (size_t)ntest) return E("leading dimension of Q0 or P0 smaller than ntest");
    return 0;
}
// ... and the description of the kernel, which a fit handle has checked when it was created
inline int applymap_nd_kernel_check(const char *entry, int family, int d, const double *hyp, int nhyp)
{
    auto E = [&](const char *what) { set_error(std::string(entry) + ": " + what); return SGPR_E_ARG; };
    if (family < SGPR_FAM_A || family > SGPR_FAM_USER) return E("unknown kernel family");
    if (d < 1 || d > 3) return E("d must be 1, 2 or 3");
    if (!hyp || nhyp != (family_has_p(family) ? 3 * d + 1 : 2 * d + 1))
        return E("hyp must hold (lq_1..lq_d, lP_1..lP_d, sig) -- (lq.., lP.., p_1..p_d, sig) for family D");
    return 0;
}

// ... and what the two tangent entries (sgpr_fit_applymap_nd_tangent, sgpr_applymap_nd_tangent_host) ask on top of it
inline int applymap_nd_tangent_check(const char *entry, int family, int mode, int nm, const double *lyap)
{
    auto E = [&](const char *what) { set_error(std::string(entry) + ": " + what); return SGPR_E_ARG; };
    if ((mode & SGPR_MAP_EXPLICIT) && !family_is_sum(family))
        return E("SGPR_MAP_EXPLICIT has a tangent map for the sum kernels only (family B, or a USER sum kernel)");
    if (lyap && nm < 2) return E("lyap needs nm >= 2");
    return 0;
}

// ... and what the two backward entries (sgpr_fit_applymap_nd_inverse, sgpr_applymap_nd_inverse_host) ask on top of it: the
// explicit product-family map P = p - G_q(q, p) has another inverse (a second solve, in p), and the sum kernels' explicit and
// implicit maps coincide, so mode 0 inverts them already -- the bit is refused for every family
inline int applymap_nd_inverse_check(const char *entry, int mode)
{
    if (mode & SGPR_MAP_EXPLICIT) {
        set_error(std::string(entry) + ": SGPR_MAP_EXPLICIT has no backward step (only the implicit map is inverted; for the sum kernels "
                                       "the two coincide)");
        return SGPR_E_ARG;
    }
    return 0;
}

// the host arrays a tangent entry fills, each or null: jac [nm - 1][ntest][2d][2d], mono [ntest][2d][2d], lyap [ntest][2d]
struct MapTangentOut {
    double *jac, *mono, *lyap;
};

// The model of a d-pair map as map_nd.hip takes it: the kernel (hyp = (lq.., lP.., [p..,] sig) on the host), the device-resident
// training points X (n0 x 2d, leading dimension ldx) and alpha, and the stream of the call.  A fit handle's comes from
// fit_map_model (capi_fit.hip), a *_host entry's from with_host_map_model (capi.hip).
struct MapModel {
    int family, d, n0;
    const double *X;
    size_t ldx;
    const double *hyp;
    int nhyp;
    const double *alpha;
    hipStream_t stream;
};

// uploads the start points, runs applymap_nd on the model, brings the orbits back and waits; with `tan` the launch is
// applymap_nd_tangent and its outputs come back too; MAP_BACKWARD runs applymap_nd_inverse (no tangent)
enum MapDirection { MAP_FORWARD, MAP_BACKWARD };
inline int applymap_nd_io(const MapModel &m, int mode, int nm, int ntest, const double *Q0, size_t ldq, const double *P0, size_t ldp,
                          double *qmap, double *pmap, int *iters, const MapTangentOut *tan = nullptr, MapDirection dir = MAP_FORWARD)
{
    const int d = m.d;
    hipStream_t st = m.stream;
    int rc;
    DevBuf q0, p0, qm, pm, it, dj, dm, dl;
    const size_t nt = (size_t)ntest, out_bytes = (size_t)nm * nt * d * sizeof(double), it_bytes = (size_t)(nm - 1) * nt * sizeof(int);
    const size_t DD = (size_t)4 * d * d, mono_bytes = nt * DD * sizeof(double), jac_bytes = (size_t)(nm - 1) * mono_bytes;
    const size_t lyap_bytes = nt * 2 * d * sizeof(double);
    if ((rc = q0.alloc(nt * d * sizeof(double))) || (rc = p0.alloc(nt * d * sizeof(double))) || (rc = qm.alloc(out_bytes)) ||
        (rc = pm.alloc(out_bytes)) || (iters && (rc = it.alloc(it_bytes))))
        return rc;
    if (tan && ((tan->jac && (rc = dj.alloc(jac_bytes))) || (tan->mono && (rc = dm.alloc(mono_bytes))) ||
                (tan->lyap && (rc = dl.alloc(lyap_bytes)))))
        return rc;
    if ((rc = copy_in(q0.p, nt, Q0, ldq, nt, d, st)) || (rc = copy_in(p0.p, nt, P0, ldp, nt, d, st))) return rc;
    double *q = q0.as<double>(), *p = p0.as<double>(), *dq = qm.as<double>(), *dp = pm.as<double>();
    int *dit = iters ? it.as<int>() : nullptr;
    if (dir == MAP_BACKWARD)
        rc = applymap_nd_inverse(m.family, d, mode, nm, ntest, m.n0, m.X, m.ldx, m.hyp, m.nhyp, m.alpha, q, p, dq, dp, dit, st);
    else if (!tan)
        rc = applymap_nd(m.family, d, mode, nm, ntest, m.n0, m.X, m.ldx, m.hyp, m.nhyp, m.alpha, q, p, dq, dp, dit, st);
    else
        rc = applymap_nd_tangent(m.family, d, mode, nm, ntest, m.n0, m.X, m.ldx, m.hyp, m.nhyp, m.alpha, q, p, dq, dp, dit,
                                 dj.as<double>(), dm.as<double>(), dl.as<double>(), st);
    if (rc) return rc;
    SGPR_HIP(hipMemcpyAsync(qmap, qm.p, out_bytes, hipMemcpyDeviceToHost, st));
    SGPR_HIP(hipMemcpyAsync(pmap, pm.p, out_bytes, hipMemcpyDeviceToHost, st));
    if (iters && it_bytes) SGPR_HIP(hipMemcpyAsync(iters, it.p, it_bytes, hipMemcpyDeviceToHost, st));
    if (tan) {
        if (tan->jac && jac_bytes) SGPR_HIP(hipMemcpyAsync(tan->jac, dj.p, jac_bytes, hipMemcpyDeviceToHost, st));
        if (tan->mono) SGPR_HIP(hipMemcpyAsync(tan->mono, dm.p, mono_bytes, hipMemcpyDeviceToHost, st));
        if (tan->lyap) SGPR_HIP(hipMemcpyAsync(tan->lyap, dl.p, lyap_bytes, hipMemcpyDeviceToHost, st));
    }
    SGPR_HIP(hipStreamSynchronize(st));
    return 0;
}

// What sgpr_fit_periodic_nd and sgpr_periodic_nd_host share: the shape of the call -- applymap_nd_call_check with the period n
// in the place of nm; the orbit is optional here, so z stands in for the two outputs that check requires -- and the search's own
// arguments.  The family's part (SGPR_MAP_EXPLICIT) is applymap_nd_tangent_check's, which the entries call as the tangent ones do.
inline int periodic_nd_call_check(const char *entry, int mode, int n, int ntest, const double *Q0, size_t ldq, const double *P0,
                                  size_t ldp, double tol, int maxit, const double *z, const double *resid, const int *its,
                                  const double *qorb, const double *porb)
{
    auto E = [&](const char *what) { set_error(std::string(entry) + ": " + what); return SGPR_E_ARG; };
    if (n < 1) return E("n < 1");
    if (maxit < 1) return E("maxit < 1");
    if (!(tol > 0.0) || !std::isfinite(tol)) return E("tol must be positive and finite");
    if (!z || !resid || !its) return E("null z, resid or its");
    if (!qorb != !porb) return E("qorb and porb must both be given or both be null");
    return applymap_nd_call_check(entry, mode, n, ntest, Q0, ldq, P0, ldp, z, z);
}

// uploads the guesses and the winding numbers (null: none), runs periodic_nd on the model, brings the results back and waits.
// Host arrays: wind ntest x d ints column-major; z [ntest][2d], resid [ntest], its [ntest]; mono [ntest][2d][2d] or null; qorb /
// porb [n][ntest][d] or both null.
inline int periodic_nd_io(const MapModel &m, int mode, int n, int ntest, const int *wind, const double *Q0, size_t ldq, const double *P0,
                          size_t ldp, double tol, int maxit, double *z, double *resid, int *its, double *mono, double *qorb,
                          double *porb)
{
    const int d = m.d;
    hipStream_t st = m.stream;
    int rc;
    DevBuf q0, p0, dw, dz, dr, di, dm, dq, dp;
    const size_t nt = (size_t)ntest, D = (size_t)2 * d, z_bytes = nt * D * sizeof(double), mono_bytes = nt * D * D * sizeof(double);
    const size_t orb_bytes = (size_t)n * nt * d * sizeof(double), wind_bytes = nt * d * sizeof(int);
    if ((rc = q0.alloc(nt * d * sizeof(double))) || (rc = p0.alloc(nt * d * sizeof(double))) || (rc = dz.alloc(z_bytes)) ||
        (rc = dr.alloc(nt * sizeof(double))) || (rc = di.alloc(nt * sizeof(int))) || (wind && (rc = dw.alloc(wind_bytes))) ||
        (mono && (rc = dm.alloc(mono_bytes))) || (qorb && ((rc = dq.alloc(orb_bytes)) || (rc = dp.alloc(orb_bytes)))))
        return rc;
    if ((rc = copy_in(q0.p, nt, Q0, ldq, nt, d, st)) || (rc = copy_in(p0.p, nt, P0, ldp, nt, d, st))) return rc;
    if (wind) SGPR_HIP(hipMemcpyAsync(dw.p, wind, wind_bytes, hipMemcpyHostToDevice, st));
    if ((rc = periodic_nd(m.family, d, mode, n, ntest, m.n0, m.X, m.ldx, m.hyp, m.nhyp, m.alpha, dw.as<int>(), q0.as<double>(),
                          p0.as<double>(), tol, maxit, dz.as<double>(), dr.as<double>(), di.as<int>(), dm.as<double>(), dq.as<double>(),
                          dp.as<double>(), st)))
        return rc;
    SGPR_HIP(hipMemcpyAsync(z, dz.p, z_bytes, hipMemcpyDeviceToHost, st));
    SGPR_HIP(hipMemcpyAsync(resid, dr.p, nt * sizeof(double), hipMemcpyDeviceToHost, st));
    SGPR_HIP(hipMemcpyAsync(its, di.p, nt * sizeof(int), hipMemcpyDeviceToHost, st));
    if (mono) SGPR_HIP(hipMemcpyAsync(mono, dm.p, mono_bytes, hipMemcpyDeviceToHost, st));
    if (qorb) {
        SGPR_HIP(hipMemcpyAsync(qorb, dq.p, orb_bytes, hipMemcpyDeviceToHost, st));
        SGPR_HIP(hipMemcpyAsync(porb, dp.p, orb_bytes, hipMemcpyDeviceToHost, st));
    }
    SGPR_HIP(hipStreamSynchronize(st));
    return 0;
}

}  // namespace sgpr
