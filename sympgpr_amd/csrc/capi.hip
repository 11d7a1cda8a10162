// capi.hip -- extern "C" entry points of libsympgpr_hip.so (see include/sympgpr_hip.h): the library's state, the stateless
// host-pointer calls, the batched fits and the profile hooks.  The fit handle is in capi_fit.hip, the *_dev primitives in
// capi_dev.hip, what they share in capi_util.h.
#include <map>
#include <mutex>
#include <string>
#include "capi_util.h"

namespace sgpr {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
int hip_fail(hipError_t e, const char *what, const char *file, int line)
{
    g_err = std::string(hipGetErrorString(e)) + " in " + what + " (" + file + ":" + std::to_string(line) + ")";
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? SGPR_E_NOMEM : SGPR_E_HIP;
}

int need_device()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        set_error("no HIP device: libsympgpr_hip.so has no CPU fallback");
        return SGPR_E_NODEVICE;
    }
    return 0;
}

// Experiment knobs of the kernels and drivers (panel widths, planner constants, tile-shape switches ...): NOT environment
// variables of the product any more.  They keep their built-in values unless a measurement tool or a test sets them through
// libsympgpr_probe.so (sgpr_probe_tune) before the code that reads them runs for the first time in the process.
static std::mutex g_tune_mu;
static std::map<std::string, double> g_tune;
double tune(const char *name, double dflt)
{
    std::lock_guard<std::mutex> lock(g_tune_mu);
    const auto it = g_tune.find(name);
    return it == g_tune.end() ? dflt : it->second;
}
void tune_set(const char *name, double v)
{
    std::lock_guard<std::mutex> lock(g_tune_mu);
    g_tune[name] = v;
}

}  // namespace sgpr

using namespace sgpr;

// The four stateless Gram wrappers over n points (x, y) and n0 points (x0, y0): the shape check (`shape_ok`, else `bad`), the
// hyperparameters, four uploads, a dense (rows x cols) result filled by launch(dx, dy, dx0, dy0, kc, G, st), its download to
// out (leading dimension ldo) and the wait.
template <typename Launch>
static int gram_host(const char *bad, bool shape_ok, int family, int n, int n0, const double *x, const double *y, const double *x0,
                     const double *y0, const double *hyp, int nhyp, size_t rows, size_t cols, double *out, size_t ldo, Launch launch)
{
    int rc = need_device();
    if (rc) return rc;
    if (!shape_ok) { set_error(bad); return SGPR_E_ARG; }
    KConst kc;
    if ((rc = make_kconst(family, hyp, nhyp, &kc))) return rc;
    if (n == 0 || n0 == 0) return 0;
    DevBuf dx, dy, dx0, dy0, dG;
    hipStream_t st = nullptr;
    if ((rc = upload(dx, x, n, st)) || (rc = upload(dy, y, n, st)) || (rc = upload(dx0, x0, n0, st)) ||
        (rc = upload(dy0, y0, n0, st)) || (rc = dG.alloc(rows * cols * sizeof(double))))
        return rc;
    if ((rc = launch(dx.as<double>(), dy.as<double>(), dx0.as<double>(), dy0.as<double>(), kc, dG.as<double>(), st))) return rc;
    if ((rc = copy_out(out, ldo, dG.p, rows, rows, cols, st))) return rc;
    SGPR_HIP(hipStreamSynchronize(st));
    return 0;
}

// The output half of the two d = 1 map entries: qmap / pmap / optional pdiff [nm][ntest] on the device, filled by
// launch(dqmap, dpmap, dpdiff), their download and the wait.
template <typename Launch>
static int map_outputs(int nm, int ntest, double *qmap, double *pmap, double *pdiff, hipStream_t st, Launch launch)
{
    int rc;
    DevBuf qm, pm, pd;
    const size_t out_bytes = (size_t)nm * ntest * sizeof(double);
    if ((rc = qm.alloc(out_bytes)) || (rc = pm.alloc(out_bytes)) || (pdiff && (rc = pd.alloc(out_bytes)))) return rc;
    if ((rc = launch(qm.as<double>(), pm.as<double>(), pdiff ? pd.as<double>() : nullptr))) return rc;
    SGPR_HIP(hipMemcpyAsync(qmap, qm.p, out_bytes, hipMemcpyDeviceToHost, st));
    SGPR_HIP(hipMemcpyAsync(pmap, pm.p, out_bytes, hipMemcpyDeviceToHost, st));
    if (pdiff) SGPR_HIP(hipMemcpyAsync(pdiff, pd.p, out_bytes, hipMemcpyDeviceToHost, st));
    SGPR_HIP(hipStreamSynchronize(st));
    return 0;
}

// The model of the d-pair *_host entries (capi_util.h: MapModel), behind their other checks: the check of the training set, the
// device, the empty call, the upload of X and alpha; run(model) is the call itself
template <typename Run>
static int with_host_map_model(const char *me, int family, int d, int ntest, const double *hyp, int nhyp, int n0, const double *X,
                               size_t ldx, const double *alpha, Run run)
{
    if (n0 < 0 || (n0 > 0 && (!X || !alpha || ldx < (size_t)n0))) {
        set_error(std::string(me) + ": n0 < 0, null X or alpha, or ldx < n0");
        return SGPR_E_ARG;
    }
    int rc = need_device();
    if (rc || ntest == 0) return rc;
    DevBuf dX, dal;
    hipStream_t st = nullptr;
    const int D = 2 * d;
    if ((rc = dX.alloc((size_t)n0 * D * sizeof(double))) || (rc = upload(dal, alpha, (size_t)D * n0, st))) return rc;
    if (n0 > 0 && (rc = copy_in(dX.p, (size_t)n0, X, ldx, (size_t)n0, D, st))) return rc;
    return run(MapModel{family, d, n0, dX.as<double>(), (size_t)n0, hyp, nhyp, dal.as<double>(), st});
}

// sgpr_applymap_nd_host (tan null), sgpr_applymap_nd_tangent_host and sgpr_applymap_nd_inverse_host (MAP_BACKWARD, tan null):
// every argument is checked before any device call
static int applymap_nd_host(const char *me, int family, int d, int mode, int nm, int ntest, const double *hyp, int nhyp, int n0,
                            const double *X, size_t ldx, const double *alpha, const double *Q0, size_t ldq, const double *P0,
                            size_t ldp, double *qmap, double *pmap, int *iters, const MapTangentOut *tan,
                            MapDirection dir = MAP_FORWARD)
{
    int rc = applymap_nd_kernel_check(me, family, d, hyp, nhyp);
    if (rc || (rc = applymap_nd_call_check(me, mode, nm, ntest, Q0, ldq, P0, ldp, qmap, pmap)) ||
        (tan && (rc = applymap_nd_tangent_check(me, family, mode, nm, tan->lyap))) ||
        (dir == MAP_BACKWARD && (rc = applymap_nd_inverse_check(me, mode))))
        return rc;
    return with_host_map_model(me, family, d, ntest, hyp, nhyp, n0, X, ldx, alpha, [&](const MapModel &m) {
        return applymap_nd_io(m, mode, nm, ntest, Q0, ldq, P0, ldp, qmap, pmap, iters, tan, dir);
    });
}

// sgpr_applymap_sections_host (tan null), sgpr_applymap_sections_tangent_host and sgpr_applymap_sections_inverse_host (MAP_BACKWARD:
// no guess GPs, no pdiff, no tangent; iters [nm - 1][ntest] or null is its own output): every argument is checked before any
// device call
static int applymap_sections_host(const char *me, int family, int mode, int nsec, int first, int nm, int ntest, const double *hyp,
                                  int nhyp, int n0, const double *xtrain, const double *ytrain, const double *alpha,
                                  const double *hypp, int nhypp, int n0p, const double *xtrainp, const double *ytrainp,
                                  const double *alphap, const double *Q0, const double *P0, double *qmap, double *pmap, double *pdiff,
                                  const MapTangentOut *tan, MapDirection dir = MAP_FORWARD, int *iters = nullptr)
{
    auto E = [&](const char *what) { set_error(std::string(me) + ": " + what); return SGPR_E_ARG; };
    const bool back = dir == MAP_BACKWARD, expl = (mode & SGPR_MAP_EXPLICIT) != 0;
    const bool guess = !back && !expl;       /* no first-guess GPs in the explicit map, nor backwards */
    if (!guess) n0p = 0;
    if (mode & ~(SGPR_MAP_WRAP_Q | SGPR_MAP_WRAP_P | SGPR_MAP_EXPLICIT | SGPR_MAP_LOSS_NEGP)) return E("unknown mode bit");
    if (back && (mode & SGPR_MAP_WRAP_P)) return E("SGPR_MAP_WRAP_P has no backward step (the two halves of a wrapped step sit at different P)");
    if (back && expl) return E("SGPR_MAP_EXPLICIT has no backward step (for the sum kernels the two maps coincide: use the implicit mode)");
    if (expl && (mode & SGPR_MAP_LOSS_NEGP)) return E("SGPR_MAP_LOSS_NEGP belongs to the implicit map");
    if (nsec < 1) return E("nsec < 1");
    if (first < 0 || first >= nsec) return E("first outside [0, nsec)");
    if (nm < 1) return E("nm < 1");
    if (ntest < 0 || n0 < 0 || n0p < 0) return E(back ? "negative ntest or n0" : "negative ntest, n0 or n0p");
    if (!hyp || (guess && !hypp) || !Q0 || !P0 || !qmap || !pmap)
        return E(back ? "null hyp, Q0, P0, qmap or pmap" : "null hyp, hypp, Q0, P0, qmap or pmap");
    if ((n0 > 0 && (!xtrain || !ytrain || !alpha)) || (n0p > 0 && (!xtrainp || !ytrainp || !alphap)))
        return E("null training points or alpha");
    if (tan) {
        if (mode & SGPR_MAP_WRAP_P) return E("SGPR_MAP_WRAP_P has no tangent map here (it would need two Hessians per step)");
        if (expl && !family_is_sum(family))
            return E("SGPR_MAP_EXPLICIT has a tangent map for the sum kernels only (family B, or a USER sum kernel)");
        if (tan->lyap && nm < 2) return E("lyap needs nm >= 2");
    }
    int rc;
    const size_t ns = (size_t)nsec;
    std::vector<KConst> kc((back ? 1 : 2) * ns);        /* the sections' constants: nsec for the map, forwards nsec for the guess */
    for (int s = 0; s < nsec; ++s) {
        if ((rc = make_kconst(family, hyp + (size_t)s * nhyp, nhyp, &kc[s]))) return rc;
        if (guess && (rc = make_kconst(family, hypp + (size_t)s * nhypp, nhypp, &kc[nsec + s]))) return rc;
    }
    if ((rc = need_device())) return rc;
    if (ntest == 0) return 0;
    DevBuf x, y, al, xp, yp, alp, dk, q0, p0, dj, dm, dl, di;
    hipStream_t st = nullptr;
    static_assert(sizeof(KConst) % sizeof(double) == 0, "KConst is uploaded as doubles");
    if ((rc = upload(x, xtrain, ns * n0, st)) || (rc = upload(y, ytrain, ns * n0, st)) || (rc = upload(al, alpha, 2 * ns * n0, st)) ||
        (rc = upload(xp, xtrainp, ns * n0p, st)) || (rc = upload(yp, ytrainp, ns * n0p, st)) || (rc = upload(alp, alphap, ns * n0p, st)) ||
        (rc = upload(dk, reinterpret_cast<const double *>(kc.data()), kc.size() * (sizeof(KConst) / sizeof(double)), st)) ||
        (rc = upload(q0, Q0, ntest, st)) || (rc = upload(p0, P0, ntest, st)))
        return rc;
    const size_t mono_bytes = (size_t)ntest * 4 * sizeof(double), jac_bytes = (size_t)(nm - 1) * mono_bytes;
    const size_t lyap_bytes = (size_t)ntest * 2 * sizeof(double), it_bytes = (size_t)(nm - 1) * ntest * sizeof(int);
    const bool want_it = back && iters && it_bytes;
    if ((want_it && (rc = di.alloc(it_bytes))) ||
        (tan && ((tan->jac && (rc = dj.alloc(jac_bytes))) || (tan->mono && (rc = dm.alloc(mono_bytes))) || (tan->lyap && (rc = dl.alloc(lyap_bytes))))))
        return rc;
    rc = map_outputs(nm, ntest, qmap, pmap, pdiff, st, [&](double *qm, double *pm, double *pd) {
        if (back)
            return applymap_sections_inverse(family, mode, nsec, first, nm, ntest, n0, x.as<double>(), y.as<double>(), al.as<double>(),
                                             dk.as<KConst>(), q0.as<double>(), p0.as<double>(), qm, pm, want_it ? di.as<int>() : nullptr, st);
        return applymap_sections(family, mode, nsec, first, nm, ntest, n0, x.as<double>(), y.as<double>(), al.as<double>(),
                                 dk.as<KConst>(), n0p, xp.as<double>(), yp.as<double>(), alp.as<double>(), dk.as<KConst>() + nsec,
                                 q0.as<double>(), p0.as<double>(), qm, pm, pd, st, tan != nullptr, dj.as<double>(), dm.as<double>(),
                                 dl.as<double>());
    });
    if (rc || (!tan && !want_it)) return rc;
    if (want_it) SGPR_HIP(hipMemcpyAsync(iters, di.p, it_bytes, hipMemcpyDeviceToHost, st));
    if (tan && tan->jac && jac_bytes) SGPR_HIP(hipMemcpyAsync(tan->jac, dj.p, jac_bytes, hipMemcpyDeviceToHost, st));
    if (tan && tan->mono) SGPR_HIP(hipMemcpyAsync(tan->mono, dm.p, mono_bytes, hipMemcpyDeviceToHost, st));
    if (tan && tan->lyap) SGPR_HIP(hipMemcpyAsync(tan->lyap, dl.p, lyap_bytes, hipMemcpyDeviceToHost, st));
    SGPR_HIP(hipStreamSynchronize(st));
    return 0;
}

extern "C" {

int sgpr_abi_version(void) { return SGPR_ABI_VERSION; }
const char *sgpr_last_error(void) { return g_err.c_str(); }

int sgpr_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int sgpr_set_device(int dev)
{
    int rc = need_device();
    if (rc) return rc;
    SGPR_HIP(hipSetDevice(dev));
    return 0;
}

int sgpr_build_k_host(int family, int n, int n0, const double *x, const double *y, const double *x0,
                      const double *y0, const double *hyp, int nhyp, double *K, size_t ldk)
{
    const size_t ld = 2 * (size_t)n;
    const bool ok = n >= 0 && n0 >= 0 && ldk >= (size_t)(2 * n);
    auto launch = [=](double *dx, double *dy, double *dx0, double *dy0, const KConst &kc, double *k, hipStream_t st) {
        return gram_pairs(family, n, n0, dx, dy, dx0, dy0, kc, k, k + n, k + ld * n0, k + n + ld * n0, ld, 0, 0.0, SGPR_G_ALL, st);
    };
    return gram_host("build_k: bad shape", ok, family, n, n0, x, y, x0, y0, hyp, nhyp, ld, 2 * (size_t)n0, K, ldk, launch);
}

int sgpr_buildkreg_host(int family, int n, int n0, const double *x, const double *y, const double *x0,
                        const double *y0, const double *hyp, int nhyp, double *K, size_t ldk)
{
    const bool ok = n >= 0 && n0 >= 0 && ldk >= (size_t)n;
    auto launch = [=](double *dx, double *dy, double *dx0, double *dy0, const KConst &kc, double *k, hipStream_t st) {
        return gram_reg(family, n, n0, dx, dy, dx0, dy0, kc, k, (size_t)n, 0, 0.0, st);
    };
    return gram_host("buildkreg: bad shape", ok, family, n, n0, x, y, x0, y0, hyp, nhyp, (size_t)n, (size_t)n0, K, ldk, launch);
}

/* build_dK (functions/func.py:80-129), one length scale: dK is (2 n0 x 2 n), rows index the "0"
 * points; entries sig * d3k..dl(x0[k], y0[k], x[lk], y[lk]).  Every entry is even under a <-> b,
 * so the pair kernel is run with the "0" points as its row points. */
int sgpr_build_dk_host(int family, int which, int n, int n0, const double *x, const double *y,
                       const double *x0, const double *y0, const double *hyp, int nhyp, double *dK, size_t ld)
{
    const size_t l = 2 * (size_t)n0;
    const bool ok = n >= 0 && n0 >= 0 && ld >= (size_t)(2 * n0) && (which == 0 || which == 1);
    auto launch = [=](double *dx, double *dy, double *dx0, double *dy0, const KConst &kc, double *d, hipStream_t st) {
        return gram_pairs(family, n0, n, dx0, dy0, dx, dy, kc, d, d + n0, d + l * n, d + n0 + l * n, l, 0, 0.0,
                          SGPR_G_ALL | (which ? SGPR_G_DLY : SGPR_G_DLX), st);
    };
    return gram_host("build_dk: bad arguments", ok, family, n, n0, x, y, x0, y0, hyp, nhyp, l, 2 * (size_t)n, dK, ld, launch);
}

/* build_dKreg (functions/func.py:52-78): dK is (n x n0), Kp[k,lk] = sig dkdl(x0[lk], y0[lk], x[k], y[k]) */
int sgpr_build_dkreg_host(int family, int which, int n, int n0, const double *x, const double *y,
                          const double *x0, const double *y0, const double *hyp, int nhyp, double *dK, size_t ld)
{
    const bool ok = n >= 0 && n0 >= 0 && ld >= (size_t)n && (which == 0 || which == 1);
    auto launch = [=](double *dx, double *dy, double *dx0, double *dy0, const KConst &kc, double *d, hipStream_t st) {
        return gram_reg(family, n, n0, dx, dy, dx0, dy0, kc, d, (size_t)n, 0, 0.0, st, which ? DERIV_LY : DERIV_LX);
    };
    return gram_host("build_dkreg: bad arguments", ok, family, n, n0, x, y, x0, y0, hyp, nhyp, (size_t)n, (size_t)n0, dK, ld, launch);
}

/* d canonical pairs: X (n x 2d), X0 (n0 x 2d) column-major, hyp = (lq_1..lq_d, lP_1..lP_d, sig);
 * K (2 d n x 2 d n0), block (a, b) at rows a n, columns b n0.  d = 1 == sgpr_build_k_host. */
int sgpr_build_k_nd_host(int family, int d, int n, int n0, const double *X, size_t ldx, const double *X0,
                         size_t ldx0, const double *hyp, int nhyp, double *K, size_t ldk)
{
    int rc = need_device();
    if (rc) return rc;
    if (d < 1 || d > 3 || n < 0 || n0 < 0 || ldk < (size_t)(2 * d * n) || ldx < (size_t)n || ldx0 < (size_t)n0) {
        set_error("build_k_nd: bad shape");
        return SGPR_E_ARG;
    }
    if (n == 0 || n0 == 0) return 0;
    const int D = 2 * d;
    DevBuf dX, dX0, dK;
    hipStream_t st = nullptr;
    if ((rc = dX.alloc((size_t)n * D * sizeof(double))) || (rc = dX0.alloc((size_t)n0 * D * sizeof(double))) ||
        (rc = dK.alloc((size_t)D * n * D * n0 * sizeof(double))))
        return rc;
    if ((rc = copy_in(dX.p, (size_t)n, X, ldx, (size_t)n, D, st)) || (rc = copy_in(dX0.p, (size_t)n0, X0, ldx0, (size_t)n0, D, st)))
        return rc;
    const size_t ld = (size_t)D * n;
    if ((rc = gram_nd(family, d, n, n0, dX.as<double>(), (size_t)n, dX0.as<double>(), (size_t)n0, hyp, nhyp,
                      dK.as<double>(), ld, (size_t)n, (size_t)n0, 0, 0.0, st)))
        return rc;
    if ((rc = copy_out(K, ldk, dK.p, ld, ld, (size_t)D * n0, st))) return rc;
    SGPR_HIP(hipStreamSynchronize(st));
    return 0;
}

int sgpr_kernel_eval_host(int family, int which, int m, const double *xa, const double *ya,
                          const double *xb, const double *yb, const double *l, int nl, double *out)
{
    int rc = need_device();
    if (rc) return rc;
    KConst kc;
    if ((rc = make_kconst_l(family, l, nl, &kc))) return rc;
    if (m <= 0) return 0;
    DevBuf a, b, c, d, o;
    hipStream_t st = nullptr;
    if ((rc = upload(a, xa, m, st)) || (rc = upload(b, ya, m, st)) || (rc = upload(c, xb, m, st)) ||
        (rc = upload(d, yb, m, st)) || (rc = o.alloc(m * sizeof(double))))
        return rc;
    rc = kernel_eval(family, which, m, a.as<double>(), b.as<double>(), c.as<double>(), d.as<double>(), kc,
                     o.as<double>(), st);
    if (rc) return rc;
    SGPR_HIP(hipMemcpyAsync(out, o.p, m * sizeof(double), hipMemcpyDeviceToHost, st));
    SGPR_HIP(hipStreamSynchronize(st));
    return 0;
}

int sgpr_potrf_host(int n, double *A, size_t lda)
{
    int rc = need_device();
    if (rc) return rc;
    if (n < 0 || (n > 0 && lda < (size_t)n)) { set_error("potrf: bad n / lda"); return SGPR_E_ARG; }
    if (n == 0) return 0;
    DevBuf dA, dW, dI;
    hipStream_t st = nullptr;
    const size_t ld = (size_t)n;
    if ((rc = dA.alloc(ld * n * sizeof(double))) || (rc = dW.alloc(potrf_workspace(n))) ||
        (rc = dI.alloc(sizeof(int))))
        return rc;
    auto put = [&]() { return copy_in(dA.p, ld, A, lda, ld, ld, st); };   // the caller's matrix is still on the host
    auto factor = [&]() { return potrf(n, dA.as<double>(), ld, dW.p, potrf_workspace(n), dI.as<int>(), st); };
    int info = 0;
    if ((rc = put()) || (rc = factor_with_retry(factor, dI.as<int>(), &info, st, put))) return rc;
    if ((rc = zero_strict_upper(n, dA.as<double>(), ld, st))) return rc;
    SGPR_HIP(hipStreamSynchronize(st));
    if (info) return info_status(info);
    if ((rc = copy_out(A, lda, dA.p, ld, ld, ld, st))) return rc;
    SGPR_HIP(hipStreamSynchronize(st));
    return 0;
}

int sgpr_potrs_host(int n, const double *L, size_t ldl, double *B, size_t ldb, int nrhs)
{
    int rc = need_device();
    if (rc) return rc;
    if (n < 0 || nrhs < 0 || (n > 0 && (ldl < (size_t)n || ldb < (size_t)n))) {
        set_error("potrs: bad shape");
        return SGPR_E_ARG;
    }
    if (n == 0 || nrhs == 0) return 0;
    DevBuf dL, dW, dB, dS;
    hipStream_t st = nullptr;
    const size_t ld = (size_t)n;
    if ((rc = dL.alloc(ld * n * sizeof(double))) || (rc = dW.alloc(potrf_workspace(n))) ||
        (rc = dB.alloc(ld * nrhs * sizeof(double))))
        return rc;
    if ((rc = copy_in(dL.p, ld, L, ldl, ld, ld, st)) || (rc = copy_in(dB.p, ld, B, ldb, ld, nrhs, st))) return rc;
    if ((rc = leaf_inverses(n, dL.as<double>(), ld, dW.p, nullptr, st))) return rc;
    if (potrs_blocked(n, nrhs, dL.as<double>(), ld) && (rc = dS.alloc(potrs_mat_scratch(n, nrhs, dL.as<double>(), ld)))) return rc;
    if ((rc = potrs_dispatch(n, dL.as<double>(), ld, dW.p, dB.as<double>(), ld, nrhs, dS.as<double>(), st))) return rc;
    if ((rc = copy_out(B, ldb, dB.p, ld, ld, nrhs, st))) return rc;
    SGPR_HIP(hipStreamSynchronize(st));
    return 0;
}

/* LAPACK dsyev('V', 'L') shaped host call: A (n x n, column-major, lower triangle read) is
 * overwritten by the eigenvectors, w (n) receives the eigenvalues in ascending order. */
int sgpr_syev_host(int n, double *A, size_t lda, double *w)
{
    int rc = need_device();
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!A || !w || lda < (size_t)n))) { set_error("syev: bad arguments"); return SGPR_E_ARG; }
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    DevBuf dA, dV;
    if ((rc = dA.alloc(N * N * sizeof(double))) || (rc = dV.alloc(N * N * sizeof(double)))) return rc;
    hipStream_t st = nullptr;
    if ((rc = copy_in(dA.p, N, A, lda, N, N, st))) return rc;
    if ((rc = sym_fill_upper(n, dA.as<double>(), N, st))) return rc;
    int sweeps = 0;
    const int status = syev_jacobi(n, dA.as<double>(), N, dV.as<double>(), N, w, 40, &sweeps, st);
    if (status < 0) return status;
    if ((rc = copy_out(A, lda, dA.p, N, N, N, st))) return rc;
    SGPR_HIP(hipStreamSynchronize(st));
    if (status > 0) set_error("syev: Jacobi sweeps did not converge");
    return status;
}

/* ---- many small fits in one launch ------------------------------------------------------- */

int sgpr_fit_batch_max_order(void) { return fit_batch_max_order(); }

/* The BatchCall (common.h) of an entry that takes its points as x | y, and of one that takes d canonical pairs per point.  The
 * mode of the call is the set of outputs the entry hands on: grad, loo, or value beside grad for the objective `which`. */
struct BatchOuts {
    double *grad = nullptr, *loo = nullptr, *value = nullptr;
    int which = SGPR_LOO_LPD;
};
static BatchCall batch_call_xy(int family, int nbatch, int n_pts, const double *x, const double *y, const double *z, const double *hyp,
                               int nhyp, const double *sig2n, unsigned flags, double *alpha, double *nll, int *info, BatchOuts o = {})
{
    const int reg = (flags & SGPR_FIT_REG) ? 1 : 0;
    return BatchCall{family, 0, reg, nbatch, n_pts, reg ? n_pts : 2 * n_pts, nhyp, x, y, z, hyp, sig2n, alpha, nll, info,
                     o.grad, o.loo, o.value, o.which};
}
static BatchCall batch_call_nd(int family, int d, int nbatch, int n_pts, const double *X, const double *z, const double *hyp, int nhyp,
                               const double *sig2n, double *alpha, double *nll, int *info, BatchOuts o = {})
{
    return BatchCall{family, d, 0, nbatch, n_pts, 2 * d * n_pts, nhyp, X, nullptr, z, hyp, sig2n, alpha, nll, info,
                     o.grad, o.loo, o.value, o.which};
}
/* Unlike the entries below this one asks for a device first, and for the family only once an empty batch has returned. */
int sgpr_fit_batch(int family, int nbatch, int n_pts, const double *x, const double *y, const double *z,
                   const double *hyp, int nhyp, const double *sig2n, unsigned flags, double *alpha, double *nll,
                   int *info)
{
    int rc = need_device();
    if (rc) return rc;
    const BatchCall c = batch_call_xy(family, nbatch, n_pts, x, y, z, hyp, nhyp, sig2n, flags, alpha, nll, info);
    if (nbatch < 0 || n_pts <= 0 || c.n > fit_batch_max_order() || !x || !y || !z || !hyp || !sig2n || !nll || !info ||
        (flags & ~(unsigned)SGPR_FIT_REG)) {
        set_error("fit_batch: bad arguments (order per problem at most 2048)");
        return SGPR_E_ARG;
    }
    if (nbatch == 0) return 0;
    if (family < SGPR_FAM_A || family > SGPR_FAM_USER) { set_error("fit_batch: unknown kernel family"); return SGPR_E_ARG; }
    return fit_batch_run(c);
}

/* The argument check of the batched entries below, before any device call: an argument error is SGPR_E_ARG on any machine, and
 * the message names the entry.  d: null for the entries that take x | y (nhyp 4 or 3, flags SGPR_FIT_REG or none), else the
 * canonical pairs per point (nhyp 3d + 1 or 2d + 1, no flags).  which: null, or the loo objective to check.  The order per problem
 * must be above nmin (0: no lower limit) and at most nmax.  outs names the required output pointers; outs_ok / ins_ok: none of
 * them / of the inputs is null. */
static int check_batch_args(const char *entry, int family, const int *d, int nhyp, unsigned flags, const int *which, int nbatch,
                            int n_pts, int nmin, int nmax, const char *outs, bool outs_ok, bool ins_ok)
{
    auto E = [entry](const std::string &what) { set_error(std::string(entry) + ": " + what); return SGPR_E_ARG; };
    if (d && (*d < 1 || *d > 3)) return E("d must be 1, 2 or 3");
    if (family < SGPR_FAM_A || family > SGPR_FAM_USER) return E("unknown kernel family");
    const int need = d ? (family_has_p(family) ? 3 * *d + 1 : 2 * *d + 1) : (family_has_p(family) ? 4 : 3);
    if (nhyp != need) return E("nhyp must be " + std::to_string(need) + (d ? " for this family and d" : " for this family"));
    if (d && flags) return E("flags must be 0 (there is no scalar-kernel d-pair fit)");
    if (flags & ~(unsigned)SGPR_FIT_REG) return E("unknown flag (only SGPR_FIT_REG)");
    if (which && *which != SGPR_LOO_LPD && *which != SGPR_LOO_PRESS) return E("which must be SGPR_LOO_LPD or SGPR_LOO_PRESS");
    if (nbatch < 0) return E("nbatch < 0");
    if (n_pts <= 0) return E("n_pts <= 0");
    const long n = d ? 2L * *d * n_pts : (flags & SGPR_FIT_REG) ? (long)n_pts : 2L * n_pts;
    if (n <= nmin) return E("order per problem " + std::to_string(n) + " is at most " + std::to_string(nmin) + ": the one-launch entry's range");
    if (n > nmax) return E("order per problem " + std::to_string(n) + " exceeds " + std::to_string(nmax));
    if (!outs_ok) return E(std::string("null ") + outs);
    if (!ins_ok) return E("null input");
    return 0;
}

/* sgpr_fit_batch for problems with d canonical pairs per point (batch.hip: fit_batch_nd_kernel up to order 256, the mid path
 * with mid_build_nd_kernel above). */
int sgpr_fit_batch_nd(int family, int d, int nbatch, int n_pts, const double *X, const double *z, const double *hyp, int nhyp,
                      const double *sig2n, unsigned flags, double *alpha, double *nll, int *info)
{
    int rc = check_batch_args("fit_batch_nd", family, &d, nhyp, flags, nullptr, nbatch, n_pts, 0, fit_batch_max_order(), "nll or info",
                              nll && info, X && z && hyp && sig2n);
    if (rc || nbatch == 0 || (rc = need_device())) return rc;
    return fit_batch_run(batch_call_nd(family, d, nbatch, n_pts, X, z, hyp, nhyp, sig2n, alpha, nll, info));
}

/* sgpr_fit_batch_nd plus the gradient of every problem's nll, every order up to the maximum (batch.hip: the gradient mode of
 * fit_batch_nd_kernel up to order 256, the mid path with mid_grad_nd_kernel above). */
int sgpr_fit_batch_nd_grad(int family, int d, int nbatch, int n_pts, const double *X, const double *z, const double *hyp, int nhyp,
                           const double *sig2n, unsigned flags, double *alpha, double *nll, double *grad, int *info)
{
    int rc = check_batch_args("fit_batch_nd_grad", family, &d, nhyp, flags, nullptr, nbatch, n_pts, 0, fit_batch_max_order(),
                              "nll, grad or info", nll && grad && info, X && z && hyp && sig2n);
    if (rc || nbatch == 0 || (rc = need_device())) return rc;
    return fit_batch_run(batch_call_nd(family, d, nbatch, n_pts, X, z, hyp, nhyp, sig2n, alpha, nll, info, {grad}));
}

/* sgpr_fit_batch_nd plus leave-one-point-out cross-validation per problem over 2d x 2d point blocks, every order up to the maximum
 * (batch.hip: the loo mode of fit_batch_nd_kernel up to order 256, the mid path with mid_loo_kernel<2d> above). */
int sgpr_fit_batch_nd_loo(int family, int d, int nbatch, int n_pts, const double *X, const double *z, const double *hyp, int nhyp,
                          const double *sig2n, unsigned flags, double *alpha, double *nll, double *loo, int *info)
{
    int rc = check_batch_args("fit_batch_nd_loo", family, &d, nhyp, flags, nullptr, nbatch, n_pts, 0, fit_batch_max_order(),
                              "nll, loo or info", nll && loo && info, X && z && hyp && sig2n);
    if (rc || nbatch == 0 || (rc = need_device())) return rc;
    return fit_batch_run(batch_call_nd(family, d, nbatch, n_pts, X, z, hyp, nhyp, sig2n, alpha, nll, info, {nullptr, loo}));
}

/* sgpr_fit_batch_nd plus one leave-one-point-out objective and its gradient per problem, orders up to 256 (batch.hip: the loograd
 * mode of fit_batch_nd_kernel). */
int sgpr_fit_batch_nd_loo_grad(int family, int d, int nbatch, int n_pts, const double *X, const double *z, const double *hyp,
                               int nhyp, const double *sig2n, unsigned flags, int which, double *alpha, double *nll,
                               double *value, double *grad, int *info)
{
    int rc = check_batch_args("fit_batch_nd_loo_grad", family, &d, nhyp, flags, &which, nbatch, n_pts, 0, fit_batch_grad_max_order(),
                              "nll, value, grad or info", nll && value && grad && info, X && z && hyp && sig2n);
    if (rc || nbatch == 0 || (rc = need_device())) return rc;
    return fit_batch_run(batch_call_nd(family, d, nbatch, n_pts, X, z, hyp, nhyp, sig2n, alpha, nll, info, {grad, nullptr, value, which}));
}

/* sgpr_fit_batch plus the gradient of every problem's nll (batch.hip: the gradient mode of fit_batch_kernel). */
int sgpr_fit_batch_grad(int family, int nbatch, int n_pts, const double *x, const double *y, const double *z,
                        const double *hyp, int nhyp, const double *sig2n, unsigned flags, double *alpha, double *nll,
                        double *grad, int *info)
{
    int rc = check_batch_args("fit_batch_grad", family, nullptr, nhyp, flags, nullptr, nbatch, n_pts, 0, fit_batch_grad_max_order(),
                              "nll, grad or info", nll && grad && info, x && y && z && hyp && sig2n);
    if (rc || nbatch == 0 || (rc = need_device())) return rc;
    return fit_batch_run(batch_call_xy(family, nbatch, n_pts, x, y, z, hyp, nhyp, sig2n, flags, alpha, nll, info, {grad}));
}

/* The same above order 256, up to sgpr_fit_batch_max_order() (batch.hip: the mid path with its gradient phase). */
int sgpr_fit_batch_grad_mid(int family, int nbatch, int n_pts, const double *x, const double *y, const double *z,
                            const double *hyp, int nhyp, const double *sig2n, unsigned flags, double *alpha, double *nll,
                            double *grad, int *info)
{
    int rc = check_batch_args("fit_batch_grad_mid", family, nullptr, nhyp, flags, nullptr, nbatch, n_pts, fit_batch_grad_max_order(),
                              fit_batch_max_order(), "nll, grad or info", nll && grad && info, x && y && z && hyp && sig2n);
    if (rc || nbatch == 0 || (rc = need_device())) return rc;
    return fit_batch_run(batch_call_xy(family, nbatch, n_pts, x, y, z, hyp, nhyp, sig2n, flags, alpha, nll, info, {grad}));
}

/* sgpr_fit_batch plus leave-one-point-out cross-validation per problem, every order up to sgpr_fit_batch_max_order() (batch.hip:
 * the loo mode of fit_batch_kernel up to order 256, the mid path with its loo phase above). */
int sgpr_fit_batch_loo(int family, int nbatch, int n_pts, const double *x, const double *y, const double *z,
                       const double *hyp, int nhyp, const double *sig2n, unsigned flags, double *alpha, double *nll,
                       double *loo, int *info)
{
    int rc = check_batch_args("fit_batch_loo", family, nullptr, nhyp, flags, nullptr, nbatch, n_pts, 0, fit_batch_max_order(),
                              "nll, loo or info", nll && loo && info, x && y && z && hyp && sig2n);
    if (rc || nbatch == 0 || (rc = need_device())) return rc;
    return fit_batch_run(batch_call_xy(family, nbatch, n_pts, x, y, z, hyp, nhyp, sig2n, flags, alpha, nll, info, {nullptr, loo}));
}

/* sgpr_fit_batch plus one leave-one-point-out objective and its gradient per problem, orders up to 256 (batch.hip: the loograd
 * mode of fit_batch_kernel). */
int sgpr_fit_batch_loo_grad(int family, int nbatch, int n_pts, const double *x, const double *y, const double *z,
                            const double *hyp, int nhyp, const double *sig2n, unsigned flags, int which, double *alpha,
                            double *nll, double *value, double *grad, int *info)
{
    int rc = check_batch_args("fit_batch_loo_grad", family, nullptr, nhyp, flags, &which, nbatch, n_pts, 0, fit_batch_grad_max_order(),
                              "nll, value, grad or info", nll && value && grad && info, x && y && z && hyp && sig2n);
    if (rc || nbatch == 0 || (rc = need_device())) return rc;
    return fit_batch_run(batch_call_xy(family, nbatch, n_pts, x, y, z, hyp, nhyp, sig2n, flags, alpha, nll, info, {grad, nullptr, value, which}));
}

/* The same above order 256, up to sgpr_fit_batch_max_order() (batch.hip: the mid path with its loo gradient stage). */
int sgpr_fit_batch_loo_grad_mid(int family, int nbatch, int n_pts, const double *x, const double *y, const double *z,
                                const double *hyp, int nhyp, const double *sig2n, unsigned flags, int which, double *alpha,
                                double *nll, double *value, double *grad, int *info)
{
    int rc = check_batch_args("fit_batch_loo_grad_mid", family, nullptr, nhyp, flags, &which, nbatch, n_pts, fit_batch_grad_max_order(),
                              fit_batch_max_order(), "nll, value, grad or info", nll && value && grad && info, x && y && z && hyp && sig2n);
    if (rc || nbatch == 0 || (rc = need_device())) return rc;
    return fit_batch_run(batch_call_xy(family, nbatch, n_pts, x, y, z, hyp, nhyp, sig2n, flags, alpha, nll, info, {grad, nullptr, value, which}));
}

/* sgpr_fit_batch_nd_loo_grad above order 256, up to sgpr_fit_batch_max_order() (batch.hip: the same stage over 2d x 2d point blocks). */
int sgpr_fit_batch_nd_loo_grad_mid(int family, int d, int nbatch, int n_pts, const double *X, const double *z, const double *hyp,
                                   int nhyp, const double *sig2n, unsigned flags, int which, double *alpha, double *nll,
                                   double *value, double *grad, int *info)
{
    int rc = check_batch_args("fit_batch_nd_loo_grad_mid", family, &d, nhyp, flags, &which, nbatch, n_pts, fit_batch_grad_max_order(),
                              fit_batch_max_order(), "nll, value, grad or info", nll && value && grad && info, X && z && hyp && sig2n);
    if (rc || nbatch == 0 || (rc = need_device())) return rc;
    return fit_batch_run(batch_call_nd(family, d, nbatch, n_pts, X, z, hyp, nhyp, sig2n, alpha, nll, info, {grad, nullptr, value, which}));
}

/* applymap / applymap_henon (functions/func.py:216-260) and the per-example variants for all Ntest
 * orbits, every time step on the device.  alpha = Kyinv ztrain (2 n0), alphap = Kyinvp ztrainp (n0p);
 * qmap, pmap, pdiff: [nm][ntest] C-ordered host arrays (row 0 = initial conditions), pdiff optional.
 * mode: SGPR_MAP_* bits. */
int sgpr_applymap_host(int family, int mode, int nm, int ntest, const double *hyp, int nhyp, int n0,
                       const double *xtrain, const double *ytrain, const double *alpha, const double *hypp,
                       int nhypp, int n0p, const double *xtrainp, const double *ytrainp, const double *alphap,
                       const double *Q0, const double *P0, double *qmap, double *pmap, double *pdiff)
{
    int rc = need_device();
    if (rc) return rc;
    const bool expl = (mode & SGPR_MAP_EXPLICIT) != 0;
    if (expl) n0p = 0;                       /* no first-guess GP in the explicit map */
    if (nm < 1 || ntest < 0 || n0 < 0 || n0p < 0 || (mode & ~15) || (expl && (mode & SGPR_MAP_LOSS_NEGP)) || !qmap || !pmap) {
        set_error("applymap: bad arguments");
        return SGPR_E_ARG;
    }
    KConst kc, kcp{};
    if ((rc = make_kconst(family, hyp, nhyp, &kc))) return rc;
    if (!expl && (rc = make_kconst(family, hypp, nhypp, &kcp))) return rc;
    if (ntest == 0) return 0;
    if (!Q0 || !P0 || (n0 > 0 && (!xtrain || !ytrain || !alpha)) || (n0p > 0 && (!xtrainp || !ytrainp || !alphap))) {
        set_error("applymap: null argument");
        return SGPR_E_ARG;
    }
    DevBuf x, y, al, xp, yp, alp, q0, p0, tw;
    hipStream_t st = nullptr;
    if ((rc = tw.alloc(applymap_team_ws(ntest, n0)))) return rc;
    if ((rc = upload(x, xtrain, n0, st)) || (rc = upload(y, ytrain, n0, st)) || (rc = upload(al, alpha, 2 * (size_t)n0, st)) ||
        (rc = upload(xp, xtrainp, n0p, st)) || (rc = upload(yp, ytrainp, n0p, st)) || (rc = upload(alp, alphap, n0p, st)) ||
        (rc = upload(q0, Q0, ntest, st)) || (rc = upload(p0, P0, ntest, st)))
        return rc;
    rc = map_outputs(nm, ntest, qmap, pmap, pdiff, st, [&](double *qm, double *pm, double *pd) {
        return applymap(family, mode, nm, ntest, n0, x.as<double>(), y.as<double>(), kc, al.as<double>(), n0p, xp.as<double>(),
                        yp.as<double>(), kcp, alp.as<double>(), q0.as<double>(), p0.as<double>(), qm, pm, pd, tw.p, st);
    });
    return rc ? rc : applymap_status(tw.p, ntest, n0);
}

/* The sectioned map (05_tokamak/Split_SympGPR/func.py:184-219): nsec GP pairs applied in turn, every step of every orbit in
 * one launch.  Every argument is checked before any device call. */
int sgpr_applymap_sections_host(int family, int mode, int nsec, int first, int nm, int ntest, const double *hyp, int nhyp, int n0,
                                const double *xtrain, const double *ytrain, const double *alpha, const double *hypp, int nhypp,
                                int n0p, const double *xtrainp, const double *ytrainp, const double *alphap, const double *Q0,
                                const double *P0, double *qmap, double *pmap, double *pdiff)
{
    return applymap_sections_host("applymap_sections_host", family, mode, nsec, first, nm, ntest, hyp, nhyp, n0, xtrain, ytrain, alpha,
                                  hypp, nhypp, n0p, xtrainp, ytrainp, alphap, Q0, P0, qmap, pmap, pdiff, nullptr);
}

/* The same with the tangent map (mapsec_tan.h, tangent_core.h): the orbit outputs have the bits of sgpr_applymap_sections_host. */
int sgpr_applymap_sections_tangent_host(int family, int mode, int nsec, int first, int nm, int ntest, const double *hyp, int nhyp,
                                        int n0, const double *xtrain, const double *ytrain, const double *alpha, const double *hypp,
                                        int nhypp, int n0p, const double *xtrainp, const double *ytrainp, const double *alphap,
                                        const double *Q0, const double *P0, double *qmap, double *pmap, double *pdiff, double *jac,
                                        double *mono, double *lyap)
{
    const MapTangentOut tan = {jac, mono, lyap};
    return applymap_sections_host("applymap_sections_tangent_host", family, mode, nsec, first, nm, ntest, hyp, nhyp, n0, xtrain, ytrain,
                                  alpha, hypp, nhypp, n0p, xtrainp, ytrainp, alphap, Q0, P0, qmap, pmap, pdiff, &tan);
}

/* The sectioned map BACKWARDS (map.hip: applymap_sections_inverse_kernel): Q0 / P0 hold the images, row i the i-th preimage, step
 * i undoes section (first - i) mod nsec.  Every argument is checked before any device call. */
int sgpr_applymap_sections_inverse_host(int family, int mode, int nsec, int first, int nm, int ntest, const double *hyp, int nhyp,
                                        int n0, const double *xtrain, const double *ytrain, const double *alpha, const double *Q0,
                                        const double *P0, double *qmap, double *pmap, int *iters)
{
    return applymap_sections_host("applymap_sections_inverse_host", family, mode, nsec, first, nm, ntest, hyp, nhyp, n0, xtrain, ytrain,
                                  alpha, nullptr, 0, 0, nullptr, nullptr, nullptr, Q0, P0, qmap, pmap, nullptr, nullptr, MAP_BACKWARD,
                                  iters);
}

/* The d-pair map from caller-supplied training points and alpha (the counterpart of sgpr_applymap_host for d canonical pairs). */
int sgpr_applymap_nd_host(int family, int d, int mode, int nm, int ntest, const double *hyp, int nhyp, int n0, const double *X,
                          size_t ldx, const double *alpha, const double *Q0, size_t ldq, const double *P0, size_t ldp,
                          double *qmap, double *pmap, int *iters)
{
    return applymap_nd_host("applymap_nd_host", family, d, mode, nm, ntest, hyp, nhyp, n0, X, ldx, alpha, Q0, ldq, P0, ldp, qmap, pmap,
                            iters, nullptr);
}

/* The same with the tangent map (maptan.h): the orbit outputs have the bits of sgpr_applymap_nd_host. */
int sgpr_applymap_nd_tangent_host(int family, int d, int mode, int nm, int ntest, const double *hyp, int nhyp, int n0,
                                  const double *X, size_t ldx, const double *alpha, const double *Q0, size_t ldq, const double *P0,
                                  size_t ldp, double *qmap, double *pmap, int *iters, double *jac, double *mono, double *lyap)
{
    const MapTangentOut tan = {jac, mono, lyap};
    return applymap_nd_host("applymap_nd_tangent_host", family, d, mode, nm, ntest, hyp, nhyp, n0, X, ldx, alpha, Q0, ldq, P0, ldp,
                            qmap, pmap, iters, &tan);
}

/* The backward orbit: Q0 / P0 hold the images (Q, P), row i of qmap / pmap is the i-th preimage. */
int sgpr_applymap_nd_inverse_host(int family, int d, int mode, int nm, int ntest, const double *hyp, int nhyp, int n0,
                                  const double *X, size_t ldx, const double *alpha, const double *Q0, size_t ldq, const double *P0,
                                  size_t ldp, double *qmap, double *pmap, int *iters)
{
    return applymap_nd_host("applymap_nd_inverse_host", family, d, mode, nm, ntest, hyp, nhyp, n0, X, ldx, alpha, Q0, ldq, P0, ldp,
                            qmap, pmap, iters, nullptr, MAP_BACKWARD);
}

/* Periodic orbits of the d-pair map from caller-supplied training points and alpha: every argument is checked before any device
 * call, in the order of the map entries (the kernel's description, the shape of the call, the mode, the training set). */
int sgpr_periodic_nd_host(int family, int d, int mode, int n, int ntest, const double *hyp, int nhyp, int n0, const double *X,
                          size_t ldx, const double *alpha, const int *wind, const double *Q0, size_t ldq, const double *P0, size_t ldp,
                          double tol, int maxit, double *z, double *resid, int *its, double *mono, double *qorb, double *porb)
{
    const char *me = "periodic_nd_host";
    int rc = applymap_nd_kernel_check(me, family, d, hyp, nhyp);
    if (rc || (rc = periodic_nd_call_check(me, mode, n, ntest, Q0, ldq, P0, ldp, tol, maxit, z, resid, its, qorb, porb)) ||
        (rc = applymap_nd_tangent_check(me, family, mode, n + 1, nullptr)))
        return rc;
    return with_host_map_model(me, family, d, ntest, hyp, nhyp, n0, X, ldx, alpha, [&](const MapModel &m) {
        return periodic_nd_io(m, mode, n, ntest, wind, Q0, ldq, P0, ldp, tol, maxit, z, resid, its, mono, qorb, porb);
    });
}

int sgpr_release_device_streams(int device)
{
    return release_device_streams(device);      // (touches the device only if this library has streams on it)
}

int sgpr_trim(void)
{
    (void)fit_batch_trim();
    return potrf_trim();
}

int sgpr_profile_begin(void) { return gemm_profile_begin(); }
int sgpr_profile_end(double *out12)
{
    if (!out12) { set_error("null argument"); return SGPR_E_ARG; }
    return gemm_profile_end(out12);
}

int sgpr_profile_launches(double *buf, int max_records) { return gemm_profile_launches(buf, max_records); }

}  // extern "C"
