// capi_fit.hip -- the fit handle of libsympgpr_hip.so: struct sgpr_fit and every sgpr_fit_* entry that takes one.  In front of the
// entries, what several of them share, once each: guard (the state an entry needs), fit_gram / fit_predict (the fit's layout to a
// kernel), fit_hyp (its hyperparameters), fit_scratch / rhs_scratch / cov_scratch (its scratch block), wait_results / check_solve
// (the wait for the results and the strip solves' give-up words); fit_map_model, the model of the d-pair map entries, stands in
// front of them.  The batched fits are in capi.hip, the map entries' checks and device traffic in capi_util.h.
#include <cmath>
#include <new>
#include <vector>
#include "capi_util.h"

using namespace sgpr;

struct sgpr_fit {
    int family = 0, npts = 0, n = 0;
    int d = 1;                 // canonical pairs per point (1 = the reference's layout)
    double hyp_nd[12] = {};    // (lq.., lP.., [p..,] sig) for d > 1
    int nhyp_nd = 0;
    double *dX = nullptr;      // all coordinates, (npts x 2d) column-major; dx = dX, dy = dX + npts
    unsigned flags = 0;
    hipStream_t st = nullptr;
    KConst kc{};
    double sig2n = 0.0;
    double *dx = nullptr, *dy = nullptr, *dz = nullptr, *dA = nullptr, *dalpha = nullptr;
    double *dscal = nullptr;  // [0] nll, [1] sum log diag
    int *dinfo = nullptr;
    void *work = nullptr;
    size_t lwork = 0;
    bool built = false, factored = false, solved = false;
    int info = 0;
    hipEvent_t ev[8] = {};    // build, factor, solve, solve_rhs: begin / end
    bool timed[4] = {false, false, false, false};
    void *rhs_scratch = nullptr;      // the block solves' scratch, kept from call to call (grown on demand, freed with the fit)
    size_t rhs_scratch_bytes = 0;
};

// What an entry needs of its handle.  guard() answers a null handle or !args_ok with SGPR_E_ARG, then the state the entry
// needs with SGPR_E_STATE, in this order; every message begins with the entry's name.
enum : unsigned { NEED_BUILT = 1, NEED_FACTOR = 2, NEED_SOLVED = 4, NEED_D1 = 8, NEED_ALL_BLOCKS = 16, NEED_PAIR_KERNEL = 32 };
constexpr unsigned ONE_BLOCK = SGPR_FIT_BLOCK_QQ | SGPR_FIT_BLOCK_PP;
static int guard(const char *entry, const sgpr_fit *f, bool args_ok, unsigned need = 0)
{
    auto fail = [&](int code, const char *what) { set_error(std::string(entry) + ": " + what); return code; };
    if (!f || !args_ok) return fail(SGPR_E_ARG, "bad arguments");
    if ((need & NEED_BUILT) && !f->built) return fail(SGPR_E_STATE, "call sgpr_fit_build first");
    if ((need & NEED_FACTOR) && !f->factored) return fail(SGPR_E_STATE, "no valid factor");
    if ((need & NEED_SOLVED) && !f->solved) return fail(SGPR_E_STATE, "not solved");
    if ((need & NEED_D1) && f->d > 1) return fail(SGPR_E_STATE, "defined for d = 1 only");
    if ((need & NEED_ALL_BLOCKS) && (f->flags & ONE_BLOCK)) return fail(SGPR_E_STATE, "not defined for a single-block fit");
    if ((need & NEED_PAIR_KERNEL) && (f->flags & SGPR_FIT_REG)) return fail(SGPR_E_STATE, "not defined for a scalar-kernel fit");
    return 0;
}

// cnt points of 2d coordinates each, coordinate c at p + c ld (d = 1: x = p, y = p + ld)
struct Points { const double *p; size_t ld; int cnt; };
static Points train_points(const sgpr_fit *f) { return {f->dX, (size_t)f->npts, f->npts}; }

// The block of the fit's kernel between row points r and column points c -- its derivative in the length `deriv`, if one is
// named (d = 1) -- plus `noise` on the diagonal, at G with leading dimension ld.  The only place that maps a fit's layout to a
// Gram kernel.  `lower`: the strict upper triangle may stay unwritten (pair layouts).
static int fit_gram(const sgpr_fit *f, Points r, Points c, double *G, size_t ld, double noise, bool lower = false,
                    int deriv = DERIV_NONE)
{
    const size_t mi = (size_t)r.cnt, mj = (size_t)c.cnt;
    if (f->d > 1)   // d canonical pairs: (2d)^2 blocks of mi x mj, block (a, b) at rows a mi, columns b mj
        return gram_nd(f->family, f->d, r.cnt, c.cnt, r.p, r.ld, c.p, c.ld, f->hyp_nd, f->nhyp_nd, G, ld, mi, mj, 0, noise, f->st);
    if (f->flags & SGPR_FIT_REG)   // buildKreg / build_dKreg  (func.py:182-183)
        return gram_reg(f->family, r.cnt, c.cnt, r.p, r.p + r.ld, c.p, c.p + c.ld, f->kc, G, ld, 0, noise, f->st, deriv);
    const unsigned opt = (lower ? SGPR_G_LOWER : 0u) | (deriv == DERIV_LX ? SGPR_G_DLX : deriv == DERIV_LY ? SGPR_G_DLY : 0u);
    if (f->flags & ONE_BLOCK)      // one diagonal block of build_K  (04_standard_map/func.py:126-135)
        return gram_pairs(f->family, r.cnt, c.cnt, r.p, r.p + r.ld, c.p, c.p + c.ld, f->kc, G, G, G, G, ld, 0, noise,
                          ((f->flags & SGPR_FIT_BLOCK_QQ) ? SGPR_G_QQ : SGPR_G_PP) | opt, f->st);
    // build_K / build_dK  (func.py:191-192), noise fused into the diagonal tiles
    return gram_pairs(f->family, r.cnt, c.cnt, r.p, r.p + r.ld, c.p, c.p + c.ld, f->kc, G, G + mi, G + ld * mj, G + mi + ld * mj,
                      ld, 0, noise, SGPR_G_ALL | opt, f->st);
}

// out (m x D, leading dimension m; D = 1 for a scalar-kernel fit, else 2d) = K*(t, training points) alpha: the only place
// that maps a fit's layout to a prediction kernel
static int fit_predict(const sgpr_fit *f, Points t, const double *alpha, double *out)
{
    const int m = t.cnt, N = f->npts;
    if (f->flags & SGPR_FIT_REG)
        return predict_reg(f->family, m, t.p, t.p + t.ld, N, f->dx, f->dy, f->kc, alpha, out, f->st);
    if (f->d == 1)
        return predict_rows(f->family, m, t.p, t.p + t.ld, N, f->dx, f->dy, f->kc, alpha, out, out + m, f->st);
    return predict_nd(f->family, f->d, m, t.p, t.ld, N, f->dX, (size_t)N, f->hyp_nd, f->nhyp_nd, alpha, out, f->st);
}

// One view of the fit's hyperparameters: the lengths l, the periods pp (zeros in a family without; d = 1 carries kc.p as it is) and
// sig as the gradient kernels take them, and vec[nhyp] = (lq.., lP.., [p..,] sig) as the d-pair kernels do, for d = 1 fits too
struct FitHyp {
    int nhyp;
    double l[6], pp[3], sig, vec[12];
};
static FitHyp fit_hyp(const sgpr_fit *f)
{
    FitHyp h{};
    const bool hasp = family_has_p(f->family);
    if (f->d > 1) {
        const int nl = 2 * f->d;
        h.nhyp = f->nhyp_nd;
        for (int m = 0; m < h.nhyp; ++m) h.vec[m] = f->hyp_nd[m];
        for (int m = 0; m < nl; ++m) h.l[m] = f->hyp_nd[m];
        for (int m = 0; m < f->d && hasp; ++m) h.pp[m] = f->hyp_nd[nl + m];
        h.sig = f->hyp_nd[h.nhyp - 1];
    } else {
        h.nhyp = hasp ? 4 : 3;
        h.l[0] = h.vec[0] = f->kc.lx; h.l[1] = h.vec[1] = f->kc.ly; h.pp[0] = f->kc.p; h.sig = f->kc.sig;
        h.vec[2] = hasp ? f->kc.p : f->kc.sig; h.vec[3] = hasp ? f->kc.sig : 0.0;
    }
    return h;
}

// scratch for a solve with nrhs right-hand sides: the fit's own block, grown when a call needs more.  (Allocating and freeing
// ~0.8 GB per call -- n = 98304 -- put milliseconds of idle device, a synchronising hipFree among them, in front of every
// solve; see sgpr_fit_solve_rhs_dev for what that does to the first launch behind it.)
static int fit_scratch(sgpr_fit_t f, size_t need, double **out)
{
    if (need > f->rhs_scratch_bytes) {
        if (f->rhs_scratch) { SGPR_HIP(hipStreamSynchronize(f->st)); (void)hipFree(f->rhs_scratch); }
        f->rhs_scratch = nullptr; f->rhs_scratch_bytes = 0;
        SGPR_HIP(hipMalloc(&f->rhs_scratch, need ? need : 8));
        f->rhs_scratch_bytes = need;
    }
    *out = static_cast<double *>(f->rhs_scratch);
    return 0;
}
static int rhs_scratch(sgpr_fit_t f, int nrhs, double **out, size_t extra = 0)
{
    return fit_scratch(f, potrs_mat_scratch(f->n, nrhs, f->dA, (size_t)f->n) + extra, out);
}

// X = L^-T L^-1 B for a device-resident B on the fit's stream, between the events of the solve_rhs stage
static int solve_rhs_device(sgpr_fit_t f, double *dB, size_t ldb, int nrhs)
{
    int rc;
    double *dS = nullptr;
    if (potrs_blocked(f->n, nrhs, f->dA, (size_t)f->n) && (rc = rhs_scratch(f, nrhs, &dS))) return rc;
    SGPR_HIP(hipEventRecord(f->ev[6], f->st));
    if ((rc = potrs_dispatch(f->n, f->dA, (size_t)f->n, f->work, dB, ldb, nrhs, dS, f->st, f->ev[7]))) return rc;
    f->timed[3] = true;
    return 0;
}

// the strip solves bound their spins: h = the 8 state words of trsv_state() once the stream has been waited for
static int strip_give_up(const char *entry, const int h[8])
{
    if (h[2] || h[6]) {
        set_error(std::string(entry) + ": a hand-off between the strips of the fit's triangular solve timed out");
        return SGPR_E_HIP;
    }
    return 0;
}

// The wait of an entry whose result copies are enqueued on the fit's stream: the strip solves' state words come back in the same
// synchronisation, so a give-up is reported at the first call that waits for the solve
static int wait_results(const char *entry, sgpr_fit_t f)
{
    int h[8] = {};
    if (trsv_uses_strips(f->n, f->dA, (size_t)f->n))
        SGPR_HIP(hipMemcpyAsync(h, trsv_state(f->n, f->work), sizeof(h), hipMemcpyDeviceToHost, f->st));
    SGPR_HIP(hipStreamSynchronize(f->st));
    return strip_give_up(entry, h);
}
// ... the same for an entry that has waited already: nothing to do unless the solve used strips
static int check_solve(const char *entry, sgpr_fit_t f)
{
    return trsv_uses_strips(f->n, f->dA, (size_t)f->n) ? wait_results(entry, f) : 0;
}

// The fit's scratch for a covariance in chunks of mc points of D outputs each, ncols = D mc right-hand-side columns: [solve scratch
// | V (n x ncols) | K** (ncols x ncols) | postcov's stage-1 partial sums], each part on a 256-byte boundary.  The solve's part is
// sized for a full chunk: a chunk of fewer columns takes the same path or, with one column, the transposed fallback, whose n
// doubles the strip scratch covers.
struct CovScratch { double *S, *V, *Kss, *part; };
static int cov_scratch(sgpr_fit_t f, int D, int mc, CovScratch *o)
{
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const int ncols = D * mc;
    const size_t n = (size_t)f->n, nc = (size_t)ncols;
    const size_t solve_raw = potrs_mat_scratch(f->n, ncols, f->dA, n), solve_b = up(solve_raw);
    const size_t v_b = up(n * nc * sizeof(double)), k_b = up(nc * nc * sizeof(double));
    const size_t p_b = up(postcov_partial_doubles(f->n, D, mc) * sizeof(double));
    const int rc = rhs_scratch(f, ncols, &o->S, solve_b - solve_raw + v_b + k_b + p_b);
    if (rc) return rc;
    char *base = reinterpret_cast<char *>(o->S);
    o->V = reinterpret_cast<double *>(base + solve_b);
    o->Kss = reinterpret_cast<double *>(base + solve_b + v_b);
    o->part = reinterpret_cast<double *>(base + solve_b + v_b + k_b);
    return 0;
}

// W (n x n, leading dimension n) = I: zeros, then one strided copy of ones onto the diagonal
static int set_identity(sgpr_fit_t f, double *w)
{
    const size_t n = (size_t)f->n;
    SGPR_HIP(hipMemsetAsync(w, 0, n * n * sizeof(double), f->st));
    std::vector<double> ones(n, 1.0);
    int rc = copy_in(w, n + 1, ones.data(), 1, 1, n, f->st);
    if (rc) return rc;
    SGPR_HIP(hipStreamSynchronize(f->st));
    return 0;
}

extern "C" {

int sgpr_fit_destroy(sgpr_fit_t f)
{
    if (!f) return 0;
    for (void *p : {(void *)f->dX, (void *)f->dz, (void *)f->dA, (void *)f->dalpha,
                    (void *)f->dscal, (void *)f->dinfo, f->work, f->rhs_scratch})
        if (p) (void)hipFree(p);
    for (auto &e : f->ev)
        if (e) (void)hipEventDestroy(e);
    delete f;
    return 0;
}

static int fit_create_common(int family, int d, int n_pts, const double *X, size_t ldx, const double *x,
                             const double *y, const double *z, const double *hyp, int nhyp, double sig2n,
                             unsigned flags, void *stream, sgpr_fit_t *out)
{
    int rc = need_device();
    if (rc) return rc;
    if (!out || n_pts <= 0 || (d == 1 ? (!x || !y) : !X)) { set_error("fit_create: bad arguments"); return SGPR_E_ARG; }
    if (flags & ~(SGPR_FIT_LOWER_ONLY | SGPR_FIT_REG | ONE_BLOCK)) { set_error("fit_create: unknown flag"); return SGPR_E_ARG; }
    if (d != 1 && (flags & SGPR_FIT_REG)) { set_error("fit_create: the scalar-kernel GP exists for d = 1 only"); return SGPR_E_ARG; }
    const unsigned single = flags & (SGPR_FIT_REG | ONE_BLOCK);
    if ((single & (single - 1)) || (d != 1 && single)) {
        set_error("fit_create: SGPR_FIT_REG / BLOCK_QQ / BLOCK_PP are mutually exclusive and need d = 1");
        return SGPR_E_ARG;
    }
    sgpr_fit *f = new (std::nothrow) sgpr_fit;
    if (!f) return SGPR_E_NOMEM;
    f->family = family; f->npts = n_pts; f->d = d; f->flags = flags;
    f->n = single ? n_pts : 2 * d * n_pts;
    f->st = static_cast<hipStream_t>(stream);
    if (d == 1) {
        if ((rc = make_kconst(family, hyp, nhyp, &f->kc))) { delete f; return rc; }
    } else {
        const int need = family_has_p(family) ? 3 * d + 1 : 2 * d + 1;
        if (d < 1 || d > 3 || nhyp != need || !hyp || family < SGPR_FAM_A || family > SGPR_FAM_USER) {
            delete f;
            set_error("fit_create_nd: d in 1..3, hyp = (lq_1..lq_d, lP_1..lP_d, sig) -- (lq.., lP.., p_1..p_d, sig) for family D");
            return SGPR_E_ARG;
        }
        for (int i = 0; i < nhyp; ++i) f->hyp_nd[i] = hyp[i];
        f->nhyp_nd = nhyp;
    }
    f->sig2n = sig2n;
    const size_t n = (size_t)f->n;
    f->lwork = potrf_workspace(f->n);
    auto fail = [&](int code) { sgpr_fit_destroy(f); return code; };
#define FIT_HIP(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return fail(hip_fail(e__, #call, __FILE__, __LINE__)); } while (0)
    FIT_HIP(hipMalloc((void **)&f->dX, (size_t)2 * d * n_pts * sizeof(double)));
    f->dx = f->dX;
    f->dy = f->dX + n_pts;
    FIT_HIP(hipMalloc((void **)&f->dz, n * sizeof(double)));
    FIT_HIP(hipMalloc((void **)&f->dalpha, n * sizeof(double)));
    FIT_HIP(hipMalloc((void **)&f->dscal, 4 * sizeof(double)));
    FIT_HIP(hipMalloc((void **)&f->dinfo, sizeof(int)));
    FIT_HIP(hipMalloc(&f->work, f->lwork));
    FIT_HIP(hipMalloc((void **)&f->dA, n * n * sizeof(double)));
    for (auto &e : f->ev) FIT_HIP(hipEventCreate(&e));
    if (d == 1) {
        FIT_HIP(hipMemcpyAsync(f->dx, x, n_pts * sizeof(double), hipMemcpyHostToDevice, f->st));
        FIT_HIP(hipMemcpyAsync(f->dy, y, n_pts * sizeof(double), hipMemcpyHostToDevice, f->st));
    } else if ((rc = copy_in(f->dX, (size_t)n_pts, X, ldx, (size_t)n_pts, (size_t)2 * d, f->st))) {
        return fail(rc);
    }
    if (z) FIT_HIP(hipMemcpyAsync(f->dz, z, n * sizeof(double), hipMemcpyHostToDevice, f->st));
    else FIT_HIP(hipMemsetAsync(f->dz, 0, n * sizeof(double), f->st));
    FIT_HIP(hipStreamSynchronize(f->st));
#undef FIT_HIP
    *out = f;
    return 0;
}

int sgpr_fit_create(int family, int n_pts, const double *x, const double *y, const double *z,
                    const double *hyp, int nhyp, double sig2n, unsigned flags, void *stream,
                    sgpr_fit_t *out)
{
    return fit_create_common(family, 1, n_pts, nullptr, 0, x, y, z, hyp, nhyp, sig2n, flags, stream, out);
}

int sgpr_fit_create_nd(int family, int d, int n_pts, const double *X, size_t ldx, const double *z,
                       const double *hyp, int nhyp, double sig2n, unsigned flags, void *stream,
                       sgpr_fit_t *out)
{
    if (d == 1) {
        if (!X || ldx < (size_t)n_pts) { set_error("fit_create_nd: bad X"); return SGPR_E_ARG; }
        return fit_create_common(family, 1, n_pts, nullptr, 0, X, X + ldx, z, hyp, nhyp, sig2n, flags, stream, out);
    }
    if (!X || ldx < (size_t)(n_pts > 0 ? n_pts : 1)) { set_error("fit_create_nd: bad X"); return SGPR_E_ARG; }
    return fit_create_common(family, d, n_pts, X, ldx, nullptr, nullptr, z, hyp, nhyp, sig2n, flags, stream, out);
}

int sgpr_fit_set_hyp(sgpr_fit_t f, const double *hyp, int nhyp, double sig2n)
{
    int rc = guard("fit_set_hyp", f, true);
    if (rc) return rc;
    if (f->d > 1) {
        if (!hyp || nhyp != f->nhyp_nd) { set_error("fit_set_hyp: hyp = (lq.., lP.., [p..,] sig)"); return SGPR_E_ARG; }
        for (int i = 0; i < nhyp; ++i) f->hyp_nd[i] = hyp[i];
    } else if ((rc = make_kconst(f->family, hyp, nhyp, &f->kc))) {
        return rc;
    }
    f->sig2n = sig2n;
    f->built = f->factored = f->solved = false;
    return 0;
}

int sgpr_fit_set_targets(sgpr_fit_t f, const double *z)
{
    int rc = guard("fit_set_targets", f, z);
    if (rc) return rc;
    SGPR_HIP(hipMemcpyAsync(f->dz, z, (size_t)f->n * sizeof(double), hipMemcpyHostToDevice, f->st));
    SGPR_HIP(hipStreamSynchronize(f->st));
    f->solved = false;
    return 0;
}

// Ky = K(x, x) + |sig2n| I between the events of the build stage
static int fit_build_impl(sgpr_fit_t f, bool lower_only)
{
    int rc = guard("fit_build", f, true);
    if (rc) return rc;
    SGPR_HIP(hipEventRecord(f->ev[0], f->st));
    if ((rc = fit_gram(f, train_points(f), train_points(f), f->dA, (size_t)f->n, std::fabs(f->sig2n), lower_only))) return rc;
    SGPR_HIP(hipEventRecord(f->ev[1], f->st));
    f->timed[0] = true;
    f->built = true;
    f->factored = f->solved = false;
    return 0;
}

int sgpr_fit_build(sgpr_fit_t f) { return fit_build_impl(f, f && (f->flags & SGPR_FIT_LOWER_ONLY)); }

/* Eigen-decomposition of Ky = K + |sig2n| I on the device (parallel cyclic Jacobi, eig.hip): the
 * positive-definiteness failure path of the drivers' nll_chol, which falls back to
 * `eigsh(Ky, neig, ...)` when cholesky raises (02_pert_pendulum/func.py:194-203).  Ky is rebuilt
 * (a failed factorisation has overwritten it), diagonalised in place, and
 * w (n, ascending eigenvalues) and c = Q^T z (n) come back; the caller forms
 * alpha = Q diag(1/w) c and the log-determinant from whichever eigenpairs it keeps.
 * Two n x n matrices in HBM.  Returns 0, or 1 if the rotations did not converge in 100 sweeps.  (The eigenvalues reach their
 * rounding floor, ~ n eps max|w|, within ~20 sweeps, but Ky has hundreds of eigenvalues crowded just above |sig2n|, and inside
 * such a cluster the off-diagonal mass falls by only ~0.8 per sweep: the 1e-14 ||Ky||_F of syev_jacobi takes ~45 sweeps at
 * n = 660 and ~56 at n = 640 of a pair fit; with the former limit of 40 those fits were reported as not converged.) */
int sgpr_fit_eig(sgpr_fit_t f, double *w, double *c)
{
    int rc = guard("fit_eig", f, w && c);
    if (rc || (rc = fit_build_impl(f, false))) return rc;
    const size_t n = (size_t)f->n;
    DevBuf V, tmp;
    if ((rc = V.alloc(n * n * sizeof(double))) || (rc = tmp.alloc(n * sizeof(double)))) return rc;
    int sweeps = 0;
    const int st = syev_jacobi(f->n, f->dA, n, V.as<double>(), n, w, 100, &sweeps, f->st);
    f->built = f->factored = f->solved = false;   // dA now holds the eigenvectors
    if (st < 0) return st;
    SGPR_HIP(hipMemsetAsync(tmp.p, 0, n * sizeof(double), f->st));
    if ((rc = gemv_t_sub(f->n, f->n, f->dA, n, f->dz, tmp.as<double>(), f->st))) return rc;   // tmp = -Q^T z
    SGPR_HIP(hipMemcpyAsync(c, tmp.p, n * sizeof(double), hipMemcpyDeviceToHost, f->st));
    SGPR_HIP(hipStreamSynchronize(f->st));
    for (size_t i = 0; i < n; ++i) c[i] = -c[i];
    if (st > 0) set_error("fit_eig: Jacobi sweeps did not converge");
    return st;
}

int sgpr_fit_factor(sgpr_fit_t f)
{
    int rc = guard("fit_factor", f, true, NEED_BUILT);
    if (rc) return rc;
    auto factor = [f]() {   // one attempt between the events of the factor stage (a retry's are the ones reported)
        SGPR_HIP(hipEventRecord(f->ev[2], f->st));
        int r = potrf(f->n, f->dA, (size_t)f->n, f->work, f->lwork, f->dinfo, f->st);
        if (r) return r;
        SGPR_HIP(hipEventRecord(f->ev[3], f->st));
        f->timed[1] = true;
        f->built = false;  // K has been overwritten by L
        return 0;
    };
    // the handle holds what Ky was built from: build it again
    auto rebuild = [f]() { return fit_build_impl(f, f->flags & SGPR_FIT_LOWER_ONLY); };
    if ((rc = factor_with_retry(factor, f->dinfo, &f->info, f->st, rebuild))) return rc;
    f->factored = f->info == 0;
    return info_status(f->info);
}

int sgpr_fit_solve(sgpr_fit_t f)
{
    int rc = guard("fit_solve", f, true, NEED_FACTOR);
    if (rc) return rc;
    const size_t n = (size_t)f->n;
    SGPR_HIP(hipEventRecord(f->ev[4], f->st));
    SGPR_HIP(hipMemcpyAsync(f->dalpha, f->dz, n * sizeof(double), hipMemcpyDeviceToDevice, f->st));
    if ((rc = potrs_vec(f->n, f->dA, n, f->work, f->dalpha, f->st))) return rc;
    if ((rc = nll_reduce(f->n, f->dA, n, f->dz, f->dalpha, f->dscal, f->st))) return rc;
    SGPR_HIP(hipEventRecord(f->ev[5], f->st));
    f->timed[2] = true;
    f->solved = true;
    return 0;
}

int sgpr_fit_run(sgpr_fit_t f)
{
    int rc = sgpr_fit_build(f);
    if (rc) return rc;
    if ((rc = sgpr_fit_factor(f))) return rc;
    return sgpr_fit_solve(f);
}

int sgpr_fit_alpha(sgpr_fit_t f, double *alpha_out)
{
    int rc = guard("fit_alpha", f, alpha_out, NEED_SOLVED);
    if (rc) return rc;
    SGPR_HIP(hipMemcpyAsync(alpha_out, f->dalpha, (size_t)f->n * sizeof(double), hipMemcpyDeviceToHost, f->st));
    return wait_results("fit_alpha", f);
}

int sgpr_fit_nll(sgpr_fit_t f, double *nll_out)
{
    int rc = guard("fit_nll", f, nll_out, NEED_SOLVED);
    if (rc) return rc;
    SGPR_HIP(hipMemcpyAsync(nll_out, f->dscal, sizeof(double), hipMemcpyDeviceToHost, f->st));
    return wait_results("fit_nll", f);
}

int sgpr_fit_ldiag(sgpr_fit_t f, double *diag_out)
{
    int rc = guard("fit_ldiag", f, diag_out, NEED_FACTOR);
    if (rc) return rc;
    DevBuf d;
    if ((rc = d.alloc((size_t)f->n * sizeof(double)))) return rc;
    if ((rc = copy_diag(f->n, f->dA, (size_t)f->n, d.as<double>(), f->st))) return rc;
    SGPR_HIP(hipMemcpyAsync(diag_out, d.p, (size_t)f->n * sizeof(double), hipMemcpyDeviceToHost, f->st));
    SGPR_HIP(hipStreamSynchronize(f->st));
    return 0;
}

int sgpr_fit_get_matrix(sgpr_fit_t f, double *A, size_t lda)
{
    int rc = guard("fit_get_matrix", f, f && A && lda >= (size_t)f->n);
    if (rc) return rc;
    if (!f->factored && !f->built) { set_error("fit_get_matrix: nothing built"); return SGPR_E_STATE; }
    const size_t n = (size_t)f->n;
    if (f->factored) {
        if ((rc = zero_strict_upper(f->n, f->dA, n, f->st))) return rc;
    } else if (f->flags & SGPR_FIT_LOWER_ONLY) {
        if ((rc = sym_fill_upper(f->n, f->dA, n, f->st))) return rc;
    }
    if ((rc = copy_out(A, lda, f->dA, n, n, n, f->st))) return rc;
    SGPR_HIP(hipStreamSynchronize(f->st));
    return 0;
}

int sgpr_fit_solve_rhs(sgpr_fit_t f, double *B, size_t ldb, int nrhs)
{
    int rc = guard("fit_solve_rhs", f, f && B && ldb >= (size_t)f->n && nrhs >= 0, NEED_FACTOR);
    if (rc || nrhs == 0) return rc;
    const size_t n = (size_t)f->n;
    DevBuf dB;
    if ((rc = dB.alloc(n * nrhs * sizeof(double)))) return rc;
    if ((rc = copy_in(dB.p, n, B, ldb, n, nrhs, f->st))) return rc;
    if ((rc = solve_rhs_device(f, dB.as<double>(), n, nrhs))) return rc;
    if ((rc = copy_out(B, ldb, dB.p, n, n, nrhs, f->st))) return rc;
    SGPR_HIP(hipStreamSynchronize(f->st));
    return 0;
}

int sgpr_fit_solve_rhs_dev(sgpr_fit_t f, double *dB, size_t ldb, int nrhs)
{
    int rc = guard("fit_solve_rhs_dev", f, f && dB && ldb >= (size_t)f->n && nrhs >= 0 && !(((uintptr_t)dB) & 7), NEED_FACTOR);
    if (rc || nrhs == 0) return rc;
    return solve_rhs_device(f, dB, ldb, nrhs);
}

int sgpr_fit_predict_rows(sgpr_fit_t f, int m, const double *q, const double *P, double *out_p,
                          double *out_q)
{
    int rc = guard("fit_predict_rows", f, m >= 0 && q && P && out_p && out_q, NEED_SOLVED | NEED_D1 | NEED_ALL_BLOCKS);
    if (rc || m == 0) return rc;
    const size_t M = (size_t)m;
    DevBuf dT, dO;   // (q | P) and (out_p | out_q); a scalar-kernel fit writes one row per test point to out_p, out_q = 0
    if ((rc = dT.alloc(2 * M * sizeof(double))) || (rc = dO.alloc(2 * M * sizeof(double)))) return rc;
    double *T = dT.as<double>(), *O = dO.as<double>();
    SGPR_HIP(hipMemcpyAsync(T, q, M * sizeof(double), hipMemcpyHostToDevice, f->st));
    SGPR_HIP(hipMemcpyAsync(T + M, P, M * sizeof(double), hipMemcpyHostToDevice, f->st));
    SGPR_HIP(hipMemsetAsync(O + M, 0, M * sizeof(double), f->st));
    if ((rc = fit_predict(f, {T, M, m}, f->dalpha, O))) return rc;
    SGPR_HIP(hipMemcpyAsync(out_p, O, M * sizeof(double), hipMemcpyDeviceToHost, f->st));
    SGPR_HIP(hipMemcpyAsync(out_q, O + M, M * sizeof(double), hipMemcpyDeviceToHost, f->st));
    SGPR_HIP(hipStreamSynchronize(f->st));
    return 0;
}

int sgpr_fit_inverse(sgpr_fit_t f, double *Kyinv, size_t ld)
{
    int rc = guard("fit_inverse", f, f && Kyinv && ld >= (size_t)f->n, NEED_FACTOR);
    if (rc) return rc;
    const size_t n = (size_t)f->n;
    DevBuf W, R;
    if ((rc = W.alloc(n * n * sizeof(double))) || (rc = R.alloc(n * n * sizeof(double)))) return rc;
    double *w = W.as<double>(), *r = R.as<double>();
    if ((rc = set_identity(f, w))) return rc;
    if ((rc = trsm_rlt(f->n, f->n, f->dA, n, w, n, f->work, f->st))) return rc;            // W = L^-T
    if ((rc = gemm_nt(f->n, f->n, f->n, 1.0, w, n, w, n, 0.0, r, n, 1, 0, f->st))) return rc;  // lower(W W^T)
    if ((rc = sym_fill_upper(f->n, r, n, f->st))) return rc;
    if ((rc = copy_out(Kyinv, ld, r, n, n, n, f->st))) return rc;
    SGPR_HIP(hipStreamSynchronize(f->st));
    return 0;
}

/* d nll / d(lx, ly) as nll_grad / nll_grad_reg compute it (functions/func.py:132-162):
 *   grad_i = -1/2 alpha^T dK_i alpha + 1/2 tr(Ky^-1 dK_i).
 * The reference forms Ky^-1 explicitly; here tr(Ky^-1 dK) = tr(L^-1 dK L^-T): W = dK, W := W L^-T
 * (panel solve), W := W^T (= L^-1 dK by symmetry), W := W L^-T again, sum of the diagonal --
 * 2 n^3 flop per length scale on the MFMA kernel, two n x n scratch matrices. */
static int nll_grad_core(const char *entry, sgpr_fit_t f, double *h)
{
    int rc = guard(entry, f, h, NEED_SOLVED | NEED_D1 | NEED_ALL_BLOCKS);
    if (rc) return rc;
    const size_t n = (size_t)f->n;
    DevBuf W, T, tmp, sc;
    if ((rc = W.alloc(n * n * sizeof(double))) || (rc = T.alloc(n * n * sizeof(double))) ||
        (rc = tmp.alloc(n * sizeof(double))) || (rc = sc.alloc(4 * sizeof(double))))
        return rc;
    double *w = W.as<double>(), *t = T.as<double>(), *s = sc.as<double>();
    for (int which = 0; which < 2; ++which) {
        if ((rc = fit_gram(f, train_points(f), train_points(f), w, n, 0.0, false, which ? DERIV_LY : DERIV_LX))) return rc;
        // alpha^T dK alpha
        SGPR_HIP(hipMemsetAsync(tmp.p, 0, n * sizeof(double), f->st));
        if ((rc = gemv_n_sub(f->n, f->n, w, n, f->dalpha, tmp.as<double>(), f->st))) return rc;  // tmp = -dK alpha
        if ((rc = dot(f->n, tmp.as<double>(), f->dalpha, s + 2 * which, f->st))) return rc;
        // tr(L^-1 dK L^-T)
        if ((rc = trsm_rlt(f->n, f->n, f->dA, n, w, n, f->work, f->st))) return rc;
        if ((rc = transpose(f->n, f->n, w, n, t, n, f->st))) return rc;
        if ((rc = trsm_rlt(f->n, f->n, f->dA, n, t, n, f->work, f->st))) return rc;
        if ((rc = trace(f->n, t, n, s + 2 * which + 1, f->st))) return rc;
    }
    SGPR_HIP(hipMemcpyAsync(h, s, 4 * sizeof(double), hipMemcpyDeviceToHost, f->st));
    SGPR_HIP(hipStreamSynchronize(f->st));
    h[0] = -h[0];   // the GEMV helper subtracts: s[0], s[2] hold -(alpha^T dK alpha)
    h[2] = -h[2];
    return 0;
}

int sgpr_fit_nll_grad(sgpr_fit_t f, double *grad2)
{
    double h[4];
    int rc = nll_grad_core("fit_nll_grad", f, grad2 ? h : nullptr);
    if (rc) return rc;
    for (int which = 0; which < 2; ++which) grad2[which] = -0.5 * h[2 * which] + 0.5 * h[2 * which + 1];
    return 0;
}

/* The pieces the per-example nll_grad variants recombine (03_henon_heiles/func.py:168-192,
 * 05_tokamak/SympGPR/func.py:152-168: a third component built from dK/dsig = K / sig):
 * terms5 = [alpha^T dK_lx alpha, tr(Ky^-1 dK_lx), alpha^T dK_ly alpha, tr(Ky^-1 dK_ly), tr(Ky^-1)].
 * tr(Ky^-1) = ||L^-1||_F^2 from a panel solve on the identity. */
int sgpr_fit_nll_grad_terms(sgpr_fit_t f, double *terms5)
{
    int rc = nll_grad_core("fit_nll_grad_terms", f, terms5);
    if (rc) return rc;
    const size_t n = (size_t)f->n;
    DevBuf W, sc;
    if ((rc = W.alloc(n * n * sizeof(double))) || (rc = sc.alloc((SUMSQ_SCRATCH + 1) * sizeof(double)))) return rc;
    double *w = W.as<double>();
    if ((rc = set_identity(f, w))) return rc;
    if ((rc = trsm_rlt(f->n, f->n, f->dA, n, w, n, f->work, f->st))) return rc;            // W = L^-T
    if ((rc = sumsq(n * n, w, sc.as<double>() + 1, sc.as<double>(), f->st))) return rc;
    SGPR_HIP(hipMemcpyAsync(terms5 + 4, sc.p, sizeof(double), hipMemcpyDeviceToHost, f->st));
    SGPR_HIP(hipStreamSynchronize(f->st));
    return 0;
}

/* The gradient of the NLL in every hyperparameter and sig2n (nllgrad.hip): Ky^-1 by row panels on the trailing blocks of
 * the cached factor, each panel contracted with dK evaluated pair by pair; the raw sums come back and are scaled here --
 * the lengths and periods by sig / 2 (the kernels differentiate k without sig), sig by 1/2, sig2n by sign(sig2n) / 2. */
int sgpr_fit_nll_grad_full(sgpr_fit_t f, double *grad, int ngrad)
{
    int rc = guard("fit_nll_grad_full", f, grad);
    if (rc) return rc;
    const FitHyp hy = fit_hyp(f);
    const int nhyp = hy.nhyp, nacc = nhyp + 1;
    if (ngrad != nhyp + 1) { set_error("fit_nll_grad_full: ngrad must be nhyp + 1 = " + std::to_string(nhyp + 1)); return SGPR_E_ARG; }
    if ((rc = guard("fit_nll_grad_full", f, true, NEED_SOLVED | NEED_ALL_BLOCKS))) return rc;
    DevBuf S, O;
    if ((rc = S.alloc(nll_grad_full_scratch(f->n, f->npts, nacc))) || (rc = O.alloc(nacc * sizeof(double)))) return rc;
    if ((rc = nll_grad_full(f->family, f->d, f->flags & SGPR_FIT_REG, f->npts, f->n, f->dA, (size_t)f->n, f->work, f->dX, f->dalpha,
                            hy.l, hy.pp, nacc, S.as<double>(), O.as<double>(), f->st)))
        return rc;
    double raw[12];
    SGPR_HIP(hipMemcpyAsync(raw, O.p, nacc * sizeof(double), hipMemcpyDeviceToHost, f->st));
    if ((rc = wait_results("fit_nll_grad_full", f))) return rc;
    scale_grad_sums(raw, nhyp, hy.sig, f->sig2n, grad);
    return 0;
}

/* Leave-one-point-out cross-validation of a solved fit (loo.hip): Ky^-1 by the row panels of the gradient, the D x D diagonal
 * block of every point copied out of the panel that holds it, then one thread per point.  The factor, alpha, nll and the
 * workspace are only read; the scratch is the fit's own block (sgpr_fit_trim gives it back). */
int sgpr_fit_loo(sgpr_fit_t f, double *loo2, double *resid, double *cov, double *lpd)
{
    int rc = guard("fit_loo", f, loo2, NEED_SOLVED | NEED_ALL_BLOCKS);
    if (rc) return rc;
    const int D = (f->flags & SGPR_FIT_REG) ? 1 : 2 * f->d, N = f->npts;
    const LooLayout o = loo_layout(f->n, N, D);
    double *S;
    if ((rc = fit_scratch(f, o.total * sizeof(double), &S))) return rc;
    if ((rc = fit_loo(D, N, f->n, f->dA, (size_t)f->n, f->work, f->dalpha, S, f->st))) return rc;
    SGPR_HIP(hipMemcpyAsync(loo2, S + o.sums, 2 * sizeof(double), hipMemcpyDeviceToHost, f->st));
    if (resid) SGPR_HIP(hipMemcpyAsync(resid, S + o.resid, (size_t)f->n * sizeof(double), hipMemcpyDeviceToHost, f->st));
    if (cov) SGPR_HIP(hipMemcpyAsync(cov, S + o.cov, (size_t)N * D * D * sizeof(double), hipMemcpyDeviceToHost, f->st));
    if (lpd) SGPR_HIP(hipMemcpyAsync(lpd, S + o.lpd, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, f->st));
    return wait_results("fit_loo", f);
}

/* The gradient of loo or press in every hyperparameter and sig2n (loograd.hip): the dense Ky^-1, one weight matrix
 * M = Ky^-1 W Ky^-1 by row panels, each contracted with dK by the rank-2 instances of nllgrad.hip's kernels; the raw sums
 * are scaled as sgpr_fit_nll_grad_full scales its own.  The scratch is the fit's own block: a block that is too small is
 * replaced only once the larger one exists, so a failed allocation leaves the handle as it was. */
int sgpr_fit_loo_grad(sgpr_fit_t f, int which, double *value, double *grad, int ngrad)
{
    int rc = guard("fit_loo_grad", f, value && grad);
    if (rc) return rc;
    const FitHyp hy = fit_hyp(f);
    const int nhyp = hy.nhyp, nacc = nhyp + 1;
    if (ngrad != nhyp + 1) { set_error("fit_loo_grad: ngrad must be nhyp + 1 = " + std::to_string(nhyp + 1)); return SGPR_E_ARG; }
    if (which != SGPR_LOO_LPD && which != SGPR_LOO_PRESS) { set_error("fit_loo_grad: which must be SGPR_LOO_LPD or SGPR_LOO_PRESS"); return SGPR_E_ARG; }
    if ((rc = guard("fit_loo_grad", f, true, NEED_SOLVED | NEED_ALL_BLOCKS))) return rc;
    const bool reg = f->flags & SGPR_FIT_REG;
    const int d = f->d, D = reg ? 1 : 2 * d;
    const LooGradLayout o = loo_grad_layout(f->n, f->npts, D, nacc);
    const size_t need = o.total * sizeof(double);
    if (need > f->rhs_scratch_bytes) {
        void *p = nullptr;
        if (hipMalloc(&p, need) != hipSuccess) {
            (void)hipGetLastError();
            set_error("fit_loo_grad: " + std::to_string(need) + " bytes of device scratch (two n x n blocks and a panel) do not fit");
            return SGPR_E_NOMEM;
        }
        if (f->rhs_scratch) { SGPR_HIP(hipStreamSynchronize(f->st)); (void)hipFree(f->rhs_scratch); }
        f->rhs_scratch = p;
        f->rhs_scratch_bytes = need;
    }
    double *S = static_cast<double *>(f->rhs_scratch);
    if ((rc = fit_loo_grad(f->family, d, reg, which, f->npts, f->n, f->dA, (size_t)f->n, f->work, f->dX, f->dalpha, hy.l, hy.pp, nacc,
                           S, f->st)))
        return rc;
    double raw[13];
    SGPR_HIP(hipMemcpyAsync(raw, S + o.sums, (nacc + 1) * sizeof(double), hipMemcpyDeviceToHost, f->st));
    if ((rc = wait_results("fit_loo_grad", f))) return rc;
    *value = which == SGPR_LOO_LPD ? -raw[nacc] : raw[nacc];
    scale_grad_sums(raw, nhyp, hy.sig, f->sig2n, grad);
    if (std::isnan(*value))   // a point without a positive definite block: its NaN reaches every sum through M; made explicit
        for (int k = 0; k <= nhyp; ++k) grad[k] = *value;
    return 0;
}

/* K*(2d x 2d N) . alpha for m test points Xt (m x 2d, column-major, leading dimension ldxt):
 * out (m x 2d, column-major, ld m): column a = predicted d F / d x_a.  The d-pair kernel reads alpha as 2d blocks of n_pts
 * entries: a scalar-kernel or single-block fit has one such block and is refused, as by the other pair predictions. */
int sgpr_fit_predict_nd(sgpr_fit_t f, int m, const double *Xt, size_t ldxt, double *out)
{
    int rc = guard("fit_predict_nd", f, m >= 0 && Xt && out && ldxt >= (size_t)(m > 0 ? m : 1),
                   NEED_SOLVED | NEED_ALL_BLOCKS | NEED_PAIR_KERNEL);
    if (rc || m == 0) return rc;
    const int D = 2 * f->d;
    DevBuf dT, dO;
    if ((rc = dT.alloc((size_t)m * D * sizeof(double))) || (rc = dO.alloc((size_t)m * D * sizeof(double)))) return rc;
    if ((rc = copy_in(dT.p, (size_t)m, Xt, ldxt, (size_t)m, D, f->st))) return rc;
    const FitHyp hy = fit_hyp(f);   // the d-pair kernel whatever the fit's layout: d = 1 too
    if ((rc = predict_nd(f->family, f->d, m, dT.as<double>(), (size_t)m, f->npts, f->dX, (size_t)f->npts, hy.vec, hy.nhyp, f->dalpha,
                         dO.as<double>(), f->st)))
        return rc;
    SGPR_HIP(hipMemcpyAsync(out, dO.p, (size_t)m * D * sizeof(double), hipMemcpyDeviceToHost, f->st));
    SGPR_HIP(hipStreamSynchronize(f->st));
    return 0;
}

/* Posterior mean and covariance (latent prior, no noise) at m test points, in chunks of mc = 256 / D points:
 *   mean = K* alpha by the prediction kernels (one launch over all m: the bits of sgpr_fit_predict_rows / _nd);
 *   per chunk  V = K*^T (n x D mc, the Gram kernels with the training points as rows, noise 0; point t's output a in column
 *              a mc + t),  V := L^-1 V (potrs_mat_fwd: the strip solves' forward passes, 64 columns each),
 *              K** = the chunk's test x test Gram block (D mc x D mc, same index map), cov_t = K**_t - V_t^T V_t (postcov.hip).
 * Scratch: the fit's rhs_scratch, [solve scratch | V | K** | stage-1 partial sums]. */
int sgpr_fit_predict_cov(sgpr_fit_t f, int m, const double *Xt, size_t ldxt, double *mean, double *cov)
{
    int rc = guard("fit_predict_cov", f, m >= 0 && Xt && mean && cov && ldxt >= (size_t)(m > 0 ? m : 1),
                   NEED_SOLVED | NEED_ALL_BLOCKS);
    if (rc || m == 0) return rc;
    const int D = (f->flags & SGPR_FIT_REG) ? 1 : 2 * f->d, nx = 2 * f->d;
    const int mc = POSTCOV_COLS / D;
    const size_t n = (size_t)f->n;
    DevBuf dT, dM, dC;
    if ((rc = dT.alloc((size_t)m * nx * sizeof(double))) || (rc = dM.alloc((size_t)m * D * sizeof(double))) ||
        (rc = dC.alloc((size_t)m * D * D * sizeof(double))))
        return rc;
    double *T = dT.as<double>(), *M = dM.as<double>(), *C = dC.as<double>();
    if ((rc = copy_in(T, (size_t)m, Xt, ldxt, (size_t)m, nx, f->st))) return rc;
    if ((rc = fit_predict(f, {T, (size_t)m, m}, f->dalpha, M))) return rc;
    CovScratch cs;
    if ((rc = cov_scratch(f, D, mc, &cs))) return rc;
    double *S = cs.S, *V = cs.V, *Kss = cs.Kss, *part = cs.part;
    for (int c0 = 0; c0 < m; c0 += mc) {
        const int cnt = m - c0 < mc ? m - c0 : mc, ncols = D * cnt;
        const Points chunk = {T + c0, (size_t)m, cnt};
        const size_t kld = (size_t)ncols;
        if ((rc = fit_gram(f, train_points(f), chunk, V, n, 0.0))) return rc;
        if ((rc = potrs_mat_fwd(f->n, f->dA, n, f->work, V, n, ncols, S, f->st))) return rc;
        if ((rc = fit_gram(f, chunk, chunk, Kss, kld, 0.0))) return rc;
        if ((rc = postcov(D, f->n, cnt, V, n, Kss, kld, part, C + (size_t)c0 * D * D, f->st))) return rc;
        // waits for the chunk; the next chunk's solve clears the give-up words, so they are read here
        if ((rc = solve_status(f->n, f->dA, n, f->work, f->st))) return rc;
    }
    SGPR_HIP(hipMemcpyAsync(mean, M, (size_t)m * D * sizeof(double), hipMemcpyDeviceToHost, f->st));
    SGPR_HIP(hipMemcpyAsync(cov, C, (size_t)m * D * D * sizeof(double), hipMemcpyDeviceToHost, f->st));
    SGPR_HIP(hipStreamSynchronize(f->st));
    return 0;
}

/* The generating function F itself at m test points (genfun_nd.hip: genfun_nd_kernel), relative to `ref` if one is given, and
 * with `var` its latent posterior variance, in chunks of mc = 256 points:
 *   per chunk  V = the cross-covariance columns v_t - v_0 (n x mc, genfun_cross_kernel) and the prior of F(x_t) - F(x_0),
 *              V := L^-1 V (potrs_mat_fwd, as sgpr_fit_predict_cov), var_t = prior_t - |V_t|^2 (postcov.hip with D = 1: the
 *              priors lie on the diagonal of its K** argument, so its kernels serve as they are).
 * The reference point travels as row m of the uploaded points.  Scratch: the fit's rhs_scratch, [solve scratch | V | the
 * 256 x 256 block whose diagonal holds the priors | stage-1 partial sums].  The factor, alpha, nll and the workspace are only read. */
int sgpr_fit_predict_genfun(sgpr_fit_t f, int m, const double *Xt, size_t ldxt, const double *ref, double *F, double *var)
{
    const char *me = "fit_predict_genfun";
    int rc = guard(me, f, m >= 0 && ldxt >= (size_t)(m > 0 ? m : 1) && (m == 0 || (Xt && F)));
    if (rc) return rc;
    if (f->flags & SGPR_FIT_REG) {
        set_error("fit_predict_genfun: a scalar-kernel fit models F itself: sgpr_fit_predict_rows returns it");
        return SGPR_E_ARG;
    }
    if ((rc = guard(me, f, true, NEED_SOLVED | NEED_ALL_BLOCKS)) || m == 0) return rc;
    const int D = 2 * f->d, mc = POSTCOV_COLS;
    const size_t n = (size_t)f->n, M1 = (size_t)m + 1;
    DevBuf dT, dF, dVar;
    if ((rc = dT.alloc(M1 * D * sizeof(double))) || (rc = dF.alloc(M1 * sizeof(double))) ||
        (var && (rc = dVar.alloc((size_t)m * sizeof(double)))))
        return rc;
    double *T = dT.as<double>(), *Fd = dF.as<double>(), *Vr = dVar.as<double>();
    if ((rc = copy_in(T, M1, Xt, ldxt, (size_t)m, D, f->st))) return rc;
    if (ref && (rc = copy_in(T + m, M1, ref, 1, 1, D, f->st))) return rc;
    const double *x0 = ref ? T + m : nullptr;
    const FitHyp hy = fit_hyp(f);   // the d-pair kernels whatever the fit's layout: d = 1 too
    const double *hyp = hy.vec;
    const int nhyp = hy.nhyp;
    if ((rc = genfun_nd(f->family, f->d, m, T, M1, ref != nullptr, f->npts, f->dX, (size_t)f->npts, hyp, nhyp, f->dalpha, Fd, f->st)))
        return rc;
    if (var) {
        CovScratch cs;   // D = 1: 256 columns, the priors on the diagonal of K**
        if ((rc = cov_scratch(f, 1, mc, &cs))) return rc;
        double *S = cs.S, *V = cs.V, *Kss = cs.Kss, *part = cs.part;
        for (int c0 = 0; c0 < m; c0 += mc) {
            const int cnt = m - c0 < mc ? m - c0 : mc;
            if ((rc = genfun_cross_nd(f->family, f->d, cnt, T + c0, M1, x0, M1, f->npts, f->dX, (size_t)f->npts, hyp, nhyp, V, n, Kss,
                                      (size_t)mc + 1, f->st)))
                return rc;
            int ncols = cnt;
            if (cnt == 1) {   // a single column would take another solve path than a block (potrs_mat_uses_strips) and get
                              // other bits than the same point has inside a larger call: a column of zeros rides along
                SGPR_HIP(hipMemsetAsync(V + n, 0, n * sizeof(double), f->st));
                ncols = 2;
            }
            if ((rc = potrs_mat_fwd(f->n, f->dA, n, f->work, V, n, ncols, S, f->st))) return rc;
            if ((rc = postcov(1, f->n, cnt, V, n, Kss, (size_t)mc, part, Vr + c0, f->st))) return rc;
            // waits for the chunk; the next chunk's solve clears the give-up words, so they are read here
            if ((rc = solve_status(f->n, f->dA, n, f->work, f->st))) return rc;
        }
        SGPR_HIP(hipMemcpyAsync(var, Vr, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, f->st));
    }
    SGPR_HIP(hipMemcpyAsync(F, Fd, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, f->st));
    SGPR_HIP(hipStreamSynchronize(f->st));
    return 0;
}

/* The last check of a d-pair map entry, the state of its handle, and the model (capi_util.h: MapModel) its launch takes: the fit's
 * own device-resident training points and alpha on its stream, the hyperparameters of `hy`; d = 1 fits run the D = 2 instance of
 * the d-pair kernels. */
static int fit_map_model(const char *me, const sgpr_fit *f, FitHyp &hy, MapModel *m)
{
    const int rc = guard(me, f, true, NEED_SOLVED | NEED_ALL_BLOCKS | NEED_PAIR_KERNEL);
    if (rc) return rc;
    hy = fit_hyp(f);
    *m = MapModel{f->family, f->d, f->npts, f->dX, (size_t)f->npts, hy.vec, hy.nhyp, f->dalpha, f->st};
    return 0;
}

/* nm steps of the fit's symplectic map (map_nd.hip: applymap_nd_kernel) for ntest orbits.  alpha is the strip solves' result: a
 * give-up there is reported by the first call that waits (as sgpr_fit_alpha), so every map entry ends on check_solve. */
int sgpr_fit_applymap_nd(sgpr_fit_t f, int mode, int nm, int ntest, const double *Q0, size_t ldq, const double *P0, size_t ldp,
                         double *qmap, double *pmap, int *iters)
{
    const char *me = "fit_applymap_nd";
    FitHyp hy;
    MapModel m;
    int rc = guard(me, f, true);
    if (rc || (rc = applymap_nd_call_check(me, mode, nm, ntest, Q0, ldq, P0, ldp, qmap, pmap)) || (rc = fit_map_model(me, f, hy, &m)) ||
        ntest == 0 || (rc = applymap_nd_io(m, mode, nm, ntest, Q0, ldq, P0, ldp, qmap, pmap, iters)))
        return rc;
    return check_solve(me, f);
}

/* The same with the tangent map (maptan.h): the orbit outputs have the bits of sgpr_fit_applymap_nd. */
int sgpr_fit_applymap_nd_tangent(sgpr_fit_t f, int mode, int nm, int ntest, const double *Q0, size_t ldq, const double *P0,
                                 size_t ldp, double *qmap, double *pmap, int *iters, double *jac, double *mono, double *lyap)
{
    const char *me = "fit_applymap_nd_tangent";
    const MapTangentOut tan = {jac, mono, lyap};
    FitHyp hy;
    MapModel m;
    int rc = guard(me, f, true);
    if (rc || (rc = applymap_nd_call_check(me, mode, nm, ntest, Q0, ldq, P0, ldp, qmap, pmap)) ||
        (rc = applymap_nd_tangent_check(me, f->family, mode, nm, lyap)) || (rc = fit_map_model(me, f, hy, &m)) || ntest == 0 ||
        (rc = applymap_nd_io(m, mode, nm, ntest, Q0, ldq, P0, ldp, qmap, pmap, iters, &tan)))
        return rc;
    return check_solve(me, f);
}

/* The backward orbit of the same map (map_nd.hip: applymap_nd_inverse_kernel): Q0 / P0 hold the images, row i the i-th preimage. */
int sgpr_fit_applymap_nd_inverse(sgpr_fit_t f, int mode, int nm, int ntest, const double *Q0, size_t ldq, const double *P0,
                                 size_t ldp, double *qmap, double *pmap, int *iters)
{
    const char *me = "fit_applymap_nd_inverse";
    FitHyp hy;
    MapModel m;
    int rc = guard(me, f, true);
    if (rc || (rc = applymap_nd_call_check(me, mode, nm, ntest, Q0, ldq, P0, ldp, qmap, pmap)) ||
        (rc = applymap_nd_inverse_check(me, mode)) || (rc = fit_map_model(me, f, hy, &m)) || ntest == 0 ||
        (rc = applymap_nd_io(m, mode, nm, ntest, Q0, ldq, P0, ldp, qmap, pmap, iters, nullptr, MAP_BACKWARD)))
        return rc;
    return check_solve(me, f);
}

/* Periodic orbits of the same map (periodic_nd.h: periodic_nd_kernel): Newton on the n-fold map from every guess, one launch. */
int sgpr_fit_periodic_nd(sgpr_fit_t f, int mode, int n, int ntest, const int *wind, const double *Q0, size_t ldq, const double *P0,
                         size_t ldp, double tol, int maxit, double *z, double *resid, int *its, double *mono, double *qorb,
                         double *porb)
{
    const char *me = "fit_periodic_nd";
    FitHyp hy;
    MapModel m;
    int rc = guard(me, f, true);
    if (rc || (rc = periodic_nd_call_check(me, mode, n, ntest, Q0, ldq, P0, ldp, tol, maxit, z, resid, its, qorb, porb)) ||
        (rc = applymap_nd_tangent_check(me, f->family, mode, n + 1, nullptr)) || (rc = fit_map_model(me, f, hy, &m)) || ntest == 0 ||
        (rc = periodic_nd_io(m, mode, n, ntest, wind, Q0, ldq, P0, ldp, tol, maxit, z, resid, its, mono, qorb, porb)))
        return rc;
    return check_solve(me, f);
}

// cond_2(Ky) from below: lambda_max by power iteration on Ky v (the rows of K are re-evaluated from the training points by the
// prediction kernel -- the matrix itself has been overwritten by its factor -- plus |sig2n| v), lambda_min by inverse iteration
// with the cached factor (two strip solves per step).  Both are Rayleigh quotients of unit vectors, so lambda_max is a lower
// and lambda_min an upper bound: the estimate never exceeds the true condition number.  Vector arithmetic on the host (n
// doubles per step); out4 = {lambda_max, lambda_min, cond, relative change of the two quotients in their last step (the larger)}.
// "report cond (or a Lanczos estimate) next to every parity number".
int sgpr_fit_cond_estimate(sgpr_fit_t f, int iters, double *out4)
{
    int rc = guard("fit_cond_estimate", f, out4 && iters >= 1, NEED_FACTOR | NEED_ALL_BLOCKS);
    if (rc) return rc;
    const size_t n = (size_t)f->n;
    DevBuf dv, dw;
    if ((rc = dv.alloc(n * sizeof(double))) || (rc = dw.alloc(n * sizeof(double)))) return rc;
    std::vector<double> v(n), w(n);
    unsigned long long lcg = 0x9E3779B97F4A7C15ull;
    double nrm = 0.0;
    for (size_t i = 0; i < n; ++i) {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        v[i] = (double)(lcg >> 11) / 9007199254740992.0 - 0.5;
        nrm += v[i] * v[i];
    }
    nrm = std::sqrt(nrm);
    for (size_t i = 0; i < n; ++i) v[i] /= nrm;
    const std::vector<double> v0 = v;
    auto normalise = [&](const std::vector<double> &src, std::vector<double> &dst, double &quot) {
        double dot = 0.0, nn = 0.0;
        for (size_t i = 0; i < n; ++i) { dot += dst[i] * src[i]; nn += src[i] * src[i]; }
        quot = dot;                                     // v^T (M v), |v| = 1
        nn = std::sqrt(nn);
        for (size_t i = 0; i < n; ++i) dst[i] = src[i] / nn;
    };
    double lmax = 0.0, lmin_inv = 0.0, ch_max = 1.0, ch_min = 1.0;
    for (int it = 0; it < iters; ++it) {                // ---- lambda_max
        SGPR_HIP(hipMemcpyAsync(dv.p, v.data(), n * sizeof(double), hipMemcpyHostToDevice, f->st));
        if ((rc = fit_predict(f, train_points(f), dv.as<double>(), dw.as<double>()))) return rc;
        SGPR_HIP(hipMemcpyAsync(w.data(), dw.p, n * sizeof(double), hipMemcpyDeviceToHost, f->st));
        SGPR_HIP(hipStreamSynchronize(f->st));
        const double s2 = std::fabs(f->sig2n);
        for (size_t i = 0; i < n; ++i) w[i] += s2 * v[i];
        double q;
        normalise(w, v, q);
        ch_max = lmax > 0.0 ? std::fabs(q - lmax) / q : 1.0;
        lmax = q;
    }
    v = v0;
    for (int it = 0; it < iters; ++it) {                // ---- 1 / lambda_min
        SGPR_HIP(hipMemcpyAsync(dw.p, v.data(), n * sizeof(double), hipMemcpyHostToDevice, f->st));
        if ((rc = potrs_vec(f->n, f->dA, n, f->work, dw.as<double>(), f->st))) return rc;
        if ((rc = solve_status(f->n, f->dA, n, f->work, f->st))) return rc;
        SGPR_HIP(hipMemcpyAsync(w.data(), dw.p, n * sizeof(double), hipMemcpyDeviceToHost, f->st));
        SGPR_HIP(hipStreamSynchronize(f->st));
        double q;
        normalise(w, v, q);
        ch_min = lmin_inv > 0.0 ? std::fabs(q - lmin_inv) / q : 1.0;
        lmin_inv = q;
    }
    out4[0] = lmax;
    out4[1] = lmin_inv > 0.0 ? 1.0 / lmin_inv : 0.0;
    out4[2] = lmax * lmin_inv;
    out4[3] = ch_max > ch_min ? ch_max : ch_min;
    return 0;
}

int sgpr_fit_trim(sgpr_fit_t f)
{
    int rc = guard("fit_trim", f, true);
    if (rc) return rc;
    if (f->rhs_scratch) {
        SGPR_HIP(hipStreamSynchronize(f->st));
        (void)hipFree(f->rhs_scratch);
        f->rhs_scratch = nullptr;
        f->rhs_scratch_bytes = 0;
    }
    return 0;
}

int sgpr_fit_stage_ms(sgpr_fit_t f, double *build_ms, double *factor_ms, double *solve_ms)
{
    int rc = guard("fit_stage_ms", f, true);
    if (rc) return rc;
    SGPR_HIP(hipStreamSynchronize(f->st));
    double *outs[3] = {build_ms, factor_ms, solve_ms};
    for (int s = 0; s < 3; ++s) {
        if (!outs[s]) continue;
        float ms = -1.0f;
        if (f->timed[s]) SGPR_HIP(hipEventElapsedTime(&ms, f->ev[2 * s], f->ev[2 * s + 1]));
        *outs[s] = ms;
    }
    return 0;
}

int sgpr_fit_solve_rhs_ms(sgpr_fit_t f, double *ms_out)
{
    int rc = guard("fit_solve_rhs_ms", f, ms_out);
    if (rc) return rc;
    SGPR_HIP(hipStreamSynchronize(f->st));
    float ms = -1.0f;
    if (f->timed[3]) SGPR_HIP(hipEventElapsedTime(&ms, f->ev[6], f->ev[7]));
    *ms_out = ms;
    return 0;
}

int sgpr_fit_device_ptrs(sgpr_fit_t f, void **dA, size_t *lda, void **dalpha)
{
    int rc = guard("fit_device_ptrs", f, true);
    if (rc) return rc;
    if (dA) *dA = f->dA;
    if (lda) *lda = (size_t)f->n;
    if (dalpha) *dalpha = f->dalpha;
    return 0;
}

}  // extern "C"
