// genfun_nd.hip -- the generating function F itself of a fit with d canonical pairs per point, of which the prediction and the
// map (gram_nd.hip, map_nd.hip) return derivatives.
//
// The observations are (dF/dq, dF/dP), so cov(F(x*), observation c of training point j) = d(sig k)/dx_train,c = E_c g_c with
// dx = x_train - x* (E = sig k, g = f'/f per coordinate: nd_eval.h), and
//     F(x*) = sum_j sum_c E_c g_c alpha_{cN+j}     (product kernels: sum_j E S, S = sum_c g_c alpha_{cN+j}),
// whose gradient in x* is K*(x*) alpha as predict_nd_kernel forms it.  The prior of F is kappa(x, x') = sig k(x, x').
#include <type_traits>
#include "common.h"
#include "devmath.h"
#include "generated/pair_generated.h"
#include "nd_args.h"

namespace sgpr {

namespace {

using namespace nd;         // all_coords, weights, is_sum, dispatch_nd (nd_eval.h); NT, NdArgs, fill_args (nd_args.h); finite_d (devmath.h)

constexpr int GF_WAVES = NT / 64;   // test points per workgroup of the mean kernel: one wave each
constexpr int GF_CT = 16;           // test points a thread of the cross kernel walks through (NTJ of the Gram kernel)

// one (training point xa, test point xb) pair: v[c] = E_c g_c, the summand of F without alpha, and kap = sig k(xa, xb)
template <int FAM, int D>
__device__ __forceinline__ void genfun_pair(const NdArgs &a, const double *xa, const double (&xb)[D], double (&v)[D], double &kap)
{
    double arg[D], g[D], nh[D], E[D];
    all_coords<FAM, D>(a.c, xa, xb, arg, g, nh);
    weights<FAM, D>(a.c, arg, E);
    kap = E[0];
    if constexpr (is_sum<FAM>()) {
#pragma unroll
        for (int c = 1; c < D; ++c) kap += E[c];
    }
#pragma unroll
    for (int c = 0; c < D; ++c) v[c] = E[c] * g[c];
}

template <int D>
__device__ __forceinline__ bool load_point(const double *X, size_t ld, size_t row, double (&x)[D])
{
    bool ok = true;
#pragma unroll
    for (int c = 0; c < D; ++c) { x[c] = X[row + (size_t)c * ld]; ok = ok && finite_d(x[c]); }
    return ok;
}

// F (a.mi values) for the test points Xb: one wave per point, the lanes on consecutive training points, one sum per lane folded
// by shuffles alone -- no LDS, no barrier, no atomics, so a point's bits depend on n0 and on nothing else of the call.  (The
// drivers' n0 = 20 - 80 keep one wave busy; a 256-thread workgroup per point would idle three of four.)  A point with a
// coordinate that is not finite gives NaN.
template <int FAM, int D>
__global__ __launch_bounds__(NT) void genfun_nd_kernel(const NdArgs a, const double *alpha, double *F)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int t = blockIdx.x * GF_WAVES + wave;
    if (t >= a.mi) return;              // the whole wave leaves: nothing below waits for another wave
    double xb[D], acc = 0.0;
    const bool ok = load_point<D>(a.Xb, a.ldxb, (size_t)t, xb);
    if (ok) {
        for (int j = lane; j < a.mj; j += 64) {
            double xa[D], v[D], kap;
#pragma unroll
            for (int c = 0; c < D; ++c) xa[c] = a.Xa[(size_t)j + (size_t)c * a.ldxa];
            genfun_pair<FAM, D>(a, xa, xb, v, kap);
#pragma unroll
            for (int c = 0; c < D; ++c) acc = __builtin_fma(v[c], alpha[(size_t)c * a.mj + j], acc);
        }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane == 0) F[t] = ok ? acc : __builtin_nan("");
}

// F[t] -= F[m], t < m: F relative to the reference point, whose value the launch before left behind the m test points
__global__ __launch_bounds__(NT) void genfun_sub_kernel(int m, double *F)
{
    const int t = blockIdx.x * NT + threadIdx.x;
    if (t < m) F[t] -= F[m];
}

// the chunk V (D n0 x a.mi, column-major) of the variance: V[c n0 + j, t] = v_t - v_0 with v_t[c n0 + j] = E_c g_c of the pair
// (training point j, test point t) and v_0 the same for the reference point x0 (null: v_0 = 0).  A thread keeps one training
// point and v_0 and walks through GF_CT test points: the lanes store consecutive rows of a column.  HBM-write bound (8 D bytes
// per pair), like the Gram kernels.  A column whose test point -- or reference -- is not finite is written as zeros, so that
// nothing but numbers enters the solves; genfun_prior_kernel gives that point a NaN prior, which is what its variance becomes.
template <int FAM, int D>
__global__ __launch_bounds__(NT) void genfun_cross_kernel(const NdArgs a, const double *x0, size_t ldx0, double *V, size_t ldv)
{
    const int j = blockIdx.x * NT + threadIdx.x, t0 = blockIdx.y * GF_CT;
    if (j >= a.mj) return;
    double xa[D], v0[D], kap;
#pragma unroll
    for (int c = 0; c < D; ++c) { xa[c] = a.Xa[(size_t)j + (size_t)c * a.ldxa]; v0[c] = 0.0; }
    bool ref_ok = true;
    if (x0) {
        double xr[D];
        ref_ok = load_point<D>(x0, ldx0, 0, xr);
        if (ref_ok) genfun_pair<FAM, D>(a, xa, xr, v0, kap);
    }
    const int t1 = min(t0 + GF_CT, a.mi);
    for (int t = t0; t < t1; ++t) {
        double xb[D], v[D];
        const bool ok = load_point<D>(a.Xb, a.ldxb, (size_t)t, xb) && ref_ok;
#pragma unroll
        for (int c = 0; c < D; ++c) v[c] = 0.0;
        if (ok) genfun_pair<FAM, D>(a, xa, xb, v, kap);
#pragma unroll
        for (int c = 0; c < D; ++c) V[(size_t)c * a.mj + j + (size_t)t * ldv] = ok ? v[c] - v0[c] : 0.0;
    }
}

// prior[t * stride] = kappa(t, t) of the a.mi test points -- kappa(t, t) - 2 kappa(t, 0) + kappa(0, 0) with a reference point,
// the prior variance of F(x_t) - F(x_0) --, every kappa from the forms above (the sum kernels have k(x, x) = D); NaN where a
// coordinate of the point or of the reference is not finite
template <int FAM, int D>
__global__ __launch_bounds__(NT) void genfun_prior_kernel(const NdArgs a, const double *x0, size_t ldx0, double *prior, size_t stride)
{
    const int t = blockIdx.x * NT + threadIdx.x;
    if (t >= a.mi) return;
    double xb[D], v[D], ktt, res;
    bool ok = load_point<D>(a.Xb, a.ldxb, (size_t)t, xb);
    genfun_pair<FAM, D>(a, xb, xb, v, ktt);
    res = ktt;
    if (x0) {
        double xr[D], kt0, k00;
        ok = load_point<D>(x0, ldx0, 0, xr) && ok;
        genfun_pair<FAM, D>(a, xb, xr, v, kt0);
        genfun_pair<FAM, D>(a, xr, xr, v, k00);
        res = __builtin_fma(-2.0, kt0, ktt) + k00;
    }
    prior[(size_t)t * stride] = ok ? res : __builtin_nan("");
}

}  // namespace

// F (device, m doubles -- m + 1 with has_ref) of the generating function at the device-resident test points Xt (m x 2d, ldxt).
// has_ref: Xt has one more row, row m, the reference point; F(x_0) is evaluated by one more wave of the same launch and left
// in F[m], and a second launch subtracts it: F[t] := F(x_t) - F(x_0), exactly 0.0 where x_t = x_0 (the same wave program, the
// same bits).
int genfun_nd(int family, int d, int m, const double *Xt, size_t ldxt, bool has_ref, int n0, const double *Xtr, size_t ldxtr,
              const double *hyp, int nhyp, const double *alpha, double *F, hipStream_t st)
{
    NdArgs a{};
    int rc = fill_args(family, d, hyp, nhyp, a);
    if (rc) return rc;
    if (m <= 0) return 0;
    a.mi = m + (has_ref ? 1 : 0); a.mj = n0; a.Xb = Xt; a.Xa = Xtr; a.ldxb = ldxt; a.ldxa = ldxtr;
    const unsigned blocks = ((unsigned)a.mi + GF_WAVES - 1) / GF_WAVES;
    if ((rc = dispatch_nd(family, d, [&](auto fam, auto dd) {
            hipLaunchKernelGGL((genfun_nd_kernel<decltype(fam)::value, decltype(dd)::value>), dim3(blocks), dim3(NT), 0, st, a, alpha, F);
            SGPR_CHECK_LAUNCH();
            return 0;
        })))
        return rc;
    if (has_ref) {
        hipLaunchKernelGGL(genfun_sub_kernel, dim3((m + NT - 1) / NT), dim3(NT), 0, st, m, F);
        SGPR_CHECK_LAUNCH();
    }
    return 0;
}

// One chunk of the variance of F: V (2 d n0 x mc, leading dimension ldv) = the cross-covariance columns v_t - v_0 of the mc
// test points Xt (device, mc x 2d, ldxt), and prior[t * prior_stride] = the prior variance of F(x_t) - F(x_0).  x0: the
// reference point on the device (coordinate c at x0[c * ldx0]) or null (v_0 = 0, the prior of F(x_t) itself).
int genfun_cross_nd(int family, int d, int mc, const double *Xt, size_t ldxt, const double *x0, size_t ldx0, int n0,
                    const double *Xtr, size_t ldxtr, const double *hyp, int nhyp, double *V, size_t ldv, double *prior,
                    size_t prior_stride, hipStream_t st)
{
    NdArgs a{};
    int rc = fill_args(family, d, hyp, nhyp, a);
    if (rc) return rc;
    if (mc <= 0 || n0 <= 0) return 0;
    if (ldv < (size_t)2 * d * n0) { set_error("genfun_cross_nd: ldv smaller than 2 d n0"); return SGPR_E_ARG; }
    a.mi = mc; a.mj = n0; a.Xb = Xt; a.Xa = Xtr; a.ldxb = ldxt; a.ldxa = ldxtr;
    const dim3 grid((n0 + NT - 1) / NT, (mc + GF_CT - 1) / GF_CT);
    if (grid.y > 65535) { set_error("genfun_cross_nd: too many test points for one launch"); return SGPR_E_ARG; }
    return dispatch_nd(family, d, [&](auto fam, auto dd) {
        constexpr int F = decltype(fam)::value, D = decltype(dd)::value;
        hipLaunchKernelGGL((genfun_cross_kernel<F, D>), grid, dim3(NT), 0, st, a, x0, ldx0, V, ldv);
        SGPR_CHECK_LAUNCH();
        hipLaunchKernelGGL((genfun_prior_kernel<F, D>), dim3((mc + NT - 1) / NT), dim3(NT), 0, st, a, x0, ldx0, prior, prior_stride);
        SGPR_CHECK_LAUNCH();
        return 0;
    });
}

}  // namespace sgpr
