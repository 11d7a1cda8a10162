// gram_nd.hip -- Gram build for d canonical pairs per training point (BASELINE configs d = 2, 3).
//
// The reference's kernels take one pair (x, y) = (q, P) (kernels.f90:1); SURVEY.md 8 generalises
// them the way its own generator would (init_func.py:24-52): inputs x = (q_1..q_d, P_1..P_d),
// product kernel k = prod_m f_m(x_m - x'_m) with f_m periodic (family A; D: with a free period p_m per q,
// hyp = (lq.., lP.., p_1..p_d, sig)) or SE (family C) on the q's and SE on the P's, and the covariance of
// the gradient observations
//     K_ab = d^2 k / dx_a dx'_b = sig k (a == b ? -f_a''/f_a : -(f_a'/f_a)(f_b'/f_b)),  a, b = 1..2d;
// family B, the SUM kernel k = sum_m f_m: K_aa = -sig f_a'', all other blocks zero (the explicit maps),
// stored as (2d)^2 blocks of N x N0, block (a, b) at rows a*N, columns b*N0.  d = 1 is build_K
// (sympgpr.f90:12-38) entry for entry.  One exp and d sincos per PAIR feed all (2d)^2 entries:
// 32 d^2 bytes written per pair, so the kernel is even more firmly HBM-write bound than d = 1.
// The symplectic map of these fits is map_nd.hip, the generating function itself genfun_nd.hip; nd_args.h holds the argument
// block the three units share.
#include <type_traits>
#include "common.h"
#include "devmath.h"
#include "generated/pair_generated.h"
#include "nd_args.h"

namespace sgpr {

namespace {

using namespace nd;         // coord, all_coords, weights, is_sum, NdConst, dispatch_nd (nd_eval.h); NT, NdArgs, fill_args (nd_args.h)

constexpr int NTI = 2 * NT, NTJ = 16;
typedef double double2_t __attribute__((ext_vector_type(2)));

template <int FAM, int D>
__global__ __launch_bounds__(NT) void gram_nd_kernel(const NdArgs a)
{
    __shared__ double sxa[NTJ][D];
    const int i0 = blockIdx.x * NTI, j0 = blockIdx.y * NTJ;
    const int t = threadIdx.x;
    const int nj = min(NTJ, a.mj - j0);
    for (int e = t; e < nj * D; e += NT) sxa[e / D][e % D] = a.Xa[(size_t)(j0 + e / D) + (size_t)(e % D) * a.ldxa];
    __syncthreads();
    const int i = i0 + 2 * t;
    const bool v0 = i < a.mi, v1 = i + 1 < a.mi;
    double xb0[D], xb1[D];
#pragma unroll
    for (int m = 0; m < D; ++m) {
        xb0[m] = v0 ? a.Xb[(size_t)i + (size_t)m * a.ldxb] : 0.0;
        xb1[m] = v1 ? a.Xb[(size_t)i + 1 + (size_t)m * a.ldxb] : 0.0;
    }
    bool even = ((a.ld | a.rstride | a.cstride) & 1) == 0;
    if (a.sel) {
#pragma unroll
        for (int c = 0; c < D; ++c) even = even && ((a.roff[c] & 1) == 0 || a.roff[c] < 0);
    }
    const bool vec = (i0 + NTI <= a.mi) && even && (((uintptr_t)a.K & 15) == 0);
    const long d0 = (long)i + a.diag_off;
    for (int jj = 0; jj < nj; ++jj) {
        double g0[D], nh0[D], g1[D], nh1[D], arg0[D], arg1[D], E0[D], E1[D];
        all_coords<FAM, D>(a.c, sxa[jj], xb0, arg0, g0, nh0);
        all_coords<FAM, D>(a.c, sxa[jj], xb1, arg1, g1, nh1);
        weights<FAM, D>(a.c, arg0, E0);
        weights<FAM, D>(a.c, arg1, E1);
        const long j = j0 + jj;
        const double n0 = (d0 == j) ? a.noise : 0.0, n1 = (d0 + 1 == j) ? a.noise : 0.0;
#pragma unroll
        for (int ca = 0; ca < D; ++ca) {
#pragma unroll
            for (int cb = 0; cb < D; ++cb) {
                const double off0 = is_sum<FAM>() ? 0.0 : -E0[ca] * (g0[ca] * g0[cb]);
                const double off1 = is_sum<FAM>() ? 0.0 : -E1[ca] * (g1[ca] * g1[cb]);
                const double k0 = (ca == cb) ? __builtin_fma(E0[ca], nh0[ca], n0) : off0;
                const double k1 = (ca == cb) ? __builtin_fma(E1[ca], nh1[ca], n1) : off1;
                if (a.sel && (a.roff[ca] < 0 || a.coff[cb] < 0)) continue;      // block not wanted by this call
                double *dst = a.sel ? a.K + (size_t)a.roff[ca] + (size_t)i + ((size_t)a.coff[cb] + (size_t)j) * a.ld
                                    : a.K + (size_t)ca * a.rstride + (size_t)i + ((size_t)cb * a.cstride + (size_t)j) * a.ld;
                if (vec) {
                    *reinterpret_cast<double2_t *>(dst) = double2_t{k0, k1};
                } else {
                    if (v0) dst[0] = k0;
                    if (v1) dst[1] = k1;
                }
            }
        }
    }
}

// K*(2d x 2d n0) . alpha for one test point per workgroup; out is (m x D) column-major
template <int FAM, int D>
__global__ __launch_bounds__(NT) void predict_nd_kernel(const NdArgs a, int m, const double *alpha, double *out)
{
    // here: Xb = test points (m x D), Xa = training points (mj = n0)
    const int k = blockIdx.x;
    double xb[D], acc[D];
#pragma unroll
    for (int c = 0; c < D; ++c) { xb[c] = a.Xb[(size_t)k + (size_t)c * a.ldxb]; acc[c] = 0.0; }
    for (int j = threadIdx.x; j < a.mj; j += NT) {
        double xa[D], g[D], nh[D], arg[D], E[D];
#pragma unroll
        for (int c = 0; c < D; ++c) xa[c] = a.Xa[(size_t)j + (size_t)c * a.ldxa];
        all_coords<FAM, D>(a.c, xa, xb, arg, g, nh);
        weights<FAM, D>(a.c, arg, E);
        double al[D], S = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) { al[c] = alpha[(size_t)c * a.mj + j]; S = __builtin_fma(g[c], al[c], S); }
#pragma unroll
        for (int c = 0; c < D; ++c) {  // sum_b K_cb alpha_b = E (nh_c al_c - g_c (S - g_c al_c)); sum kernel: E_c nh_c al_c
            const double cross = is_sum<FAM>() ? 0.0 : -g[c] * (S - g[c] * al[c]);
            acc[c] = __builtin_fma(E[c], __builtin_fma(nh[c], al[c], cross), acc[c]);
        }
    }
    __shared__ double sh[NT / 64][D];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        double v = acc[c];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < D) {
        double v = 0.0;
        for (int w = 0; w < NT / 64; ++w) v += sh[w][threadIdx.x];
        out[(size_t)k + (size_t)threadIdx.x * m] = v;
    }
}

}  // namespace

// what gram_nd and gram_nd_sel share once their own checks are past: the geometry of the pairs, the grid and the launch
static int gram_nd_launch(int family, int d, NdArgs &a, int mi, int mj, const double *Xb, size_t ldxb, const double *Xa, size_t ldxa,
                          double *K, size_t ld, hipStream_t st)
{
    a.mi = mi; a.mj = mj; a.Xb = Xb; a.Xa = Xa; a.ldxb = ldxb; a.ldxa = ldxa;
    a.K = K; a.ld = ld;
    const dim3 grid((mi + NTI - 1) / NTI, (mj + NTJ - 1) / NTJ);
    if (grid.y > 65535) { set_error("too many pair columns for one launch"); return SGPR_E_ARG; }
    return dispatch_nd(family, d, [&](auto fam, auto dd) {
        hipLaunchKernelGGL((gram_nd_kernel<decltype(fam)::value, decltype(dd)::value>), grid, dim3(NT), 0, st, a);
        SGPR_CHECK_LAUNCH();
        return 0;
    });
}

int gram_nd(int family, int d, int mi, int mj, const double *Xb, size_t ldxb, const double *Xa, size_t ldxa,
            const double *hyp, int nhyp, double *K, size_t ld, size_t rstride, size_t cstride, long diag_off,
            double noise, hipStream_t st)
{
    NdArgs a{};
    int rc = fill_args(family, d, hyp, nhyp, a);
    if (rc) return rc;
    if (mi <= 0 || mj <= 0) return 0;
    a.rstride = rstride; a.cstride = cstride; a.diag_off = diag_off; a.noise = noise;
    return gram_nd_launch(family, d, a, mi, mj, Xb, ldxb, Xa, ldxa, K, ld, st);
}

// the same pairs, but only the blocks (a, b) with roff[a] >= 0 and coff[b] >= 0, block (a, b) at K + roff[a] + coff[b] * ld
// (a block-cyclic rank whose coordinate blocks hold different points: sympgpr_amd/dist.py)
int gram_nd_sel(int family, int d, int mi, int mj, const double *Xb, size_t ldxb, const double *Xa, size_t ldxa,
                const double *hyp, int nhyp, double *K, size_t ld, const long *roff, const long *coff, hipStream_t st)
{
    NdArgs a{};
    int rc = fill_args(family, d, hyp, nhyp, a);
    if (rc) return rc;
    if (mi <= 0 || mj <= 0) return 0;
    if (!roff || !coff) { set_error("gram_nd_sel: null offsets"); return SGPR_E_ARG; }
    a.rstride = 0; a.cstride = 0; a.diag_off = 1L << 60; a.noise = 0.0;
    a.sel = 1;
    bool any = false;
    for (int c = 0; c < 2 * d; ++c) { a.roff[c] = roff[c]; a.coff[c] = coff[c]; }
    for (int c = 0; c < 2 * d; ++c)
        for (int e = 0; e < 2 * d; ++e) any = any || (roff[c] >= 0 && coff[e] >= 0);
    if (!any) return 0;
    return gram_nd_launch(family, d, a, mi, mj, Xb, ldxb, Xa, ldxa, K, ld, st);
}

int predict_nd(int family, int d, int m, const double *Xt, size_t ldxt, int n0, const double *Xtr, size_t ldxtr,
               const double *hyp, int nhyp, const double *alpha, double *out, hipStream_t st)
{
    NdArgs a{};
    int rc = fill_args(family, d, hyp, nhyp, a);
    if (rc) return rc;
    if (m <= 0) return 0;
    a.mi = m; a.mj = n0; a.Xb = Xt; a.Xa = Xtr; a.ldxb = ldxt; a.ldxa = ldxtr;
    return dispatch_nd(family, d, [&](auto fam, auto dd) {
        hipLaunchKernelGGL((predict_nd_kernel<decltype(fam)::value, decltype(dd)::value>), dim3(m), dim3(NT), 0, st, a, m,
                           alpha, out);
        SGPR_CHECK_LAUNCH();
        return 0;
    });
}

bool family_is_sum(int family) { return family == SGPR_FAM_B || (family == SGPR_FAM_USER && gen::user_is_sum); }

}  // namespace sgpr
