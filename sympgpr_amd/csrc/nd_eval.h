// nd_eval.h -- the entry formulas of the d-pair kernels (gram_nd.hip has the derivation), shared by gram_nd.hip (Gram build,
// prediction), map_nd.hip (the symplectic map), genfun_nd.hip (the generating function) and batch.hip (the batched d-pair
// fits).  Per-problem constants live in NdConst: the single-problem kernels carry one inside their argument block
// (NdArgs::c, nd_args.h), the batched kernels read one per problem, as they read one KConst per problem for d = 1.
#pragma once
#include <type_traits>
#include "common.h"
#include "devmath.h"
#include "generated/pair_generated.h"

namespace sgpr {
namespace nd {

struct NdConst {
    double sig;
    double l[6], l2[6], inv_l2[6], inv_l4[6];
    double hs[6];            // periodic coordinates: sin(hs (x - x')), hs = 1/2 (A, B) or p_m (D)
};

// per coordinate: exponent of f_m, g = f'/f, nh = -f''/f
template <int FAM, int D, int M>
__device__ __forceinline__ void coord(const NdConst &a, double dx, double &arg, double &g, double &nh)
{
    if constexpr (FAM == SGPR_FAM_USER) {
        // the user's kernel: its generated factor forms (tools/gen_kernels.py), the q's with hs = p_m when it has one
        double o[3];
        if constexpr (M < D / 2) gen::factor<SGPR_FAM_USER, 1>(dx, a.l[M], a.hs[M], o);
        else                     gen::factor<SGPR_FAM_USER, 0>(dx, a.l[M], 0.0, o);
        arg = o[0]; g = o[1]; nh = o[2];
    } else if constexpr (FAM != SGPR_FAM_C && M < D / 2) {
        double s, c;
        const double h = a.hs[M] * dx;
        sincos_fast(h, s, c);
        const double s2 = s * s, sc = s * c;
        arg = -0.5 * a.inv_l2[M] * s2;
        g = -a.hs[M] * sc * a.inv_l2[M];
        nh = (a.hs[M] * a.hs[M]) * (a.l2[M] * cos2h_sel<false>(h, s2, a.l2[M]) - sc * sc) * a.inv_l4[M];   // devmath.h
    } else {
        const double d2 = dx * dx;
        arg = -0.5 * a.inv_l2[M] * d2;
        g = -dx * a.inv_l2[M];
        nh = (a.l2[M] - d2) * a.inv_l4[M];
    }
}

template <int FAM, int D, int M = 0>
__device__ __forceinline__ void all_coords(const NdConst &a, const double *xa, const double (&xb)[D],
                                           double (&arg)[D], double (&g)[D], double (&nh)[D])
{
    if constexpr (M < D) {
        coord<FAM, D, M>(a, xa[M] - xb[M], arg[M], g[M], nh[M]);
        all_coords<FAM, D, M + 1>(a, xa, xb, arg, g, nh);
    }
}

// E[m]: the factor that multiplies nh[m] on the diagonal blocks -- sig k for the product kernels (one exp
// per pair), sig f_m for the sum kernel (one exp per coordinate)
using gen::is_sum;

template <int FAM, int D>
__device__ __forceinline__ void weights(const NdConst &a, const double (&arg)[D], double (&E)[D])
{
    if constexpr (is_sum<FAM>()) {
#pragma unroll
        for (int m = 0; m < D; ++m) E[m] = a.sig * exp_fast(arg[m]);
    } else {
        double t = 0.0;
#pragma unroll
        for (int m = 0; m < D; ++m) t += arg[m];
        const double e = a.sig * exp_fast(t);
#pragma unroll
        for (int m = 0; m < D; ++m) E[m] = e;
    }
}

// the constants of one problem from hyp = (lq_1..lq_d, lP_1..lP_d, [p_1..p_d,] sig); checks d, the family and nhyp
inline int fill_consts(int family, int d, const double *hyp, int nhyp, NdConst &a)
{
    if (d < 1 || d > 3) { set_error("d must be 1, 2 or 3"); return SGPR_E_ARG; }
    if (family < SGPR_FAM_A || family > SGPR_FAM_USER) { set_error("unknown kernel family"); return SGPR_E_ARG; }
    const bool has_p = family_has_p(family);
    const int need = has_p ? 3 * d + 1 : 2 * d + 1;
    if (!hyp || nhyp != need) {
        set_error("hyp must hold (lq_1..lq_d, lP_1..lP_d, sig) -- (lq.., lP.., p_1..p_d, sig) for family D");
        return SGPR_E_ARG;
    }
    for (int m = 0; m < 2 * d; ++m) {
        a.l[m] = hyp[m];
        a.l2[m] = hyp[m] * hyp[m];
        a.inv_l2[m] = 1.0 / a.l2[m];
        a.inv_l4[m] = a.inv_l2[m] * a.inv_l2[m];
        a.hs[m] = (has_p && m < d) ? hyp[2 * d + m] : 0.5;
    }
    a.sig = hyp[nhyp - 1];
    return 0;
}

// f(std::integral_constant<int, family>(), std::integral_constant<int, 2 d>()) for the (family, d) chosen at run time
template <typename F>
int dispatch_nd(int family, int d, F &&f)
{
#define SGPR_ND_CASE(FAMV, DV) if (family == FAMV && d == DV) return f(std::integral_constant<int, FAMV>(), std::integral_constant<int, 2 * DV>())
    SGPR_ND_CASE(SGPR_FAM_A, 1); SGPR_ND_CASE(SGPR_FAM_A, 2); SGPR_ND_CASE(SGPR_FAM_A, 3);
    SGPR_ND_CASE(SGPR_FAM_C, 1); SGPR_ND_CASE(SGPR_FAM_C, 2); SGPR_ND_CASE(SGPR_FAM_C, 3);
    SGPR_ND_CASE(SGPR_FAM_B, 1); SGPR_ND_CASE(SGPR_FAM_B, 2); SGPR_ND_CASE(SGPR_FAM_B, 3);
    SGPR_ND_CASE(SGPR_FAM_D, 1); SGPR_ND_CASE(SGPR_FAM_D, 2); SGPR_ND_CASE(SGPR_FAM_D, 3);
    SGPR_ND_CASE(SGPR_FAM_USER, 1); SGPR_ND_CASE(SGPR_FAM_USER, 2); SGPR_ND_CASE(SGPR_FAM_USER, 3);
#undef SGPR_ND_CASE
    set_error("unsupported (family, d)");
    return SGPR_E_ARG;
}

}  // namespace nd
}  // namespace sgpr
