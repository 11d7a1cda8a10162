// maptan.h -- the d-pair half of the tangent map of the d-pair symplectic map: the Hessian pass of the TAN = true instances of
// applymap_nd_kernel on the d-pair data layout.  What follows from the Hessian -- the step matrix, the monodromy product, the
// Benettin step -- knows no layout and is in tangent_core.h, which the sectioned d = 1 map (map.hip, mapsec_tan.h) shares.
//
// Included by map_nd.hip INSIDE its anonymous namespace, after tangent_core.h (block_sum_n, hess_idx) and the map's own pieces
// (NdArgs, MapNdArgs, all_coords, weights), which it uses as they are; map_nd.hip is its only includer.
//
// One step (q, p) -> (Q, P) of the map solves P = p - G_q(q, P), then Q = q + G_P(q, P), with G(x) = K*(x) alpha the gradient of
// the learned generating function.  Its Jacobian needs the Hessian H = dG/dx (D x D, symmetric) at the accepted (q, P): with
// A = H_qq, B = H_qP, C = H_PP and T = (I + B)^-1
//     dP = T dp - T A dq,      dQ = (I + B^T) dq + C dP        =>      M = [ I + B^T - C T A    C T ]      rows (Q, P),
//                                                                          [      - T A          T  ]      columns (q, p)
// which is symplectic for any symmetric A and C.  H is summed over the training points once per step, one sum per UNORDERED
// pair (c, e) -- D (D + 1) / 2 = 21 at D = 6 --, so it is symmetric by construction.  With dx = x_train - x, E = sig k,
// g = f'/f, nh = -f''/f, th = f'''/f per coordinate, S = sum_b g_b alpha_b (dE/ddx_e = E g_e, dg_e/ddx_e = -(nh_e + g_e^2),
// dnh_e/ddx_e = -th_e - nh_e g_e, and d/dx = -d/ddx):
//     product kernels   H_cc = sum_j E (alpha_c th_c - nh_c (S - g_c alpha_c))
//                       H_ce = - sum_j E [ g_e nh_c alpha_c + g_c nh_e alpha_e - g_c g_e (S - g_c alpha_c - g_e alpha_e) ]   (c != e)
//     sum kernels       H_cc = sum_j E_c alpha_c th_c,  H_ce = 0: B = 0, A depends on q only and C on P only, so the pass at
//                       (q, P) serves the explicit map P = p - G_q(q), Q = q + G_P(P) as well.
// The products mono := M mono and the Benettin step (Z = M Qmat, modified Gram-Schmidt on the columns of Z in column order,
// log |r_cc| added to sum c) are column-wise: lane c of wave 0 owns column c of mono and of Qmat and sum c, kept in LDS
// between the steps so that no register lives across the Newton passes; the Gram-Schmidt sweep broadcasts one column at a time.
#pragma once

struct MapNdTanArgs : MapNdArgs {
    double *jac;                       // [nm - 1][ntest][D][D] or null
    double *mono;                      // [ntest][D][D] or null
    double *lyap;                      // [ntest][D] or null
};

// th = f'''/f of coordinate M.  The authoritative form is gen::factor3 (tools/gen_kernels.py); the hand-written families take it
// from g and nh, which the pass holds anyway: with a = log f, f'''/f = a''' + 3 a' a'' + a'^3, a' = g, a'' = -nh - g^2, and
// a''' = -4 hs^2 g for the periodic factor exp(-sin^2(hs dx) / (2 l^2)), 0 for the squared exponential:
//     th = -g (4 hs^2 + 3 nh + 2 g^2)    resp.    th = -g (3 nh + 2 g^2)
// -- 4 flops instead of four sin / cos calls and a division per periodic coordinate (DESIGN 3.8 has the instruction counts).
// MAPTAN_GEN_TH = true runs gen::factor3 for every family; tests/test_applymap_tangent_cpu.py holds the two forms together.
constexpr bool MAPTAN_GEN_TH = false;

template <int FAM, int D, int M>
__device__ __forceinline__ double coord_th(const NdArgs &a, double dx, double g, double nh)
{
    constexpr int Q = M < D / 2 ? 1 : 0;
    if constexpr (FAM == SGPR_FAM_USER || MAPTAN_GEN_TH) {
        return gen::factor3<FAM, Q>(dx, a.c.l[M], Q ? a.c.hs[M] : 0.0);
    } else if constexpr (FAM != SGPR_FAM_C && Q) {
        return -g * __builtin_fma(4.0 * a.c.hs[M], a.c.hs[M], __builtin_fma(2.0 * g, g, 3.0 * nh));
    } else {
        return -g * __builtin_fma(2.0 * g, g, 3.0 * nh);
    }
}

template <int FAM, int D, int M = 0>
__device__ __forceinline__ void all_th(const NdArgs &a, const double *xa, const double (&xb)[D], const double (&g)[D],
                                       const double (&nh)[D], double (&th)[D])
{
    if constexpr (M < D) {
        th[M] = coord_th<FAM, D, M>(a, xa[M] - xb[M], g[M], nh[M]);
        all_th<FAM, D, M + 1>(a, xa, xb, g, nh, th);
    }
}

// The Hessian pass can be split at compile time into NG groups of consecutive pairs, every group folded in the same fixed
// order, for an instance whose pass of all pairs at once would not fit its registers.  No shipped instance needs it: with the
// step's M handed over through LDS and no log inside the step loop all of them run one pass without scratch (DESIGN 3.8 has
// the table).  The sum kernels have D sums (the diagonal) in one pass.
template <int FAM, int D, int TT> constexpr int maptan_groups() { return 1; }

// H[LO .. HI) (product kernels) or the diagonal of H (sum kernels; the rest is set to 0) over all n0 training points at x
template <int FAM, int D, int TT, int LO, int HI>
__device__ __forceinline__ void maptan_hess_pass(const MapNdArgs &a, const double (&x)[D], stage_ptr stg,
                                                 double (&H)[D * (D + 1) / 2], double *part, double *res)
{
    constexpr bool SUM = is_sum<FAM>();
    constexpr int NS = SUM ? D : HI - LO;
    double acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = 0.0;
    const int n0 = a.k.mj;
    for (int j = threadIdx.x; j < n0; j += TT) {
        double xa[D], al[D], g[D], nh[D], th[D], arg[D], E[D];
        if (stg) {
#pragma unroll
            for (int c = 0; c < D; ++c) { xa[c] = stg[c * MAPND_STAGE_PTS + j]; al[c] = stg[(D + c) * MAPND_STAGE_PTS + j]; }
        } else {
#pragma unroll
            for (int c = 0; c < D; ++c) { xa[c] = a.k.Xa[(size_t)j + (size_t)c * a.k.ldxa]; al[c] = a.alpha[(size_t)c * n0 + j]; }
        }
        all_coords<FAM, D>(a.k.c, xa, x, arg, g, nh);
        weights<FAM, D>(a.k.c, arg, E);
        all_th<FAM, D>(a.k, xa, x, g, nh, th);
        if constexpr (SUM) {
#pragma unroll
            for (int c = 0; c < D; ++c) acc[c] = __builtin_fma(E[c], al[c] * th[c], acc[c]);
        } else {
            double S = 0.0;
#pragma unroll
            for (int c = 0; c < D; ++c) S = __builtin_fma(g[c], al[c], S);
#pragma unroll
            for (int c = 0; c < D; ++c) {
#pragma unroll
                for (int e = c; e < D; ++e) {
                    const int s = hess_idx(D, c, e);
                    if (s < LO || s >= HI) continue;
                    double t;
                    if (c == e) {
                        t = __builtin_fma(al[c], th[c], -nh[c] * (S - g[c] * al[c]));
                    } else {
                        const double rest = S - g[c] * al[c] - g[e] * al[e];
                        t = g[c] * g[e] * rest - g[e] * nh[c] * al[c] - g[c] * nh[e] * al[e];
                    }
                    acc[s - LO] = __builtin_fma(E[0], t, acc[s - LO]);
                }
            }
        }
    }
    block_sum_n<NS, TT>(acc, part, res);
    if constexpr (SUM) {
#pragma unroll
        for (int s = 0; s < D * (D + 1) / 2; ++s) H[s] = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) H[hess_idx(D, c, c)] = acc[c];
    } else {
#pragma unroll
        for (int s = LO; s < HI; ++s) H[s] = acc[s - LO];
    }
}

// all groups of the Hessian pass, one after the other; the two LDS halves keep alternating with seq
template <int FAM, int D, int TT, int G = 0>
__device__ __forceinline__ void maptan_hessian(const MapNdArgs &a, const double (&x)[D], stage_ptr stg,
                                               double (&H)[D * (D + 1) / 2], double *part0, double *res0, int part_half,
                                               int res_half, unsigned &seq)
{
    constexpr int NP = D * (D + 1) / 2, NG = is_sum<FAM>() ? 1 : maptan_groups<FAM, D, TT>();
    if constexpr (G < NG) {
        constexpr int LO = NP * G / NG, HI = NP * (G + 1) / NG;
        ++seq;
        maptan_hess_pass<FAM, D, TT, LO, HI>(a, x, stg, H, part0 + (seq & 1u) * part_half, res0 + (seq & 1u) * res_half);
        maptan_hessian<FAM, D, TT, G + 1>(a, x, stg, H, part0, res0, part_half, res_half, seq);
    }
}

// the most sums any pass of the instance folds: what the two LDS halves have to hold
template <int FAM, int D, int TT>
constexpr int maptan_max_sums()
{
    constexpr int d = D / 2, NP = D * (D + 1) / 2, NG = is_sum<FAM>() ? 1 : maptan_groups<FAM, D, TT>();
    constexpr int hess = is_sum<FAM>() ? D : (NP + NG - 1) / NG, newton = D + d * d;
    return hess > newton ? hess : newton;
}
