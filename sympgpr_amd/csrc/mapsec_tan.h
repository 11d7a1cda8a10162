// mapsec_tan.h -- the d = 1 half of the tangent map of the sectioned map: the Hessian sums of the TAN = true instance of
// applymap_sections_kernel on the d = 1 kernels' constants (KConst) and data layout.  What follows from the Hessian -- the step
// matrix, the monodromy product, the Benettin step -- is the D = 2 instance of tangent_core.h, which the d-pair map shares.
//
// Included by map.hip INSIDE its anonymous namespace, after MapSecArgs, which it uses as it is; nothing else includes it.
// maptan.h (the d-pair map's Hessian pass, map_nd.hip) has the derivation; the operation order is maptan.h's at D = 2.
//
// One step (q, p) -> (Q, P) of section m solves P = p - G_q(q, P), then Q = q + G_P(q, P).  After an accepted step one more pass
// over section m's training points sums the Hessian of the generating function at x = (q, P): A = H_qq, B = H_qP, C = H_PP.
// With dx = x_train - x, E = sig k, g = f'/f, nh = -f''/f, th = f'''/f per coordinate and the point's weights a1, a2:
//     product kernels   A = sum E (a1 th_q - nh_q g_P a2)      C = sum E (a2 th_P - nh_P g_q a1)
//                       B = - sum E (g_P nh_q a1 + g_q nh_P a2)
//     sum kernels       A = sum E_q a1 th_q,  C = sum E_P a2 th_P,  B = 0 (so the pass serves the explicit map as well)
// and with T = 1 / (1 + B), rows (Q, P), columns (q, p)
//     M = [ 1 + B - C T A    C T ]
//         [     - T A         T  ]
// which has determinant 1 for any A, B, C.  mono := M mono and the Benettin step (Z = M Qmat, modified Gram-Schmidt on the
// columns of Z in column order, log |r_cc| added to sum c) are column-wise: lanes 0 and 1 of wave 0 own one column each, kept in
// static LDS between the steps so that no register lives across the map step (tangent_core.h: maptan_advance<2>).
#pragma once

struct MapSecTanArgs : MapSecArgs {
    double *jac;                       // [nm - 1][ntest][2][2] or null
    double *mono;                      // [ntest][2][2] or null
    double *lyap;                      // [ntest][2] or null
};

// one coordinate's exponent, g = f'/f, nh = -f''/f and th = f'''/f at dx = x_train - x (Q = 1: the q factor, Q = 0: the P factor).
// th in maptan.h's closed form: -g (4 hs^2 + 3 nh + 2 g^2) for a periodic factor, -g (3 nh + 2 g^2) for a squared exponential;
// the user slot has nothing but generated code.
template <int FAM, int Q>
__device__ __forceinline__ void sec_coord(const KConst &kc, double dx, double &arg, double &g, double &nh, double &th)
{
    const double l = Q ? kc.lx : kc.ly, l2 = Q ? kc.lx2 : kc.ly2, inv_l2 = Q ? kc.inv_lx2 : kc.inv_ly2;
    const double inv_l4 = inv_l2 * inv_l2;
    if constexpr (FAM == SGPR_FAM_USER) {
        const double hs = Q ? (gen::user_has_p ? kc.p : 0.5) : 0.0;
        double o[3];
        gen::factor<SGPR_FAM_USER, Q>(dx, l, hs, o);
        arg = o[0]; g = o[1]; nh = o[2];
        th = gen::factor3<SGPR_FAM_USER, Q>(dx, l, hs);
    } else if constexpr (FAM != SGPR_FAM_C && Q) {
        const double hs = kc.hscale;
        double s, c;
        const double h = hs * dx;
        sincos_fast(h, s, c);
        const double s2 = s * s, sc = s * c;
        arg = -0.5 * inv_l2 * s2;
        g = -hs * sc * inv_l2;
        nh = (hs * hs) * (l2 * cos2h_sel<false>(h, s2, l2) - sc * sc) * inv_l4;
        th = -g * __builtin_fma(4.0 * hs, hs, __builtin_fma(2.0 * g, g, 3.0 * nh));
    } else {
        const double d2 = dx * dx;
        arg = -0.5 * inv_l2 * d2;
        g = -dx * inv_l2;
        nh = (l2 - d2) * inv_l4;
        th = -g * __builtin_fma(2.0 * g, g, 3.0 * nh);
    }
}

// One thread's share of the three Hessian sums at (q, P): the points j, j + dj, ... < n in that order, point j + i dj at index
// l + i dl of the four arrays -- rows_part's arguments (LDS or memory: each call site passes one kind)
template <int FAM>
__device__ __forceinline__ void sec_hess_part(const double *x, const double *y, const double *w1, const double *w2, int l, int dl,
                                              int j, int dj, int n, double q, double P, const KConst &kc, double &hA, double &hB,
                                              double &hC)
{
    hA = 0.0; hB = 0.0; hC = 0.0;
    for (; j < n; j += dj, l += dl) {
        double arg0, g0, nh0, th0, arg1, g1, nh1, th1;
        sec_coord<FAM, 1>(kc, x[l] - q, arg0, g0, nh0, th0);
        sec_coord<FAM, 0>(kc, y[l] - P, arg1, g1, nh1, th1);
        const double a1 = w1[l], a2 = w2[l];
        if constexpr (gen::is_sum<FAM>()) {
            const double E0 = kc.sig * exp_fast(arg0), E1 = kc.sig * exp_fast(arg1);
            hA = __builtin_fma(E0, a1 * th0, hA);
            hC = __builtin_fma(E1, a2 * th1, hC);
        } else {
            double t = 0.0;
            t += arg0;
            t += arg1;
            const double E = kc.sig * exp_fast(t);
            double S = 0.0;
            S = __builtin_fma(g0, a1, S);
            S = __builtin_fma(g1, a2, S);
            const double tA = __builtin_fma(a1, th0, -nh0 * (S - g0 * a1));
            const double rest = S - g0 * a1 - g1 * a2;
            const double tB = g0 * g1 * rest - g1 * nh0 * a1 - g0 * nh1 * a2;
            const double tC = __builtin_fma(a2, th1, -nh1 * (S - g1 * a2));
            hA = __builtin_fma(E, tA, hA);
            hB = __builtin_fma(E, tB, hB);
            hC = __builtin_fma(E, tC, hC);
        }
    }
}
