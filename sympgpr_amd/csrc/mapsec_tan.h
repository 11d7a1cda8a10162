// mapsec_tan.h -- the tangent map of the sectioned d = 1 map: the TAN = true half of applymap_sections_kernel.
//
// Included by map.hip INSIDE its anonymous namespace, after block_sum2 and MapSecArgs, which it uses as they are; nothing else
// includes it.  maptan.h (the d-pair map's tangent, map_nd.hip) has the derivation; this is its D = 2 case restated on the
// d = 1 kernels' constants (KConst) and data layout, with the operation order of maptan.h at D = 2.
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
// static LDS between the steps so that no register lives across the map step.
#pragma once

struct MapSecTanArgs : MapSecArgs {
    double *jac;                       // [nm - 1][ntest][2][2] or null
    double *mono;                      // [ntest][2][2] or null
    double *lyap;                      // [ntest][2] or null
};

__device__ __forceinline__ bool sec_finite(double v) { return __builtin_fabs(v) < __builtin_inf(); }

template <int FAM> constexpr bool sec_is_sum() { return FAM == SGPR_FAM_B || (FAM == SGPR_FAM_USER && gen::user_is_sum); }

// block_sum2 with a third sum; `sh`: 3 * (TT / 64) doubles of the LDS half the call before did not use
template <int TT>
__device__ __forceinline__ void block_sum3(double &a, double &b, double &c, double *sh)
{
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o, 64);
        b += __shfl_down(b, o, 64);
        c += __shfl_down(c, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sh[3 * (threadIdx.x >> 6)] = a;
        sh[3 * (threadIdx.x >> 6) + 1] = b;
        sh[3 * (threadIdx.x >> 6) + 2] = c;
    }
    __syncthreads();
    double x = 0.0, y = 0.0, z = 0.0;
#pragma unroll
    for (int w = 0; w < TT / 64; ++w) { x += sh[3 * w]; y += sh[3 * w + 1]; z += sh[3 * w + 2]; }
    a = x; b = y; c = z;
}

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
        if constexpr (sec_is_sum<FAM>()) {
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

// M from A, B, C (block-uniform values, every thread alike).  false (and M all NaN): 1 + B is 0 or something is not finite.
__device__ __forceinline__ bool sec_tan_matrix(double A, double B, double C, double (&M)[4])
{
    const double det = B + 1.0, T = 1.0 / det;
    const double TA = __builtin_fma(T, A, 0.0), CT = __builtin_fma(C, T, 0.0), CTA = __builtin_fma(C, TA, 0.0);
    M[0] = 1.0 + B - CTA;
    M[1] = CT;
    M[2] = -TA;
    M[3] = T;
    bool ok = sec_finite(det) && det != 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) ok = ok && sec_finite(M[s]);
    if (!ok) {
#pragma unroll
        for (int s = 0; s < 4; ++s) M[s] = __builtin_nan("");
    }
    return ok;
}

// Lane c < 2 of wave 0 owns column c of mono and of Qmat and the sum c of log |r_cc|: entry i of lane c at st[2 i + c] (i < 2:
// mono, 2 <= i < 4: Qmat, i = 4, 5: the sum).  Only the owner reads or writes its entries.  The sum is kept as log(m) + e log 2
// with the product m of the r_cc's mantissas in [1, 2) and the sum e of their exponents, renormalised every step; the one log is
// taken when the orbit is done.  Behind them the step's M (4 doubles), which thread 0 hands to wave 0.
constexpr int SEC_TAN_M_AT = 12;
__device__ __forceinline__ double *sec_tan_state()
{
    __shared__ double st[SEC_TAN_M_AT + 4];
    return st;
}

__device__ __forceinline__ void sec_tan_init()
{
    double *st = sec_tan_state();
    const int lane = threadIdx.x;
    if (lane < 2) {
#pragma unroll
        for (int r = 0; r < 2; ++r) st[r * 2 + lane] = st[(2 + r) * 2 + lane] = (r == lane) ? 1.0 : 0.0;
        st[8 + lane] = 1.0;
        st[10 + lane] = 0.0;
    }
}

// thread 0 publishes the step's M: to jac (if wanted) and to wave 0
__device__ __forceinline__ void sec_tan_publish(const double (&M)[4], double *jac_out)
{
    double *ms = sec_tan_state() + SEC_TAN_M_AT;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int s = 0; s < 4; ++s) ms[s] = M[s];
        if (jac_out) {
#pragma unroll
            for (int s = 0; s < 4; ++s) jac_out[s] = M[s];
        }
    }
    __syncthreads();
}

// mono := M mono;  Z = M Qmat, Qmat := the orthonormal columns of Z by modified Gram-Schmidt in column order, sum c += log |r_cc|.
// Wave 0 only, all of its 64 lanes (the broadcasts).
__device__ __forceinline__ void sec_tan_advance()
{
    if (threadIdx.x >= 64) return;
    constexpr int D = 2;
    double *st = sec_tan_state();
    const double *M = st + SEC_TAN_M_AT;
    const int lane = threadIdx.x;
    double mo[D], qv[D], mn[D], mc[D], lm = 1.0, le = 0.0;
#pragma unroll
    for (int r = 0; r < D; ++r) { mo[r] = 0.0; qv[r] = 0.0; }
    if (lane < D) {
#pragma unroll
        for (int r = 0; r < D; ++r) { mo[r] = st[r * D + lane]; qv[r] = st[(D + r) * D + lane]; }
        lm = st[2 * D * D + lane];
        le = st[(2 * D + 1) * D + lane];
    }
#pragma unroll
    for (int r = 0; r < D; ++r) {
        double v = 0.0, w = 0.0;
#pragma unroll
        for (int s = 0; s < D; ++s) { v = __builtin_fma(M[r * D + s], mo[s], v); w = __builtin_fma(M[r * D + s], qv[s], w); }
        mn[r] = v;
        mc[r] = w;                         // column `lane` of Z
    }
#pragma unroll
    for (int c = 0; c < D; ++c) {
        double n2 = 0.0;
#pragma unroll
        for (int r = 0; r < D; ++r) n2 = __builtin_fma(mc[r], mc[r], n2);
        const double nrm = __builtin_sqrt(n2);
        const double rcc = __shfl(nrm, c, 64), inv = 1.0 / rcc;
        double qc[D], dot = 0.0;
#pragma unroll
        for (int r = 0; r < D; ++r) {
            qc[r] = __shfl(mc[r], c, 64) * inv;
            dot = __builtin_fma(qc[r], mc[r], dot);
        }
        if (lane == c) {
            int e1, e2;
            lm *= 2.0 * __builtin_frexp(rcc, &e1);     // both factors in [1, 2): the product is below 4
            lm = 2.0 * __builtin_frexp(lm, &e2);
            le += (double)(e1 + e2 - 2);
        }
#pragma unroll
        for (int r = 0; r < D; ++r) mc[r] = (lane == c) ? qc[r] : (lane > c ? __builtin_fma(-dot, qc[r], mc[r]) : mc[r]);
    }
    if (lane < D) {
#pragma unroll
        for (int r = 0; r < D; ++r) { st[r * D + lane] = mn[r]; st[(D + r) * D + lane] = mc[r]; }
        st[2 * D * D + lane] = lm;
        st[(2 * D + 1) * D + lane] = le;
    }
}

// the orbit's mono (column by column) and exponents, by their owners
__device__ __forceinline__ void sec_tan_finish(const MapSecTanArgs &a, int k)
{
    const double *st = sec_tan_state();
    const int lane = threadIdx.x;
    if (lane < 2) {
        if (a.mono) {
#pragma unroll
            for (int r = 0; r < 2; ++r) a.mono[((size_t)k * 2 + r) * 2 + lane] = st[r * 2 + lane];
        }
        if (a.lyap) {
            const double sum = __builtin_fma(st[10 + lane], 0.693147180559945309417, log(st[8 + lane]));
            a.lyap[(size_t)k * 2 + lane] = a.nm > 1 ? sum / (double)(a.nm - 1) : 0.0;
        }
    }
}
