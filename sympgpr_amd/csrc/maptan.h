// maptan.h -- the tangent map of the d-pair symplectic map: the TAN = true half of applymap_nd_kernel.
//
// Included by map_nd.hip INSIDE its anonymous namespace, after the map's own pieces (NdArgs, MapNdArgs, all_coords, weights,
// block_sum_n, finite_d), which it uses as they are; map_nd.hip is its only includer.
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

// the unordered pair (c, e), c <= e, in H: row after row of the upper triangle
constexpr int hess_idx(int D, int c, int e) { return c * D - c * (c - 1) / 2 + (e - c); }
constexpr int hess_at(int D, int c, int e) { return c <= e ? hess_idx(D, c, e) : hess_idx(D, e, c); }

// The Hessian pass can be split at compile time into NG groups of consecutive pairs, every group folded in the same fixed
// order, for an instance whose pass of all pairs at once would not fit its registers.  No shipped instance needs it: with the
// step's M handed over through LDS and no log inside the step loop all of them run one pass without scratch (DESIGN 3.8 has
// the table).  The sum kernels have D sums (the diagonal) in one pass.
template <int FAM, int D, int TT> constexpr int maptan_groups() { return 1; }

// H[LO .. HI) (product kernels) or the diagonal of H (sum kernels; the rest is set to 0) over all n0 training points at x
template <int FAM, int D, int TT, int LO, int HI>
__device__ __forceinline__ void maptan_hess_pass(const MapNdArgs &a, const double (&x)[D], const double *stg,
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
__device__ __forceinline__ void maptan_hessian(const MapNdArgs &a, const double (&x)[D], const double *stg,
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

// C (d x d) := A B
template <int d>
__device__ __forceinline__ void mat_mul(const double (&A)[d * d], const double (&B)[d * d], double (&C)[d * d])
{
#pragma unroll
    for (int r = 0; r < d; ++r)
#pragma unroll
        for (int c = 0; c < d; ++c) {
            double v = 0.0;
#pragma unroll
            for (int s = 0; s < d; ++s) v = __builtin_fma(A[r * d + s], B[s * d + c], v);
            C[r * d + c] = v;
        }
}

// M from H (block-uniform values, every thread alike); T = (I + B)^-1 in closed form, the adjugate as in newton_step.
// false (and M all NaN): I + B singular or something not finite.
template <int D>
__device__ __forceinline__ bool maptan_matrix(const double (&H)[D * (D + 1) / 2], double (&M)[D * D])
{
    constexpr int d = D / 2;
    double A[d * d], Bm[d * d], C[d * d], K[d * d], T[d * d], TA[d * d], CT[d * d], CTA[d * d];
#pragma unroll
    for (int c = 0; c < d; ++c)
#pragma unroll
        for (int e = 0; e < d; ++e) {
            A[c * d + e] = H[hess_at(D, c, e)];
            Bm[c * d + e] = H[hess_idx(D, c, d + e)];
            C[c * d + e] = H[hess_at(D, d + c, d + e)];
            K[c * d + e] = Bm[c * d + e] + (c == e ? 1.0 : 0.0);
        }
    double det;
    if constexpr (d == 1) {
        det = K[0];
        T[0] = 1.0 / det;
    } else if constexpr (d == 2) {
        det = K[0] * K[3] - K[1] * K[2];
        const double id = 1.0 / det;
        T[0] = K[3] * id; T[1] = -K[1] * id;
        T[2] = -K[2] * id; T[3] = K[0] * id;
    } else {
        const double c00 = K[4] * K[8] - K[5] * K[7], c01 = K[5] * K[6] - K[3] * K[8], c02 = K[3] * K[7] - K[4] * K[6];
        const double c10 = K[2] * K[7] - K[1] * K[8], c11 = K[0] * K[8] - K[2] * K[6], c12 = K[1] * K[6] - K[0] * K[7];
        const double c20 = K[1] * K[5] - K[2] * K[4], c21 = K[2] * K[3] - K[0] * K[5], c22 = K[0] * K[4] - K[1] * K[3];
        det = K[0] * c00 + K[1] * c01 + K[2] * c02;
        const double id = 1.0 / det;
        T[0] = c00 * id; T[1] = c10 * id; T[2] = c20 * id;      // the adjugate is the transposed cofactor matrix
        T[3] = c01 * id; T[4] = c11 * id; T[5] = c21 * id;
        T[6] = c02 * id; T[7] = c12 * id; T[8] = c22 * id;
    }
    mat_mul<d>(T, A, TA);
    mat_mul<d>(C, T, CT);
    mat_mul<d>(C, TA, CTA);
    bool ok = finite_d(det) && det != 0.0;
#pragma unroll
    for (int c = 0; c < d; ++c)
#pragma unroll
        for (int e = 0; e < d; ++e) {
            M[c * D + e] = (c == e ? 1.0 : 0.0) + Bm[e * d + c] - CTA[c * d + e];
            M[c * D + d + e] = CT[c * d + e];
            M[(d + c) * D + e] = -TA[c * d + e];
            M[(d + c) * D + d + e] = T[c * d + e];
        }
#pragma unroll
    for (int s = 0; s < D * D; ++s) ok = ok && finite_d(M[s]);
    if (!ok) {
#pragma unroll
        for (int s = 0; s < D * D; ++s) M[s] = __builtin_nan("");
    }
    return ok;
}

// Lane c < D of wave 0 owns column c of mono and of Qmat and the sum c of log |r_cc|: (2 D + 2) D doubles in LDS, entry i of
// lane c at st[i * D + c] (i < D: mono, D <= i < 2 D: Qmat, i = 2 D, 2 D + 1: the sum).  Only the owner reads or writes its
// entries.  The sum is kept as log(m) + e log 2 with the product m of the r_cc's mantissas in [1, 2) and the sum e of their
// exponents, renormalised every step; the one log is taken when the orbit is done (maptan_finish).  A log call inside the step
// loop cost the D = 6 instances 20 VGPRs at their tightest point, and the 512-thread ones spilled.
// Behind them the step's M (D D doubles), which thread 0 hands to wave 0 through LDS: held in registers next to the columns it
// cost the D = 6 instances 30 VGPRs more than the passes need, and the 512-thread ones spilled.
template <int D>
__device__ __forceinline__ double *maptan_state()
{
    __shared__ double st[(2 * D + 2) * D + D * D];
    return st;
}
template <int D> constexpr int maptan_m_at() { return (2 * D + 2) * D; }

// thread 0 publishes the step's M: to jac (if wanted) and to wave 0
template <int D>
__device__ __forceinline__ void maptan_publish(const double (&M)[D * D], double *jac_out)
{
    double *ms = maptan_state<D>() + maptan_m_at<D>();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int s = 0; s < D * D; ++s) ms[s] = M[s];
        if (jac_out) {
#pragma unroll
            for (int s = 0; s < D * D; ++s) jac_out[s] = M[s];
        }
    }
    __syncthreads();
}

template <int D>
__device__ __forceinline__ void maptan_init()
{
    double *st = maptan_state<D>();
    const int lane = threadIdx.x;
    if (lane < D) {
#pragma unroll
        for (int r = 0; r < D; ++r) st[r * D + lane] = st[(D + r) * D + lane] = (r == lane) ? 1.0 : 0.0;
        st[2 * D * D + lane] = 1.0;
        st[(2 * D + 1) * D + lane] = 0.0;
    }
}

// mono := M mono;  Z = M Qmat, Qmat := the orthonormal columns of Z by modified Gram-Schmidt in column order (column c is
// normalised, then taken out of every later column), sum c += log |r_cc|.  Wave 0 only, all of its 64 lanes (the broadcasts).
template <int D>
__device__ __forceinline__ void maptan_advance()
{
    if (threadIdx.x >= 64) return;
    double *st = maptan_state<D>();
    const double *M = st + maptan_m_at<D>();
    const int lane = threadIdx.x;
    double mo[D], qv[D], mn[D], mc[D], lm = 1.0, le = 0.0;      // the owner's columns of mono and Qmat; their images under M
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
#pragma unroll 1
    for (int c = 0; c < D; ++c) {          // not unrolled: c only selects the lane, and D copies of the sweep cost registers
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
template <int D>
__device__ __forceinline__ void maptan_finish(const MapNdTanArgs &a, int k)
{
    const double *st = maptan_state<D>();
    const int lane = threadIdx.x;
    if (lane < D) {
        if (a.mono) {
#pragma unroll
            for (int r = 0; r < D; ++r) a.mono[((size_t)k * D + r) * D + lane] = st[r * D + lane];
        }
        if (a.lyap) {
            const double sum = __builtin_fma(st[(2 * D + 1) * D + lane], 0.693147180559945309417, log(st[2 * D * D + lane]));
            a.lyap[(size_t)k * D + lane] = a.nm > 1 ? sum / (double)(a.nm - 1) : 0.0;
        }
    }
}
