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
#include <type_traits>
#include "common.h"
#include "devmath.h"
#include "generated/pair_generated.h"
#include "nd_eval.h"

namespace sgpr {

namespace {

using namespace nd;         // coord, all_coords, weights, is_sum, NdConst, fill_consts, dispatch_nd

constexpr int NT = 256, NTI = 2 * NT, NTJ = 16;
typedef double double2_t __attribute__((ext_vector_type(2)));

// the geometry of one call and, last, the constants of the fit (nd_eval.h)
struct NdArgs {
    int mi, mj;
    const double *Xb, *Xa;   // row points (mi x D), column points (mj x D), column-major
    size_t ldxb, ldxa;
    double *K;
    size_t ld, rstride, cstride;   // element distance between consecutive row / column blocks
    int sel;                       // 1: block (a, b) goes to K + roff[a] + coff[b] * ld instead, skipped when either is < 0
    long roff[6], coff[6];
    long diag_off;
    double noise;
    NdConst c;
};

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

// the hyper-parameters of the call into the constants of its argument block (nd_eval.h)
int fill_args(int family, int d, const double *hyp, int nhyp, NdArgs &a) { return fill_consts(family, d, hyp, nhyp, a.c); }

// ---- applymap_nd: the symplectic map of a d-pair fit, every step of one orbit inside one workgroup ------------------------
// x = (q_1..q_d, P_1..P_d), G(x) = K*(x) alpha as predict_nd_kernel forms it: G_q = dF/dq = p - P, G_P = dF/dP = Q - q.  One step
// solves f(P) = G_q(q, P) - p + P = 0 for P in R^d by Newton from P = p, then Q = q + G_P(q, P).  The Jacobian is analytic:
// one pass over the training points accumulates the 2d sums of G and the d^2 sums of dG_q/dP together (15 at d = 3).  With
// dx = x_train - x, E = sig k, S = sum_b g_b alpha_b and T_c = nh_c alpha_c - g_c (S - g_c alpha_c)  (G_c = sum_j E T_c),
//     d(G)_c / dP_e = - sum_j E [ g_e T_c + g_c alpha_e (nh_e + g_e^2) ]     (c a q index, e a P index: c != e always, so no
// third derivative of a factor appears; dE/ddx_e = E g_e, dg_e/ddx_e = -(nh_e + g_e^2)).  The sum kernels' G_q does not depend
// on P: their Jacobian sums are not formed and the first Newton step is exact.
constexpr int MAPND_T_SMALL = 256, MAPND_T_LARGE = 512;    // threads per orbit: n0 <= MAPND_STAGE_PTS / larger training sets
constexpr int MAPND_STAGE_PTS = 4 * MAPND_T_SMALL;         // training points a 256-thread workgroup keeps in LDS (2 D doubles each: 96 KiB at D = 6)

struct MapNdArgs {
    NdArgs k;                          // Xa = training points (mj = n0 of them), the hyper-parameters
    int nm, ntest, mode, maxiter;
    double tol;
    const double *alpha;               // 2 d n0
    const double *Q0, *P0;             // ntest x d, column-major, leading dimension ntest
    double *qmap, *pmap;               // [nm][ntest][d]
    int *iters;                        // [nm - 1][ntest], may be null
};

// v[s] := the sum over the workgroup of every thread's v[s], the same bits in every thread: wave shuffle, one row of NS sums
// per wave in LDS, folded in wave order.  8 waves: lanes 0 .. NS-1 fold one sum each and publish it (NS instead of 8 NS
// reads per thread).  `part` (W NS doubles) and `res` (NS) are the halves the call before did NOT use -- the callers alternate,
// as block_sum2 of map.hip does: the barrier of call n + 1 lies between the reads of call n and the writes of call n + 2.
template <int NS, int TT>
__device__ __forceinline__ void block_sum_n(double (&v)[NS], double *part, double *res)
{
    constexpr int W = TT / 64;
#pragma unroll
    for (int s = 0; s < NS; ++s)
        for (int o = 32; o > 0; o >>= 1) v[s] += __shfl_down(v[s], o, 64);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int s = 0; s < NS; ++s) part[(threadIdx.x >> 6) * NS + s] = v[s];
    }
    __syncthreads();
    if constexpr (W <= 4) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            double x = 0.0;
#pragma unroll
            for (int w = 0; w < W; ++w) x += part[w * NS + s];
            v[s] = x;
        }
    } else {
        if (threadIdx.x < NS) {
            double x = 0.0;
#pragma unroll
            for (int w = 0; w < W; ++w) x += part[w * NS + threadIdx.x];
            res[threadIdx.x] = x;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < NS; ++s) v[s] = res[s];
    }
}

// G = K*(x) alpha (D sums) and, with JAC, J[c * d + e] = d G_c / d P_e (d^2 sums) over all n0 training points: thread t takes
// the points t, t + TT, ...  `stg`: the staged points ([coordinate | alpha block][MAPND_STAGE_PTS]) or null (read from memory)
template <int FAM, int D, int TT, bool JAC>
__device__ __forceinline__ void mapnd_pass(const MapNdArgs &a, const double (&x)[D], const double *stg, double (&G)[D],
                                           double (&J)[(D / 2) * (D / 2)], double *part, double *res)
{
    constexpr int d = D / 2;
    constexpr bool WITH_J = JAC && !is_sum<FAM>();
    constexpr int NS = D + (WITH_J ? d * d : 0);
    double acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = 0.0;
    const int n0 = a.k.mj;
    for (int j = threadIdx.x; j < n0; j += TT) {
        double xa[D], al[D], g[D], nh[D], arg[D], E[D], T[D];
        if (stg) {
#pragma unroll
            for (int c = 0; c < D; ++c) { xa[c] = stg[c * MAPND_STAGE_PTS + j]; al[c] = stg[(D + c) * MAPND_STAGE_PTS + j]; }
        } else {
#pragma unroll
            for (int c = 0; c < D; ++c) { xa[c] = a.k.Xa[(size_t)j + (size_t)c * a.k.ldxa]; al[c] = a.alpha[(size_t)c * n0 + j]; }
        }
        all_coords<FAM, D>(a.k.c, xa, x, arg, g, nh);
        weights<FAM, D>(a.k.c, arg, E);
        double S = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) S = __builtin_fma(g[c], al[c], S);
#pragma unroll
        for (int c = 0; c < D; ++c) {  // as predict_nd_kernel
            const double cross = is_sum<FAM>() ? 0.0 : -g[c] * (S - g[c] * al[c]);
            T[c] = __builtin_fma(nh[c], al[c], cross);
            acc[c] = __builtin_fma(E[c], T[c], acc[c]);
        }
        if constexpr (WITH_J) {
#pragma unroll
            for (int c = 0; c < d; ++c) {
#pragma unroll
                for (int e = 0; e < d; ++e) {
                    const double ge = g[d + e];
                    const double t = __builtin_fma(ge, T[c], g[c] * al[d + e] * __builtin_fma(ge, ge, nh[d + e]));
                    acc[D + c * d + e] = __builtin_fma(-E[0], t, acc[D + c * d + e]);
                }
            }
        }
    }
    block_sum_n<NS, TT>(acc, part, res);
#pragma unroll
    for (int c = 0; c < D; ++c) G[c] = acc[c];
#pragma unroll
    for (int s = 0; s < d * d; ++s) {
        if constexpr (WITH_J) J[s] = acc[D + s];
        else J[s] = 0.0;
    }
}

__device__ __forceinline__ bool finite_d(double v) { return __builtin_fabs(v) <= 1.79769313486231570815e308; }   // false for NaN too

// dP := -(I + J)^-1 f in closed form (d <= 3; block-uniform values, every thread alike).  false: singular or not finite.
template <int d>
__device__ __forceinline__ bool newton_step(const double (&J)[d * d], const double (&f)[d], double (&dP)[d])
{
    double A[d * d];
#pragma unroll
    for (int c = 0; c < d; ++c)
#pragma unroll
        for (int e = 0; e < d; ++e) A[c * d + e] = J[c * d + e] + (c == e ? 1.0 : 0.0);
    double det;
    if constexpr (d == 1) {
        det = A[0];
        dP[0] = -f[0] / det;
    } else if constexpr (d == 2) {
        det = A[0] * A[3] - A[1] * A[2];
        dP[0] = -(A[3] * f[0] - A[1] * f[1]) / det;
        dP[1] = -(A[0] * f[1] - A[2] * f[0]) / det;
    } else {
        const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
        const double c10 = A[2] * A[7] - A[1] * A[8], c11 = A[0] * A[8] - A[2] * A[6], c12 = A[1] * A[6] - A[0] * A[7];
        const double c20 = A[1] * A[5] - A[2] * A[4], c21 = A[2] * A[3] - A[0] * A[5], c22 = A[0] * A[4] - A[1] * A[3];
        det = A[0] * c00 + A[1] * c01 + A[2] * c02;
        dP[0] = -(c00 * f[0] + c10 * f[1] + c20 * f[2]) / det;     // the adjugate is the transposed cofactor matrix
        dP[1] = -(c01 * f[0] + c11 * f[1] + c21 * f[2]) / det;
        dP[2] = -(c02 * f[0] + c12 * f[1] + c22 * f[2]) / det;
    }
    bool ok = finite_d(det) && det != 0.0;
#pragma unroll
    for (int c = 0; c < d; ++c) ok = ok && finite_d(dP[c]);
    return ok;
}

#include "maptan.h"   // the tangent map: what TAN = true adds to the kernel below

// One workgroup per orbit runs all nm steps; nothing waits on another workgroup, and an orbit's bits depend on nothing but its
// own start point (TT is chosen from n0 alone).  TT = 256: the training points and alpha are staged in LDS once when they fit
// (every thread reads back what it wrote itself: no barrier); TT = 512 reads them from memory (L2) on every pass.  512, not 1024:
// the D = 6 passes hold 150 - 196 VGPRs, and a 1024-thread workgroup leaves 128 per thread -- the compiler spilled up to 86 of
// them to scratch there; at 512 threads (256 VGPRs each) no instance spills.
// TAN: after every accepted step one more pass (maptan.h) sums the Hessian of the generating function at (q, P); the step's
// Jacobian M, the product of the M's and the Benettin sums follow from it.  The orbit itself takes the same passes in the same
// order as without TAN and has the same bits.  A lost orbit's M is NaN from that step on, and with it mono and the exponents.
template <int FAM, int D, int TT, bool TAN = false>
__global__ __launch_bounds__(TT) void applymap_nd_kernel(const std::conditional_t<TAN, MapNdTanArgs, MapNdArgs> a)
{
    constexpr int d = D / 2, W = TT / 64, NSMAX = TAN ? maptan_max_sums<FAM, D, TT>() : D + d * d;
    constexpr bool HAS_STAGE = TT == MAPND_T_SMALL;
    __shared__ double part[2][W * NSMAX];
    __shared__ double res[2][NSMAX];
    __shared__ double stage[HAS_STAGE ? 2 * D * MAPND_STAGE_PTS : 1];
    const int k = blockIdx.x, n0 = a.k.mj;
    const double *stg = nullptr;
    if (HAS_STAGE && n0 <= MAPND_STAGE_PTS) {
        for (int j = threadIdx.x; j < n0; j += TT) {
#pragma unroll
            for (int c = 0; c < D; ++c) {
                stage[c * MAPND_STAGE_PTS + j] = a.k.Xa[(size_t)j + (size_t)c * a.k.ldxa];
                stage[(D + c) * MAPND_STAGE_PTS + j] = a.alpha[(size_t)c * n0 + j];
            }
        }
        stg = stage;
    }
    unsigned seq = 0;
    double q[d], p[d];
#pragma unroll
    for (int c = 0; c < d; ++c) {
        q[c] = a.Q0[(size_t)k + (size_t)c * a.ntest];
        p[c] = a.P0[(size_t)k + (size_t)c * a.ntest];
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < d; ++c) { a.qmap[(size_t)k * d + c] = q[c]; a.pmap[(size_t)k * d + c] = p[c]; }
    }
    const double nan = __builtin_nan("");
    const double twopi = 6.283185307179586477;
    if constexpr (TAN) maptan_init<D>();
    for (int i = 0; i + 1 < a.nm; ++i) {
        bool good = true;                                   // block-uniform, like everything below
#pragma unroll
        for (int c = 0; c < d; ++c) good = good && finite_d(q[c]) && finite_d(p[c]);   // a lost (NaN) orbit stays lost
        int its = 0;
        double x[D], G[D], J[d * d], P[d], Q[d];
#pragma unroll
        for (int c = 0; c < d; ++c) { x[c] = q[c]; P[c] = p[c]; Q[c] = nan; }
        if (good && (a.mode & SGPR_MAP_EXPLICIT)) {         // P = p - G_q(q, p), no solve
#pragma unroll
            for (int c = 0; c < d; ++c) x[d + c] = p[c];
            ++seq;
            mapnd_pass<FAM, D, TT, false>(a, x, stg, G, J, part[seq & 1u], res[seq & 1u]);
#pragma unroll
            for (int c = 0; c < d; ++c) { P[c] = p[c] - G[c]; good = good && finite_d(P[c]); }
        } else if (good) {                                  // Newton on f(P) = G_q(q, P) - p + P from P = p
            for (int it = 0; it < a.maxiter; ++it) {
#pragma unroll
                for (int c = 0; c < d; ++c) x[d + c] = P[c];
                ++seq;
                mapnd_pass<FAM, D, TT, true>(a, x, stg, G, J, part[seq & 1u], res[seq & 1u]);
                double f[d], dP[d], step = 0.0, size = 1.0;
#pragma unroll
                for (int c = 0; c < d; ++c) f[c] = G[c] - p[c] + P[c];
                if (!newton_step<d>(J, f, dP)) { good = false; break; }
#pragma unroll
                for (int c = 0; c < d; ++c) {
                    P[c] += dP[c];
                    step = fmax(step, fabs(dP[c]));
                    size = fmax(size, fabs(P[c]));
                }
                ++its;
                if (step <= a.tol * size) break;
            }
        }
        if (good) {                                         // one pass without the Jacobian at the final P: the residual and G_P
#pragma unroll
            for (int c = 0; c < d; ++c) x[d + c] = P[c];
            ++seq;
            mapnd_pass<FAM, D, TT, false>(a, x, stg, G, J, part[seq & 1u], res[seq & 1u]);
            if (!(a.mode & SGPR_MAP_EXPLICIT)) {
                double r = 0.0, pmax = 1.0;
#pragma unroll
                for (int c = 0; c < d; ++c) {
                    const double fc = G[c] - p[c] + P[c];
                    good = good && finite_d(fc);
                    r = fmax(r, fabs(fc));
                    pmax = fmax(pmax, fabs(p[c]));
                }
                good = good && r <= 1e-8 * pmax;            // the d = 1 map's acceptance rule
            }
#pragma unroll
            for (int c = 0; c < d; ++c) {
                Q[c] = q[c] + G[d + c];
                good = good && finite_d(Q[c]);
                if (a.mode & SGPR_MAP_WRAP_Q) Q[c] -= twopi * floor(Q[c] / twopi);
            }
        }
#pragma unroll
        for (int c = 0; c < d; ++c) { q[c] = good ? Q[c] : nan; p[c] = good ? P[c] : nan; }
        if (threadIdx.x == 0) {
            const size_t o = ((size_t)(i + 1) * a.ntest + k) * d;
#pragma unroll
            for (int c = 0; c < d; ++c) { a.qmap[o + c] = q[c]; a.pmap[o + c] = p[c]; }
            if (a.iters) a.iters[(size_t)i * a.ntest + k] = good ? its : -1;
        }
        if constexpr (TAN) {                                // x is still (q, P) of the accepted step
            double M[D * D];
            bool tan_ok = false;
            if (good) {
                double H[D * (D + 1) / 2];
                maptan_hessian<FAM, D, TT>(a, x, stg, H, &part[0][0], &res[0][0], W * NSMAX, NSMAX, seq);
                tan_ok = maptan_matrix<D>(H, M);
            }
            if (!tan_ok) {
#pragma unroll
                for (int s = 0; s < D * D; ++s) M[s] = nan;
            }
            maptan_publish<D>(M, a.jac ? a.jac + ((size_t)i * a.ntest + k) * (D * D) : nullptr);
            maptan_advance<D>();
        }
    }
    if constexpr (TAN) maptan_finish<D>(a, k);
}

// The backward step: rows qmap[0], pmap[0] hold (Q, P), and one step returns the (q, p) that the kernel above takes there.  The
// point of the passes is the same x = (q, P); now P is known and q is not: Newton on f(q) = q + G_P(q, P) - Q = 0 from q = Q,
// then p = P + G_q(q, P).  The Jacobian is I + dG_P/dq, and G is a gradient (of the generating function), so dG_P/dq is the
// transpose of the dG_q/dP that mapnd_pass<.., true> sums: the same pass, the same 2d + d^2 sums, newton_step on the transposed
// block.  The closing pass and the acceptance rule are the forward ones with the roles swapped (|f| <= 1e-8 max(1, max|Q|));
// SGPR_MAP_WRAP_Q wraps the q that was solved for.  The sum kernels' G_P does not depend on q: the first step is exact.
// SGPR_MAP_EXPLICIT never arrives here (the C entries refuse it).  Staging, TT, the seq alternation and the lost-orbit rule (NaN
// from that step on, iters = -1) are those of applymap_nd_kernel; there is no TAN instance -- the backward step's Jacobian is
// the symplectic inverse of the forward step matrix at the same (q, P).
template <int FAM, int D, int TT>
__global__ __launch_bounds__(TT) void applymap_nd_inverse_kernel(const MapNdArgs a)
{
    constexpr int d = D / 2, W = TT / 64, NSMAX = D + d * d;
    constexpr bool HAS_STAGE = TT == MAPND_T_SMALL;
    __shared__ double part[2][W * NSMAX];
    __shared__ double res[2][NSMAX];
    __shared__ double stage[HAS_STAGE ? 2 * D * MAPND_STAGE_PTS : 1];
    const int k = blockIdx.x, n0 = a.k.mj;
    const double *stg = nullptr;
    if (HAS_STAGE && n0 <= MAPND_STAGE_PTS) {               // as applymap_nd_kernel: every thread reads back what it wrote itself
        for (int j = threadIdx.x; j < n0; j += TT) {
#pragma unroll
            for (int c = 0; c < D; ++c) {
                stage[c * MAPND_STAGE_PTS + j] = a.k.Xa[(size_t)j + (size_t)c * a.k.ldxa];
                stage[(D + c) * MAPND_STAGE_PTS + j] = a.alpha[(size_t)c * n0 + j];
            }
        }
        stg = stage;
    }
    unsigned seq = 0;
    double Q[d], P[d];                                      // the point the next step starts from: the image (Q, P)
#pragma unroll
    for (int c = 0; c < d; ++c) {
        Q[c] = a.Q0[(size_t)k + (size_t)c * a.ntest];
        P[c] = a.P0[(size_t)k + (size_t)c * a.ntest];
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < d; ++c) { a.qmap[(size_t)k * d + c] = Q[c]; a.pmap[(size_t)k * d + c] = P[c]; }
    }
    const double nan = __builtin_nan("");
    const double twopi = 6.283185307179586477;
    for (int i = 0; i + 1 < a.nm; ++i) {
        bool good = true;                                   // block-uniform, like everything below
#pragma unroll
        for (int c = 0; c < d; ++c) good = good && finite_d(Q[c]) && finite_d(P[c]);   // a lost (NaN) orbit stays lost
        int its = 0;
        double x[D], G[D], J[d * d], q[d], p[d];
#pragma unroll
        for (int c = 0; c < d; ++c) { x[c] = Q[c]; x[d + c] = P[c]; q[c] = nan; p[c] = nan; }
        if (good) {                                         // Newton on f(q) = q + G_P(q, P) - Q from q = Q
            for (int it = 0; it < a.maxiter; ++it) {
                ++seq;
                mapnd_pass<FAM, D, TT, true>(a, x, stg, G, J, part[seq & 1u], res[seq & 1u]);
                double f[d], Jt[d * d], dq[d], step = 0.0, size = 1.0;
#pragma unroll
                for (int c = 0; c < d; ++c) {
                    f[c] = x[c] + G[d + c] - Q[c];
#pragma unroll
                    for (int e = 0; e < d; ++e) Jt[c * d + e] = J[e * d + c];   // dG_P,c / dq_e = dG_q,e / dP_c
                }
                if (!newton_step<d>(Jt, f, dq)) { good = false; break; }
#pragma unroll
                for (int c = 0; c < d; ++c) {
                    x[c] += dq[c];
                    step = fmax(step, fabs(dq[c]));
                    size = fmax(size, fabs(x[c]));
                }
                ++its;
                if (step <= a.tol * size) break;
            }
        }
        if (good) {                                         // one pass without the Jacobian at the final q: the residual and G_q
            ++seq;
            mapnd_pass<FAM, D, TT, false>(a, x, stg, G, J, part[seq & 1u], res[seq & 1u]);
            double r = 0.0, qmax = 1.0;
#pragma unroll
            for (int c = 0; c < d; ++c) {
                const double fc = x[c] + G[d + c] - Q[c];
                good = good && finite_d(fc);
                r = fmax(r, fabs(fc));
                qmax = fmax(qmax, fabs(Q[c]));
            }
            good = good && r <= 1e-8 * qmax;                // the forward rule with the roles swapped
#pragma unroll
            for (int c = 0; c < d; ++c) {
                p[c] = P[c] + G[c];
                good = good && finite_d(p[c]);
                q[c] = x[c];
                if (a.mode & SGPR_MAP_WRAP_Q) q[c] -= twopi * floor(q[c] / twopi);
            }
        }
#pragma unroll
        for (int c = 0; c < d; ++c) { Q[c] = good ? q[c] : nan; P[c] = good ? p[c] : nan; }
        if (threadIdx.x == 0) {
            const size_t o = ((size_t)(i + 1) * a.ntest + k) * d;
#pragma unroll
            for (int c = 0; c < d; ++c) { a.qmap[o + c] = Q[c]; a.pmap[o + c] = P[c]; }
            if (a.iters) a.iters[(size_t)i * a.ntest + k] = good ? its : -1;
        }
    }
}

// ---- genfun: the generating function F itself, of which every entry above returns derivatives ------------------------------
// The observations are (dF/dq, dF/dP), so cov(F(x*), observation c of training point j) = d(sig k)/dx_train,c = E_c g_c with
// dx = x_train - x* (E, g as above), and
//     F(x*) = sum_j sum_c E_c g_c alpha_{cN+j}     (product kernels: sum_j E S, S = sum_c g_c alpha_{cN+j}),
// whose gradient in x* is K*(x*) alpha as predict_nd_kernel forms it.  The prior of F is kappa(x, x') = sig k(x, x').
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

int gram_nd(int family, int d, int mi, int mj, const double *Xb, size_t ldxb, const double *Xa, size_t ldxa,
            const double *hyp, int nhyp, double *K, size_t ld, size_t rstride, size_t cstride, long diag_off,
            double noise, hipStream_t st)
{
    NdArgs a{};
    int rc = fill_args(family, d, hyp, nhyp, a);
    if (rc) return rc;
    if (mi <= 0 || mj <= 0) return 0;
    a.mi = mi; a.mj = mj; a.Xb = Xb; a.Xa = Xa; a.ldxb = ldxb; a.ldxa = ldxa;
    a.K = K; a.ld = ld; a.rstride = rstride; a.cstride = cstride; a.diag_off = diag_off; a.noise = noise;
    const dim3 grid((mi + NTI - 1) / NTI, (mj + NTJ - 1) / NTJ);
    if (grid.y > 65535) { set_error("too many pair columns for one launch"); return SGPR_E_ARG; }
    return dispatch_nd(family, d, [&](auto fam, auto dd) {
        hipLaunchKernelGGL((gram_nd_kernel<decltype(fam)::value, decltype(dd)::value>), grid, dim3(NT), 0, st, a);
        SGPR_CHECK_LAUNCH();
        return 0;
    });
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
    a.mi = mi; a.mj = mj; a.Xb = Xb; a.Xa = Xa; a.ldxb = ldxb; a.ldxa = ldxa;
    a.K = K; a.ld = ld; a.rstride = 0; a.cstride = 0; a.diag_off = 1L << 60; a.noise = 0.0;
    a.sel = 1;
    bool any = false;
    for (int c = 0; c < 2 * d; ++c) { a.roff[c] = roff[c]; a.coff[c] = coff[c]; }
    for (int c = 0; c < 2 * d; ++c)
        for (int e = 0; e < 2 * d; ++e) any = any || (roff[c] >= 0 && coff[e] >= 0);
    if (!any) return 0;
    const dim3 grid((mi + NTI - 1) / NTI, (mj + NTJ - 1) / NTJ);
    if (grid.y > 65535) { set_error("too many pair columns for one launch"); return SGPR_E_ARG; }
    return dispatch_nd(family, d, [&](auto fam, auto dd) {
        hipLaunchKernelGGL((gram_nd_kernel<decltype(fam)::value, decltype(dd)::value>), grid, dim3(NT), 0, st, a);
        SGPR_CHECK_LAUNCH();
        return 0;
    });
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

// threads per orbit, from n0 alone: up to MAPND_STAGE_PTS points (4 per thread, the d = 1 kernel's staging depth) run from LDS
// on 256 threads; more points go to 512 threads (see applymap_nd_kernel for why not 1024).  DESIGN 3.8 has the measured passes.
static int applymap_nd_threads(int n0) { return n0 <= MAPND_STAGE_PTS ? MAPND_T_SMALL : MAPND_T_LARGE; }

// everything device-resident: Xtr (n0 x 2d, ldxtr), alpha (2 d n0), Q0 / P0 (ntest x d, leading dimension ntest),
// qmap / pmap ([nm][ntest][d]), iters ([nm - 1][ntest] or null); mode: SGPR_MAP_WRAP_Q | SGPR_MAP_EXPLICIT (checked by the C entries)
int applymap_nd(int family, int d, int mode, int nm, int ntest, int n0, const double *Xtr, size_t ldxtr, const double *hyp,
                int nhyp, const double *alpha, const double *Q0, const double *P0, double *qmap, double *pmap, int *iters,
                hipStream_t st)
{
    MapNdArgs a{};
    int rc = fill_args(family, d, hyp, nhyp, a.k);
    if (rc) return rc;
    if (nm <= 0 || ntest <= 0) return 0;
    a.k.mj = n0; a.k.Xa = Xtr; a.k.ldxa = ldxtr;
    a.nm = nm; a.ntest = ntest; a.mode = mode; a.maxiter = 60; a.tol = 1e-13;   // the d = 1 map's tol and maxiter
    a.alpha = alpha; a.Q0 = Q0; a.P0 = P0; a.qmap = qmap; a.pmap = pmap; a.iters = iters;
    const bool small = applymap_nd_threads(n0) == MAPND_T_SMALL;
    return dispatch_nd(family, d, [&](auto fam, auto dd) {
        constexpr int F = decltype(fam)::value, D = decltype(dd)::value;
        if (small) hipLaunchKernelGGL((applymap_nd_kernel<F, D, MAPND_T_SMALL>), dim3(ntest), dim3(MAPND_T_SMALL), 0, st, a);
        else       hipLaunchKernelGGL((applymap_nd_kernel<F, D, MAPND_T_LARGE>), dim3(ntest), dim3(MAPND_T_LARGE), 0, st, a);
        SGPR_CHECK_LAUNCH();
        return 0;
    });
}

// the backward orbit: Q0 / P0 hold the images (Q, P), row i of qmap / pmap is the i-th preimage.  Arguments and shapes as
// applymap_nd; mode: SGPR_MAP_WRAP_Q only (the C entries refuse SGPR_MAP_EXPLICIT)
int applymap_nd_inverse(int family, int d, int mode, int nm, int ntest, int n0, const double *Xtr, size_t ldxtr, const double *hyp,
                        int nhyp, const double *alpha, const double *Q0, const double *P0, double *qmap, double *pmap, int *iters,
                        hipStream_t st)
{
    MapNdArgs a{};
    int rc = fill_args(family, d, hyp, nhyp, a.k);
    if (rc) return rc;
    if (nm <= 0 || ntest <= 0) return 0;
    a.k.mj = n0; a.k.Xa = Xtr; a.k.ldxa = ldxtr;
    a.nm = nm; a.ntest = ntest; a.mode = mode; a.maxiter = 60; a.tol = 1e-13;   // as applymap_nd
    a.alpha = alpha; a.Q0 = Q0; a.P0 = P0; a.qmap = qmap; a.pmap = pmap; a.iters = iters;
    const bool small = applymap_nd_threads(n0) == MAPND_T_SMALL;
    return dispatch_nd(family, d, [&](auto fam, auto dd) {
        constexpr int F = decltype(fam)::value, D = decltype(dd)::value;
        if (small) hipLaunchKernelGGL((applymap_nd_inverse_kernel<F, D, MAPND_T_SMALL>), dim3(ntest), dim3(MAPND_T_SMALL), 0, st, a);
        else       hipLaunchKernelGGL((applymap_nd_inverse_kernel<F, D, MAPND_T_LARGE>), dim3(ntest), dim3(MAPND_T_LARGE), 0, st, a);
        SGPR_CHECK_LAUNCH();
        return 0;
    });
}

// the same launch with the tangent map: jac ([nm - 1][ntest][D][D]), mono ([ntest][D][D]), lyap ([ntest][D]), each device-resident
// or null.  The orbit outputs have the bits of applymap_nd.
int applymap_nd_tangent(int family, int d, int mode, int nm, int ntest, int n0, const double *Xtr, size_t ldxtr, const double *hyp,
                        int nhyp, const double *alpha, const double *Q0, const double *P0, double *qmap, double *pmap, int *iters,
                        double *jac, double *mono, double *lyap, hipStream_t st)
{
    MapNdTanArgs a{};
    int rc = fill_args(family, d, hyp, nhyp, a.k);
    if (rc) return rc;
    if (nm <= 0 || ntest <= 0) return 0;
    a.k.mj = n0; a.k.Xa = Xtr; a.k.ldxa = ldxtr;
    a.nm = nm; a.ntest = ntest; a.mode = mode; a.maxiter = 60; a.tol = 1e-13;   // as applymap_nd
    a.alpha = alpha; a.Q0 = Q0; a.P0 = P0; a.qmap = qmap; a.pmap = pmap; a.iters = iters;
    a.jac = jac; a.mono = mono; a.lyap = lyap;
    const bool small = applymap_nd_threads(n0) == MAPND_T_SMALL;
    return dispatch_nd(family, d, [&](auto fam, auto dd) {
        constexpr int F = decltype(fam)::value, D = decltype(dd)::value;
        if (small) hipLaunchKernelGGL((applymap_nd_kernel<F, D, MAPND_T_SMALL, true>), dim3(ntest), dim3(MAPND_T_SMALL), 0, st, a);
        else       hipLaunchKernelGGL((applymap_nd_kernel<F, D, MAPND_T_LARGE, true>), dim3(ntest), dim3(MAPND_T_LARGE), 0, st, a);
        SGPR_CHECK_LAUNCH();
        return 0;
    });
}

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

bool family_is_sum(int family) { return family == SGPR_FAM_B || (family == SGPR_FAM_USER && gen::user_is_sum); }

}  // namespace sgpr
