// map_nd.hip -- the symplectic map of a fit with d canonical pairs per point, forwards (with or without its tangent map:
// maptan.h sums the Hessian, tangent_core.h, shared with map.hip, has what follows from it) and backwards: every step of one
// orbit inside one workgroup.  gram_nd.hip has the kernel's derivation, nd_eval.h its entry formulas.
//
// x = (q_1..q_d, P_1..P_d), G(x) = K*(x) alpha as predict_nd_kernel forms it: G_q = dF/dq = p - P, G_P = dF/dP = Q - q.  One step
// solves f(P) = G_q(q, P) - p + P = 0 for P in R^d by Newton from P = p, then Q = q + G_P(q, P).  The Jacobian is analytic:
// one pass over the training points accumulates the 2d sums of G and the d^2 sums of dG_q/dP together (15 at d = 3).  With
// dx = x_train - x, E = sig k, S = sum_b g_b alpha_b and T_c = nh_c alpha_c - g_c (S - g_c alpha_c)  (G_c = sum_j E T_c),
//     d(G)_c / dP_e = - sum_j E [ g_e T_c + g_c alpha_e (nh_e + g_e^2) ]     (c a q index, e a P index: c != e always, so no
// third derivative of a factor appears; dE/ddx_e = E g_e, dg_e/ddx_e = -(nh_e + g_e^2)).  The sum kernels' G_q does not depend
// on P: their Jacobian sums are not formed and the first Newton step is exact.
#include <type_traits>
#include "common.h"
#include "devmath.h"
#include "generated/pair_generated.h"
#include "nd_args.h"

namespace sgpr {

namespace {

using namespace nd;         // all_coords, weights, is_sum, dispatch_nd (nd_eval.h); NdArgs, fill_args (nd_args.h); finite_d (devmath.h)

constexpr int MAPND_T_SMALL = 256, MAPND_T_LARGE = 512;    // threads per orbit: n0 <= MAPND_STAGE_PTS / larger training sets
constexpr int MAPND_STAGE_PTS = 4 * MAPND_T_SMALL;         // training points a 256-thread workgroup keeps in LDS (2 D doubles each: 96 KiB at D = 6)

// The staged points, where a kernel has them: a pointer into LDS by its type.  As a generic pointer the compiler merged the
// staged and the unstaged reads of a pass into flat loads through a pointer chosen per thread, and with the step in a function
// of its own (mapnd_step) the backend failed on that cast ("illegal instruction": the LDS aperture moved into VCC).
typedef const __attribute__((address_space(3))) double *stage_ptr;

struct MapNdArgs {
    NdArgs k;                          // Xa = training points (mj = n0 of them), the hyper-parameters
    int nm, ntest, mode, maxiter;
    double tol;
    const double *alpha;               // 2 d n0
    const double *Q0, *P0;             // ntest x d, column-major, leading dimension ntest
    double *qmap, *pmap;               // [nm][ntest][d]
    int *iters;                        // [nm - 1][ntest], may be null
};

#include "tangent_core.h"   // block_sum_n; the step matrix and the monodromy / Benettin step of the TAN instances

// G = K*(x) alpha (D sums) and, with JAC, J[c * d + e] = d G_c / d P_e (d^2 sums) over all n0 training points: thread t takes
// the points t, t + TT, ...  `stg`: the staged points ([coordinate | alpha block][MAPND_STAGE_PTS]) or null (read from memory)
template <int FAM, int D, int TT, bool JAC>
__device__ __forceinline__ void mapnd_pass(const MapNdArgs &a, const double (&x)[D], stage_ptr stg, double (&G)[D],
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

#include "maptan.h"   // the Hessian pass of the tangent map: with tangent_core.h what TAN = true adds to the kernel below

// One forward step from (q, p), the step of every kernel that runs the map forwards (applymap_nd_kernel, periodic_nd_kernel):
// explicit or Newton in P, the closing pass, the acceptance rule and the wrap.  Block-uniform values, every thread alike.
// -> whether the step is accepted; then P, Q (wrapped with SGPR_MAP_WRAP_Q) hold the image, x = (q, P) is the point of the
// passes, turn[c] = floor(Q_c / 2 pi), the turns the wrap took out of Q_c (0 without the wrap), `its` the Newton iterations.
// part / res: the two LDS halves of the workgroup sums, alternating with seq.
template <int FAM, int D, int TT, int PH, int RH>
__device__ __forceinline__ bool mapnd_step(const MapNdArgs &a, stage_ptr stg, const double (&q)[D / 2], const double (&p)[D / 2],
                                           double (&x)[D], double (&Q)[D / 2], double (&P)[D / 2], double (&turn)[D / 2], int &its,
                                           unsigned &seq, double (&part)[2][PH], double (&res)[2][RH])
{
    constexpr int d = D / 2;
    const double nan = __builtin_nan("");
    const double twopi = 6.283185307179586477;
    bool good = true;
#pragma unroll
    for (int c = 0; c < d; ++c) good = good && finite_d(q[c]) && finite_d(p[c]);   // a lost (NaN) orbit stays lost
    its = 0;
    double G[D], J[d * d];
#pragma unroll
    for (int c = 0; c < d; ++c) { x[c] = q[c]; P[c] = p[c]; Q[c] = nan; turn[c] = 0.0; }
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
            if (a.mode & SGPR_MAP_WRAP_Q) {
                turn[c] = floor(Q[c] / twopi);
                Q[c] -= twopi * turn[c];
            }
        }
    }
    return good;
}

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
    stage_ptr stg = nullptr;
    if (HAS_STAGE && n0 <= MAPND_STAGE_PTS) {
        for (int j = threadIdx.x; j < n0; j += TT) {
#pragma unroll
            for (int c = 0; c < D; ++c) {
                stage[c * MAPND_STAGE_PTS + j] = a.k.Xa[(size_t)j + (size_t)c * a.k.ldxa];
                stage[(D + c) * MAPND_STAGE_PTS + j] = a.alpha[(size_t)c * n0 + j];
            }
        }
        stg = (stage_ptr)stage;
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
    if constexpr (TAN) maptan_init<D>();
    for (int i = 0; i + 1 < a.nm; ++i) {
        int its = 0;
        double x[D], P[d], Q[d], turn[d];                   // block-uniform, like everything below
        const bool good = mapnd_step<FAM, D, TT>(a, stg, q, p, x, Q, P, turn, its, seq, part, res);
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
            maptan_advance<D, false>();
        }
    }
    if constexpr (TAN) maptan_finish<D>(a.mono, a.lyap, a.nm, k);
}

#include "periodic_nd.h"   // periodic_nd_kernel: Newton on the n-fold map around mapnd_step and the TAN pieces above

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
    stage_ptr stg = nullptr;
    if (HAS_STAGE && n0 <= MAPND_STAGE_PTS) {               // as applymap_nd_kernel: every thread reads back what it wrote itself
        for (int j = threadIdx.x; j < n0; j += TT) {
#pragma unroll
            for (int c = 0; c < D; ++c) {
                stage[c * MAPND_STAGE_PTS + j] = a.k.Xa[(size_t)j + (size_t)c * a.k.ldxa];
                stage[(D + c) * MAPND_STAGE_PTS + j] = a.alpha[(size_t)c * n0 + j];
            }
        }
        stg = (stage_ptr)stage;
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

}  // namespace

// threads per orbit, from n0 alone: up to MAPND_STAGE_PTS points (4 per thread, the d = 1 kernel's staging depth) run from LDS
// on 256 threads; more points go to 512 threads (see applymap_nd_kernel for why not 1024).  DESIGN 3.8 has the measured passes.
static int applymap_nd_threads(int n0) { return n0 <= MAPND_STAGE_PTS ? MAPND_T_SMALL : MAPND_T_LARGE; }

// The one launcher of the three entries below.  `a` is a zeroed MapNdArgs -- or MapNdTanArgs, whose own three pointers the
// tangent entry has set -- and is filled here; `kernel(fam, dd, tt)` names the entry's kernel instance for the family, D = 2 d
// and the threads per orbit.  Everything is device-resident: Xtr (n0 x 2d, ldxtr), alpha (2 d n0), Q0 / P0 (ntest x d, leading
// dimension ntest), qmap / pmap ([nm][ntest][d]), iters ([nm - 1][ntest] or null).
template <typename Args, typename Kernel>
static int applymap_nd_launch(Args &a, Kernel &&kernel, int family, int d, int mode, int nm, int ntest, int n0, const double *Xtr,
                              size_t ldxtr, const double *hyp, int nhyp, const double *alpha, const double *Q0, const double *P0,
                              double *qmap, double *pmap, int *iters, hipStream_t st)
{
    int rc = fill_args(family, d, hyp, nhyp, a.k);
    if (rc) return rc;
    if (nm <= 0 || ntest <= 0) return 0;
    a.k.mj = n0; a.k.Xa = Xtr; a.k.ldxa = ldxtr;
    a.nm = nm; a.ntest = ntest; a.mode = mode; a.maxiter = 60; a.tol = 1e-13;   // the d = 1 map's tol and maxiter
    a.alpha = alpha; a.Q0 = Q0; a.P0 = P0; a.qmap = qmap; a.pmap = pmap; a.iters = iters;
    const bool small = applymap_nd_threads(n0) == MAPND_T_SMALL;
    return dispatch_nd(family, d, [&](auto fam, auto dd) {
        using Small = std::integral_constant<int, MAPND_T_SMALL>;
        using Large = std::integral_constant<int, MAPND_T_LARGE>;
        if (small) hipLaunchKernelGGL(kernel(fam, dd, Small()), dim3(ntest), dim3(MAPND_T_SMALL), 0, st, a);
        else       hipLaunchKernelGGL(kernel(fam, dd, Large()), dim3(ntest), dim3(MAPND_T_LARGE), 0, st, a);
        SGPR_CHECK_LAUNCH();
        return 0;
    });
}

// mode: SGPR_MAP_WRAP_Q | SGPR_MAP_EXPLICIT (checked by the C entries)
int applymap_nd(int family, int d, int mode, int nm, int ntest, int n0, const double *Xtr, size_t ldxtr, const double *hyp,
                int nhyp, const double *alpha, const double *Q0, const double *P0, double *qmap, double *pmap, int *iters,
                hipStream_t st)
{
    MapNdArgs a{};
    auto kernel = [](auto fam, auto dd, auto tt) {
        return applymap_nd_kernel<decltype(fam)::value, decltype(dd)::value, decltype(tt)::value>;
    };
    return applymap_nd_launch(a, kernel, family, d, mode, nm, ntest, n0, Xtr, ldxtr, hyp, nhyp, alpha, Q0, P0, qmap, pmap, iters, st);
}

// the backward orbit: Q0 / P0 hold the images (Q, P), row i of qmap / pmap is the i-th preimage.  Arguments and shapes as
// applymap_nd; mode: SGPR_MAP_WRAP_Q only (the C entries refuse SGPR_MAP_EXPLICIT)
int applymap_nd_inverse(int family, int d, int mode, int nm, int ntest, int n0, const double *Xtr, size_t ldxtr, const double *hyp,
                        int nhyp, const double *alpha, const double *Q0, const double *P0, double *qmap, double *pmap, int *iters,
                        hipStream_t st)
{
    MapNdArgs a{};
    auto kernel = [](auto fam, auto dd, auto tt) {
        return applymap_nd_inverse_kernel<decltype(fam)::value, decltype(dd)::value, decltype(tt)::value>;
    };
    return applymap_nd_launch(a, kernel, family, d, mode, nm, ntest, n0, Xtr, ldxtr, hyp, nhyp, alpha, Q0, P0, qmap, pmap, iters, st);
}

// the same launch with the tangent map: jac ([nm - 1][ntest][D][D]), mono ([ntest][D][D]), lyap ([ntest][D]), each device-resident
// or null.  The orbit outputs have the bits of applymap_nd.
int applymap_nd_tangent(int family, int d, int mode, int nm, int ntest, int n0, const double *Xtr, size_t ldxtr, const double *hyp,
                        int nhyp, const double *alpha, const double *Q0, const double *P0, double *qmap, double *pmap, int *iters,
                        double *jac, double *mono, double *lyap, hipStream_t st)
{
    MapNdTanArgs a{};
    a.jac = jac; a.mono = mono; a.lyap = lyap;
    auto kernel = [](auto fam, auto dd, auto tt) {
        return applymap_nd_kernel<decltype(fam)::value, decltype(dd)::value, decltype(tt)::value, true>;
    };
    return applymap_nd_launch(a, kernel, family, d, mode, nm, ntest, n0, Xtr, ldxtr, hyp, nhyp, alpha, Q0, P0, qmap, pmap, iters, st);
}

// Periodic orbits of the map of applymap_nd (periodic_nd.h): per guess (Q0, P0) Newton on the n-fold map with the winding
// numbers wind (ntest x d, leading dimension ntest, or null), every pass inside the one launch.  Device buffers: z [ntest][2d],
// resid [ntest], its [ntest]; mono [ntest][2d][2d] or null; qorb / porb [n][ntest][d] or both null.  mode as applymap_nd_tangent.
int periodic_nd(int family, int d, int mode, int n, int ntest, int n0, const double *Xtr, size_t ldxtr, const double *hyp, int nhyp,
                const double *alpha, const int *wind, const double *Q0, const double *P0, double tol, int maxit, double *z,
                double *resid, int *its, double *mono, double *qorb, double *porb, hipStream_t st)
{
    PeriodicNdArgs a{};
    a.wind = wind; a.ptol = tol; a.pmaxit = maxit; a.z = z; a.resid = resid; a.its = its; a.mono = mono;
    auto kernel = [](auto fam, auto dd, auto tt) {
        return periodic_nd_kernel<decltype(fam)::value, decltype(dd)::value, decltype(tt)::value>;
    };
    return applymap_nd_launch(a, kernel, family, d, mode, n, ntest, n0, Xtr, ldxtr, hyp, nhyp, alpha, Q0, P0, qorb, porb, nullptr, st);
}

}  // namespace sgpr
