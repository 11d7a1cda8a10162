// batch.hip -- many small independent fits in ONE launch.
//
// The reference's only batch axis: `nphmap` independent GP pairs, one per toroidal section, and the
// CMA-ES populations that evaluate nll_chol for a set of hyper-parameter vectors over the same data
// (python/05_tokamak/Split_SympGPR/main.py:36-41,63-66,96-112), at matrix orders n = 40 ... 160.  At
// those sizes one nll_chol through a device-resident handle is pure set-up (create / upload / five
// launches / download: 0.2 - 1 ms, tools/nll_call_cost.py); here one workgroup runs the whole body of
// nll_chol (python/functions/func.py:189-196) for one problem -- Gram build, Cholesky, both triangular
// solves, the negative log-likelihood -- and a launch covers the batch.
//
// Per problem (order n <= 256 = two leaves): Ky -> scratch (global, L2-resident, 512 KiB per
// workgroup);  L11 = leaf(A11) in LDS (leaf.h), X11 = inv(L11);  L21 = A21 X11^T;  A22 -= L21 L21^T;
// L22 = leaf(A22);  y = L^-1 z and alpha = L^-T y through the leaf inverses.  Latency-bound by
// construction: throughput comes from the number of problems in flight, not from the matrix cores.
// Problems with d canonical pairs per point (sgpr_fit_batch_nd) take the same path behind a Gram stage of their own: the entry
// formulas of nd_eval.h, fit_batch_nd_kernel / mid_build_nd_kernel below.
#include <cmath>
#include <cstring>

#include "common.h"
#include "gemm_tile.h"
#include "leaf.h"
#include "loo_block.h"
#include "nllgrad_pair.h"
#include "nd_eval.h"
#include "pair_eval.h"

namespace sgpr {

namespace {

using namespace leaf;
using namespace pairf;

constexpr int BMAX = 2 * LEAF;            // largest order per problem
constexpr size_t PER_WG = (size_t)BMAX * BMAX + 2 * (size_t)LEAF * LEAF + 2 * BMAX;   // scratch doubles per workgroup (fit)

struct BatchArgs {
    int nbatch, npts, n, reg;
    const double *x, *y, *z;              // nbatch x npts, nbatch x npts, nbatch x n
    const KConst *kc;                     // per problem
    const double *noise;                  // per problem, >= 0
    double *scratch;                      // per workgroup: BMAX*BMAX (Ky / L) + 2*LEAF*LEAF (leaf inverses) + 2*BMAX
                                          // [+ BMAX*BMAX (U = L^-T) for the gradient and loo] [+ BMAX*BMAX (M) for the loo gradient]
    double *alpha, *nll;                  // outputs (alpha may be null); the gradient kernel writes problem b's raw sums at
                                          // nll + nbatch + b * grad_nacc<FAM>(), the loo kernel {loo, press} at nll + nbatch + 2 b,
                                          // the loo gradient kernel {loo, press, raw sums} at nll + nbatch + b * (2 + grad_nacc<FAM>())
    int *info;                            // per problem, zero on entry
    int which;                            // the loo gradient's objective (SGPR_LOO_LPD / SGPR_LOO_PRESS), the same for the launch
};

template <int FAM> constexpr bool grad_has_p() { return FAM == SGPR_FAM_D || (FAM == SGPR_FAM_USER && gen::user_has_p); }
template <int FAM> constexpr int grad_nacc() { return grad_has_p<FAM>() ? 5 : 4; }    // lx, ly, [p,] sig, sig2n

enum { MODE_FIT = 0, MODE_GRAD = 1, MODE_LOO = 2, MODE_LOOGRAD = 3 };

template <int FAM, int MODE>
__device__ void grad_problem(const BatchArgs &a, int b, double *s, double *A, const double *inv, double *U, const double *al);

// Everything of one problem behind its Gram stage, for the workgroup that has just written the lower triangle of Ky (order n, n1 =
// min(n, LEAF), n2 = n - n1) into A (ld = BMAX): the fence, both leaves, L21, the SYRK, y = L^-1 z and alpha = L^-T y through the
// leaf inverses, nll and the alpha write-out (alpha: the problem's row of the output or null).  Shared by the d = 1 kernel and
// the d-pair one (fit_batch_nd_kernel): one text, one sequence of operations.  s: LEAF_LDS doubles, red: LT / 64; v: y, then alpha
// at v + BMAX (al).  Ends on the fence and barrier that free A, inv and s for the next problem.
__device__ __forceinline__ void fit_solve_body(double *s, double *red, double *A, double *inv, double *v, double *al, const double *z,
                                               int n, int n1, int n2, double *alpha, double *nll, int *info)
{
    constexpr size_t ld = BMAX;
    const int tid = threadIdx.x;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // ---- L11, X11 = inv(L11)
    leaf_body(s, n1, A, ld, inv, info, 0, (int)LEAF_FACTOR,
              nullptr);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (n2 > 0) {
        // L21 = A21 X11^T  (X11 lower: k >= c), staged through LDS so that A21 can be overwritten
        for (int e = tid; e < n2 * n1; e += LT) {
            const int i = e % n2, c = e / n2;
            double acc = 0.0;
            for (int k = 0; k <= c; ++k) acc = __builtin_fma(A[(n1 + i) + k * ld], inv[c + k * LEAF], acc);
            s[e] = acc;
        }
        __syncthreads();
        for (int e = tid; e < n2 * n1; e += LT) A[(n1 + e % n2) + (e / n2) * ld] = s[e];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // A22 -= L21 L21^T (lower)
        for (int e = tid; e < n2 * n2; e += LT) {
            const int i = e % n2, j = e / n2;
            if (i < j) continue;
            double acc = A[(n1 + i) + (n1 + j) * ld];
            for (int k = 0; k < n1; ++k) acc = __builtin_fma(-A[(n1 + i) + k * ld], A[(n1 + j) + k * ld], acc);
            A[(n1 + i) + (n1 + j) * ld] = acc;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        leaf_body(s, n2, A + n1 + n1 * ld, ld, inv + LEAF * LEAF,
                  info, n1, (int)LEAF_FACTOR, nullptr);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    // ---- y = L^-1 z:  y1 = X11 z1;  y2 = X22 (z2 - L21 y1)
    double *yv = v;
    if (tid < n1) {
        double acc = 0.0;
        for (int k = 0; k <= tid; ++k) acc = __builtin_fma(inv[tid + k * LEAF], z[k], acc);
        yv[tid] = acc;
    }
    __syncthreads();
    if (n2 > 0) {
        if (tid < n2) {
            double acc = z[n1 + tid];
            for (int k = 0; k < n1; ++k) acc = __builtin_fma(-A[(n1 + tid) + k * ld], yv[k], acc);
            s[tid] = acc;
        }
        __syncthreads();
        if (tid < n2) {
            double acc = 0.0;
            const double *X22 = inv + LEAF * LEAF;
            for (int k = 0; k <= tid; ++k) acc = __builtin_fma(X22[tid + k * LEAF], s[k], acc);
            yv[n1 + tid] = acc;
        }
        __syncthreads();
        // ---- alpha = L^-T y:  a2 = X22^T y2;  a1 = X11^T (y1 - L21^T a2)
        if (tid < n2) {
            double acc = 0.0;
            const double *X22 = inv + LEAF * LEAF;
            for (int k = tid; k < n2; ++k) acc = __builtin_fma(X22[k + tid * LEAF], yv[n1 + k], acc);
            al[n1 + tid] = acc;
        }
        __syncthreads();
        if (tid < n1) {
            double acc = yv[tid];
            for (int k = 0; k < n2; ++k) acc = __builtin_fma(-A[(n1 + k) + tid * ld], al[n1 + k], acc);
            s[tid] = acc;
        }
        __syncthreads();
    } else {
        if (tid < n1) s[tid] = yv[tid];
        __syncthreads();
    }
    if (tid < n1) {
        double acc = 0.0;
        for (int k = tid; k < n1; ++k) acc = __builtin_fma(inv[k + tid * LEAF], s[k], acc);
        al[tid] = acc;
    }
    __syncthreads();
    // ---- nll = z.alpha / 2 + sum log L_ii  (func.py:195)
    double q = 0.0;
    for (int i = tid; i < n; i += LT) q += 0.5 * z[i] * al[i] + log(A[i + i * ld]);
    for (int o = 32; o > 0; o >>= 1) q += __shfl_down(q, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = q;
    __syncthreads();
    if (tid == 0) *nll = red[0] + red[1] + red[2] + red[3];
    if (alpha)
        for (int i = tid; i < n; i += LT) alpha[i] = al[i];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// MODE_GRAD: after the fit, the gradient of problem b's nll (grad_problem below); MODE_LOO: its leave-one-point-out sums
// (grad_problem's Ky^-1, then one thread per point).  Scratch then PER_WG + BMAX^2 doubles per workgroup.  MODE_LOOGRAD: the sums
// and the gradient of one of them; a third block (M): PER_WG + 2 BMAX^2 doubles = 1 839 104 bytes (~1.8 MiB) per workgroup, ~1.8 GiB at
// the 1024-workgroup grid
template <int FAM, int MODE = MODE_FIT>
__global__ __launch_bounds__(LT) void fit_batch_kernel(const BatchArgs a)
{
    __shared__ double s[LEAF_LDS];
    __shared__ double red[LT / 64];
    const int tid = threadIdx.x;
    const int n = a.n, N = a.npts;
    const size_t per_wg = (size_t)BMAX * BMAX + 2 * (size_t)LEAF * LEAF + 2 * BMAX + (MODE != MODE_FIT ? (size_t)BMAX * BMAX : 0) +
                          (MODE == MODE_LOOGRAD ? (size_t)BMAX * BMAX : 0);                    // PER_WG [+ U] [+ M]
    double *A = a.scratch + (size_t)blockIdx.x * per_wg;     // column-major, ld = BMAX
    double *inv = A + (size_t)BMAX * BMAX;
    double *v = inv + 2 * (size_t)LEAF * LEAF;                // y, then alpha
    constexpr size_t ld = BMAX;
    const int n1 = min(n, (int)LEAF), n2 = n - n1;
    for (int b = blockIdx.x; b < a.nbatch; b += gridDim.x) {
        const KConst kc = a.kc[b];
        const double *x = a.x + (size_t)b * N, *y = a.y + (size_t)b * N, *z = a.z + (size_t)b * n;
        const double noise = a.noise[b];
        // ---- Ky = build_K(x, x) + |sig2n| I (lower triangle; func.py:191-192) or buildKreg (func.py:182-183)
        if (a.reg) {
            for (int e = tid; e < N * N; e += LT) {
                const int i = e % N, j = e / N;
                if (i < j) continue;
                double k = kc.sig * kern_eval<FAM, false>(x[j], y[j], x[i], y[i], kc);
                if (i == j) k += noise;
                A[i + j * ld] = k;
            }
        } else {
            for (int e = tid; e < N * N; e += LT) {
                const int i = e % N, j = e / N;               // pair (row point i, column point j)
                double kxx, kxy, kyy;
                pair_eval<FAM, false>(x[j], y[j], x[i], y[i], kc, kxx, kxy, kyy);
                if (i == j) { kxx += noise; kyy += noise; }
                A[(N + i) + j * ld] = kxy;                    // Pq block: always below the diagonal
                if (i >= j) {
                    A[i + j * ld] = kxx;
                    A[(N + i) + (N + j) * ld] = kyy;
                }
            }
        }
        double *al = v + BMAX;
        fit_solve_body(s, red, A, inv, v, al, z, n, n1, n2, a.alpha ? a.alpha + (size_t)b * n : nullptr, a.nll + b, a.info + b);
        if constexpr (MODE != MODE_FIT) grad_problem<FAM, MODE>(a, b, s, A, inv, v + 2 * BMAX, al);
    }
}

// ---- d canonical pairs per point (D = 2 d coordinates, order n = D N <= BMAX): the fit of fit_batch_kernel with the Gram
// stage of gram_nd.hip.  Ky is (D)^2 blocks of N x N, block (ca, cb) at rows ca N, columns cb N; a point pair (i, j) is evaluated
// once (one exp, d sincos: nd_eval.h) and feeds its entry of every block of the LOWER triangle: blocks ca > cb whole, blocks
// ca = cb for i >= j, blocks ca < cb not at all; the noise sits on the diagonal of the blocks ca = cb.  The sum kernels' blocks
// ca > cb are written as the zeros they are (the scratch holds the previous problem's factor).
struct BatchNdArgs {
    int nbatch, npts, n;
    const double *X, *z;                  // nbatch x D x npts (coordinate m of point i of problem b at (b D + m) npts + i), nbatch x n
    const nd::NdConst *nc;                // per problem
    const double *noise;                  // per problem, >= 0
    double *scratch;                      // per workgroup: PER_WG doubles, as fit_batch_kernel<FAM, MODE_FIT>
    double *alpha, *nll;                  // outputs (alpha may be null)
    int *info;                            // per problem, zero on entry
};

// entry (i, j) of the blocks (ca, 0 .. ca) of one evaluated pair into the lower triangle at P = A + i + j ld (ld: the leading
// dimension, N the block size); one row of blocks is live at a time
template <int FAM, int D>
__device__ __forceinline__ void store_pair_lower(double *P, size_t ld, int N, bool on_or_below, bool diag, double noise,
                                                 const double (&E)[D], const double (&g)[D], const double (&nh)[D])
{
#pragma unroll
    for (int ca = 0; ca < D; ++ca) {
#pragma unroll
        for (int cb = 0; cb < ca; ++cb)
            P[(size_t)ca * N + (size_t)cb * N * ld] = nd::is_sum<FAM>() ? 0.0 : -E[ca] * (g[ca] * g[cb]);
        if (on_or_below) P[(size_t)ca * N + (size_t)ca * N * ld] = __builtin_fma(E[ca], nh[ca], diag ? noise : 0.0);
    }
}

template <int FAM, int D>
__global__ __launch_bounds__(LT) void fit_batch_nd_kernel(const BatchNdArgs a)
{
    __shared__ double s[LEAF_LDS];
    __shared__ double red[LT / 64];
    const int tid = threadIdx.x;
    const int n = a.n, N = a.npts;
    double *A = a.scratch + (size_t)blockIdx.x * PER_WG;      // column-major, ld = BMAX
    double *inv = A + (size_t)BMAX * BMAX;
    double *v = inv + 2 * (size_t)LEAF * LEAF;                // y, then alpha
    constexpr size_t ld = BMAX;
    const int n1 = min(n, (int)LEAF), n2 = n - n1;
    for (int b = blockIdx.x; b < a.nbatch; b += gridDim.x) {
        const nd::NdConst nc = a.nc[b];
        const double *X = a.X + (size_t)b * D * N, *z = a.z + (size_t)b * n;
        const double noise = a.noise[b];
        // the problem's points into LDS (D N <= BMAX doubles; fit_solve_body's closing barrier has freed s)
        for (int e = tid; e < D * N; e += LT) s[e] = X[e];
        __syncthreads();
        for (int e = tid; e < N * N; e += LT) {
            const int i = e % N, j = e / N;                   // pair (row point i, column point j)
            double xa[D], xb[D], arg[D], g[D], nh[D], E[D];
#pragma unroll
            for (int m = 0; m < D; ++m) { xa[m] = s[m * N + j]; xb[m] = s[m * N + i]; }
            nd::all_coords<FAM, D>(nc, xa, xb, arg, g, nh);
            nd::weights<FAM, D>(nc, arg, E);
            store_pair_lower<FAM, D>(A + i + j * ld, ld, N, i >= j, i == j, noise, E, g, nh);
        }
        fit_solve_body(s, red, A, inv, v, v + BMAX, z, n, n1, n2, a.alpha ? a.alpha + (size_t)b * n : nullptr, a.nll + b, a.info + b);
    }
}

// Point i's leave-one-point-out quantities from the lower triangle of Ky^-1 (A) and alpha: its block {A[i,i], A[N+i,i], A[N+i,N+i]}
// (one entry for reg) through loo_block.h -> r, S (packed lower; the entries a reg fit does not have are zero), lpd and |r|^2.
__device__ __forceinline__ void loo_point(const double *A, const double *al, int i, int N, int reg, double (&r)[2], double (&S)[3],
                                          double &lpd, double &rr)
{
    constexpr size_t ld = BMAX;
    if (reg) {
        const double C[1] = {A[i + i * ld]}, ai[1] = {al[i]};
        double r1[1], S1[1];
        loo::block<1>(C, ai, r1, S1, lpd);
        rr = r1[0] * r1[0];
        r[0] = r1[0]; r[1] = 0.0;
        S[0] = S1[0]; S[1] = 0.0; S[2] = 0.0;
    } else {
        const double C[3] = {A[i + i * ld], A[(N + i) + i * ld], A[(N + i) + (N + i) * ld]}, ai[2] = {al[i], al[N + i]};
        loo::block<2>(C, ai, r, S, lpd);
        rr = __builtin_fma(r[1], r[1], r[0] * r[0]);
    }
}

// The per-thread {lpd, |r|^2} fold wave by wave in a fixed order (through s[0 .. 7]) into out = {loo, press}.  Ends on a barrier.
__device__ __forceinline__ void loo_fold(const double (&lv)[2], double *s, double *out)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        double v = lv[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) s[wave * 2 + k] = v;
    }
    __syncthreads();
    if (tid < 2) {
        const double v = s[tid] + s[2 + tid] + s[4 + tid] + s[6 + tid];
        out[tid] = tid == 0 ? -v : v;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// Step (3) of grad_problem, for any symmetric weight: thread i owns row i of W, given as wf(i, alpha_i, col) for col <= i, and walks
// the column points j, each pair evaluated once with dK from the generated forms (nllgrad_pair.h), entries on and below the
// diagonal weighted W_ii and 2 W_ij; W_ii also goes to the noise sum.  The points and alpha go to LDS first (s: x | y | alpha at
// multiples of BMAX, the wave partials behind them).  The per-thread sums fold wave by wave in a fixed order into out[0 .. NACC).
template <int FAM, class WF>
__device__ __forceinline__ void contract_rows(const BatchArgs &a, int b, double *s, const double *al, double *out, WF wf)
{
    constexpr bool HASP = grad_has_p<FAM>();
    constexpr int NACC = grad_nacc<FAM>();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = tid;
    const int n = a.n, N = a.npts;
    double *sx = s, *sy = s + BMAX, *sal = s + 2 * BMAX, *red = s + 3 * BMAX;
    for (int e = tid; e < N; e += LT) { sx[e] = a.x[(size_t)b * N + e]; sy[e] = a.y[(size_t)b * N + e]; }
    for (int e = tid; e < n; e += LT) sal[e] = al[e];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const KConst kc = a.kc[b];
    const double l[2] = {kc.lx, kc.ly}, pp[1] = {kc.p};
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    if (i < n) {
        const double ai = sal[i];
        if (a.reg) {
            const double xi = sx[i], yi = sy[i];
            for (int j = 0; j <= i; ++j) {
                const double W = wf(i, ai, j);
                if (j == i) acc[NACC - 1] += W;
                nllg::reg_grad<FAM, HASP>(sx[j], sy[j], xi, yi, j == i ? W : 2.0 * W, l, kc.p, acc);
            }
        } else {
            const int r = i < N ? 0 : 1, pi = i - r * N;
            const double xi[2] = {sx[pi], sy[pi]};
            for (int pj = 0; pj < N; ++pj) {
                double w[2];
                bool any = false;
#pragma unroll
                for (int c = 0; c < 2; ++c) {                 // columns pj (q part) and N + pj (P part)
                    const int col = c * N + pj;
                    w[c] = 0.0;
                    if (col <= i) {
                        const double W = wf(i, ai, col);
                        if (col == i) { w[c] = W; acc[NACC - 1] += W; }
                        else w[c] = 2.0 * W;
                        any = true;
                    }
                }
                if (!any) break;                              // column pj > i: so are all after it
                const double xj[2] = {sx[pj], sy[pj]};
                nllg::pair_grad<FAM, 2, HASP>(xi, xj, w, r, l, pp, acc);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        double v = acc[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) red[wave * NACC + k] = v;
    }
    __syncthreads();
    if (tid < NACC) out[tid] = red[tid] + red[NACC + tid] + red[2 * NACC + tid] + red[3 * NACC + tid];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                      // A, U and s are the next problem's
}

// The gradient of problem b's nll in (lx, ly, [p,] sig, sig2n), by the workgroup that has just fitted it: A holds L, inv the
// leaf inverses X11 = L11^-1 and X22 = L22^-1, al alpha; U is BMAX^2 doubles of the workgroup's scratch.
//   (1) U = L^-T, column-major, zero below the diagonal:  L^-1 = [[X11, 0], [-X22 L21 X11, X22]];  T = L21 X11 goes through LDS.
//   (2) Ky^-1 = L^-T L^-1 = U U^T, lower triangle, into A (over L: the nll has read its diagonal):  n^3 / 3 flop.
//   (3) thread i owns row i of W = Ky^-1 - alpha alpha^T and walks the column points j, each pair evaluated once with dK from
//       the generated forms (nllgrad_pair.h), entries on and below the diagonal weighted W_ii and 2 W_ij.  The per-thread
//       sums fold wave by wave in a fixed order: a problem's bits do not depend on its place in the batch or on the grid.
// The sums leave unscaled, as nll_grad_full's (nllgrad.hip): the host applies sig / 2, 1/2 and sign(sig2n) / 2.
// MODE_LOO: steps (1) and (2), then in place of (3) thread i < N takes point i's block {A[i,i], A[N+i,i], A[N+i,N+i]} of Ky^-1 (one
// entry for reg) through loo_block.h; lpd and |r|^2 fold wave by wave in the same fixed order into {loo, press}.
// MODE_LOOGRAD: MODE_LOO's steps and sums by the same code (the same bits), then the gradient of loo or press (a.which) by the
// formulas of loograd.hip, with a third BMAX^2 block M behind U:
//   (L1) thread i < N keeps point i's weight block W~_i (packed lower, 3 doubles; 1 for reg) and v[B_i] in LDS:
//        loo  W~_i = r_i r_i^T + S_i, v = r_i;   press  W~_i = 2 (r_i s_i^T + s_i r_i^T), v = 2 s_i, s_i = S_i r_i.
//        Meanwhile thread i MIRRORS row i of Ky^-1 into column i: A is full and symmetric from here on, every later read of
//        Ky^-1 is a plain A[row + col ld] with the row on the lanes;
//   (L2) beta = Ky^-1 v, thread i its entry (n^2 flop), into LDS;  Y = W~ Ky^-1 over U (dead after (2)): row c N + i of Y is
//        sum_e W~_i[c, e] (row e N + i of Ky^-1), two rows of Ky^-1 per row of Y;
//   (L3) M = Ky^-1 Y, lower triangle, thread i its row, four columns at a time, k = 0 .. n - 1 in order: n^3 flop; what is stored
//        in the third block is W' = M - beta alpha^T - alpha beta^T (the weight is then one load per entry in (L4): with the three
//        terms formed there the family D instance spilled 20 bytes per lane);
//   (L4) step (3) on W' (contract_rows: the same code as the nll gradient's).
// A point whose block has a pivot that is not positive and finite has NaN in W~_i: two rows of Y, so all of M, so every sum.
// Output: {loo, press, the NACC raw sums}, unscaled.
template <int FAM, int MODE>
__device__ void grad_problem(const BatchArgs &a, int b, double *s, double *A, const double *inv, double *U, const double *al)
{
    constexpr int NACC = grad_nacc<FAM>(), NOUT = MODE == MODE_LOO ? 2 : MODE == MODE_LOOGRAD ? 2 + NACC : NACC;
    constexpr size_t ld = BMAX;
    const int tid = threadIdx.x;
    const int n = a.n, N = a.npts, n1 = min(n, (int)LEAF), n2 = n - n1;
    double *out = a.nll + a.nbatch + (size_t)b * NOUT;
    // not positive definite (leaf_body's flag, read from L2: the same value for every thread): NaN, nothing computed
    if (__hip_atomic_load(a.info + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
        if (tid < NOUT) out[tid] = __builtin_nan("");
        return;
    }
    // ---- (1) U = L^-T.  The diagonal blocks (transposed leaf inverses) and the zeros; U[i + k ld] = (L^-1)[k, i]
    for (int e = tid; e < n * n; e += LT) {
        const int i = e % n, k = e / n;
        if (i < n1 && k >= n1) continue;                  // the block right of X11^T: below
        double u = 0.0;
        if (k >= i) u = k < n1 ? inv[k + i * LEAF] : inv[LEAF * LEAF + (k - n1) + (i - n1) * LEAF];
        U[i + k * ld] = u;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (n2 > 0) {                                         // then n1 = LEAF
        // T = L21 X11 (n2 x LEAF) into LDS, T[m, c] at s[c + m LEAF]; X11[q, c] = U[c + q ld], zero for q < c, so a wave
        // (64 consecutive c) may start at its first c
        for (int e = tid; e < n2 * (int)LEAF; e += LT) {
            const int c = e % LEAF, m = e / LEAF;
            double acc = 0.0;
            for (int q = c & ~63; q < (int)LEAF; ++q) acc = __builtin_fma(A[(n1 + m) + q * ld], U[c + q * ld], acc);
            s[e] = acc;
        }
        __syncthreads();
        // (L^-1)_21 = -X22 T:  its row k is column n1 + k of U
        const double *X22 = inv + LEAF * LEAF;
        for (int e = tid; e < n2 * (int)LEAF; e += LT) {
            const int c = e % LEAF, k = e / LEAF;
            double acc = 0.0;
            for (int m = 0; m <= k; ++m) acc = __builtin_fma(-X22[k + m * LEAF], s[c + m * LEAF], acc);
            U[c + (n1 + k) * ld] = acc;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    // ---- (2) Ky^-1[i, j] = sum_{k >= i} U[i, k] U[j, k], i >= j: thread i (n <= LT); k starts at the wave's first row
    const int i = tid;
    for (int j = 0; j < n; ++j) {
        if (i < n && i >= j) {
            double acc = 0.0;
            for (int k = max(j, i & ~63); k < n; ++k) acc = __builtin_fma(U[i + k * ld], U[j + k * ld], acc);
            A[i + j * ld] = acc;
        }
    }
    [[maybe_unused]] double *sal = s + 2 * BMAX;          // contract_rows' alpha
    if constexpr (MODE == MODE_GRAD) {
        // ---- (3) the points and alpha into LDS (T is dead), then the contraction
        contract_rows<FAM>(a, b, s, al, out, [=](int row, double ai, int col) { return A[row + col * ld] - ai * sal[col]; });
        return;
    }
    // ---- the points of leave-one-point-out; LDS behind contract_rows' part: W~ (3 BMAX), v, beta
    [[maybe_unused]] double *sW = s + 4 * BMAX, *sv = s + 7 * BMAX, *sbeta = s + 8 * BMAX;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                      // point i's block has entries written by thread N + i; T is dead
    double lv[2] = {0.0, 0.0};
    if (i < N) {
        double r[2], S[3], lpd, rr;
        loo_point(A, al, i, N, a.reg, r, S, lpd, rr);
        lv[0] = lpd; lv[1] = rr;
        if constexpr (MODE == MODE_LOOGRAD) {
            // (L1) W~_i and v[B_i]
            double w[3], v[2];
            if (a.which == SGPR_LOO_PRESS) {
                const double sr[2] = {__builtin_fma(S[1], r[1], S[0] * r[0]), __builtin_fma(S[2], r[1], S[1] * r[0])};   // s = S r
#pragma unroll
                for (int e = 0; e < 2; ++e) {
#pragma unroll
                    for (int c = 0; c <= e; ++c) w[loo::pk(e, c)] = 2.0 * __builtin_fma(r[e], sr[c], sr[e] * r[c]);
                    v[e] = 2.0 * sr[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
#pragma unroll
                    for (int c = 0; c <= e; ++c) w[loo::pk(e, c)] = __builtin_fma(r[e], r[c], S[loo::pk(e, c)]);
                    v[e] = r[e];
                }
            }
            sW[i] = w[0]; sW[BMAX + i] = w[1]; sW[2 * BMAX + i] = w[2];
            sv[i] = v[0];
            if (!a.reg) sv[N + i] = v[1];
        }
    }
    if constexpr (MODE == MODE_LOOGRAD) {
        // the mirror: strictly above the diagonal, which no thread reads in this phase
        if (i < n)
            for (int j = 0; j < i; ++j) A[j + i * ld] = A[i + j * ld];
    }
    loo_fold(lv, s, out);                                 // ends on the fence: the mirror and the LDS vectors are visible
    if constexpr (MODE == MODE_LOOGRAD) {
        // ---- (L2) beta and Y
        if (i < n) {
            double acc = 0.0;
            for (int j = 0; j < n; ++j) acc = __builtin_fma(A[i + j * ld], sv[j], acc);
            sbeta[i] = acc;
            // row i = c N + pi of Y from the point's rows r0 = pi and r1 = N + pi of Ky^-1 (reg: its one row, the second weight is 0)
            const int c = (!a.reg && i >= N) ? 1 : 0, pi = i - c * N;
            const int r0 = pi, r1 = a.reg ? pi : N + pi;
            const double wa = sW[c * BMAX + pi], wb = sW[(c + 1) * BMAX + pi];
            for (int k = 0; k < n; ++k) U[i + k * ld] = __builtin_fma(wa, A[r0 + k * ld], wb * A[r1 + k * ld]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // ---- (L3) W'[i, j] from M[i, j] = sum_k Ky^-1[i, k] Y[k, j], i >= j: thread i, columns j0 .. j0 + 3 from one pass over
        // its row (a column past n - 1 is clamped: computed again, not stored)
        double *M = U + (size_t)BMAX * BMAX;
        for (int j0 = 0; j0 < n; j0 += 4) {
            if (i < n && i >= j0) {
                const double *y0 = U + j0 * ld, *y1 = U + min(j0 + 1, n - 1) * ld, *y2 = U + min(j0 + 2, n - 1) * ld,
                             *y3 = U + min(j0 + 3, n - 1) * ld;
                double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
                for (int k = 0; k < n; ++k) {
                    const double kik = A[i + k * ld];
                    m0 = __builtin_fma(kik, y0[k], m0);
                    m1 = __builtin_fma(kik, y1[k], m1);
                    m2 = __builtin_fma(kik, y2[k], m2);
                    m3 = __builtin_fma(kik, y3[k], m3);
                }
                const double bi = sbeta[i], ali = al[i];
                auto wp = [=](double m, int j) { return m - bi * al[j] - ali * sbeta[j]; };
                M[i + j0 * ld] = wp(m0, j0);
                if (j0 + 1 <= i) M[i + (j0 + 1) * ld] = wp(m1, j0 + 1);
                if (j0 + 2 <= i) M[i + (j0 + 2) * ld] = wp(m2, j0 + 2);
                if (j0 + 3 <= i) M[i + (j0 + 3) * ld] = wp(m3, j0 + 3);
            }
        }
        // ---- (L4) thread i reads the row of W' it wrote
        contract_rows<FAM>(a, b, s, al, out + 2, [=](int row, double, int col) { return M[row + col * ld]; });
    }
}

// ---- mid-size problems: 256 < n <= 2048 (a CMA-ES generation at N = 512 ... 1024 points) --------------------------
// Three launches for the whole batch: (1) every Ky_b, lower triangle, into an npad x npad image (npad = n rounded up to
// 128; the padding is an identity block: det 1, alpha 0 there); (2) chol.hip's panel_batch_kernel: W = npad / 128
// workgroups per problem run the leaf chain on their own matrix, problems side by side; (3) one workgroup per problem:
// y = L^-1 z and alpha = L^-T y through the leaf inverses, and the negative log-likelihood.
constexpr int MT = 256;                   // build: pair rows per tile (one per thread)
constexpr int MJ = 16;                    // build: pair columns per tile
constexpr int ST = 512;                   // solve: threads per problem

struct MidArgs {
    int nbatch, npts, n, npad, reg;
    const double *x, *y, *z;              // nbatch x npts, nbatch x npts, nbatch x n
    const KConst *kc;
    const double *noise;
    double *A;                            // problem b at A + b * npad * npad, ld = npad
    const double *inv;                    // leaf inverses: problem b at inv + b * (npad / 128) * 128 * 128
    double *alpha, *nll;
    const int *info;
};

template <int FAM>
__global__ __launch_bounds__(MT) void mid_build_kernel(const MidArgs a)
{
    __shared__ double sx[MJ], sy[MJ];
    const int b = blockIdx.z, N = a.npts, t = threadIdx.x;
    const int i0 = blockIdx.x * MT, j0 = blockIdx.y * MJ;
    const size_t ld = (size_t)a.npad;
    double *A = a.A + (size_t)b * ld * ld;
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (int r = a.n + t; r < a.npad; r += MT) A[r + r * ld] = 1.0;     // the padding's diagonal (the rest was cleared)
    const bool tile_lower = i0 + MT - 1 >= j0;        // some (i, j) of the tile has i >= j
    if (a.reg && !tile_lower) return;
    const double *x = a.x + (size_t)b * N, *y = a.y + (size_t)b * N;
    const int nj = min(MJ, N - j0);
    if (t < nj) { sx[t] = x[j0 + t]; sy[t] = y[j0 + t]; }
    __syncthreads();
    const int i = i0 + t;
    if (i >= N) return;
    const KConst kc = a.kc[b];
    const double noise = a.noise[b];
    const double xi = x[i], yi = y[i];
    if (a.reg) {
        for (int jj = 0; jj < nj; ++jj) {
            const int j = j0 + jj;
            if (i < j) break;
            double k = kc.sig * kern_eval<FAM, false>(sx[jj], sy[jj], xi, yi, kc);
            if (i == j) k += noise;
            A[i + j * ld] = k;
        }
        return;
    }
    for (int jj = 0; jj < nj; ++jj) {
        const int j = j0 + jj;
        double kxx, kxy, kyy;
        pair_eval<FAM, false>(sx[jj], sy[jj], xi, yi, kc, kxx, kxy, kyy);
        if (i == j) { kxx += noise; kyy += noise; }
        A[(N + i) + j * ld] = kxy;                     // Pq block: always below the diagonal
        if (i >= j) {
            A[i + j * ld] = kxx;
            A[(N + i) + (N + j) * ld] = kyy;
        }
    }
}

// The build for d canonical pairs per point (D = 2 d, n = D N): mid_build_kernel's tiling -- MT point rows per workgroup, one per
// thread, MJ point columns in LDS, now D coordinates each, blockIdx.z the problem -- and fit_batch_nd_kernel's entries and
// lower-triangle rule (store_pair_lower) at ld = npad.
struct MidNdArgs {
    int npts, n, npad;
    const double *X;                      // nbatch x D x npts
    const nd::NdConst *nc;
    const double *noise;
    double *A;                            // problem b at A + b * npad * npad, ld = npad
};

template <int FAM, int D>
__global__ __launch_bounds__(MT) void mid_build_nd_kernel(const MidNdArgs a)
{
    __shared__ double sxa[MJ][D];
    const int b = blockIdx.z, N = a.npts, t = threadIdx.x;
    const int i0 = blockIdx.x * MT, j0 = blockIdx.y * MJ;
    const size_t ld = (size_t)a.npad;
    double *A = a.A + (size_t)b * ld * ld;
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (int r = a.n + t; r < a.npad; r += MT) A[r + r * ld] = 1.0;     // the padding's diagonal (the rest was cleared)
    const double *X = a.X + (size_t)b * D * N;
    const int nj = min(MJ, N - j0);
    for (int e = t; e < nj * D; e += MT) sxa[e / D][e % D] = X[(size_t)(e % D) * N + j0 + e / D];
    __syncthreads();
    const int i = i0 + t;
    if (i >= N) return;
    const nd::NdConst nc = a.nc[b];
    const double noise = a.noise[b];
    double xb[D];
#pragma unroll
    for (int m = 0; m < D; ++m) xb[m] = X[(size_t)m * N + i];
    for (int jj = 0; jj < nj; ++jj) {
        const int j = j0 + jj;
        double arg[D], g[D], nh[D], E[D];
        nd::all_coords<FAM, D>(nc, sxa[jj], xb, arg, g, nh);
        nd::weights<FAM, D>(nc, arg, E);
        store_pair_lower<FAM, D>(A + i + (size_t)j * ld, ld, N, i >= j, i == j, noise, E, g, nh);
    }
}

// Above order 1024 a problem is factored as two panels; between them, for every problem, the rank-k update of the block that
// is left: A22 -= L21 L21^T (lower tiles only), 128 x 128 tiles of the grid-wide MFMA kernel's LDS-DMA body (gemm_tile.h).
struct MidSyrk {
    double *A;            // problem b at A + b * stride (column-major, ld)
    size_t stride, ld;
    int k, m2;            // width of the first panel; order of the block behind it (multiples of 128)
};

__global__ __launch_bounds__(256, 2) void mid_syrk_kernel(const MidSyrk a)
{
    __shared__ double smem[2 * tile::BK * (2 * (128 + tile::PAD))];
    int t = (int)blockIdx.x, r = 0;            // lower tiles row by row: row r holds r + 1 of them
    while (t > r) { t -= r + 1; ++r; }
    double *base = a.A + (size_t)blockIdx.y * a.stride;
    tile::GemmArgs g{};
    g.m = a.m2; g.n = a.m2; g.k = a.k;
    g.alpha = -1.0; g.beta = 1.0;
    g.A = base + a.k; g.lda = a.ld;
    g.B = base + a.k; g.ldb = a.ld;
    g.C = base + a.k + (size_t)a.k * a.ld; g.ldc = a.ld;
    tile::gemm_body_dma<128, 128, 2>(g, smem, r, t);
}

__device__ __forceinline__ double wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;      // lane 0 holds the sum
}

// The solves of the batch: the right-hand sides padded to npad ...
__global__ __launch_bounds__(256) void mid_rhs_kernel(const MidArgs a, double *r)
{
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i < a.npad) r[(size_t)b * a.npad + i] = i < a.n ? a.z[(size_t)b * a.n + i] : 0.0;
}
// ... two launches of trsv.hip's strip solve over all problems (one workgroup per 128-row strip and problem, W x nbatch of
// them; round 3 ran both solves of a problem in ONE workgroup: 64 problems of order 1024 kept 64 CUs busy for 0.6 ms, a third
// of the whole call) ... and, per problem, nll = z.alpha / 2 + sum log L_ii (func.py:195) and alpha.
__global__ __launch_bounds__(ST) void mid_finish_kernel(const MidArgs a, const double *r, const int *state, int *info)
{
    __shared__ double red[ST / 64];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = a.n;
    const size_t ld = (size_t)a.npad;
    const double *A = a.A + (size_t)b * ld * ld;
    const double *z = a.z + (size_t)b * n;
    const double *al = r + (size_t)b * ld;
    // a strip solve that gave up on a hand-off (state word 2 of either pass): an error of the call, not a result
    if (a.info[b] == 0 && (state[8 * b + 2] | state[8 * b + 6]) != 0) {
        if (t == 0) { info[b] = SOLVE_HANDOFF_TIMEOUT; a.nll[b] = __builtin_nan(""); }
        return;
    }
    if (a.info[b] != 0) {                  // not positive definite: the host turns info into NaN / +inf
        if (t == 0) a.nll[b] = __builtin_nan("");
        if (a.alpha)
            for (int i = t; i < n; i += ST) a.alpha[(size_t)b * n + i] = __builtin_nan("");
        return;
    }
    double q = 0.0;
    for (int i = t; i < n; i += ST) q += 0.5 * z[i] * al[i] + log(A[i + i * ld]);
    q = wave_sum(q);
    if (lane == 0) red[wave] = q;
    __syncthreads();
    if (t == 0) {
        double v = 0.0;
        for (int w = 0; w < ST / 64; ++w) v += red[w];
        a.nll[b] = v;
    }
    if (a.alpha)
        for (int i = t; i < n; i += ST) a.alpha[(size_t)b * n + i] = al[i];
}

// ---- the gradient of the mid-size problems (sgpr_fit_batch_grad_mid) -------------------------------------------------
// After the solves a problem's image holds L, `inv` its 128 x 128 leaf inverses and r its alpha.  Three steps, every one a
// grid over all problems of the chunk, ordered by the stream alone (no workgroup waits for another one):
//   (a) U = L^-T into a second image, U[i + k ld] = (L^-1)[k, i] as grad_problem's: the diagonal tiles are the transposed
//       leaf inverses (mid_udiag_kernel); then the block size doubles, 128, 256, ... : for adjacent diagonal blocks 1, 2
//           T = U11 L21^T   (STEP 0, NT, into the block (1, 2) of the L image: its strict upper triangle is free),
//           U12 = -T U22    (STEP 1, the TRANSB form),
//       one 128 x 128 tile per workgroup; the last block 2 is ragged when W is no power of two.  The k range of a tile stops
//       at the zeros of the triangular operand: U11's tile row ti starts at k = 128 ti, U22's tile column tj ends at
//       128 (tj + 1).
//   (b) Ky^-1 = U U^T, lower tiles, over L (mid_kinv_kernel): tile (I, J) sums k >= 128 I.
//   (c) the contraction of W = Ky^-1 - alpha alpha^T with dK (mid_grad_kernel) in per-workgroup partials, folded per problem in
//       a fixed order (mid_grad_fold_kernel).
// A problem that is not positive definite has an arbitrary image: every loop bound here comes from the shape alone.
constexpr int GT = 256;                   // contraction: rows per workgroup (one per thread)
constexpr int GCJ = 64;                   // contraction: column points per workgroup
constexpr int GPART = 8;                  // doubles per workgroup partial (>= grad_nacc)

struct MidInv {
    double *L, *U;        // problem b at L / U + b * stride (column-major, ld)
    const double *inv;    // its leaf inverses at inv + b * stride_inv
    size_t stride, ld, stride_inv;
    int W, S;             // 128-tiles per side; tiles per side of a (full) diagonal block of this level
};

__global__ __launch_bounds__(256) void mid_udiag_kernel(const MidInv a)
{
    const double *X = a.inv + (size_t)blockIdx.y * a.stride_inv + (size_t)blockIdx.x * LEAF * LEAF;
    double *U = a.U + (size_t)blockIdx.y * a.stride + (size_t)blockIdx.x * LEAF * (a.ld + 1);
    for (int e = threadIdx.x; e < (int)(LEAF * LEAF); e += 256) {
        const int i = e % (int)LEAF, k = e / (int)LEAF;
        U[i + k * a.ld] = k >= i ? X[k + i * LEAF] : 0.0;         // the tile's lower part: zeros that (b) reads
    }
}

template <int STEP>
__global__ __launch_bounds__(256, 2) void mid_inv_level_kernel(const MidInv a)
{
    __shared__ double smem[2 * tile::BK * (2 * (128 + tile::PAD))];
    const int S = a.S, per = S * S;
    const int p = (int)blockIdx.x / per, rem = (int)blockIdx.x - p * per, ti = rem % S, tj = rem / S;
    const int t1 = 2 * S * p, t2 = t1 + S;            // first tile of block 1 (S tiles, full) and of block 2
    if (t2 + tj >= a.W) return;                       // past the ragged last block (the whole workgroup)
    double *L = a.L + (size_t)blockIdx.y * a.stride, *U = a.U + (size_t)blockIdx.y * a.stride;
    const size_t ld = a.ld, r1 = (size_t)t1 * LEAF, r2 = (size_t)t2 * LEAF, ri = r1 + (size_t)ti * LEAF, cj = r2 + (size_t)tj * LEAF;
    tile::GemmArgs g{};
    g.m = 128; g.n = 128; g.beta = 0.0;
    g.lda = ld; g.ldb = ld; g.ldc = ld;
    if constexpr (STEP == 0) {
        // T(ti, tj) = sum_{k >= 128 ti} U11[ti, k] L21[tj, k]
        g.k = (S - ti) * (int)LEAF; g.alpha = 1.0;
        g.A = U + ri + ri * ld;
        g.B = L + cj + ri * ld;
        g.C = L + ri + cj * ld;
        tile::gemm_body_dma<128, 128, 2>(g, smem, 0, 0);
    } else {
        // U12(ti, tj) = -sum_{k < 128 (tj + 1)} T[ti, k] U22[k, tj]
        g.k = (tj + 1) * (int)LEAF; g.alpha = -1.0; g.transb = 1;
        g.A = L + ri + r2 * ld;
        g.B = U + r2 + cj * ld;
        g.C = U + ri + cj * ld;
        tile::gemm_body<128, 128, true, true>(g, smem, 0, 0);
    }
}

__global__ __launch_bounds__(256, 2) void mid_kinv_kernel(const MidInv a)
{
    __shared__ double smem[2 * tile::BK * (2 * (128 + tile::PAD))];
    int t = (int)blockIdx.x, r = 0;            // lower tiles row by row, as mid_syrk_kernel
    while (t > r) { t -= r + 1; ++r; }
    const double *U = a.U + (size_t)blockIdx.y * a.stride;
    const size_t ld = a.ld, ri = (size_t)r * LEAF, cj = (size_t)t * LEAF;
    tile::GemmArgs g{};
    g.m = 128; g.n = 128; g.k = (a.W - r) * (int)LEAF;
    g.alpha = 1.0; g.beta = 0.0;
    g.A = U + ri + ri * ld; g.lda = ld;        // U[I, k] = 0 for k < 128 I
    g.B = U + cj + ri * ld; g.ldb = ld;
    g.C = a.L + (size_t)blockIdx.y * a.stride + ri + cj * ld; g.ldc = ld;
    tile::gemm_body_dma<128, 128, 2>(g, smem, 0, 0);
}

struct MidGrad {
    int npts, n, reg, nwg, nacc;
    size_t ld;                            // npad: Ky^-1 (lower) of problem b at K + b ld^2, its alpha at alpha + b ld
    const double *x, *y;
    const KConst *kc;
    const double *K, *alpha;
    double *part;                         // sum k of workgroup w of problem b at part[(b nwg + w) GPART + k]
    const int *info;
    double *out;                          // problem b's raw sums at out + b nacc
};

// rows i0 .. i0 + GT (one per thread) x column points p0 .. p0 + GCJ of problem blockIdx.z: entries on and below the diagonal,
// weighted W_ii and 2 W_ij, as grad_problem's step (3); rows and columns below n only
template <int FAM>
__global__ __launch_bounds__(GT) void mid_grad_kernel(const MidGrad a)
{
    constexpr bool HASP = grad_has_p<FAM>();
    constexpr int NACC = grad_nacc<FAM>();
    __shared__ double sx[GCJ], sy[GCJ], sal[2][GCJ];
    __shared__ double red[GT / 64][NACC];
    const int b = blockIdx.z, N = a.npts, n = a.n, tid = threadIdx.x;
    const int p0 = blockIdx.y * GCJ, np = min(GCJ, N - p0);
    const int i = blockIdx.x * GT + tid;
    const double *K = a.K + (size_t)b * a.ld * a.ld, *al = a.alpha + (size_t)b * a.ld;
    if (tid < np) {
        sx[tid] = a.x[(size_t)b * N + p0 + tid];
        sy[tid] = a.y[(size_t)b * N + p0 + tid];
        sal[0][tid] = al[p0 + tid];
        sal[1][tid] = a.reg ? 0.0 : al[N + p0 + tid];
    }
    __syncthreads();
    const KConst kc = a.kc[b];
    const double l[2] = {kc.lx, kc.ly}, pp[1] = {kc.p};
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    if (i < n && p0 <= i) {
        const double ai = al[i];
        const double *Krow = K + i;
        if (a.reg) {
            const double xi = a.x[(size_t)b * N + i], yi = a.y[(size_t)b * N + i];
            for (int jj = 0; jj < np; ++jj) {
                const int j = p0 + jj;
                if (j > i) break;
                const double W = Krow[(size_t)j * a.ld] - ai * sal[0][jj];
                if (j == i) acc[NACC - 1] += W;
                nllg::reg_grad<FAM, HASP>(sx[jj], sy[jj], xi, yi, j == i ? W : 2.0 * W, l, kc.p, acc);
            }
        } else {
            const int r = i < N ? 0 : 1, pi = i - r * N;
            const double xi[2] = {a.x[(size_t)b * N + pi], a.y[(size_t)b * N + pi]};
            for (int jj = 0; jj < np; ++jj) {
                const int pj = p0 + jj;
                double w[2];
                bool any = false;
#pragma unroll
                for (int c = 0; c < 2; ++c) {                 // columns pj (q part) and N + pj (P part)
                    const int col = c * N + pj;
                    w[c] = 0.0;
                    if (col <= i) {
                        const double W = Krow[(size_t)col * a.ld] - ai * sal[c][jj];
                        if (col == i) { w[c] = W; acc[NACC - 1] += W; }
                        else w[c] = 2.0 * W;
                        any = true;
                    }
                }
                if (!any) break;                              // column pj > i: so are all after it
                const double xj[2] = {sx[jj], sy[jj]};
                nllg::pair_grad<FAM, 2, HASP>(xi, xj, w, r, l, pp, acc);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        const double v = wave_sum(acc[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < NACC) {
        double v = red[0][tid];
#pragma unroll
        for (int w = 1; w < GT / 64; ++w) v += red[w][tid];
        a.part[((size_t)b * a.nwg + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * GPART + tid] = v;
    }
}

// problem blockIdx.x: its workgroups' partials in their fixed order; NaN where the factorisation failed
__global__ __launch_bounds__(64) void mid_grad_fold_kernel(const MidGrad a)
{
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= a.nacc) return;
    const double *p = a.part + (size_t)b * a.nwg * GPART + k;
    double v = 0.0;
    for (int w = 0; w < a.nwg; ++w) v += p[(size_t)w * GPART];
    a.out[(size_t)b * a.nacc + k] = a.info[b] != 0 ? __builtin_nan("") : v;
}

// ---- leave-one-point-out sums of the mid-size problems (sgpr_fit_batch_loo): behind step (b) above, in place of (c) ----------
struct MidLoo {
    int npts, reg, nwg;
    size_t ld;                            // npad: Ky^-1 (lower) of problem b at K + b ld^2, its alpha at alpha + b ld
    const double *K, *alpha;
    double *part;                         // sum k of workgroup w of problem b at part[(b nwg + w) 2 + k]: k = 0 lpd, 1 |r|^2
    const int *info;
    double *out;                          // problem b's {loo, press} at out + 2 b
};

// points blockIdx.x GT .. + GT (one per thread) of problem blockIdx.z: the point's block from the lower triangle of Ky^-1
__global__ __launch_bounds__(GT) void mid_loo_kernel(const MidLoo a)
{
    __shared__ double red[GT / 64][2];
    const int b = blockIdx.z, N = a.npts, tid = threadIdx.x, i = blockIdx.x * GT + tid;
    const double *K = a.K + (size_t)b * a.ld * a.ld, *al = a.alpha + (size_t)b * a.ld;
    double lv[2] = {0.0, 0.0};
    if (i < N) {
        double lpd, rr;
        if (a.reg) {
            const double C[1] = {K[i + i * a.ld]}, ai[1] = {al[i]};
            double r[1], S[1];
            loo::block<1>(C, ai, r, S, lpd);
            rr = r[0] * r[0];
        } else {
            const double C[3] = {K[i + i * a.ld], K[(N + i) + i * a.ld], K[(N + i) + (N + i) * a.ld]}, ai[2] = {al[i], al[N + i]};
            double r[2], S[3];
            loo::block<2>(C, ai, r, S, lpd);
            rr = __builtin_fma(r[1], r[1], r[0] * r[0]);
        }
        lv[0] = lpd; lv[1] = rr;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double v = wave_sum(lv[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < 2) {
        double v = red[0][tid];
#pragma unroll
        for (int w = 1; w < GT / 64; ++w) v += red[w][tid];
        a.part[((size_t)b * a.nwg + blockIdx.x) * 2 + tid] = v;
    }
}

// problem blockIdx.x: its workgroups' partials in their fixed order; NaN where the factorisation failed
__global__ __launch_bounds__(64) void mid_loo_fold_kernel(const MidLoo a)
{
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= 2) return;
    const double *p = a.part + (size_t)b * a.nwg * 2 + k;
    double v = 0.0;
    for (int w = 0; w < a.nwg; ++w) v += p[(size_t)w * 2];
    a.out[(size_t)b * 2 + k] = a.info[b] != 0 ? __builtin_nan("") : (k == 0 ? -v : v);
}

// Device + pinned-host staging of one calling thread, grown on demand and kept: a call is then one H2D copy,
// one launch and one D2H copy (nine hipMalloc / hipFree pairs and eight small pageable copies per call were
// most of a single small fit's 230 us through a handle).
struct Arena {
    char *dev = nullptr, *host = nullptr;
    size_t cap_dev = 0, cap_host = 0;
    int device = -1;
    // no destructor: at thread / process exit the HIP runtime may already be gone; the OS reclaims
    void release()
    {
        if (dev) (void)hipFree(dev);
        if (host) (void)hipHostFree(host);
        dev = host = nullptr;
        cap_dev = cap_host = 0;
    }
    int reserve(size_t need_dev, size_t need_host)
    {
        int cur = 0;
        SGPR_HIP(hipGetDevice(&cur));
        if (cur != device) { release(); device = cur; }
        // grown for a large batch once, asked for a small one now: give the difference back (a CMA-ES population at order 2048
        // must not keep gigabytes pinned under the full-size fit that follows it)
        if (cap_dev > (256ull << 20) && need_dev * 4 < cap_dev) { if (dev) (void)hipFree(dev); dev = nullptr; cap_dev = 0; }
        if (need_dev > cap_dev) {
            if (dev) (void)hipFree(dev);
            dev = nullptr; cap_dev = 0;
            SGPR_HIP(hipMalloc((void **)&dev, need_dev));
            cap_dev = need_dev;
        }
        if (need_host > cap_host) {
            if (host) (void)hipHostFree(host);
            host = nullptr; cap_host = 0;
            SGPR_HIP(hipHostMalloc((void **)&host, need_host, hipHostMallocDefault));
            cap_host = need_host;
        }
        return 0;
    }
};
thread_local Arena t_arena;

inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace

int fit_batch_max_order() { return potrf_batch_max_order(); }
int fit_batch_trim() { t_arena.release(); return 0; }     // the calling thread's device arena and pinned staging block

namespace {

// the contraction launch of a chunk (step (c) of the gradient phase)
template <int FAM>
void launch_mid_grad(const MidGrad &g, dim3 grid, hipStream_t st) { hipLaunchKernelGGL(mid_grad_kernel<FAM>, grid, dim3(GT), 0, st, g); }

// problems of order 256 < n <= 2048: see the kernels above.  Chunks of problems share the scratch images.
// grad (nbatch x (nhyp + 1)) non-null: sgpr_fit_batch_grad_mid -- a second image per problem (U = L^-T), both images cleared
// on entry, and the gradient phase behind the solves of every chunk; its raw sums come back behind nll in the chunk's one
// device-to-host copy and are scaled here as fit_batch_small scales the one-launch gradient's.
// loo (nbatch x 2) non-null: sgpr_fit_batch_loo -- the same images, clear, chunks and steps (a), (b); then mid_loo_kernel and its
// fold in place of the contraction, {loo, press} behind nll in the same copy.
int fit_batch_mid(int family, int nbatch, int npts, int n, int reg, const double *x, const double *y, const double *z,
                  const double *hyp, int nhyp, const double *sig2n, double *alpha, double *nll, int *info, double *grad = nullptr,
                  double *loo = nullptr, int d = 0, const double *X = nullptr)
{
    const bool kinv = grad || loo;         // the phase behind the solves that forms Ky^-1
    // d > 0: problems with d canonical pairs per point (sgpr_fit_batch_nd) -- X (nbatch x 2d x npts) in place of x | y, one NdConst
    // per problem in place of its KConst, mid_build_nd_kernel in place of mid_build_kernel; no gradient or loo phase
    const size_t D = 2 * (size_t)d;
    const size_t xb = d ? D * npts * 8 : (size_t)npts * 8, yb = d ? 0 : (size_t)npts * 8, kcb = d ? sizeof(nd::NdConst) : sizeof(KConst);
    const int npad = (n + (int)LEAF - 1) / (int)LEAF * (int)LEAF, W = npad / (int)LEAF;
    const size_t img = (size_t)npad * npad * 8, invb = (size_t)W * LEAF * LEAF * 8;
    const size_t nimg = kinv ? 2 : 1, nacc = grad ? (size_t)nhyp + 1 : loo ? 2 : 0;
    // at most ~2 GiB of images per chunk (64 problems of order 2048, 32 with the gradient's second image: 2 x 32 MiB each; round 3:
    // 6 GiB), at least one chip-full of strips (256 workgroups)
    int chunk = (int)std::min<size_t>((size_t)nbatch, std::max<size_t>((256 + W - 1) / W, (2ull << 30) / (nimg * img)));
    if (chunk > 16384) chunk = 16384;      // grid.z of the build launch
    if (kinv) {                            // tunable "batch_gradmid_chunk" > 0 caps it (tests: several chunks of few problems)
        const int cap = (int)tune("batch_gradmid_chunk", 0);
        if (cap > 0 && chunk > cap) chunk = cap;
    }
    const size_t C = (size_t)chunk;
    const int ggx = (n + GT - 1) / GT, ggy = (npts + GCJ - 1) / GCJ, gnwg = ggx * ggy;      // contraction workgroups per problem
    const int lnwg = (npts + GT - 1) / GT;                                                   // loo workgroups per problem
    const size_t o_x = 0, o_y = o_x + up256(C * xb), o_z = o_y + up256(C * yb), o_kc = o_z + up256(C * n * 8),
                 o_no = o_kc + up256(C * kcb), in_bytes = o_no + up256(C * 8);
    // (with the gradient: problem b's raw sums at nll + chunk + b * nacc)
    const size_t o_al = 0, o_nll = o_al + up256(C * n * 8), o_info = o_nll + up256(C * (1 + nacc) * 8),
                 out_bytes = o_info + up256(C * sizeof(int));
    // (+ the solves: right-hand sides / solution padded to npad, the two publication buffers, 8 state words per problem)
    // (with the gradient: the U images directly behind the L images, and the contraction's partials at the end)
    const size_t o_A = 0, o_inv = o_A + nimg * up256(C * img), o_fl = o_inv + up256(C * invb), o_fl2 = o_fl + up256(potrf_batch_flag_bytes(chunk)),
                 o_r = o_fl2 + up256(potrf_batch_flag_bytes(chunk)), o_pub = o_r + up256(C * npad * 8), o_st = o_pub + up256(2 * C * npad * 8),
                 o_part = o_st + up256(C * 8 * sizeof(int)), scr_bytes = o_part + (grad ? up256(C * gnwg * GPART * 8) : loo ? up256(C * lnwg * 2 * 8) : 0);
    Arena &ar = t_arena;
    int rc = ar.reserve(in_bytes + out_bytes + scr_bytes, in_bytes + out_bytes);
    if (rc) return rc;
    char *hin = ar.host, *hout = ar.host + in_bytes;
    char *din = ar.dev, *dout = ar.dev + in_bytes, *dscr = ar.dev + in_bytes + out_bytes;
    hipStream_t st = nullptr;
    for (int b0 = 0; b0 < nbatch; b0 += chunk) {
        const int nb = std::min(chunk, nbatch - b0);
        const size_t B = (size_t)nb;
        if (d) memcpy(hin + o_x, X + (size_t)b0 * D * npts, B * xb);
        else {
            memcpy(hin + o_x, x + (size_t)b0 * npts, B * npts * 8);
            memcpy(hin + o_y, y + (size_t)b0 * npts, B * npts * 8);
        }
        memcpy(hin + o_z, z + (size_t)b0 * n, B * n * 8);
        KConst *kcs = reinterpret_cast<KConst *>(hin + o_kc);
        nd::NdConst *ncs = reinterpret_cast<nd::NdConst *>(hin + o_kc);
        double *noise = reinterpret_cast<double *>(hin + o_no);
        for (int b = 0; b < nb; ++b) {
            if (d) rc = nd::fill_consts(family, d, hyp + (size_t)(b0 + b) * nhyp, nhyp, ncs[b]);
            else rc = make_kconst(family, hyp + (size_t)(b0 + b) * nhyp, nhyp, &kcs[b]);
            if (rc) return rc;
            noise[b] = std::fabs(sig2n[b0 + b]);
        }
        SGPR_HIP(hipMemcpyAsync(din, hin, in_bytes, hipMemcpyHostToDevice, st));
        double *dA = reinterpret_cast<double *>(dscr + o_A), *dinv = reinterpret_cast<double *>(dscr + o_inv);
        int *dinfo = reinterpret_cast<int *>(dout + o_info);
        double *dU = dA + C * (img / 8);
        if (kinv) {
            // both images, unconditionally: the zeros the gradient phase reads above L's diagonal, below U's and in the images of
            // a problem whose factorisation stops early come from here (and the leaf inverses of such a problem are defined)
            SGPR_HIP(hipMemsetAsync(dA, 0, (C + B) * img, st));
            SGPR_HIP(hipMemsetAsync(dinv, 0, B * invb, st));
        } else if (npad != n) SGPR_HIP(hipMemsetAsync(dA, 0, B * img, st));
        MidArgs a{nb, npts, n, npad, reg, reinterpret_cast<double *>(din + o_x), reinterpret_cast<double *>(din + o_y),
                  reinterpret_cast<double *>(din + o_z), reinterpret_cast<KConst *>(din + o_kc),
                  reinterpret_cast<double *>(din + o_no), dA, dinv, alpha ? reinterpret_cast<double *>(dout + o_al) : nullptr,
                  reinterpret_cast<double *>(dout + o_nll), dinfo};
        const dim3 grid((npts + MT - 1) / MT, (npts + MJ - 1) / MJ, nb);
        if (d) {
            const MidNdArgs an{npts, n, npad, reinterpret_cast<double *>(din + o_x), reinterpret_cast<nd::NdConst *>(din + o_kc),
                               reinterpret_cast<double *>(din + o_no), dA};
            if ((rc = nd::dispatch_nd(family, d, [&](auto fam, auto dd) {
                    hipLaunchKernelGGL((mid_build_nd_kernel<decltype(fam)::value, decltype(dd)::value>), grid, dim3(MT), 0, st, an);
                    return 0;
                })))
                return rc;
        } else
        switch (family) {
        case SGPR_FAM_A: hipLaunchKernelGGL(mid_build_kernel<SGPR_FAM_A>, grid, dim3(MT), 0, st, a); break;
        case SGPR_FAM_B: hipLaunchKernelGGL(mid_build_kernel<SGPR_FAM_B>, grid, dim3(MT), 0, st, a); break;
        case SGPR_FAM_C: hipLaunchKernelGGL(mid_build_kernel<SGPR_FAM_C>, grid, dim3(MT), 0, st, a); break;
        case SGPR_FAM_USER: hipLaunchKernelGGL(mid_build_kernel<SGPR_FAM_USER>, grid, dim3(MT), 0, st, a); break;
        default:         hipLaunchKernelGGL(mid_build_kernel<SGPR_FAM_D>, grid, dim3(MT), 0, st, a); break;
        }
        SGPR_CHECK_LAUNCH();
        int *fl = reinterpret_cast<int *>(dscr + o_fl);
        static const int two_min = (int)tune("batch_two_min", 512);
        if (npad <= two_min) {
            if ((rc = potrf_batch(nb, npad, dA, (size_t)npad * npad, (size_t)npad, dinv, (size_t)W * LEAF * LEAF, fl, dinfo, st)))
                return rc;
        } else {
            // two panels above order 512 (SGPR_BATCH_TWO_MIN): in ONE panel the last strip alone has ~W^2 / 2 products of 128^3 to
            // do in a row (n = 2048: 3.0 ms for the launch); as W/2 + W/2 leaf columns (at most 8 first) with the update of the
            // second half on the matrix cores between them it is ~2 ms (per fit at 16 per batch: n = 2048 947 -> 326 us,
            // n = 1024 85 -> 75 us)
            const int W1 = std::min(8, (W + 1) / 2), k1 = W1 * (int)LEAF, m2 = npad - k1;
            SGPR_HIP(hipMemsetAsync(dinfo, 0, B * sizeof(int), st));
            if ((rc = potrf_batch_panel(nb, npad, 0, W1, dA, (size_t)npad * npad, (size_t)npad, dinv, (size_t)W * LEAF * LEAF, fl,
                                        dinfo, st)))
                return rc;
            const int t2 = m2 / (int)LEAF;
            hipLaunchKernelGGL(mid_syrk_kernel, dim3((unsigned)(t2 * (t2 + 1) / 2), (unsigned)nb), dim3(256), 0, st,
                               MidSyrk{dA, (size_t)npad * npad, (size_t)npad, k1, m2});
            SGPR_CHECK_LAUNCH();
            if ((rc = potrf_batch_panel(nb, npad, k1, W - W1, dA, (size_t)npad * npad, (size_t)npad, dinv, (size_t)W * LEAF * LEAF,
                                        reinterpret_cast<int *>(dscr + o_fl2), dinfo, st)))
                return rc;
        }
        // y = L^-1 z, alpha = L^-T y for every problem: the strip solve of trsv.hip, W x nb workgroups per launch
        double *dr = reinterpret_cast<double *>(dscr + o_r), *dpub = reinterpret_cast<double *>(dscr + o_pub);
        int *dst = reinterpret_cast<int *>(dscr + o_st);
        SGPR_HIP(hipMemsetAsync(dst, 0, B * 8 * sizeof(int), st));
        SGPR_HIP(hipMemsetAsync(dpub, 0xFF, 2 * B * npad * 8, st));
        hipLaunchKernelGGL(mid_rhs_kernel, dim3((unsigned)((npad + 255) / 256), (unsigned)nb), dim3(256), 0, st, a, dr);
        SGPR_CHECK_LAUNCH();
        if ((rc = trsv_strips_batch(nb, npad, dA, (size_t)npad * npad, (size_t)npad, dinv, (size_t)W * LEAF * LEAF, dr, (size_t)npad, 0,
                                    dst, 8, dpub, st)))
            return rc;
        if ((rc = trsv_strips_batch(nb, npad, dA, (size_t)npad * npad, (size_t)npad, dinv, (size_t)W * LEAF * LEAF, dr, (size_t)npad, 1,
                                    dst + 4, 8, dpub + B * npad, st)))
            return rc;
        hipLaunchKernelGGL(mid_finish_kernel, dim3(nb), dim3(ST), 0, st, a, (const double *)dr, (const int *)dst, dinfo);
        SGPR_CHECK_LAUNCH();
        if (kinv) {
            // (a) U = L^-T: the diagonal tiles, then two launches per doubling of the block size
            MidInv mi{dA, dU, dinv, (size_t)npad * npad, (size_t)npad, (size_t)W * LEAF * LEAF, W, 1};
            hipLaunchKernelGGL(mid_udiag_kernel, dim3((unsigned)W, (unsigned)nb), dim3(256), 0, st, mi);
            SGPR_CHECK_LAUNCH();
            for (int S = 1; S < W; S *= 2) {
                mi.S = S;
                const dim3 gl((unsigned)((W - S + 2 * S - 1) / (2 * S) * S * S), (unsigned)nb);
                hipLaunchKernelGGL(mid_inv_level_kernel<0>, gl, dim3(256), 0, st, mi);
                SGPR_CHECK_LAUNCH();
                hipLaunchKernelGGL(mid_inv_level_kernel<1>, gl, dim3(256), 0, st, mi);
                SGPR_CHECK_LAUNCH();
            }
            // (b) Ky^-1 = U U^T over L
            hipLaunchKernelGGL(mid_kinv_kernel, dim3((unsigned)(W * (W + 1) / 2), (unsigned)nb), dim3(256), 0, st, mi);
            SGPR_CHECK_LAUNCH();
        }
        if (loo) {
            MidLoo ml{npts, reg, lnwg, (size_t)npad, dA, dr, reinterpret_cast<double *>(dscr + o_part), dinfo,
                      reinterpret_cast<double *>(dout + o_nll) + C};
            hipLaunchKernelGGL(mid_loo_kernel, dim3((unsigned)lnwg, 1, (unsigned)nb), dim3(GT), 0, st, ml);
            SGPR_CHECK_LAUNCH();
            hipLaunchKernelGGL(mid_loo_fold_kernel, dim3(nb), dim3(64), 0, st, ml);
            SGPR_CHECK_LAUNCH();
        }
        if (grad) {
            // (c) the contraction and its fold
            MidGrad mg{npts, n, reg, gnwg, (int)nacc, (size_t)npad, a.x, a.y, a.kc, dA, dr,
                       reinterpret_cast<double *>(dscr + o_part), dinfo, reinterpret_cast<double *>(dout + o_nll) + C};
            const dim3 gg((unsigned)ggx, (unsigned)ggy, (unsigned)nb);
            switch (family) {
            case SGPR_FAM_A: launch_mid_grad<SGPR_FAM_A>(mg, gg, st); break;
            case SGPR_FAM_B: launch_mid_grad<SGPR_FAM_B>(mg, gg, st); break;
            case SGPR_FAM_C: launch_mid_grad<SGPR_FAM_C>(mg, gg, st); break;
            case SGPR_FAM_USER: launch_mid_grad<SGPR_FAM_USER>(mg, gg, st); break;
            default:         launch_mid_grad<SGPR_FAM_D>(mg, gg, st); break;
            }
            SGPR_CHECK_LAUNCH();
            hipLaunchKernelGGL(mid_grad_fold_kernel, dim3(nb), dim3(64), 0, st, mg);
            SGPR_CHECK_LAUNCH();
        }
        const size_t from = alpha ? 0 : o_nll;
        SGPR_HIP(hipMemcpyAsync(hout + from, dout + from, out_bytes - from, hipMemcpyDeviceToHost, st));
        SGPR_HIP(hipStreamSynchronize(st));
        if (alpha) memcpy(alpha + (size_t)b0 * n, hout + o_al, B * n * 8);
        memcpy(nll + b0, hout + o_nll, B * 8);
        memcpy(info + b0, hout + o_info, B * sizeof(int));
        for (int b = 0; b < nb; ++b)
            if (info[b0 + b] < 0) return info_status(info[b0 + b]);     // a hand-off timed out: an error of the call
        if (grad) {
            const double *raw = reinterpret_cast<const double *>(hout + o_nll) + C;
            for (size_t b = 0; b < B; ++b) {
                const double *r = raw + b * nacc;
                double *g = grad + ((size_t)b0 + b) * nacc;
                if (info[b0 + b] != 0) {
                    nll[b0 + b] = std::nan("");
                    for (size_t k = 0; k < nacc; ++k) g[k] = std::nan("");
                    continue;
                }
                const double sig = kcs[b].sig;
                for (int k = 0; k < nhyp - 1; ++k) g[k] = 0.5 * sig * r[k];
                g[nhyp - 1] = 0.5 * r[nhyp - 1];
                g[nhyp] = (sig2n[b0 + b] < 0.0 ? -0.5 : 0.5) * r[nhyp];
            }
        }
        if (loo) {
            const double *raw = reinterpret_cast<const double *>(hout + o_nll) + C;
            for (size_t b = 0; b < B; ++b) {
                const bool bad = info[b0 + b] != 0;
                if (bad) nll[b0 + b] = std::nan("");
                for (int k = 0; k < 2; ++k) loo[((size_t)b0 + b) * 2 + k] = bad ? std::nan("") : raw[b * 2 + k];
            }
        }
    }
    return 0;
}

}  // namespace

namespace {

// problems of order n <= BMAX: one launch of fit_batch_kernel, one workgroup per problem.  grad (nbatch x (nhyp + 1)) non-null:
// the gradient kernel, whose raw sums come back behind nll in the same device-to-host copy and are scaled here.  loo (nbatch x 2)
// non-null: the loo kernel, whose {loo, press} come back the same way.  value (nbatch) non-null beside grad: the loo gradient
// kernel for the objective `which` -- {loo, press, raw sums} per problem, a third BMAX^2 block of scratch per workgroup.
int fit_batch_small(int family, int nbatch, int npts, int n, int reg, const double *x, const double *y, const double *z,
                    const double *hyp, int nhyp, const double *sig2n, double *alpha, double *nll, int *info, double *grad,
                    double *loo = nullptr, double *value = nullptr, int which = SGPR_LOO_LPD)
{
    const size_t B = (size_t)nbatch;
    const int grid = nbatch < 1024 ? nbatch : 1024;
    const size_t per_wg = PER_WG + (grad || loo ? (size_t)BMAX * BMAX : 0) + (value ? (size_t)BMAX * BMAX : 0);
    const size_t ngrad = (size_t)nhyp + 1, nacc = grad ? ngrad + (value ? 2 : 0) : loo ? 2 : 0;     // doubles behind nll per problem
    // input block (one H2D): x | y | z | KConst | noise ; output block (one D2H): alpha | nll [| raw gradient sums] | info
    const size_t o_x = 0, o_y = o_x + up256(B * npts * 8), o_z = o_y + up256(B * npts * 8), o_kc = o_z + up256(B * n * 8),
                 o_no = o_kc + up256(B * sizeof(KConst)), in_bytes = o_no + up256(B * 8);
    const size_t o_al = 0, o_nll = o_al + up256(B * n * 8), o_info = o_nll + up256(B * (1 + nacc) * 8),
                 out_bytes = o_info + up256(B * sizeof(int));
    const size_t scr_bytes = (size_t)grid * per_wg * 8;
    Arena &ar = t_arena;
    int rc = ar.reserve(in_bytes + out_bytes + scr_bytes, in_bytes + out_bytes);
    if (rc) return rc;
    char *hin = ar.host, *hout = ar.host + in_bytes;
    char *din = ar.dev, *dout = ar.dev + in_bytes, *dscr = ar.dev + in_bytes + out_bytes;
    memcpy(hin + o_x, x, B * npts * 8);
    memcpy(hin + o_y, y, B * npts * 8);
    memcpy(hin + o_z, z, B * n * 8);
    KConst *kcs = reinterpret_cast<KConst *>(hin + o_kc);
    double *noise = reinterpret_cast<double *>(hin + o_no);
    for (int b = 0; b < nbatch; ++b) {
        if ((rc = make_kconst(family, hyp + (size_t)b * nhyp, nhyp, &kcs[b]))) return rc;
        noise[b] = std::fabs(sig2n[b]);
    }
    hipStream_t st = nullptr;
    SGPR_HIP(hipMemcpyAsync(din, hin, in_bytes, hipMemcpyHostToDevice, st));
    SGPR_HIP(hipMemsetAsync(dout + o_info, 0, B * sizeof(int), st));
    BatchArgs a{nbatch, npts, n, reg, reinterpret_cast<double *>(din + o_x), reinterpret_cast<double *>(din + o_y),
                reinterpret_cast<double *>(din + o_z), reinterpret_cast<KConst *>(din + o_kc),
                reinterpret_cast<double *>(din + o_no), reinterpret_cast<double *>(dscr),
                reinterpret_cast<double *>(dout + o_al), reinterpret_cast<double *>(dout + o_nll),
                reinterpret_cast<int *>(dout + o_info), which};
    const dim3 g(grid), t(LT);
    if (value) {
        switch (family) {
        case SGPR_FAM_A: hipLaunchKernelGGL((fit_batch_kernel<SGPR_FAM_A, MODE_LOOGRAD>), g, t, 0, st, a); break;
        case SGPR_FAM_B: hipLaunchKernelGGL((fit_batch_kernel<SGPR_FAM_B, MODE_LOOGRAD>), g, t, 0, st, a); break;
        case SGPR_FAM_C: hipLaunchKernelGGL((fit_batch_kernel<SGPR_FAM_C, MODE_LOOGRAD>), g, t, 0, st, a); break;
        case SGPR_FAM_USER: hipLaunchKernelGGL((fit_batch_kernel<SGPR_FAM_USER, MODE_LOOGRAD>), g, t, 0, st, a); break;
        default:         hipLaunchKernelGGL((fit_batch_kernel<SGPR_FAM_D, MODE_LOOGRAD>), g, t, 0, st, a); break;
        }
    } else if (grad) {
        switch (family) {
        case SGPR_FAM_A: hipLaunchKernelGGL((fit_batch_kernel<SGPR_FAM_A, MODE_GRAD>), g, t, 0, st, a); break;
        case SGPR_FAM_B: hipLaunchKernelGGL((fit_batch_kernel<SGPR_FAM_B, MODE_GRAD>), g, t, 0, st, a); break;
        case SGPR_FAM_C: hipLaunchKernelGGL((fit_batch_kernel<SGPR_FAM_C, MODE_GRAD>), g, t, 0, st, a); break;
        case SGPR_FAM_USER: hipLaunchKernelGGL((fit_batch_kernel<SGPR_FAM_USER, MODE_GRAD>), g, t, 0, st, a); break;
        default:         hipLaunchKernelGGL((fit_batch_kernel<SGPR_FAM_D, MODE_GRAD>), g, t, 0, st, a); break;
        }
    } else if (loo) {
        switch (family) {
        case SGPR_FAM_A: hipLaunchKernelGGL((fit_batch_kernel<SGPR_FAM_A, MODE_LOO>), g, t, 0, st, a); break;
        case SGPR_FAM_B: hipLaunchKernelGGL((fit_batch_kernel<SGPR_FAM_B, MODE_LOO>), g, t, 0, st, a); break;
        case SGPR_FAM_C: hipLaunchKernelGGL((fit_batch_kernel<SGPR_FAM_C, MODE_LOO>), g, t, 0, st, a); break;
        case SGPR_FAM_USER: hipLaunchKernelGGL((fit_batch_kernel<SGPR_FAM_USER, MODE_LOO>), g, t, 0, st, a); break;
        default:         hipLaunchKernelGGL((fit_batch_kernel<SGPR_FAM_D, MODE_LOO>), g, t, 0, st, a); break;
        }
    } else {
        switch (family) {
        case SGPR_FAM_A: hipLaunchKernelGGL(fit_batch_kernel<SGPR_FAM_A>, g, t, 0, st, a); break;
        case SGPR_FAM_B: hipLaunchKernelGGL(fit_batch_kernel<SGPR_FAM_B>, g, t, 0, st, a); break;
        case SGPR_FAM_C: hipLaunchKernelGGL(fit_batch_kernel<SGPR_FAM_C>, g, t, 0, st, a); break;
        case SGPR_FAM_USER: hipLaunchKernelGGL(fit_batch_kernel<SGPR_FAM_USER>, g, t, 0, st, a); break;
        default:         hipLaunchKernelGGL(fit_batch_kernel<SGPR_FAM_D>, g, t, 0, st, a); break;
        }
    }
    SGPR_CHECK_LAUNCH();
    // without alpha only the tail of the output block comes back
    const size_t from = alpha ? 0 : o_nll;
    SGPR_HIP(hipMemcpyAsync(hout + from, dout + from, out_bytes - from, hipMemcpyDeviceToHost, st));
    SGPR_HIP(hipStreamSynchronize(st));
    if (alpha) memcpy(alpha, hout + o_al, B * n * 8);
    memcpy(nll, hout + o_nll, B * 8);
    memcpy(info, hout + o_info, B * sizeof(int));
    if (grad) {
        const double *raw = reinterpret_cast<const double *>(hout + o_nll) + B;
        for (size_t b = 0; b < B; ++b) {
            const double *r = raw + b * nacc + (value ? 2 : 0);
            double *g = grad + b * ngrad;
            if (info[b] != 0) {
                nll[b] = std::nan("");
                if (value) value[b] = std::nan("");
                for (size_t k = 0; k < ngrad; ++k) g[k] = std::nan("");
                continue;
            }
            const double sig = kcs[b].sig;
            for (int k = 0; k < nhyp - 1; ++k) g[k] = 0.5 * sig * r[k];
            g[nhyp - 1] = 0.5 * r[nhyp - 1];
            g[nhyp] = (sig2n[b] < 0.0 ? -0.5 : 0.5) * r[nhyp];
            if (value) value[b] = raw[b * nacc + (which == SGPR_LOO_PRESS ? 1 : 0)];
        }
    }
    if (loo) {
        const double *raw = reinterpret_cast<const double *>(hout + o_nll) + B;
        for (size_t b = 0; b < B; ++b) {
            const bool bad = info[b] != 0;
            if (bad) nll[b] = std::nan("");
            for (int k = 0; k < 2; ++k) loo[b * 2 + k] = bad ? std::nan("") : raw[b * 2 + k];
        }
    }
    return 0;
}

}  // namespace

// host buffers in, host buffers out; see include/sympgpr_hip.h (sgpr_fit_batch)
int fit_batch(int family, int nbatch, int npts, const double *x, const double *y, const double *z, const double *hyp,
              int nhyp, const double *sig2n, unsigned flags, double *alpha, double *nll, int *info)
{
    const int reg = (flags & SGPR_FIT_REG) ? 1 : 0;
    const int n = reg ? npts : 2 * npts;
    if (nbatch < 0 || npts <= 0 || n > potrf_batch_max_order() || !x || !y || !z || !hyp || !sig2n || !nll || !info ||
        (flags & ~(unsigned)SGPR_FIT_REG)) {
        set_error("fit_batch: bad arguments (order per problem at most 2048)");
        return SGPR_E_ARG;
    }
    if (nbatch == 0) return 0;
    if (family < SGPR_FAM_A || family > SGPR_FAM_USER) { set_error("fit_batch: unknown kernel family"); return SGPR_E_ARG; }
    if (n > BMAX) return fit_batch_mid(family, nbatch, npts, n, reg, x, y, z, hyp, nhyp, sig2n, alpha, nll, info);
    return fit_batch_small(family, nbatch, npts, n, reg, x, y, z, hyp, nhyp, sig2n, alpha, nll, info, nullptr);
}

namespace {

// sgpr_fit_batch_nd, orders n = 2 d npts <= BMAX: one launch of fit_batch_nd_kernel, one workgroup per problem; the staging of
// fit_batch_small with X in place of x | y and one NdConst per problem
int fit_batch_nd_small(int family, int d, int nbatch, int npts, int n, const double *X, const double *z, const double *hyp, int nhyp,
                       const double *sig2n, double *alpha, double *nll, int *info)
{
    const size_t B = (size_t)nbatch;
    const int grid = nbatch < 1024 ? nbatch : 1024;
    // input block (one H2D): X | z | NdConst | noise ; output block (one D2H): alpha | nll | info
    const size_t o_x = 0, o_z = o_x + up256(B * n * 8), o_nc = o_z + up256(B * n * 8), o_no = o_nc + up256(B * sizeof(nd::NdConst)),
                 in_bytes = o_no + up256(B * 8);
    const size_t o_al = 0, o_nll = o_al + up256(B * n * 8), o_info = o_nll + up256(B * 8), out_bytes = o_info + up256(B * sizeof(int));
    const size_t scr_bytes = (size_t)grid * PER_WG * 8;
    Arena &ar = t_arena;
    int rc = ar.reserve(in_bytes + out_bytes + scr_bytes, in_bytes + out_bytes);
    if (rc) return rc;
    char *hin = ar.host, *hout = ar.host + in_bytes;
    char *din = ar.dev, *dout = ar.dev + in_bytes, *dscr = ar.dev + in_bytes + out_bytes;
    memcpy(hin + o_x, X, B * n * 8);           // 2 d npts = n doubles per problem
    memcpy(hin + o_z, z, B * n * 8);
    nd::NdConst *ncs = reinterpret_cast<nd::NdConst *>(hin + o_nc);
    double *noise = reinterpret_cast<double *>(hin + o_no);
    for (int b = 0; b < nbatch; ++b) {
        if ((rc = nd::fill_consts(family, d, hyp + (size_t)b * nhyp, nhyp, ncs[b]))) return rc;
        noise[b] = std::fabs(sig2n[b]);
    }
    hipStream_t st = nullptr;
    SGPR_HIP(hipMemcpyAsync(din, hin, in_bytes, hipMemcpyHostToDevice, st));
    SGPR_HIP(hipMemsetAsync(dout + o_info, 0, B * sizeof(int), st));
    const BatchNdArgs a{nbatch, npts, n, reinterpret_cast<double *>(din + o_x), reinterpret_cast<double *>(din + o_z),
                        reinterpret_cast<nd::NdConst *>(din + o_nc), reinterpret_cast<double *>(din + o_no),
                        reinterpret_cast<double *>(dscr), alpha ? reinterpret_cast<double *>(dout + o_al) : nullptr,
                        reinterpret_cast<double *>(dout + o_nll), reinterpret_cast<int *>(dout + o_info)};
    if ((rc = nd::dispatch_nd(family, d, [&](auto fam, auto dd) {
            hipLaunchKernelGGL((fit_batch_nd_kernel<decltype(fam)::value, decltype(dd)::value>), dim3(grid), dim3(LT), 0, st, a);
            return 0;
        })))
        return rc;
    SGPR_CHECK_LAUNCH();
    const size_t from = alpha ? 0 : o_nll;     // without alpha only the tail of the output block comes back
    SGPR_HIP(hipMemcpyAsync(hout + from, dout + from, out_bytes - from, hipMemcpyDeviceToHost, st));
    SGPR_HIP(hipStreamSynchronize(st));
    if (alpha) memcpy(alpha, hout + o_al, B * n * 8);
    memcpy(nll, hout + o_nll, B * 8);
    memcpy(info, hout + o_info, B * sizeof(int));
    return 0;
}

}  // namespace

// sgpr_fit_batch_nd: the arguments have been checked (capi.hip), nbatch > 0, n = 2 d npts <= fit_batch_max_order()
int fit_batch_nd(int family, int d, int nbatch, int npts, const double *X, const double *z, const double *hyp, int nhyp,
                 const double *sig2n, double *alpha, double *nll, int *info)
{
    const int n = 2 * d * npts;
    if (n > BMAX)
        return fit_batch_mid(family, nbatch, npts, n, 0, nullptr, nullptr, z, hyp, nhyp, sig2n, alpha, nll, info, nullptr, nullptr, d, X);
    return fit_batch_nd_small(family, d, nbatch, npts, n, X, z, hyp, nhyp, sig2n, alpha, nll, info);
}

int fit_batch_grad_max_order() { return BMAX; }

// sgpr_fit_batch_grad_mid: the arguments have been checked (capi.hip), nbatch > 0, BMAX < n <= fit_batch_max_order()
int fit_batch_grad_mid(int family, int nbatch, int npts, const double *x, const double *y, const double *z, const double *hyp,
                       int nhyp, const double *sig2n, unsigned flags, double *alpha, double *nll, double *grad, int *info)
{
    const int reg = (flags & SGPR_FIT_REG) ? 1 : 0;
    return fit_batch_mid(family, nbatch, npts, reg ? npts : 2 * npts, reg, x, y, z, hyp, nhyp, sig2n, alpha, nll, info, grad);
}

// sgpr_fit_batch_grad: the arguments have been checked (capi.hip), nbatch > 0, n <= BMAX
int fit_batch_grad(int family, int nbatch, int npts, const double *x, const double *y, const double *z, const double *hyp,
                   int nhyp, const double *sig2n, unsigned flags, double *alpha, double *nll, double *grad, int *info)
{
    const int reg = (flags & SGPR_FIT_REG) ? 1 : 0;
    return fit_batch_small(family, nbatch, npts, reg ? npts : 2 * npts, reg, x, y, z, hyp, nhyp, sig2n, alpha, nll, info, grad);
}

// sgpr_fit_batch_loo: the arguments have been checked (capi.hip), nbatch > 0, n <= fit_batch_max_order()
int fit_batch_loo(int family, int nbatch, int npts, const double *x, const double *y, const double *z, const double *hyp,
                  int nhyp, const double *sig2n, unsigned flags, double *alpha, double *nll, double *loo, int *info)
{
    const int reg = (flags & SGPR_FIT_REG) ? 1 : 0, n = reg ? npts : 2 * npts;
    if (n > BMAX) return fit_batch_mid(family, nbatch, npts, n, reg, x, y, z, hyp, nhyp, sig2n, alpha, nll, info, nullptr, loo);
    return fit_batch_small(family, nbatch, npts, n, reg, x, y, z, hyp, nhyp, sig2n, alpha, nll, info, nullptr, loo);
}

// sgpr_fit_batch_loo_grad: the arguments have been checked (capi.hip), nbatch > 0, n <= BMAX
int fit_batch_loo_grad(int family, int nbatch, int npts, const double *x, const double *y, const double *z, const double *hyp,
                       int nhyp, const double *sig2n, unsigned flags, int which, double *alpha, double *nll, double *value,
                       double *grad, int *info)
{
    const int reg = (flags & SGPR_FIT_REG) ? 1 : 0;
    return fit_batch_small(family, nbatch, npts, reg ? npts : 2 * npts, reg, x, y, z, hyp, nhyp, sig2n, alpha, nll, info, grad,
                           nullptr, value, which);
}

}  // namespace sgpr
