// batch_small.h -- device code of the one-launch batched fits (order n <= 256, one workgroup per problem): the shared fit body,
// the d = 1 and d-pair kernels, the leave-one-point-out sums and the gradient phases (d = 1: grad_problem; d pairs:
// grad_problem_nd).  Included only by batch.hip, behind its other headers (one translation unit).
#pragma once

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
    double *scratch;                      // per workgroup: PER_WG doubles [+ BMAX*BMAX (U = L^-T) for the gradient and loo]
                                          // [+ BMAX*BMAX (W') for the loo gradient], as fit_batch_kernel
    double *alpha, *nll;                  // outputs (alpha may be null); the gradient kernel writes problem b's raw sums at
                                          // nll + nbatch + b * grad_nacc_nd<FAM, D>(), the loo kernel {loo, press} at nll + nbatch + 2 b,
                                          // the loo gradient kernel {loo, press, raw sums} at nll + nbatch + b * (2 + grad_nacc_nd<FAM, D>())
    int *info;                            // per problem, zero on entry
    int which;                            // the loo gradient's objective (SGPR_LOO_LPD / SGPR_LOO_PRESS), the same for the launch
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

template <int FAM, int D, int MODE>
__device__ void grad_problem_nd(const BatchNdArgs &a, int b, const nd::NdConst &nc, double *s, double *A, const double *inv, double *U,
                                const double *al);

// The modes of fit_batch_kernel (grad_problem_nd below).  MODE_GRAD: after the fit, the gradient of problem b's nll; MODE_LOO: its
// leave-one-point-out sums over D x D point blocks; scratch then PER_WG + BMAX^2 doubles per workgroup.  MODE_LOOGRAD: the sums and
// the gradient of one of them, with a third block: PER_WG + 2 BMAX^2 doubles per workgroup, as fit_batch_kernel<FAM, MODE_LOOGRAD>.
template <int FAM, int D, int MODE = MODE_FIT>
__global__ __launch_bounds__(LT) void fit_batch_nd_kernel(const BatchNdArgs a)
{
    static_assert(MODE >= MODE_FIT && MODE <= MODE_LOOGRAD, "fit, nll gradient, loo or loo gradient");
    __shared__ double s[LEAF_LDS];
    __shared__ double red[LT / 64];
    const int tid = threadIdx.x;
    const int n = a.n, N = a.npts;
    const size_t per_wg = PER_WG + (MODE != MODE_FIT ? (size_t)BMAX * BMAX : 0) +
                          (MODE == MODE_LOOGRAD ? (size_t)BMAX * BMAX : 0);                    // PER_WG [+ U] [+ W']
    double *A = a.scratch + (size_t)blockIdx.x * per_wg;      // column-major, ld = BMAX
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
        if constexpr (MODE != MODE_FIT) grad_problem_nd<FAM, D, MODE>(a, b, nc, s, A, inv, v + 2 * BMAX, v + BMAX);
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

// The same for a point with D rows {c N + i} (d-pair fits: D = 2 d; the mid path's d = 1 fits: D = 1 for reg, 2 for pairs): the block's
// entries (e N + i, c N + i), e >= c, from the lower triangle of Ky^-1 (K, leading dimension ld), packed with loo::pk.
template <int D>
__device__ __forceinline__ void loo_point_nd(const double *K, size_t ld, const double *al, int i, int N, double (&r)[D],
                                             double (&S)[D * (D + 1) / 2], double &lpd, double &rr)
{
    double C[D * (D + 1) / 2], ai[D];
#pragma unroll
    for (int e = 0; e < D; ++e) {
#pragma unroll
        for (int c = 0; c <= e; ++c) C[loo::pk(e, c)] = K[((size_t)e * N + i) + ((size_t)c * N + i) * ld];
        ai[e] = al[e * N + i];
    }
    loo::block<D>(C, ai, r, S, lpd);
    rr = r[0] * r[0];
#pragma unroll
    for (int k = 1; k < D; ++k) rr = __builtin_fma(r[k], r[k], rr);
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

// Steps (1) and (2) of grad_problem, for the workgroup that has just fitted a problem of order n (n1 = min(n, LEAF), n2 = n - n1):
// A holds L (ld = BMAX), inv the leaf inverses; U = L^-T goes to U (BMAX^2 doubles), then Ky^-1 = U U^T, lower triangle, over L.
// Neither step needs the points or the kernel's constants: the d = 1 and the d-pair kernels call this one text.  s: LEAF_LDS
// doubles (T = L21 X11).  No barrier behind step (2): thread i has written row i of Ky^-1.
__device__ __forceinline__ void kinv_problem(double *s, double *A, const double *inv, double *U, int n, int n1, int n2)
{
    constexpr size_t ld = BMAX;
    const int tid = threadIdx.x;
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
}

// The gradient of problem b's nll in (lx, ly, [p,] sig, sig2n), by the workgroup that has just fitted it: A holds L, inv the
// leaf inverses X11 = L11^-1 and X22 = L22^-1, al alpha; U is BMAX^2 doubles of the workgroup's scratch.  (1) and (2) are
// kinv_problem above.
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
    kinv_problem(s, A, inv, U, n, n1, n2);                // (1) and (2)
    const int i = tid;
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

// ---- the nll gradient for d canonical pairs per point (D = 2 d): lq_1..lq_d, lP_1..lP_d, [p_1..p_d,] sig, sig2n
template <int FAM, int D> constexpr int grad_nacc_nd() { return D + (grad_has_p<FAM>() ? D / 2 : 0) + 2; }

// Step (3) for D x D blocks of point pairs, for any symmetric weight: thread i < n owns row i of W, given as wf(i, alpha_i, col) for
// col <= i (the nll gradient: Ky^-1 - alpha alpha^T from the lower triangle of Ky^-1; the loo gradient: a load of W'), which is
// part r = i / N of point pi = i % N, and walks the column points pj = 0 .. N - 1.  Each pair is evaluated once
// (nllg::pair_grad, dK from the generated forms) and feeds the D entries (i, c N + pj): W_ii on the diagonal (also the noise sum),
// 2 W_ij below it, 0 above it; the walk stops at the first pj with no entry on or below the diagonal (pj > i).  The points (D N <=
// BMAX doubles, coordinate m of point p at s[m N + p]) and alpha (at s + 2 BMAX) go to LDS first, the wave partials behind them.
// Lengths and periods as nllgrad.hip fills GradArgs::l / pp, from the problem's NdConst.  The per-thread sums fold wave by wave in a
// fixed order into out[0 .. NACC), unscaled.
template <int FAM, int D, class WF>
__device__ __forceinline__ void contract_rows_nd(const double *X, const nd::NdConst &nc, int N, int n, double *s, const double *al,
                                                 double *out, WF wf)
{
    constexpr bool HASP = grad_has_p<FAM>();
    constexpr int NACC = grad_nacc_nd<FAM, D>(), d = D / 2;
    static_assert(3 * BMAX + 4 * NACC <= (int)LEAF_LDS, "points | alpha | wave partials fit in the leaf's LDS");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = tid;
    double *sx = s, *sal = s + 2 * BMAX, *red = s + 3 * BMAX;
    for (int e = tid; e < n; e += LT) { sx[e] = X[e]; sal[e] = al[e]; }      // D N = n
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    double l[D], pp[d];
#pragma unroll
    for (int m = 0; m < D; ++m) l[m] = nc.l[m];
#pragma unroll
    for (int m = 0; m < d; ++m) pp[m] = HASP ? nc.hs[m] : 0.0;
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    if (i < n) {
        const int r = i / N, pi = i - r * N;
        const double ai = sal[i];
        double xi[D];
#pragma unroll
        for (int m = 0; m < D; ++m) xi[m] = sx[m * N + pi];
        for (int pj = 0; pj < N; ++pj) {
            if (pj > i) break;                                // no entry of this column point on or below the diagonal, nor after it
            double w[D], xj[D];
#pragma unroll
            for (int c = 0; c < D; ++c) {                     // column c N + pj: part c of the column point
                const int col = c * N + pj;
                w[c] = 0.0;
                if (col <= i) {
                    const double W = wf(i, ai, col);
                    if (col == i) { w[c] = W; acc[NACC - 1] += W; }
                    else w[c] = 2.0 * W;
                }
            }
#pragma unroll
            for (int m = 0; m < D; ++m) xj[m] = sx[m * N + pj];
            nllg::pair_grad<FAM, D, HASP>(xi, xj, w, r, l, pp, acc);
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

// Step (L3) of the d-pair loo gradient: grad_problem's (L3), statement by statement (neither the points nor the block size enter;
// the d = 1 kernel keeps its inline text, and with it its compiled code): W'[i, j] from M[i, j] = sum_k Ky^-1[i, k] Y[k, j], i >= j,
// with Ky^-1 full in A and Y in Y (ld = BMAX): thread i its row, columns j0 .. j0 + 3 from one pass over the row (a column past
// n - 1 is clamped: computed again, not stored), k = 0 .. n - 1 in order.  Stored in M: W' = M - beta alpha^T - alpha beta^T (al:
// global, sbeta: LDS).  No barrier: thread i reads back its own row.
__device__ __forceinline__ void wprime_rows(const double *A, const double *Y, double *M, const double *al, const double *sbeta, int n)
{
    constexpr size_t ld = BMAX;
    const int i = threadIdx.x;
    for (int j0 = 0; j0 < n; j0 += 4) {
        if (i < n && i >= j0) {
            const double *y0 = Y + j0 * ld, *y1 = Y + min(j0 + 1, n - 1) * ld, *y2 = Y + min(j0 + 2, n - 1) * ld,
                         *y3 = Y + min(j0 + 3, n - 1) * ld;
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
}

// grad_problem for the d-pair kernel: the NaN row of a problem that is not positive definite, kinv_problem (steps (1) and (2), the
// text the d = 1 kernel runs), then by mode
//   MODE_GRAD     contract_rows_nd on Ky^-1 - alpha alpha^T.  The sums leave unscaled: the host applies sig / 2 (sig from the staged
//                 NdConst), 1/2 and sign(sig2n) / 2;
//   MODE_LOO      thread i < N takes point i's D x D block of Ky^-1 (loo_point_nd) through loo_block.h; lpd and |r|^2 fold wave by
//                 wave in the fixed order (loo_fold) into {loo, press};
//   MODE_LOOGRAD  MODE_LOO's steps and sums by the same code (the same bits), then grad_problem's phases (L1) - (L4) over D x D
//                 blocks: (L1) W~_i (packed lower, T = D (D + 1) / 2 doubles per point, entry t of point i at sW[t N + i]: T N =
//                 (D + 1) n / 2 <= 3.5 BMAX doubles at D = 6) and v[B_i] into LDS, with v and beta behind W~, and the mirror of
//                 Ky^-1; (L2) beta = Ky^-1 v and Y = W~ Ky^-1 over U, row c N + i of Y from the point's D rows of Ky^-1; (L3)
//                 wprime_rows into the third block; (L4) contract_rows_nd with a plain load of W'.
// Output: MODE_GRAD the NACC raw sums, MODE_LOO {loo, press}, MODE_LOOGRAD {loo, press, the NACC raw sums}.
template <int FAM, int D, int MODE>
__device__ void grad_problem_nd(const BatchNdArgs &a, int b, const nd::NdConst &nc, double *s, double *A, const double *inv, double *U,
                                const double *al)
{
    constexpr int NACC = grad_nacc_nd<FAM, D>(), NOUT = MODE == MODE_LOO ? 2 : MODE == MODE_LOOGRAD ? 2 + NACC : NACC;
    constexpr int T = D * (D + 1) / 2;
    // LDS: contract_rows_nd's points | alpha | partials in [0, 4 BMAX), then W~ (T N <= (D + 1) BMAX / 2), v, beta
    static_assert((D + 1) * BMAX / 2 <= 4 * BMAX && 10 * BMAX <= (int)LEAF_LDS, "W~, v and beta fit in the leaf's LDS behind the contraction's part");
    constexpr size_t ld = BMAX;
    const int tid = threadIdx.x;
    const int n = a.n, N = a.npts, n1 = min(n, (int)LEAF), n2 = n - n1;
    const double *X = a.X + (size_t)b * D * N;
    double *out = a.nll + a.nbatch + (size_t)b * NOUT;
    if (__hip_atomic_load(a.info + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
        if (tid < NOUT) out[tid] = __builtin_nan("");
        return;
    }
    kinv_problem(s, A, inv, U, n, n1, n2);
    [[maybe_unused]] double *sal = s + 2 * BMAX;          // contract_rows_nd's alpha
    if constexpr (MODE == MODE_GRAD) {
        contract_rows_nd<FAM, D>(X, nc, N, n, s, al, out, [=](int row, double ai, int col) { return A[row + col * ld] - ai * sal[col]; });
        return;
    }
    const int i = tid;
    [[maybe_unused]] double *sW = s + 4 * BMAX, *sv = s + 8 * BMAX, *sbeta = s + 9 * BMAX;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                      // point i's block has entries written by the threads c N + i; T is dead
    double lv[2] = {0.0, 0.0};
    if (i < N) {
        double r[D], S[T], lpd, rr;
        loo_point_nd<D>(A, ld, al, i, N, r, S, lpd, rr);
        lv[0] = lpd; lv[1] = rr;
        if constexpr (MODE == MODE_LOOGRAD) {
            // (L1) W~_i and v[B_i]
            if (a.which == SGPR_LOO_PRESS) {
                double sr[D];                             // s = S r
#pragma unroll
                for (int e = 0; e < D; ++e) {
                    double acc = S[loo::pk(e, 0)] * r[0];
#pragma unroll
                    for (int c = 1; c < D; ++c) acc = __builtin_fma(S[c <= e ? loo::pk(e, c) : loo::pk(c, e)], r[c], acc);
                    sr[e] = acc;
                }
#pragma unroll
                for (int e = 0; e < D; ++e) {
#pragma unroll
                    for (int c = 0; c <= e; ++c) sW[loo::pk(e, c) * N + i] = 2.0 * __builtin_fma(r[e], sr[c], sr[e] * r[c]);
                    sv[e * N + i] = 2.0 * sr[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < D; ++e) {
#pragma unroll
                    for (int c = 0; c <= e; ++c) sW[loo::pk(e, c) * N + i] = __builtin_fma(r[e], r[c], S[loo::pk(e, c)]);
                    sv[e * N + i] = r[e];
                }
            }
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
            // row i = c N + pi of Y from the point's rows e N + pi of Ky^-1, weights W~_pi[c, e]
            const int c = i / N, pi = i - c * N;
            double w[D];
#pragma unroll
            for (int e = 0; e < D; ++e) w[e] = sW[(e >= c ? loo::pk(e, c) : loo::pk(c, e)) * N + pi];
            const double *Ap = A + pi;
            for (int k = 0; k < n; ++k) {
                double y = w[D - 1] * Ap[(size_t)(D - 1) * N + k * ld];
#pragma unroll
                for (int e = D - 2; e >= 0; --e) y = __builtin_fma(w[e], Ap[(size_t)e * N + k * ld], y);
                U[i + k * ld] = y;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // ---- (L3) W' into the third block, (L4) thread i reads the row of W' it wrote
        double *M = U + (size_t)BMAX * BMAX;
        wprime_rows(A, U, M, al, sbeta, n);
        contract_rows_nd<FAM, D>(X, nc, N, n, s, al, out + 2, [=](int row, double, int col) { return M[row + col * ld]; });
    }
}

}  // namespace

}  // namespace sgpr
