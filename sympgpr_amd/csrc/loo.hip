// loo.hip -- leave-one-point-out cross-validation of a solved fit (sgpr_fit_loo).
// An observation is a training POINT: point i owns the D rows B_i = {c N + i, c = 0 .. D-1} of Ky (D = 2d for a pair fit,
// 1 for reg), and leaving it out removes them together.  With C_i = (Ky^-1)[B_i, B_i] and a_i = alpha[B_i] (loo_block.h)
//     r_i = C_i^-1 a_i,   S_i = C_i^-1,   lpd_i = -1/2 a_i^T C_i^-1 a_i + 1/2 log det C_i - D/2 log 2 pi,
//     loo = -sum_i lpd_i,   press = sum_i |r_i|^2.
// Ky^-1 is formed by the row panels of nllgrad.hip (kyinv_row_panel: 2 n^3 / 3 flop, one nb x n block of scratch); after
// each panel one launch copies the block entries that panel holds into N packed lower blocks: panel row J + t = c N + i
// holds entry (e, c) of point i at column e N + i - J for every e >= c -- the partner row e N + i >= J + t is never left of
// the panel -- so every entry is read from exactly one panel and written once.  Then one thread per point does the D x D
// algebra in registers; lpd and |r|^2 leave as per-workgroup partials (a fixed wave order) and one workgroup per sum folds
// them in workgroup order.  No atomics: a repeated call gives the same bits.
#include "common.h"
#include "loo_block.h"

namespace sgpr {

namespace {

constexpr int LT_ = 256;       // threads per workgroup of every kernel here

// entry (e = blockIdx.y, c) of the points whose part-c row lies in this panel; lanes on consecutive panel rows t (the panel
// is column-major, its rows contiguous), the column strided by N.  blocks: entry k of point i at blocks[k N + i]
__global__ __launch_bounds__(LT_) void loo_extract_kernel(int N, int J, int rows, const double *R, size_t ldr, double *blocks)
{
    const int t = blockIdx.x * LT_ + threadIdx.x, e = blockIdx.y;
    if (t >= rows) return;
    const long g = (long)J + t;
    const int c = (int)(g / N), i = (int)(g - (long)c * N);
    if (e < c) return;
    blocks[(size_t)loo::pk(e, c) * N + i] = R[(size_t)t + ((size_t)e * N + i - J) * ldr];
}

struct PointArgs {
    int N;
    const double *blocks, *alpha;
    double *resid, *cov, *lpd;     // n (the layout of z), N x D x D, N
    double *part;                  // sum k of workgroup w at part[k gridDim.x + w]: k = 0 lpd, 1 |r|^2
};

template <int D>
__global__ __launch_bounds__(LT_) void loo_point_kernel(const PointArgs a)
{
    constexpr int T = D * (D + 1) / 2;
    __shared__ double red[LT_ / 64][2];
    const int i = blockIdx.x * LT_ + threadIdx.x;
    double acc[2] = {0.0, 0.0};
    if (i < a.N) {
        double C[T], al[D], r[D], S[T], lpd;
#pragma unroll
        for (int k = 0; k < T; ++k) C[k] = a.blocks[(size_t)k * a.N + i];
#pragma unroll
        for (int c = 0; c < D; ++c) al[c] = a.alpha[(size_t)c * a.N + i];
        loo::block<D>(C, al, r, S, lpd);
        double rr = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            a.resid[(size_t)c * a.N + i] = r[c];
            rr = __builtin_fma(r[c], r[c], rr);
        }
#pragma unroll
        for (int e = 0; e < D; ++e)
#pragma unroll
            for (int c = 0; c <= e; ++c) {
                const double v = S[loo::pk(e, c)];       // both triangles from one value
                a.cov[((size_t)i * D + e) * D + c] = v;
                a.cov[((size_t)i * D + c) * D + e] = v;
            }
        a.lpd[i] = lpd;
        acc[0] = lpd;
        acc[1] = rr;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        double s = acc[k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < LT_ / 64; ++w) s += red[w][threadIdx.x];
        a.part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = s;
    }
}

// sum blockIdx.x of the partials, as nllgrad_fold_kernel; out = {loo = -sum lpd, press}
__global__ __launch_bounds__(LT_) void loo_fold_kernel(const double *part, size_t nwg, double *out)
{
    __shared__ double sh[LT_];
    const double *p = part + (size_t)blockIdx.x * nwg;
    double s = 0.0;
    for (size_t w = threadIdx.x; w < nwg; w += LT_) s += p[w];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int h = LT_ / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = blockIdx.x == 0 ? -sh[0] : sh[0];
}

template <int D>
void launch_points(const PointArgs &a, int nwg, hipStream_t st)
{
    hipLaunchKernelGGL(loo_point_kernel<D>, dim3(nwg), dim3(LT_), 0, st, a);
}

}  // namespace

// the panel width is nll_grad_full's rule (tunable "loo_nb" > 0, a multiple of 128, overrides it: tests and measurement tools)
LooLayout loo_layout(int n, int N, int D)
{
    const size_t nb = (size_t)kyinv_panel_width(n, "loo_nb"), ldr = (size_t)n < nb ? (size_t)n : nb;
    const size_t nwg = ((size_t)N + LT_ - 1) / LT_;
    LooLayout o;
    o.panel = 0;
    o.blocks = ldr * (size_t)n;
    o.part = o.blocks + (size_t)N * D * (D + 1) / 2;
    o.resid = o.part + 2 * nwg;
    o.cov = o.resid + (size_t)n;
    o.lpd = o.cov + (size_t)N * D * D;
    o.sums = o.lpd + (size_t)N;
    o.total = o.sums + 2;
    return o;
}

int fit_loo(int D, int N, int n, const double *L, size_t ldl, const void *work, const double *alpha, double *scratch,
            hipStream_t st)
{
    if (N <= 0 || (D != 1 && D != 2 && D != 4 && D != 6) || (long)n != (long)D * N) { set_error("fit_loo: bad shape"); return SGPR_E_ARG; }
    const LooLayout o = loo_layout(n, N, D);
    const int nb = kyinv_panel_width(n, "loo_nb"), ldr = n < nb ? n : nb;
    const int npanels = (n + nb - 1) / nb, nwg = (N + LT_ - 1) / LT_;
    double *R = scratch + o.panel, *blocks = scratch + o.blocks;
    int rc;
    for (int p = 0; p < npanels; ++p) {
        const int J = p * nb, rows = n - J < nb ? n - J : nb;
        if ((rc = kyinv_row_panel(n, J, rows, L, ldl, work, R, (size_t)ldr, st))) return rc;
        hipLaunchKernelGGL(loo_extract_kernel, dim3((rows + LT_ - 1) / LT_, D), dim3(LT_), 0, st, N, J, rows, (const double *)R,
                           (size_t)ldr, blocks);
        SGPR_CHECK_LAUNCH();
    }
    const PointArgs a{N, blocks, alpha, scratch + o.resid, scratch + o.cov, scratch + o.lpd, scratch + o.part};
    switch (D) {
    case 1: launch_points<1>(a, nwg, st); break;
    case 2: launch_points<2>(a, nwg, st); break;
    case 4: launch_points<4>(a, nwg, st); break;
    default: launch_points<6>(a, nwg, st); break;
    }
    SGPR_CHECK_LAUNCH();
    hipLaunchKernelGGL(loo_fold_kernel, dim3(2), dim3(LT_), 0, st, (const double *)(scratch + o.part), (size_t)nwg, scratch + o.sums);
    SGPR_CHECK_LAUNCH();
    return 0;
}

}  // namespace sgpr
