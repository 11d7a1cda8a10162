// loograd.hip -- the exact gradient of the leave-one-point-out objectives of a solved fit (sgpr_fit_loo_grad).
// Notation as loo.hip: point i owns the D rows B_i = {c N + i} of Ky, C_i = (Ky^-1)[B_i, B_i], a_i = alpha[B_i], S_i = C_i^-1,
// r_i = S_i a_i, loo = -sum lpd_i, press = sum |r_i|^2.  From d alpha = -Ky^-1 dK alpha and d Ky^-1 = -Ky^-1 dK Ky^-1,
//     d obj / d theta = 1/2 sum_jk (M - beta alpha^T - alpha beta^T)_jk dKy_jk / d theta,   M = Ky^-1 W~ Ky^-1,  beta = Ky^-1 v,
//     loo:    W~[B_i, B_i] = r_i r_i^T + S_i,               v[B_i] = r_i
//     press:  W~[B_i, B_i] = 2 (r_i s_i^T + s_i r_i^T),     v[B_i] = 2 s_i,   s_i = S_i r_i
// with W~ zero outside the N blocks: ONE weight matrix for every hyperparameter, contracted with dKy pair by pair by the
// rank-2 instances of nllgrad.hip's kernels.  On the fit's stream, in this order:
//   1. U = L^-T (trsm_rlt on the identity), Ky^-1 = lower(U U^T) filled up: sgpr_fit_inverse's sequence, n x n each;
//   2. loograd_point_kernel<D>: one thread per point reads its block of Ky^-1, runs loo_block.h, writes W_i, v and the
//      objective's per-workgroup partials (the wave order of loo_point_kernel);
//   3. beta = Ky^-1 v by the one-right-hand-side solve with the cached factor (potrs_vec);
//   4. loograd_apply_kernel<D>: Y[:, B_i] = Ky^-1[:, B_i] W_i into U's block (U is dead): n^2 doubles read, n^2 written;
//   5. per row panel J .. J + nb:  M_p = Y[J:J+nb, :] Ky^-1[:, J:]  (one gemm_nt, nb x (n - J), k = n: Ky^-1 is stored full
//      and symmetric), then the contraction launch on it -- n^3 flop over the panels;
//   6. the folds of nllgrad.hip (fixed order, no atomics: a repeated call gives the same bits).
// Scratch: [Ky^-1 | U / Y | M_p panel | W | v | beta | partials | sums], two n x n blocks beside L.
#include "common.h"
#include "loo_block.h"

namespace sgpr {

namespace {

constexpr int LG_T = 256;      // threads per workgroup of every kernel here
constexpr int LG_PPB = 4;      // points per workgroup of the apply kernel
typedef double double2_t __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(LG_T) void loograd_identity_kernel(int n, double *U)
{
    const int t = blockIdx.x * LG_T + threadIdx.x;
    if (t < n) U[(size_t)t * n + t] = 1.0;
}

struct PointArgs {
    int N, n, press;
    const double *Kinv, *alpha;    // n x n (leading dimension n), n
    double *W, *v;                 // point i's D x D block at W[i D D + e D + c] (symmetric); v in the layout of z
    double *part;                  // the objective's sum of workgroup w at part[w]: sum lpd (loo) or sum |r|^2 (press)
};

template <int D>
__global__ __launch_bounds__(LG_T) void loograd_point_kernel(const PointArgs a)
{
    constexpr int T = D * (D + 1) / 2;
    __shared__ double red[LG_T / 64];
    const int i = blockIdx.x * LG_T + threadIdx.x;
    double obj = 0.0;
    if (i < a.N) {
        double C[T], al[D], r[D], S[T], lpd;
#pragma unroll
        for (int e = 0; e < D; ++e)
#pragma unroll
            for (int c = 0; c <= e; ++c) C[loo::pk(e, c)] = a.Kinv[((size_t)e * a.N + i) + ((size_t)c * a.N + i) * (size_t)a.n];
#pragma unroll
        for (int c = 0; c < D; ++c) al[c] = a.alpha[(size_t)c * a.N + i];
        loo::block<D>(C, al, r, S, lpd);
        double rr = 0.0, s[D];
#pragma unroll
        for (int c = 0; c < D; ++c) rr = __builtin_fma(r[c], r[c], rr);
#pragma unroll
        for (int e = 0; e < D; ++e) {      // s = S r
            double t = 0.0;
#pragma unroll
            for (int c = 0; c < D; ++c) t = __builtin_fma(S[e >= c ? loo::pk(e, c) : loo::pk(c, e)], r[c], t);
            s[e] = t;
        }
        double *Wi = a.W + (size_t)i * D * D;
#pragma unroll
        for (int e = 0; e < D; ++e) {
#pragma unroll
            for (int c = 0; c <= e; ++c) {
                const double w = a.press ? 2.0 * __builtin_fma(r[e], s[c], s[e] * r[c]) : __builtin_fma(r[e], r[c], S[loo::pk(e, c)]);
                Wi[e * D + c] = w;             // both triangles from one value
                Wi[c * D + e] = w;
            }
            a.v[(size_t)e * a.N + i] = a.press ? 2.0 * s[e] : r[e];
        }
        obj = a.press ? rr : lpd;
    }
    for (int o = 32; o > 0; o >>= 1) obj += __shfl_down(obj, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = obj;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = red[0];
#pragma unroll
        for (int w = 1; w < LG_T / 64; ++w) t += red[w];
        a.part[blockIdx.x] = t;
    }
}

// Y[:, c N + i] = sum_e Kinv[:, e N + i] W_i[e][c] for the LG_PPB points of blockIdx.y; a thread owns two consecutive rows
// (one 16-byte access per column where n is even, so that every column starts on a 16-byte boundary), lanes on consecutive
// row pairs: every access is contiguous across the wave.  W_i is the same for the whole workgroup: its address is uniform,
// so it arrives by scalar loads.
template <int D>
__global__ __launch_bounds__(LG_T) void loograd_apply_kernel(int N, int n, const double *__restrict__ Kinv,
                                                             const double *__restrict__ W, double *__restrict__ Y)
{
    const size_t r0 = 2 * ((size_t)blockIdx.x * LG_T + threadIdx.x), ld = (size_t)n;
    if (r0 >= ld) return;
    const bool two = r0 + 1 < ld, vec = !(n & 1);
    const int i0 = blockIdx.y * LG_PPB, i1 = min(i0 + LG_PPB, N);
    for (int i = i0; i < i1; ++i) {
        const double *Wi = W + (size_t)i * D * D;
        double x0[D], x1[D];
#pragma unroll
        for (int e = 0; e < D; ++e) {
            const double *src = Kinv + ((size_t)e * N + i) * ld + r0;
            if (vec) {
                const double2_t t = *reinterpret_cast<const double2_t *>(src);
                x0[e] = t.x; x1[e] = t.y;
            } else {
                x0[e] = src[0];
                x1[e] = two ? src[1] : 0.0;
            }
        }
#pragma unroll
        for (int c = 0; c < D; ++c) {
            double y0 = 0.0, y1 = 0.0;
#pragma unroll
            for (int e = 0; e < D; ++e) {
                const double w = Wi[e * D + c];
                y0 = __builtin_fma(x0[e], w, y0);
                y1 = __builtin_fma(x1[e], w, y1);
            }
            double *dst = Y + ((size_t)c * N + i) * ld + r0;
            if (vec) {
                double2_t t;
                t.x = y0; t.y = y1;
                *reinterpret_cast<double2_t *>(dst) = t;
            } else {
                dst[0] = y0;
                if (two) dst[1] = y1;
            }
        }
    }
}

template <int D>
int launch_points(const PointArgs &a, int nwg, hipStream_t st)
{
    hipLaunchKernelGGL(loograd_point_kernel<D>, dim3(nwg), dim3(LG_T), 0, st, a);
    SGPR_CHECK_LAUNCH();
    return 0;
}

template <int D>
int launch_apply(int N, int n, const double *Kinv, const double *W, double *Y, hipStream_t st)
{
    const dim3 grid(((n + 1) / 2 + LG_T - 1) / LG_T, (N + LG_PPB - 1) / LG_PPB);
    hipLaunchKernelGGL(loograd_apply_kernel<D>, grid, dim3(LG_T), 0, st, N, n, Kinv, W, Y);
    SGPR_CHECK_LAUNCH();
    return 0;
}

}  // namespace

// the panel width is nll_grad_full's rule (tunable "loograd_nb" > 0, a multiple of 128, overrides it: tests and measurement tools)
LooGradLayout loo_grad_layout(int n, int N, int D, int nacc)
{
    const size_t nn = (size_t)n * n, nb = (size_t)kyinv_panel_width(n, "loograd_nb"), ldr = (size_t)n < nb ? (size_t)n : nb;
    const size_t npanels = ((size_t)n + nb - 1) / nb;
    LooGradLayout o;
    o.nb = (int)nb; o.ldr = (int)ldr;
    o.nwg_points = ((size_t)N + LG_T - 1) / LG_T;
    o.nwg = npanels * grad_contract_wgs((int)ldr, N);
    o.kinv = 0;
    o.y = nn;
    o.panel = 2 * nn;
    o.w = o.panel + ldr * (size_t)n;
    o.v = o.w + (size_t)N * D * D;
    o.beta = o.v + (size_t)n;
    o.part = o.beta + (size_t)n;
    o.part_obj = o.part + o.nwg * (size_t)nacc;
    o.sums = o.part_obj + o.nwg_points;
    o.total = o.sums + (size_t)nacc + 1;
    return o;
}

// Leaves the nacc raw sums of nll_grad_full's layout (with W' = M - beta alpha^T - alpha beta^T for its W) at scratch + sums
// and, behind them, the objective's raw sum: sum lpd (which = SGPR_LOO_LPD; loo is its negative) or sum |r|^2 (press).
int fit_loo_grad(int family, int d, bool reg, int which, int N, int n, const double *L, size_t ldl, void *work, const double *X,
                 const double *alpha, const double *l, const double *pp, int nacc, double *scratch, hipStream_t st)
{
    const int D = reg ? 1 : 2 * d;
    if (N <= 0 || d < 1 || d > 3 || (reg && d != 1) || (long)n != (long)D * N || ldl != (size_t)n) { set_error("loo_grad: bad shape"); return SGPR_E_ARG; }
    if (nacc != (reg ? 2 : 2 * d) + (family_has_p(family) ? d : 0) + 2) { set_error("loo_grad: bad component count"); return SGPR_E_ARG; }
    if ((N + LG_PPB - 1) / LG_PPB > 65535) { set_error("loo_grad: too many points for one launch"); return SGPR_E_ARG; }
    const LooGradLayout o = loo_grad_layout(n, N, D, nacc);
    double *Kinv = scratch + o.kinv, *Y = scratch + o.y, *Mp = scratch + o.panel, *W = scratch + o.w;
    double *v = scratch + o.v, *beta = scratch + o.beta, *part = scratch + o.part, *pobj = scratch + o.part_obj;
    const size_t ld = (size_t)n;
    int rc;
    // 1. Ky^-1
    SGPR_HIP(hipMemsetAsync(Y, 0, ld * ld * sizeof(double), st));
    hipLaunchKernelGGL(loograd_identity_kernel, dim3((n + LG_T - 1) / LG_T), dim3(LG_T), 0, st, n, Y);
    SGPR_CHECK_LAUNCH();
    if ((rc = trsm_rlt(n, n, L, ldl, Y, ld, work, st))) return rc;                        // U = L^-T
    if ((rc = gemm_nt(n, n, n, 1.0, Y, ld, Y, ld, 0.0, Kinv, ld, 1, 0, st))) return rc;   // lower(U U^T)
    if ((rc = sym_fill_upper(n, Kinv, ld, st))) return rc;
    // 2. the points
    const PointArgs a{N, n, which == SGPR_LOO_PRESS, Kinv, alpha, W, v, pobj};
    switch (D) {
    case 1: rc = launch_points<1>(a, (int)o.nwg_points, st); break;
    case 2: rc = launch_points<2>(a, (int)o.nwg_points, st); break;
    case 4: rc = launch_points<4>(a, (int)o.nwg_points, st); break;
    default: rc = launch_points<6>(a, (int)o.nwg_points, st); break;
    }
    if (rc) return rc;
    // 3. beta = Ky^-1 v with the cached factor
    SGPR_HIP(hipMemcpyAsync(beta, v, ld * sizeof(double), hipMemcpyDeviceToDevice, st));
    if ((rc = potrs_vec(n, L, ldl, work, beta, st))) return rc;
    // 4. Y = Ky^-1 W~ over U
    switch (D) {
    case 1: rc = launch_apply<1>(N, n, Kinv, W, Y, st); break;
    case 2: rc = launch_apply<2>(N, n, Kinv, W, Y, st); break;
    case 4: rc = launch_apply<4>(N, n, Kinv, W, Y, st); break;
    default: rc = launch_apply<6>(N, n, Kinv, W, Y, st); break;
    }
    if (rc) return rc;
    // 5. the row panels of M and their contraction
    const size_t wgs = grad_contract_wgs(o.ldr, N);
    int p = 0;
    for (int J = 0; J < n; J += o.nb, ++p) {
        const int rows = n - J < o.nb ? n - J : o.nb;
        if ((rc = gemm_nt(rows, n - J, n, 1.0, Y + J, ld, Kinv + J, ld, 0.0, Mp, (size_t)o.ldr, 0, 0, st))) return rc;
        if ((rc = grad_contract_rank2(family, d, reg, N, J, rows, Mp, (size_t)o.ldr, alpha, beta, X, l, pp, part, o.nwg,
                                      (size_t)p * wgs, st)))
            return rc;
    }
    // 6. the folds
    if ((rc = grad_fold(part, o.nwg, nacc, scratch + o.sums, st))) return rc;
    return grad_fold(pobj, o.nwg_points, 1, scratch + o.sums + nacc, st);
}

}  // namespace sgpr
