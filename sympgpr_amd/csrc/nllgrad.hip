// nllgrad.hip -- the exact NLL gradient of a solved fit in all its hyperparameters (sgpr_fit_nll_grad_full):
//     d nll / d theta = 1/2 sum_ij (Ky^-1 - alpha alpha^T)_ij dKy_ij / d theta.
// Ky^-1 is formed by row panels, never all of it at once: for the panel of rows J .. J + nb,
//     R = [I_nb | 0] (nb x (n - J)),  R := R L_tt^-T,  R := R L_tt^-1,  L_tt = L[J:, J:]
// (the recursive panel solves of solve.hip on the trailing block, with the factor's own leaf inverses), after which
// R = Ky^-1[J:J+nb, J:] -- 2 nb (n - J)^2 flop per panel, 2 n^3 / 3 in all, one nb x n block of scratch.  Then one launch
// contracts the panel with the derivatives of K, evaluated pair by pair in registers, never stored:
//   * every workgroup takes NG_T panel rows (one per thread) x NG_CJ column POINTS; a thread's row i is (part r, point
//     pi), and for each column point pj it evaluates the pair once and visits the D entries (i, c N + pj), c = 0 .. D-1
//     (D = 2d output parts of a pair fit, one for reg).  Entries below the diagonal are skipped, those above it count
//     twice (Ky^-1 and dK are symmetric), the diagonal once -- and also feeds the sig2n component, sum_i W_ii;
//   * pair fits (d = 1 .. 3): the product kernel K_ab = sig k B_ab, k = prod_m f_m, B_ab = (a == b ? -f_a''/f_a :
//     -(f_a'/f_a)(f_b'/f_b)) (gram_nd.hip), so with gen::factor / factor_dl / factor_dp (tools/gen_kernels.py)
//         dK_ab / dl_m = K_ab d(log f_m)/dl_m + sig k dB_ab/dl_m,   the same for a period p_m,   dK / dsig = k B;
//     the sum kernel (family B): K_aa = sig f_a (-f_a''/f_a), other blocks zero;
//   * reg fits: K = sig k(x_j, y_j, x_i, y_i) and its derivatives from gen::pair / pair_dlx / pair_dly / pair_dp.
// The sums are deterministic, with no atomics: per-workgroup partials (a fixed wave order), folded at the end by one
// workgroup per component in a fixed order.  Per panel the contraction costs nb N pair evaluations against
// 2 nb (n - J)^2 flop of the solves: a small part of the whole.
// The same kernels with their last template flag set contract the weight of the LOO gradient (loograd.hip), whose panel
// holds M = Ky^-1 W~ Ky^-1 and whose rank-1 term is the rank-2 beta alpha^T + alpha beta^T: everything after W is shared.
#include <type_traits>

#include "common.h"
#include "generated/pair_generated.h"
#include "nllgrad_pair.h"

namespace sgpr {

namespace {

constexpr int NG_T = 256;      // panel rows per workgroup, one per thread
constexpr int NG_CJ = 64;      // column points per workgroup
constexpr int NG_FOLD = 256;   // threads of a fold workgroup

struct GradArgs {
    int N, J, rows;            // points, first row of the panel, its rows
    size_t ldr;
    const double *R;           // Ky^-1[J:J+rows, J:], leading dimension ldr
    const double *alpha;       // n
    const double *X;           // points (N x 2d, column-major: q_1..q_d, P_1..P_d; (x, y) for reg)
    double l[6], pp[3];        // the lengths, the q factors' periods (unused without one)
    double *part;              // accumulator k of workgroup w at part[k nwg + w]
    size_t nwg, wg0;           // workgroups of all panels, this panel's first
};
struct GradArgs2 : GradArgs {  // the rank-2 weight of the LOO gradient (loograd.hip): R holds a panel of M = Ky^-1 W~ Ky^-1
    const double *beta;        // n
};

using nllg::sum_kernel;

// the workgroup's NACC sums, wave by wave in a fixed order, to its slot of the partials
template <int NACC>
__device__ __forceinline__ void store_partials(const GradArgs &a, double (&acc)[NACC])
{
    __shared__ double red[NG_T / 64][NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        double s = acc[k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < NACC) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < NG_T / 64; ++w) s += red[w][threadIdx.x];
        a.part[(size_t)threadIdx.x * a.nwg + a.wg0 + (size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

// pair fits, D = 2d parts; accumulators: l_0 .. l_{D-1}, [p_0 .. p_{d-1},] sig, noise (sig factor applied by the caller).
// nllgrad_pair.h's pair_grad is this loop body for the batched gradient; it stays inline here (see that header)
// R2: the weight is R - (beta_i alpha_col + alpha_i beta_col) (loograd.hip: R holds a panel of M) instead of R - alpha_i alpha_col
template <int FAM, int D, bool HASP, bool R2 = false>
__global__ __launch_bounds__(NG_T) void nllgrad_pairs_kernel(const std::conditional_t<R2, GradArgs2, GradArgs> a)
{
    constexpr int d = D / 2, NP = HASP ? d : 0, NACC = D + NP + 2;
    __shared__ double sx[NG_CJ][D];
    __shared__ double sal[D][NG_CJ];
    __shared__ double sbe[R2 ? D : 1][R2 ? NG_CJ : 1];
    const int p0 = blockIdx.y * NG_CJ, np = min(NG_CJ, a.N - p0);
    const int li = blockIdx.x * NG_T + threadIdx.x;                  // row inside the panel
    const long i = (long)a.J + li;                                   // row of Ky
    for (int e = threadIdx.x; e < np * D; e += NG_T) {
        const int j = e % np, m = e / np;
        sx[j][m] = a.X[(size_t)(p0 + j) + (size_t)m * a.N];
        sal[m][j] = a.alpha[(size_t)m * a.N + p0 + j];
        if constexpr (R2) sbe[m][j] = a.beta[(size_t)m * a.N + p0 + j];
    }
    __syncthreads();
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    // the last column this chunk reaches is (D - 1) N + p0 + np - 1: rows past it have nothing above the diagonal here
    if (li < a.rows && (long)(D - 1) * a.N + p0 + np - 1 >= i) {
        const int r = (int)(i / a.N), pi = (int)(i - (long)r * a.N);
        double xi[D];
#pragma unroll
        for (int m = 0; m < D; ++m) xi[m] = a.X[(size_t)pi + (size_t)m * a.N];
        const double ai = a.alpha[i];
        double bi = 0.0;
        if constexpr (R2) bi = a.beta[i];
        const double *Rrow = a.R + li;
        for (int jj = 0; jj < np; ++jj) {
            const long pj = p0 + jj;
            double w[D];
            bool any = false;
#pragma unroll
            for (int c = 0; c < D; ++c) {
                const long col = (long)c * a.N + pj;
                w[c] = 0.0;
                if (col >= i) {
                    double W;
                    if constexpr (R2) W = Rrow[(size_t)(col - a.J) * a.ldr] - __builtin_fma(bi, sal[c][jj], ai * sbe[c][jj]);
                    else W = Rrow[(size_t)(col - a.J) * a.ldr] - ai * sal[c][jj];
                    if (col == i) { w[c] = W; acc[NACC - 1] += W; }
                    else w[c] = 2.0 * W;
                    any = true;
                }
            }
            if (!any) continue;
            double arg[D], g[D], nh[D], dar[D], dg[D], dnh[D], par[d], pg[d], pnh[d];
#pragma unroll
            for (int m = 0; m < D; ++m) {
                const double dx = sx[jj][m] - xi[m];   // column point - row point, as gram_nd
                double o[3], od[3];
                if (m < d) {
                    gen::factor<FAM, 1>(dx, a.l[m], a.pp[m], o);
                    gen::factor_dl<FAM, 1>(dx, a.l[m], a.pp[m], od);
                    if constexpr (HASP) {
                        double op[3];
                        gen::factor_dp<FAM, 1>(dx, a.l[m], a.pp[m], op);
                        par[m] = op[0]; pg[m] = op[1]; pnh[m] = op[2];
                    }
                } else {
                    gen::factor<FAM, 0>(dx, a.l[m], 0.0, o);
                    gen::factor_dl<FAM, 0>(dx, a.l[m], 0.0, od);
                }
                arg[m] = o[0]; g[m] = o[1]; nh[m] = o[2];
                dar[m] = od[0]; dg[m] = od[1]; dnh[m] = od[2];
            }
            // this thread's part r: its factor data (r is a runtime value; the unrolled selects keep all in registers)
            double wr = 0.0, gr = 0.0, nhr = 0.0, dgr = 0.0, dnhr = 0.0, darr = 0.0, argr = 0.0, pgr = 0.0, pnhr = 0.0, parr = 0.0;
#pragma unroll
            for (int m = 0; m < D; ++m)
                if (m == r) { wr = w[m]; gr = g[m]; nhr = nh[m]; dgr = dg[m]; dnhr = dnh[m]; darr = dar[m]; argr = arg[m]; }
            if constexpr (HASP) {
#pragma unroll
                for (int m = 0; m < d; ++m)
                    if (m == r) { pgr = pg[m]; pnhr = pnh[m]; parr = par[m]; }
            }
            if constexpr (sum_kernel<FAM>()) {
                // only the diagonal block (r, r): K = sig f_r nh_r
                const double e = wr * exp(argr);
                acc[D + NP] += e * nhr;
#pragma unroll
                for (int m = 0; m < D; ++m)
                    if (m == r) acc[m] += e * __builtin_fma(darr, nhr, dnhr);
                if constexpr (HASP) {
#pragma unroll
                    for (int m = 0; m < d; ++m)
                        if (m == r) acc[D + m] += e * __builtin_fma(parr, nhr, pnhr);
                }
            } else {
                double t = 0.0, S = 0.0;
#pragma unroll
                for (int m = 0; m < D; ++m) { t += arg[m]; S = __builtin_fma(w[m], g[m], S); }
                const double k = exp(t);
                const double So = S - wr * gr;                       // sum over the columns' other parts of w_c g_c
                const double TB = __builtin_fma(wr, nhr, -gr * So);  // sum_c w_c B_rc
                acc[D + NP] += k * TB;
#pragma unroll
                for (int m = 0; m < D; ++m) {
                    const double own = __builtin_fma(wr, dnhr, -dgr * So), other = -w[m] * gr * dg[m];
                    acc[m] += k * __builtin_fma(dar[m], TB, m == r ? own : other);
                }
                if constexpr (HASP) {
#pragma unroll
                    for (int m = 0; m < d; ++m) {
                        const double own = __builtin_fma(wr, pnhr, -pgr * So), other = -w[m] * gr * pg[m];
                        acc[D + m] += k * __builtin_fma(par[m], TB, m == r ? own : other);
                    }
                }
            }
        }
    }
    store_partials<NACC>(a, acc);
}

// reg fits (one part); accumulators: lx, ly, [p,] sig, noise
template <int FAM, bool HASP, bool R2 = false>
__global__ __launch_bounds__(NG_T) void nllgrad_reg_kernel(const std::conditional_t<R2, GradArgs2, GradArgs> a)
{
    constexpr int NACC = HASP ? 5 : 4;
    __shared__ double sx[NG_CJ], sy[NG_CJ], sal[NG_CJ];
    __shared__ double sbe[R2 ? NG_CJ : 1];
    const int p0 = blockIdx.y * NG_CJ, np = min(NG_CJ, a.N - p0);
    const int li = blockIdx.x * NG_T + threadIdx.x;
    const long i = (long)a.J + li;
    for (int j = threadIdx.x; j < np; j += NG_T) {
        sx[j] = a.X[p0 + j];
        sy[j] = a.X[(size_t)a.N + p0 + j];
        sal[j] = a.alpha[p0 + j];
        if constexpr (R2) sbe[j] = a.beta[p0 + j];
    }
    __syncthreads();
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    if (li < a.rows && (long)p0 + np - 1 >= i) {
        const double xi = a.X[i], yi = a.X[(size_t)a.N + i], ai = a.alpha[i];
        double bi = 0.0;
        if constexpr (R2) bi = a.beta[i];
        const double *Rrow = a.R + li;
        for (int jj = 0; jj < np; ++jj) {
            const long col = p0 + jj;
            if (col < i) continue;
            double W;
            if constexpr (R2) W = Rrow[(size_t)(col - a.J) * a.ldr] - __builtin_fma(bi, sal[jj], ai * sbe[jj]);
            else W = Rrow[(size_t)(col - a.J) * a.ldr] - ai * sal[jj];
            const double w = col == i ? W : 2.0 * W;
            if (col == i) acc[NACC - 1] += W;
            nllg::reg_grad<FAM, HASP>(sx[jj], sy[jj], xi, yi, w, a.l, a.pp[0], acc);      // nllgrad_pair.h
        }
    }
    store_partials<NACC>(a, acc);
}

__global__ __launch_bounds__(NG_FOLD) void nllgrad_fold_kernel(const double *part, size_t nwg, double *out)
{
    __shared__ double sh[NG_FOLD];
    const double *p = part + (size_t)blockIdx.x * nwg;
    double s = 0.0;
    for (size_t w = threadIdx.x; w < nwg; w += NG_FOLD) s += p[w];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int h = NG_FOLD / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

__global__ void panel_identity_kernel(int rows, double *R, size_t ldr)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < rows) R[(size_t)t + (size_t)t * ldr] = 1.0;
}

struct Shape { int nb, ldr, npanels, gx, gy; size_t nwg; };

// the panel width is fixed by n (a multiple of the 128 leaf): 2048 rows up to n = 8192, 4096 above.  Each panel solve
// runs one in-place leaf product per 128 columns whose grid is nb / 64 workgroups: latency-bound, so the call time falls
// almost in proportion to the panels (n = 16 384: 237 / 150 / 109 ms at nb = 1024 / 2048 / 4096; d = 3, n = 49 152:
// 2197 / 1741 ms at 2048 / 4096).  (tunable "nllgrad_nb" > 0, a multiple of 128, overrides it: measurement tools only)
Shape shape_of(int n, int N)
{
    Shape s;
    s.nb = kyinv_panel_width(n, "nllgrad_nb");
    s.ldr = n < s.nb ? n : s.nb;
    s.npanels = (n + s.nb - 1) / s.nb;
    s.gx = (s.ldr + NG_T - 1) / NG_T;
    s.gy = (N + NG_CJ - 1) / NG_CJ;
    s.nwg = (size_t)s.npanels * s.gx * s.gy;
    return s;
}

// one contraction launch of the family's instance: with beta, the R2 instances (the rank-2 weight)
int launch_contract(int family, int d, bool reg, const double *beta, dim3 grid, const GradArgs &a, hipStream_t st)
{
    const bool rank2 = beta != nullptr;
    GradArgs2 a2{};
    static_cast<GradArgs &>(a2) = a;
    a2.beta = beta;
    auto launch = [&](auto fam, auto dd, auto hp) {
        constexpr int F = decltype(fam)::value, DD = decltype(dd)::value;
        constexpr bool HP = decltype(hp)::value;
        if constexpr (DD == 0) {
            if (rank2) hipLaunchKernelGGL((nllgrad_reg_kernel<F, HP, true>), grid, dim3(NG_T), 0, st, a2);
            else hipLaunchKernelGGL((nllgrad_reg_kernel<F, HP>), grid, dim3(NG_T), 0, st, a);
        } else {
            if (rank2) hipLaunchKernelGGL((nllgrad_pairs_kernel<F, DD, HP, true>), grid, dim3(NG_T), 0, st, a2);
            else hipLaunchKernelGGL((nllgrad_pairs_kernel<F, DD, HP>), grid, dim3(NG_T), 0, st, a);
        }
        SGPR_CHECK_LAUNCH();
        return 0;
    };
    auto by_d = [&](auto fam, auto hp) {
        if (reg) return launch(fam, std::integral_constant<int, 0>{}, hp);
        if (d == 1) return launch(fam, std::integral_constant<int, 2>{}, hp);
        if (d == 2) return launch(fam, std::integral_constant<int, 4>{}, hp);
        return launch(fam, std::integral_constant<int, 6>{}, hp);
    };
    using T = std::true_type;
    using F = std::false_type;
    switch (family) {
    case SGPR_FAM_A: return by_d(std::integral_constant<int, SGPR_FAM_A>{}, F{});
    case SGPR_FAM_B: return by_d(std::integral_constant<int, SGPR_FAM_B>{}, F{});
    case SGPR_FAM_C: return by_d(std::integral_constant<int, SGPR_FAM_C>{}, F{});
    case SGPR_FAM_D: return by_d(std::integral_constant<int, SGPR_FAM_D>{}, T{});
    case SGPR_FAM_USER: return by_d(std::integral_constant<int, SGPR_FAM_USER>{}, std::integral_constant<bool, gen::user_has_p>{});
    }
    set_error("nll_grad_full: unknown kernel family");
    return SGPR_E_ARG;
}

}  // namespace

// the rows of a panel of Ky^-1 (shape_of's rule, shared with loo.hip); `knob`: the caller's tunable
int kyinv_panel_width(int n, const char *knob)
{
    const int t = (int)tune(knob, 0);
    return t > 0 && t % LEAF == 0 ? t : (n <= 8192 ? 2048 : 4096);
}

// R (rows x (n - J), leading dimension ldr) = Ky^-1[J:J+rows, J:] from the factor L (order n) and its workspace
int kyinv_row_panel(int n, int J, int rows, const double *L, size_t ldl, const void *work, double *R, size_t ldr, hipStream_t st)
{
    const int w = n - J;
    int rc;
    SGPR_HIP(hipMemsetAsync(R, 0, ldr * w * sizeof(double), st));
    hipLaunchKernelGGL(panel_identity_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, rows, R, ldr);
    SGPR_CHECK_LAUNCH();
    const double *Ltt = L + J + (size_t)J * ldl;
    if ((rc = trsm_rlt_off(rows, w, Ltt, ldl, R, ldr, work, J, st))) return rc;   // R := R L_tt^-T
    if ((rc = trsm_rl_off(rows, w, Ltt, ldl, R, ldr, work, J, st))) return rc;    // R := R L_tt^-1
    return 0;
}

// what loograd.hip needs of the contraction: the workgroups of one panel of ldr rows, one launch with the rank-2 weight
// M_p - (beta alpha^T + alpha beta^T) on the panel Mp = M[J:J+rows, J:] (the geometry of R above), and the fold
size_t grad_contract_wgs(int ldr, int N) { return (size_t)((ldr + NG_T - 1) / NG_T) * (size_t)((N + NG_CJ - 1) / NG_CJ); }

int grad_contract_rank2(int family, int d, bool reg, int N, int J, int rows, const double *Mp, size_t ldr, const double *alpha,
                        const double *beta, const double *X, const double *l, const double *pp, double *part, size_t nwg,
                        size_t wg0, hipStream_t st)
{
    const int gx = ((int)ldr + NG_T - 1) / NG_T, gy = (N + NG_CJ - 1) / NG_CJ;
    if (gy > 65535) { set_error("loo_grad: too many points for one launch"); return SGPR_E_ARG; }
    const bool hasp = family_has_p(family);
    GradArgs a{};
    a.N = N; a.J = J; a.rows = rows; a.ldr = ldr; a.R = Mp; a.alpha = alpha; a.X = X;
    for (int m = 0; m < (reg ? 2 : 2 * d); ++m) a.l[m] = l[m];
    for (int m = 0; m < (reg ? 1 : d); ++m) a.pp[m] = hasp ? pp[m] : 0.0;
    a.part = part; a.nwg = nwg; a.wg0 = wg0;
    return launch_contract(family, d, reg, beta, dim3(gx, gy), a, st);
}

int grad_fold(const double *part, size_t nwg, int nacc, double *out, hipStream_t st)
{
    hipLaunchKernelGGL(nllgrad_fold_kernel, dim3(nacc), dim3(NG_FOLD), 0, st, part, nwg, out);
    SGPR_CHECK_LAUNCH();
    return 0;
}

size_t nll_grad_full_scratch(int n, int N, int nacc)
{
    const Shape s = shape_of(n, N);
    return ((size_t)s.ldr * n + s.nwg * nacc) * sizeof(double);
}

// out (device, nacc doubles): the raw sums -- per length / period sum_ij W_ij dK_ij / sig, then sum_ij W_ij K_ij / sig,
// then sum_i W_ii -- with W = Ky^-1 - alpha alpha^T; the caller scales them.  nacc = 2d + [d] + 2 (pair fits, d = 1 .. 3)
// or 2 + [1] + 2 (reg), the brackets for a family with a period.  scratch: nll_grad_full_scratch(n, N, nacc) bytes.
int nll_grad_full(int family, int d, bool reg, int N, int n, const double *L, size_t ldl, const void *work, const double *X,
                  const double *alpha, const double *l, const double *pp, int nacc, double *scratch, double *out,
                  hipStream_t st)
{
    if (N <= 0 || n != (reg ? N : 2 * d * N) || d < 1 || d > 3 || (reg && d != 1)) { set_error("nll_grad_full: bad shape"); return SGPR_E_ARG; }
    const bool hasp = family_has_p(family);
    if (nacc != (reg ? 2 : 2 * d) + (hasp ? d : 0) + 2) { set_error("nll_grad_full: bad component count"); return SGPR_E_ARG; }
    const Shape s = shape_of(n, N);
    if (s.gy > 65535) { set_error("nll_grad_full: too many points for one launch"); return SGPR_E_ARG; }
    GradArgs a{};
    a.N = N; a.ldr = (size_t)s.ldr; a.R = scratch; a.alpha = alpha; a.X = X;
    for (int m = 0; m < (reg ? 2 : 2 * d); ++m) a.l[m] = l[m];
    for (int m = 0; m < (reg ? 1 : d); ++m) a.pp[m] = hasp ? pp[m] : 0.0;
    a.part = scratch + (size_t)s.ldr * n;
    a.nwg = s.nwg;
    double *R = scratch;
    int rc;
    for (int p = 0; p < s.npanels; ++p) {
        const int J = p * s.nb, rows = n - J < s.nb ? n - J : s.nb;
        if ((rc = kyinv_row_panel(n, J, rows, L, ldl, work, R, (size_t)s.ldr, st))) return rc;
        a.J = J; a.rows = rows; a.wg0 = (size_t)p * s.gx * s.gy;
        if ((rc = launch_contract(family, d, reg, nullptr, dim3(s.gx, s.gy), a, st))) return rc;
    }
    hipLaunchKernelGGL(nllgrad_fold_kernel, dim3(nacc), dim3(NG_FOLD), 0, st, a.part, s.nwg, out);
    SGPR_CHECK_LAUNCH();
    return 0;
}

}  // namespace sgpr
