// postcov.hip -- the reduction of the predictive covariance (sgpr_fit_predict_cov): with V = L^-1 K*^T (n x D mc, the
// columns of test point t at a mc + t, a = 0 .. D-1) and the chunk's test x test Gram block K** (D mc x D mc, same index map),
//     cov_t(a, b) = K**(a mc + t, b mc + t) - sum_k V(k, a mc + t) V(k, b mc + t).
// Two launches, no atomics, so a repeated call gives the same bits:
//   stage 1: one workgroup per (slab of PC_SLAB rows, point): the D (D + 1) / 2 products of the upper triangle summed over its
//            rows (lanes on consecutive rows: every column read is coalesced), folded wave by wave in a fixed order;
//   stage 2: one wave per point folds the slabs in order, subtracts from K**, writes both triangles from the one value.
// The slabs depend on n alone, so a point's partial sums do not depend on which chunk it falls in.  HBM-read bound (V read
// once: 8 n D mc bytes per chunk), small next to the forward solve that produced V (4 n^2 bytes per 64 columns).
#include <type_traits>

#include "common.h"

namespace sgpr {

constexpr int PC_T = 256;       // threads of a stage-1 workgroup
constexpr int PC_SLAB = 2048;   // rows of V per stage-1 workgroup (8 per thread)

static int postcov_slabs(int n) { return (n + PC_SLAB - 1) / PC_SLAB; }

// pair p of the upper triangle (a <= b), row by row: (0,0), (0,1) .. (0,D-1), (1,1) ..
template <int D>
__device__ __forceinline__ void postcov_pair(int p, int &a, int &b)
{
    a = 0;
    while (p >= D - a) { p -= D - a; ++a; }
    b = a + p;
}

template <int D>
__global__ __launch_bounds__(PC_T) void postcov_partial_kernel(int n, int mc, const double *V, size_t ldv, double *part)
{
    constexpr int NP = D * (D + 1) / 2;
    const int slab = blockIdx.x, t = blockIdx.y, nslab = gridDim.x;
    const int k1 = min(n, (slab + 1) * PC_SLAB);
    const double *col[D];
#pragma unroll
    for (int a = 0; a < D; ++a) col[a] = V + (size_t)(a * mc + t) * ldv;
    double acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = 0.0;
#pragma unroll 4
    for (int k = slab * PC_SLAB + (int)threadIdx.x; k < k1; k += PC_T) {
        double v[D];
#pragma unroll
        for (int a = 0; a < D; ++a) v[a] = col[a][k];
        int p = 0;
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = a; b < D; ++b, ++p) acc[p] = __builtin_fma(v[a], v[b], acc[p]);
    }
    __shared__ double sh[PC_T / 64][NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        double s = acc[p];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][p] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < NP) {
        double s = sh[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < PC_T / 64; ++w) s += sh[w][threadIdx.x];
        part[((size_t)t * nslab + slab) * NP + threadIdx.x] = s;
    }
}

template <int D>
__global__ __launch_bounds__(64) void postcov_fold_kernel(int nslab, int mc, const double *Kss, size_t ldk, const double *part,
                                                          double *cov)
{
    constexpr int NP = D * (D + 1) / 2;
    const int t = blockIdx.x, p = threadIdx.x;
    if (p >= NP) return;
    int a, b;
    postcov_pair<D>(p, a, b);
    const double *pp = part + (size_t)t * nslab * NP + p;
    double s = 0.0;
    for (int j = 0; j < nslab; ++j) s += pp[(size_t)j * NP];
    const double c = Kss[(size_t)(a * mc + t) + (size_t)(b * mc + t) * ldk] - s;
    double *o = cov + (size_t)t * D * D;
    o[a + b * D] = c;
    o[b + a * D] = c;
}

size_t postcov_partial_doubles(int n, int D, int mc)
{
    return n <= 0 || mc <= 0 ? 0 : (size_t)postcov_slabs(n) * mc * (D * (D + 1) / 2);
}

// cov (mc blocks of D x D, column-major, block t at cov + t D D) for the chunk whose V (ld ldv >= n) and K** (ld ldk >= D mc)
// are given; part: postcov_partial_doubles(n, D, mc) doubles of device scratch
int postcov(int D, int n, int mc, const double *V, size_t ldv, const double *Kss, size_t ldk, double *part, double *cov,
            hipStream_t st)
{
    if (n <= 0 || mc <= 0) return 0;
    if (D * mc > POSTCOV_COLS || ldv < (size_t)n || ldk < (size_t)D * mc) { set_error("postcov: bad chunk shape"); return SGPR_E_ARG; }
    const int nslab = postcov_slabs(n);
    auto run = [&](auto dd) {
        constexpr int DD = decltype(dd)::value;
        hipLaunchKernelGGL(postcov_partial_kernel<DD>, dim3(nslab, mc), dim3(PC_T), 0, st, n, mc, V, ldv, part);
        SGPR_CHECK_LAUNCH();
        hipLaunchKernelGGL(postcov_fold_kernel<DD>, dim3(mc), dim3(64), 0, st, nslab, mc, Kss, ldk, part, cov);
        SGPR_CHECK_LAUNCH();
        return 0;
    };
    switch (D) {
    case 1: return run(std::integral_constant<int, 1>{});
    case 2: return run(std::integral_constant<int, 2>{});
    case 4: return run(std::integral_constant<int, 4>{});
    case 6: return run(std::integral_constant<int, 6>{});
    default: set_error("postcov: D must be 1, 2, 4 or 6"); return SGPR_E_ARG;
    }
}

}  // namespace sgpr
