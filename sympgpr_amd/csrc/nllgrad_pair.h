// nllgrad_pair.h -- one (row, column point) term of the NLL gradient contraction
//     sum_ij W_ij dK_ij / d theta,  W = Ky^-1 - alpha alpha^T,
// with dK evaluated in registers from the generated derivative forms (tools/gen_kernels.py), never stored: the per-pair body
// of nllgrad.hip's nllgrad_pairs_kernel / nllgrad_reg_kernel, for the one-workgroup gradient of a batch of small fits
// (batch.hip).  nllgrad_reg_kernel calls reg_grad (the same instructions as its former inline body); nllgrad_pairs_kernel
// keeps its inline copy of pair_grad: routed through the function, its d = 2, 3 instances fused a different set of
// multiply-adds and sgpr_fit_nll_grad_full moved by up to 1e-13 (relative) on seeded inputs.  tests/test_gpu_batch_grad.py
// holds the two together: every batched row is checked against SympFit.nll_grad_full.  The caller picks the entries, weights them (W on the diagonal, 2 W off it, 0 for an entry it does
// not visit) and keeps the sig2n sum (sum_i W_ii) itself.
#pragma once

#include "common.h"
#include "generated/pair_generated.h"

namespace sgpr {
namespace nllg {

template <int FAM> constexpr bool sum_kernel() { return gen::is_sum<FAM>(); }

// Pair fits, D = 2d output parts.  The row is part r of the point xi; w[c] weights the entry (row, c N + pj) of the column
// point xj.  Accumulators: acc[0 .. D-1] the lengths, acc[D .. D+NP-1] the periods (HASP), acc[D+NP] sig -- all without
// the factor sig, which the caller applies.
//   the product kernel K_ab = sig k B_ab, k = prod_m f_m, B_ab = (a == b ? -f_a''/f_a : -(f_a'/f_a)(f_b'/f_b)) (gram_nd.hip):
//       dK_ab / dl_m = K_ab d(log f_m)/dl_m + sig k dB_ab/dl_m,   the same for a period p_m,   dK / dsig = k B;
//   the sum kernel (family B): K_aa = sig f_a (-f_a''/f_a), other blocks zero.
template <int FAM, int D, bool HASP, int NACC>
__device__ __forceinline__ void pair_grad(const double (&xi)[D], const double *xj, const double (&w)[D], int r, const double *l,
                                          const double *pp, double (&acc)[NACC])
{
    constexpr int d = D / 2, NP = HASP ? d : 0;
    double arg[D], g[D], nh[D], dar[D], dg[D], dnh[D], par[d], pg[d], pnh[d];
#pragma unroll
    for (int m = 0; m < D; ++m) {
        const double dx = xj[m] - xi[m];   // column point - row point, as gram_nd
        double o[3], od[3];
        if (m < d) {
            gen::factor<FAM, 1>(dx, l[m], pp[m], o);
            gen::factor_dl<FAM, 1>(dx, l[m], pp[m], od);
            if constexpr (HASP) {
                double op[3];
                gen::factor_dp<FAM, 1>(dx, l[m], pp[m], op);
                par[m] = op[0]; pg[m] = op[1]; pnh[m] = op[2];
            }
        } else {
            gen::factor<FAM, 0>(dx, l[m], 0.0, o);
            gen::factor_dl<FAM, 0>(dx, l[m], 0.0, od);
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

// Reg fits (one part), K = sig k(x_j, y_j, x_i, y_i): the entry (i, j) weighted by w.  Accumulators: acc[0] lx, acc[1] ly,
// acc[2] p (HASP), acc[NACC - 2] sig -- without the factor sig; acc[NACC - 1] (sig2n) is the caller's.
template <int FAM, bool HASP, int NACC>
__device__ __forceinline__ void reg_grad(double xj, double yj, double xi, double yi, double w, const double *l, double p,
                                         double (&acc)[NACC])
{
    double o[4];
    gen::pair<FAM>(xj, yj, xi, yi, l[0], l[1], p, o);
    acc[NACC - 2] += w * o[0];
    gen::pair_dlx<FAM>(xj, yj, xi, yi, l[0], l[1], p, o);
    acc[0] += w * o[0];
    gen::pair_dly<FAM>(xj, yj, xi, yi, l[0], l[1], p, o);
    acc[1] += w * o[0];
    if constexpr (HASP) {
        gen::pair_dp<FAM>(xj, yj, xi, yi, l[0], l[1], p, o);
        acc[2] += w * o[0];
    }
}

}  // namespace nllg
}  // namespace sgpr
