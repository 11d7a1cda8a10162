// gram.hip -- Gram-matrix build for gfx950 (MI355X).
//
// Replaces the pair loop of the reference's build_K / buildKreg
// (python/05_tokamak/SympGPR/sympgpr.f90:25-37, :54-59; pure-Python form
// python/01_pendulum/implicit/func.py:55-64) and the scalar kernels they call
// (kernels.f90:1-11,58-94 and the kernels_sq / kernels_sum / period-unknown variants).
//
// Roofline: HBM write.  One pair (i,j) yields four fp64 entries = 32 B written and costs one
// exp + one sincos + ~20 FMA, all on the fp64 VALU.  Layout decisions:
//   * column-major output, so the row index i is the contiguous one: a thread owns TWO
//     consecutive rows (one 16-B store per part), a wave writes 1 KiB contiguous per store
//     instruction, a workgroup owns a 512-row x 16-column pair tile = 4 x 64 KiB of K;
//   * the 16 column points of the tile are staged once in LDS and read back as broadcasts;
//   * sig scaling, the |sig2n| diagonal and the lower-triangle cut are fused here (the
//     reference spends three more n^2 passes on them: sympgpr.f90:37, func.py:192).
#include "common.h"
#include "devmath.h"
#include "pair_eval.h"

namespace sgpr {

namespace {

constexpr int GT = 256;        // threads per workgroup
constexpr int TI = 2 * GT;     // pair rows per tile (2 per thread)
constexpr int TJ = 16;         // pair columns per tile (32 -> 16: n = 16384 0.49 -> 0.46 ms, no change at n = 131072)

typedef double double2_t __attribute__((ext_vector_type(2)));

struct GramArgs {
    int mi, mj;
    const double *xb, *yb, *xa, *ya;
    double *dst[4];  // qq, Pq, qP, PP
    size_t ld;
    long diag_off;
    double noise;
    unsigned flags;
    KConst kc;
};

using namespace pairf;

template <int FAM, bool OCML, int DL>
__global__ __launch_bounds__(GT) void gram_pairs_kernel(const GramArgs a)
{
    __shared__ double sxa[TJ], sya[TJ];
    const int i0 = blockIdx.x * TI;
    const int j0 = blockIdx.y * TJ;
    const int t = threadIdx.x;
    const int nj = min(TJ, a.mj - j0);
    if (t < nj) {
        sxa[t] = a.xa[j0 + t];
        sya[t] = a.ya[j0 + t];
    }
    // which parts does this tile write?  (block-uniform)
    const bool lower = a.flags & SGPR_G_LOWER;
    const long last_row = (long)min(i0 + TI, a.mi) - 1 + a.diag_off;
    const bool on_or_below = !lower || last_row >= (long)j0;
    double *const pqq = (a.flags & SGPR_G_QQ) && on_or_below ? a.dst[0] : nullptr;
    double *const pPq = (a.flags & SGPR_G_PQ) ? a.dst[1] : nullptr;
    double *const pqP = (a.flags & SGPR_G_QP) && !lower ? a.dst[2] : nullptr;
    double *const pPP = (a.flags & SGPR_G_PP) && on_or_below ? a.dst[3] : nullptr;
    __syncthreads();
    if (!pqq && !pPq && !pqP && !pPP) return;

    const int i = i0 + 2 * t;
    const bool v0 = i < a.mi, v1 = i + 1 < a.mi;
    const double xb0 = v0 ? a.xb[i] : 0.0, yb0 = v0 ? a.yb[i] : 0.0;
    const double xb1 = v1 ? a.xb[i + 1] : 0.0, yb1 = v1 ? a.yb[i + 1] : 0.0;
    // 16-B vector stores need every part's (i, j) address 16-B aligned: i is even, so the
    // base pointers and ld decide (block-uniform); the ragged last row tile goes scalar.
    const bool vec = (i0 + TI <= a.mi) && ((a.ld & 1) == 0) &&
                     ((((uintptr_t)a.dst[0] | (uintptr_t)a.dst[1] | (uintptr_t)a.dst[2] |
                        (uintptr_t)a.dst[3]) & 15) == 0);
    const long d0 = (long)i + a.diag_off;  // global column that is "diagonal" for row i
    const double noise = a.noise;

    if (vec) {
#pragma unroll 2
        for (int jj = 0; jj < nj; ++jj) {
            const double xa = sxa[jj], ya = sya[jj];
            double kxx0, kxy0, kyy0, kxx1, kxy1, kyy1;
            pair_any<FAM, OCML, DL>(xa, ya, xb0, yb0, a.kc, kxx0, kxy0, kyy0);
            pair_any<FAM, OCML, DL>(xa, ya, xb1, yb1, a.kc, kxx1, kxy1, kyy1);
            const long j = j0 + jj;
            const double n0 = (d0 == j) ? noise : 0.0, n1 = (d0 + 1 == j) ? noise : 0.0;
            const size_t off = (size_t)i + (size_t)j * a.ld;
            if (pqq) *reinterpret_cast<double2_t *>(pqq + off) = double2_t{kxx0 + n0, kxx1 + n1};
            if (pPq) *reinterpret_cast<double2_t *>(pPq + off) = double2_t{kxy0, kxy1};
            if (pqP) *reinterpret_cast<double2_t *>(pqP + off) = double2_t{kxy0, kxy1};
            if (pPP) *reinterpret_cast<double2_t *>(pPP + off) = double2_t{kyy0 + n0, kyy1 + n1};
        }
    } else {
        for (int jj = 0; jj < nj; ++jj) {
            const double xa = sxa[jj], ya = sya[jj];
            double kxx0, kxy0, kyy0, kxx1, kxy1, kyy1;
            pair_any<FAM, OCML, DL>(xa, ya, xb0, yb0, a.kc, kxx0, kxy0, kyy0);
            pair_any<FAM, OCML, DL>(xa, ya, xb1, yb1, a.kc, kxx1, kxy1, kyy1);
            const long j = j0 + jj;
            const double n0 = (d0 == j) ? noise : 0.0, n1 = (d0 + 1 == j) ? noise : 0.0;
            const size_t off = (size_t)i + (size_t)j * a.ld;
            if (v0) {
                if (pqq) pqq[off] = kxx0 + n0;
                if (pPq) pPq[off] = kxy0;
                if (pqP) pqP[off] = kxy0;
                if (pPP) pPP[off] = kyy0 + n0;
            }
            if (v1) {
                if (pqq) pqq[off + 1] = kxx1 + n1;
                if (pPq) pPq[off + 1] = kxy1;
                if (pqP) pqP[off + 1] = kxy1;
                if (pPP) pPP[off + 1] = kyy1 + n1;
            }
        }
    }
}

struct RegArgs {
    int mi, mj;
    const double *xb, *yb, *xa, *ya;
    double *G;
    size_t ld;
    long diag_off;
    double noise;
    KConst kc;
};

template <int FAM, bool OCML, int DL>
__global__ __launch_bounds__(GT) void gram_reg_kernel(const RegArgs a)
{
    __shared__ double sxa[TJ], sya[TJ];
    const int i0 = blockIdx.x * TI;
    const int j0 = blockIdx.y * TJ;
    const int t = threadIdx.x;
    const int nj = min(TJ, a.mj - j0);
    if (t < nj) {
        sxa[t] = a.xa[j0 + t];
        sya[t] = a.ya[j0 + t];
    }
    __syncthreads();
    const int i = i0 + 2 * t;
    const bool v0 = i < a.mi, v1 = i + 1 < a.mi;
    const double xb0 = v0 ? a.xb[i] : 0.0, yb0 = v0 ? a.yb[i] : 0.0;
    const double xb1 = v1 ? a.xb[i + 1] : 0.0, yb1 = v1 ? a.yb[i + 1] : 0.0;
    const bool vec = (i0 + TI <= a.mi) && ((a.ld & 1) == 0) && (((uintptr_t)a.G & 15) == 0);
    const long d0 = (long)i + a.diag_off;
    for (int jj = 0; jj < nj; ++jj) {
        const double xa = sxa[jj], ya = sya[jj];
        const long j = j0 + jj;
        const double k0 = a.kc.sig * kern_any<FAM, OCML, DL>(xa, ya, xb0, yb0, a.kc) +
                          ((d0 == j) ? a.noise : 0.0);
        const double k1 = a.kc.sig * kern_any<FAM, OCML, DL>(xa, ya, xb1, yb1, a.kc) +
                          ((d0 + 1 == j) ? a.noise : 0.0);
        const size_t off = (size_t)i + (size_t)j * a.ld;
        if (vec) {
            *reinterpret_cast<double2_t *>(a.G + off) = double2_t{k0, k1};
        } else {
            if (v0) a.G[off] = k0;
            if (v1) a.G[off + 1] = k1;
        }
    }
}

// kernels.<name>_num, elementwise (sig = 1).  DL selects the length-scale derivative family
// (dkdlx_num, d3kdxdx0dlx_num, ... kernels.f90:133-231).
template <int FAM, int DL>
__global__ void kernel_eval_kernel(int which, int m, const double *xa, const double *ya,
                                   const double *xb, const double *yb, const KConst kc, double *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double r;
    if (which == SGPR_K_KERN) {
        r = kern_any<FAM, false, DL>(xa[i], ya[i], xb[i], yb[i], kc);
    } else {
        double kxx, kxy, kyy;
        pair_any<FAM, false, DL>(xa[i], ya[i], xb[i], yb[i], kc, kxx, kxy, kyy);
        r = which == SGPR_K_DXDX0 ? kxx : (which == SGPR_K_DYDY0 ? kyy : kxy);
    }
    out[i] = r;
}

// The seven generated functions no caller of the reference uses (first derivatives, third derivatives
// with respect to y_b: kernels.f90:12-57,95-132 and the sibling files), for the completeness of the
// `kernels` module.  Not a hot path: plain device-libs sin / cos / exp.
template <int FAM>
__device__ double extra_eval(int which, double xa, double ya, double xb, double yb, const KConst &kc)
{
    if constexpr (FAM == SGPR_FAM_USER) return gen::extra<SGPR_FAM_USER>(which, xa, ya, xb, yb, kc.lx, kc.ly, kc.p);
    const double lx2 = kc.lx2, ly2 = kc.ly2, dy = ya - yb;
    if constexpr (FAM == SGPR_FAM_A || FAM == SGPR_FAM_D) {
        const double h = FAM == SGPR_FAM_A ? 0.5 * xa - 0.5 * xb : kc.p * (xa - xb);
        const double hs = FAM == SGPR_FAM_A ? 0.5 : kc.p;
        const double s = sin(h), c = cos(h), cd = cos(2.0 * h);
        const double E = exp(-0.5 * (lx2 * dy * dy + ly2 * s * s) / (lx2 * ly2));
        switch (which) {
        case SGPR_K_DX: return -hs * E * s * c / lx2;
        case SGPR_K_DY: return -dy * E / ly2;
        case SGPR_K_DX0: return hs * E * s * c / lx2;
        case SGPR_K_DY0: return dy * E / ly2;
        case SGPR_K_DXDX0DY0: return hs * hs * dy * (lx2 * cd - s * s * c * c) * E / (lx2 * lx2 * ly2);
        case SGPR_K_DYDY0DY0: return (3.0 * ly2 - dy * dy) * dy * E / (ly2 * ly2 * ly2);
        default: return hs * (ly2 - dy * dy) * E * s * c / (lx2 * ly2 * ly2);   // SGPR_K_DXDY0DY0
        }
    } else if constexpr (FAM == SGPR_FAM_B) {
        const double h = 0.5 * xa - 0.5 * xb, s = sin(h), c = cos(h);
        const double ex = exp(-0.5 * s * s / lx2);
        const double ey = exp((-0.5 * ya * ya + ya * yb - 0.5 * yb * yb) / ly2);
        switch (which) {
        case SGPR_K_DX: return -0.5 * ex * s * c / lx2;
        case SGPR_K_DY: return -dy * ey / ly2;
        case SGPR_K_DX0: return 0.5 * ex * s * c / lx2;
        case SGPR_K_DY0: return dy * ey / ly2;
        case SGPR_K_DYDY0DY0: return (3.0 * ly2 - dy * dy) * dy * ey / (ly2 * ly2 * ly2);
        default: return 0.0;                                                    // the mixed ones vanish
        }
    } else {
        const double dx = xa - xb;
        const double E = exp(-0.5 * (lx2 * dy * dy + ly2 * dx * dx) / (lx2 * ly2));
        switch (which) {
        case SGPR_K_DX: return -dx * E / lx2;
        case SGPR_K_DY: return -dy * E / ly2;
        case SGPR_K_DX0: return dx * E / lx2;
        case SGPR_K_DY0: return dy * E / ly2;
        case SGPR_K_DXDX0DY0: return (lx2 - dx * dx) * dy * E / (lx2 * lx2 * ly2);
        case SGPR_K_DYDY0DY0: return (3.0 * ly2 - dy * dy) * dy * E / (ly2 * ly2 * ly2);
        default: return (ly2 - dy * dy) * dx * E / (lx2 * ly2 * ly2);
        }
    }
}

template <int FAM>
__global__ void kernel_extra_kernel(int which, int m, const double *xa, const double *ya, const double *xb,
                                    const double *yb, const KConst kc, double *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) out[i] = extra_eval<FAM>(which, xa[i], ya[i], xb[i], yb[i], kc);
}

// K*(2 x 2n0) . alpha for one test point per workgroup (sympgpr.f90:75-86, :112-124 with
// alpha = Kyinv ztrain cached): row 1 -> out_p, row 2 -> out_q.
template <int FAM>
__global__ __launch_bounds__(GT) void predict_rows_kernel(int n0, const double *q, const double *P,
                                                          const double *xtr, const double *ytr,
                                                          const KConst kc, const double *alpha,
                                                          double *out_p, double *out_q)
{
    const int k = blockIdx.x;
    const double xb = q[k], yb = P[k];
    double r1 = 0.0, r2 = 0.0;
    for (int j = threadIdx.x; j < n0; j += GT) {
        double kxx, kxy, kyy;
        pair_eval<FAM, false>(xtr[j], ytr[j], xb, yb, kc, kxx, kxy, kyy);
        const double a1 = alpha[j], a2 = alpha[n0 + j];
        r1 += kxx * a1 + kxy * a2;
        r2 += kxy * a1 + kyy * a2;
    }
    __shared__ double s1[GT / 64], s2[GT / 64];
    for (int o = 32; o > 0; o >>= 1) {
        r1 += __shfl_down(r1, o, 64);
        r2 += __shfl_down(r2, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s1[threadIdx.x >> 6] = r1;
        s2[threadIdx.x >> 6] = r2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t1 = 0.0, t2 = 0.0;
        for (int w = 0; w < GT / 64; ++w) {
            t1 += s1[w];
            t2 += s2[w];
        }
        out_p[k] = t1;
        out_q[k] = t2;
    }
}

// Kstar(1 x n0) . alpha_p with the scalar kernel (sympgpr.f90:62-73 guessP)
template <int FAM>
__global__ __launch_bounds__(GT) void predict_reg_kernel(int n0, const double *q, const double *P,
                                                         const double *xtr, const double *ytr,
                                                         const KConst kc, const double *alpha,
                                                         double *out)
{
    const int k = blockIdx.x;
    const double xb = q[k], yb = P[k];
    double r = 0.0;
    for (int j = threadIdx.x; j < n0; j += GT)
        r += kc.sig * kern_eval<FAM, false>(xtr[j], ytr[j], xb, yb, kc) * alpha[j];
    __shared__ double s1[GT / 64];
    for (int o = 32; o > 0; o >>= 1) r += __shfl_down(r, o, 64);
    if ((threadIdx.x & 63) == 0) s1[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < GT / 64; ++w) t += s1[w];
        out[k] = t;
    }
}

}  // namespace

bool family_has_p(int family) { return family == SGPR_FAM_D || (family == SGPR_FAM_USER && gen::user_has_p); }

int make_kconst(int family, const double *hyp, int nhyp, KConst *out)
{
    const bool has_p = family_has_p(family);
    const int need = has_p ? 4 : 3;
    if (family < SGPR_FAM_A || family > SGPR_FAM_USER || !hyp || nhyp != need) {
        set_error("hyp must hold (lx, ly, sig) -- (lx, ly, p, sig) for family D");
        return SGPR_E_ARG;
    }
    KConst k{};
    k.lx = hyp[0];
    k.ly = hyp[1];
    k.p = has_p ? hyp[2] : 0.0;
    k.sig = hyp[nhyp - 1];
    k.lx2 = k.lx * k.lx;
    k.ly2 = k.ly * k.ly;
    k.inv_lx2 = 1.0 / k.lx2;
    k.inv_ly2 = 1.0 / k.ly2;
    const double pp = family == SGPR_FAM_D ? k.p * k.p : (family == SGPR_FAM_C ? 1.0 : 0.25);
    const double pm = family == SGPR_FAM_D ? k.p : (family == SGPR_FAM_C ? 1.0 : 0.5);
    k.cxx = k.sig * pp / (k.lx2 * k.lx2);
    k.cyy = k.sig / (k.ly2 * k.ly2);
    k.cxy = -k.sig * pm / (k.lx2 * k.ly2);
    k.hscale = family == SGPR_FAM_D ? k.p : 0.5;
    k.inv_lx = 1.0 / k.lx;
    k.inv_ly = 1.0 / k.ly;
    k.inv_lx3 = 1.0 / (k.lx2 * k.lx);
    k.inv_ly3 = 1.0 / (k.ly2 * k.ly);
    k.gxx = k.sig * pp;
    *out = k;
    return 0;
}

int make_kconst_l(int family, const double *l, int nl, KConst *out)
{
    double h[4];
    const int need = family_has_p(family) ? 3 : 2;
    if (!l || nl != need) {
        set_error("l must hold (lx, ly) -- (lx, ly, p) for family D");
        return SGPR_E_ARG;
    }
    for (int i = 0; i < nl; ++i) h[i] = l[i];
    h[nl] = 1.0;
    return make_kconst(family, h, nl + 1, out);
}

int gram_pairs(int family, int mi, int mj, const double *xb, const double *yb, const double *xa,
               const double *ya, const KConst &kc, double *qq, double *Pq, double *qP, double *PP,
               size_t ld, long diag_off, double noise, unsigned flags, hipStream_t st)
{
    if (mi < 0 || mj < 0) { set_error("negative extent"); return SGPR_E_ARG; }
    if (mi == 0 || mj == 0) return 0;
    unsigned parts = flags & SGPR_G_ALL;
    if (!qq) parts &= ~SGPR_G_QQ;
    if (!Pq) parts &= ~SGPR_G_PQ;
    if (!qP) parts &= ~SGPR_G_QP;
    if (!PP) parts &= ~SGPR_G_PP;
    if (!parts) return 0;
    if (ld < (size_t)mi) { set_error("ld smaller than the tile's row count"); return SGPR_E_ARG; }
    GramArgs a;
    a.mi = mi; a.mj = mj; a.xb = xb; a.yb = yb; a.xa = xa; a.ya = ya;
    a.dst[0] = qq; a.dst[1] = Pq; a.dst[2] = qP; a.dst[3] = PP;
    a.ld = ld; a.diag_off = diag_off; a.noise = noise;
    a.flags = parts | (flags & SGPR_G_LOWER);
    a.kc = kc;
    const dim3 grid((mi + TI - 1) / TI, (mj + TJ - 1) / TJ);
    if (grid.y > 65535) { set_error("too many pair columns for one launch"); return SGPR_E_ARG; }
    const bool ocml = flags & SGPR_G_OCML;
    const int deriv = (flags & SGPR_G_DLX) ? DERIV_LX : ((flags & SGPR_G_DLY) ? DERIV_LY : DERIV_NONE);
    return dispatch_family(family, [&](auto fam) {
        constexpr int F = decltype(fam)::value;
        if (deriv == DERIV_LX)      hipLaunchKernelGGL((gram_pairs_kernel<F, false, DERIV_LX>), grid, dim3(GT), 0, st, a);
        else if (deriv == DERIV_LY) hipLaunchKernelGGL((gram_pairs_kernel<F, false, DERIV_LY>), grid, dim3(GT), 0, st, a);
        else if (ocml) hipLaunchKernelGGL((gram_pairs_kernel<F, true, DERIV_NONE>), grid, dim3(GT), 0, st, a);
        else           hipLaunchKernelGGL((gram_pairs_kernel<F, false, DERIV_NONE>), grid, dim3(GT), 0, st, a);
        SGPR_CHECK_LAUNCH();
        return 0;
    });
}

int gram_reg(int family, int mi, int mj, const double *xb, const double *yb, const double *xa,
             const double *ya, const KConst &kc, double *G, size_t ld, long diag_off, double noise,
             hipStream_t st, int deriv)
{
    if (mi < 0 || mj < 0) { set_error("negative extent"); return SGPR_E_ARG; }
    if (mi == 0 || mj == 0) return 0;
    if (ld < (size_t)mi) { set_error("ld smaller than the tile's row count"); return SGPR_E_ARG; }
    RegArgs a{mi, mj, xb, yb, xa, ya, G, ld, diag_off, noise, kc};
    const dim3 grid((mi + TI - 1) / TI, (mj + TJ - 1) / TJ);
    if (grid.y > 65535) { set_error("too many pair columns for one launch"); return SGPR_E_ARG; }
    return dispatch_family(family, [&](auto fam) {
        constexpr int F = decltype(fam)::value;
        if (deriv == DERIV_LX)      hipLaunchKernelGGL((gram_reg_kernel<F, false, DERIV_LX>), grid, dim3(GT), 0, st, a);
        else if (deriv == DERIV_LY) hipLaunchKernelGGL((gram_reg_kernel<F, false, DERIV_LY>), grid, dim3(GT), 0, st, a);
        else                        hipLaunchKernelGGL((gram_reg_kernel<F, false, DERIV_NONE>), grid, dim3(GT), 0, st, a);
        SGPR_CHECK_LAUNCH();
        return 0;
    });
}

int kernel_eval(int family, int which, int m, const double *xa, const double *ya, const double *xb,
                const double *yb, const KConst &kc, double *out, hipStream_t st)
{
    if (m <= 0) return 0;
    if (which >= SGPR_K_DX && which <= SGPR_K_DXDY0DY0)
        return dispatch_family(family, [&](auto fam) {
            constexpr int F = decltype(fam)::value;
            hipLaunchKernelGGL((kernel_extra_kernel<F>), dim3((m + 255) / 256), dim3(256), 0, st, which, m, xa, ya,
                               xb, yb, kc, out);
            SGPR_CHECK_LAUNCH();
            return 0;
        });
    const int deriv = which >> 2;
    which &= 3;
    if (deriv < 0 || deriv > 2) { set_error("unknown kernel function"); return SGPR_E_ARG; }
    return dispatch_family(family, [&](auto fam) {
        constexpr int F = decltype(fam)::value;
        const dim3 grid((m + 255) / 256);
        if (deriv == DERIV_LX)      hipLaunchKernelGGL((kernel_eval_kernel<F, DERIV_LX>), grid, dim3(256), 0, st, which, m, xa, ya, xb, yb, kc, out);
        else if (deriv == DERIV_LY) hipLaunchKernelGGL((kernel_eval_kernel<F, DERIV_LY>), grid, dim3(256), 0, st, which, m, xa, ya, xb, yb, kc, out);
        else                        hipLaunchKernelGGL((kernel_eval_kernel<F, DERIV_NONE>), grid, dim3(256), 0, st, which, m, xa, ya, xb, yb, kc, out);
        SGPR_CHECK_LAUNCH();
        return 0;
    });
}

int predict_rows(int family, int m, const double *q, const double *P, int n0, const double *xtr,
                 const double *ytr, const KConst &kc, const double *alpha, double *out_p,
                 double *out_q, hipStream_t st)
{
    if (m <= 0) return 0;
    return dispatch_family(family, [&](auto fam) {
        constexpr int F = decltype(fam)::value;
        hipLaunchKernelGGL((predict_rows_kernel<F>), dim3(m), dim3(GT), 0, st, n0, q, P, xtr, ytr,
                           kc, alpha, out_p, out_q);
        SGPR_CHECK_LAUNCH();
        return 0;
    });
}

int predict_reg(int family, int m, const double *q, const double *P, int n0, const double *xtr,
                const double *ytr, const KConst &kc, const double *alpha, double *out,
                hipStream_t st)
{
    if (m <= 0) return 0;
    return dispatch_family(family, [&](auto fam) {
        constexpr int F = decltype(fam)::value;
        hipLaunchKernelGGL((predict_reg_kernel<F>), dim3(m), dim3(GT), 0, st, n0, q, P, xtr, ytr,
                           kc, alpha, out);
        SGPR_CHECK_LAUNCH();
        return 0;
    });
}

}  // namespace sgpr
