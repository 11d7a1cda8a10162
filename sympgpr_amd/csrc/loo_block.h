// loo_block.h -- the per-point algebra of leave-one-point-out cross-validation, shared by loo.hip (a fit handle) and
// batch.hip (the batched fits).  Point i owns the D rows B_i = {c N + i} of Ky; with C = (Ky^-1)[B_i, B_i] and a = alpha[B_i]
//     r = C^-1 a                      the observed rows minus their prediction from the fit without point i,
//     S = C^-1                        the covariance of that prediction (noise included),
//     lpd = -1/2 a^T C^-1 a + 1/2 log det C - D/2 log 2 pi
// (Rasmussen & Williams 5.4.2, for a block of rows).  Everything stays in registers: C = G G^T, X = G^-1, y = X a,
// r = X^T y, S = X^T X, 1/2 log det C = sum log G_kk.  A pivot that is not positive and finite gives NaN in every output.
#pragma once

namespace sgpr {
namespace loo {

constexpr double LOG_2PI = 1.8378770664093454835606594728112;

// packed lower triangle, row by row: (e, c), e >= c
__host__ __device__ constexpr int pk(int e, int c) { return e * (e + 1) / 2 + c; }

template <int D>
__device__ __forceinline__ void block(const double (&C)[D * (D + 1) / 2], const double (&a)[D], double (&r)[D],
                                      double (&S)[D * (D + 1) / 2], double &lpd)
{
    constexpr int T = D * (D + 1) / 2;
    double G[T], X[T], y[D];
    bool ok = true;
    double logdet = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        double d = C[pk(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d = __builtin_fma(-G[pk(j, k)], G[pk(j, k)], d);
        if (!(d > 0.0) || !__builtin_isfinite(d)) ok = false;
        const double g = sqrt(d), gi = 1.0 / g;
        G[pk(j, j)] = g;
        X[pk(j, j)] = gi;
        logdet += log(g);
#pragma unroll
        for (int i = j + 1; i < D; ++i) {
            double s = C[pk(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) s = __builtin_fma(-G[pk(i, k)], G[pk(j, k)], s);
            G[pk(i, j)] = s * gi;
        }
    }
    // X = G^-1, column by column
#pragma unroll
    for (int j = 0; j < D; ++j) {
#pragma unroll
        for (int i = j + 1; i < D; ++i) {
            double s = 0.0;
#pragma unroll
            for (int k = j; k < i; ++k) s = __builtin_fma(G[pk(i, k)], X[pk(k, j)], s);
            X[pk(i, j)] = -s * X[pk(i, i)];
        }
    }
    double quad = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k <= i; ++k) s = __builtin_fma(X[pk(i, k)], a[k], s);
        y[i] = s;
        quad = __builtin_fma(s, s, quad);
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
        double s = 0.0;
#pragma unroll
        for (int i = k; i < D; ++i) s = __builtin_fma(X[pk(i, k)], y[i], s);
        r[k] = s;
    }
#pragma unroll
    for (int e = 0; e < D; ++e) {
#pragma unroll
        for (int c = 0; c <= e; ++c) {
            double s = 0.0;
#pragma unroll
            for (int k = e; k < D; ++k) s = __builtin_fma(X[pk(k, e)], X[pk(k, c)], s);
            S[pk(e, c)] = s;
        }
    }
    lpd = -0.5 * quad + logdet - 0.5 * D * LOG_2PI;
    if (!ok) {
        const double nan = __builtin_nan("");
        lpd = nan;
#pragma unroll
        for (int k = 0; k < D; ++k) r[k] = nan;
#pragma unroll
        for (int k = 0; k < T; ++k) S[k] = nan;
    }
}

}  // namespace loo
}  // namespace sgpr
