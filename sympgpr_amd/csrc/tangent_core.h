// tangent_core.h -- the half of the tangent map that knows no data layout: the workgroup sum of NS values, the step matrix M
// from the Hessian of the generating function, and the monodromy product / Benettin step that follow from M.
//
// Included by map.hip (the sectioned d = 1 map: mapsec_tan.h sums its Hessian, D = 2) and by map_nd.hip (the d-pair map:
// maptan.h sums its Hessian, D = 2 d), each INSIDE its anonymous namespace.  It depends on common.h and devmath.h (finite_d) only:
// nothing here reads training points, hyper-parameters or an argument block.  maptan.h has the derivation of M.
#pragma once

// v[s] := the sum over the workgroup of every thread's v[s], the same bits in every thread: wave shuffle, one row of NS sums
// per wave in LDS, folded in wave order.  8 waves: lanes 0 .. NS-1 fold one sum each and publish it (NS instead of 8 NS
// reads per thread).  `part` (W NS doubles) and `res` (NS; not read with W <= 4) are the halves the call before did NOT use --
// the callers alternate, as block_sum2 of map.hip does: the barrier of call n + 1 lies between the reads of call n and the
// writes of call n + 2.
template <int NS, int TT>
__device__ __forceinline__ void block_sum_n(double (&v)[NS], double *part, double *res)
{
    constexpr int W = TT / 64;
#pragma unroll
    for (int s = 0; s < NS; ++s)
        for (int o = 32; o > 0; o >>= 1) v[s] += __shfl_down(v[s], o, 64);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int s = 0; s < NS; ++s) part[(threadIdx.x >> 6) * NS + s] = v[s];
    }
    __syncthreads();
    if constexpr (W <= 4) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            double x = 0.0;
#pragma unroll
            for (int w = 0; w < W; ++w) x += part[w * NS + s];
            v[s] = x;
        }
    } else {
        if (threadIdx.x < NS) {
            double x = 0.0;
#pragma unroll
            for (int w = 0; w < W; ++w) x += part[w * NS + threadIdx.x];
            res[threadIdx.x] = x;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < NS; ++s) v[s] = res[s];
    }
}

// the unordered pair (c, e), c <= e, in H: row after row of the upper triangle (D = 2: H = {A, B, C})
constexpr int hess_idx(int D, int c, int e) { return c * D - c * (c - 1) / 2 + (e - c); }
constexpr int hess_at(int D, int c, int e) { return c <= e ? hess_idx(D, c, e) : hess_idx(D, e, c); }

// C (d x d) := A B
template <int d>
__device__ __forceinline__ void mat_mul(const double (&A)[d * d], const double (&B)[d * d], double (&C)[d * d])
{
#pragma unroll
    for (int r = 0; r < d; ++r)
#pragma unroll
        for (int c = 0; c < d; ++c) {
            double v = 0.0;
#pragma unroll
            for (int s = 0; s < d; ++s) v = __builtin_fma(A[r * d + s], B[s * d + c], v);
            C[r * d + c] = v;
        }
}

// M from H (block-uniform values, every thread alike); T = (I + B)^-1 in closed form, the adjugate as in newton_step.
// false (and M all NaN): I + B singular or something not finite.
template <int D>
__device__ __forceinline__ bool maptan_matrix(const double (&H)[D * (D + 1) / 2], double (&M)[D * D])
{
    constexpr int d = D / 2;
    double A[d * d], Bm[d * d], C[d * d], K[d * d], T[d * d], TA[d * d], CT[d * d], CTA[d * d];
#pragma unroll
    for (int c = 0; c < d; ++c)
#pragma unroll
        for (int e = 0; e < d; ++e) {
            A[c * d + e] = H[hess_at(D, c, e)];
            Bm[c * d + e] = H[hess_idx(D, c, d + e)];
            C[c * d + e] = H[hess_at(D, d + c, d + e)];
            K[c * d + e] = Bm[c * d + e] + (c == e ? 1.0 : 0.0);
        }
    double det;
    if constexpr (d == 1) {
        det = K[0];
        T[0] = 1.0 / det;
    } else if constexpr (d == 2) {
        det = K[0] * K[3] - K[1] * K[2];
        const double id = 1.0 / det;
        T[0] = K[3] * id; T[1] = -K[1] * id;
        T[2] = -K[2] * id; T[3] = K[0] * id;
    } else {
        const double c00 = K[4] * K[8] - K[5] * K[7], c01 = K[5] * K[6] - K[3] * K[8], c02 = K[3] * K[7] - K[4] * K[6];
        const double c10 = K[2] * K[7] - K[1] * K[8], c11 = K[0] * K[8] - K[2] * K[6], c12 = K[1] * K[6] - K[0] * K[7];
        const double c20 = K[1] * K[5] - K[2] * K[4], c21 = K[2] * K[3] - K[0] * K[5], c22 = K[0] * K[4] - K[1] * K[3];
        det = K[0] * c00 + K[1] * c01 + K[2] * c02;
        const double id = 1.0 / det;
        T[0] = c00 * id; T[1] = c10 * id; T[2] = c20 * id;      // the adjugate is the transposed cofactor matrix
        T[3] = c01 * id; T[4] = c11 * id; T[5] = c21 * id;
        T[6] = c02 * id; T[7] = c12 * id; T[8] = c22 * id;
    }
    mat_mul<d>(T, A, TA);
    mat_mul<d>(C, T, CT);
    mat_mul<d>(C, TA, CTA);
    bool ok = finite_d(det) && det != 0.0;
#pragma unroll
    for (int c = 0; c < d; ++c)
#pragma unroll
        for (int e = 0; e < d; ++e) {
            M[c * D + e] = (c == e ? 1.0 : 0.0) + Bm[e * d + c] - CTA[c * d + e];
            M[c * D + d + e] = CT[c * d + e];
            M[(d + c) * D + e] = -TA[c * d + e];
            M[(d + c) * D + d + e] = T[c * d + e];
        }
#pragma unroll
    for (int s = 0; s < D * D; ++s) ok = ok && finite_d(M[s]);
    if (!ok) {
#pragma unroll
        for (int s = 0; s < D * D; ++s) M[s] = __builtin_nan("");
    }
    return ok;
}

// Lane c < D of wave 0 owns column c of mono and of Qmat and the sum c of log |r_cc|: (2 D + 2) D doubles in LDS, entry i of
// lane c at st[i * D + c] (i < D: mono, D <= i < 2 D: Qmat, i = 2 D, 2 D + 1: the sum).  Only the owner reads or writes its
// entries.  The sum is kept as log(m) + e log 2 with the product m of the r_cc's mantissas in [1, 2) and the sum e of their
// exponents, renormalised every step; the one log is taken when the orbit is done (maptan_finish).  A log call inside the step
// loop cost the D = 6 instances 20 VGPRs at their tightest point, and the 512-thread ones spilled.
// Behind them the step's M (D D doubles), which thread 0 hands to wave 0 through LDS: held in registers next to the columns it
// cost the D = 6 instances 30 VGPRs more than the passes need, and the 512-thread ones spilled.
template <int D>
__device__ __forceinline__ double *maptan_state()
{
    __shared__ double st[(2 * D + 2) * D + D * D];
    return st;
}
template <int D> constexpr int maptan_m_at() { return (2 * D + 2) * D; }

// thread 0 publishes the step's M: to jac (if wanted) and to wave 0
template <int D>
__device__ __forceinline__ void maptan_publish(const double (&M)[D * D], double *jac_out)
{
    double *ms = maptan_state<D>() + maptan_m_at<D>();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int s = 0; s < D * D; ++s) ms[s] = M[s];
        if (jac_out) {
#pragma unroll
            for (int s = 0; s < D * D; ++s) jac_out[s] = M[s];
        }
    }
    __syncthreads();
}

template <int D>
__device__ __forceinline__ void maptan_init()
{
    double *st = maptan_state<D>();
    const int lane = threadIdx.x;
    if (lane < D) {
#pragma unroll
        for (int r = 0; r < D; ++r) st[r * D + lane] = st[(D + r) * D + lane] = (r == lane) ? 1.0 : 0.0;
        st[2 * D * D + lane] = 1.0;
        st[(2 * D + 1) * D + lane] = 0.0;
    }
}

// mono := M mono;  Z = M Qmat, Qmat := the orthonormal columns of Z by modified Gram-Schmidt in column order (column c is
// normalised, then taken out of every later column), sum c += log |r_cc|.  Wave 0 only, all of its 64 lanes (the broadcasts).
// UNROLL_SWEEP: the sweep over c as D copies (the sectioned map, whose kernel has the registers) or as a loop (the d-pair map:
// c only selects the lane, and D copies of the sweep cost registers that its D = 6 instances do not have).
template <int D, bool UNROLL_SWEEP>
__device__ __forceinline__ void maptan_advance()
{
    if (threadIdx.x >= 64) return;
    double *st = maptan_state<D>();
    const double *M = st + maptan_m_at<D>();
    const int lane = threadIdx.x;
    constexpr int SWEEP = UNROLL_SWEEP ? D : 1;                 // copies of the Gram-Schmidt sweep below
    double mo[D], qv[D], mn[D], mc[D], lm = 1.0, le = 0.0;      // the owner's columns of mono and Qmat; their images under M
#pragma unroll
    for (int r = 0; r < D; ++r) { mo[r] = 0.0; qv[r] = 0.0; }
    if (lane < D) {
#pragma unroll
        for (int r = 0; r < D; ++r) { mo[r] = st[r * D + lane]; qv[r] = st[(D + r) * D + lane]; }
        lm = st[2 * D * D + lane];
        le = st[(2 * D + 1) * D + lane];
    }
#pragma unroll
    for (int r = 0; r < D; ++r) {
        double v = 0.0, w = 0.0;
#pragma unroll
        for (int s = 0; s < D; ++s) { v = __builtin_fma(M[r * D + s], mo[s], v); w = __builtin_fma(M[r * D + s], qv[s], w); }
        mn[r] = v;
        mc[r] = w;                         // column `lane` of Z
    }
#pragma unroll SWEEP
    for (int c = 0; c < D; ++c) {
        double n2 = 0.0;
#pragma unroll
        for (int r = 0; r < D; ++r) n2 = __builtin_fma(mc[r], mc[r], n2);
        const double nrm = __builtin_sqrt(n2);
        const double rcc = __shfl(nrm, c, 64), inv = 1.0 / rcc;
        double qc[D], dot = 0.0;
#pragma unroll
        for (int r = 0; r < D; ++r) {
            qc[r] = __shfl(mc[r], c, 64) * inv;
            dot = __builtin_fma(qc[r], mc[r], dot);
        }
        if (lane == c) {
            int e1, e2;
            lm *= 2.0 * __builtin_frexp(rcc, &e1);     // both factors in [1, 2): the product is below 4
            lm = 2.0 * __builtin_frexp(lm, &e2);
            le += (double)(e1 + e2 - 2);
        }
#pragma unroll
        for (int r = 0; r < D; ++r) mc[r] = (lane == c) ? qc[r] : (lane > c ? __builtin_fma(-dot, qc[r], mc[r]) : mc[r]);
    }
    if (lane < D) {
#pragma unroll
        for (int r = 0; r < D; ++r) { st[r * D + lane] = mn[r]; st[(D + r) * D + lane] = mc[r]; }
        st[2 * D * D + lane] = lm;
        st[(2 * D + 1) * D + lane] = le;
    }
}

// mono := M mono alone, for a caller that wants neither Qmat nor the sums (the periodic-orbit search): the owners' columns, the
// FMA chain of maptan_advance in its order, so mono has the bits the TAN instances give it
template <int D>
__device__ __forceinline__ void maptan_advance_mono()
{
    if (threadIdx.x >= D) return;
    double *st = maptan_state<D>();
    const double *M = st + maptan_m_at<D>();
    const int lane = threadIdx.x;
    double mo[D], mn[D];
#pragma unroll
    for (int r = 0; r < D; ++r) mo[r] = st[r * D + lane];
#pragma unroll
    for (int r = 0; r < D; ++r) {
        double v = 0.0;
#pragma unroll
        for (int s = 0; s < D; ++s) v = __builtin_fma(M[r * D + s], mo[s], v);
        mn[r] = v;
    }
#pragma unroll
    for (int r = 0; r < D; ++r) st[r * D + lane] = mn[r];
}

// orbit k's mono [ntest][D][D] (column by column) and exponents lyap [ntest][D] over nm - 1 steps, by their owners; each or null
template <int D>
__device__ __forceinline__ void maptan_finish(double *mono, double *lyap, int nm, int k)
{
    const double *st = maptan_state<D>();
    const int lane = threadIdx.x;
    if (lane < D) {
        if (mono) {
#pragma unroll
            for (int r = 0; r < D; ++r) mono[((size_t)k * D + r) * D + lane] = st[r * D + lane];
        }
        if (lyap) {
            const double sum = __builtin_fma(st[(2 * D + 1) * D + lane], 0.693147180559945309417, log(st[2 * D * D + lane]));
            lyap[(size_t)k * D + lane] = nm > 1 ? sum / (double)(nm - 1) : 0.0;
        }
    }
}
