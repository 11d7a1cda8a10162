// periodic_nd.h -- periodic orbits of the d-pair symplectic map: Newton on the n-fold map, every pass of one guess inside one
// workgroup of one launch.
//
// Included by map_nd.hip INSIDE its anonymous namespace, after mapnd_step (the step of applymap_nd_kernel, called here as it is
// called there), maptan.h (the Hessian pass) and tangent_core.h (the step matrix, the monodromy product); map_nd.hip is its
// only includer.
//
// A guess z = (q, p) with period n and winding numbers w (d integers) is a periodic orbit when
//     r(z) = ( q_n - q_0 - 2 pi w,  p_n - p_0 ) = 0,        (q_n, p_n) the n-th image of z in lifted (unwrapped) coordinates.
// One pass runs the n steps from z with the tangent map: mono = M_n ... M_1 is dr/dz + I.  Plain Newton, no damping:
//     z <- z - (mono - I)^-1 r(z).
// Converged: the pass that STARTED from z has max|r| <= tol max(1, max|z|); that z is returned with the residual, the orbit
// and the monodromy evaluated there.  Failed (NaN in every floating output, its = -1): maxit passes without convergence, a
// lost orbit (mapnd_step's rule; a guess that starts non-finite is one), a step whose I + B is singular, a singular mono - I
// (a zero or non-finite pivot) or an update that is not finite.
// Winding: with SGPR_MAP_WRAP_Q the step takes floor(Q / 2 pi) turns out of every Q; they are counted per coordinate and the
// q-residual is (Q_n - q_0) + 2 pi (turns - w), the small difference first.  Without the wrap it is Q_n - q_0 - 2 pi w: a
// periodic family run unwrapped is a legitimate lifted map.  With the wrap every updated q_0 is wrapped into [0, 2 pi).
// What lives across the step loop is in LDS, not in registers (the D = 6, 512-thread passes leave none): z_0, the turn counts
// (periodic_state) and mono (maptan_state, advanced by maptan_advance_mono: no Benettin sums, no per-step jac).
#pragma once

struct PeriodicNdArgs : MapNdArgs {    // nm = the period n; qmap / pmap = the orbit [n][ntest][d] or both null; iters unused
    const int *wind;                   // ntest x d, column-major, leading dimension ntest, or null (all 0)
    double ptol;                       // the outer Newton's tol and maxit (tol, maxiter are the step's own)
    int pmaxit;
    double *z;                         // [ntest][D]
    double *resid;                     // [ntest]
    int *its;                          // [ntest]
    double *mono;                      // [ntest][D][D] or null
};

// z_0 (D), the point the next step starts from (D), the turn counts and the winding numbers (d each, integers held as doubles)
// and the verdict of the last solve (1 entry: 0 = the update is good)
template <int D>
__device__ __forceinline__ double *periodic_state()
{
    __shared__ double ps[3 * D + 1];
    return ps;
}

// delta := (mono - I)^-1 (-r) by Gaussian elimination with partial pivoting (mono - I is not diagonally dominant).  Wave 0
// only, all of its 64 lanes (the broadcasts): lane c < D owns column c of mono - I, read from maptan_state where the same lane
// keeps its column of mono, lane D the right-hand side.  Every row operation is one instruction over the columns; the pivot
// column is broadcast first, so the pivot row and the multipliers are the same in every lane.  The first largest |entry| of
// the column at or below the diagonal is the pivot; a NaN there is never chosen and ends in a non-finite delta, which the caller
// refuses.  false: a zero or non-finite pivot.
template <int D>
__device__ __forceinline__ bool periodic_solve(const double (&r)[D], double (&delta)[D])
{
    const double *st = maptan_state<D>();
    const int lane = threadIdx.x;
    double a[D];
#pragma unroll
    for (int i = 0; i < D; ++i) a[i] = 0.0;
    if (lane < D) {
#pragma unroll
        for (int i = 0; i < D; ++i) a[i] = st[i * D + lane] - (i == lane ? 1.0 : 0.0);
    } else if (lane == D) {
#pragma unroll
        for (int i = 0; i < D; ++i) a[i] = -r[i];
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        double col[D];
#pragma unroll
        for (int i = k; i < D; ++i) col[i] = __shfl(a[i], k, 64);
        int piv = k;
        double big = fabs(col[k]);
#pragma unroll
        for (int i = k + 1; i < D; ++i) {
            const double v = fabs(col[i]);
            if (v > big) { big = v; piv = i; }
        }
#pragma unroll
        for (int i = k + 1; i < D; ++i) {               // rows k and piv change places
            if (piv == i) {
                double t = a[k]; a[k] = a[i]; a[i] = t;
                t = col[k]; col[k] = col[i]; col[i] = t;
            }
        }
        ok = ok && finite_d(col[k]) && col[k] != 0.0;
#pragma unroll
        for (int i = k + 1; i < D; ++i) a[i] = __builtin_fma(-(col[i] / col[k]), a[k], a[i]);
    }
#pragma unroll
    for (int k = D - 1; k >= 0; --k) {                  // back substitution: the arithmetic is lane D's, the broadcasts everyone's
        const double xk = a[k] / __shfl(a[k], k, 64);
        if (lane == D) a[k] = xk;
#pragma unroll
        for (int i = 0; i < k; ++i) {
            const double u = __shfl(a[i], k, 64);
            if (lane == D) a[i] = __builtin_fma(-u, xk, a[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < D; ++i) delta[i] = __shfl(a[i], D, 64);
    return ok;
}

// One workgroup per guess runs every Newton pass of that guess; nothing waits on another workgroup, and a guess's bits depend
// on nothing but its own inputs (TT is chosen from n0 alone).  Staging, TT and the seq alternation of the workgroup sums are
// those of applymap_nd_kernel.  A pass is the TAN = true step loop of that kernel without jac and the Benettin step: mapnd_step,
// the Hessian pass, the step matrix, mono := M mono.  Thread 0 writes the orbit rows as the pass goes: the last pass run is
// the one whose start point is returned.  Everything that decides the control flow is block-uniform.
template <int FAM, int D, int TT>
__global__ __launch_bounds__(TT) void periodic_nd_kernel(const PeriodicNdArgs a)
{
    constexpr int d = D / 2, W = TT / 64, NSMAX = maptan_max_sums<FAM, D, TT>();
    constexpr bool HAS_STAGE = TT == MAPND_T_SMALL;
    __shared__ double part[2][W * NSMAX];
    __shared__ double res[2][NSMAX];
    __shared__ double stage[HAS_STAGE ? 2 * D * MAPND_STAGE_PTS : 1];
    const int k = blockIdx.x, n0 = a.k.mj;
    stage_ptr stg = nullptr;
    if (HAS_STAGE && n0 <= MAPND_STAGE_PTS) {               // as applymap_nd_kernel: every thread reads back what it wrote itself
        for (int j = threadIdx.x; j < n0; j += TT) {
#pragma unroll
            for (int c = 0; c < D; ++c) {
                stage[c * MAPND_STAGE_PTS + j] = a.k.Xa[(size_t)j + (size_t)c * a.k.ldxa];
                stage[(D + c) * MAPND_STAGE_PTS + j] = a.alpha[(size_t)c * n0 + j];
            }
        }
        stg = (stage_ptr)stage;
    }
    double *z0 = periodic_state<D>(), *cur = z0 + D, *turns = z0 + 2 * D, *wind = turns + d, *verdict = z0 + 3 * D;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < d; ++c) {
            z0[c] = cur[c] = a.Q0[(size_t)k + (size_t)c * a.ntest];
            z0[d + c] = cur[d + c] = a.P0[(size_t)k + (size_t)c * a.ntest];
            wind[c] = a.wind ? (double)a.wind[(size_t)k + (size_t)c * a.ntest] : 0.0;
        }
    }
    __syncthreads();
    const double nan = __builtin_nan("");
    const double twopi = 6.283185307179586477;
    const bool wrap = a.mode & SGPR_MAP_WRAP_Q;
    unsigned seq = 0;
    int passes = 0;
    bool converged = false;
#pragma nounroll
    while (passes < a.pmaxit) {
        if (threadIdx.x == 0) {
#pragma unroll
            for (int c = 0; c < d; ++c) turns[c] = 0.0;
        }
        maptan_init<D>();
        bool good = true;
#pragma nounroll
        for (int i = 0; i < a.nm; ++i) {
            double q[d], p[d];                              // thread 0 wrote them ahead of a barrier: the solve's, or the step's
#pragma unroll
            for (int c = 0; c < d; ++c) { q[c] = cur[c]; p[c] = cur[d + c]; }
            if (threadIdx.x == 0 && a.qmap) {
                const size_t o = ((size_t)i * a.ntest + k) * d;
#pragma unroll
                for (int c = 0; c < d; ++c) { a.qmap[o + c] = q[c]; a.pmap[o + c] = p[c]; }
            }
            int its;
            double x[D], M[D * D];
            {                                               // nothing but x lives across the Hessian pass: the image goes to LDS
                double P[d], Q[d], turn[d];                 // (every thread has read the old one: the step's passes have barriers)
                good = mapnd_step<FAM, D, TT>(a, stg, q, p, x, Q, P, turn, its, seq, part, res);
                if (!good) break;
                if (threadIdx.x == 0) {
#pragma unroll
                    for (int c = 0; c < d; ++c) { cur[c] = Q[c]; cur[d + c] = P[c]; turns[c] += turn[c]; }
                }
            }
            double H[D * (D + 1) / 2];                      // x is (q, P) of the accepted step
            maptan_hessian<FAM, D, TT>(a, x, stg, H, &part[0][0], &res[0][0], W * NSMAX, NSMAX, seq);
            good = maptan_matrix<D>(H, M);
            if (!good) break;
            maptan_publish<D>(M, nullptr);                  // its barrier is also the one behind the image and the turn counts
            maptan_advance_mono<D>();
        }
        ++passes;
        if (!good) break;
        double r[D], rmax = 0.0, zmax = 1.0;
#pragma unroll
        for (int c = 0; c < d; ++c) {
            r[c] = wrap ? (cur[c] - z0[c]) + twopi * (turns[c] - wind[c]) : cur[c] - z0[c] - twopi * wind[c];
            r[d + c] = cur[d + c] - z0[d + c];
        }
#pragma unroll
        for (int c = 0; c < D; ++c) {
            good = good && finite_d(r[c]);
            rmax = fmax(rmax, fabs(r[c]));
            zmax = fmax(zmax, fabs(z0[c]));
        }
        if (!good) break;
        if (rmax <= a.ptol * zmax) {                        // z_0 is the answer: the residual is the one evaluated there
            if (threadIdx.x == 0) {
#pragma unroll
                for (int c = 0; c < D; ++c) a.z[(size_t)k * D + c] = z0[c];
                a.resid[k] = rmax;
                a.its[k] = passes;
            }
            converged = true;
            break;
        }
        if (passes == a.pmaxit) break;
        __syncthreads();                                    // every thread has read z_0, the image and the turn counts
        if (threadIdx.x < 64) {
            double delta[D], zn[D];
            bool ok = periodic_solve<D>(r, delta);
#pragma unroll
            for (int c = 0; c < D; ++c) {
                zn[c] = z0[c] + delta[c];
                ok = ok && finite_d(zn[c]);
                if (wrap && c < d) zn[c] -= twopi * floor(zn[c] / twopi);
            }
            if (threadIdx.x == 0) {
#pragma unroll
                for (int c = 0; c < D; ++c) z0[c] = cur[c] = zn[c];
                *verdict = ok ? 0.0 : 1.0;
            }
        }
        __syncthreads();
        if (*verdict != 0.0) break;
    }
    if (converged) {
        maptan_finish<D>(a.mono, nullptr, a.nm + 1, k);
        return;
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < D; ++c) a.z[(size_t)k * D + c] = nan;
        a.resid[k] = nan;
        a.its[k] = -1;
        if (a.qmap) {
            for (int i = 0; i < a.nm; ++i) {
                const size_t o = ((size_t)i * a.ntest + k) * d;
#pragma unroll
                for (int c = 0; c < d; ++c) { a.qmap[o + c] = nan; a.pmap[o + c] = nan; }
            }
        }
    }
    if (threadIdx.x < D && a.mono) {
#pragma unroll
        for (int i = 0; i < D; ++i) a.mono[((size_t)k * D + i) * D + threadIdx.x] = nan;
    }
}
