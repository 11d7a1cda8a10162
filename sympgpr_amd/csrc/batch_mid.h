// batch_mid.h -- device code of the batched fits of order 256 < n <= 2048: build, the rank-k update between two panels, the
// solves' ends, and the Ky^-1, gradient, leave-one-point-out and loo gradient phases.  Included only by batch.hip, behind batch_small.h.
#pragma once

namespace sgpr {

namespace {

// ---- mid-size problems: 256 < n <= 2048 (a CMA-ES generation at N = 512 ... 1024 points) --------------------------
// Three launches for the whole batch: (1) every Ky_b, lower triangle, into an npad x npad image (npad = n rounded up to
// 128; the padding is an identity block: det 1, alpha 0 there); (2) panel.hip's panel_batch_kernel: W = npad / 128
// workgroups per problem run the leaf chain on their own matrix, problems side by side; (3) one workgroup per problem:
// y = L^-1 z and alpha = L^-T y through the leaf inverses, and the negative log-likelihood.
constexpr int MT = 256;                   // build: pair rows per tile (one per thread)
constexpr int MJ = 16;                    // build: pair columns per tile
constexpr int ST = 512;                   // solve: threads per problem

struct MidArgs {
    int nbatch, npts, n, npad, reg;
    const double *x, *y, *z;              // nbatch x npts, nbatch x npts, nbatch x n
    const KConst *kc;
    const double *noise;
    double *A;                            // problem b at A + b * npad * npad, ld = npad
    const double *inv;                    // leaf inverses: problem b at inv + b * (npad / 128) * 128 * 128
    double *alpha, *nll;
    const int *info;
};

template <int FAM>
__global__ __launch_bounds__(MT) void mid_build_kernel(const MidArgs a)
{
    __shared__ double sx[MJ], sy[MJ];
    const int b = blockIdx.z, N = a.npts, t = threadIdx.x;
    const int i0 = blockIdx.x * MT, j0 = blockIdx.y * MJ;
    const size_t ld = (size_t)a.npad;
    double *A = a.A + (size_t)b * ld * ld;
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (int r = a.n + t; r < a.npad; r += MT) A[r + r * ld] = 1.0;     // the padding's diagonal (the rest was cleared)
    const bool tile_lower = i0 + MT - 1 >= j0;        // some (i, j) of the tile has i >= j
    if (a.reg && !tile_lower) return;
    const double *x = a.x + (size_t)b * N, *y = a.y + (size_t)b * N;
    const int nj = min(MJ, N - j0);
    if (t < nj) { sx[t] = x[j0 + t]; sy[t] = y[j0 + t]; }
    __syncthreads();
    const int i = i0 + t;
    if (i >= N) return;
    const KConst kc = a.kc[b];
    const double noise = a.noise[b];
    const double xi = x[i], yi = y[i];
    if (a.reg) {
        for (int jj = 0; jj < nj; ++jj) {
            const int j = j0 + jj;
            if (i < j) break;
            double k = kc.sig * kern_eval<FAM, false>(sx[jj], sy[jj], xi, yi, kc);
            if (i == j) k += noise;
            A[i + j * ld] = k;
        }
        return;
    }
    for (int jj = 0; jj < nj; ++jj) {
        const int j = j0 + jj;
        double kxx, kxy, kyy;
        pair_eval<FAM, false>(sx[jj], sy[jj], xi, yi, kc, kxx, kxy, kyy);
        if (i == j) { kxx += noise; kyy += noise; }
        A[(N + i) + j * ld] = kxy;                     // Pq block: always below the diagonal
        if (i >= j) {
            A[i + j * ld] = kxx;
            A[(N + i) + (N + j) * ld] = kyy;
        }
    }
}

// The build for d canonical pairs per point (D = 2 d, n = D N): mid_build_kernel's tiling -- MT point rows per workgroup, one per
// thread, MJ point columns in LDS, now D coordinates each, blockIdx.z the problem -- and fit_batch_nd_kernel's entries and
// lower-triangle rule (store_pair_lower) at ld = npad.
struct MidNdArgs {
    int npts, n, npad;
    const double *X;                      // nbatch x D x npts
    const nd::NdConst *nc;
    const double *noise;
    double *A;                            // problem b at A + b * npad * npad, ld = npad
};

template <int FAM, int D>
__global__ __launch_bounds__(MT) void mid_build_nd_kernel(const MidNdArgs a)
{
    __shared__ double sxa[MJ][D];
    const int b = blockIdx.z, N = a.npts, t = threadIdx.x;
    const int i0 = blockIdx.x * MT, j0 = blockIdx.y * MJ;
    const size_t ld = (size_t)a.npad;
    double *A = a.A + (size_t)b * ld * ld;
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (int r = a.n + t; r < a.npad; r += MT) A[r + r * ld] = 1.0;     // the padding's diagonal (the rest was cleared)
    const double *X = a.X + (size_t)b * D * N;
    const int nj = min(MJ, N - j0);
    for (int e = t; e < nj * D; e += MT) sxa[e / D][e % D] = X[(size_t)(e % D) * N + j0 + e / D];
    __syncthreads();
    const int i = i0 + t;
    if (i >= N) return;
    const nd::NdConst nc = a.nc[b];
    const double noise = a.noise[b];
    double xb[D];
#pragma unroll
    for (int m = 0; m < D; ++m) xb[m] = X[(size_t)m * N + i];
    for (int jj = 0; jj < nj; ++jj) {
        const int j = j0 + jj;
        double arg[D], g[D], nh[D], E[D];
        nd::all_coords<FAM, D>(nc, sxa[jj], xb, arg, g, nh);
        nd::weights<FAM, D>(nc, arg, E);
        store_pair_lower<FAM, D>(A + i + (size_t)j * ld, ld, N, i >= j, i == j, noise, E, g, nh);
    }
}

// Above order 1024 a problem is factored as two panels; between them, for every problem, the rank-k update of the block that
// is left: A22 -= L21 L21^T (lower tiles only), 128 x 128 tiles of the grid-wide MFMA kernel's LDS-DMA body (gemm_tile.h).
struct MidSyrk {
    double *A;            // problem b at A + b * stride (column-major, ld)
    size_t stride, ld;
    int k, m2;            // width of the first panel; order of the block behind it (multiples of 128)
};

__global__ __launch_bounds__(256, 2) void mid_syrk_kernel(const MidSyrk a)
{
    __shared__ double smem[2 * tile::BK * (2 * (128 + tile::PAD))];
    int t = (int)blockIdx.x, r = 0;            // lower tiles row by row: row r holds r + 1 of them
    while (t > r) { t -= r + 1; ++r; }
    double *base = a.A + (size_t)blockIdx.y * a.stride;
    tile::GemmArgs g{};
    g.m = a.m2; g.n = a.m2; g.k = a.k;
    g.alpha = -1.0; g.beta = 1.0;
    g.A = base + a.k; g.lda = a.ld;
    g.B = base + a.k; g.ldb = a.ld;
    g.C = base + a.k + (size_t)a.k * a.ld; g.ldc = a.ld;
    tile::gemm_body_dma<128, 128, 2>(g, smem, r, t);
}

__device__ __forceinline__ double wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;      // lane 0 holds the sum
}

// The solves of the batch: the right-hand sides padded to npad ...
__global__ __launch_bounds__(256) void mid_rhs_kernel(const MidArgs a, double *r)
{
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i < a.npad) r[(size_t)b * a.npad + i] = i < a.n ? a.z[(size_t)b * a.n + i] : 0.0;
}
// ... two launches of trsv.hip's strip solve over all problems (one workgroup per 128-row strip and problem, W x nbatch of
// them; round 3 ran both solves of a problem in ONE workgroup: 64 problems of order 1024 kept 64 CUs busy for 0.6 ms, a third
// of the whole call) ... and, per problem, nll = z.alpha / 2 + sum log L_ii (func.py:195) and alpha.
__global__ __launch_bounds__(ST) void mid_finish_kernel(const MidArgs a, const double *r, const int *state, int *info)
{
    __shared__ double red[ST / 64];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = a.n;
    const size_t ld = (size_t)a.npad;
    const double *A = a.A + (size_t)b * ld * ld;
    const double *z = a.z + (size_t)b * n;
    const double *al = r + (size_t)b * ld;
    // a strip solve that gave up on a hand-off (state word 2 of either pass): an error of the call, not a result
    if (a.info[b] == 0 && (state[8 * b + 2] | state[8 * b + 6]) != 0) {
        if (t == 0) { info[b] = SOLVE_HANDOFF_TIMEOUT; a.nll[b] = __builtin_nan(""); }
        return;
    }
    if (a.info[b] != 0) {                  // not positive definite: the host turns info into NaN / +inf
        if (t == 0) a.nll[b] = __builtin_nan("");
        if (a.alpha)
            for (int i = t; i < n; i += ST) a.alpha[(size_t)b * n + i] = __builtin_nan("");
        return;
    }
    double q = 0.0;
    for (int i = t; i < n; i += ST) q += 0.5 * z[i] * al[i] + log(A[i + i * ld]);
    q = wave_sum(q);
    if (lane == 0) red[wave] = q;
    __syncthreads();
    if (t == 0) {
        double v = 0.0;
        for (int w = 0; w < ST / 64; ++w) v += red[w];
        a.nll[b] = v;
    }
    if (a.alpha)
        for (int i = t; i < n; i += ST) a.alpha[(size_t)b * n + i] = al[i];
}

// ---- the gradient of the mid-size problems (sgpr_fit_batch_grad_mid) -------------------------------------------------
// After the solves a problem's image holds L, `inv` its 128 x 128 leaf inverses and r its alpha.  Three steps, every one a
// grid over all problems of the chunk, ordered by the stream alone (no workgroup waits for another one):
//   (a) U = L^-T into a second image, U[i + k ld] = (L^-1)[k, i] as grad_problem's: the diagonal tiles are the transposed
//       leaf inverses (mid_udiag_kernel); then the block size doubles, 128, 256, ... : for adjacent diagonal blocks 1, 2
//           T = U11 L21^T   (STEP 0, NT, into the block (1, 2) of the L image: its strict upper triangle is free),
//           U12 = -T U22    (STEP 1, the TRANSB form),
//       one 128 x 128 tile per workgroup; the last block 2 is ragged when W is no power of two.  The k range of a tile stops
//       at the zeros of the triangular operand: U11's tile row ti starts at k = 128 ti, U22's tile column tj ends at
//       128 (tj + 1).
//   (b) Ky^-1 = U U^T, lower tiles, over L (mid_kinv_kernel): tile (I, J) sums k >= 128 I.
//   (c) the contraction of W = Ky^-1 - alpha alpha^T with dK (mid_grad_kernel) in per-workgroup partials, folded per problem in
//       a fixed order (mid_grad_fold_kernel).
// A problem that is not positive definite has an arbitrary image: every loop bound here comes from the shape alone.
constexpr int GT = 256;                   // contraction: rows per workgroup (one per thread)
constexpr int GCJ = 64;                   // contraction: column points per workgroup
constexpr int GPART = 8;                  // doubles per workgroup partial (>= grad_nacc)
constexpr int GPART_ND = 16;              // the same for d canonical pairs per point (>= grad_nacc_nd: 11 at d = 3 with periods)

struct MidInv {
    double *L, *U;        // problem b at L / U + b * stride (column-major, ld)
    const double *inv;    // its leaf inverses at inv + b * stride_inv
    size_t stride, ld, stride_inv;
    int W, S;             // 128-tiles per side; tiles per side of a (full) diagonal block of this level
};

__global__ __launch_bounds__(256) void mid_udiag_kernel(const MidInv a)
{
    const double *X = a.inv + (size_t)blockIdx.y * a.stride_inv + (size_t)blockIdx.x * LEAF * LEAF;
    double *U = a.U + (size_t)blockIdx.y * a.stride + (size_t)blockIdx.x * LEAF * (a.ld + 1);
    for (int e = threadIdx.x; e < (int)(LEAF * LEAF); e += 256) {
        const int i = e % (int)LEAF, k = e / (int)LEAF;
        U[i + k * a.ld] = k >= i ? X[k + i * LEAF] : 0.0;         // the tile's lower part: zeros that (b) reads
    }
}

template <int STEP>
__global__ __launch_bounds__(256, 2) void mid_inv_level_kernel(const MidInv a)
{
    __shared__ double smem[2 * tile::BK * (2 * (128 + tile::PAD))];
    const int S = a.S, per = S * S;
    const int p = (int)blockIdx.x / per, rem = (int)blockIdx.x - p * per, ti = rem % S, tj = rem / S;
    const int t1 = 2 * S * p, t2 = t1 + S;            // first tile of block 1 (S tiles, full) and of block 2
    if (t2 + tj >= a.W) return;                       // past the ragged last block (the whole workgroup)
    double *L = a.L + (size_t)blockIdx.y * a.stride, *U = a.U + (size_t)blockIdx.y * a.stride;
    const size_t ld = a.ld, r1 = (size_t)t1 * LEAF, r2 = (size_t)t2 * LEAF, ri = r1 + (size_t)ti * LEAF, cj = r2 + (size_t)tj * LEAF;
    tile::GemmArgs g{};
    g.m = 128; g.n = 128; g.beta = 0.0;
    g.lda = ld; g.ldb = ld; g.ldc = ld;
    if constexpr (STEP == 0) {
        // T(ti, tj) = sum_{k >= 128 ti} U11[ti, k] L21[tj, k]
        g.k = (S - ti) * (int)LEAF; g.alpha = 1.0;
        g.A = U + ri + ri * ld;
        g.B = L + cj + ri * ld;
        g.C = L + ri + cj * ld;
        tile::gemm_body_dma<128, 128, 2>(g, smem, 0, 0);
    } else {
        // U12(ti, tj) = -sum_{k < 128 (tj + 1)} T[ti, k] U22[k, tj]
        g.k = (tj + 1) * (int)LEAF; g.alpha = -1.0; g.transb = 1;
        g.A = L + ri + r2 * ld;
        g.B = U + r2 + cj * ld;
        g.C = U + ri + cj * ld;
        tile::gemm_body<128, 128, true, true>(g, smem, 0, 0);
    }
}

__global__ __launch_bounds__(256, 2) void mid_kinv_kernel(const MidInv a)
{
    __shared__ double smem[2 * tile::BK * (2 * (128 + tile::PAD))];
    int t = (int)blockIdx.x, r = 0;            // lower tiles row by row, as mid_syrk_kernel
    while (t > r) { t -= r + 1; ++r; }
    const double *U = a.U + (size_t)blockIdx.y * a.stride;
    const size_t ld = a.ld, ri = (size_t)r * LEAF, cj = (size_t)t * LEAF;
    tile::GemmArgs g{};
    g.m = 128; g.n = 128; g.k = (a.W - r) * (int)LEAF;
    g.alpha = 1.0; g.beta = 0.0;
    g.A = U + ri + ri * ld; g.lda = ld;        // U[I, k] = 0 for k < 128 I
    g.B = U + cj + ri * ld; g.ldb = ld;
    g.C = a.L + (size_t)blockIdx.y * a.stride + ri + cj * ld; g.ldc = ld;
    tile::gemm_body_dma<128, 128, 2>(g, smem, 0, 0);
}

struct MidGrad {
    int npts, n, reg, nwg, nacc, gpart;   // gpart: doubles per partial (GPART; GPART_ND behind mid_grad_nd_kernel)
    size_t ld;                            // npad: Ky^-1 (lower) of problem b at K + b ld^2, its alpha at alpha + b ld
    const double *x, *y;
    const KConst *kc;
    const double *K, *alpha;
    double *part;                         // sum k of workgroup w of problem b at part[(b nwg + w) gpart + k]
    const int *info;
    double *out;                          // problem b's raw sums at out + b nacc
};

// rows i0 .. i0 + GT (one per thread) x column points p0 .. p0 + GCJ of problem blockIdx.z: entries on and below the diagonal,
// weighted W_ii and 2 W_ij, as grad_problem's step (3); rows and columns below n only
template <int FAM>
__global__ __launch_bounds__(GT) void mid_grad_kernel(const MidGrad a)
{
    constexpr bool HASP = grad_has_p<FAM>();
    constexpr int NACC = grad_nacc<FAM>();
    __shared__ double sx[GCJ], sy[GCJ], sal[2][GCJ];
    __shared__ double red[GT / 64][NACC];
    const int b = blockIdx.z, N = a.npts, n = a.n, tid = threadIdx.x;
    const int p0 = blockIdx.y * GCJ, np = min(GCJ, N - p0);
    const int i = blockIdx.x * GT + tid;
    const double *K = a.K + (size_t)b * a.ld * a.ld, *al = a.alpha + (size_t)b * a.ld;
    if (tid < np) {
        sx[tid] = a.x[(size_t)b * N + p0 + tid];
        sy[tid] = a.y[(size_t)b * N + p0 + tid];
        sal[0][tid] = al[p0 + tid];
        sal[1][tid] = a.reg ? 0.0 : al[N + p0 + tid];
    }
    __syncthreads();
    const KConst kc = a.kc[b];
    const double l[2] = {kc.lx, kc.ly}, pp[1] = {kc.p};
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    if (i < n && p0 <= i) {
        const double ai = al[i];
        const double *Krow = K + i;
        if (a.reg) {
            const double xi = a.x[(size_t)b * N + i], yi = a.y[(size_t)b * N + i];
            for (int jj = 0; jj < np; ++jj) {
                const int j = p0 + jj;
                if (j > i) break;
                const double W = Krow[(size_t)j * a.ld] - ai * sal[0][jj];
                if (j == i) acc[NACC - 1] += W;
                nllg::reg_grad<FAM, HASP>(sx[jj], sy[jj], xi, yi, j == i ? W : 2.0 * W, l, kc.p, acc);
            }
        } else {
            const int r = i < N ? 0 : 1, pi = i - r * N;
            const double xi[2] = {a.x[(size_t)b * N + pi], a.y[(size_t)b * N + pi]};
            for (int jj = 0; jj < np; ++jj) {
                const int pj = p0 + jj;
                double w[2];
                bool any = false;
#pragma unroll
                for (int c = 0; c < 2; ++c) {                 // columns pj (q part) and N + pj (P part)
                    const int col = c * N + pj;
                    w[c] = 0.0;
                    if (col <= i) {
                        const double W = Krow[(size_t)col * a.ld] - ai * sal[c][jj];
                        if (col == i) { w[c] = W; acc[NACC - 1] += W; }
                        else w[c] = 2.0 * W;
                        any = true;
                    }
                }
                if (!any) break;                              // column pj > i: so are all after it
                const double xj[2] = {sx[jj], sy[jj]};
                nllg::pair_grad<FAM, 2, HASP>(xi, xj, w, r, l, pp, acc);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        const double v = wave_sum(acc[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < NACC) {
        double v = red[0][tid];
#pragma unroll
        for (int w = 1; w < GT / 64; ++w) v += red[w][tid];
        a.part[((size_t)b * a.nwg + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * GPART + tid] = v;
    }
}

// The contraction for d canonical pairs per point (D = 2 d, n = D N): mid_grad_kernel's grid and tiling -- GT rows per workgroup,
// one per thread, GCJ column points in LDS, now D coordinates and D alpha entries each, blockIdx.z the problem -- and
// contract_rows_nd's rows (row i is part r = i / N of point i % N), weights and stop.  NACC = grad_nacc_nd (up to 11) sums per
// workgroup, GPART_ND doubles apart; mid_grad_fold_kernel sums them (MidGrad::gpart).
struct MidGradNd {
    int npts, n, nwg;
    size_t ld;                            // npad: Ky^-1 (lower) of problem b at K + b ld^2, its alpha at alpha + b ld
    const double *X;                      // nbatch x D x npts
    const nd::NdConst *nc;
    const double *K, *alpha;
    double *part;                         // sum k of workgroup w of problem b at part[(b nwg + w) GPART_ND + k]
};

template <int FAM, int D>
__global__ __launch_bounds__(GT) void mid_grad_nd_kernel(const MidGradNd a)
{
    constexpr bool HASP = grad_has_p<FAM>();
    constexpr int NACC = grad_nacc_nd<FAM, D>(), d = D / 2;
    static_assert(NACC <= GPART_ND, "a workgroup's sums fit in its partial");
    __shared__ double sxa[GCJ][D], sal[D][GCJ];
    __shared__ double red[GT / 64][NACC];
    const int b = blockIdx.z, N = a.npts, n = a.n, tid = threadIdx.x;
    const int p0 = blockIdx.y * GCJ, np = min(GCJ, N - p0);
    const int i = blockIdx.x * GT + tid;
    const double *X = a.X + (size_t)b * D * N;
    const double *K = a.K + (size_t)b * a.ld * a.ld, *al = a.alpha + (size_t)b * a.ld;
    for (int e = tid; e < np * D; e += GT) {
        const int jj = e % np, m = e / np;
        sxa[jj][m] = X[(size_t)m * N + p0 + jj];
        sal[m][jj] = al[(size_t)m * N + p0 + jj];
    }
    __syncthreads();
    const nd::NdConst nc = a.nc[b];
    double l[D], pp[d];
#pragma unroll
    for (int m = 0; m < D; ++m) l[m] = nc.l[m];
#pragma unroll
    for (int m = 0; m < d; ++m) pp[m] = HASP ? nc.hs[m] : 0.0;
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    if (i < n && p0 <= i) {
        const int r = i / N, pi = i - r * N;
        const double ai = al[i];
        const double *Krow = K + i;
        double xi[D];
#pragma unroll
        for (int m = 0; m < D; ++m) xi[m] = X[(size_t)m * N + pi];
        for (int jj = 0; jj < np; ++jj) {
            const int pj = p0 + jj;
            if (pj > i) break;                                // column pj > i: so are all after it
            double w[D], xj[D];
#pragma unroll
            for (int c = 0; c < D; ++c) {                     // column c N + pj: part c of the column point
                const int col = c * N + pj;
                w[c] = 0.0;
                if (col <= i) {
                    const double W = Krow[(size_t)col * a.ld] - ai * sal[c][jj];
                    if (col == i) { w[c] = W; acc[NACC - 1] += W; }
                    else w[c] = 2.0 * W;
                }
            }
#pragma unroll
            for (int m = 0; m < D; ++m) xj[m] = sxa[jj][m];
            nllg::pair_grad<FAM, D, HASP>(xi, xj, w, r, l, pp, acc);
        }
    }
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        const double v = wave_sum(acc[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < NACC) {
        double v = red[0][tid];
#pragma unroll
        for (int w = 1; w < GT / 64; ++w) v += red[w][tid];
        a.part[((size_t)b * a.nwg + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * GPART_ND + tid] = v;
    }
}

// problem blockIdx.x: its workgroups' partials in their fixed order; NaN where the factorisation failed
__global__ __launch_bounds__(64) void mid_grad_fold_kernel(const MidGrad a)
{
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= a.nacc) return;
    const double *p = a.part + (size_t)b * a.nwg * a.gpart + k;
    double v = 0.0;
    for (int w = 0; w < a.nwg; ++w) v += p[(size_t)w * a.gpart];
    a.out[(size_t)b * a.nacc + k] = a.info[b] != 0 ? __builtin_nan("") : v;
}

// ---- leave-one-point-out sums of the mid-size problems (sgpr_fit_batch_loo): behind step (b) above, in place of (c) ----------
struct MidLoo {
    int npts, nwg;
    size_t ld;                            // npad: Ky^-1 (lower) of problem b at K + b ld^2, its alpha at alpha + b ld
    const double *K, *alpha;
    double *part;                         // sum k of workgroup w of problem b at part[(b nwg + w) 2 + k]: k = 0 lpd, 1 |r|^2
    const int *info;
    double *out;                          // problem b's {loo, press} at out + 2 b
};

// points blockIdx.x GT .. + GT (one per thread) of problem blockIdx.z: the point's D x D block from the lower triangle of Ky^-1
// (loo_point_nd, batch_small.h).  D = 1: reg fits, D = 2: pairs (d = 1 or one canonical pair), D = 4, 6: d-pair fits; no family enters.
template <int D>
__global__ __launch_bounds__(GT) void mid_loo_kernel(const MidLoo a)
{
    __shared__ double red[GT / 64][2];
    const int b = blockIdx.z, N = a.npts, tid = threadIdx.x, i = blockIdx.x * GT + tid;
    const double *K = a.K + (size_t)b * a.ld * a.ld, *al = a.alpha + (size_t)b * a.ld;
    double lv[2] = {0.0, 0.0};
    if (i < N) {
        double r[D], S[D * (D + 1) / 2], lpd, rr;
        loo_point_nd<D>(K, a.ld, al, i, N, r, S, lpd, rr);
        lv[0] = lpd; lv[1] = rr;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double v = wave_sum(lv[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < 2) {
        double v = red[0][tid];
#pragma unroll
        for (int w = 1; w < GT / 64; ++w) v += red[w][tid];
        a.part[((size_t)b * a.nwg + blockIdx.x) * 2 + tid] = v;
    }
}

// problem blockIdx.x: its workgroups' partials in their fixed order; NaN where the factorisation failed
__global__ __launch_bounds__(64) void mid_loo_fold_kernel(const MidLoo a)
{
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= 2) return;
    const double *p = a.part + (size_t)b * a.nwg * 2 + k;
    double v = 0.0;
    for (int w = 0; w < a.nwg; ++w) v += p[(size_t)w * 2];
    a.out[(size_t)b * 2 + k] = a.info[b] != 0 ? __builtin_nan("") : (k == 0 ? -v : v);
}

// ---- the gradient of one leave-one-point-out objective of the mid-size problems (sgpr_fit_batch_loo_grad_mid): behind step (b) -----
// The formulas of loograd.hip and of grad_problem's phases (L1) - (L4), every step a grid over all problems of the chunk, ordered
// by the stream alone; a third npad x npad image per problem (M) stands behind the U images.
//   (p) the point pass (mid_loow_kernel): mid_loo_kernel's statements, so {loo, press} have its bits, and per point the weight block
//       W~_i (packed lower, T = D (D + 1) / 2 doubles, entry t of point i at wt[t N + i]) and v[B_i] (npad doubles, zero in the padding):
//       loo  W~_i = r r^T + S, v = r;   press  W~_i = 2 (r s^T + s r^T), v = 2 s, s = S r;
//   (m) the mirror (mid_mirror_kernel): Ky^-1's lower triangle into the strict upper one of its image, 64 x 64 blocks through LDS;
//   (z) beta = Ky^-1 v (mid_beta_kernel, n^2 flop) and Z = Ky^-1 W~ over the U image, dead after (b) (mid_z_kernel): column c N + i of
//       Z is sum_e W~_i[e, c] (column e N + i of Ky^-1); the whole npad x npad image is written, zeros in the padding rows and columns;
//   (M) M = Ky^-1 Z^T, lower 128 x 128 tiles, k over npad (mid_m_kernel): n^3 flop per problem on the matrix cores;
//   (w) W' = M - beta alpha^T - alpha beta^T over M's lower triangle (mid_wprime_kernel, the expression of grad_problem's (L3));
//   (c) the contraction of W' with dK by the nll gradient's own instances, mid_grad_kernel / mid_grad_nd_kernel, handed the M image
//       for Ky^-1 and a vector of zeros for alpha (their weight K[i, j] - alpha_i alpha_j is then W'[i, j] - 0, exactly): no second
//       set of contraction instances, and the existing ones keep their code; then one fold of both sets of partials
//       (mid_loograd_fold_kernel): {loo, press, raw sums}.
// A point whose block has a pivot that is not positive and finite has NaN in W~_i: D columns of Z, so all of M, so every sum.
struct MidLooW {
    int npts, n, nwg, which;              // which: SGPR_LOO_LPD / SGPR_LOO_PRESS, the same for the launch
    size_t ld;                            // npad: Ky^-1 (lower) of problem b at K + b ld^2, its alpha at alpha + b ld
    const double *K, *alpha;
    double *part;                         // as MidLoo::part
    double *wt, *v;                       // problem b's W~ at wt + b T npts, its v at v + b ld
};

template <int D>
__global__ __launch_bounds__(GT) void mid_loow_kernel(const MidLooW a)
{
    constexpr int T = D * (D + 1) / 2;
    __shared__ double red[GT / 64][2];
    const int b = blockIdx.z, N = a.npts, tid = threadIdx.x, i = blockIdx.x * GT + tid;
    const double *K = a.K + (size_t)b * a.ld * a.ld, *al = a.alpha + (size_t)b * a.ld;
    double *wt = a.wt + (size_t)b * T * N, *v = a.v + (size_t)b * a.ld;
    if (blockIdx.x == 0)
        for (int r = a.n + tid; r < (int)a.ld; r += GT) v[r] = 0.0;
    double lv[2] = {0.0, 0.0};
    if (i < N) {
        double r[D], S[T], lpd, rr;
        loo_point_nd<D>(K, a.ld, al, i, N, r, S, lpd, rr);
        lv[0] = lpd; lv[1] = rr;
        if (a.which == SGPR_LOO_PRESS) {
            double sr[D];                                 // s = S r
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
                for (int c = 0; c <= e; ++c) wt[(size_t)loo::pk(e, c) * N + i] = 2.0 * __builtin_fma(r[e], sr[c], sr[e] * r[c]);
                v[e * N + i] = 2.0 * sr[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < D; ++e) {
#pragma unroll
                for (int c = 0; c <= e; ++c) wt[(size_t)loo::pk(e, c) * N + i] = __builtin_fma(r[e], r[c], S[loo::pk(e, c)]);
                v[e * N + i] = r[e];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double s = wave_sum(lv[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = s;
    }
    __syncthreads();
    if (tid < 2) {
        double s = red[0][tid];
#pragma unroll
        for (int w = 1; w < GT / 64; ++w) s += red[w][tid];
        a.part[((size_t)b * a.nwg + blockIdx.x) * 2 + tid] = s;
    }
}

constexpr int MB = 64;                    // mirror: block side

// 64 x 64 block (r, t), r >= t, of problem blockIdx.y's Ky^-1 into block (t, r), transposed; a diagonal block: its strict upper part
__global__ __launch_bounds__(256) void mid_mirror_kernel(const MidInv a)
{
    __shared__ double s[MB][MB + 1];
    int t = (int)blockIdx.x, r = 0;            // lower blocks row by row, as mid_syrk_kernel
    while (t > r) { t -= r + 1; ++r; }
    double *K = a.L + (size_t)blockIdx.y * a.stride;
    const size_t ld = a.ld, r0 = (size_t)r * MB, c0 = (size_t)t * MB;
    for (int e = threadIdx.x; e < MB * MB; e += 256) {
        const int i = e % MB, j = e / MB;
        s[j][i] = K[(r0 + i) + (c0 + j) * ld];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < MB * MB; e += 256) {
        const int i = e % MB, j = e / MB;                 // entry (c0 + i, r0 + j) = entry (r0 + j, c0 + i)
        if (r != t || i < j) K[(c0 + i) + (r0 + j) * ld] = s[i][j];
    }
}

constexpr int ZP = 32;                    // Z: points per workgroup

struct MidZ {
    int npts, n;
    size_t ld;                            // npad: Ky^-1 (full) of problem b at K + b ld^2, Z at Z + b ld^2, v and beta at + b ld
    const double *K, *wt, *v;
    double *beta, *Z;
};

// row blockIdx.x GT + tid of beta = Ky^-1 v of problem blockIdx.y, the columns in order; zero in the padding
__global__ __launch_bounds__(GT) void mid_beta_kernel(const MidZ a)
{
    const int b = blockIdx.y, r = blockIdx.x * GT + threadIdx.x;
    if (r >= (int)a.ld) return;
    const double *K = a.K + (size_t)b * a.ld * a.ld + r, *v = a.v + (size_t)b * a.ld;
    double acc = 0.0;
    for (int k = 0; k < a.n; ++k) acc = __builtin_fma(K[(size_t)k * a.ld], v[k], acc);
    a.beta[(size_t)b * a.ld + r] = r < a.n ? acc : 0.0;
}

// rows blockIdx.x GT .. + GT (one per thread) x the D columns of each of the points blockIdx.y ZP .. + ZP of problem blockIdx.z's Z; the
// last blockIdx.y: the padding columns.  Rows below n only; the padding rows are zeros.
template <int D>
__global__ __launch_bounds__(GT) void mid_z_kernel(const MidZ a)
{
    constexpr int T = D * (D + 1) / 2;
    __shared__ double sw[T][ZP];
    const int b = blockIdx.z, N = a.npts, n = a.n, tid = threadIdx.x, r = blockIdx.x * GT + tid;
    const size_t ld = a.ld;
    const double *K = a.K + (size_t)b * ld * ld;
    double *Z = a.Z + (size_t)b * ld * ld;
    if (blockIdx.y == gridDim.y - 1) {
        if (r < (int)ld)
            for (int col = n; col < (int)ld; ++col) Z[r + (size_t)col * ld] = 0.0;
        return;
    }
    const int p0 = blockIdx.y * ZP, np = min(ZP, N - p0);
    for (int e = tid; e < T * np; e += GT) sw[e / np][e % np] = a.wt[(size_t)b * T * N + (size_t)(e / np) * N + p0 + e % np];
    __syncthreads();
    if (r >= (int)ld) return;
    for (int jj = 0; jj < np; ++jj) {
        const int i = p0 + jj;
        double kc[D];
#pragma unroll
        for (int e = 0; e < D; ++e) kc[e] = K[r + ((size_t)e * N + i) * ld];
#pragma unroll
        for (int c = 0; c < D; ++c) {
            double z = sw[loo::pk(D - 1, c)][jj] * kc[D - 1];
#pragma unroll
            for (int e = D - 2; e >= 0; --e) z = __builtin_fma(sw[e >= c ? loo::pk(e, c) : loo::pk(c, e)][jj], kc[e], z);
            Z[r + ((size_t)c * N + i) * ld] = r < n ? z : 0.0;
        }
    }
}

struct MidM {
    const double *K, *Z;  // problem b's Ky^-1 (full) and Z at + b * stride (column-major, ld)
    double *M;
    size_t stride, ld;
    int k;                // npad
};

__global__ __launch_bounds__(256, 2) void mid_m_kernel(const MidM a)
{
    __shared__ double smem[2 * tile::BK * (2 * (128 + tile::PAD))];
    int t = (int)blockIdx.x, r = 0;            // lower tiles row by row, as mid_syrk_kernel
    while (t > r) { t -= r + 1; ++r; }
    const size_t off = (size_t)blockIdx.y * a.stride, ld = a.ld, ri = (size_t)r * LEAF, cj = (size_t)t * LEAF;
    tile::GemmArgs g{};
    g.m = 128; g.n = 128; g.k = a.k;
    g.alpha = 1.0; g.beta = 0.0;
    g.A = a.K + off + ri; g.lda = ld;          // M[i, j] = sum_k Ky^-1[i, k] Z[j, k]
    g.B = a.Z + off + cj; g.ldb = ld;
    g.C = a.M + off + ri + cj * ld; g.ldc = ld;
    tile::gemm_body_dma<128, 128, 2>(g, smem, 0, 0);
}

constexpr int WC = 64;                    // W': columns per workgroup

struct MidWp {
    int n;
    size_t ld;                            // npad: M of problem b at M + b ld^2, alpha and beta at + b ld
    const double *alpha, *beta;
    double *M;
};

// rows blockIdx.x GT .. + GT (one per thread) x columns blockIdx.y WC .. + WC of problem blockIdx.z, on and below the diagonal, below n
__global__ __launch_bounds__(GT) void mid_wprime_kernel(const MidWp a)
{
    __shared__ double sal[WC], sbe[WC];
    const int b = blockIdx.z, tid = threadIdx.x, i = blockIdx.x * GT + tid, j0 = blockIdx.y * WC, nj = min(WC, a.n - j0);
    if ((int)(blockIdx.x * GT + GT - 1) < j0) return;     // the whole tile is above the diagonal
    const double *al = a.alpha + (size_t)b * a.ld, *be = a.beta + (size_t)b * a.ld;
    if (tid < nj) { sal[tid] = al[j0 + tid]; sbe[tid] = be[j0 + tid]; }
    __syncthreads();
    if (i >= a.n) return;
    double *Mrow = a.M + (size_t)b * a.ld * a.ld + i;
    const double bi = be[i], ali = al[i];
    for (int jj = 0; jj < nj; ++jj) {
        const int j = j0 + jj;
        if (j > i) break;
        Mrow[(size_t)j * a.ld] = Mrow[(size_t)j * a.ld] - bi * sal[jj] - ali * sbe[jj];
    }
}

// problem blockIdx.x: {loo, press} from the point pass's partials (mid_loo_fold_kernel's order and signs) and, behind them, the raw
// gradient sums from the contraction's (mid_grad_fold_kernel's order), nacc = 2 + the number of sums apart; NaN where the
// factorisation failed
__global__ __launch_bounds__(64) void mid_loograd_fold_kernel(const MidGrad a, const double *lpart, int lnwg)
{
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= a.nacc) return;
    double v = 0.0;
    if (k < 2) {
        const double *p = lpart + (size_t)b * lnwg * 2 + k;
        for (int w = 0; w < lnwg; ++w) v += p[(size_t)w * 2];
        if (k == 0) v = -v;
    } else {
        const double *p = a.part + (size_t)b * a.nwg * a.gpart + (k - 2);
        for (int w = 0; w < a.nwg; ++w) v += p[(size_t)w * a.gpart];
    }
    a.out[(size_t)b * a.nacc + k] = a.info[b] != 0 ? __builtin_nan("") : v;
}

}  // namespace

}  // namespace sgpr
