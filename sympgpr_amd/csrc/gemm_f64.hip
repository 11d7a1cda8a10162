// gemm_f64.hip -- C = beta C + alpha A B^T in fp64 on the gfx950 matrix cores
// (v_mfma_f64_16x16x4_f64).  This is where the n^3/3 flop of the Cholesky
// (scipy.linalg.cholesky -> LAPACK dpotrf at python/functions/func.py:166,184,193) are spent:
// the SYRK/GEMM trailing updates and the panel solves all run through this kernel.
//
// Roofline: fp64 MFMA.  One 16x16x4 MFMA = 2048 flop per wave for one fp64 operand register
// per side, so the kernel is arranged to keep the matrix pipe issuing back to back:
//   * workgroup tile 256 x 128 (8 waves, each 64 x 64 = 16 accumulators of 4 fp64 = 128
//     VGPRs -> two waves per SIMD fit), k-step 16, LDS double-buffered, one barrier per k-step,
//     the next k-tile's global loads in flight under the current tile's 64 MFMAs per wave;
//   * both operands are "row index contiguous, k strided" (column-major panels of the
//     factor), which is exactly the MFMA A/B fragment order (lane&15 = row, lane>>4 = k), so the
//     LDS image is the global image: [k][row] with the row stride padded by 16 doubles
//     (2*stride mod 64 banks = 32 -> the two k-rows of a 32-lane ds_read_b64 group hit
//     disjoint bank halves);
//   * the MFMA is fed with the B(n)-side as its A operand and the A(m)-side as its B operand:
//     the accumulator then has lane&15 = m (memory-contiguous in column-major C) and
//     4*reg+(lane>>4) = n, so every C access of a 16-lane quarter is one full 128-B line.
//     (fp64 C/D layout: col = lane&15, row = (lane>>4) + 4*reg -- NOT the f32 map.)
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <vector>

#include "common.h"
#include "gemm_tile.h"

namespace sgpr {

namespace {

// Optional per-launch HIP-event timing (bench.py's roofline pass); off by default.  The events come
// from a fixed pool created on the first gemm_profile_begin() and reused by every later window: the
// launch path never creates or destroys an event (round 1 created two per launch -- thousands of
// live events per step).  All state is behind one mutex: several fit handles may launch from their
// own threads while a window is open.
struct ProfRec { double flop; int big; int m, n, k, lower, overlap; };
struct Prof {
    std::mutex mu;
    std::atomic<bool> on{false};       // read outside the mutex on the launch path
    std::vector<hipEvent_t> pool;      // 2 * PROF_POOL events, created once per process
    std::vector<ProfRec> recs;         // record i uses pool[2 i], pool[2 i + 1]
    long dropped = 0;                  // launches beyond the pool (not timed)
};
constexpr int PROF_POOL = 8192;
Prof g_prof;
thread_local int t_overlap = 0;        // set by the look-ahead driver: launches share the device

using namespace tile;

// second launch-bound argument = waves per SIMD: both tile shapes are sized for TWO waves per SIMD
// (<= 256 VGPRs): one 512-thread workgroup per CU (256x128), or two independent 256-thread
// workgroups per CU (128x128) whose barriers do not line up.
template <int BM, int BN>
__global__ __launch_bounds__(64 * (BM / 64) * (BN / 64), (BM >= 128 ? 2 : 1)) void gemm_nt_kernel(const GemmArgs g)
{
    constexpr int LDA_S = BM + PAD, LDB_S = BN + PAD;
    // SGPR_GEMM_STAGES for the one-workgroup-per-CU shape (3 = 156 KiB of the CU's 160), two otherwise
    constexpr int STAGES = (BM == 256 && BN == 128) ? SGPR_GEMM_STAGES : 2;
    __shared__ double smem[STAGES * BK * (LDA_S + LDB_S)];
    int tile_r, tile_c;
    if (!tile_of<(SR * BM) / (4 * BN)>(g, tile_r, tile_c)) return;
    const int row0 = tile_r * BM, col0 = tile_c * BN;
    if (g.lower) {
        const long rb = ((long)min(row0 + BM, g.m) - 1) / g.lblk, cb = (long)col0 / g.lblk;
        if (rb * g.lpr + g.lpi < cb * g.lpc + g.lpj) return;
    }
    const bool aligned = ((((uintptr_t)g.A | (uintptr_t)g.B) & 15) == 0) && (((g.lda | g.ldb) & 1) == 0);
    const bool fast = aligned && (row0 + BM <= g.m) && (col0 + BN <= g.n) && (g.k % BK == 0);
    if (g.transb) {
        if (fast) gemm_body<BM, BN, true, true>(g, smem, tile_r, tile_c);
        else      gemm_body<BM, BN, false, true>(g, smem, tile_r, tile_c);
        return;
    }
    if constexpr (BM % 128 == 0) {
        if (fast && !(g.dbg & 16)) { gemm_body_dma<BM, BN, STAGES>(g, smem, tile_r, tile_c); return; }
    }
    if (fast) gemm_body<BM, BN, true>(g, smem, tile_r, tile_c);
    else      gemm_body<BM, BN, false>(g, smem, tile_r, tile_c);
}

// The same product with TWO destinations (the Strassen front end below): C = beta C + alpha P and C2 += alpha2 P from one
// set of accumulators.  A kernel of its own, so that gemm_nt_kernel is compiled exactly as without it.
__global__ __launch_bounds__(512, 2) void gemm_nt2_kernel(const GemmArgs g)
{
    constexpr int BM = 256, BN = 128, LDA_S = BM + PAD, LDB_S = BN + PAD;
    __shared__ double smem[SGPR_GEMM_STAGES * BK * (LDA_S + LDB_S)];
    int tile_r, tile_c;
    if (!tile_of<(SR * BM) / (4 * BN)>(g, tile_r, tile_c)) return;
    const int row0 = tile_r * BM, col0 = tile_c * BN;
    const bool aligned = ((((uintptr_t)g.A | (uintptr_t)g.B) & 15) == 0) && (((g.lda | g.ldb) & 1) == 0);
    const bool fast = aligned && (row0 + BM <= g.m) && (col0 + BN <= g.n) && (g.k % BK == 0);
    if (fast) gemm_body_dma<BM, BN, SGPR_GEMM_STAGES, true>(g, smem, tile_r, tile_c);
    else      gemm_body<BM, BN, false, false, true>(g, smem, tile_r, tile_c);
}

// ... and with up to FOUR (two Strassen levels: an inner product of an outer product): C = beta C + alpha P, then C_d += alpha_d P
// for g.ndst - 1 further destinations.  Again a kernel of its own: the two above are compiled exactly as without it.
__global__ __launch_bounds__(512, 2) void gemm_nt4_kernel(const GemmArgs g)
{
    constexpr int BM = 256, BN = 128, LDA_S = BM + PAD, LDB_S = BN + PAD;
    __shared__ double smem[SGPR_GEMM_STAGES * BK * (LDA_S + LDB_S)];
    int tile_r, tile_c;
    if (!tile_of<(SR * BM) / (4 * BN)>(g, tile_r, tile_c)) return;
    const int row0 = tile_r * BM, col0 = tile_c * BN;
    const bool aligned = ((((uintptr_t)g.A | (uintptr_t)g.B) & 15) == 0) && (((g.lda | g.ldb) & 1) == 0);
    const bool fast = aligned && (row0 + BM <= g.m) && (col0 + BN <= g.n) && (g.k % BK == 0);
    if (fast) gemm_body_dma<BM, BN, SGPR_GEMM_STAGES, false, true>(g, smem, tile_r, tile_c);
    else      gemm_body<BM, BN, false, false, false, true>(g, smem, tile_r, tile_c);
}

// a further destination of a product: C += alpha A B^T
struct Dst { double *C; size_t ld; double alpha; };

// T (rows x cols, leading dimension rows) = X + sign Y on column-major blocks: the operand sums of the Strassen front end.
// HBM-bound (two reads, one write per element): 16-byte accesses, 4 columns per thread in flight, grid-stride over
// pieces of 512 rows x 4 columns.  rows even, all three bases 16-byte aligned, ldx / ldy even (checked by the caller).
__global__ __launch_bounds__(256) void block_sum_kernel(int rows, int cols, const double *X, size_t ldx, const double *Y, size_t ldy,
                                                        double sign, double *T)
{
    const int nrc = (rows + 511) / 512, ncg = (cols + 3) / 4;
    const long pieces = (long)nrc * ncg;
    for (long p = blockIdx.x; p < pieces; p += gridDim.x) {
        const int cg = (int)(p / nrc), rc = (int)(p - (long)cg * nrc);
        const int r = rc * 512 + 2 * (int)threadIdx.x;
        if (r >= rows) continue;
        double2_t x[4], y[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = min(cg * 4 + u, cols - 1);
            x[u] = *reinterpret_cast<const double2_t *>(X + (size_t)r + (size_t)c * ldx);
            y[u] = *reinterpret_cast<const double2_t *>(Y + (size_t)r + (size_t)c * ldy);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = cg * 4 + u;
            if (c < cols) *reinterpret_cast<double2_t *>(T + (size_t)r + (size_t)c * (size_t)rows) = x[u] + sign * y[u];
        }
    }
}

}  // namespace

int gemm_nt(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B,
            size_t ldb, double beta, double *C, size_t ldc, int lower, long diag_off,
            hipStream_t st)
{
    const int bc[5] = {1, 1, (int)diag_off, 1, 0};
    return gemm_nt_bc(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, lower, bc, st);
}

static int gemm_launch(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B,
                       size_t ldb, double beta, double *C, size_t ldc, int lower, const int *bc, int transb,
                       hipStream_t st, unsigned long long *stamps = nullptr, int dbg = 0, const Dst *x = nullptr, int nx = 0,
                       bool k4 = false);

// `bc` = {blk, pr, pi, pc, pj}: the block-cyclic form of the lower-mode skip test (GemmArgs)
static int gemm_chunked(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B,
                        size_t ldb, double beta, double *C, size_t ldc, int lower, const int *bc,
                        hipStream_t st, const Dst *x, int nx, bool k4)
{
    // Products deeper than 8192 run as back-to-back launches of <= 8192 columns each (C re-read per launch, negligible
    // beside the flop), so that the 32 workgroups sharing a super-tile's operand panels restart in step instead of drifting
    // apart over a 65536-deep loop.  Measured on one MI355X (profiles/r03/kmax.md): m = 65536 lower, k = 65536: 71.6 -> 72.6
    // TFLOP/s (16384: 72.0), k = 32768: 71.5 -> 72.6; the n = 131072 step 70.0 -> 71.1.  SGPR_GEMM_KMAX=<k> overrides, 0 = off.
    static const int kmax = [] { const char *e = getenv("SGPR_GEMM_KMAX"); return e ? atoi(e) : 8192; }();
    if (kmax >= 128 && k > kmax) {
        const int nchunk = (k + kmax - 1) / kmax;
        const int step = ((k + nchunk - 1) / nchunk + 127) / 128 * 128;
        for (int k0 = 0; k0 < k; k0 += step) {
            const int rc = gemm_launch(m, n, std::min(step, k - k0), alpha, A + (size_t)k0 * lda, lda, B + (size_t)k0 * ldb, ldb,
                                       k0 == 0 ? beta : 1.0, C, ldc, lower, bc, 0, st, nullptr, 0, x, nx, k4);
            if (rc) return rc;
        }
        return 0;
    }
    return gemm_launch(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, lower, bc, 0, st, nullptr, 0, x, nx, k4);
}

int gemm_nt_bc(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B,
               size_t ldb, double beta, double *C, size_t ldc, int lower, const int *bc,
               hipStream_t st)
{
    return gemm_chunked(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, lower, bc, st, nullptr, 0, false);
}

// C = beta C + alpha A B^T and C2 += alpha2 A B^T in one pass over the operands (every k chunk adds to both)
int gemm_nt_two(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb, double beta,
             double *C, size_t ldc, double alpha2, double *C2, size_t ldc2, hipStream_t st)
{
    const int bc[5] = {1, 1, 0, 1, 0};
    if (!C2) { set_error("gemm_nt_two: null second destination"); return SGPR_E_ARG; }
    const Dst x{C2, ldc2, alpha2};
    return gemm_chunked(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, 0, bc, st, &x, 1, false);
}

// count (2 .. 4) destinations from one product, disjoint blocks: C[0] = beta C[0] + alpha[0] A B^T, C[d] += alpha[d] A B^T
// (gemm_nt4_kernel; every k chunk adds to all of them)
int gemm_nt_multi(int m, int n, int k, const double *A, size_t lda, const double *B, size_t ldb, double beta, int count,
                  double *const *C, const size_t *ldc, const double *alpha, hipStream_t st)
{
    const int bc[5] = {1, 1, 0, 1, 0};
    if (count < 2 || count > 4 || !C || !ldc || !alpha) { set_error("gemm_nt_multi: 2 to 4 destinations"); return SGPR_E_ARG; }
    Dst x[3];
    for (int d = 0; d < count; ++d) {
        if (!C[d]) { set_error("gemm_nt_multi: null destination"); return SGPR_E_ARG; }
        if (d) x[d - 1] = Dst{C[d], ldc[d], alpha[d]};
    }
    return gemm_chunked(m, n, k, alpha[0], A, lda, B, ldb, beta, C[0], ldc[0], 0, bc, st, x, count - 1, true);
}

static int gemm_launch(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B,
                       size_t ldb, double beta, double *C, size_t ldc, int lower, const int *bc, int transb,
                       hipStream_t st, unsigned long long *stamps, int dbg, const Dst *x, int nx, bool k4)
{
    const bool plain = bc[0] == 1 && bc[1] == 1 && bc[3] == 1 && bc[4] == 0;
    const long diag_off = plain ? bc[2] : 1;  // != 0 disables the triangular tile enumeration
    if (bc[0] < 1 || bc[1] < 1 || bc[3] < 1) { set_error("gemm_nt: bad block-cyclic descriptor"); return SGPR_E_ARG; }
    if (m < 0 || n < 0 || k < 0) { set_error("gemm_nt: negative extent"); return SGPR_E_ARG; }
    if (m == 0 || n == 0) return 0;
    if (lda < (size_t)m || ldb < (size_t)(transb ? k : n) || ldc < (size_t)m) {
        set_error("gemm: leading dimension too small");
        return SGPR_E_ARG;
    }
    if (nx < 0 || nx > 3 || (nx && !x)) { set_error("gemm: bad destination count"); return SGPR_E_ARG; }
    Dst d[3] = {};
    for (int i = 0; i < nx; ++i) {
        d[i] = x[i];
        if (!d[i].C || lower || transb || d[i].ld < (size_t)m) { set_error("gemm: bad second destination"); return SGPR_E_ARG; }
    }
    GemmArgs g{m, n, k, alpha, beta, A, lda, B, ldb, C, ldc, lower, diag_off, transb, stamps, 0, 0, 0, 0, 0, 0,
               0, 0, bc[0], bc[1], bc[2], bc[3], bc[4], dbg, nullptr, d[0].C, d[0].ld, d[0].alpha,
               d[1].C, d[1].ld, d[1].alpha, d[2].C, d[2].ld, d[2].alpha, nx + 1};
    auto set_map = [&](int bm, int bn) {
        g.tiles_m = (m + bm - 1) / bm;
        g.tiles_n = (n + bn - 1) / bn;
        const int SC = (SR * bm) / (4 * bn);  // 4 for 256x128, 2 for 128x128
        g.n_sr = (g.tiles_m + SR - 1) / SR;
        g.n_sc = (g.tiles_n + SC - 1) / SC;
        g.tri = (lower && diag_off == 0 && m == n) ? 1 : 0;
        if (g.tri) {
            // full super-tiles below the first needed row of every super-column, then 4 diagonal
            // slots per group (slots of a partial last group that do not exist exit at once)
            long full = 0;
            for (int sc = 0; sc < g.n_sc; ++sc) full += std::max(g.n_sr - sc / 4 - 1, 0);
            g.n_full = (int)full;
            g.n_grp = (g.n_sc + 3) / 4;
            g.n_super = g.n_full + 4 * g.n_grp;
        }
        if (!g.tri) g.n_super = g.n_sr * g.n_sc;
        return (unsigned)(((g.n_super + 7) / 8) * 8 * SR * SC);
    };
    // profile window open: take the next event pair of the pool (none left: the launch goes untimed)
    int slot = -1;
    ProfRec rec{};
    if (g_prof.on.load(std::memory_order_acquire)) {
        std::lock_guard<std::mutex> lock(g_prof.mu);
        if (g_prof.on.load(std::memory_order_relaxed)) {
            if ((int)g_prof.recs.size() < PROF_POOL) {
                // algorithmic flop of this launch: 2k per updated element (lower: on/below the diagonal)
                double elems = (double)m * n;
                if (lower && plain) {
                    elems = 0.0;
                    for (int j = 0; j < n; ++j) {
                        long first = (long)j - diag_off;  // first row with row + diag_off >= col
                        if (first < 0) first = 0;
                        if (first < m) elems += (double)(m - first);
                    }
                } else if (lower) {
                    // local piece of a block-cyclic matrix: element (i, j) counts iff its GLOBAL position is
                    // on or below the diagonal: block (i / blk) pr + pi against (j / blk) pc + pj, then the
                    // offsets inside the block
                    elems = 0.0;
                    const long blk = bc[0];
                    for (long j = 0; j < n; ++j) {
                        const long cbg = (j / blk) * bc[3] + bc[4], jo = j % blk;
                        for (long rb = 0; rb * blk < m; ++rb) {
                            const long rbg = rb * bc[1] + bc[2], rows = std::min(blk, (long)m - rb * blk);
                            if (rbg > cbg) elems += (double)rows;
                            else if (rbg == cbg) elems += (double)std::max(0L, rows - jo);
                        }
                    }
                }
                rec.flop = 2.0 * k * elems;
                rec.m = m; rec.n = n; rec.k = k; rec.lower = lower; rec.overlap = t_overlap;
                slot = (int)g_prof.recs.size();
                g_prof.recs.push_back(rec);
            } else {
                ++g_prof.dropped;
            }
        }
    }
    if (slot >= 0) SGPR_HIP(hipEventRecord(g_prof.pool[2 * slot], st));
    // big tile once it yields enough workgroups to fill 256 CUs, small tile below that
    const long big = (long)((m + 255) / 256) * ((n + 127) / 128);
    // Tile choice, measured on MI355X: at 8192^3 two independent 128x128 workgroups per CU reach
    // 71.5 TFLOP/s against 69.5 for one 256x128 workgroup (their barriers do not line up), but
    // inside the n = 131072 factorisation the 256x128 shape wins (61.7 vs 58.4 TFLOP/s overall:
    // a third less operand traffic per flop, and the triangular tile map below needs its 2:1
    // aspect).  So: 256x128 whenever it yields >= 256 workgroups, 128x128 below.
    // tunable "gemm_small_tile" = 1 forces the 128x128 shape (A/B experiments, sgpr_probe_tune).
    static const bool prefer_big = tune("gemm_small_tile", 0) == 0;
    // tunable "gemm_small_mb" = <MB>: take the 128x128 shape for products whose operand panels are smaller than
    // that (experiments; default off).  Alone, lower-triangular m = 15360, 256x128 vs 128x128 tiles:
    // k = 256 47.4 vs 55.8, 512 49.0 vs 52.1, 1024 56.8 vs 61.2, 2048 61.2 vs 64.3 TFLOP/s -- but inside the
    // blocked factorisation, beside the panel stream, the small shape LOSES (n = 16384 39.0 vs 34.5 ms,
    // n = 32768 231 vs 208 ms): two of its workgroups share a CU and its LDS bandwidth with nothing to spare.
    static const double small_mb = tune("gemm_small_mb", 0.0);
    const double op_bytes = 8.0 * (double)k * ((A == B && lda == ldb) ? (double)std::max(m, n) : (double)m + n);
    const bool small_k = op_bytes <= small_mb * 1e6 && m > 128 && n > 128;
    if (nx) {
        // several destinations: always the 256x128 shape (the front end only sends products that fill the chip)
        const dim3 grid(set_map(256, 128));
        if (k4 || nx > 1) hipLaunchKernelGGL(gemm_nt4_kernel, grid, dim3(512), 0, st, g);
        else              hipLaunchKernelGGL(gemm_nt2_kernel, grid, dim3(512), 0, st, g);
        rec.big = 1;
    } else if (n <= 128 && m <= 32768 && !(dbg & 8)) {
        // one column tile (the in-place panel solve against an inverted leaf, k = n <= 128): a
        // latency problem, not a throughput one -- 64-row tiles quadruple the workgroup count and
        // halve the per-workgroup critical path (two waves, register-staged operands)
        const dim3 grid(set_map(64, 128));
        hipLaunchKernelGGL((gemm_nt_kernel<64, 128>), grid, dim3(128), 0, st, g);
    } else if (prefer_big && !(dbg & 8) && !small_k && (big >= 256 || (m >= 256 && n == 128))) {
        const dim3 grid(set_map(256, 128));
        hipLaunchKernelGGL((gemm_nt_kernel<256, 128>), grid, dim3(512), 0, st, g);
        rec.big = 1;
    } else {
        const dim3 grid(set_map(128, 128));
        hipLaunchKernelGGL((gemm_nt_kernel<128, 128>), grid, dim3(256), 0, st, g);
    }
    SGPR_CHECK_LAUNCH();
    if (slot >= 0) {
        SGPR_HIP(hipEventRecord(g_prof.pool[2 * slot + 1], st));
        if (rec.big) {
            std::lock_guard<std::mutex> lock(g_prof.mu);
            if (slot < (int)g_prof.recs.size()) g_prof.recs[slot].big = 1;
        }
    }
    return 0;
}

// diagnostics only (libsympgpr_probe.so): one product with per-workgroup clock stamps and the
// tile-shape / staging switches (8 = 128x128 tiles, 16 = register-staged body); nothing global
int gemm_nt_diag(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb,
                 double beta, double *C, size_t ldc, int lower, unsigned long long *stamps, int dbg, hipStream_t st)
{
    const int bc[5] = {1, 1, 0, 1, 0};
    return gemm_launch(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, lower, bc, 0, st, stamps, dbg);
}

// C (m x n) = beta C + alpha A (m x k) B (k x n): the "NN" product (B's k index contiguous)
int gemm_nn(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb,
            double beta, double *C, size_t ldc, hipStream_t st)
{
    const int bc[5] = {1, 1, 0, 1, 0};
    return gemm_launch(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, 0, bc, 1, st);
}

void gemm_set_overlap(int on) { t_overlap = on; }

int gemm_profile_begin()
{
    std::lock_guard<std::mutex> lock(g_prof.mu);
    if (g_prof.pool.empty()) {
        g_prof.pool.resize(2 * (size_t)PROF_POOL);
        for (size_t i = 0; i < g_prof.pool.size(); ++i) {
            const hipError_t e = hipEventCreate(&g_prof.pool[i]);
            if (e != hipSuccess) {
                for (size_t j = 0; j < i; ++j) (void)hipEventDestroy(g_prof.pool[j]);
                g_prof.pool.clear();
                return hip_fail(e, "hipEventCreate (profile pool)", __FILE__, __LINE__);
            }
        }
        g_prof.recs.reserve(PROF_POOL);
    }
    g_prof.recs.clear();
    g_prof.dropped = 0;
    g_prof.on = true;
    return 0;
}

// per-launch records of the last profile window: 7 doubles each (m, n, k, lower, big, ms, overlap)
static std::vector<double> g_last_launches;
int gemm_profile_launches(double *buf, int max_records)
{
    std::lock_guard<std::mutex> lock(g_prof.mu);
    const int n = (int)(g_last_launches.size() / 7);
    if (buf)
        for (int i = 0; i < n && i < max_records; ++i)
            for (int j = 0; j < 7; ++j) buf[7 * i + j] = g_last_launches[7 * i + j];
    return n;
}

// out[0..2]: big-tile launches / flop / ms that ran alone on the device; out[3..5]: small-tile launches
// (all); out[6..7]: largest launch flop / ms; out[8..10]: big-tile launches / flop / ms issued inside the
// look-ahead driver (two streams share the chip: their durations overlap); out[11]: launches not timed
int gemm_profile_end(double *out)
{
    std::lock_guard<std::mutex> lock(g_prof.mu);
    g_prof.on = false;
    g_last_launches.clear();
    for (int i = 0; i < 12; ++i) out[i] = 0.0;
    out[11] = (double)g_prof.dropped;
    for (size_t i = 0; i < g_prof.recs.size(); ++i) {
        const ProfRec &r = g_prof.recs[i];
        SGPR_HIP(hipEventSynchronize(g_prof.pool[2 * i + 1]));
        float ms = 0.f;
        SGPR_HIP(hipEventElapsedTime(&ms, g_prof.pool[2 * i], g_prof.pool[2 * i + 1]));
        const int o = r.big ? (r.overlap ? 8 : 0) : 3;
        out[o] += 1.0; out[o + 1] += r.flop; out[o + 2] += ms;
        if (r.flop > out[6]) { out[6] = r.flop; out[7] = ms; }
        for (double v : {(double)r.m, (double)r.n, (double)r.k, (double)r.lower, (double)r.big, (double)ms, (double)r.overlap})
            g_last_launches.push_back(v);
    }
    g_prof.recs.clear();
    return 0;
}

// ---- one level of Strassen's algorithm in front of the NT product ------------------------------------------------
// P = A B^T with A = [A11 A12; A21 A22] (m halves x k halves), B likewise (n halves x k halves) needs 7 half-size
// products instead of 8:
//   M1 = (A11 + A22)(B11 + B22)^T -> C11, C22     M2 = (A21 + A22) B11^T -> C21, -C22    M3 = A11 (B21 - B22)^T -> C12, C22
//   M4 = A22 (B12 - B11)^T -> C11, C21            M5 = (A11 + A12) B22^T -> -C11, C12    M6 = (A21 - A11)(B11 + B21)^T -> C22
//   M7 = (A12 - A22)(B12 + B22)^T -> C11
// Every M is accumulated straight into its destination blocks by the two-destination kernel: no M temporaries, no
// block-accumulate passes; the ten operand sums go through two scratch blocks (one per side) reused product after product
// in stream order.  The whole decision -- which sums, which products, which destinations and signs, what stays classical --
// is host code that emits a list of records (strassen_plan); the device path below executes exactly that list, and
// tests/test_strassen_plan_cpu.py replays it in numpy.
// Record = 16 words.  [0] = kind:
//   PLAN_SUM   [1] side (0: rows of A -> the A scratch, 1: rows of B -> the B scratch) [2] rows [3] cols
//              [4] xr [5] xc [6] yr [7] yc [8] sign         T = X + sign Y, X / Y the blocks at (row, k column) of that operand
//   PLAN_PROD  [1] a_src (0: block of A at ([2], [3]), 1: the A scratch) [4] b_src, ([5], [6]) likewise [7] m [8] n [9] k
//              [10] [11] first destination (row, column of C) [12] its sign [13] [14] [15] the second one (sign 0: none)
//   PLAN_CLASSIC  [1] lower [2] ar [3] ac [4] br [5] bc [6] m [7] n [8] k [9] cr [10] cc      the classical launch on a block
namespace {
struct PlanCfg {
    long smin;      // smallest half-size of m and n that qualifies (half of k: smin / 2)
    long kslab;     // k is processed in slabs of at most this many columns (bounds the scratch)
    size_t scratch; // doubles of scratch available
};
void put(std::vector<long long> &out, std::initializer_list<long long> v)
{
    size_t i = 0;
    for (long long x : v) { out.push_back(x); ++i; }
    for (; i < STRASSEN_REC; ++i) out.push_back(0);
}
// slab length of a k extent (0: the extent does not qualify): near-equal slabs of at most kslab columns, multiples of 32
long slab_of(long k, const PlanCfg &c)
{
    if (k <= 0 || k % 32 != 0 || c.kslab < 32) return 0;
    const long nslab = (k + c.kslab - 1) / c.kslab;
    const long step = ((k + nslab - 1) / nslab + 31) / 32 * 32;
    const long kmin = std::max(c.smin / 2, 16L);
    const long last = k - (nslab - 1) * step;
    if (last <= 0 || step / 2 < kmin || last / 2 < kmin) return 0;
    return step;
}
bool qualifies(long m, long n, long k, const PlanCfg &c)
{
    // halves stay multiples of the 256 x 128 tile, so every workgroup takes the LDS-DMA body
    if (m <= 0 || n <= 0 || m % 512 != 0 || n % 256 != 0) return false;
    if (m / 2 < c.smin || n / 2 < c.smin) return false;
    const long step = slab_of(k, c);
    if (!step) return false;
    return (size_t)(m / 2 + n / 2) * (size_t)(step / 2) <= c.scratch;
}
// the ten sums and seven products of one k slab [k0, k0 + 2 k2) of the m2-, n2-halved product at rows ar / br, destination
// (cr, cc); `kind_sum` / `kind_prod`: the inner level's records or the outer level's (PLAN2_*, same layout)
void seven(int kind_sum, int kind_prod, long m2, long n2, long k2, long k0, long ar, long br, long cr, long cc, std::vector<long long> &out)
{
    // block (i, j) of an operand: row offset, k-column offset
    const long a1 = ar, a2 = ar + m2, b1 = br, b2 = br + n2, j1 = k0, j2 = k0 + k2;
    const long c1r = cr, c2r = cr + m2, c1c = cc, c2c = cc + n2;
    auto sum = [&](int side, long xr, long xc, long yr, long yc, int sign) {
        put(out, {kind_sum, side, side ? n2 : m2, k2, xr, xc, yr, yc, sign});
    };
    auto prod = [&](int as, long pr, long pc, int bs, long qr, long qc, long d1r, long d1c, int s1, long d2r, long d2c, int s2) {
        put(out, {kind_prod, as, pr, pc, bs, qr, qc, m2, n2, k2, d1r, d1c, s1, d2r, d2c, s2});
    };
    sum(0, a1, j1, a2, j2, +1); sum(1, b1, j1, b2, j2, +1);                      // M1
    prod(1, 0, 0, 1, 0, 0, c1r, c1c, +1, c2r, c2c, +1);
    sum(0, a2, j1, a2, j2, +1);                                                    // M2
    prod(1, 0, 0, 0, b1, j1, c2r, c1c, +1, c2r, c2c, -1);
    sum(1, b2, j1, b2, j2, -1);                                                    // M3
    prod(0, a1, j1, 1, 0, 0, c1r, c2c, +1, c2r, c2c, +1);
    sum(1, b1, j2, b1, j1, -1);                                                    // M4
    prod(0, a2, j2, 1, 0, 0, c1r, c1c, +1, c2r, c1c, +1);
    sum(0, a1, j1, a1, j2, +1);                                                    // M5
    prod(1, 0, 0, 0, b2, j2, c1r, c1c, -1, c1r, c2c, +1);
    sum(0, a2, j1, a1, j1, -1); sum(1, b1, j1, b2, j1, +1);                      // M6
    prod(1, 0, 0, 1, 0, 0, c2r, c2c, +1, 0, 0, 0);
    sum(0, a1, j2, a2, j2, -1); sum(1, b1, j2, b2, j2, +1);                      // M7
    prod(1, 0, 0, 1, 0, 0, c1r, c1c, +1, 0, 0, 0);
}
void plan_gemm(long m, long n, long k, long ar, long br, long cr, long cc, const PlanCfg &c, std::vector<long long> &out)
{
    if (!qualifies(m, n, k, c)) {
        put(out, {PLAN_CLASSIC, 0, ar, 0, br, 0, m, n, k, cr, cc});
        return;
    }
    const long step = slab_of(k, c);
    for (long k0 = 0; k0 < k; k0 += step) seven(PLAN_SUM, PLAN_PROD, m / 2, n / 2, std::min(step, k - k0) / 2, k0, ar, br, cr, cc, out);
}
// lower update of the square block at row / column r0: while its off-diagonal square qualifies, the two diagonal halves
// recurse and the square goes through plan_gemm; then the triangular launch as before
void plan_syrk(long n, long k, long r0, const PlanCfg &c, std::vector<long long> &out)
{
    const long h = n / 2;
    if (n % 2 != 0 || !qualifies(h, h, k, c)) {
        put(out, {PLAN_CLASSIC, 1, r0, 0, r0, 0, n, n, k, r0, r0});
        return;
    }
    plan_syrk(h, k, r0, c, out);
    plan_gemm(h, h, k, r0 + h, r0, r0 + h, r0, c, out);
    plan_syrk(h, k, r0 + h, c, out);
}
size_t plan_need(const std::vector<long long> &plan)
{
    size_t need[2] = {0, 0};
    for (size_t i = 0; i + STRASSEN_REC <= plan.size(); i += STRASSEN_REC)
        if (plan[i] == PLAN_SUM) need[plan[i + 1]] = std::max(need[plan[i + 1]], (size_t)plan[i + 2] * (size_t)plan[i + 3]);
    return need[0] + need[1];
}

// 0: classical only, 1: one level (bit for bit what the tree did before the outer level existed), 2: both at the library's
// thresholds everywhere (bit for bit the tree before the recursion had thresholds of its own); unset: both, and the recursive
// factorisation plans each of its products with its own thresholds (strassen_rec_values)
int strassen_levels()
{
    static const int lv = [] { const char *e = getenv("SGPR_GEMM_STRASSEN"); return !e ? 2 : (e[0] == '0' ? 0 : (e[0] == '1' ? 1 : 2)); }();
    return lv;
}
bool strassen_on() { return strassen_levels() > 0; }
// Default threshold: profiles/strassen/sweep.txt.  Tunables "gemm_strassen_min" (half-size of m and n; k: half of it),
// "gemm_strassen_kslab", "gemm_strassen_noscratch" (tests: the scratch allocation is reported as failed).
PlanCfg default_cfg()
{
    static const long smin = std::max(128L, (long)tune("gemm_strassen_min", 8192));
    static const long kslab = std::max(32L, (long)tune("gemm_strassen_kslab", 16384));
    return PlanCfg{smin, kslab, ~(size_t)0};
}

// ---- the outer level: one more Strassen level AROUND the plan above -----------------------------------
// The same seven formulas on the halves of the largest products; each outer product M_i = X Y^T (X, Y a raw block or an outer
// operand sum) is not a launch but a call of the inner level with a PAIR of destinations: the blocks of C that M_i goes to, each
// with its sign.  The inner plan of M_i is strassen_plan(m / 2, n / 2, kslab2 / 2) as it stands; run_plan turns its records into
// launches with twice the destinations (a product for two quadrants of M_i accumulates into four blocks of C).
// The outer list holds the inner level's records unchanged wherever the outer level does not apply (a call that does not
// qualify at all gives exactly strassen_plan's list), plus two kinds of its own with the layouts of PLAN_SUM / PLAN_PROD:
//   PLAN2_SUM   outer scratch of that side = X + sign Y
//   PLAN2_PROD  operands: raw block or the OUTER scratch; [7] [8] [9] the half-size extents; destinations as in PLAN_PROD
// k: whole slabs of exactly kslab2 columns take the outer level; a remainder shorter than that goes through plan_gemm.
struct Plan2Cfg {
    PlanCfg in;     // the inner level (its scratch member is not used here)
    long smin2;     // smallest half-size of m and n that takes the outer level
    long kslab2;    // its k slab: exactly this many columns, a multiple of 64 (quarters stay multiples of the k-step)
    size_t scratch; // doubles available for the inner and the outer pair together
    long smin_under = -1;   // the inner threshold UNDER an outer product (negative: in.smin); the recursion's calls set it
};
// the inner level as it holds under an outer product (its scratch member is the caller's business)
PlanCfg under_of(const Plan2Cfg &c)
{
    PlanCfg ci = c.in;
    if (c.smin_under >= 0) ci.smin = c.smin_under;
    return ci;
}
// the recursion's shipped values (strassen_rec_values below)
constexpr long REC_SMIN_GEMM = 4096, REC_SMIN_SYRK = 8192, REC_SMIN2_GEMM = 8192, REC_SMIN2_SYRK = 8192, REC_KSLAB2_SHORT = 16384;
// Default thresholds: profiles/strassen2/sweep.txt.  Tunables "gemm_strassen2_min", "gemm_strassen2_kslab",
// "gemm_strassen2_noscratch" (tests: the allocation of the outer part is reported as failed -> one level).
Plan2Cfg default_cfg2()
{
    static const long smin2 = std::max(256L, (long)tune("gemm_strassen2_min", 16384));
    static const long kslab2 = std::max(64L, (long)tune("gemm_strassen2_kslab", 32768));
    return Plan2Cfg{default_cfg(), smin2, kslab2, ~(size_t)0};
}
bool outer_noscratch()
{
    static const bool forced_fail = tune("gemm_strassen2_noscratch", 0) != 0;
    return forced_fail;
}
bool qualifies2(long m, long n, long k, const Plan2Cfg &c)
{
    // halves multiples of 512 x 256: the quarters stay multiples of the tile
    if (m <= 0 || n <= 0 || m % 1024 != 0 || n % 512 != 0) return false;
    if (m / 2 < c.smin2 || n / 2 < c.smin2) return false;
    if (c.kslab2 < 64 || c.kslab2 % 64 != 0 || k < c.kslab2) return false;
    const size_t pair = (size_t)(m / 2 + n / 2) * (size_t)(c.kslab2 / 2);
    if (pair > c.scratch) return false;
    // ... and everything the inner level asks of an outer product, with the scratch that is left
    PlanCfg ci = under_of(c);
    ci.scratch = c.scratch - pair;
    return qualifies(m / 2, n / 2, c.kslab2 / 2, ci);
}
PlanCfg inner_of(const Plan2Cfg &c)
{
    PlanCfg ci = c.in;
    ci.scratch = c.scratch;
    return ci;
}
void plan2_gemm(long m, long n, long k, long ar, long br, long cr, long cc, const Plan2Cfg &c, std::vector<long long> &out)
{
    if (!qualifies2(m, n, k, c)) { plan_gemm(m, n, k, ar, br, cr, cc, inner_of(c), out); return; }
    long k0 = 0;
    for (; k0 + c.kslab2 <= k; k0 += c.kslab2) seven(PLAN2_SUM, PLAN2_PROD, m / 2, n / 2, c.kslab2 / 2, k0, ar, br, cr, cc, out);
    if (k0 == k) return;
    // the remainder of k through the inner level alone; plan_gemm counts k columns from 0: move its records to k0
    size_t i = out.size();
    plan_gemm(m, n, k - k0, ar, br, cr, cc, inner_of(c), out);
    for (; i + STRASSEN_REC <= out.size(); i += STRASSEN_REC) {
        long long *r = &out[i];
        if (r[0] == PLAN_SUM) { r[5] += k0; r[7] += k0; }
        else if (r[0] == PLAN_PROD) { if (!r[1]) r[3] += k0; if (!r[4]) r[6] += k0; }
        else { r[3] += k0; r[5] += k0; }
    }
}
// lower update: the split around the off-diagonal square happens at the outer level first
void plan2_syrk(long n, long k, long r0, const Plan2Cfg &c, std::vector<long long> &out)
{
    const long h = n / 2;
    if (n % 2 != 0 || !qualifies2(h, h, k, c)) { plan_syrk(n, k, r0, inner_of(c), out); return; }
    plan2_syrk(h, k, r0, c, out);
    plan2_gemm(h, h, k, r0 + h, r0, r0 + h, r0, c, out);
    plan2_syrk(h, k, r0 + h, c, out);
}
// the inner plan of one outer product (no offsets: its operands and destinations are passed as pointers)
void inner_plan(const long long *r, const PlanCfg &ci, std::vector<long long> &out)
{
    out.clear();
    plan_gemm(r[7], r[8], r[9], 0, 0, 0, 0, ci, out);
}
// doubles of scratch per region: inner A side, inner B side, outer A side, outer B side
struct Need2 { size_t v[4] = {0, 0, 0, 0}; size_t inner() const { return v[0] + v[1]; } size_t total() const { return v[0] + v[1] + v[2] + v[3]; } };
Need2 plan2_need(const std::vector<long long> &plan, const Plan2Cfg &c)
{
    Need2 nd;
    std::vector<long long> in;
    auto sums = [&](const long long *r, int base) {
        size_t &v = nd.v[base + r[1]];
        v = std::max(v, (size_t)r[2] * (size_t)r[3]);
    };
    PlanCfg ci = under_of(c);
    ci.scratch = ~(size_t)0;
    for (size_t i = 0; i + STRASSEN_REC <= plan.size(); i += STRASSEN_REC) {
        const long long *r = &plan[i];
        if (r[0] == PLAN_SUM) sums(r, 0);
        else if (r[0] == PLAN2_SUM) sums(r, 2);
        else if (r[0] == PLAN2_PROD) {
            inner_plan(r, ci, in);
            for (size_t j = 0; j + STRASSEN_REC <= in.size(); j += STRASSEN_REC)
                if (in[j] == PLAN_SUM) sums(&in[j], 0);
        }
    }
    return nd;
}

// Scratch of the operand sums: one buffer per device, owned by the library, grown to the largest qualifying call and
// released by strassen_trim().  Calls are serialised by the mutex while they ENQUEUE; on the device a call on another
// stream first waits for the event the previous user recorded behind its last product.
struct Scratch {
    std::mutex mu;
    double *p = nullptr;
    size_t cap = 0, failed = 0;     // doubles; smallest request that could not be allocated (0: none)
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;
    bool used = false;
    std::vector<hipEvent_t> pool;   // events of the overlapped execution (run_schedule), timing disabled, created on demand
};
Scratch g_scratch[64];

bool scratch_ensure(Scratch &s, size_t need)
{
    static const bool forced_fail = tune("gemm_strassen_noscratch", 0) != 0;
    if (forced_fail) return false;
    if (s.cap >= need) return true;
    if (s.failed && need >= s.failed) return false;
    if (s.p) { (void)hipFree(s.p); s.p = nullptr; s.cap = 0; s.used = false; }   // hipFree waits for the device
    if (hipMalloc((void **)&s.p, need * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        s.p = nullptr;
        s.failed = need;
        return false;
    }
    s.cap = need;
    return true;
}
int device_of(hipStream_t st)
{
    int dev = -1;
    if ((st ? hipStreamGetDevice(st, &dev) : hipGetDevice(&dev)) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return (dev >= 0 && dev < 64) ? dev : -1;
}

constexpr long SUM_WGS = 2048;     // most workgroups of one sum (the kernel strides over its pieces)
int block_sum(int rows, int cols, const double *X, size_t ldx, const double *Y, size_t ldy, double sign, double *T, hipStream_t st,
              long wgs = SUM_WGS)
{
    const long pieces = (long)((rows + 511) / 512) * ((cols + 3) / 4);
    hipLaunchKernelGGL(block_sum_kernel, dim3((unsigned)std::min(pieces, wgs)), dim3(256), 0, st, rows, cols, X, ldx, Y, ldy, sign, T);
    SGPR_CHECK_LAUNCH();
    return 0;
}

// Execute nrec inner-level records.  C2 == nullptr: C = beta C + alpha A B^T, one launch per record as the list says.
// C2 != nullptr (the records are the inner plan of an outer product): the same product also goes to C2 with factor alpha2 --
// a PLAN_PROD record with two destinations becomes a four-destination launch, one with one destination and a PLAN_CLASSIC
// record a two-destination launch.
int run_plan(const long long *recs, size_t nrec, double alpha, const double *A, size_t lda, const double *B, size_t ldb,
             double beta, double *C, size_t ldc, double alpha2, double *C2, size_t ldc2, double *SA, double *SB, hipStream_t st,
             long sum_wgs = SUM_WGS)
{
    for (size_t i = 0; i < nrec; ++i) {
        const long long *r = recs + i * STRASSEN_REC;
        int rc = 0;
        if (r[0] == PLAN_SUM) {
            const double *P = r[1] ? B : A;
            const size_t ld = r[1] ? ldb : lda;
            rc = block_sum((int)r[2], (int)r[3], P + r[4] + (size_t)r[5] * ld, ld, P + r[6] + (size_t)r[7] * ld, ld, (double)r[8],
                           r[1] ? SB : SA, st, sum_wgs);
        } else if (r[0] == PLAN_PROD) {
            const int m = (int)r[7], n = (int)r[8], k = (int)r[9];
            const double *Ap = r[1] ? SA : A + r[2] + (size_t)r[3] * lda;
            const double *Bp = r[4] ? SB : B + r[5] + (size_t)r[6] * ldb;
            const size_t la = r[1] ? (size_t)m : lda, lb = r[4] ? (size_t)n : ldb;
            double *C1 = C + r[10] + (size_t)r[11] * ldc;
            if (C2) {
                double *cs[4] = {C1, nullptr, nullptr, nullptr};
                size_t ls[4] = {ldc, 0, 0, 0};
                double as[4] = {alpha * (double)r[12], 0.0, 0.0, 0.0};
                int cnt = 1;
                auto add = [&](double *p, size_t l, double a) { cs[cnt] = p; ls[cnt] = l; as[cnt] = a; ++cnt; };
                if (r[15]) add(C + r[13] + (size_t)r[14] * ldc, ldc, alpha * (double)r[15]);
                add(C2 + r[10] + (size_t)r[11] * ldc2, ldc2, alpha2 * (double)r[12]);
                if (r[15]) add(C2 + r[13] + (size_t)r[14] * ldc2, ldc2, alpha2 * (double)r[15]);
                if (cnt == 2) rc = gemm_nt_two(m, n, k, as[0], Ap, la, Bp, lb, 1.0, cs[0], ls[0], as[1], cs[1], ls[1], st);
                else          rc = gemm_nt_multi(m, n, k, Ap, la, Bp, lb, 1.0, cnt, cs, ls, as, st);
            } else if (r[15]) {
                rc = gemm_nt_two(m, n, k, alpha * (double)r[12], Ap, la, Bp, lb, 1.0, C1, ldc,
                                 alpha * (double)r[15], C + r[13] + (size_t)r[14] * ldc, ldc, st);
            } else {
                rc = gemm_nt(m, n, k, alpha * (double)r[12], Ap, la, Bp, lb, 1.0, C1, ldc, 0, 0, st);
            }
        } else if (r[0] == PLAN_CLASSIC) {
            const double *Ap = A + r[2] + (size_t)r[3] * lda, *Bp = B + r[4] + (size_t)r[5] * ldb;
            if (C2) rc = gemm_nt_two((int)r[6], (int)r[7], (int)r[8], alpha, Ap, lda, Bp, ldb, beta, C + r[9] + (size_t)r[10] * ldc, ldc,
                                     alpha2, C2 + r[9] + (size_t)r[10] * ldc2, ldc2, st);
            else    rc = gemm_nt((int)r[6], (int)r[7], (int)r[8], alpha, Ap, lda, Bp, ldb, beta, C + r[9] + (size_t)r[10] * ldc, ldc, (int)r[1], 0, st);
        } else {
            set_error("run_plan: unknown record");
            rc = SGPR_E_ARG;
        }
        if (rc) return rc;
    }
    return 0;
}
int run_plan(const std::vector<long long> &plan, double alpha, const double *A, size_t lda, const double *B, size_t ldb,
             double beta, double *C, size_t ldc, double *SA, double *SB, hipStream_t st)
{
    return run_plan(plan.data(), plan.size() / STRASSEN_REC, alpha, A, lda, B, ldb, beta, C, ldc, 0.0, nullptr, 0, SA, SB, st);
}
// Execute an outer list: S = the scratch buffer, laid out as [inner A | inner B | outer A | outer B] with the sizes of nd
int run_plan2(const std::vector<long long> &plan, const Plan2Cfg &c, const Need2 &nd, double alpha, const double *A, size_t lda,
              const double *B, size_t ldb, double beta, double *C, size_t ldc, double *S, hipStream_t st)
{
    double *const SA = S, *const SB = S + nd.v[0], *const OA = SB + nd.v[1], *const OB = OA + nd.v[2];
    PlanCfg ci = under_of(c);
    ci.scratch = nd.inner();
    std::vector<long long> in;
    for (size_t i = 0; i + STRASSEN_REC <= plan.size(); i += STRASSEN_REC) {
        const long long *r = &plan[i];
        int rc = 0;
        if (r[0] == PLAN2_SUM) {
            const double *P = r[1] ? B : A;
            const size_t ld = r[1] ? ldb : lda;
            rc = block_sum((int)r[2], (int)r[3], P + r[4] + (size_t)r[5] * ld, ld, P + r[6] + (size_t)r[7] * ld, ld, (double)r[8],
                           r[1] ? OB : OA, st);
        } else if (r[0] == PLAN2_PROD) {
            const double *X = r[1] ? OA : A + r[2] + (size_t)r[3] * lda;
            const double *Y = r[4] ? OB : B + r[5] + (size_t)r[6] * ldb;
            inner_plan(r, ci, in);
            rc = run_plan(in.data(), in.size() / STRASSEN_REC, alpha * (double)r[12], X, r[1] ? (size_t)r[7] : lda, Y, r[4] ? (size_t)r[8] : ldb,
                          1.0, C + r[10] + (size_t)r[11] * ldc, ldc, alpha * (double)r[15], r[15] ? C + r[13] + (size_t)r[14] * ldc : nullptr, ldc,
                          SA, SB, st);
        } else {
            rc = run_plan(r, 1, alpha, A, lda, B, ldb, beta, C, ldc, 0.0, nullptr, 0, SA, SB, st);
        }
        if (rc) return rc;
    }
    return 0;
}

// ---- the operand sums beside the products -------------------------------------------------------------
// The sums are HBM streaming, the products MFMA-bound; a sum needs neither LDS nor more registers than two product waves per
// SIMD leave.  So a list can be executed with its sums on a low-priority side stream, each under the product before the one
// that needs it.  Again the decision is host code that emits records and the device path executes exactly those:
// schedule_of turns a list into a SCHEDULE -- the same records in the same order, the inner plan of every outer product expanded
// behind it the way run_plan2 expands it, each record annotated (SCHED_REC words):
//   [0 .. 15] the record   [16] level: 0 a record of the list, 1 a record of the inner plan of the outer product before it
//   [17] stream: 0 the caller's (products, classical launches, the outer-product headers, which launch nothing), 1 / 2 a side stream
//   [18] a sum: the buffer of its region it writes; a product: the buffer of the A-side scratch it reads (-1: a raw block) --
//        PLAN_PROD the inner A region, PLAN2_PROD the outer one (its inner records read THAT buffer where they read "A")
//   [19] a product: likewise for the B side (-1 otherwise)   [20] number of waits   [21 ...] the records it waits for
// Regions: inner A, inner B, outer A, outer B, each with one buffer or two; the sums of a region alternate between its buffers.
// Edges: a product waits for the sums whose buffers it reads; a sum waits for the last product that read the buffer it overwrites
// (one buffer per region already lets the B sum of M3 run under M2, which reads the A scratch and a raw B block); an inner sum
// or product that reads an outer buffer waits for the outer sum that wrote it; an outer sum waits for the last inner sum of each
// side stream and the last inner product that read the buffer it overwrites.  "The last" is enough because a stream runs its
// records in order; every wait points backwards in the list, so the host records an event before it enqueues a wait on it.
// tests/test_strassen_overlap_cpu.py replays schedules in numpy in every order these edges allow.
struct SchedCfg {
    int nbuf[4] = {1, 1, 1, 1};     // buffers per region
    size_t off[4][2] = {};          // their offsets in the scratch: the pinned layout first, second buffers behind it
    int nstreams = 1;               // side streams: 1, or 2 = one per operand side
};
// Second buffers come out of the SLACK of the scratch (capacity - the call's need, capped by the tunable
// "gemm_strassen_overlap_slack": < 0 all of it, 0 none), in the order inner A, inner B, outer A, outer B while it lasts.
// Tunable "gemm_strassen_overlap_streams": 2 = the sums of the B side on a side stream of their own.
SchedCfg sched_cfg_of(const Need2 &nd, size_t cap)
{
    SchedCfg sc;
    sc.nstreams = tune("gemm_strassen_overlap_streams", 1) >= 2 ? 2 : 1;
    const double lim = tune("gemm_strassen_overlap_slack", -1);
    size_t slack = cap > nd.total() ? cap - nd.total() : 0, pos = 0;
    if (lim >= 0) slack = std::min(slack, (size_t)lim);
    for (int r = 0; r < 4; ++r) { sc.off[r][0] = pos; pos += nd.v[r]; }
    for (int r = 0; r < 4; ++r) {
        if (!nd.v[r]) continue;
        if (nd.v[r] > slack) break;
        sc.nbuf[r] = 2; sc.off[r][1] = pos; pos += nd.v[r]; slack -= nd.v[r];
    }
    return sc;
}
void schedule_of(const std::vector<long long> &plan, const Plan2Cfg &c, const Need2 &nd, const SchedCfg &sc, std::vector<long long> &out)
{
    struct Buf { long long writer = -1, prod_reader = -1, sum_reader[2] = {-1, -1}; };
    Buf buf[4][2];
    int next[4] = {0, 0, 0, 0}, cur[4] = {0, 0, 0, 0};
    out.clear();
    auto emit = [&](const long long *r, int level) {
        const size_t at = out.size();
        out.resize(at + SCHED_REC, 0);
        for (int j = 0; j < STRASSEN_REC; ++j) out[at + j] = r[j];
        out[at + 16] = level; out[at + 18] = out[at + 19] = -1;
        return at;
    };
    auto wait = [&](size_t at, long long idx) {
        if (idx < 0) return;
        const int nw = (int)out[at + 20];
        for (int j = 0; j < nw; ++j) if (out[at + 21 + j] == idx) return;
        if (nw < SCHED_REC - 21) { out[at + 21 + nw] = idx; out[at + 20] = nw + 1; }   // (at most 4 by construction)
    };
    // record `at` reads buffer b of region rg as an operand of a launch on the caller's stream
    auto read = [&](size_t at, int rg, int b) {
        wait(at, buf[rg][b].writer);
        buf[rg][b].prod_reader = (long long)(at / SCHED_REC);
    };
    // a sum into region rg; src >= 0: its operand is buffer sb of (outer) region src
    auto sum = [&](const long long *r, int level, int rg, int src, int sb) {
        const size_t at = emit(r, level);
        const long long idx = (long long)(at / SCHED_REC);
        const int stream = sc.nstreams == 2 ? 1 + (int)r[1] : 1, b = next[rg];
        next[rg] = (b + 1) % sc.nbuf[rg];
        Buf &t = buf[rg][b];
        wait(at, t.prod_reader); wait(at, t.sum_reader[0]); wait(at, t.sum_reader[1]);
        if (!out[at + 20]) wait(at, t.writer);
        if (src >= 0) { wait(at, buf[src][sb].writer); buf[src][sb].sum_reader[stream - 1] = idx; }
        t = Buf{};
        t.writer = idx;
        cur[rg] = b;
        out[at + 17] = stream; out[at + 18] = b;
    };
    PlanCfg ci = under_of(c);
    ci.scratch = nd.inner();
    std::vector<long long> in;
    for (size_t i = 0; i + STRASSEN_REC <= plan.size(); i += STRASSEN_REC) {
        const long long *r = &plan[i];
        if (r[0] == PLAN_SUM || r[0] == PLAN2_SUM) {
            sum(r, 0, (r[0] == PLAN2_SUM ? 2 : 0) + (int)r[1], -1, 0);
        } else if (r[0] == PLAN_PROD) {
            const size_t at = emit(r, 0);
            if (r[1]) { out[at + 18] = cur[0]; read(at, 0, cur[0]); }
            if (r[4]) { out[at + 19] = cur[1]; read(at, 1, cur[1]); }
        } else if (r[0] == PLAN2_PROD) {
            const size_t hd = emit(r, 0);
            const int xa = r[1] ? cur[2] : -1, yb = r[4] ? cur[3] : -1;     // the outer buffers its inner records read as A, B
            out[hd + 18] = xa; out[hd + 19] = yb;
            inner_plan(r, ci, in);
            for (size_t j = 0; j + STRASSEN_REC <= in.size(); j += STRASSEN_REC) {
                const long long *q = &in[j];
                if (q[0] == PLAN_SUM) {
                    const int ob = q[1] ? yb : xa;
                    sum(q, 1, (int)q[1], ob >= 0 ? 2 + (int)q[1] : -1, std::max(ob, 0));
                    continue;
                }
                const size_t at = emit(q, 1);
                const bool a_scr = q[0] == PLAN_PROD && q[1], b_scr = q[0] == PLAN_PROD && q[4];
                if (a_scr) { out[at + 18] = cur[0]; read(at, 0, cur[0]); } else if (xa >= 0) read(at, 2, xa);
                if (b_scr) { out[at + 19] = cur[1]; read(at, 1, cur[1]); } else if (yb >= 0) read(at, 3, yb);
            }
        } else {
            (void)emit(r, 0);       // a classical launch: raw blocks only
        }
    }
}

// On by default: n = 131 072 step 9303.1 / 9309.6 -> 9135.5 / 9137.6 ms (profiles/strassen_overlap/step.txt).  0: everything on the
// caller's stream in list order (run_plan / run_plan2).
bool overlap_on() { return tune("gemm_strassen_overlap", 1) != 0; }
// Workgroups of a side-stream sum: one per CU, so that ONE sum wave (40 registers) sits beside the two product waves of a SIMD,
// which leave 64 or 48 of 512; a second one (80) would keep the next product workgroup off that CU until the sums have drained.
// Measured in the step (sweep.txt): 256 -1.8 %, 512 and 2048 (one launch's grid on the caller's stream) 0 ... -0.6 %.
constexpr long SUM_WGS_SIDE = 256;

// Execute a list through its schedule: S = the scratch (s.p), laid out by sc.  At entry the side streams wait for everything that
// is on the caller's stream (the operands may have been written by the launches just before the call, and the scratch is
// whoever used it last until the wait on Scratch::ev in front of this); every sum is consumed by a product of the caller's
// stream, and on EVERY return, an error part-way through included, the caller's stream waits for the side streams once more:
// the scratch may be reused or freed next.  All waits of a product are enqueued before gemm_nt* is called, so the start event of
// an open profile window (gemm_launch) lies behind them.  Tunable "gemm_strassen_sum_wgs": most workgroups of a sum.
int run_schedule(const std::vector<long long> &plan, const Plan2Cfg &c, const Need2 &nd, double alpha, const double *A, size_t lda,
                 const double *B, size_t ldb, double beta, double *C, size_t ldc, Scratch &s, hipStream_t st)
{
    const SchedCfg sc = sched_cfg_of(nd, s.cap);
    std::vector<long long> sch;
    schedule_of(plan, c, nd, sc, sch);
    const size_t nrec = sch.size() / SCHED_REC;
    const long wgs = std::min(65535L, std::max(1L, (long)tune("gemm_strassen_sum_wgs", (double)SUM_WGS_SIDE)));
    hipStream_t str[3] = {st, nullptr, nullptr};
    int rc = strassen_sum_streams(st, sc.nstreams, str + 1);
    if (rc) return rc;
    // events: [0 .. nstreams) entry and exit, 2 + i behind record i where a record of another stream waits for it
    std::vector<char> needs(nrec, 0);
    for (size_t i = 0; i < nrec; ++i) {
        const long long *q = &sch[i * SCHED_REC];
        for (int j = 0; j < (int)q[20]; ++j)
            if (sch[(size_t)q[21 + j] * SCHED_REC + 17] != q[17]) needs[(size_t)q[21 + j]] = 1;
    }
    if (s.pool.size() < nrec + 2) s.pool.resize(nrec + 2, nullptr);
    auto event = [&](size_t i) {
        if (!s.pool[i]) SGPR_HIP(hipEventCreateWithFlags(&s.pool[i], hipEventDisableTiming));
        return 0;
    };
    if ((rc = event(0)) || (rc = event(1))) return rc;
    SGPR_HIP(hipEventRecord(s.pool[0], st));
    for (int t = 1; t <= sc.nstreams; ++t) SGPR_HIP(hipStreamWaitEvent(str[t], s.pool[0], 0));
    struct Join {
        hipStream_t *str; int n; hipEvent_t *ev;
        ~Join()
        {
            for (int t = 1; t <= n; ++t)
                if (hipEventRecord(ev[t - 1], str[t]) != hipSuccess || hipStreamWaitEvent(str[0], ev[t - 1], 0) != hipSuccess) {
                    (void)hipGetLastError();
                    (void)hipStreamSynchronize(str[t]);
                }
        }
    } join{str, sc.nstreams, s.pool.data()};
    auto at = [&](int rg, long long b) { return s.p + sc.off[rg][b < 0 ? 0 : b]; };
    const long long *hd = nullptr;      // the outer product whose inner records are running
    for (size_t i = 0; i < nrec; ++i) {
        const long long *q = &sch[i * SCHED_REC];
        hipStream_t me = str[q[17]];
        for (int j = 0; j < (int)q[20]; ++j) {
            const size_t w = (size_t)q[21 + j];
            if (sch[w * SCHED_REC + 17] != q[17]) SGPR_HIP(hipStreamWaitEvent(me, s.pool[2 + w], 0));
        }
        if (q[0] == PLAN2_PROD) {
            hd = q;
            continue;
        }
        if (q[0] == PLAN2_SUM) {
            const double *P = q[1] ? B : A;
            const size_t ld = q[1] ? ldb : lda;
            rc = block_sum((int)q[2], (int)q[3], P + q[4] + (size_t)q[5] * ld, ld, P + q[6] + (size_t)q[7] * ld, ld, (double)q[8],
                           at(2 + (int)q[1], q[18]), me, wgs);
        } else if (q[16] == 0) {
            // a sum's [18] is the buffer it writes, a product's [18] / [19] the buffers it reads
            rc = run_plan(q, 1, alpha, A, lda, B, ldb, beta, C, ldc, 0.0, nullptr, 0, at(0, q[0] == PLAN_SUM && q[1] ? 0 : q[18]),
                          at(1, q[0] == PLAN_SUM ? q[18] : q[19]), me, wgs);
        } else {
            const long long *r = hd;
            const double *X = r[1] ? at(2, r[18]) : A + r[2] + (size_t)r[3] * lda;
            const double *Y = r[4] ? at(3, r[19]) : B + r[5] + (size_t)r[6] * ldb;
            rc = run_plan(q, 1, alpha * (double)r[12], X, r[1] ? (size_t)r[7] : lda, Y, r[4] ? (size_t)r[8] : ldb, 1.0,
                          C + r[10] + (size_t)r[11] * ldc, ldc, alpha * (double)r[15], r[15] ? C + r[13] + (size_t)r[14] * ldc : nullptr, ldc,
                          at(0, q[0] == PLAN_SUM && q[1] ? 0 : q[18]), at(1, q[0] == PLAN_SUM ? q[18] : q[19]), me, wgs);
        }
        if (rc) return rc;
        if (needs[i]) {
            if ((rc = event(2 + i))) return rc;
            SGPR_HIP(hipEventRecord(s.pool[2 + i], me));
        }
    }
    return 0;
}
}  // namespace

// the plan of one call as the host decides it (no device): smin / kslab < 0 = the built-in values or tunables
int strassen_plan(int m, int n, int k, int lower, long smin, long kslab, size_t scratch_doubles, std::vector<long long> &out)
{
    if (m < 0 || n < 0 || k < 0 || (lower && m != n)) { set_error("strassen_plan: bad extents"); return SGPR_E_ARG; }
    PlanCfg c = default_cfg();
    if (smin >= 0) c.smin = std::max(128L, smin);
    if (kslab >= 0) c.kslab = std::max(32L, kslab);
    c.scratch = scratch_doubles;
    out.clear();
    if (lower) plan_syrk(n, k, 0, c, out);
    else       plan_gemm(m, n, k, 0, 0, 0, 0, c, out);
    return 0;
}

namespace {
Plan2Cfg cfg2_of(long smin, long kslab, long smin2, long kslab2, size_t scratch_doubles)
{
    Plan2Cfg c = default_cfg2();
    if (smin >= 0) c.in.smin = std::max(128L, smin);
    if (kslab >= 0) c.in.kslab = std::max(32L, kslab);
    if (smin2 >= 0) c.smin2 = std::max(256L, smin2);
    if (kslab2 >= 0) c.kslab2 = std::max(64L, kslab2);
    c.scratch = scratch_doubles;
    return c;
}
Plan2Cfg cfg2_of(const StrassenCfg &cfg, size_t scratch_doubles)
{
    Plan2Cfg c = cfg2_of(cfg.smin, cfg.kslab, cfg.smin2, cfg.kslab2, scratch_doubles);
    if (cfg.smin_under >= 0) c.smin_under = std::max(128L, cfg.smin_under);
    return c;
}
void outer_plan_of(int m, int n, int k, int lower, const Plan2Cfg &c, std::vector<long long> &out)
{
    out.clear();
    if (lower) plan2_syrk(n, k, 0, c, out);
    else       plan2_gemm(m, n, k, 0, 0, 0, 0, c, out);
}
}  // namespace

// ... and the list with the outer level around it (smin2 / kslab2 < 0 = the built-in values or tunables)
int strassen_outer_plan(int m, int n, int k, int lower, long smin, long kslab, long smin2, long kslab2, size_t scratch_doubles,
                   std::vector<long long> &out)
{
    if (m < 0 || n < 0 || k < 0 || (lower && m != n)) { set_error("strassen_outer_plan: bad extents"); return SGPR_E_ARG; }
    outer_plan_of(m, n, k, lower, cfg2_of(smin, kslab, smin2, kslab2, scratch_doubles), out);
    return 0;
}

// The recursion's values.  Tunables "rec_strassen_min_gemm" / "rec_strassen_min_syrk" (inner threshold of trsm_rec's products /
// of the lower updates), "rec_strassen2_min_gemm" / "rec_strassen2_min_syrk" (outer threshold), "rec_strassen2_kslab_short" (outer
// k slab of a call whose k is below the long one; 0: none), "rec_strassen_kslab" / "rec_strassen2_kslab" (inner and long outer
// k slab: the library's unless set).  Read at every factorisation, not once per process.
// Defaults: profiles/strassen_rec/sweep.txt, class by class.  SGPR_GEMM_STRASSEN set to anything: the library's.
StrassenRec strassen_rec_values()
{
    StrassenRec v;
    v.on = getenv("SGPR_GEMM_STRASSEN") == nullptr;
    const Plan2Cfg lib = default_cfg2();
    // (a library threshold lowered below the recursion's own -- tests at small orders do that -- holds for the recursion too)
    v.smin_gemm = std::max(128L, (long)tune("rec_strassen_min_gemm", std::min(REC_SMIN_GEMM, lib.in.smin)));
    v.smin_syrk = std::max(128L, (long)tune("rec_strassen_min_syrk", std::min(REC_SMIN_SYRK, lib.in.smin)));
    v.smin2_gemm = std::max(256L, (long)tune("rec_strassen2_min_gemm", std::min(REC_SMIN2_GEMM, lib.smin2)));
    v.smin2_syrk = std::max(256L, (long)tune("rec_strassen2_min_syrk", std::min(REC_SMIN2_SYRK, lib.smin2)));
    v.kslab = std::max(32L, (long)tune("rec_strassen_kslab", lib.in.kslab));
    v.kslab2 = std::max(64L, (long)tune("rec_strassen2_kslab", lib.kslab2));
    v.kslab2_short = (long)tune("rec_strassen2_kslab_short", REC_KSLAB2_SHORT);
    if (v.kslab2_short < 64 || v.kslab2_short % 64 != 0 || v.kslab2_short >= v.kslab2) v.kslab2_short = 0;
    return v;
}
// One call's thresholds: k at least the library's outer slab keeps that slab (measured two points better on the two largest
// products, profiles/strassen2/sweep.txt); a shorter k that holds a whole short slab takes the short one.  Under an outer
// product the inner level applies wherever the outer threshold let the product in: min(smin, smin2 / 2).
StrassenCfg strassen_rec_cfg(const StrassenRec &v, int k, int lower)
{
    StrassenCfg c;
    if (!v.on) return c;
    c.smin = lower ? v.smin_syrk : v.smin_gemm;
    c.smin2 = lower ? v.smin2_syrk : v.smin2_gemm;
    c.smin_under = std::min(c.smin, c.smin2 / 2);
    c.kslab = v.kslab;
    c.kslab2 = (k < v.kslab2 && v.kslab2_short > 0 && k >= v.kslab2_short) ? v.kslab2_short : v.kslab2;
    return c;
}
int strassen_rec_plan(int m, int n, int k, int lower, long cfg_out[5], size_t scratch_doubles, std::vector<long long> &out)
{
    if (m < 0 || n < 0 || k < 0 || (lower && m != n)) { set_error("strassen_rec_plan: bad extents"); return SGPR_E_ARG; }
    const Plan2Cfg c = cfg2_of(strassen_rec_cfg(strassen_rec_values(), k, lower), scratch_doubles);
    if (cfg_out) { cfg_out[0] = c.in.smin; cfg_out[1] = c.in.kslab; cfg_out[2] = c.smin2; cfg_out[3] = c.kslab2; cfg_out[4] = under_of(c).smin; }
    outer_plan_of(m, n, k, lower, c, out);
    return 0;
}

// The schedule of that call (schedule_of) for a scratch buffer of cap_doubles: the list as gemm_nt_strassen_cfg plans it with
// the scratch it needs (both levels, as far as SGPR_GEMM_STRASSEN allows).  info: [0 .. 3] doubles per region (inner A, inner B,
// outer A, outer B), [4 .. 7] buffers per region, [8] side streams, [9] the capacity.  A capacity below the need is an error.
int strassen_schedule(int m, int n, int k, int lower, long long cap_doubles, long long info[12], std::vector<long long> &out)
{
    if (m < 0 || n < 0 || k < 0 || (lower && m != n)) { set_error("strassen_schedule: bad extents"); return SGPR_E_ARG; }
    const Plan2Cfg c = cfg2_of(strassen_rec_cfg(strassen_rec_values(), k, lower), ~(size_t)0);
    std::vector<long long> plan;
    if (strassen_levels() >= 2 && !outer_noscratch()) outer_plan_of(m, n, k, lower, c, plan);
    else {
        const int rc = strassen_plan(m, n, k, lower, c.in.smin, c.in.kslab, ~(size_t)0, plan);
        if (rc) return rc;
    }
    const Need2 nd = plan2_need(plan, c);
    const size_t cap = cap_doubles < 0 ? nd.total() : (size_t)cap_doubles;
    if (cap < nd.total()) { set_error("strassen_schedule: the capacity is below the call's need"); return SGPR_E_ARG; }
    const SchedCfg sc = sched_cfg_of(nd, cap);
    schedule_of(plan, c, nd, sc, out);
    if (info) {
        for (int i = 0; i < 12; ++i) info[i] = 0;
        for (int r = 0; r < 4; ++r) { info[r] = (long long)nd.v[r]; info[4 + r] = sc.nbuf[r]; }
        info[8] = sc.nstreams; info[9] = (long long)cap;
    }
    return 0;
}

// scratch of one call: levels = 1 the inner pair alone, 2 both pairs (as far as SGPR_GEMM_STRASSEN allows)
size_t strassen_scratch_doubles(int m, int n, int k, int lower, int levels)
{
    return strassen_scratch_doubles_cfg(m, n, k, lower, levels, StrassenCfg{});
}
size_t strassen_scratch_doubles_cfg(int m, int n, int k, int lower, int levels, const StrassenCfg &cfg)
{
    std::vector<long long> plan;
    if (!strassen_on() || m < 0 || n < 0 || k < 0 || (lower && m != n)) return 0;
    const Plan2Cfg c2 = cfg2_of(cfg, ~(size_t)0);
    if (levels >= 2 && strassen_levels() >= 2) {
        outer_plan_of(m, n, k, lower, c2, plan);
        return plan2_need(plan, c2).total();
    }
    if (strassen_plan(m, n, k, lower, c2.in.smin, c2.in.kslab, ~(size_t)0, plan)) return 0;
    return plan_need(plan);
}

// make room for calls that need up to `both` doubles of scratch on st's device (potrf: once, before the first product);
// if that much cannot be had, `one` (what one level needs): the outer level is then skipped call by call
void strassen_reserve(size_t both, size_t one, hipStream_t st)
{
    const int dev = device_of(st);
    if (dev < 0 || !strassen_on()) return;
    Scratch &s = g_scratch[dev];
    std::lock_guard<std::mutex> lock(s.mu);
    if (both > one && !outer_noscratch() && scratch_ensure(s, both)) return;
    if (one) (void)scratch_ensure(s, one);
}

namespace { void top_trim(); }

int strassen_trim()
{
    top_trim();                                   // the top level's buffer (below)
    for (Scratch &s : g_scratch) {
        std::lock_guard<std::mutex> lock(s.mu);
        if (s.p) (void)hipFree(s.p);          // waits for whatever still uses it
        if (s.ev) (void)hipEventDestroy(s.ev);
        for (hipEvent_t e : s.pool) if (e) (void)hipEventDestroy(e);
        s.pool.clear();
        s.p = nullptr; s.ev = nullptr; s.cap = 0; s.failed = 0; s.used = false; s.last = nullptr;
    }
    (void)hipGetLastError();
    return 0;
}

// C = beta C + alpha A B^T (lower: on and below the diagonal of a square C only) through the plans above.  Whatever does
// not qualify -- sizes, alignment, beta != 1, no scratch, SGPR_GEMM_STRASSEN=0 -- is the classical launch, bit for bit;
// without room for the outer pair (or with SGPR_GEMM_STRASSEN=1) the call is the one-level call, bit for bit.
int gemm_nt_strassen(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb, double beta,
                     double *C, size_t ldc, int lower, hipStream_t st)
{
    return gemm_nt_strassen_cfg(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, lower, StrassenCfg{}, st);
}
int gemm_nt_strassen_rec(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb, double beta,
                         double *C, size_t ldc, int lower, hipStream_t st)
{
    return gemm_nt_strassen_cfg(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, lower, strassen_rec_cfg(strassen_rec_values(), k, lower), st);
}
// ... with the thresholds of this one call (the recursive factorisation's calls: chol.hip)
int gemm_nt_strassen_cfg(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb, double beta,
                         double *C, size_t ldc, int lower, const StrassenCfg &cfg, hipStream_t st)
{
    const Plan2Cfg c2 = cfg2_of(cfg, ~(size_t)0);
    const bool aligned = ((((uintptr_t)A | (uintptr_t)B) & 15) == 0) && (((lda | ldb) & 1) == 0);
    // (the size test first: the short products of the panel solves come through here by the thousand)
    if (std::min(m, n) / 2 < std::min(c2.in.smin, under_of(c2).smin) || !strassen_on() || !aligned || beta != 1.0 || (lower && m != n))
        return gemm_nt(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, lower, 0, st);
    std::vector<long long> plan;
    int rc = 0;
    const int dev = device_of(st);
    const bool overlap = overlap_on();      // the sums on a side stream under the products (run_schedule)
    auto enqueue = [&](Scratch &s, auto &&run) {
        if (!s.ev) SGPR_HIP(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
        if (s.used && s.last != st) SGPR_HIP(hipStreamWaitEvent(st, s.ev, 0));
        const int r = run();
        SGPR_HIP(hipEventRecord(s.ev, st));
        s.last = st;
        s.used = true;
        return r;
    };
    // both levels, where a product is large enough for the outer one and its scratch can be had
    if (strassen_levels() >= 2 && dev >= 0 && !outer_noscratch() && std::min(lower ? m / 2 : m, lower ? n / 2 : n) / 2 >= c2.smin2) {
        outer_plan_of(m, n, k, lower, c2, plan);
        const Need2 nd = plan2_need(plan, c2);
        if (nd.v[2] + nd.v[3]) {
            Scratch &s = g_scratch[dev];
            std::lock_guard<std::mutex> lock(s.mu);
            if (scratch_ensure(s, nd.total()))
                return enqueue(s, [&] {
                    return overlap ? run_schedule(plan, c2, nd, alpha, A, lda, B, ldb, beta, C, ldc, s, st)
                                   : run_plan2(plan, c2, nd, alpha, A, lda, B, ldb, beta, C, ldc, s.p, st);
                });
        }
    }
    rc = strassen_plan(m, n, k, lower, c2.in.smin, c2.in.kslab, ~(size_t)0, plan);
    if (rc) return rc;
    const size_t need = plan_need(plan);
    if (!need) return run_plan(plan, alpha, A, lda, B, ldb, beta, C, ldc, nullptr, nullptr, st);
    if (dev < 0) return gemm_nt(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, lower, 0, st);
    Scratch &s = g_scratch[dev];
    std::lock_guard<std::mutex> lock(s.mu);
    if (!scratch_ensure(s, need)) {
        // plan again with what there is (possibly nothing): smaller products of a SYRK may still fit
        if ((rc = strassen_plan(m, n, k, lower, c2.in.smin, c2.in.kslab, s.cap, plan))) return rc;
        if (!plan_need(plan)) return run_plan(plan, alpha, A, lda, B, ldb, beta, C, ldc, nullptr, nullptr, st);
    }
    // (a list of the inner level alone: plan2_need gives its two regions, the layout is [A | B] either way)
    const Need2 nd = plan2_need(plan, c2);
    if (overlap) return enqueue(s, [&] { return run_schedule(plan, c2, nd, alpha, A, lda, B, ldb, beta, C, ldc, s, st); });
    return enqueue(s, [&] { return run_plan(plan, alpha, A, lda, B, ldb, beta, C, ldc, s.p, s.p + nd.v[0], st); });
}

// ---- a third level ON TOP of the front end, for the recursion's two largest products ----------------------------
// The seven formulas once more on the halves of a product, per top k slab.  Unlike the two levels above, a top product M_i is not
// accumulated into C by the product kernel (that would take eight destinations): it is formed in a temporary T (m/2 x n/2, zeroed
// first) by ONE half-size call of gemm_nt_strassen_cfg -- which takes its two levels and its sum overlap exactly as today -- and
// then added to its one or two blocks of C with alpha * sign by a streaming pass (block_acc_kernel).  Only kernels that exist
// are launched, plus that pass.  Again host code emits records and the device path executes exactly that list:
//   PLAN3_SUM   layout of PLAN_SUM; the result goes to the TOP scratch of that side
//   PLAN3_ZERO  [1] rows [2] cols                                       T = 0
//   PLAN3_PROD  [1] a_src (0: block of A at ([2], [3]), 1: the top A scratch) [4] b_src, ([5], [6]) likewise [7] m [8] n [9] k
//               [10 .. 14] the thresholds of the half-size call (smin, kslab, smin2, kslab2, smin_under)
//               T += X Y^T through gemm_nt_strassen_cfg(m, n, k, 1, X, Y, 1, T, ld m, not lower, those thresholds)
//   PLAN3_ACC   [1] rows [2] cols [3] [4] first destination (row, column of C) [5] its sign [6] [7] [8] the second (sign 0: none)
//               C1 += alpha sign1 T; C2 += alpha sign2 T
//   PLAN3_PASS  layout of PLAN_CLASSIC ([1] lower [2] ar [3] ac [4] br [5] bc [6] m [7] n [8] k [9] cr [10] cc), [11 .. 15] thresholds:
//               that block through gemm_nt_strassen_cfg as before.  A call that does not qualify is this record alone.
// Qualifies: m % 2048 == 0, n % 1024 == 0 (the halves stay multiples of what the outer level asks), m / 2 and n / 2 >= smin3,
// k holds a whole top slab (kslab3 if k reaches it, else kslab3_short); a remainder of k shorter than the slab is a PLAN3_PASS at
// its k offset.  A lower update splits around its off-diagonal square as plan2_syrk does: lower(h), the square, lower(h).
namespace {
constexpr long REC_SMIN3 = 16384, REC_KSLAB3 = 65536, REC_KSLAB3_SHORT = 32768;

// C1 += a1 T and, where C2 is given, C2 += a2 T: T (rows x cols, leading dimension rows) is read once.  The pattern of
// block_sum_kernel: 16-byte accesses, 4 columns per thread in flight, grid-stride over pieces of 512 rows x 4 columns; rows even,
// all bases 16-byte aligned, ldc even (checked by the caller).  A kernel of its own behind the others: they compile as without it.
__global__ __launch_bounds__(256) void block_acc_kernel(int rows, int cols, const double *T, double *C1, double a1, double *C2, double a2,
                                                        size_t ldc)
{
    const int nrc = (rows + 511) / 512, ncg = (cols + 3) / 4;
    const long pieces = (long)nrc * ncg;
    for (long p = blockIdx.x; p < pieces; p += gridDim.x) {
        const int cg = (int)(p / nrc), rc = (int)(p - (long)cg * nrc);
        const int r = rc * 512 + 2 * (int)threadIdx.x;
        if (r >= rows) continue;
        double2_t t[4], c1[4], c2[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = min(cg * 4 + u, cols - 1);
            t[u] = *reinterpret_cast<const double2_t *>(T + (size_t)r + (size_t)c * (size_t)rows);
            c1[u] = *reinterpret_cast<const double2_t *>(C1 + (size_t)r + (size_t)c * ldc);
            if (C2) c2[u] = *reinterpret_cast<const double2_t *>(C2 + (size_t)r + (size_t)c * ldc);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = cg * 4 + u;
            if (c >= cols) continue;
            *reinterpret_cast<double2_t *>(C1 + (size_t)r + (size_t)c * ldc) = c1[u] + a1 * t[u];
            if (C2) *reinterpret_cast<double2_t *>(C2 + (size_t)r + (size_t)c * ldc) = c2[u] + a2 * t[u];
        }
    }
}
int block_acc(int rows, int cols, const double *T, double *C1, double a1, double *C2, double a2, size_t ldc, hipStream_t st, long wgs)
{
    const long pieces = (long)((rows + 511) / 512) * ((cols + 3) / 4);
    hipLaunchKernelGGL(block_acc_kernel, dim3((unsigned)std::min(pieces, wgs)), dim3(256), 0, st, rows, cols, T, C1, a1, C2, a2, ldc);
    SGPR_CHECK_LAUNCH();
    return 0;
}

long top_slab(long k, const StrassenTop &t)
{
    const long s = (t.kslab3 > 0 && k >= t.kslab3) ? t.kslab3 : t.kslab3_short;
    return (s >= 128 && s % 128 == 0 && k >= s) ? s : 0;
}
bool top_qualifies(long m, long n, long k, const StrassenRec &v, const StrassenTop &t, size_t scratch)
{
    if (!v.on || t.smin3 <= 0 || m <= 0 || n <= 0 || m % 2048 != 0 || n % 1024 != 0) return false;
    if (m / 2 < t.smin3 || n / 2 < t.smin3) return false;
    const long slab = top_slab(k, t);
    return slab && (size_t)(m / 2) * (size_t)(n / 2) + (size_t)(m / 2 + n / 2) * (size_t)(slab / 2) <= scratch;
}
void put_cfg(std::vector<long long> &out, int at, const StrassenCfg &c)
{
    long long *r = &out[out.size() - STRASSEN_REC + at];
    r[0] = c.smin; r[1] = c.kslab; r[2] = c.smin2; r[3] = c.kslab2; r[4] = c.smin_under;
}
// `kind`: the thresholds are those of a lower update's call (1) or of a product of trsm_rec (0), whatever the block itself is
void top_pass(int lower, long ar, long ac, long br, long bc, long m, long n, long k, long cr, long cc, int kind, const StrassenRec &v,
              std::vector<long long> &out)
{
    put(out, {PLAN3_PASS, lower, ar, ac, br, bc, m, n, k, cr, cc});
    put_cfg(out, 11, strassen_rec_cfg(v, (int)k, kind));
}
void top_gemm(long m, long n, long k, long ar, long br, long cr, long cc, int kind, const StrassenRec &v, const StrassenTop &t,
              size_t scratch, std::vector<long long> &out)
{
    if (!top_qualifies(m, n, k, v, t, scratch)) { top_pass(0, ar, 0, br, 0, m, n, k, cr, cc, kind, v, out); return; }
    const long slab = top_slab(k, t), m2 = m / 2, n2 = n / 2, k2 = slab / 2;
    std::vector<long long> seven_recs;
    long k0 = 0;
    for (; k0 + slab <= k; k0 += slab) {
        seven_recs.clear();
        seven(PLAN3_SUM, PLAN3_PROD, m2, n2, k2, k0, ar, br, cr, cc, seven_recs);
        for (size_t i = 0; i + STRASSEN_REC <= seven_recs.size(); i += STRASSEN_REC) {
            const long long *r = &seven_recs[i];
            if (r[0] == PLAN3_SUM) { out.insert(out.end(), r, r + STRASSEN_REC); continue; }
            put(out, {PLAN3_ZERO, m2, n2});
            put(out, {PLAN3_PROD, r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9]});
            put_cfg(out, 10, strassen_rec_cfg(v, (int)k2, kind));
            put(out, {PLAN3_ACC, m2, n2, r[10], r[11], r[12], r[13], r[14], r[15]});
        }
    }
    if (k0 < k) top_pass(0, ar, k0, br, k0, m, n, k - k0, cr, cc, kind, v, out);
}
void top_syrk(long n, long k, const StrassenRec &v, const StrassenTop &t, size_t scratch, std::vector<long long> &out)
{
    const long h = n / 2;
    if (n % 2 != 0 || !top_qualifies(h, h, k, v, t, scratch)) { top_pass(1, 0, 0, 0, 0, n, n, k, 0, 0, 1, v, out); return; }
    top_pass(1, 0, 0, 0, 0, h, h, k, 0, 0, 1, v, out);
    top_gemm(h, h, k, h, 0, h, 0, 1, v, t, scratch, out);
    top_pass(1, h, 0, h, 0, h, h, k, h, h, 1, v, out);
}
// doubles per region of the top scratch: T, the A side, the B side
struct Need3 { size_t v[3] = {0, 0, 0}; size_t total() const { return v[0] + v[1] + v[2]; } };
Need3 top_need(const std::vector<long long> &plan)
{
    Need3 nd;
    for (size_t i = 0; i + STRASSEN_REC <= plan.size(); i += STRASSEN_REC) {
        const long long *r = &plan[i];
        if (r[0] == PLAN3_ZERO) nd.v[0] = std::max(nd.v[0], (size_t)r[1] * (size_t)r[2]);
        else if (r[0] == PLAN3_SUM) nd.v[1 + r[1]] = std::max(nd.v[1 + r[1]], (size_t)r[2] * (size_t)r[3]);
    }
    return nd;
}

// The top scratch: a buffer of its own per device behind its own mutex -- the half-size calls take g_scratch's lock themselves.
// Laid out as [T | A side | B side], a second set behind the first where there is room for it.
struct TopScratch {
    std::mutex mu;
    double *p = nullptr;
    size_t cap = 0, failed = 0;     // doubles; smallest request that could not be allocated (0: none)
    hipEvent_t ev = nullptr;        // behind the last call that used the buffer
    hipStream_t last = nullptr;
    bool used = false;
    std::vector<hipEvent_t> pool;   // events of the overlapped passes, timing disabled, created on demand
};
TopScratch g_top[64];

// tunable "rec_strassen3_buffers": 2 (built in) = a second [T | A | B] set, so that the passes of one top product run under the
// next; "rec_strassen3_overlap" = 0: all passes on the caller's stream in list order (and one set)
int top_buffers_wanted() { return (tune("rec_strassen3_overlap", 1) != 0 && tune("rec_strassen3_buffers", 2) >= 2) ? 2 : 1; }
// room for a call that needs `need` doubles per set: `sets` of them if that can be had, else one
bool top_ensure(TopScratch &s, size_t need, int sets)
{
    if (tune("rec_strassen3_noscratch", 0) != 0) return false;     // tests: the allocation is reported as failed
    if (s.cap >= need) return true;
    if (s.failed && need >= s.failed) return false;
    if (s.p) { (void)hipFree(s.p); s.p = nullptr; s.cap = 0; s.used = false; }   // hipFree waits for the device
    for (int b = sets; b >= 1; --b) {
        const size_t want = need * (size_t)b;
        if (s.failed && want >= s.failed) continue;
        if (hipMalloc((void **)&s.p, want * sizeof(double)) == hipSuccess) { s.cap = want; return true; }
        (void)hipGetLastError();
        s.p = nullptr;
        s.failed = want;
    }
    return false;
}
void top_trim()
{
    for (TopScratch &s : g_top) {
        std::lock_guard<std::mutex> lock(s.mu);
        if (s.p) (void)hipFree(s.p);
        if (s.ev) (void)hipEventDestroy(s.ev);
        for (hipEvent_t e : s.pool) if (e) (void)hipEventDestroy(e);
        s.pool.clear();
        s.p = nullptr; s.ev = nullptr; s.cap = 0; s.failed = 0; s.used = false; s.last = nullptr;
    }
    (void)hipGetLastError();
}

// Execute a top list.  Serial form: every record on the caller's stream in list order.  Overlapped form: the sums, the zeroing
// and the accumulations go to the library's low-priority top stream `sd` (one stream: they run in the order they are enqueued,
// so the accumulations of a C block stay in list order); the half-size calls and the pass-through calls stay on the caller's.
// With two buffer sets the accumulation of M_i is enqueued BEHIND the sums and the zeroing of M_i+1:
//     sd:  S0 Z0 S1 Z1 | A0 S2 Z2 | A1 S3 Z3 | ...          caller:  P0 | P1 | P2 ...
// P_i waits for the event behind Z_i, A_i for the event behind P_i; S_i+2 / Z_i+2 overwrite the set of M_i behind A_i, which has
// waited for P_i.  So the passes of M_i and the preparation of M_i+2 run under P_i+1.  With one set the accumulation goes in front
// of the next sums (list order): correct, and nothing overlaps.  sd waits for the caller's stream at entry (the operands may come
// from the launches just before), the caller's stream waits for sd in front of every pass-through call and on EVERY return.
int run_top(const std::vector<long long> &plan, const Need3 &nd, double alpha, const double *A, size_t lda, const double *B, size_t ldb,
            double *C, size_t ldc, TopScratch &s, hipStream_t st)
{
    const size_t need = nd.total();
    const bool overlap = tune("rec_strassen3_overlap", 1) != 0;
    const int nbuf = (top_buffers_wanted() >= 2 && s.cap >= 2 * need) ? 2 : 1;
    const long wgs = overlap ? std::min(65535L, std::max(1L, (long)tune("gemm_strassen_sum_wgs", (double)SUM_WGS_SIDE))) : SUM_WGS;
    hipStream_t sd = st;
    int rc = 0;
    if (overlap && (rc = strassen_top_stream(st, &sd))) return rc;
    auto at = [&](int region, int b) { return s.p + (size_t)b * need + (region == 0 ? 0 : (region == 1 ? nd.v[0] : nd.v[0] + nd.v[1])); };
    // events: 0 entry, 1 exit / joins, 2 + 2 p behind the zeroing of product p, 3 + 2 p behind product p
    auto event = [&](size_t i) {
        if (s.pool.size() <= i) s.pool.resize(i + 1, nullptr);
        if (!s.pool[i]) SGPR_HIP(hipEventCreateWithFlags(&s.pool[i], hipEventDisableTiming));
        return 0;
    };
    auto join = [&]() {     // the caller's stream waits for everything on sd
        if (!overlap) return 0;
        SGPR_HIP(hipEventRecord(s.pool[1], sd));
        SGPR_HIP(hipStreamWaitEvent(st, s.pool[1], 0));
        return 0;
    };
    struct Join {
        bool on; hipStream_t sd, st; hipEvent_t ev;
        ~Join()
        {
            if (on && (hipEventRecord(ev, sd) != hipSuccess || hipStreamWaitEvent(st, ev, 0) != hipSuccess)) {
                (void)hipGetLastError();
                (void)hipStreamSynchronize(sd);
            }
        }
    };
    if ((rc = event(0)) || (rc = event(1))) return rc;
    if (overlap) {
        SGPR_HIP(hipEventRecord(s.pool[0], st));
        SGPR_HIP(hipStreamWaitEvent(sd, s.pool[0], 0));
    }
    Join at_exit{overlap, sd, st, s.pool[1]};
    struct Pend { const long long *r; int b; size_t p; };
    std::vector<Pend> pending;
    size_t p = 0;       // the top product the records belong to; its buffer set: p % nbuf
    auto flush = [&]() {
        for (const Pend &q : pending) {
            const long long *r = q.r;
            if (overlap) SGPR_HIP(hipStreamWaitEvent(sd, s.pool[3 + 2 * q.p], 0));
            const int e = block_acc((int)r[1], (int)r[2], at(0, q.b), C + r[3] + (size_t)r[4] * ldc, alpha * (double)r[5],
                                    r[8] ? C + r[6] + (size_t)r[7] * ldc : nullptr, alpha * (double)r[8], ldc, sd, wgs);
            if (e) return e;
        }
        pending.clear();
        return 0;
    };
    for (size_t i = 0; i + STRASSEN_REC <= plan.size(); i += STRASSEN_REC) {
        const long long *r = &plan[i];
        const int b = (int)(p % (size_t)nbuf);
        if (r[0] == PLAN3_SUM) {
            if (nbuf == 1 && (rc = flush())) return rc;
            const double *P = r[1] ? B : A;
            const size_t ld = r[1] ? ldb : lda;
            rc = block_sum((int)r[2], (int)r[3], P + r[4] + (size_t)r[5] * ld, ld, P + r[6] + (size_t)r[7] * ld, ld, (double)r[8],
                           at(1 + (int)r[1], b), sd, wgs);
        } else if (r[0] == PLAN3_ZERO) {
            if (nbuf == 1 && (rc = flush())) return rc;
            SGPR_HIP(hipMemsetAsync(at(0, b), 0, (size_t)r[1] * (size_t)r[2] * sizeof(double), sd));
        } else if (r[0] == PLAN3_PROD) {
            const int m = (int)r[7], n = (int)r[8], k = (int)r[9];
            if (overlap) {
                if ((rc = event(2 + 2 * p)) || (rc = event(3 + 2 * p))) return rc;
                SGPR_HIP(hipEventRecord(s.pool[2 + 2 * p], sd));
                SGPR_HIP(hipStreamWaitEvent(st, s.pool[2 + 2 * p], 0));
            }
            const double *X = r[1] ? at(1, b) : A + r[2] + (size_t)r[3] * lda;
            const double *Y = r[4] ? at(2, b) : B + r[5] + (size_t)r[6] * ldb;
            StrassenCfg cfg;
            cfg.smin = (long)r[10]; cfg.kslab = (long)r[11]; cfg.smin2 = (long)r[12]; cfg.kslab2 = (long)r[13]; cfg.smin_under = (long)r[14];
            rc = gemm_nt_strassen_cfg(m, n, k, 1.0, X, r[1] ? (size_t)m : lda, Y, r[4] ? (size_t)n : ldb, 1.0, at(0, b), (size_t)m, 0, cfg, st);
            if (rc) return rc;
            if (overlap) SGPR_HIP(hipEventRecord(s.pool[3 + 2 * p], st));
            rc = flush();       // the accumulations of the products before this one: behind its sums, under it
        } else if (r[0] == PLAN3_ACC) {
            pending.push_back(Pend{r, b, p});
            ++p;
        } else if (r[0] == PLAN3_PASS) {
            if ((rc = flush()) || (rc = join())) return rc;
            StrassenCfg cfg;
            cfg.smin = (long)r[11]; cfg.kslab = (long)r[12]; cfg.smin2 = (long)r[13]; cfg.kslab2 = (long)r[14]; cfg.smin_under = (long)r[15];
            rc = gemm_nt_strassen_cfg((int)r[6], (int)r[7], (int)r[8], alpha, A + r[2] + (size_t)r[3] * lda, lda, B + r[4] + (size_t)r[5] * ldb, ldb,
                                      1.0, C + r[9] + (size_t)r[10] * ldc, ldc, (int)r[1], cfg, st);
        } else {
            set_error("run_top: unknown record");
            rc = SGPR_E_ARG;
        }
        if (rc) return rc;
    }
    return flush();
}
}  // namespace

StrassenTop strassen_top_values()
{
    StrassenTop t;
    t.smin3 = std::max(0L, (long)tune("rec_strassen3_min", (double)REC_SMIN3));
    t.kslab3 = std::max(0L, (long)tune("rec_strassen3_kslab", (double)REC_KSLAB3));
    t.kslab3_short = std::max(0L, (long)tune("rec_strassen3_kslab_short", (double)REC_KSLAB3_SHORT));
    return t;
}

// the top list of one call as the host decides it (no device)
int strassen_top_plan(int m, int n, int k, int lower, const StrassenRec *vp, const StrassenTop *tp, size_t scratch_doubles,
                      std::vector<long long> &out)
{
    const StrassenRec v = vp ? *vp : strassen_rec_values();
    const StrassenTop t = tp ? *tp : strassen_top_values();
    if (m < 0 || n < 0 || k < 0 || (lower && m != n)) { set_error("strassen_top_plan: bad extents"); return SGPR_E_ARG; }
    out.clear();
    if (lower) top_syrk(n, k, v, t, scratch_doubles, out);
    else       top_gemm(m, n, k, 0, 0, 0, 0, 0, v, t, scratch_doubles, out);
    return 0;
}
int strassen_cfg_plan(int m, int n, int k, int lower, const long cfg[5], std::vector<long long> &out)
{
    if (m < 0 || n < 0 || k < 0 || (lower && m != n) || !cfg) { set_error("strassen_cfg_plan: bad arguments"); return SGPR_E_ARG; }
    StrassenCfg c;
    c.smin = cfg[0]; c.kslab = cfg[1]; c.smin2 = cfg[2]; c.kslab2 = cfg[3]; c.smin_under = cfg[4];
    outer_plan_of(m, n, k, lower, cfg2_of(c, ~(size_t)0), out);
    return 0;
}
size_t strassen_top_scratch_doubles(int m, int n, int k, int lower, const StrassenRec &v, const StrassenTop &t)
{
    std::vector<long long> plan;
    if (strassen_levels() < 2 || strassen_top_plan(m, n, k, lower, &v, &t, ~(size_t)0, plan)) return 0;
    return top_need(plan).total();
}
// make room for the top level's calls of one factorisation (potrf: once, before the first launch): two buffer sets if they can
// be had, else one; if not even that, the top level is off call by call and nothing else changes
void strassen_top_reserve(size_t need, hipStream_t st)
{
    const int dev = device_of(st);
    if (dev < 0 || !need) return;
    TopScratch &s = g_top[dev];
    std::lock_guard<std::mutex> lock(s.mu);
    if (s.cap >= need * (size_t)top_buffers_wanted()) return;
    if (s.cap >= need && s.failed && need * 2 >= s.failed) return;      // the second set has been refused before
    if (s.p) { (void)hipFree(s.p); s.p = nullptr; s.cap = 0; s.used = false; }
    (void)top_ensure(s, need, top_buffers_wanted());
}

// C += alpha A B^T as the recursion issues it, with the top level where it applies.  Whatever does not qualify is exactly the
// call gemm_nt_strassen_cfg(..., strassen_rec_cfg(v, k, lower), st) that stood here before.
int strassen_top_gemm(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb, double beta,
                      double *C, size_t ldc, int lower, const StrassenRec *vp, const StrassenTop *tp, hipStream_t st)
{
    const StrassenRec v = vp ? *vp : strassen_rec_values();
    const StrassenTop t = tp ? *tp : strassen_top_values();
    const StrassenCfg cfg = strassen_rec_cfg(v, k, lower);
    // (the size test first: the short products of the panel solves come through here by the thousand)
    const bool aligned = ((((uintptr_t)A | (uintptr_t)B | (uintptr_t)C) & 15) == 0) && (((lda | ldb | ldc) & 1) == 0);
    const int dev = (!v.on || t.smin3 <= 0 || std::min(lower ? m / 2 : m, lower ? n / 2 : n) / 2 < t.smin3) ? -1 : device_of(st);
    if (dev < 0 || strassen_levels() < 2 || !aligned || beta != 1.0 || (lower && m != n))
        return gemm_nt_strassen_cfg(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, lower, cfg, st);
    std::vector<long long> plan;
    int rc = strassen_top_plan(m, n, k, lower, &v, &t, ~(size_t)0, plan);
    if (rc) return rc;
    const Need3 nd = top_need(plan);
    if (nd.total()) {
        TopScratch &s = g_top[dev];
        std::lock_guard<std::mutex> lock(s.mu);
        if (top_ensure(s, nd.total(), top_buffers_wanted())) {
            if (!s.ev) SGPR_HIP(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
            if (s.used && s.last != st) SGPR_HIP(hipStreamWaitEvent(st, s.ev, 0));
            rc = run_top(plan, nd, alpha, A, lda, B, ldb, C, ldc, s, st);
            SGPR_HIP(hipEventRecord(s.ev, st));
            s.last = st;
            s.used = true;
            return rc;
        }
    }
    return gemm_nt_strassen_cfg(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, lower, cfg, st);
}

}  // namespace sgpr
