// panel.hip -- the kernels that factor: the leaf kernel and the persistent panel kernel of the blocked Cholesky drivers (chol.hip,
// cholq.hip, batch.hip), with their launchers.  A translation unit of its own: a change to a driver does not recompile it;
// panel.h is what the drivers see.  The two share leaf_body (leaf.h) and stay in ONE unit: which of its lambdas the compiler
// inlines depends on all their call sites, and apart the same source gave other instructions for both.
#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "cholq.h"
#include "common.h"
#include "strassen.h"
#include "gemm_tile.h"
#include "leaf.h"
#include "panel.h"

namespace sgpr {

namespace {

using namespace leaf;


__global__ __launch_bounds__(LT) void leaf_kernel(int nb, double *A, size_t lda, double *inv,
                                                  int *dinfo, int goff, int mode,
                                                  unsigned long long *stamps)
{
    __shared__ double s[LEAF_LDS];
    // a full leaf gets its loop bounds at compile time (59 us; with the run-time order of a partial leaf 64)
    if (nb == LEAF) leaf_body(s, (int)LEAF, A, lda, inv, dinfo, goff, mode, stamps);
    else            leaf_body(s, nb, A, lda, inv, dinfo, goff, mode, stamps);
}

// ---- persistent panel kernel ------------------------------------------------------------------
// One launch factors a whole block column ("panel") of the blocked right-looking driver: the
// nb x nb diagonal block (W = nb / 128 leaf columns) and all rows below it (R strips of 128 rows,
// the first W of them being the diagonal block's).  In round 1 every leaf column cost three dependent
// launches (leaf, rows-below x inverse, fold into the remaining columns: 60 + 74 + 99 us) on the
// stream the whole factorisation waits for; here the same tasks run inside ONE grid and hand their
// results over through flags in global memory:
//     diagonal strip g (its own workgroup), columns c = 0 .. g-1:
//         wait E[c];  X = A(g,c) inv(L_cc)^T by a blocked solve in the MFMA accumulators (trsm_solve: needs L_cc
//         and its 16 x 16 diagonal inverses only)                                          -> F[g][c]
//         c < g-1:  A(g,g) -= X X^T out of an LDS image of X;  wait F[c'][c];  A(g,c') -= X L(c',c)^T, c' in (c, g)
//         c = g-1:  A(g,g) -= X X^T lands in the leaf's LDS block and the strip goes straight on to
//     leaf(g): factor A(g,g) in LDS, L out write-through as its columns become final,
//         L + diagonal inverses handed over                                                -> E[g]
//         full inverse (recursive doubling)                                                -> I[g]
//     the chain the next panel step waits for is  leaf -> E -> solve -> update -> leaf  inside ONE CU's
//     registers and LDS per column (~70 us; as three launches per column it was 233 us).
//     strip r below the diagonal block (shared round-robin by the other workgroups), columns c = 0 .. W-1:
//         wait I[c];  X = A(r,c) inv(L_cc)^T  (a 128^3 product on the matrix cores);  wait F[c'][c];
//         A(r,c') -= X L(c',c)^T for c' in (c, W);  on the LAST column: wait E[c] and the blocked solve.
// Two tickets: diagonal strips go to workgroups whose id is a multiple of 8 (one XCD), in their order of arrival;
// everybody else, and the leftovers of the first kind, takes the strips below in order of arrival.
// Hand-off protocol (cdna_hip_programming.md, guideline 16): plain payload stores -> every storing
// wave drains vmcnt -> workgroup barrier -> one lane: agent-scope release fence, drain, relaxed
// agent-scope flag store (panel_publish); payloads stored write-through (sc1) skip the fence
// (panel_publish_wt, the leaf's E hand-off).  The consumer polls the word relaxed (one lane, s_sleep between
// polls), then ONE agent-scope acquire, drain, workgroup barrier, plain loads.
// Forward progress does not rely on co-residency of the grid: a workgroup only waits for flags of diagonal
// strips, whose tickets the first eligible workgroups to arrive hold, in order -- every flag a diagonal strip
// waits for is set by one that started before it.  Every spin is bounded; a timeout is reported through *dinfo
// (PANEL_TIMEOUT).
constexpr int PANEL_TIMEOUT = POTRF_HANDOFF_TIMEOUT;   // *dinfo value: a hand-off was never published
typedef __attribute__((address_space(1))) int gint;

__device__ __forceinline__ void panel_publish(int *flag)
{
    // every wave has drained its stores before the barrier; then one lane releases and signals
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store((gint *)flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ... with a value (the task-queue driver's version words)
__device__ __forceinline__ void panel_publish_val(int *word, int val)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store((gint *)word, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the same for a payload that went out with write-through (sc1) stores only: no L2 write-back to wait for
__device__ __forceinline__ void panel_publish_wt(int *flag)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store((gint *)flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Wait until every word flags[idx[0..cnt)] has reached `need`.  Returns false (workgroup-uniform) on timeout, or when
// the task-queue driver has given the factorisation up (`abort` word set; null outside that driver).
__device__ __forceinline__ bool panel_wait_ge(const int *flags, const int *idx, int cnt, int need, int *dinfo, int *sh,
                                              int *abort = nullptr)
{
    if (threadIdx.x == 0) {
        int ok = 1;
        for (int q = 0; q < cnt && ok; ++q) {
            gint *f = (gint *)(flags + idx[q]);
            unsigned spins = 0;
            const unsigned long long twait0 = abort ? __builtin_amdgcn_s_memrealtime() : 0;
            while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need) {
                __builtin_amdgcn_s_sleep(16);
                ++spins;
                if (abort) {
                    // task-queue driver: a long wait backs off to one look every ~2 us (7 us cost 1 - 2 % of the whole
                    // factorisation: the chain is its critical path), and gives up when the workers have, or after 20 s of
                    // REAL time
                    if (spins > 16) __builtin_amdgcn_s_sleep(64);
                    if ((spins & 15u) == 0) {
                        if (__hip_atomic_load((gint *)abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) { ok = -1; break; }
                        if (__builtin_amdgcn_s_memrealtime() - twait0 > 20ull * 100000000ull) { ok = 0; break; }
                    }
                } else if (spins > (3u << 20)) { ok = 0; break; }    // ~ 3 s
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (ok == 0) {
            atomicCAS(dinfo, 0, PANEL_TIMEOUT);
            if (abort) {
                // task-queue driver's post-mortem words (abort = qs + Q_ABORT): who gave up waiting for what
                if (atomicCAS(abort + 7, 0, 1) == 0) {
                    abort[8] = (int)blockIdx.x; abort[9] = idx[0]; abort[10] = cnt; abort[11] = need;
                    abort[12] = (int)(flags == nullptr);
                }
                __hip_atomic_store((gint *)abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        *sh = ok > 0;
    }
    __syncthreads();
    const int ok = *sh;
    __syncthreads();
    return ok != 0;
}
__device__ __forceinline__ bool panel_wait(int *flags, const int *idx, int cnt, int *dinfo, int *sh, int *abort = nullptr)
{
    return panel_wait_ge(flags, idx, cnt, 1, dinfo, sh, abort);
}

// C (128 x 128) := beta C + alpha A B^T, k = 128, one workgroup of 256 threads, operands / result in
// global memory (column-major panels: see gemm_tile.h)
__device__ __forceinline__ void panel_product(double *smem, double alpha, const double *A, size_t lda,
                                              const double *B, size_t ldb, double beta, double *C, size_t ldc)
{
    tile::GemmArgs ga{};
    ga.m = LEAF; ga.n = LEAF; ga.k = LEAF;
    ga.alpha = alpha; ga.beta = beta;
    ga.A = A; ga.lda = lda; ga.B = B; ga.ldb = ldb; ga.C = C; ga.ldc = ldc;
    ga.stamps = nullptr;
    // the previous task's stores are visible to this workgroup, and its LDS reads are finished
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    tile::gemm_body_dma<LEAF, LEAF, 2>(ga, smem, 0, 0);
}

// ---- the chain of the factorisation inside the panel kernel: solve -> update -> leaf in registers and LDS --------
// X (128 x 128, in place) := X inv(L_cc)^T WITHOUT the leaf's full inverse: a right-looking blocked solve over the
// eight 16-column blocks,  X_j = S_j inv(L_jj)^T;  S_j' -= X_j L(j',j)^T for j' > j,  that needs L_cc and the
// inverses of its 16 x 16 diagonal blocks only -- what a leaf hands over ~20 us before its full inverse (E[c]).
// The rows of X are independent, so every wave takes 32 of them and runs alone: the tile lives in its MFMA
// accumulators (row = lane & 15, column = 4 r + lane >> 4), and that layout IS the operand layout of the next
// product (k = 4 r + lane >> 4), so X_j goes from one v_mfma to the next without touching LDS; only L_cc is
// staged (its 28 blocks below the diagonal, and the inverted diagonal blocks in place of L's own).  288 MFMAs per
// wave.  The tile is fetched BEFORE the wait for E[c] (trsm_prefetch): it has been final since the previous column.
// leading dimension of the LDS images the matrix cores read their operands from here: 16 rows x 4 k-columns per
// fragment read, so the column stride must put k, k+1 32 banks apart (144 * 8 B = 2 * 576 B): conflict-free.  With the
// leaf's own 130 the same reads were 2-4-way conflicts and the X X^T update took 17 us instead of 9.
constexpr int ILD = LEAF + 16;
typedef double4_t XTile[2][8];      // this wave's 32 rows: [row block][16-column block][r]

// block t = 0..27 of the strictly lower 16 x 16 blocks of a 128 x 128 tile: t = bi (bi - 1) / 2 + bj, 0 <= bj < bi <= 7
__device__ __forceinline__ constexpr int below_bi(int t)
{
    int bi = 1;
    while ((bi + 1) * bi / 2 <= t) ++bi;
    return bi;
}
__device__ __forceinline__ constexpr int below_bj(int t) { return t - below_bi(t) * (below_bi(t) - 1) / 2; }

__device__ __forceinline__ void trsm_prefetch(const double *X, size_t lda, XTile &x)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                x[rb][j][r] = X[(size_t)(32 * wave + 16 * rb + l15) + (size_t)(16 * j + 4 * r + l4) * lda];
}

__device__ __forceinline__ void trsm_solve(double *s, const double *Lcc, const double *invd, size_t lda, XTile &x,
                                           unsigned long long *st = nullptr)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int l15 = lane & 15, l4 = lane >> 4;
    __syncthreads();                                   // the previous task is done with the LDS buffer
    // the 28 blocks below the diagonal ones: 14 16-byte loads per thread, ALL in flight at once (one round trip to
    // wherever the leaf's write-through stores went; in batches of 8 the staging took 8.7 us, four round trips)
    double2_t lv[14];
#pragma unroll
    for (int q = 0; q < 14; ++q) {
        // 16-byte piece e = 256 q + tid of 28 blocks x 16 columns x 8 row pairs: block 2 q + (tid >> 7), a compile-
        // time pair per q (a per-lane search for it cost 3 us: the loop diverges)
        const int col = (tid >> 3) & 15, rp = tid & 7;
        const int bi = (tid & 128) ? below_bi(2 * q + 1) : below_bi(2 * q);
        const int bj = (tid & 128) ? below_bj(2 * q + 1) : below_bj(2 * q);
        lv[q] = *reinterpret_cast<const double2_t *>(Lcc + (size_t)(16 * bi + 2 * rp) + (size_t)(16 * bj + col) * lda);
    }
    double dv[LEAF * PW / LT];
#pragma unroll
    for (int it = 0; it < LEAF * PW / LT; ++it) {
        const int idx = it * LT + tid;
        const int i = idx % LEAF, c = (i / PW) * PW + idx / LEAF;
        dv[it] = invd[(size_t)i + (size_t)c * LEAF];
    }
    if (PANEL_DBG && st) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tid == 0) st[-3] = __builtin_amdgcn_s_memrealtime();   // slot 3
    }
#pragma unroll
    for (int q = 0; q < 14; ++q) {
        const int col = (tid >> 3) & 15, rp = tid & 7;
        const int bi = (tid & 128) ? below_bi(2 * q + 1) : below_bi(2 * q);
        const int bj = (tid & 128) ? below_bj(2 * q + 1) : below_bj(2 * q);
        *reinterpret_cast<double2_t *>(s + (16 * bj + col) * ILD + 16 * bi + 2 * rp) = -lv[q];   // -L: S_j' += X_j (-L)^T
    }
#pragma unroll
    for (int it = 0; it < LEAF * PW / LT; ++it) {      // inv(L_jj) where L_jj would be
        const int idx = it * LT + tid;
        const int i = idx % LEAF, c = (i / PW) * PW + idx / LEAF;
        s[c * ILD + i] = dv[it];
    }
    __syncthreads();
    if (PANEL_DBG && st && tid == 0) st[0] = __builtin_amdgcn_s_memrealtime();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            double4_t y = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                y = __builtin_amdgcn_mfma_f64_16x16x4f64(s[(16 * j + 4 * kk + l4) * ILD + 16 * j + l15], x[rb][j][kk], y, 0, 0, 0);
            x[rb][j] = y;
        }
#pragma unroll
        for (int jj = j + 1; jj < 8; ++jj) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const double lneg = s[(16 * j + 4 * kk + l4) * ILD + 16 * jj + l15];
#pragma unroll
                for (int rb = 0; rb < 2; ++rb)
                    x[rb][jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(lneg, x[rb][j][kk], x[rb][jj], 0, 0, 0);
            }
        }
    }
    if (PANEL_DBG && st && tid == 0) st[1] = __builtin_amdgcn_s_memrealtime();
}

// write-through (sc1) stores: the flag that hands X over needs no L2 write-back (panel_publish_wt)
__device__ __forceinline__ void trsm_store(double *X, size_t lda, const XTile &x)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                store_wt(X + (size_t)(32 * wave + 16 * rb + l15) + (size_t)(16 * j + 4 * r + l4) * lda, x[rb][j][r]);
}

// The 36 16 x 16 blocks of the lower triangle of a 128 x 128 tile, nine per wave, as block PAIRS {b, b'} of the
// eight row blocks: two {b,b}, two each with b' - b = 1, 2, 3 (mod 8) and one with b' - b = 4.  In terms of eight
// SLOTS the nine pairs are the same for every wave -- only the slot -> block map depends on the wave -- so the
// registers the MFMAs name are compile-time while the LDS / memory addresses carry the wave:
//   slot i = 0..4 -> block (2 w + i) mod 8,   slot 6 -> block w,   slot 7 -> block w + 4
// A pair whose first block is the smaller one is the TRANSPOSE of a lower block (C is symmetric): it is fetched
// and stored with rows and columns exchanged.
constexpr int DP[9][2] = {{0, 0}, {1, 1}, {1, 0}, {2, 0}, {3, 0}, {2, 1}, {3, 1}, {4, 1}, {7, 6}};   // (rows' slot, columns' slot)
typedef double4_t CTile[9];
struct DiagMap {
    int blk[8];
    __device__ __forceinline__ DiagMap(int wave)
    {
#pragma unroll
        for (int i = 0; i < 5; ++i) blk[i] = (2 * wave + i) & 7;
        blk[5] = 0; blk[6] = wave; blk[7] = wave + 4;
    }
    // Pair p in a column-major tile with leading dimension ld: element r of lane (l15, l4) sits at
    // base + voff + r * rstep, where base and rstep are wave-uniform and voff is one of two per-lane offsets.
    // (accumulator: rows <- l15 of block bp, columns <- 4 r + l4 of block bq; bp < bq: the transposed block)
    __device__ __forceinline__ void where(int p, size_t ld, int l15, int l4, size_t &base, unsigned &voff, size_t &rstep, bool &diagonal) const
    {
        const int bp = blk[DP[p][0]], bq = blk[DP[p][1]];
        const bool lower = bp >= bq;
        base = lower ? (size_t)16 * bp + (size_t)16 * bq * ld : (size_t)16 * bq + (size_t)16 * bp * ld;
        voff = lower ? (unsigned)l15 + (unsigned)l4 * (unsigned)ld : (unsigned)l4 + (unsigned)l15 * (unsigned)ld;   // < 2^31: ld <= 2^24
        rstep = lower ? 4 * ld : 4;
        diagonal = bp == bq;
    }
};

// this wave's nine blocks of C
__device__ __forceinline__ void diag_prefetch(const double *C, size_t lda, CTile &c)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const DiagMap dm(wave);
#pragma unroll
    for (int p = 0; p < 9; ++p) {
        size_t base, rstep;
        unsigned voff;
        bool dg;
        dm.where(p, lda, l15, l4, base, voff, rstep, dg);
#pragma unroll
        for (int r = 0; r < 4; ++r) c[p][r] = (C + base + r * rstep)[voff];   // uniform pointer + 32-bit lane offset
    }
}

// C (the strip's diagonal tile) -= X X^T, lower blocks only: X goes from the solve's accumulators into LDS as a
// [k][row] image, every wave multiplies its nine blocks out of it (per k-chunk: the fragments of its seven row
// blocks, fetched one chunk ahead, then nine MFMAs on registers).
__device__ __forceinline__ void diag_multiply(double *s, const XTile &x, CTile &c, unsigned long long *st = nullptr)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    __syncthreads();                                   // every wave is done with L_cc in s
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[(16 * j + 4 * r + l4) * ILD + 32 * wave + 16 * rb + l15] = x[rb][j][r];
    __syncthreads();
    if (PANEL_DBG && st && tid == 0) st[0] = __builtin_amdgcn_s_memrealtime();
    const DiagMap dm(wave);
    double f[2][8];
    auto fetch = [&](int k, double (&ff)[8]) {
        const double *row = s + (4 * k + l4) * ILD + l15;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i != 5) ff[i] = row[16 * dm.blk[i]];
    };
    fetch(0, f[0]);
#pragma unroll 4
    for (int k = 0; k < LEAF / 4; ++k) {
        if (k + 1 < LEAF / 4) fetch(k + 1, f[(k + 1) & 1]);
#pragma unroll
        for (int p = 0; p < 9; ++p)
            c[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(-f[k & 1][DP[p][1]], f[k & 1][DP[p][0]], c[p], 0, 0, 0);
    }
    if (PANEL_DBG && st && tid == 0) st[2] = __builtin_amdgcn_s_memrealtime();
}

// ... and straight into the leaf's LDS block, where leaf_body expects the tile: no trip through memory between
// the solve, the update and the factorisation of the chain
__device__ __forceinline__ void diag_update_into_leaf(double *s, const XTile &x, CTile &c, unsigned long long *st = nullptr)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    diag_multiply(s, x, c, st);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the X stores of trsm_store: drained long ago)
    __syncthreads();                                   // every wave is done with the image
    // (the blocks above the diagonal keep whatever the image left there: leaf_body never reads them -- every
    // read of s in it is on or below the diagonal, or masked by a select)
    const DiagMap dm(wave);
#pragma unroll
    for (int p = 0; p < 9; ++p) {
        size_t base, rstep;
        unsigned voff;
        bool dg;
        dm.where(p, LLD, l15, l4, base, voff, rstep, dg);
#pragma unroll
        for (int r = 0; r < 4; ++r) s[base + voff + r * rstep] = (!dg || l15 >= 4 * r + l4) ? c[p][r] : 0.0;
    }
    __syncthreads();
}

// the same update with the tile staying in memory (an earlier column of the strip)
__device__ __forceinline__ void diag_update_global(double *s, const XTile &x, CTile &c, double *C, size_t lda)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    diag_multiply(s, x, c);
    const DiagMap dm(wave);
#pragma unroll
    for (int p = 0; p < 9; ++p) {
        size_t base, rstep;
        unsigned voff;
        bool dg;
        dm.where(p, lda, l15, l4, base, voff, rstep, dg);
#pragma unroll
        for (int r = 0; r < 4; ++r) (C + base + r * rstep)[voff] = c[p][r];
    }
}

// One strip of one panel (g < W: diagonal strip g; otherwise a strip below the diagonal block).  False: a hand-off timed
// out or the factorisation has been given up.  `s`: LEAF * ILD doubles of LDS, `sh`: two ints.
__device__ __forceinline__ bool panel_strip(const PanelArgs &a, const int g, double *s, int *sh)
{
    const int tid = threadIdx.x;
    const int W = a.W, R = a.R, G = a.G;
    unsigned long long *const cen = (a.census && blockIdx.x < 32) ? a.census + 4 * blockIdx.x : nullptr;
    if (cen && tid == 0) {
        cen[0] = ((unsigned long long)(unsigned)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) << 32) |
                 (unsigned)__builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));
        cen[1] = __builtin_amdgcn_s_memrealtime();
        cen[3] = (unsigned long long)g;
    }
    const int E0 = 2 + PW_MAX, F0 = 2 + 2 * PW_MAX;
    auto tileptr = [&](int r, int c) { return a.P + (size_t)r * LEAF + (size_t)c * LEAF * a.lda; };
    int idx[PW_MAX];
    if (g < W) {
        // ---- a diagonal strip: row g of the diagonal block, columns 0..g-1, then its own leaf.  Its solves need
        // E[c] only; the last column (c = g - 1) is the chain: solve -> update of (g,g) -> leaf without leaving the CU
        const bool dbg = PANEL_DBG && a.dbg && tid == 0;
        if (a.ver) {
            // task-queue driver: this strip's tiles have taken the updates of every earlier panel?
            const int vi = a.ver_i0 + (g >> 1);
            for (int c = 0; c <= g; ++c) idx[c] = (vi * a.ver_ld + a.ver_j0 + c) * (int)cholq::VS;
            if (!panel_wait_ge(a.ver, idx, g + 1, a.ver_need, a.dinfo, sh + 1, a.abort)) return false;
        }
        // Tiles (g, c'), 1 <= c' < g: whoever gets there first.  A helper workgroup that is running has put 1 into the
        // tile's word (3 once the tile carries every column c < c'); this strip takes the others for itself (2) and
        // updates them behind each of its solves as before -- it never waits for a workgroup that has not started.
        unsigned helped = 0;
        auto claim_tiles = [&]() {                      // (behind this strip's first solve: a helper that is going to run has started by now)
            if (tid == 0) {
                unsigned m = 0;
                for (int cp = 1; cp < g; ++cp) {
                    const int old = atomicCAS(a.flags + F0 + cp * PW_MAX + g, 0, 2);
                    if (old == 1 || old == 3) m |= 1u << cp;
                }
                sh[1] = (int)m;
            }
            __syncthreads();
            helped = (unsigned)sh[1];
            __syncthreads();
        };
        auto wait_helper = [&](int cp) -> bool {       // tile (g, cp) has taken the columns before cp?
            if (!((helped >> cp) & 1u)) return true;
            idx[0] = F0 + cp * PW_MAX + g;
            return panel_wait_ge(a.flags, idx, 1, 3, a.dinfo, sh + 1, a.abort);
        };
        for (int c = 0; c + 1 < g; ++c) {
            double *X = tileptr(g, c);
            XTile x;
            CTile cd;
            if (!wait_helper(c)) return false;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the updates this workgroup applied to (g,c) have
            __syncthreads();                                      // landed, whichever wave stored them
            trsm_prefetch(X, a.lda, x);
            diag_prefetch(tileptr(g, g), a.lda, cd);
            idx[0] = E0 + c;
            if (!panel_wait(a.flags, idx, 1, a.dinfo, sh + 1, a.abort)) return false;
            trsm_solve(s, tileptr(c, c), a.inv + (size_t)c * LEAF * LEAF, a.lda, x);
            trsm_store(X, a.lda, x);
            // X = L(g,c) goes to the strips below; the strip's own diagonal tile takes X X^T straight from the
            // accumulators (lower blocks only); the update of its tiles (g, c+1..g-1) needs L(c',c) of the diagonal
            // strips c' in (c, g)
            panel_publish_wt(a.flags + F0 + g * PW_MAX + c);
            diag_update_global(s, x, cd, tileptr(g, g), a.lda);
            if (c == 0 && a.NH > 0) claim_tiles();
            int cnt = 0;
            for (int cc = c + 1; cc < g; ++cc)
                if (!((helped >> cc) & 1u)) idx[cnt++] = F0 + cc * PW_MAX + c;
            if (cnt && !panel_wait(a.flags, idx, cnt, a.dinfo, sh + 1, a.abort)) return false;
            for (int t = 1; t < g - c; ++t)
                if (!((helped >> (c + t)) & 1u))
                    panel_product(s, -1.0, X, a.lda, tileptr(c + t, c), a.lda, 1.0, tileptr(g, c + t), a.lda);
        }
        if (g > 0) {
            const int c = g - 1;
            double *X = tileptr(g, c);
            XTile x;
            CTile cd;
            if (!wait_helper(c)) return false;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this workgroup's updates of (g,c) and (g,g) have landed
            __syncthreads();
            trsm_prefetch(X, a.lda, x);
            diag_prefetch(tileptr(g, g), a.lda, cd);
            idx[0] = E0 + c;
            if (dbg) a.dbg[16 * g + 2] = __builtin_amdgcn_s_memrealtime();
            if (!panel_wait(a.flags, idx, 1, a.dinfo, sh + 1, a.abort)) return false;
            if (dbg) a.dbg[16 * g + 0] = __builtin_amdgcn_s_memrealtime();
            trsm_solve(s, tileptr(c, c), a.inv + (size_t)c * LEAF * LEAF, a.lda, x, a.dbg ? a.dbg + 16 * g + 6 : nullptr);
            trsm_store(X, a.lda, x);
            if (dbg) a.dbg[16 * g + 1] = __builtin_amdgcn_s_memrealtime();
            diag_update_into_leaf(s, x, cd, a.dbg ? a.dbg + 16 * g + 8 : nullptr);           // (ends behind a barrier that every wave's drained X stores precede)
            if (tid == 0) __hip_atomic_store((gint *)(a.flags + F0 + g * PW_MAX + c), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // this strip's diagonal tile has taken the updates of all earlier columns: factor + invert it
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (dbg) a.dbg[16 * g + 4] = __builtin_amdgcn_s_memrealtime();
        leaf_body(s, (int)LEAF, tileptr(g, g), a.lda,
                  a.inv + (size_t)g * LEAF * LEAF, a.dinfo, a.goff + g * LEAF, (int)LEAF_FACTOR, nullptr,
                  a.flags + E0 + g, g > 0, dbg ? a.dbg + 16 * g + 11 : nullptr);
        panel_publish(a.flags + 2 + g);
        // task-queue driver: "something moved" (the workers drain their kernel instance when nothing does, cholq.h)
        if (a.abort && tid == 0)
            __hip_atomic_fetch_add((gint *)(a.abort + (cholq::Q_PROG - cholq::Q_ABORT)), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (dbg) a.dbg[16 * g + 5] = __builtin_amdgcn_s_memrealtime();
        if (cen && tid == 0) cen[2] = __builtin_amdgcn_s_memrealtime();
        return true;
    }
    if (g < W + a.NH) {
        // ---- a helper: tile (gg, cp) of the diagonal block takes the columns c < cp as their rows X(gg, c), X(cp, c)
        // are published by the two diagonal strips (tickets 0 .. W-1: they started before this workgroup or are waited
        // for like the strips below wait for them)
        int h = g - W, cp = 1, gg = 2;
        while (h >= W - 1 - cp) { h -= W - 1 - cp; ++cp; }
        gg = cp + 1 + h;
        int *word = a.flags + F0 + cp * PW_MAX + gg;
        if (tid == 0) sh[1] = atomicCAS(word, 0, 1);
        __syncthreads();
        const int old = sh[1];
        __syncthreads();
        if (old != 0) return true;                      // strip gg was there first and does it itself
        if (a.ver) {
            idx[0] = ((a.ver_i0 + (gg >> 1)) * a.ver_ld + a.ver_j0 + cp) * (int)cholq::VS;
            if (!panel_wait_ge(a.ver, idx, 1, a.ver_need, a.dinfo, sh + 1, a.abort)) return false;
        }
        for (int c = 0; c < cp; ++c) {
            idx[0] = F0 + gg * PW_MAX + c;
            idx[1] = F0 + cp * PW_MAX + c;
            if (!panel_wait(a.flags, idx, 2, a.dinfo, sh + 1, a.abort)) return false;
            panel_product(s, -1.0, tileptr(gg, c), a.lda, tileptr(cp, c), a.lda, 1.0, tileptr(gg, cp), a.lda);
        }
        panel_publish_val(word, 3);
        return true;
    }
    const int gb = g - a.NH;
    if (a.tiles) {
        // ---- one tile (r, cp) of the rows below: left-looking -- it takes the columns c < cp as X(r, c) (its row's
        // progress word) and L(cp, c) (diagonal strip cp) appear, is solved on the early hand-off of leaf cp, and moves its
        // row's progress on.  Waits only for smaller tickets (same row, earlier column) and for diagonal strips.
        // Tiles are DRAWN in column-major order from a counter (the last word of the same spare block), so a tile's
        // predecessors were drawn before it by workgroups that are running or done -- whatever the number of workgroups.
        const int nbel = R - W, ntiles = nbel * W;
        int *const counter = a.flags + 2 * PFLAG_STRIDE - 1;
        for (;;) {
            if (tid == 0) sh[1] = atomicAdd(counter, 1);
            __syncthreads();
            const int q = sh[1];
            __syncthreads();
            if (q >= ntiles) return true;
            const int cp = q / nbel, r = W + q % nbel;
            const int pword = PFLAG_STRIDE + (r - W);
            if (a.ver) {
                idx[0] = ((a.ver_i0 + (r >> 1)) * a.ver_ld + a.ver_j0 + cp) * (int)cholq::VS;
                if (!panel_wait_ge(a.ver, idx, 1, a.ver_need, a.dinfo, sh + 1, a.abort)) return false;
            }
            for (int c = 0; c < cp; ++c) {
                idx[0] = pword;
                if (!panel_wait_ge(a.flags, idx, 1, c + 1, a.dinfo, sh + 1, a.abort)) return false;
                idx[0] = F0 + cp * PW_MAX + c;
                if (!panel_wait(a.flags, idx, 1, a.dinfo, sh + 1, a.abort)) return false;
                panel_product(s, -1.0, tileptr(r, c), a.lda, tileptr(cp, c), a.lda, 1.0, tileptr(r, cp), a.lda);
            }
            {
                double *X = tileptr(r, cp);
                XTile x;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                trsm_prefetch(X, a.lda, x);
                idx[0] = E0 + cp;
                if (!panel_wait(a.flags, idx, 1, a.dinfo, sh + 1, a.abort)) return false;
                trsm_solve(s, tileptr(cp, cp), a.inv + (size_t)cp * LEAF * LEAF, a.lda, x);
                trsm_store(X, a.lda, x);
            }
            // X went out write-through: drained stores, the barrier, then the row's progress word (as panel_publish_wt)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) __hip_atomic_store((gint *)(a.flags + pword), cp + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cp == W - 1) {
                if (a.tver) panel_publish_val(a.tver + (size_t)(a.tver_r0 + r) * cholq::VS, a.tver_val);
                if (a.abort && tid == 0)
                    __hip_atomic_fetch_add((gint *)(a.abort + (cholq::Q_PROG - cholq::Q_ABORT)), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    // ---- strips below the diagonal block, shared round-robin by the other workgroups
    const int nw = G - W;
    const int r_first = W + (gb - W), r_step = nw > 0 ? nw : R;
    if (a.ver) {
        // task-queue driver: one strip per workgroup here; its W tiles carry the updates of every earlier panel?
        const int vi = a.ver_i0 + (r_first >> 1);
        for (int c = 0; c < W; ++c) idx[c] = (vi * a.ver_ld + a.ver_j0 + c) * (int)cholq::VS;
        if (r_first < R && !panel_wait_ge(a.ver, idx, W, a.ver_need, a.dinfo, sh + 1, a.abort)) return false;
    }
    const bool below_early = a.below_early != 0;
    for (int c = 0; c < W; ++c) {
        bool have_inv = false, have_early = false, have_rows = false;
        for (int r = r_first; r < R; r += r_step) {
            double *X = tileptr(r, c);
            if (c == W - 1 || below_early) {
                // the blocked solve, which can start on E[c], ~20 us before the leaf's full inverse is there (12 us
                // against the 20 of a staged product with the inverse); the updates of the later columns follow below
                XTile x;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                trsm_prefetch(X, a.lda, x);
                if (!have_early) {
                    idx[0] = E0 + c;
                    if (!panel_wait(a.flags, idx, 1, a.dinfo, sh + 1, a.abort)) return false;
                    have_early = true;
                }
                trsm_solve(s, tileptr(c, c), a.inv + (size_t)c * LEAF * LEAF, a.lda, x);
                trsm_store(X, a.lda, x);
                if (c == W - 1) continue;
            } else {
                if (!have_inv) {                           // inv(L_cc) published by strip c's workgroup
                    idx[0] = 2 + c;
                    if (!panel_wait(a.flags, idx, 1, a.dinfo, sh + 1, a.abort)) return false;
                    have_inv = true;
                }
                panel_product(s, 1.0, X, a.lda, a.inv + (size_t)c * LEAF * LEAF, (size_t)LEAF, 0.0, X, a.lda);
            }
            for (int t = 1; t <= W - 1 - c; ++t) {     // columns c+1..W-1 of this strip take the update
                if (t == 1 && !have_rows) {            // ... which needs L(c',c) of the diagonal strips c' in (c, W)
                    int cnt = 0;
                    for (int cc = c + 1; cc < W; ++cc) idx[cnt++] = F0 + cc * PW_MAX + c;
                    if (cnt && !panel_wait(a.flags, idx, cnt, a.dinfo, sh + 1, a.abort)) return false;
                    have_rows = true;
                }
                panel_product(s, -1.0, X, a.lda, tileptr(c + t, c), a.lda, 1.0, tileptr(r, c + t), a.lda);
            }
        }
    }
    if (a.tver && r_first < R) panel_publish_val(a.tver + (size_t)(a.tver_r0 + r_first) * cholq::VS, a.tver_val);
    if (a.abort && tid == 0)
        __hip_atomic_fetch_add((gint *)(a.abort + (cholq::Q_PROG - cholq::Q_ABORT)), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cen && tid == 0) cen[2] = __builtin_amdgcn_s_memrealtime();
    return true;
}

__global__ __launch_bounds__(LT) void panel_kernel(const PanelArgs a)
{
    __shared__ double s[LEAF * ILD];   // the leaf's 128 x 130 block / the chain's 128 x 144 images; the products stage through its first 72 KiB
    __shared__ int sh[2];
    static_assert(2 * tile::BK * 2 * (LEAF + tile::PAD) <= LEAF_LDS && LEAF_LDS <= LEAF * ILD, "product staging and the leaf fit the buffer");
    const int tid = threadIdx.x;
    const int W = a.W, G = a.G;
    // Two tickets.  The diagonal strips -- the chain -- go to workgroups whose id is a multiple of 8, i.e. (with the
    // dispatcher's round-robin) to ONE XCD, so that what a leaf hands to the next strip is found in that XCD's L2
    // and not in memory; the strips below go to everybody else, and to the leftovers of the first kind.  Arrival
    // order within each kind: a workgroup still only waits for flags of workgroups that started before it or of
    // diagonal strips, which the first eligible workgroups to arrive take (the placement is a speed-only assumption).
    if (tid == 0) {
        int t = -1;
        if ((blockIdx.x & 7) == 0) {
            t = atomicAdd(a.flags, 1);
            if (t >= W) t = -1;
        }
        if (t < 0) t = W + atomicAdd(a.flags + 1, 1);
        sh[0] = t;
    }
    __syncthreads();
    const int g = sh[0];
    __syncthreads();
    if (g >= G + a.NH) return;
    (void)panel_strip(a, g, s, sh);
}

// The task-queue driver's form (cholq.h): ONE launch walks all panels of the block.  Workgroup b is strip b of every
// panel -- diagonal strip b while b < W, else row strip b - W of the next diagonal block -- and goes from one panel to the
// next without a kernel boundary: what it waits for are the version counters of its tiles.  (One launch per panel put 31
// command-processor dispatches on the path every worker spins on, and once in a few hundred factorisations one of them
// came 1.5 s late: tools/queue_stress.py.)

__global__ __launch_bounds__(LT) void panel_seq_kernel(const PanelSeq q)
{
    __shared__ double s[LEAF * ILD];
    __shared__ int sh[2];
    const int g = blockIdx.x;
    for (int k = 0; k < q.nblk; ++k) {
        const int k0 = q.pstart[k], w = q.pstart[k + 1] - k0, wnext = k + 1 < q.nblk_all ? q.pstart[k + 2] - q.pstart[k + 1] : 0;
        PanelArgs a{};
        a.P = q.A + k0 + (size_t)k0 * q.lda; a.lda = q.lda;
        a.W = w / LEAF;
        a.R = a.G = (w + wnext) / LEAF;
        a.below_early = q.tiles;
        a.NH = (q.helpers && a.W > 2 && a.G + (a.W - 1) * (a.W - 2) / 2 <= (int)gridDim.x) ? (a.W - 1) * (a.W - 2) / 2 : 0;
        if (q.tiles && wnext > 0 && a.W >= 2 && (int)gridDim.x - a.W - a.NH >= 1) {
            a.tiles = 1;
            a.G = a.W + min((int)gridDim.x - a.W - a.NH, (a.R - a.W) * a.W);
        }
        a.inv = q.inv + (size_t)(k0 / LEAF) * LEAF * LEAF;
        a.dinfo = q.dinfo; a.goff = q.goff + k0;
        a.flags = q.flags + (size_t)(k0 / LEAF) * PFLAG_STRIDE;
        a.dbg = nullptr;
        a.ver = q.ver; a.ver_ld = q.ver_ld; a.ver_i0 = k0 / cholq::TM; a.ver_j0 = k0 / cholq::TN; a.ver_need = k0 / LEAF;
        a.tver = q.tver; a.tver_r0 = k0 / LEAF; a.tver_val = (k0 + w) / LEAF;
        a.abort = q.abort;
        a.census = (q.census && k < (int)cholq::TRACE_PANELS) ? q.census + 4 * cholq::TRACE_PANEL_WGS * (size_t)k : nullptr;
        if (g < a.G + a.NH && !panel_strip(a, g, s, sh)) return;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
}

// Many independent factorisations of order <= PW_MAX leaves side by side in ONE launch (batch.hip: the population of a
// CMA-ES generation, python/05_tokamak/Split_SympGPR/main.py:63-66): each problem is a single panel whose W diagonal strips
// are W workgroups running the chain above on their own matrix.  Tickets in arrival order: ticket t is strip t % W of
// problem t / W, so a strip only ever waits for strips with smaller tickets -- resident or finished, whatever number of
// workgroups the chip holds at once.

__global__ __launch_bounds__(LT) void panel_batch_kernel(const PanelBatch q)
{
    __shared__ double s[LEAF * ILD];
    __shared__ int sh[2];
    if (threadIdx.x == 0) sh[0] = atomicAdd(q.ticket, 1);
    __syncthreads();
    const int t = sh[0];
    __syncthreads();
    const int p = t / q.G, g = t - p * q.G;      // (diagonal strips 0 .. W-1 hold the smallest tickets of their problem)
    if (p >= q.nbatch) return;
    PanelArgs a{};
    a.P = q.A + (size_t)p * q.stride_a + (size_t)q.k0 + (size_t)q.k0 * q.lda; a.lda = q.lda;
    a.W = q.W; a.R = q.R; a.G = q.G;
    a.inv = q.inv + (size_t)p * q.stride_inv + (size_t)(q.k0 / (int)LEAF) * LEAF * LEAF;
    a.dinfo = q.info + p; a.goff = q.k0;
    a.flags = q.flags + (size_t)p * PFLAG_STRIDE;
    a.below_early = 1;            // (no helpers, no tiles here: a strip may only wait for smaller tickets, whatever the batch size)
    (void)panel_strip(a, g, s, sh);
}

}  // namespace

int launch_leaf(int nb, double *A, size_t lda, double *inv, int *dinfo, int goff, int mode, unsigned long long *stamps, hipStream_t st)
{
    hipLaunchKernelGGL(leaf_kernel, dim3(1), dim3(LT), 0, st, nb, A, lda, inv, dinfo, goff, mode, stamps);
    SGPR_CHECK_LAUNCH();
    return 0;
}

int launch_panel(const PanelArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(panel_kernel, dim3(panel_grid(a.G, a.NH, a.W)), dim3(LT), 0, st, a);
    SGPR_CHECK_LAUNCH();
    return 0;
}

int launch_panel_seq(const PanelSeq &q, int grid, hipStream_t st)
{
    hipLaunchKernelGGL(panel_seq_kernel, dim3(grid), dim3(LT), 0, st, q);
    SGPR_CHECK_LAUNCH();
    return 0;
}

int launch_panel_batch(const PanelBatch &q, hipStream_t st)
{
    hipLaunchKernelGGL(panel_batch_kernel, dim3((unsigned)(q.nbatch * q.G)), dim3(LT), 0, st, q);
    SGPR_CHECK_LAUNCH();
    return 0;
}

}  // namespace sgpr
