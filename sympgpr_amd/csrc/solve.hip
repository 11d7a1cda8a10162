// solve.hip -- the triangular solves against a factor of potrf() (or of leaf_inverses()).
//
// Replaces the two solve_triangular -> dtrtrs calls of python/functions/func.py:165-177,184-186,193-195.  Every solve is a
// multiply with the leaf inverses kept in the factor's workspace: one right-hand side by the strip kernels of trsv.hip or, for
// small orders and odd layouts, by the recursion below; blocks of right-hand sides by trsm.hip or by the recursions over the
// grid-wide MFMA kernel (trsm_rec in chol.hip, trsm_rl_rec here).
#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "cholq.h"
#include "common.h"
#include "strassen.h"
#include "gemm_tile.h"
#include "leaf.h"
#include "chol.h"
#include "panel.h"

namespace sgpr {

namespace {

using namespace leaf;
using cplan::split;

// b(nb) := inv(L) b  or  inv(L)^T b   (inv: LEAF x LEAF lower, zero upper).
// 1024 threads: row i = t & 127, k-slice = t >> 7 (8 slices of 16): sixteen independent loads per
// thread instead of one 128-long dependent chain (25 us -> ~3 us per call).
constexpr int MV_T = 1024;
__global__ __launch_bounds__(MV_T) void leaf_matvec_kernel(int nb, const double *inv, double *b,
                                                           int trans)
{
    __shared__ double sb[LEAF];
    __shared__ double part[MV_T / LEAF][LEAF];
    const int t = threadIdx.x, i = t & (LEAF - 1), ks = t >> 7;
    if (t < LEAF) sb[t] = t < nb ? b[t] : 0.0;
    __syncthreads();
    double acc = 0.0;
#pragma unroll
    for (int kk = 0; kk < LEAF / (MV_T / LEAF); ++kk) {
        const int k = ks * (LEAF / (MV_T / LEAF)) + kk;
        // inv is zero above the diagonal and outside nb x nb, so no triangular bounds are needed
        const double m = trans ? inv[k + i * LEAF] : inv[i + k * LEAF];
        acc = __builtin_fma(m, sb[k], acc);
    }
    part[ks][i] = acc;
    __syncthreads();
    if (t < nb) {
        double r = 0.0;
#pragma unroll
        for (int q = 0; q < MV_T / LEAF; ++q) r += part[q][t];
        b[t] = r;
    }
}

// b(n) := L^-1 b (trans = 0) or L^-T b (trans = 1) for a diagonal block of up to TRSV_BLOCK rows in
// ONE single-workgroup launch: the leaf-by-leaf substitution (x_j = inv(L_jj) b_j, off-diagonal
// leaf rows folded in before it) that the recursion would spread over 2 n/128 - 1 launches.  A
// triangular solve with one right-hand side is a chain of dependent ~10 us launches otherwise --
// 510 of them for n = 16384, where the solve stage was a tenth of the whole fit.
constexpr int TRSV_BLOCK = 512;
__global__ __launch_bounds__(MV_T) void trsv_block_kernel(int n, const double *L, size_t ldl,
                                                          const double *inv, double *b, int trans)
{
    __shared__ double sx[TRSV_BLOCK];               // b on entry, x as it is produced
    __shared__ double part[MV_T / LEAF][LEAF];
    const int t = threadIdx.x, i = t & (LEAF - 1), ks = t >> 7;    // 128 rows x 8 slices
    const int lane = t & 63, wave = t >> 6;
    for (int r = t; r < TRSV_BLOCK; r += MV_T) sx[r] = r < n ? b[r] : 0.0;
    __syncthreads();
    const int nl = (n + LEAF - 1) / LEAF;
    for (int jj = 0; jj < nl; ++jj) {
        const int j = trans ? nl - 1 - jj : jj;
        const int r0 = j * LEAF, nj = min(LEAF, n - r0);
        // ---- fold the already known x into b_j
        if (!trans) {
            // b_j[i] -= sum_{c < r0} L[r0 + i, c] x[c]: rows contiguous -> thread (i, slice) strides the columns
            // (r0 is a multiple of 128: 16 columns per slice and leaf, four independent chains)
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            if (i < nj) {
                const double *row = L + (size_t)(r0 + i);
                for (int c = ks; c < r0; c += 4 * (MV_T / LEAF)) {
                    const double l0 = row[(size_t)c * ldl], l1 = row[(size_t)(c + 8) * ldl];
                    const double l2 = row[(size_t)(c + 16) * ldl], l3 = row[(size_t)(c + 24) * ldl];
                    a0 = __builtin_fma(l0, sx[c], a0);
                    a1 = __builtin_fma(l1, sx[c + 8], a1);
                    a2 = __builtin_fma(l2, sx[c + 16], a2);
                    a3 = __builtin_fma(l3, sx[c + 24], a3);
                }
            }
            const double acc = (a0 + a1) + (a2 + a3);
            part[ks][i] = acc;
            __syncthreads();
            if (t < nj) {
                double r = 0.0;
#pragma unroll
                for (int q = 0; q < MV_T / LEAF; ++q) r += part[q][t];
                sx[r0 + t] -= r;
            }
        } else {
            // b_j[c] -= sum_{r >= r0 + LEAF} L[r, r0 + c] x[r]: one wave per column, lanes stride the rows
            const int rb = r0 + LEAF;
            constexpr int NWV = MV_T / 64, CPW = LEAF / NWV;   // 16 waves, 8 columns each
            double acc[CPW];
#pragma unroll
            for (int q = 0; q < CPW; ++q) acc[q] = 0.0;
            const double *col0 = L + (size_t)(r0 + wave) * ldl;
            for (int r = rb + lane; r < n; r += 64) {          // the 8 columns' loads go out together
                const double xr = sx[r];
#pragma unroll
                for (int q = 0; q < CPW; ++q) {
                    const int c = wave + q * NWV;
                    const double v = c < nj ? col0[(size_t)q * NWV * ldl + r] : 0.0;
                    acc[q] = __builtin_fma(v, xr, acc[q]);
                }
            }
#pragma unroll
            for (int q = 0; q < CPW; ++q) {
                double a = acc[q];
                for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
                if (lane == 0) part[0][wave + q * NWV] = a;
            }
            __syncthreads();
            if (t < nj) sx[r0 + t] -= part[0][t];
        }
        __syncthreads();
        // ---- x_j = inv(L_jj) b_j  or  inv(L_jj)^T b_j  (inv is zero above the diagonal and outside nj x nj)
        const double *iv = inv + (size_t)j * LEAF * LEAF;
        double acc = 0.0;
#pragma unroll
        for (int kk = 0; kk < LEAF / (MV_T / LEAF); ++kk) {
            const int k = ks * (LEAF / (MV_T / LEAF)) + kk;
            const double m = trans ? iv[k + i * LEAF] : iv[i + k * LEAF];
            acc = __builtin_fma(m, sx[r0 + k], acc);
        }
        __syncthreads();                            // every thread has read b_j before it is overwritten
        part[ks][i] = acc;
        __syncthreads();
        if (t < nj) {
            double r = 0.0;
#pragma unroll
            for (int q = 0; q < MV_T / LEAF; ++q) r += part[q][t];
            sx[r0 + t] = r;
        }
        __syncthreads();
    }
    for (int r = t; r < n; r += MV_T) b[r] = sx[r];
}

// b(n) := L^-1 b (trans = 0) or L^-T b (trans = 1), recursively: forward solves the first part, folds it into the second
// and goes on there; backward the other way round.
int trsv_rec(int n, const double *L, size_t ldl, double *b, int trans, int off, const Ctx &c)
{
    if (n <= TRSV_BLOCK) {
        const double *inv = c.inv + (size_t)(off / LEAF) * LEAF * LEAF;
        if (n <= LEAF) hipLaunchKernelGGL(leaf_matvec_kernel, dim3(1), dim3(MV_T), 0, c.st, n, inv, b, trans);
        else           hipLaunchKernelGGL(trsv_block_kernel, dim3(1), dim3(MV_T), 0, c.st, n, L, ldl, inv, b, trans);
        SGPR_CHECK_LAUNCH();
        return 0;
    }
    const int n1 = split(n), n2 = n - n1;
    const double *L21 = L + n1, *L22 = L + n1 + (size_t)n1 * ldl;
    int rc;
    if (!trans) {
        if ((rc = trsv_rec(n1, L, ldl, b, 0, off, c))) return rc;
        if ((rc = gemv_n_sub(n2, n1, L21, ldl, b, b + n1, c.st))) return rc;  // b2 -= L21 b1
        return trsv_rec(n2, L22, ldl, b + n1, 0, off + n1, c);
    }
    if ((rc = trsv_rec(n2, L22, ldl, b + n1, 1, off + n1, c))) return rc;
    if ((rc = gemv_t_sub(n2, n1, L21, ldl, b + n1, b, c.st))) return rc;      // b1 -= L21^T b2
    return trsv_rec(n1, L, ldl, b, 1, off, c);
}

// B (m x n) := B L^-1 (L lower, its leaf inverses in the workspace): the backward half of a
// multi-right-hand-side solve with the right-hand sides stored as ROWS.
//   X2 = B2 L22^-1 ;  B1 -= X2 L21 ("NN" product) ;  X1 = B1 L11^-1
int trsm_rl_rec(int m, int n, const double *L, size_t ldl, double *B, size_t ldb, int off, const Ctx &c)
{
    if (n <= LEAF)  // B := B inv(L), in place (one column tile, workgroups own full rows)
        return gemm_nn(m, n, n, 1.0, B, ldb, c.inv + (size_t)(off / LEAF) * LEAF * LEAF, LEAF, 0.0, B, ldb, c.st);
    const int n1 = split(n), n2 = n - n1;
    int rc = trsm_rl_rec(m, n2, L + n1 + (size_t)n1 * ldl, ldl, B + (size_t)n1 * ldb, ldb, off + n1, c);
    if (rc) return rc;
    rc = gemm_nn(m, n1, n2, -1.0, B + (size_t)n1 * ldb, ldb, L + n1, ldl, 1.0, B, ldb, c.st);
    if (rc) return rc;
    return trsm_rl_rec(m, n1, L, ldl, B, ldb, off, c);
}

// a solve reads the leaf inverses of the factor's workspace and nothing else of the context
Ctx solve_ctx(const void *work, hipStream_t st) { return Ctx{const_cast<double *>(static_cast<const double *>(work)), nullptr, st}; }

// The strip kernels (trsv.hip) take over above one block of the single-workgroup kernel; their ticket /
// progress words live in the flag area behind the leaf inverses (idle once the factor exists).
// SGPR_TRSV=rec keeps the recursive GEMV form (A/B runs).
bool use_strips(int n, const double *L, size_t ldl)
{
    static const bool off = [] { const char *e = getenv("SGPR_TRSV"); return e && e[0] == 'r'; }();
    return !off && n > TRSV_BLOCK && trsv_strips_ok(n, L, ldl);
}
// (the queue's part lies behind both: its size does not move them)
int *solve_state(int n, const void *work)
{
    return reinterpret_cast<int *>(const_cast<char *>(static_cast<const char *>(work)) + cplan::work_layout(n, 0).flags);
}
double *solve_pub(int n, const void *work)
{
    return reinterpret_cast<double *>(const_cast<char *>(static_cast<const char *>(work)) + cplan::work_layout(n, 0).pub);
}
// `passes` strip passes (1 or 2) armed on st: 4 zeroed state words and n doubles of all-ones bytes each
int arm_strips(int n, const void *work, int passes, hipStream_t st, int **state, double **pub)
{
    *state = solve_state(n, work);
    *pub = solve_pub(n, work);
    SGPR_HIP(hipMemsetAsync(*state, 0, (size_t)4 * passes * sizeof(int), st));
    SGPR_HIP(hipMemsetAsync(*pub, 0xFF, (size_t)passes * n * sizeof(double), st));
    return 0;
}

// potrs_mat (backward) or its forward half alone, on the path potrs_mat takes for this block
int potrs_mat_passes(int n, const double *L, size_t ldl, const void *work, double *B, size_t ldb, int nrhs, double *scratch,
                     bool backward, hipStream_t st)
{
    if (n <= 0 || nrhs <= 0) return 0;
    if (potrs_mat_uses_strips(n, nrhs, L, ldl)) {
        const double *inv = static_cast<const double *>(work);
        return backward ? potrs_strips(n, L, ldl, inv, B, ldb, nrhs, solve_state(n, work), scratch, st)
                        : trsm_strips_fwd(n, L, ldl, inv, B, ldb, nrhs, solve_state(n, work), scratch, st);
    }
    int rc = transpose(n, nrhs, B, ldb, scratch, (size_t)nrhs, st);
    if (rc) return rc;
    if ((rc = trsm_rlt(nrhs, n, L, ldl, scratch, (size_t)nrhs, work, st))) return rc;
    if (backward && (rc = trsm_rl(nrhs, n, L, ldl, scratch, (size_t)nrhs, work, st))) return rc;
    return transpose(nrhs, n, scratch, (size_t)nrhs, B, ldb, st);
}

}  // namespace

// After a potrs_vec / trsv on this workspace has been waited for: did a strip kernel give up on a hand-off
// (a bounded spin ran out: a bug or a device problem, never a property of the matrix)?  `host8` = the 8 state
// words copied back by the caller (null when the strip kernels were not used for this order).
bool trsv_uses_strips(int n, const double *L, size_t ldl) { return use_strips(n, L, ldl); }

// Waits for the stream and reports a strip solve that gave up on a hand-off (never a property of the matrix).
int solve_status(int n, const double *L, size_t ldl, const void *work, hipStream_t st)
{
    if (n <= 0 || !use_strips(n, L, ldl)) { SGPR_HIP(hipStreamSynchronize(st)); return 0; }
    int h[8] = {};
    SGPR_HIP(hipMemcpyAsync(h, solve_state(n, work), sizeof(h), hipMemcpyDeviceToHost, st));
    SGPR_HIP(hipStreamSynchronize(st));
    if (h[2] || h[6]) { set_error("triangular solve: a hand-off between strips timed out"); return SGPR_E_HIP; }
    return 0;
}
const int *trsv_state(int n, const void *work) { return solve_state(n, work); }

int potrs_vec(int n, const double *L, size_t ldl, void *work, double *b, hipStream_t st)
{
    if (n <= 0) return 0;
    const Ctx c = solve_ctx(work, st);
    int rc;
    if (use_strips(n, L, ldl)) {
        int *state;
        double *pub;
        if ((rc = arm_strips(n, work, 2, st, &state, &pub))) return rc;
        if ((rc = trsv_strips(n, L, ldl, c.inv, b, 0, state, pub, st))) return rc;
        return trsv_strips(n, L, ldl, c.inv, b, 1, state + 4, pub + n, st);
    }
    if ((rc = trsv_rec(n, L, ldl, b, 0, 0, c))) return rc;
    return trsv_rec(n, L, ldl, b, 1, 0, c);
}

// one-sided solve: b := L^-1 b (trans = 0) or L^-T b (trans = 1)
int trsv(int n, const double *L, size_t ldl, void *work, double *b, int trans, hipStream_t st)
{
    if (n <= 0) return 0;
    const Ctx c = solve_ctx(work, st);
    if (use_strips(n, L, ldl)) {
        int *state;
        double *pub;
        const int rc = arm_strips(n, work, 1, st, &state, &pub);
        if (rc) return rc;
        return trsv_strips(n, L, ldl, c.inv, b, trans, state, pub, st);
    }
    return trsv_rec(n, L, ldl, b, trans ? 1 : 0, 0, c);
}

// The two panel solves against the trailing block L[off:, off:] of a factor (off a multiple of LEAF; L points at that
// block, n is its order): the recursion's leaf-aligned offset picks the factor's own leaf inverses from `work`.
int trsm_rlt_off(int m, int n, const double *L, size_t ldl, double *B, size_t ldb, const void *work, int off, hipStream_t st)
{
    if (m <= 0 || n <= 0) return 0;
    if (off < 0 || off % (int)LEAF) { set_error("trsm_rlt_off: offset not on a leaf boundary"); return SGPR_E_ARG; }
    return trsm_rec(m, n, L, ldl, B, ldb, off, solve_ctx(work, st));
}
int trsm_rl_off(int m, int n, const double *L, size_t ldl, double *B, size_t ldb, const void *work, int off, hipStream_t st)
{
    if (m <= 0 || n <= 0) return 0;
    if (off < 0 || off % (int)LEAF) { set_error("trsm_rl_off: offset not on a leaf boundary"); return SGPR_E_ARG; }
    return trsm_rl_rec(m, n, L, ldl, B, ldb, off, solve_ctx(work, st));
}
// ... against the whole factor
int trsm_rlt(int m, int n, const double *L, size_t ldl, double *B, size_t ldb, const void *work, hipStream_t st)
{
    return trsm_rlt_off(m, n, L, ldl, B, ldb, work, 0, st);
}
int trsm_rl(int m, int n, const double *L, size_t ldl, double *B, size_t ldb, const void *work, hipStream_t st)
{
    return trsm_rl_off(m, n, L, ldl, B, ldb, work, 0, st);
}

// Blocks of 2 .. 256 right-hand sides take the one-launch strip solves of trsm.hip (L streamed once per 64 columns);
// more than that is compute-bound and stays with the recursion over the grid-wide MFMA kernel.  SGPR_TRSM=rec: always.
bool potrs_mat_uses_strips(int n, int nrhs, const double *L, size_t ldl)
{
    return nrhs >= 2 && nrhs <= 256 && use_strips(n, L, ldl) && trsm_strips_ok(n, L, ldl);
}
size_t potrs_mat_scratch(int n, int nrhs, const double *L, size_t ldl)
{
    if (n <= 0 || nrhs <= 0) return 8;
    return potrs_mat_uses_strips(n, nrhs, L, ldl) ? trsm_strips_scratch(n) : (size_t)n * nrhs * sizeof(double);
}

// B (n x nrhs) := L^-T L^-1 B.  Few right-hand sides: trsm.hip.  Many: through the MFMA kernel, the right-hand sides
// transposed into rows (scratch, nrhs x n), X^T = B^T L^-T (forward) then X^T L^-1 (backward), transposed back.
int potrs_mat(int n, const double *L, size_t ldl, const void *work, double *B, size_t ldb, int nrhs,
              double *scratch, hipStream_t st)
{
    return potrs_mat_passes(n, L, ldl, work, B, ldb, nrhs, scratch, true, st);
}

// B (n x nrhs) := L^-1 B, the forward half of potrs_mat on the path potrs_mat would take for this block: the strip solves'
// forward passes, or the right-hand sides transposed into rows (scratch, nrhs x n), X^T = B^T L^-T, transposed back.
// scratch: potrs_mat_scratch(n, nrhs, L, ldl) bytes; a give-up of a strip pass is read through solve_status.
int potrs_mat_fwd(int n, const double *L, size_t ldl, const void *work, double *B, size_t ldb, int nrhs,
                  double *scratch, hipStream_t st)
{
    return potrs_mat_passes(n, L, ldl, work, B, ldb, nrhs, scratch, false, st);
}

// leaf inverses of an existing factor (for solves against an L that was not produced by potrf())
int leaf_inverses(int n, const double *L, size_t ldl, void *work, int *dinfo, hipStream_t st)
{
    double *inv = static_cast<double *>(work), *Lw = const_cast<double *>(L);
    for (int off = 0; off < n; off += LEAF) {
        const int nb = n - off < LEAF ? n - off : LEAF;
        const int rc = launch_leaf(nb, Lw + off + (size_t)off * ldl, ldl, inv + (size_t)(off / LEAF) * LEAF * LEAF, dinfo, off,
                                   (int)LEAF_INVERT_ONLY, nullptr, st);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace sgpr
