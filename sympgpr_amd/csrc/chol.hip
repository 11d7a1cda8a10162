// chol.hip -- lower Cholesky factor on one MI355X: recursion, look-ahead driver, potrf().  Host code only.
//
// Replaces scipy.linalg.cholesky(Ky, lower=True) -> LAPACK dpotrf of python/functions/func.py:165-177,184-186,193-195
// (the two solve_triangular -> dtrtrs calls there: solve.hip).
//
// Structure (right-looking, recursively blocked): at every level
//     factor the leading block  ->  panel solve A21 := A21 L11^-T  ->  trailing update
//     A22 -= A21 A21^T (SYRK, lower tiles only)  ->  factor A22,
// with the split at a multiple of LEAF near the middle, so almost all of the n^3/3 flop are
// large-k GEMM/SYRK calls on the fp64 MFMA kernel (gemm_f64.hip) and the trailing matrix is
// re-read log2(n/LEAF) times instead of n/nb times.  The recursion bottoms out in LEAF = 128
// diagonal blocks that ONE workgroup factors entirely in LDS (128 x 129 fp64 = 129 KiB of the
// CU's 160 KiB) and then inverts in place; the inverse (LEAF x LEAF, zero upper) is kept in
// the workspace so that every panel solve and every triangular solve below is a multiply with
// inv(L_leaf) -- i.e. GEMM work on the matrix cores instead of a substitution.
//
// The pieces around this file (chol.h): panel.hip the leaf kernel and the persistent panel kernel, cholq.hip the task-queue driver, solve.hip
// the triangular solves, streams.hip the streams and events, chol_plan.hip every decision that is host arithmetic.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cholq.h"
#include "common.h"
#include "strassen.h"
#include "leaf.h"
#include "chol.h"
#include "panel.h"
#include "streams.h"

namespace sgpr {

namespace {

using namespace leaf;   // LEAF_FACTOR
using cplan::split;

unsigned long long *g_panel_dbg = nullptr;   // debug builds only (one factorisation at a time there); never read otherwise

}  // namespace

int trsm_rec(int m, int n, const double *L, size_t ldl, double *B, size_t ldb, int off, const Ctx &c)
{
    if (n <= LEAF) {
        // B := B inv(L)^T, in place: one column tile (n <= 128), every workgroup owns full rows
        return gemm_nt(m, n, n, 1.0, B, ldb, c.inv + (size_t)(off / LEAF) * LEAF * LEAF, LEAF, 0.0,
                       B, ldb, 0, 0, c.st);
    }
    const int n1 = split(n), n2 = n - n1;
    int rc = trsm_rec(m, n1, L, ldl, B, ldb, off, c);
    if (rc) return rc;
    // B2 -= B1 L21^T
    if (c.strassen) rc = strassen_top_gemm(m, n2, n1, -1.0, B, ldb, L + n1, ldl, 1.0, B + (size_t)n1 * ldb, ldb, 0, &c.rec, &c.top, c.st);
    else            rc = gemm_nt(m, n2, n1, -1.0, B, ldb, L + n1, ldl, 1.0, B + (size_t)n1 * ldb, ldb, 0, 0, c.st);
    if (rc) return rc;
    return trsm_rec(m, n2, L + n1 + (size_t)n1 * ldl, ldl, B + (size_t)n1 * ldb, ldb, off + n1, c);
}

namespace {

int potrf_rec(int n, double *A, size_t lda, int off, const Ctx &c)
{
    if (n <= LEAF) return launch_leaf(n, A, lda, c.inv + (size_t)(off / LEAF) * LEAF * LEAF, c.dinfo, off, (int)LEAF_FACTOR, nullptr, c.st);
    // mid-size blocks (also the halves a large recursive factorisation splits into): blocked
    // right-looking with the next panel on a side stream
    if (n > 4 * LEAF && n <= c.la_max) return potrf_lookahead(n, A, lda, c, 0, off);
    const int n1 = split(n), n2 = n - n1;
    double *A21 = A + n1, *A22 = A + n1 + (size_t)n1 * lda;
    int rc = potrf_rec(n1, A, lda, off, c);
    if (rc) return rc;
    rc = trsm_rec(n2, n1, A, lda, A21, lda, off, c);
    if (rc) return rc;
    // SYRK, lower (large ones: split around their square off-diagonal part, which takes the Strassen front end)
    if (c.strassen) rc = strassen_top_gemm(n2, n2, n1, -1.0, A21, lda, A21, lda, 1.0, A22, lda, 1, &c.rec, &c.top, c.st);
    else            rc = gemm_nt(n2, n2, n1, -1.0, A21, lda, A21, lda, 1.0, A22, lda, 1, 0, c.st);
    if (rc) return rc;
    return potrf_rec(n2, A22, lda, off + n1, c);
}

}  // namespace

// [ leaf inverses | hand-off words | two n-vectors the strip solves publish their segments through | the queue's part ]
size_t potrf_workspace(int n) { return cplan::work_layout(n, n <= 0 ? 0 : cholq::ws_bytes(n)).total; }

namespace {

// Panel k of the look-ahead driver in its multi-launch forms (the persistent panel kernel does not take the shape, or an A/B
// run asks for them; tunable "la_panel"): 0 "column": leaf column by leaf column, factor the 128 x 128 leaf, multiply the
// rows below by its inverse, fold that column into the panel's remaining columns (3 launches per leaf column; round 1's
// default); 1 folds left-looking instead; 2 factors the diagonal block recursively and then solves the rows below (19
// launches for nb = 512).  Akk: the panel's diagonal block, w its width, rows = w + the rows below, goff its global index;
// cp: the context of the P stream.
int panel_multi_launch(int pmode, int rows, int w, double *Akk, size_t lda, int goff, const Ctx &cp)
{
    const bool left = pmode != 2, right_in = pmode == 0 || pmode == 3;
    const int below = rows - w;
    const hipStream_t sp = cp.st;
    if (!left) {
        int rc = potrf_rec(w, Akk, lda, goff, cp);
        if (rc) return rc;
        if (below > 0) rc = trsm_rec(below, w, Akk, lda, Akk + w, lda, goff, cp);
        return rc;
    }
    for (int c0 = 0; c0 < w; c0 += LEAF) {
        const int nj = std::min((int)LEAF, w - c0), mrows = rows - c0;
        double *Pj = Akk + c0 + (size_t)c0 * lda;          // P[c0:, c0:c0+nj]
        int rc;
        if (!right_in && c0 > 0 &&
            (rc = gemm_nt(mrows, nj, c0, -1.0, Akk + c0, lda, Akk + c0, lda, 1.0, Pj, lda, 0, 0, sp)))
            return rc;
        double *invj = cp.inv + (size_t)((goff + c0) / LEAF) * LEAF * LEAF;
        if ((rc = launch_leaf(nj, Pj, lda, invj, cp.dinfo, goff + c0, (int)LEAF_FACTOR, nullptr, sp))) return rc;
        if (mrows > nj && (rc = gemm_nt(mrows - nj, nj, nj, 1.0, Pj + nj, lda, invj, LEAF, 0.0, Pj + nj, lda, 0, 0, sp)))
            return rc;
        const int ncols = w - c0 - nj;
        if (right_in && ncols > 0 &&
            (rc = gemm_nt(mrows - nj, ncols, nj, -1.0, Pj + nj, lda, Pj + nj, lda, 1.0, Pj + nj + (size_t)nj * lda, lda, 1, 0, sp)))
            return rc;
    }
    return 0;
}

}  // namespace

// Right-looking blocked factorisation with one panel of look-ahead on a side stream -- the form
// used below ~50k, where the recursion's serial chain of leaves and small panel solves would leave
// most of the chip idle.  Per block column k (width nb):
//     P stream:  factor A(k,k) (recursively, leaves in LDS), solve the panel below it
//     U stream:  U1 = update of block column k+1 only  ->  signals P to start panel k+1
//                U2 = the rest of the trailing update (the big MFMA SYRK), runs beside panel k+1
// Measured (factor stage, ms, recursive -> this): n = 8192 21.9 -> 16.4, 16384 66 -> 53,
// 32768 270 -> 240, 49152 766 -> 705, 65536 1537 -> 1578 (so the recursion takes over there).
// The overlap is partial: every CU is held by a workgroup of the big update for ~100 us at a time,
// so the panel's short dependent kernels queue behind them (they run 2x longer than alone).
// Reserving CUs for the panel with a CU-masked stream was tried and is slower overall (the update
// loses 6 % of the chip and the tile map its 256-CU geometry).
// The numbers are the same operations in a different order; the leaf workspace layout is shared with
// the recursive driver, so the solves do not care which one produced L.
// What is decided here is only what needs the device: streams, events, launches.  The block schedule, every panel's
// geometry and the chain_bound switch are chol_plan.hip's.
int potrf_lookahead(int n, double *A, size_t lda, const Ctx &c, int nb, int off0)
{
    if (nb == 0 && c.qws && c.flags && cholq::eligible(n) && (lda & 1) == 0 && (((uintptr_t)A & 15) == 0) && off0 % LEAF == 0) {
        const int rq = potrf_queue(n, A, lda, c, off0);
        if (rq <= 0) return rq;                 // done, or a real error; 1: not available here
    }
    hipStream_t sp = nullptr;
    {
        int dev = -1;
        const int rc0 = side_stream(c.st, &sp, &dev);
        if (rc0) return rc0;
    }
    // Panel kernel usable?  (The multi-launch panels remain for shapes it does not take and for A/B runs.)
    static const int pmode = (int)tune("la_panel", 3);     // 3: the persistent panel kernel; 1 left-looking, 2 recursive, 0 column-wise multi-launch panels
    const bool fused_cap = pmode == 3 && c.flags && n % LEAF == 0 && (lda & 1) == 0 && (((uintptr_t)A & 15) == 0) &&
                           off0 % LEAF == 0;
    const std::vector<int> starts = cplan::la_starts(n, nb, fused_cap);
    const int nblk = (int)starts.size() - 1;
    int wmax = 0;
    for (int k = 0; k < nblk; ++k) wmax = std::max(wmax, starts[k + 1] - starts[k]);
    EventSet es;
    {
        const int rc0 = es.create(3 * (size_t)nblk + 3);
        if (rc0) return rc0;
    }
    std::vector<hipEvent_t> &ev = es.ev;
    const hipStream_t su = c.st;
    Ctx cp{c.inv, c.dinfo, sp, 0, c.flags};
    // Panel k = diagonal block + everything below it.  Default: ONE launch of the persistent panel
    // kernel (panel.hip), with the geometry the planner gives it; else panel_multi_launch.
    const bool fused_ok = fused_cap && wmax % LEAF == 0 && wmax / LEAF <= PW_MAX;
    auto panel = [&](int k) -> int {   // on the P stream
        const int k0 = starts[k], w = starts[k + 1] - k0, rows = n - k0, below = rows - w;
        double *Akk = A + k0 + (size_t)k0 * lda;
        if (!fused_ok) return panel_multi_launch(pmode, rows, w, Akk, lda, off0 + k0, cp);
        const cplan::PanelGeom g = cplan::panel_geometry(rows, w, k > 0 ? starts[k] - starts[k - 1] : 0, k);
        PanelArgs pa{};
        pa.P = Akk; pa.lda = lda;
        pa.R = g.R; pa.W = g.W; pa.G = g.G; pa.NH = g.NH;
        pa.below_early = g.below_early; pa.tiles = g.tiles;
        const int t0 = (off0 + k0) / LEAF;
        pa.inv = cp.inv + (size_t)t0 * LEAF * LEAF;
        pa.dinfo = cp.dinfo; pa.goff = off0 + k0;
        pa.flags = c.flags + (size_t)t0 * PFLAG_STRIDE;
        pa.dbg = (PANEL_DBG && g_panel_dbg) ? g_panel_dbg + (size_t)16 * t0 : nullptr;
        const int rc = launch_panel(pa, sp);
        if (rc) return rc;
        if (g.split) return trsm_rec(below, w, Akk, lda, Akk + w, lda, off0 + k0, cp);
        return 0;
    };
    int rc;
    SGPR_HIP(hipEventRecord(ev[2 * nblk], su));                // the side stream joins the caller's stream ...
    SGPR_HIP(hipStreamWaitEvent(sp, ev[2 * nblk], 0));
    StreamJoin join{sp, su, ev[2 * nblk + 1]};                 // ... and leaves it again on every exit path
    gemm_set_overlap(1);                                       // launches below share the device (profile records)
    // Schedule (P = high-priority side stream, U = the caller's stream):
    //   P:  panel(0);  for k:  [after U2(k-1)]  U1(k) = update of block column k+1 by panel k;  panel(k+1)
    //   U:             for k:  [after panel(k)]  U2(k) = update of everything right of block column k+1
    // U1 is a short launch (m x nb x nb) that fills half the chip at best; on the P stream it runs beside
    // the start of U2(k) instead of in front of it, so the U stream does big updates back to back.
    if ((rc = panel(0))) return rc;
    SGPR_HIP(hipEventRecord(ev[0], sp));
    for (int k = 0; k < nblk; ++k) {
        const int k0 = starts[k], w = starts[k + 1] - k0;
        const int k1 = k0 + w;                                 // first row / column of block column k+1
        if (k1 >= n) break;
        const int w1 = starts[k + 2] - k1, k2 = k1 + w1;
        const double *Lk = A + (size_t)k0 * lda;               // panel k: columns k0..k0+w
        // U1 on P: block column k+1 (rows k1.., columns k1..k2); U2(k-1) has touched it before
        if (k > 0) SGPR_HIP(hipStreamWaitEvent(sp, ev[2 * (k - 1) + 1], 0));
        if ((rc = gemm_nt(n - k1, w1, w, -1.0, Lk + k1, lda, Lk + k1, lda, 1.0, A + k1 + (size_t)k1 * lda, lda, 1, 0, sp)))
            return rc;
        const bool chain_bound = cplan::chain_bound(n - k2, w, w1);   // U2(k) starts only when U1(k) has run
        if (chain_bound) SGPR_HIP(hipEventRecord(ev[2 * nblk + 2 + k], sp));
        if ((rc = panel(k + 1))) return rc;
        SGPR_HIP(hipEventRecord(ev[2 * (k + 1)], sp));
        // U2 on U: the rest of the trailing matrix (rows / columns k2..), as soon as panel k is there
        SGPR_HIP(hipStreamWaitEvent(su, chain_bound ? ev[2 * nblk + 2 + k] : ev[2 * k], 0));
        if (k2 < n &&
            (rc = gemm_nt(n - k2, n - k2, w, -1.0, Lk + k2, lda, Lk + k2, lda, 1.0, A + k2 + (size_t)k2 * lda, lda, 1, 0, su)))
            return rc;
        SGPR_HIP(hipEventRecord(ev[2 * k + 1], su));
    }
    return 0;
}

size_t potrf_batch_flag_bytes(int nbatch) { return ((size_t)nbatch * PFLAG_STRIDE + 1) * sizeof(int); }
int potrf_batch_max_order() { return PW_MAX * (int)LEAF; }

// nbatch lower Cholesky factorisations of order npad (a multiple of 128, <= potrf_batch_max_order()) in one launch;
// `flags`: potrf_batch_flag_bytes(nbatch) bytes of scratch; info[p]: 0 or the 1-based failing minor of problem p
int potrf_batch(int nbatch, int npad, double *A, size_t stride_a, size_t lda, double *inv, size_t stride_inv, int *flags,
                int *info, hipStream_t st)
{
    if (nbatch < 0 || npad <= 0 || npad % LEAF != 0 || npad > PW_MAX * (int)LEAF || lda < (size_t)npad || (lda & 1) != 0 ||
        ((uintptr_t)A & 15) != 0 || (stride_a & 1) != 0) {
        set_error("potrf_batch: bad order / leading dimension / alignment");
        return SGPR_E_ARG;
    }
    if (nbatch == 0) return 0;
    SGPR_HIP(hipMemsetAsync(info, 0, (size_t)nbatch * sizeof(int), st));
    return potrf_batch_panel(nbatch, npad, 0, npad / (int)LEAF, A, stride_a, lda, inv, stride_inv, flags, info, st);
}

// One panel of every problem: columns [k0, k0 + 128 Wd) -- its diagonal block is factored (leaf chain), the rows below it,
// down to row npad, are solved against it.  What a blocked factorisation of the batch composes (batch.hip: two panels with a
// batched rank-k update between them above order 1024).  `flags`: potrf_batch_flag_bytes(nbatch) bytes of scratch of this
// call's own; info is NOT cleared here.
int potrf_batch_panel(int nbatch, int npad, int k0, int Wd, double *A, size_t stride_a, size_t lda, double *inv, size_t stride_inv,
                      int *flags, int *info, hipStream_t st)
{
    const int R = (npad - k0) / (int)LEAF;
    if (nbatch <= 0 || k0 < 0 || k0 % LEAF != 0 || Wd < 1 || Wd > PW_MAX || Wd > R || R > PANEL_G_MAX) {
        set_error("potrf_batch_panel: bad panel");
        return SGPR_E_ARG;
    }
    SGPR_HIP(hipMemsetAsync(flags, 0, potrf_batch_flag_bytes(nbatch), st));
    // workgroups for the strips below the diagonal block: tunable "batch_below" (sgpr_probe_tune), default one per strip
    const int below_max = (int)tune("batch_below", 0);
    const int below = R - Wd <= 0 ? 0 : (below_max > 0 && below_max < R - Wd ? below_max : R - Wd);
    PanelBatch q{A, stride_a, lda, inv, stride_inv, flags, info, flags + (size_t)nbatch * PFLAG_STRIDE, Wd, nbatch, R, k0, Wd + below};
    return launch_panel_batch(q, st);
}

// the calling thread's pooled events (every device); call with no factorisation of this thread in flight
int potrf_trim()
{
    trim_event_pool();
    return strassen_trim();   // ... and the scratch of the Strassen front end's operand sums
}

namespace {

// -DSGPR_PANEL_DBG builds with SGPR_PANEL_DBG set: the chain's time stamps per leaf column (T columns), as medians on stderr
void panel_dbg_report(int n, int T, hipStream_t st)
{
    (void)hipStreamSynchronize(st);
    std::vector<unsigned long long> h(16 * (size_t)T);
    (void)hipMemcpy(h.data(), g_panel_dbg, h.size() * 8, hipMemcpyDeviceToHost);
    (void)hipFree(g_panel_dbg);
    g_panel_dbg = nullptr;
    std::vector<double> d[9];
    for (int t = 1; t + 1 < T; ++t) {
        const unsigned long long *p = &h[16 * t], *q = &h[16 * (t + 1)];
        if (!p[0] || !p[5] || !q[0]) continue;               // first column of a panel: no chain stamps
        d[0].push_back((p[1] - p[0]) * 0.01);                 // E seen -> solve done
        d[1].push_back((p[2] - p[1]) * 0.01);                 // -> F published (at t == 1 entry)
        d[2].push_back((p[3] - p[2]) * 0.01);                 // -> update done
        d[3].push_back((p[4] - p[3]) * 0.01);                 // -> leaf entered
        d[4].push_back(((double)q[0] - (double)p[4]) * 0.01); // leaf entered -> next strip saw E
        d[5].push_back((p[5] - p[4]) * 0.01);                 // whole leaf incl. inverse + publish
        d[3].back() = ((double)p[4] - (double)p[1]) * 0.01;   // solve stored -> leaf entered (the update)
        d[1].back() = (p[6] - p[0]) * 0.01;                   // E seen -> L staged
        d[2].back() = (p[7] - p[6]) * 0.01;                   // -> MFMA part done
        d[6].push_back((p[11] - p[4]) * 0.01);                // leaf entered -> factor done
        d[7].push_back((p[12] - p[11]) * 0.01);               // -> early flag set
        d[8].push_back(((double)q[2] - (double)p[4]) * 0.01); // leaf entered -> next strip at its wait for E
        if (getenv("SGPR_PANEL_DBG_ALL"))
            fprintf(stderr, "  col %3d: leaf entry -> factor %.1f -> flag %.1f | next strip at wait %.1f, saw E %.1f | its solve %.1f, update %.1f\n", t,
                    (p[11] - p[4]) * 0.01, (p[12] - p[4]) * 0.01, ((double)q[2] - (double)p[4]) * 0.01, ((double)q[0] - (double)p[4]) * 0.01,
                    (q[1] - q[0]) * 0.01, ((double)q[4] - (double)q[1]) * 0.01);
    }
    auto med = [](std::vector<double> &x) { std::sort(x.begin(), x.end()); return x.empty() ? 0.0 : x[x.size() / 2]; };
    fprintf(stderr, "panel chain n=%d (%zu columns): E seen -> solve stored %.1f | E seen -> staged %.1f | -> MFMA part done %.1f | (solve stored -> leaf entry %.1f) | "
            "leaf entry -> next E seen %.1f (factor %.1f, -> flag set %.1f; next strip at its wait %.1f) | whole leaf %.1f us\n", n, d[0].size(), med(d[0]), med(d[1]), med(d[2]), med(d[3]), med(d[4]),
            med(d[6]), med(d[7]), med(d[8]), med(d[5]));
}

}  // namespace

int potrf(int n, double *A, size_t lda, void *work, size_t lwork, int *dinfo, hipStream_t st)
{
    if (n < 0 || (n > 0 && lda < (size_t)n)) { set_error("potrf: bad n / lda"); return SGPR_E_ARG; }
    const size_t qbytes = n > 0 ? cholq::ws_bytes(n) : 0;
    const cplan::WorkLayout lay = cplan::work_layout(n, qbytes);
    if (lwork < lay.total) { set_error("potrf: workspace too small"); return SGPR_E_ARG; }
    SGPR_HIP(hipMemsetAsync(dinfo, 0, sizeof(int), st));
    if (n == 0) return 0;
    // hand-off flags of the panel kernel (behind the leaf inverses): zero before every factorisation
    int *flags = reinterpret_cast<int *>(static_cast<char *>(work) + lay.flags);
    SGPR_HIP(hipMemsetAsync(flags, 0, lay.flag_bytes, st));
    // blocked + look-ahead for mid sizes and for the mid-size blocks of a large recursive
    // factorisation, recursive above (measured crossover; SGPR_POTRF=rec|la overrides)
    static const int mode = [] { const char *e = getenv("SGPR_POTRF"); return !e ? 0 : (e[0] == 'r' ? 1 : 2); }();
    static const int nb_env = [] { const char *e = getenv("SGPR_POTRF_NB"); return e ? atoi(e) : 0; }();
    const int la_max_env = cplan::la_max_value();
    potrf_clear_queue_mark();
    Ctx c{static_cast<double *>(work), dinfo, st, mode == 1 ? 0 : la_max_env, flags};
    if (qbytes > 0) c.qws = static_cast<char *>(work) + lay.queue;
    c.strassen = true;
    c.rec = strassen_rec_values();
    c.top = strassen_top_values();
    if (n > c.la_max && n > LEAF) {
        // size the operand-sum scratch once, before the first launch: the largest need over the plans of this order
        size_t need[2];
        potrf_strassen_need(n, need);
        strassen_reserve(need[0], need[1], st);   // both levels' operand sums, or the inner level's alone if that does not fit
        strassen_top_reserve(potrf_strassen_top_need(n), st);     // the top level's buffer; without it that level is off
    }
    const bool dbg = PANEL_DBG && getenv("SGPR_PANEL_DBG") != nullptr;
    const int T = (n + LEAF - 1) / LEAF;
    if (dbg) {
        (void)hipMalloc((void **)&g_panel_dbg, sizeof(unsigned long long) * 16 * T);
        (void)hipMemset(g_panel_dbg, 0, sizeof(unsigned long long) * 16 * T);
    }
    int rc;
    if (mode == 2 || (nb_env > 0 && mode == 0 && n > 4 * LEAF && n <= c.la_max))
        rc = potrf_lookahead(n, A, lda, c, nb_env > 0 ? nb_env : 0, 0);
    else
        rc = potrf_rec(n, A, lda, 0, c);
    if (dbg) panel_dbg_report(n, T, st);
    return rc;
}

// diagnostic: one leaf factorisation with per-phase cycle counts (load, diag, panel, update,
// write-back, inv diag, inv rows, tail)
int leaf_probe(double *A, size_t lda, double *inv, int *dinfo, unsigned long long *stamps, hipStream_t st)
{
    return launch_leaf((int)LEAF, A, lda, inv, dinfo, 0, (int)LEAF_FACTOR, stamps, st);
}

}  // namespace sgpr
