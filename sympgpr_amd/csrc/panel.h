// panel.h -- the leaf kernel and the persistent panel kernel (panel.hip) as the drivers see them: the limits, the argument
// blocks of the panel kernel's three forms and the launchers.  No HIP type in here, so the host planner (chol_plan.hip) reads the limits from the same place.
#pragma once
#include <algorithm>
#include <cstddef>

namespace sgpr {

constexpr int PW_MAX = 16;                      // leaf columns per panel (nb <= 2048)
constexpr int PFLAG_STRIDE = 2 + 2 * PW_MAX + PW_MAX * PW_MAX + 6;   // ints of flag state per panel (296)
constexpr int PANEL_G_MAX = 256;                // workgroups (each holds a whole CU: 133 KiB of LDS)

struct PanelArgs {
    double *P;        // panel origin: element (k0, k0) of the matrix
    size_t lda;
    int R, W, G;      // row strips (incl. the W diagonal ones), leaf columns, workgroups (diagonal strips + strips below)
    int NH;           // helper workgroups, tickets W .. W+NH-1 (0 or (W-1)(W-2)/2): one per tile (g, c'), 1 <= c' < g < W, of the
                      // diagonal block -- it applies the columns c < c' to that tile so that strip g does not have to
    int below_early;  // strips below: every column by the blocked solve on the early hand-off (not only the last one)
    int tiles;        // rows below the diagonal block TILE by tile (r, c') instead of strip by strip: the G - W workgroups behind the
                      // helpers draw tiles in column-major order; row r's progress (columns solved) in flags[PFLAG_STRIDE + r - W]
                      // -- the words of the panel's second leaf column, which no panel kernel of this schedule uses (needs W >= 2,
                      // R - W < PFLAG_STRIDE)
    double *inv;      // leaf inverses of this panel's W leaves (LEAF x LEAF each)
    int *dinfo;
    int goff;         // global index of the panel's first row / column (LAPACK info)
    unsigned long long *dbg;   // per-leaf-column time stamps (16 each) or null; written only in -DSGPR_PANEL_DBG builds
    int *flags;       // PFLAG_STRIDE ints, zero on entry: [0] ticket, [2 + c] I[c], [2 + PW_MAX + c] E[c], [2 + 2 PW_MAX + r * PW_MAX + c] F[r][c]
    // task-queue driver (cholq.h): the trailing updates of the earlier panels arrive tile by tile instead of behind a
    // kernel boundary.  Diagonal strip g starts once its tiles (row tile ver_i0 + g / 2, column tiles ver_j0 .. ver_j0 + g)
    // carry ver_need updates; `abort` is the queue's give-up word (set here too when a hand-off times out).  Null otherwise.
    // The strips below the diagonal block (there: the rows of the NEXT diagonal block) wait the same way for their W tiles
    // and leave tver[tver_r0 + r] = ver_need + 1 behind (strip r of the panel solved against this panel).
    const int *ver;
    int ver_ld, ver_i0, ver_j0, ver_need;
    int *tver;
    int tver_r0, tver_val;
    int *abort;
    unsigned long long *census;   // diagnostics: 4 words per workgroup (place, start, end, strip), or null
};

#ifdef SGPR_PANEL_DBG
constexpr bool PANEL_DBG = true;
#else
constexpr bool PANEL_DBG = false;    // make EXTRA=-DSGPR_PANEL_DBG + SGPR_PANEL_DBG=1: the chain's time stamps per leaf column
#endif

// panel_seq_kernel: ONE launch walks all panels of a block of the task-queue driver (cholq.hip)
struct PanelSeq {
    double *A;              // origin of the block being factored
    size_t lda;
    int nblk;               // panels this kernel runs: 0 .. nblk-1 (the queue's part of the schedule)
    int nblk_all;           // panels of the whole schedule (the band of panel nblk-1 is the diagonal block of panel nblk, if any)
    const int *pstart;      // nblk_all + 1 panel boundaries (device)
    double *inv;            // leaf inverses of the block
    int *dinfo;
    int goff;               // global index of the block's first row (LAPACK info)
    int *flags;             // hand-off words of the block: panel starting at leaf column t at flags + t * PFLAG_STRIDE
    const int *ver;
    int ver_ld;
    int *tver;
    int *abort;
    unsigned long long *census;
    int helpers, tiles;     // the look-ahead driver's helper workgroups / tile-by-tile rows below (PanelArgs), from the surplus of the grid
};

// panel_batch_kernel: one panel of many independent problems side by side (batch.hip)
struct PanelBatch {
    double *A;              // problem p at A + p * stride_a (column-major, lda), lower triangle filled
    size_t stride_a, lda;
    double *inv;            // leaf inverses of problem p at inv + p * stride_inv (W leaves)
    size_t stride_inv;
    int *flags;             // PFLAG_STRIDE ints per problem, zero on entry
    int *info;              // per problem: 0, the 1-based failing minor, or PANEL_TIMEOUT
    int *ticket;            // one int, zero on entry
    int W, nbatch;          // diagonal strips of this panel (its width / 128)
    int R;                  // row strips from the panel's first row to the end of the matrix (>= W): W .. R-1 are solved against it
    int k0;                 // first row / column of the panel inside its problem (a multiple of 128)
    int G;                  // workgroups per problem: W for the diagonal strips + G - W that share the R - W strips below
};

// workgroups of a panel_kernel launch: at least W with an id that is a multiple of 8 (surplus ones find no ticket and leave)
inline int panel_grid(int G, int NH, int W) { return std::max(G + NH, 8 * (W - 1) + 1); }

#ifdef SGPR_HIP_TYPES
// one launch each on `st`; the grid follows from the arguments (panel_grid; nbatch * G workgroups for a batch)
int launch_panel(const PanelArgs &a, hipStream_t st);
// the leaf kernel alone (one workgroup): factor + invert the nb x nb block at A, or invert only (mode: leaf.h); goff: LAPACK info
int launch_leaf(int nb, double *A, size_t lda, double *inv, int *dinfo, int goff, int mode, unsigned long long *stamps, hipStream_t st);
int launch_panel_seq(const PanelSeq &q, int grid, hipStream_t st);
int launch_panel_batch(const PanelBatch &q, hipStream_t st);
#endif

}  // namespace sgpr
