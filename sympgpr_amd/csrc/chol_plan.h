// chol_plan.h -- the host arithmetic of the Cholesky drivers (chol_plan.hip): where the recursion splits, how the workspace is
// laid out, which blocks the look-ahead driver walks and what geometry each panel kernel gets.  No HIP type in here.
#pragma once
#include <cstddef>
#include <vector>

namespace sgpr {
namespace cplan {

constexpr int LEAF_ORDER = 128;   // = LEAF (common.h; chol.h asserts it)

int split(int n);      // first part of a recursive split: a multiple of the leaf order close to n/2 (>= one leaf, < n)
int la_block(int n);   // the look-ahead driver's uniform block width where the panel kernel is not used
int la_max_value();    // blocks of order <= this go to the look-ahead driver (SGPR_LA_MAX, tunable "la_max")
int walk_la_max();     // ... as the sizing walk sees it (0 under SGPR_POTRF=rec)

// The factor workspace: [ leaf inverses | hand-off words | two n-vectors the strip solves publish their segments through |
// the task-queue driver's part ], byte offsets of each and the total.  queue_bytes: cholq::ws_bytes(n).
struct WorkLayout { size_t inv, flags, flag_bytes, pub, queue, total; };
WorkLayout work_layout(int n, size_t queue_bytes);

// block boundaries of the look-ahead driver for a block of order n: nb > 0 uniform, else by what is left ("la_t0/t1/t2");
// fused_cap: the persistent panel kernel can take this block
std::vector<int> la_starts(int n, int nb, bool fused_cap);

// One panel kernel of the look-ahead driver: `rows` rows from the panel's first row to the end of the block, width w, the
// previous panel's width wprev (k > 0), k = index of the panel.  The members are PanelArgs'; split: the kernel takes the
// diagonal block only (G == W == R) and the rows below go to trsm_rec afterwards.
struct PanelGeom { int R, W, G, NH, below_early, tiles; bool split; };
PanelGeom panel_geometry(int rows, int w, int wprev, int k);
// U2(k) waits for U1(k): rest = order of what U2 updates, w = its k extent, w1 = width of the next panel
bool chain_bound(int rest, int w, int w1);

// the task-queue driver's panel grid for a schedule: workgroups of the widest panel kernel (+ helpers, + tile workgroups),
// and R = CUs per XCD set aside for them (the driver takes the block only while R <= 4)
struct QueueGeom { int band, nh_max, pgrid, R; bool helpers, tiles; };
QueueGeom queue_geometry(const std::vector<int> &starts);

}  // namespace cplan
}  // namespace sgpr
