// chol_plan.hip -- the host arithmetic of the Cholesky drivers (chol_plan.h): the recursion's split, the workspace layout, the
// sizing walk for the Strassen scratch, the look-ahead driver's block schedule and panel geometry, the queue driver's panel grid.
// Host C++ only: no HIP header, no HIP call; tune() and set_error() are all it takes from the library besides the Strassen
// planner (strassen_plan.hip, host C++ too), so the file also compiles on its own (g++ -x c++ -std=c++17) for
// tests/test_chol_plan_cpu.py.  Every tunable is read once, on first use.
#include <algorithm>
#include <cstdlib>

#include "strassen.h"
#include "panel.h"
#include "chol_plan.h"

namespace sgpr {
namespace cplan {

constexpr int LEAF = LEAF_ORDER;

int split(int n)
{
    // first part: a multiple of LEAF close to n/2 (>= LEAF, < n)
    int n1 = ((n / 2 + LEAF - 1) / LEAF) * LEAF;
    if (n1 >= n) n1 -= LEAF;
    return n1;
}

// measured with the left-looking panel (factor ms at nb = 256 / 512 / 1024 / 2048): n = 8192 12.1 / 13.0 /
// 15.2 / 20.1, 16384 49.6 / 43.9 / 46.8 / 56.5, 32768 307 / 250 / 228 / 229, 49152 964 / 770 / 682 / 656
int la_block(int n) { return n <= 4096 ? 256 : (n <= 24576 ? 512 : (n <= 40960 ? 1024 : 2048)); }

// blocks of order <= la_max go to the blocked look-ahead driver, larger ones split recursively
// (SGPR_LA_MAX overrides; measured crossover of round 1)
// tunable "la_max": the same through sgpr_probe_tune (tests that need the recursive driver at a small order)
int la_max_value()
{
    static const int v = [] { const char *e = getenv("SGPR_LA_MAX"); return (int)tune("la_max", e ? atoi(e) : 57344); }();
    return v;
}
int walk_la_max()
{
    static const bool rec_mode = [] { const char *e = getenv("SGPR_POTRF"); return e && e[0] == 'r'; }();
    return rec_mode ? 0 : la_max_value();
}

WorkLayout work_layout(int n, size_t queue_bytes)
{
    WorkLayout w{};
    if (n <= 0) { w.total = 256; return w; }
    const size_t leaves = (size_t)((n + LEAF - 1) / LEAF);
    w.inv = 0;
    w.flags = leaves * LEAF * LEAF * sizeof(double);
    // flag block of the panel that starts at leaf column t: flags + t * PFLAG_STRIDE
    w.flag_bytes = ((leaves * PFLAG_STRIDE * sizeof(int)) + 255) / 256 * 256;
    w.pub = w.flags + w.flag_bytes;
    w.queue = w.pub + ((size_t)2 * n * sizeof(double) + 255) / 256 * 256;
    w.total = w.queue + queue_bytes + 256;
    return w;
}

std::vector<int> la_starts(int n, int nb, bool fused_cap)
{
    // Block schedule.  nb > 0: uniform width (the caller's choice).  nb == 0: widths follow the order of
    // what is left: wide blocks (alone, k = 2048 / 1024 / 512 products run at 61 / 57 / 49 TFLOP/s) while the trailing
    // update is what each step waits for, narrower ones once the chain of leaves is (the chain costs the
    // same per column at any width, and a narrow step loses less to its own update of block column k+1).
    std::vector<int> starts;
    // 2048-wide steps (k = 2048 updates: 61 TFLOP/s) pay off only when the early updates are long enough to
    // hide a 16-leaf chain: measured n = 32768 198.5 -> 194.0 ms, 49152 620 -> 603, but 16384 34.0 -> 35.6
    static const int t0_env = (int)tune("la_t0", 0);
    const int t0 = t0_env > 0 ? t0_env : (n >= 24576 ? 12288 : 1 << 30);
    static const int t1 = (int)tune("la_t1", 6144);   // swept 2048 .. 9216: n = 12288 18.7 -> 18.1 ms, 16384 34.2 -> 33.4
    static const int t2 = (int)tune("la_t2", 2048);
    for (int pos = 0; pos < n;) {
        starts.push_back(pos);
        const int rem = n - pos;
        int w = nb > 0 ? nb : (rem > t0 ? 2048 : (rem > t1 ? 1024 : (rem > t2 ? 512 : 256)));
        if (nb == 0 && !fused_cap) w = la_block(n);
        pos += std::min(w, rem);
    }
    starts.push_back(n);
    return starts;
}

PanelGeom panel_geometry(int rows, int w, int wprev, int k)
{
    PanelGeom pa{};
    pa.R = rows / LEAF; pa.W = w / LEAF;
    const int nbelow = pa.R - pa.W;
    // While the step is bound by the trailing update running beside the panel (not by the chain of
    // leaves), the kernel takes the diagonal block only -- W workgroups, the chain -- and the rows
    // below are solved by the grid-wide MFMA kernel afterwards: inside the persistent kernel a strip
    // below costs ~W (W + 3) / 2 products of 128^3, each on a CU of its own at 20 us alone and 2-3x
    // that beside a bandwidth-hungry update (a 1024-wide panel over 14336 rows: 3.1 - 5.7 ms).
    // Once the chain is what the step waits for, every strip gets its own workgroup: one launch, the
    // strips below finish ~20 us after the last leaf.
    const double m_u2 = (double)(rows + w);                    // order of the update running beside
    const double u2_us = k > 0 ? m_u2 * m_u2 * wprev / 55e6 : 0.0;
    static const double split_ratio = tune("panel_split_ratio", 3.0);
    pa.split = nbelow > 0 && k > 0 && u2_us > split_ratio * (125.0 * pa.W + 100.0);
    if (pa.split) {
        pa.R = pa.W;
        pa.G = pa.W;
    } else {
        // strips below per workgroup: as many as still finish under the update (each workgroup holds
        // a whole CU, 133 KiB of LDS, that the update loses); one each once the chain is the limit
        const double strip_us = 30.0 * (pa.W * (pa.W + 1) / 2 + pa.W), chain_us = 125.0 * pa.W;
        int per_wg = (int)((0.7 * u2_us - 0.5 * chain_us) / strip_us);
        per_wg = std::max(1, std::min(per_wg, 4));
        const int nwg = std::min((nbelow + per_wg - 1) / per_wg, PANEL_G_MAX - pa.W);
        pa.G = pa.W + (nbelow > 0 ? std::max(1, nwg) : 0);
    }
    // helpers for the tiles inside the diagonal block (tunable "panel_helpers", default on) and the early-hand-off
    // solve for every column of the strips below ("panel_below_early")
    static const bool helpers_on = tune("panel_helpers", 1) != 0, below_early_on = tune("panel_below_early", 1) != 0;
    pa.NH = helpers_on && pa.W > 2 ? (pa.W - 1) * (pa.W - 2) / 2 : 0;
    if (pa.G + pa.NH > PANEL_G_MAX) pa.NH = 0;
    pa.below_early = below_early_on ? 1 : 0;
    // one workgroup per tile of the rows below while they all fit the chip (the chain-bound sizes: a strip below is
    // W solves + W (W - 1) / 2 products of 20 - 30 us on ONE CU, 265 us for W = 4 against the chain's 215)
    static const bool tiles_on = tune("panel_tiles", 1) != 0;
    static const double tile_mult = tune("panel_tile_mult", 1.0);   // 1 / 2 / 3: n = 8192 6.94 / 7.06 / 7.12 ms, 12288 16.1 / 16.5 / 16.6
    if (tiles_on && !pa.split && nbelow > 0 && pa.W >= 2 && nbelow < PFLAG_STRIDE) {
        // workgroups for the tiles: all of them while the step waits for the chain anyway, else a multiple of the
        // strips' number (every one holds a CU that the update beside loses)
        const double chain_us = 60.0 * pa.W + 50.0;
        int nt = u2_us < chain_us ? nbelow * pa.W : (int)(tile_mult * (pa.G - pa.W));
        nt = std::max(1, std::min(std::min(nt, nbelow * pa.W), PANEL_G_MAX - pa.W - pa.NH));
        pa.tiles = 1;
        pa.G = pa.W + nt;
    }
    return pa;
}

bool chain_bound(int rest, int w, int w1)
{
    // Once the steps are bound by the chain panel -> U1 -> panel and no longer by U2, U2(k) starts only
    // when U1(k) has run: beside a freshly started U2 the short U1 waits for CUs and takes 2-3x longer.
    const double u2_us = (double)rest * rest * w / 55e6;
    return u2_us < 1.5 * (125.0 * (w1 / LEAF) + 100.0);
}

QueueGeom queue_geometry(const std::vector<int> &starts)
{
    QueueGeom q{};
    // workgroups of the widest panel kernel: its diagonal strips + the rows of the next diagonal block
    for (size_t k = 0; k + 1 < starts.size(); ++k)
        q.band = std::max(q.band, (starts[k + 1] - starts[k] + (k + 2 < starts.size() ? starts[k + 2] - starts[k + 1] : 0)) / LEAF);
    // helper workgroups for the tiles inside the diagonal blocks and extra ones for the rows of the next diagonal block tile
    // by tile (tunables "q_helpers", "q_tiles" = number of extra workgroups, 0 = strips as before)
    static const int q_helpers = (int)tune("q_helpers", 0), q_tiles = (int)tune("q_tiles", 0);   // measured at n = 16384: 29.6 ms without, 30.1 - 30.8 with (8 workers fewer)
    for (size_t k = 0; k + 1 < starts.size(); ++k) {
        const int W = (starts[k + 1] - starts[k]) / LEAF;
        if (q_helpers && W > 2) q.nh_max = std::max(q.nh_max, (W - 1) * (W - 2) / 2);
    }
    q.pgrid = q.band + q.nh_max + std::max(0, q_tiles);
    q.R = (q.pgrid + 7) / 8;
    q.helpers = q_helpers != 0;
    q.tiles = q_tiles > 0;
    return q;
}

namespace {
// The largest scratch over the products the recursion will issue (the same walk as potrf_rec / trsm_rec, sizes only): every
// call plans with thresholds of its own, so the largest product need not be the one with the largest need.  need_of(m, n, k,
// lower): the scratch of one product; cut: below this many rows or columns nothing qualifies.
template <typename F>
void need_trsm(int m, int n, long cut, F &need_of, size_t &need)
{
    if (n <= LEAF || std::min(m, n) < cut) return;
    const int n1 = split(n), n2 = n - n1;
    need_trsm(m, n1, cut, need_of, need);
    need = std::max(need, need_of(m, n2, n1, 0));
    need_trsm(m, n2, cut, need_of, need);
}
template <typename F>
void need_potrf(int n, int la_max, long cut, F &need_of, size_t &need)
{
    if (n <= LEAF || (n > 4 * LEAF && n <= la_max)) return;
    const int n1 = split(n), n2 = n - n1;
    need_potrf(n1, la_max, cut, need_of, need);
    need_trsm(n2, n1, cut, need_of, need);
    need = std::max(need, need_of(n2, n2, n1, 1));
    need_potrf(n2, la_max, cut, need_of, need);
}
}  // namespace

}  // namespace cplan

size_t potrf_strassen_top_need(int n)
{
    const StrassenRec v = strassen_rec_values();
    const StrassenTop t = strassen_top_values();
    size_t need = 0;
    auto need_of = [&](int m, int nn, int k, int lower) { return strassen_top_scratch_doubles(m, nn, k, lower, v, t); };
    if (v.on && t.smin3 > 0) cplan::need_potrf(n, cplan::walk_la_max(), 2 * t.smin3, need_of, need);    // halves of at least smin3
    return need;
}

void potrf_strassen_need(int n, size_t out[2])
{
    const StrassenRec v = strassen_rec_values();
    out[0] = out[1] = 0;
    for (int levels = 2; levels >= 1; --levels) {
        auto need_of = [&](int m, int nn, int k, int lower) { return strassen_scratch_doubles_cfg(m, nn, k, lower, levels, strassen_rec_cfg(v, k, lower)); };
        cplan::need_potrf(n, cplan::walk_la_max(), 256, need_of, out[2 - levels]);      // every threshold is at least 128 per half
    }
}

}  // namespace sgpr
