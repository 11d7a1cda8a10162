// The stand-alone program of tests/test_chol_plan_cpu.py: sympgpr_amd/csrc/chol_plan.hip (and the Strassen planner its sizing
// walk calls, strassen_plan.hip) compiled as plain C++ next to this file, with the two functions they take from the library
// defined here.  Walks the look-ahead driver's decisions -- block schedule, every panel's geometry, the chain_bound switch -- for
// the orders below, the queue driver's panel grid over its window of orders, the workspace layout and the sizing walk, checks
// the invariants that follow from the panel kernel's own limits (panel.h) and prints everything as one JSON document.
// argv[1] (optional): the value of the tunable "la_max".  Status 0: every invariant held.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../sympgpr_amd/csrc/strassen.h"
#include "../sympgpr_amd/csrc/panel.h"
#include "../sympgpr_amd/csrc/chol_plan.h"

static std::map<std::string, double> g_tune;
static int g_errors = 0, g_bad = 0;

namespace sgpr {
double tune(const char *name, double dflt)
{
    const auto it = g_tune.find(name);
    return it == g_tune.end() ? dflt : it->second;
}
void set_error(const std::string &msg)
{
    ++g_errors;
    std::fprintf(stderr, "error: %s\n", msg.c_str());
}
}  // namespace sgpr

using namespace sgpr;

#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++g_bad;                                                       \
            std::fprintf(stderr, "violated: %s  [", #cond);                \
            std::fprintf(stderr, __VA_ARGS__);                             \
            std::fprintf(stderr, "]\n");                                   \
        }                                                                  \
    } while (0)

// one block as potrf_lookahead walks it: the schedule, then per panel what the driver would launch
static void block(int n, int nb, bool fused, bool first)
{
    const int LEAF = cplan::LEAF_ORDER;
    const bool fused_cap = fused && n % LEAF == 0;
    const std::vector<int> starts = cplan::la_starts(n, nb, fused_cap);
    const int nblk = (int)starts.size() - 1;
    CHECK(nblk >= 1 && starts[0] == 0 && starts.back() == n, "n=%d nb=%d", n, nb);
    int wmax = 0;
    for (int k = 0; k < nblk; ++k) {
        const int w = starts[k + 1] - starts[k];
        CHECK(w > 0, "n=%d nb=%d k=%d", n, nb, k);
        if (k + 1 < nblk) CHECK(w == 256 || w == 512 || w == 1024 || w == 2048 || w == nb, "n=%d nb=%d k=%d w=%d", n, nb, k, w);
        wmax = w > wmax ? w : wmax;
    }
    const bool fused_ok = fused_cap && wmax % LEAF == 0 && wmax / LEAF <= PW_MAX;
    std::printf("%s\n  {\"n\": %d, \"nb\": %d, \"fused\": %d, \"starts\": [", first ? "" : ",", n, nb, fused_ok ? 1 : 0);
    for (int k = 0; k <= nblk; ++k) std::printf("%s%d", k ? ", " : "", starts[k]);
    std::printf("],\n   \"chain_bound\": [");
    for (int k = 0; k + 1 < nblk; ++k) {
        const int w = starts[k + 1] - starts[k], w1 = starts[k + 2] - starts[k + 1];
        std::printf("%s%d", k ? ", " : "", cplan::chain_bound(n - starts[k + 2], w, w1) ? 1 : 0);
    }
    // per panel: R, W, G, NH, below_early, tiles, split, the launcher's grid
    std::printf("],\n   \"panels\": [");
    for (int k = 0; fused_ok && k < nblk; ++k) {
        const int k0 = starts[k], w = starts[k + 1] - k0, rows = n - k0;
        const cplan::PanelGeom g = cplan::panel_geometry(rows, w, k > 0 ? starts[k] - starts[k - 1] : 0, k);
        const int nbelow = rows / LEAF - w / LEAF, grid = panel_grid(g.G, g.NH, g.W);
        CHECK(g.W == w / LEAF && g.W >= 1 && g.W <= PW_MAX, "n=%d k=%d W=%d", n, k, g.W);
        CHECK(g.R >= g.W && g.R <= rows / LEAF && g.G >= g.W, "n=%d k=%d R=%d G=%d", n, k, g.R, g.G);
        CHECK(g.NH >= 0 && g.G + g.NH <= PANEL_G_MAX, "n=%d k=%d G=%d NH=%d", n, k, g.G, g.NH);
        CHECK(!g.tiles || (g.W >= 2 && nbelow < PFLAG_STRIDE && !g.split), "n=%d k=%d W=%d nbelow=%d", n, k, g.W, nbelow);
        CHECK(!g.split || (g.G == g.W && g.R == g.W), "n=%d k=%d", n, k);
        CHECK(g.split || g.R == rows / LEAF, "n=%d k=%d R=%d", n, k, g.R);
        CHECK(nbelow == 0 || g.split || g.G > g.W, "n=%d k=%d: rows below without a workgroup", n, k);
        CHECK(grid >= 8 * (g.W - 1) + 1 && grid >= g.G + g.NH, "n=%d k=%d grid=%d", n, k, grid);
        std::printf("%s[%d, %d, %d, %d, %d, %d, %d, %d]", k ? ", " : "", g.R, g.W, g.G, g.NH, g.below_early, g.tiles, g.split ? 1 : 0, grid);
    }
    std::printf("]}");
}

// the look-ahead blocks of a factorisation of order n, as potrf_rec reaches them
static void rec_blocks(int n, int la_max, std::map<int, int> &blocks)
{
    if (n <= cplan::LEAF_ORDER) return;
    if (n > 4 * cplan::LEAF_ORDER && n <= la_max) { ++blocks[n]; return; }
    const int n1 = cplan::split(n);
    CHECK(n1 >= cplan::LEAF_ORDER && n1 < n && n1 % cplan::LEAF_ORDER == 0, "split(%d) = %d", n, n1);
    rec_blocks(n1, la_max, blocks);
    rec_blocks(n - n1, la_max, blocks);
}

static void layout_checks(int n, size_t q)
{
    const cplan::WorkLayout w = cplan::work_layout(n, q);
    if (n <= 0) { CHECK(w.total == 256, "n=%d", n); return; }
    const size_t leaves = (size_t)((n + 127) / 128);
    CHECK(w.inv == 0 && w.flags == leaves * 128 * 128 * 8, "n=%d", n);
    CHECK(w.flags % 256 == 0 && w.flag_bytes % 256 == 0 && w.pub % 256 == 0 && w.queue % 256 == 0, "n=%d", n);
    CHECK(w.flag_bytes >= leaves * PFLAG_STRIDE * 4 && w.pub == w.flags + w.flag_bytes, "n=%d", n);
    CHECK(w.queue >= w.pub + (size_t)2 * n * 8 && w.queue < w.pub + (size_t)2 * n * 8 + 256, "n=%d", n);
    CHECK(w.total == w.queue + q + 256, "n=%d", n);
}

int main(int argc, char **argv)
{
    if (argc > 1) g_tune["la_max"] = std::atof(argv[1]);
    const bool dflt = argc <= 1;
    const int la_max = cplan::la_max_value();
    CHECK(la_max == (dflt ? 57344 : std::atoi(argv[1])), "la_max=%d", la_max);
    const int ORDERS[] = {256, 384, 1000, 2048, 4096, 8192, 12288, 16384, 24576, 32768, 57344}, REC[] = {4096, 65536, 131072};
    std::printf("{\"la_max\": %d,\n \"blocks\": [", la_max);
    bool first = true;
    if (dflt)
        for (int n : ORDERS)
            for (int nb : {0, 256})
                for (int fused = 1; fused >= 0; --fused) { block(n, nb, fused != 0, first); first = false; }
    // what the recursion hands to the look-ahead driver at these orders (nb = 0, the panel kernel usable)
    std::printf("],\n \"recursion\": [");
    std::set<int> seen;
    std::string rec_json;
    for (int n : REC) {
        std::map<int, int> blocks;
        rec_blocks(n, la_max, blocks);
        CHECK(!blocks.empty(), "n=%d", n);
        rec_json += (rec_json.empty() ? "" : ", ") + ("{\"n\": " + std::to_string(n) + ", \"blocks\": {");
        bool f = true;
        for (const auto &b : blocks) {
            rec_json += std::string(f ? "" : ", ") + "\"" + std::to_string(b.first) + "\": " + std::to_string(b.second);
            f = false;
            seen.insert(b.first);
        }
        rec_json += "}}";
    }
    first = true;
    for (int n : seen) { block(n, 0, true, first); first = false; }
    std::printf("],\n \"recursion_blocks\": [%s],\n", rec_json.c_str());
    // the queue driver's panel grid: its default window of orders (SGPR_Q_MIN .. SGPR_Q_MAX, multiples of 256), uniform panels
    // of the default width ("q_w" = 512): wherever cholq::eligible says yes the driver must find R <= 4
    std::printf(" \"queue\": [");
    for (int n = 13312; n <= 28672; n += 256) {
        std::vector<int> s;
        for (int pos = 0; pos < n; pos += 512) s.push_back(pos);
        s.push_back(n);
        const cplan::QueueGeom q = cplan::queue_geometry(s);
        CHECK(q.R >= 1 && q.R <= 4 && q.pgrid <= 8 * q.R && q.band >= 4 && q.pgrid >= q.band + q.nh_max, "n=%d R=%d pgrid=%d", n, q.R, q.pgrid);
        if (n % 4096 == 0) std::printf("%s[%d, %d, %d, %d, %d]", n == 16384 ? "" : ", ", n, q.band, q.nh_max, q.pgrid, q.R);
    }
    // the workspace layout (queue part 0 bytes and some), and what potrf() reserves for the Strassen front end
    std::printf("],\n \"layout\": [");
    first = true;
    for (int n : {-1, 0, 1, 127, 128, 129, 256, 384, 1000, 2048, 4096, 8192, 12288, 16384, 24576, 32768, 57344, 65536, 131072}) {
        for (size_t q : {(size_t)0, (size_t)256, (size_t)123456 * 256}) layout_checks(n, q);
        const cplan::WorkLayout w = cplan::work_layout(n, 0);
        std::printf("%s[%d, %zu, %zu, %zu, %zu, %zu]", first ? "" : ", ", n, w.flags, w.flag_bytes, w.pub, w.queue, w.total);
        first = false;
    }
    std::printf("],\n \"need\": [");
    first = true;
    for (int n : {256, 384, 1000, 2048, 4096, 8192, 12288, 16384, 24576, 32768, 57344, 65536, 131072}) {
        size_t need[2];
        potrf_strassen_need(n, need);
        std::printf("%s[%d, %zu, %zu, %zu]", first ? "" : ", ", n, need[0], need[1], potrf_strassen_top_need(n));
        first = false;
    }
    std::printf("]}\n");
    return (g_bad || g_errors) ? 1 : 0;
}
