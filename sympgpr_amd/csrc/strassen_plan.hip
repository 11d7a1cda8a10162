// strassen_plan.hip -- the planner of the Strassen front end (strassen.h): which records, which thresholds, which schedule.
// Host C++ only: no HIP header, no HIP call; tune() and set_error() are all it takes from the library, so the file also compiles
// on its own (g++ -x c++ -std=c++17) for tests/test_strassen_plan_sanitized_cpu.py.  tests/test_strassen*_cpu.py replay its lists.
#include <cstdlib>
#include <initializer_list>

#include "strassen.h"

namespace sgpr {
using namespace splan;

namespace {
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
// (cr, cc); `kind_sum` / `kind_prod`: the inner level's records or another level's (PLAN2_*, PLAN3_*: same layout)
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
    if (!qualifies(m, n, k, c)) { put(out, {PLAN_CLASSIC, 0, ar, 0, br, 0, m, n, k, cr, cc}); return; }
    const long step = slab_of(k, c);
    for (long k0 = 0; k0 < k; k0 += step) seven(PLAN_SUM, PLAN_PROD, m / 2, n / 2, std::min(step, k - k0) / 2, k0, ar, br, cr, cc, out);
}
// lower update of the square block at row / column r0: while its off-diagonal square qualifies, the two diagonal halves
// recurse and the square goes through plan_gemm; then the triangular launch as before
void plan_syrk(long n, long k, long r0, const PlanCfg &c, std::vector<long long> &out)
{
    const long h = n / 2;
    if (n % 2 != 0 || !qualifies(h, h, k, c)) { put(out, {PLAN_CLASSIC, 1, r0, 0, r0, 0, n, n, k, r0, r0}); return; }
    plan_syrk(h, k, r0, c, out);
    plan_gemm(h, h, k, r0 + h, r0, r0 + h, r0, c, out);
    plan_syrk(h, k, r0 + h, c, out);
}
// Default threshold: profiles/strassen/sweep.txt.  Tunables "gemm_strassen_min" (half-size of m and n; k: half of it),
// "gemm_strassen_kslab", "gemm_strassen_noscratch" (tests: the scratch allocation is reported as failed; strassen.hip).
PlanCfg default_cfg()
{
    static const long smin = std::max(128L, (long)tune("gemm_strassen_min", 8192));
    static const long kslab = std::max(32L, (long)tune("gemm_strassen_kslab", 16384));
    return PlanCfg{smin, kslab, ~(size_t)0};
}
// the recursion's shipped values (strassen_rec_values / strassen_top_values below)
constexpr long REC_SMIN_GEMM = 4096, REC_SMIN_SYRK = 8192, REC_SMIN2_GEMM = 8192, REC_SMIN2_SYRK = 8192, REC_KSLAB2_SHORT = 16384;
constexpr long REC_SMIN3 = 16384, REC_KSLAB3 = 65536, REC_KSLAB3_SHORT = 32768;
// Default thresholds: profiles/strassen2/sweep.txt.  Tunables "gemm_strassen2_min", "gemm_strassen2_kslab",
// "gemm_strassen2_noscratch" (tests: the allocation of the outer part is reported as failed -> one level).
Plan2Cfg default_cfg2()
{
    static const long smin2 = std::max(256L, (long)tune("gemm_strassen2_min", 16384));
    static const long kslab2 = std::max(64L, (long)tune("gemm_strassen2_kslab", 32768));
    return Plan2Cfg{default_cfg(), smin2, kslab2, ~(size_t)0};
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
PlanCfg inner_of(const Plan2Cfg &c) { return PlanCfg{c.in.smin, c.in.kslab, c.scratch}; }
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
}  // namespace

// 0: classical only, 1: one level (bit for bit what the tree did before the outer level existed), 2: both at the library's
// thresholds everywhere (bit for bit the tree before the recursion had thresholds of its own); unset: both, and the recursive
// factorisation plans each of its products with its own thresholds (strassen_rec_values)
int splan::strassen_levels()
{
    static const int lv = [] { const char *e = getenv("SGPR_GEMM_STRASSEN"); return !e ? 2 : (e[0] == '0' ? 0 : (e[0] == '1' ? 1 : 2)); }();
    return lv;
}
bool splan::outer_noscratch()
{
    static const bool forced_fail = tune("gemm_strassen2_noscratch", 0) != 0;
    return forced_fail;
}
// the inner level as it holds under an outer product (its scratch member is the caller's business)
PlanCfg splan::under_of(const Plan2Cfg &c) { return PlanCfg{c.smin_under >= 0 ? c.smin_under : c.in.smin, c.in.kslab, c.in.scratch}; }
Plan2Cfg splan::cfg2_of(const StrassenCfg &cfg, size_t scratch_doubles)
{
    Plan2Cfg c = default_cfg2();
    if (cfg.smin >= 0) c.in.smin = std::max(128L, cfg.smin);
    if (cfg.kslab >= 0) c.in.kslab = std::max(32L, cfg.kslab);
    if (cfg.smin2 >= 0) c.smin2 = std::max(256L, cfg.smin2);
    if (cfg.kslab2 >= 0) c.kslab2 = std::max(64L, cfg.kslab2);
    if (cfg.smin_under >= 0) c.smin_under = std::max(128L, cfg.smin_under);
    c.scratch = scratch_doubles;
    return c;
}
void splan::outer_plan_of(int m, int n, int k, int lower, const Plan2Cfg &c, std::vector<long long> &out)
{
    out.clear();
    if (lower) plan2_syrk(n, k, 0, c, out);
    else       plan2_gemm(m, n, k, 0, 0, 0, 0, c, out);
}
// scratch of a list of the inner level, the outer level or both (an inner-only list: its two regions, the layout is [A | B]
// either way); the inner plans of the outer products count with the threshold that holds under them
Need2 splan::plan_need(const std::vector<long long> &plan, const Plan2Cfg &c)
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

// Second buffers come out of the SLACK of the scratch (capacity - the call's need, capped by the tunable
// "gemm_strassen_overlap_slack": < 0 all of it, 0 none), in the order inner A, inner B, outer A, outer B while it lasts.
// Tunable "gemm_strassen_overlap_streams": 2 = the sums of the B side on a side stream of their own.
// overlap = false: the serial form -- no side stream, one buffer per region in the pinned layout.
SchedCfg splan::sched_cfg_of(const Need2 &nd, size_t cap, bool overlap)
{
    SchedCfg sc;
    size_t pos = 0;
    for (int r = 0; r < 4; ++r) { sc.off[r][0] = pos; pos += nd.v[r]; }
    sc.nstreams = !overlap ? 0 : (tune("gemm_strassen_overlap_streams", 1) >= 2 ? 2 : 1);
    if (!overlap) return sc;
    const double lim = tune("gemm_strassen_overlap_slack", -1);
    size_t slack = cap > nd.total() ? cap - nd.total() : 0;
    if (lim >= 0) slack = std::min(slack, (size_t)lim);
    for (int r = 0; r < 4; ++r) {
        if (!nd.v[r]) continue;
        if (nd.v[r] > slack) break;
        sc.nbuf[r] = 2; sc.off[r][1] = pos; pos += nd.v[r]; slack -= nd.v[r];
    }
    return sc;
}
void splan::schedule_of(const std::vector<long long> &plan, const Plan2Cfg &c, const Need2 &nd, const SchedCfg &sc, std::vector<long long> &out)
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
        const int stream = sc.nstreams == 2 ? 1 + (int)r[1] : std::min(sc.nstreams, 1), b = next[rg];
        next[rg] = (b + 1) % sc.nbuf[rg];
        Buf &t = buf[rg][b];
        wait(at, t.prod_reader); wait(at, t.sum_reader[0]); wait(at, t.sum_reader[1]);
        if (!out[at + 20]) wait(at, t.writer);
        if (src >= 0) { wait(at, buf[src][sb].writer); buf[src][sb].sum_reader[std::max(stream - 1, 0)] = idx; }
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

// the plan of one call as the host decides it (no device): smin / kslab < 0 = the built-in values or tunables
int strassen_plan(int m, int n, int k, int lower, long smin, long kslab, size_t scratch_doubles, std::vector<long long> &out)
{
    if (bad_extents(m, n, k, lower)) { set_error("strassen_plan: bad extents"); return SGPR_E_ARG; }
    PlanCfg c = default_cfg();
    if (smin >= 0) c.smin = std::max(128L, smin);
    if (kslab >= 0) c.kslab = std::max(32L, kslab);
    c.scratch = scratch_doubles;
    out.clear();
    if (lower) plan_syrk(n, k, 0, c, out);
    else       plan_gemm(m, n, k, 0, 0, 0, 0, c, out);
    return 0;
}
// ... and the list with the outer level around it (smin2 / kslab2 < 0 = the built-in values or tunables)
int strassen_outer_plan(int m, int n, int k, int lower, long smin, long kslab, long smin2, long kslab2, size_t scratch_doubles,
                   std::vector<long long> &out)
{
    if (bad_extents(m, n, k, lower)) { set_error("strassen_outer_plan: bad extents"); return SGPR_E_ARG; }
    outer_plan_of(m, n, k, lower, cfg2_of(StrassenCfg{smin, kslab, smin2, kslab2, -1}, scratch_doubles), out);
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
    if (bad_extents(m, n, k, lower)) { set_error("strassen_rec_plan: bad extents"); return SGPR_E_ARG; }
    const Plan2Cfg c = cfg2_of(strassen_rec_cfg(strassen_rec_values(), k, lower), scratch_doubles);
    if (cfg_out) cfg_to_words(StrassenCfg{c.in.smin, c.in.kslab, c.smin2, c.kslab2, under_of(c).smin}, cfg_out);
    outer_plan_of(m, n, k, lower, c, out);
    return 0;
}

// The schedule of that call (schedule_of) for a scratch buffer of cap_doubles: the list as gemm_nt_strassen_cfg plans it with
// the scratch it needs (both levels, as far as SGPR_GEMM_STRASSEN allows).  info: [0 .. 3] doubles per region (inner A, inner B,
// outer A, outer B), [4 .. 7] buffers per region, [8] side streams, [9] the capacity.  A capacity below the need is an error.
int strassen_schedule(int m, int n, int k, int lower, long long cap_doubles, long long info[12], std::vector<long long> &out)
{
    if (bad_extents(m, n, k, lower)) { set_error("strassen_schedule: bad extents"); return SGPR_E_ARG; }
    const Plan2Cfg c = cfg2_of(strassen_rec_cfg(strassen_rec_values(), k, lower), ~(size_t)0);
    std::vector<long long> plan;
    if (strassen_levels() >= 2 && !outer_noscratch()) outer_plan_of(m, n, k, lower, c, plan);
    else {
        const int rc = strassen_plan(m, n, k, lower, c.in.smin, c.in.kslab, ~(size_t)0, plan);
        if (rc) return rc;
    }
    const Need2 nd = plan_need(plan, c);
    const size_t cap = cap_doubles < 0 ? nd.total() : (size_t)cap_doubles;
    if (cap < nd.total()) { set_error("strassen_schedule: the capacity is below the call's need"); return SGPR_E_ARG; }
    const SchedCfg sc = sched_cfg_of(nd, cap, true);
    schedule_of(plan, c, nd, sc, out);
    if (info) {
        for (int i = 0; i < 12; ++i) info[i] = 0;
        for (int r = 0; r < 4; ++r) { info[r] = (long long)nd.v[r]; info[4 + r] = sc.nbuf[r]; }
        info[8] = sc.nstreams; info[9] = (long long)cap;
    }
    return 0;
}

// scratch of one call: levels = 1 the inner pair alone, 2 both pairs (as far as SGPR_GEMM_STRASSEN allows)
size_t strassen_scratch_doubles_cfg(int m, int n, int k, int lower, int levels, const StrassenCfg &cfg)
{
    std::vector<long long> plan;
    if (!strassen_levels() || bad_extents(m, n, k, lower)) return 0;
    const Plan2Cfg c2 = cfg2_of(cfg, ~(size_t)0);
    if (levels >= 2 && strassen_levels() >= 2) outer_plan_of(m, n, k, lower, c2, plan);
    else if (strassen_plan(m, n, k, lower, c2.in.smin, c2.in.kslab, ~(size_t)0, plan)) return 0;
    return plan_need(plan, c2).total();
}

// ---- the top level (strassen.h: kinds 6 - 10)
namespace {
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
// the thresholds of a call into words [at, at + 5) of the record just emitted
void put_cfg(std::vector<long long> &out, int at, const StrassenCfg &c) { cfg_to_words(c, &out[out.size() - STRASSEN_REC + at]); }
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
}  // namespace

Need3 splan::top_need(const std::vector<long long> &plan)
{
    Need3 nd;
    for (size_t i = 0; i + STRASSEN_REC <= plan.size(); i += STRASSEN_REC) {
        const long long *r = &plan[i];
        if (r[0] == PLAN3_ZERO) nd.v[0] = std::max(nd.v[0], (size_t)r[1] * (size_t)r[2]);
        else if (r[0] == PLAN3_SUM) nd.v[1 + r[1]] = std::max(nd.v[1 + r[1]], (size_t)r[2] * (size_t)r[3]);
    }
    return nd;
}
// tunable "rec_strassen3_buffers": 2 (built in) = a second [T | A | B] set, so that the passes of one top product run under the
// next; "rec_strassen3_overlap" = 0: all passes on the caller's stream in list order (and one set)
int splan::top_buffers_wanted() { return (tune("rec_strassen3_overlap", 1) != 0 && tune("rec_strassen3_buffers", 2) >= 2) ? 2 : 1; }

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
    if (bad_extents(m, n, k, lower)) { set_error("strassen_top_plan: bad extents"); return SGPR_E_ARG; }
    out.clear();
    if (lower) top_syrk(n, k, v, t, scratch_doubles, out);
    else       top_gemm(m, n, k, 0, 0, 0, 0, 0, v, t, scratch_doubles, out);
    return 0;
}
int strassen_cfg_plan(int m, int n, int k, int lower, const long cfg[5], std::vector<long long> &out)
{
    if (bad_extents(m, n, k, lower) || !cfg) { set_error("strassen_cfg_plan: bad arguments"); return SGPR_E_ARG; }
    outer_plan_of(m, n, k, lower, cfg2_of(cfg_of_words(cfg), ~(size_t)0), out);
    return 0;
}
size_t strassen_top_scratch_doubles(int m, int n, int k, int lower, const StrassenRec &v, const StrassenTop &t)
{
    std::vector<long long> plan;
    if (strassen_levels() < 2 || strassen_top_plan(m, n, k, lower, &v, &t, ~(size_t)0, plan)) return 0;
    return top_need(plan).total();
}

}  // namespace sgpr
