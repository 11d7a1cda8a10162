// The stand-alone program of tests/test_strassen_plan_sanitized_cpu.py: sympgpr_amd/csrc/strassen_plan.hip compiled as plain C++
// next to this file, with the two functions it takes from the library defined here.  Walks the scaled-down grid of
// tools/strassen_lists.py through every plan, need and schedule entry and prints, per entry, the number of lists, of records and
// the sum of all their words (needs: the sum of the doubles).
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../sympgpr_amd/csrc/strassen.h"

static std::map<std::string, double> g_tune = {
    {"rec_strassen_min_gemm", 128}, {"rec_strassen_min_syrk", 128}, {"rec_strassen2_min_gemm", 256}, {"rec_strassen2_min_syrk", 256},
    {"rec_strassen2_kslab_short", 512}, {"rec_strassen_kslab", 512}, {"rec_strassen2_kslab", 1024},
    {"rec_strassen3_min", 512}, {"rec_strassen3_kslab", 2048}, {"rec_strassen3_kslab_short", 1024}};
static int g_errors = 0;

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

struct Tally { long long lists = 0, records = 0, words = 0; };
static void count(Tally &t, const std::vector<long long> &v, int rec)
{
    ++t.lists;
    t.records += (long long)(v.size() / rec);
    for (long long w : v) t.words += w;
}

int main()
{
    using namespace sgpr;
    const int MN[] = {256, 512, 768, 1024, 1536, 2048, 3072, 4096}, K[] = {64, 256, 512, 544, 1024, 1536, 2048, 2560, 4096};
    const size_t unlimited = (size_t)1 << 62;
    const long cfg5[5] = {128, 512, 256, 1024, 128};
    Tally rec, top, sched, plan1, plan2, cfgp, need2, need3;
    std::vector<long long> out;
    int rc = 0;
    for (int lower = 0; lower < 2; ++lower)
        for (int m : MN)
            for (int n : MN) {
                if (lower && n != m) continue;
                for (int k : K) {
                    for (size_t cap : {unlimited, (size_t)(m / 2 + n / 2) * 256}) {
                        long resolved[5];
                        rc |= strassen_rec_plan(m, n, k, lower, resolved, cap, out);
                        count(rec, out, STRASSEN_REC);
                        for (long w : resolved) rec.words += w;
                        rc |= strassen_top_plan(m, n, k, lower, nullptr, nullptr, cap, out);
                        count(top, out, STRASSEN_REC);
                        rc |= strassen_plan(m, n, k, lower, 128, 512, cap, out);
                        count(plan1, out, STRASSEN_REC);
                        rc |= strassen_outer_plan(m, n, k, lower, 128, 512, 256, 1024, cap, out);
                        count(plan2, out, STRASSEN_REC);
                    }
                    rc |= strassen_cfg_plan(m, n, k, lower, cfg5, out);
                    count(cfgp, out, STRASSEN_REC);
                    long long info[12];
                    rc |= strassen_schedule(m, n, k, lower, -1, info, out);
                    count(sched, out, SCHED_REC);
                    const long long need = info[0] + info[1] + info[2] + info[3];
                    rc |= strassen_schedule(m, n, k, lower, 4 * need, info, out);
                    count(sched, out, SCHED_REC);
                    for (int i = 0; i < 12; ++i) sched.words += info[i];
                    const StrassenRec v = strassen_rec_values();
                    ++need2.lists;
                    need2.words += (long long)strassen_scratch_doubles_cfg(m, n, k, lower, 2, strassen_rec_cfg(v, k, lower));
                    ++need3.lists;
                    need3.words += (long long)strassen_top_scratch_doubles(m, n, k, lower, v, strassen_top_values());
                }
            }
    // what the entries refuse
    if (strassen_plan(-1, 8, 8, 0, -1, -1, 0, out) != SGPR_E_ARG || strassen_schedule(512, 256, 64, 1, -1, nullptr, out) != SGPR_E_ARG ||
        strassen_cfg_plan(512, 512, 64, 0, nullptr, out) != SGPR_E_ARG || strassen_schedule(4096, 4096, 2048, 0, 1, nullptr, out) != SGPR_E_ARG)
        rc |= 64;
    const struct { const char *name; const Tally &t; } rows[] = {{"rec_plan", rec}, {"top_plan", top}, {"schedule", sched}, {"plan", plan1},
                                                                 {"plan2", plan2}, {"cfg_plan", cfgp}, {"need2", need2}, {"need3", need3}};
    for (const auto &r : rows) std::printf("%s %lld %lld %lld\n", r.name, r.t.lists, r.t.records, r.t.words);
    return (rc || g_errors != 4) ? 1 : 0;
}
