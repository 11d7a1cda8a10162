// strassen.h -- the Strassen front end of the fp64 NT product: record layouts, thresholds and entry points.
// strassen_plan.hip holds the planner (host C++ without a HIP header: which records, which thresholds, which schedule),
// strassen.hip the scratch, the executors and the two streaming kernels, streams.hip the side streams, chol_plan.hip the sizing walk.
// The part behind SGPR_HIP_TYPES needs common.h in front of it; the rest compiles with any C++17 compiler.
#pragma once
#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

#include "../../include/sympgpr_hip.h"

namespace sgpr {

void set_error(const std::string &msg);
double tune(const char *name, double dflt);

// ---- one level in front of gemm_nt -------------------------------------------------------------------------------
// P = A B^T with A = [A11 A12; A21 A22] (m halves x k halves), B likewise (n halves x k halves) needs 7 half-size
// products instead of 8:
//   M1 = (A11 + A22)(B11 + B22)^T -> C11, C22     M2 = (A21 + A22) B11^T -> C21, -C22    M3 = A11 (B21 - B22)^T -> C12, C22
//   M4 = A22 (B12 - B11)^T -> C11, C21            M5 = (A11 + A12) B22^T -> -C11, C12    M6 = (A21 - A11)(B11 + B21)^T -> C22
//   M7 = (A12 - A22)(B12 + B22)^T -> C11
// Every M is accumulated straight into its destination blocks by the two-destination kernel: no M temporaries, no
// block-accumulate passes; the ten operand sums go through two scratch blocks (one per side) reused product after product
// in stream order.  The whole decision -- which sums, which products, which destinations and signs, what stays classical --
// is host code that emits a list of records (strassen_plan); the device path executes exactly that list, and
// tests/test_strassen_plan_cpu.py replays it in numpy.  lower: the SYRK decomposition around it.
// Record = 16 words.  [0] = kind:
//   PLAN_SUM   [1] side (0: rows of A -> the A scratch, 1: rows of B -> the B scratch) [2] rows [3] cols
//              [4] xr [5] xc [6] yr [7] yc [8] sign         T = X + sign Y, X / Y the blocks at (row, k column) of that operand
//   PLAN_PROD  [1] a_src (0: block of A at ([2], [3]), 1: the A scratch) [4] b_src, ([5], [6]) likewise [7] m [8] n [9] k
//              [10] [11] first destination (row, column of C) [12] its sign [13] [14] [15] the second one (sign 0: none)
//   PLAN_CLASSIC  [1] lower [2] ar [3] ac [4] br [5] bc [6] m [7] n [8] k [9] cr [10] cc      the classical launch on a block
constexpr int STRASSEN_REC = 16;                 // words per plan record
enum { PLAN_SUM = 1, PLAN_PROD = 2, PLAN_CLASSIC = 3 };
int strassen_plan(int m, int n, int k, int lower, long smin, long kslab, size_t scratch_doubles, std::vector<long long> &out);

// ---- the outer level: one more level AROUND that list for the largest products -------------------------------------
// The same seven formulas on the halves; each outer product M_i = X Y^T (X, Y a raw block or an outer operand sum) is not a
// launch but a call of the inner level with a PAIR of destinations: the blocks of C that M_i goes to, each with its sign.  The
// inner plan of M_i is strassen_plan(m / 2, n / 2, kslab2 / 2) as it stands; run_plan turns its records into launches with
// twice the destinations (a product for two quadrants of M_i accumulates into four blocks of C).
// The outer list holds the inner level's records unchanged wherever the outer level does not apply (a call that does not
// qualify at all gives exactly strassen_plan's list), plus two kinds of its own with the layouts of PLAN_SUM / PLAN_PROD:
//   PLAN2_SUM   outer scratch of that side = X + sign Y
//   PLAN2_PROD  operands: raw block or the OUTER scratch; [7] [8] [9] the half-size extents; destinations as in PLAN_PROD
// k: whole slabs of exactly kslab2 columns take the outer level; a remainder shorter than that goes through the inner level.
enum { PLAN2_SUM = 4, PLAN2_PROD = 5 };
int strassen_outer_plan(int m, int n, int k, int lower, long smin, long kslab, long smin2, long kslab2, size_t scratch_doubles,
                   std::vector<long long> &out);
// The thresholds of ONE call of the front end; a negative member: the library's value (gemm_strassen_* / gemm_strassen2_*).
// smin_under: the inner threshold that holds under an outer product (negative: smin).
struct StrassenCfg { long smin = -1, kslab = -1, smin2 = -1, kslab2 = -1, smin_under = -1; };
// ... as the five words a record or a probe argument carries them in (smin, kslab, smin2, kslab2, smin_under)
template <typename T> void cfg_to_words(const StrassenCfg &c, T *w)
{
    w[0] = (T)c.smin; w[1] = (T)c.kslab; w[2] = (T)c.smin2; w[3] = (T)c.kslab2; w[4] = (T)c.smin_under;
}
template <typename T> StrassenCfg cfg_of_words(const T *w)
{
    StrassenCfg c;
    c.smin = (long)w[0]; c.kslab = (long)w[1]; c.smin2 = (long)w[2]; c.kslab2 = (long)w[3]; c.smin_under = (long)w[4];
    return c;
}
// the extents every plan entry refuses
inline bool bad_extents(int m, int n, int k, int lower) { return m < 0 || n < 0 || k < 0 || (lower && m != n); }
size_t strassen_scratch_doubles_cfg(int m, int n, int k, int lower, int levels, const StrassenCfg &cfg);
// The recursive factorisation's own values (potrf_rec / trsm_rec; tunables "rec_strassen_*"): inner and outer
// threshold for the products of trsm_rec and for the lower updates, and the outer k slab of a call whose k is shorter than
// the long outer slab (0: such a call takes no outer level); the inner and the long outer k slab are the library's unless
// tuned.  on = false (SGPR_GEMM_STRASSEN set): the library's values.
struct StrassenRec { bool on = false; long smin_gemm = 0, smin_syrk = 0, smin2_gemm = 0, smin2_syrk = 0, kslab = 0, kslab2 = 0, kslab2_short = 0; };
StrassenRec strassen_rec_values();
StrassenCfg strassen_rec_cfg(const StrassenRec &v, int k, int lower);
// the list of one call as the recursion would plan it; cfg_out (may be null): the thresholds it resolved to
int strassen_rec_plan(int m, int n, int k, int lower, long cfg_out[5], size_t scratch_doubles, std::vector<long long> &out);

// ---- the operand sums beside the products ---------------------------------------------------------------------------
// The sums are HBM streaming, the products MFMA-bound; a sum needs neither LDS nor more registers than two product waves per
// SIMD leave.  So a list can be executed with its sums on a low-priority side stream, each under the product before the one
// that needs it.  Again the decision is host code that emits records and the device path executes exactly those:
// schedule_of turns a list into a SCHEDULE -- the same records in the same order, the inner plan of every outer product expanded
// behind it, each record annotated (SCHED_REC words):
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
// The serial form (tunable "gemm_strassen_overlap" = 0) is the schedule with NO side stream: every record on stream 0, one
// buffer per region, so no wait crosses a stream and the executor records no event.
constexpr int SCHED_REC = 32;                    // words per schedule record: the plan record + its annotations
// the schedule of one call for a scratch buffer of cap_doubles (< 0: the call's need), side streams on
int strassen_schedule(int m, int n, int k, int lower, long long cap_doubles, long long info[12], std::vector<long long> &out);

// ---- a third level ON TOP of the front end, for the recursion's two largest products ---------------------------------
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
// its k offset.  A lower update splits around its off-diagonal square as the outer level does: lower(h), the square, lower(h).
enum { PLAN3_SUM = 6, PLAN3_ZERO = 7, PLAN3_PROD = 8, PLAN3_ACC = 9, PLAN3_PASS = 10 };
// Tunables "rec_strassen3_min" (half-size of m and n; 0: off), "rec_strassen3_kslab" / "rec_strassen3_kslab_short" (top k slab of
// a call whose k reaches the long one / of a shorter call; 0: none), read with the recursion's other values.
struct StrassenTop { long smin3 = 0, kslab3 = 0, kslab3_short = 0; };
StrassenTop strassen_top_values();
// (v / t null: the values as the next factorisation would read them)
int strassen_top_plan(int m, int n, int k, int lower, const StrassenRec *v, const StrassenTop *t, size_t scratch_doubles,
                      std::vector<long long> &out);
// the list of one call under explicit thresholds (what a PLAN3_PROD / PLAN3_PASS record's call turns into)
int strassen_cfg_plan(int m, int n, int k, int lower, const long cfg[5], std::vector<long long> &out);
size_t strassen_top_scratch_doubles(int m, int n, int k, int lower, const StrassenRec &v, const StrassenTop &t);

void potrf_strassen_need(int n, size_t out[2]);  // chol_plan.hip: what potrf() reserves at order n (both levels, one level)
size_t potrf_strassen_top_need(int n);           // chol_plan.hip: doubles of top-level scratch at order n (one buffer per region)

// ---- what the executors (strassen.hip) take from the planner (strassen_plan.hip)
namespace splan {
struct PlanCfg {
    long smin;      // smallest half-size of m and n that qualifies (half of k: smin / 2)
    long kslab;     // k is processed in slabs of at most this many columns (bounds the scratch)
    size_t scratch; // doubles of scratch available
};
struct Plan2Cfg {
    PlanCfg in;     // the inner level (its scratch member is not used here)
    long smin2;     // smallest half-size of m and n that takes the outer level
    long kslab2;    // its k slab: exactly this many columns, a multiple of 64 (quarters stay multiples of the k-step)
    size_t scratch; // doubles available for the inner and the outer pair together
    long smin_under = -1;   // the inner threshold UNDER an outer product (negative: in.smin); the recursion's calls set it
};
// doubles of scratch per region: inner A side, inner B side, outer A side, outer B side
struct Need2 { size_t v[4] = {0, 0, 0, 0}; size_t inner() const { return v[0] + v[1]; } size_t total() const { return v[0] + v[1] + v[2] + v[3]; } };
struct SchedCfg {
    int nbuf[4] = {1, 1, 1, 1};     // buffers per region
    size_t off[4][2] = {};          // their offsets in the scratch: the pinned layout first, second buffers behind it
    int nstreams = 1;               // side streams: 1, or 2 = one per operand side; 0 = the serial form
};
// doubles per region of the top scratch: T, the A side, the B side
struct Need3 { size_t v[3] = {0, 0, 0}; size_t total() const { return v[0] + v[1] + v[2]; } };

int strassen_levels();              // SGPR_GEMM_STRASSEN: 0 classical only, 1 one level, 2 (or unset) both
bool outer_noscratch();             // tunable "gemm_strassen2_noscratch", read once
Plan2Cfg cfg2_of(const StrassenCfg &cfg, size_t scratch_doubles);
PlanCfg under_of(const Plan2Cfg &c);
void outer_plan_of(int m, int n, int k, int lower, const Plan2Cfg &c, std::vector<long long> &out);
Need2 plan_need(const std::vector<long long> &plan, const Plan2Cfg &c);      // lists of kinds 1 - 5
SchedCfg sched_cfg_of(const Need2 &nd, size_t cap, bool overlap);
void schedule_of(const std::vector<long long> &plan, const Plan2Cfg &c, const Need2 &nd, const SchedCfg &sc, std::vector<long long> &out);
Need3 top_need(const std::vector<long long> &plan);
int top_buffers_wanted();
}  // namespace splan

#ifdef SGPR_HIP_TYPES
// ---- strassen.hip
int gemm_nt_strassen(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb, double beta,
                     double *C, size_t ldc, int lower, hipStream_t st);
int gemm_nt_strassen_cfg(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb, double beta,
                         double *C, size_t ldc, int lower, const StrassenCfg &cfg, hipStream_t st);
// one product as the recursion would issue it (its thresholds for this k and kind)
int gemm_nt_strassen_rec(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb, double beta,
                         double *C, size_t ldc, int lower, hipStream_t st);
// the recursion's entry (not named gemm_nt_strassen*: those are the front end's exported entries, csrc/exports.map)
int strassen_top_gemm(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb, double beta,
                      double *C, size_t ldc, int lower, const StrassenRec *v, const StrassenTop *t, hipStream_t st);
void strassen_reserve(size_t both, size_t one, hipStream_t st);
void strassen_top_reserve(size_t need, hipStream_t st);
int strassen_trim();                             // release the scratch of the operand sums and of the top level (every device)
// streams.hip: the library's low-priority streams on the device of `caller`, created on first use and released with the look-ahead
// driver's side stream -- for the operand sums (count = 1 or 2) and for the top level's passes
int strassen_sum_streams(hipStream_t caller, int count, hipStream_t *out);
int strassen_top_stream(hipStream_t caller, hipStream_t *out);
#endif

}  // namespace sgpr
