// strassen.hip -- the device side of the Strassen front end (strassen.h): the two streaming kernels, the scratch of the operand
// sums, the executors of the lists strassen_plan.hip emits, and the entry points.  Every product is a launch of gemm_f64.hip.
#include <algorithm>
#include <cstdint>
#include <mutex>
#include <vector>

#include "common.h"
#include "gemm_tile.h"
#include "strassen.h"

namespace sgpr {
using namespace splan;

namespace {
using namespace tile;

// T (rows x cols, leading dimension rows) = X + sign Y on column-major blocks: the operand sums of the Strassen front end.
// HBM-bound (two reads, one write per element): 16-byte accesses, 4 columns per thread in flight, grid-stride over
// pieces of 512 rows x 4 columns.  rows even, all three bases 16-byte aligned, ldx / ldy even (checked by the caller).
__global__ __launch_bounds__(256) void block_sum_kernel(int rows, int cols, const double *X, size_t ldx, const double *Y, size_t ldy,
                                                        double sign, double *T)
{
    const int nrc = (rows + 511) / 512, ncg = (cols + 3) / 4;
    const long pieces = (long)nrc * ncg;
    for (long p = blockIdx.x; p < pieces; p += gridDim.x) {
        const int cg = (int)(p / nrc), rc = (int)(p - (long)cg * nrc);
        const int r = rc * 512 + 2 * (int)threadIdx.x;
        if (r >= rows) continue;
        double2_t x[4], y[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = min(cg * 4 + u, cols - 1);
            x[u] = *reinterpret_cast<const double2_t *>(X + (size_t)r + (size_t)c * ldx);
            y[u] = *reinterpret_cast<const double2_t *>(Y + (size_t)r + (size_t)c * ldy);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = cg * 4 + u;
            if (c < cols) *reinterpret_cast<double2_t *>(T + (size_t)r + (size_t)c * (size_t)rows) = x[u] + sign * y[u];
        }
    }
}

// C1 += a1 T and, where C2 is given, C2 += a2 T: T (rows x cols, leading dimension rows) is read once.  The pattern of
// block_sum_kernel: 16-byte accesses, 4 columns per thread in flight, grid-stride over pieces of 512 rows x 4 columns; rows even,
// all bases 16-byte aligned, ldc even (checked by the caller).  A kernel of its own behind the others: they compile as without it.
__global__ __launch_bounds__(256) void block_acc_kernel(int rows, int cols, const double *T, double *C1, double a1, double *C2, double a2,
                                                        size_t ldc)
{
    const int nrc = (rows + 511) / 512, ncg = (cols + 3) / 4;
    const long pieces = (long)nrc * ncg;
    for (long p = blockIdx.x; p < pieces; p += gridDim.x) {
        const int cg = (int)(p / nrc), rc = (int)(p - (long)cg * nrc);
        const int r = rc * 512 + 2 * (int)threadIdx.x;
        if (r >= rows) continue;
        double2_t t[4], c1[4], c2[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = min(cg * 4 + u, cols - 1);
            t[u] = *reinterpret_cast<const double2_t *>(T + (size_t)r + (size_t)c * (size_t)rows);
            c1[u] = *reinterpret_cast<const double2_t *>(C1 + (size_t)r + (size_t)c * ldc);
            if (C2) c2[u] = *reinterpret_cast<const double2_t *>(C2 + (size_t)r + (size_t)c * ldc);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = cg * 4 + u;
            if (c >= cols) continue;
            *reinterpret_cast<double2_t *>(C1 + (size_t)r + (size_t)c * ldc) = c1[u] + a1 * t[u];
            if (C2) *reinterpret_cast<double2_t *>(C2 + (size_t)r + (size_t)c * ldc) = c2[u] + a2 * t[u];
        }
    }
}

constexpr long SUM_WGS = 2048;     // most workgroups of one pass on the caller's stream (the kernels stride over their pieces)
// Workgroups of a side-stream pass: one per CU, so that ONE sum wave (40 registers) sits beside the two product waves of a SIMD,
// which leave 64 or 48 of 512; a second one (80) would keep the next product workgroup off that CU until the sums have drained.
// Measured in the step (sweep.txt): 256 -1.8 %, 512 and 2048 (one launch's grid on the caller's stream) 0 ... -0.6 %.
// Tunable "gemm_strassen_sum_wgs": most workgroups of a side-stream pass.
constexpr long SUM_WGS_SIDE = 256;
long side_wgs() { return std::min(65535L, std::max(1L, (long)tune("gemm_strassen_sum_wgs", (double)SUM_WGS_SIDE))); }

int block_sum(int rows, int cols, const double *X, size_t ldx, const double *Y, size_t ldy, double sign, double *T, hipStream_t st, long wgs)
{
    const long pieces = (long)((rows + 511) / 512) * ((cols + 3) / 4);
    hipLaunchKernelGGL(block_sum_kernel, dim3((unsigned)std::min(pieces, wgs)), dim3(256), 0, st, rows, cols, X, ldx, Y, ldy, sign, T);
    SGPR_CHECK_LAUNCH();
    return 0;
}
int block_acc(int rows, int cols, const double *T, double *C1, double a1, double *C2, double a2, size_t ldc, hipStream_t st, long wgs)
{
    const long pieces = (long)((rows + 511) / 512) * ((cols + 3) / 4);
    hipLaunchKernelGGL(block_acc_kernel, dim3((unsigned)std::min(pieces, wgs)), dim3(256), 0, st, rows, cols, T, C1, a1, C2, a2, ldc);
    SGPR_CHECK_LAUNCH();
    return 0;
}

// ---- one decoder per record shape (layouts: strassen.h)
struct Mat { const double *p; size_t ld; };     // a column-major operand: A, B, or a block or a scratch image of either
// the block of an operand at (row, column)
template <typename T> T *block(T *P, size_t ld, long long row, long long col) { return P + row + (size_t)col * ld; }
// launch the sum a SUM-layout record (PLAN_SUM, PLAN2_SUM, PLAN3_SUM) describes into T
int sum_into(const long long *r, Mat A, Mat B, double *T, hipStream_t st, long wgs)
{
    const Mat P = r[1] ? B : A;
    return block_sum((int)r[2], (int)r[3], block(P.p, P.ld, r[4], r[5]), P.ld, block(P.p, P.ld, r[6], r[7]), P.ld, (double)r[8], T, st, wgs);
}
// the operand on side `side` of a PROD-layout record (PLAN_PROD, PLAN2_PROD, PLAN3_PROD): a raw block, or that side's scratch S
Mat operand_of(const long long *r, int side, Mat P, const double *S)
{
    const long long *o = r + 1 + 3 * side;      // [src, row, k column]
    return o[0] ? Mat{S, (size_t)r[7 + side]} : Mat{block(P.p, P.ld, o[1], o[2]), P.ld};
}
// the destination pair of a record, d = its six words [row, column, sign] x 2 (PLAN*_PROD: r + 10, PLAN3_ACC: r + 3)
struct Dests { double *C1; double a1; double *C2; double a2; };       // C2 null: one destination
Dests dests_of(const long long *d, double alpha, double *C, size_t ldc)
{
    return Dests{block(C, ldc, d[0], d[1]), alpha * (double)d[2], d[5] ? block(C, ldc, d[3], d[4]) : nullptr, alpha * (double)d[5]};
}

// ---- the scratch.  One owner per (level, device): [0] the operand sums of the two lower levels, laid out by the schedule;
// [1] the top level's [T | A side | B side] sets.  Owned by the library, grown to the largest qualifying call and released by
// strassen_trim().  Calls are serialised by the mutex while they ENQUEUE; on the device a call on another stream first waits
// for the event the previous user recorded behind its last launch (Use).  The top level holds its mutex while its half-size
// calls take the lower one, never the other way round.
struct Scratch {
    std::mutex mu;
    double *p = nullptr;
    size_t cap = 0, failed = 0;     // doubles; smallest request that could not be allocated (0: none)
    hipEvent_t ev = nullptr;        // behind the last call that used the buffer
    hipStream_t last = nullptr;
    bool used = false;
    std::vector<hipEvent_t> pool;   // events of the overlapped execution, timing disabled, created on demand
    int event(size_t i)
    {
        if (pool.size() <= i) pool.resize(i + 1, nullptr);
        if (!pool[i]) SGPR_HIP(hipEventCreateWithFlags(&pool[i], hipEventDisableTiming));
        return 0;
    }
};
Scratch g_scratch[2][MAX_DEVICES];
// tunables that report the allocation as failed (tests): the two lower ones are read once per process, the top one at every call
bool lower_noscratch()
{
    static const bool forced_fail = tune("gemm_strassen_noscratch", 0) != 0;
    return forced_fail;
}
bool top_noscratch() { return tune("rec_strassen3_noscratch", 0) != 0; }

void scratch_free(Scratch &s)
{
    if (s.p) (void)hipFree(s.p);        // waits for whatever still uses it
    s.p = nullptr; s.cap = 0; s.used = false;
}
// room for a call that needs `need` doubles per set: `sets` of them if that can be had, else fewer, down to one
bool ensure(Scratch &s, size_t need, int sets, bool forced_fail)
{
    if (forced_fail) return false;
    if (s.cap >= need) return true;
    if (s.failed && need >= s.failed) return false;
    scratch_free(s);
    for (int b = sets; b >= 1; --b) {
        const size_t want = need * (size_t)b;
        if (s.failed && want >= s.failed) continue;
        if (hipMalloc((void **)&s.p, want * sizeof(double)) == hipSuccess) { s.cap = want; return true; }
        (void)hipGetLastError();
        s.p = nullptr;
        s.failed = want;
    }
    return false;
}
// One use of the buffer by a call on `st` (the mutex held): begin() makes st wait for the previous user where that was another
// stream; every exit after it records the event behind whatever the call enqueued.
struct Use {
    Scratch &s; hipStream_t st; bool begun = false;
    Use(Scratch &s_, hipStream_t st_) : s(s_), st(st_) {}
    int begin()
    {
        if (!s.ev) SGPR_HIP(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
        if (s.used && s.last != st) SGPR_HIP(hipStreamWaitEvent(st, s.ev, 0));
        begun = true;
        return 0;
    }
    ~Use()
    {
        if (!begun) return;
        if (hipEventRecord(s.ev, st) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(st); }
        s.last = st;
        s.used = true;
    }
};

// On EVERY exit of an overlapped execution the caller's stream waits for its n side streams once more (one event each): the
// scratch may be reused or freed next.
struct Join {
    hipStream_t st; int n; hipStream_t side[2]; hipEvent_t ev[2];
    ~Join()
    {
        for (int t = 0; t < n; ++t)
            if (hipEventRecord(ev[t], side[t]) != hipSuccess || hipStreamWaitEvent(st, ev[t], 0) != hipSuccess) {
                (void)hipGetLastError();
                (void)hipStreamSynchronize(side[t]);
            }
    }
};

// Execute nrec inner-level records.  C2 == nullptr: C = beta C + alpha A B^T, one launch per record as the list says.
// C2 != nullptr (the records are the inner plan of an outer product): the same product also goes to C2 with factor alpha2 --
// a PLAN_PROD record with two destinations becomes a four-destination launch, one with one destination and a PLAN_CLASSIC
// record a two-destination launch.
int run_plan(const long long *recs, size_t nrec, double alpha, Mat A, Mat B, double beta, double *C, size_t ldc, double alpha2,
             double *C2, size_t ldc2, double *SA, double *SB, hipStream_t st, long sum_wgs = SUM_WGS)
{
    for (size_t i = 0; i < nrec; ++i) {
        const long long *r = recs + i * STRASSEN_REC;
        int rc = 0;
        if (r[0] == PLAN_SUM) {
            rc = sum_into(r, A, B, r[1] ? SB : SA, st, sum_wgs);
        } else if (r[0] == PLAN_PROD) {
            const int m = (int)r[7], n = (int)r[8], k = (int)r[9];
            const Mat X = operand_of(r, 0, A, SA), Y = operand_of(r, 1, B, SB);
            const Dests d = dests_of(r + 10, alpha, C, ldc);
            if (C2) {
                const Dests e = dests_of(r + 10, alpha2, C2, ldc2);
                double *cs[4] = {d.C1, nullptr, nullptr, nullptr};
                size_t ls[4] = {ldc, 0, 0, 0};
                double as[4] = {d.a1, 0.0, 0.0, 0.0};
                int cnt = 1;
                auto add = [&](double *p, size_t l, double a) { cs[cnt] = p; ls[cnt] = l; as[cnt] = a; ++cnt; };
                if (d.C2) add(d.C2, ldc, d.a2);
                add(e.C1, ldc2, e.a1);
                if (e.C2) add(e.C2, ldc2, e.a2);
                if (cnt == 2) rc = gemm_nt_two(m, n, k, as[0], X.p, X.ld, Y.p, Y.ld, 1.0, cs[0], ls[0], as[1], cs[1], ls[1], st);
                else          rc = gemm_nt_multi(m, n, k, X.p, X.ld, Y.p, Y.ld, 1.0, cnt, cs, ls, as, st);
            } else if (d.C2) {
                rc = gemm_nt_two(m, n, k, d.a1, X.p, X.ld, Y.p, Y.ld, 1.0, d.C1, ldc, d.a2, d.C2, ldc, st);
            } else {
                rc = gemm_nt(m, n, k, d.a1, X.p, X.ld, Y.p, Y.ld, 1.0, d.C1, ldc, 0, 0, st);
            }
        } else if (r[0] == PLAN_CLASSIC) {
            const double *Ap = block(A.p, A.ld, r[2], r[3]), *Bp = block(B.p, B.ld, r[4], r[5]);
            if (C2) rc = gemm_nt_two((int)r[6], (int)r[7], (int)r[8], alpha, Ap, A.ld, Bp, B.ld, beta, block(C, ldc, r[9], r[10]), ldc,
                                     alpha2, block(C2, ldc2, r[9], r[10]), ldc2, st);
            else    rc = gemm_nt((int)r[6], (int)r[7], (int)r[8], alpha, Ap, A.ld, Bp, B.ld, beta, block(C, ldc, r[9], r[10]), ldc, (int)r[1], 0, st);
        } else {
            set_error("run_plan: unknown record");
            rc = SGPR_E_ARG;
        }
        if (rc) return rc;
    }
    return 0;
}

// Execute a list of the two lower levels through its schedule (strassen.h): S = the scratch (s.p), laid out by the schedule's
// SchedCfg.  Overlapped form: at entry the side streams wait for everything that is on the caller's stream (the operands may have
// been written by the launches just before the call, and the scratch is whoever used it last until the wait in Use::begin in
// front of this); every sum is consumed by a product of the caller's stream, and on EVERY return, an error part-way through
// included, the caller's stream waits for the side streams once more: the scratch may be reused or freed next.  All waits of a
// product are enqueued before gemm_nt* is called, so the start event of an open profile window (gemm_launch) lies behind them.
// Serial form (overlap = false): the schedule has no side stream, so this is the list in order on the caller's stream, the sums
// on the grid they have there; no side stream is asked for, no event but Use's is created, recorded or waited for.
int run_schedule(const std::vector<long long> &plan, const Plan2Cfg &c, const Need2 &nd, bool overlap, double alpha, Mat A, Mat B,
                 double beta, double *C, size_t ldc, Scratch &s, hipStream_t st)
{
    Use use(s, st);
    int rc = use.begin();
    if (rc) return rc;
    const SchedCfg sc = sched_cfg_of(nd, s.cap, overlap);
    std::vector<long long> sch;
    schedule_of(plan, c, nd, sc, sch);
    const size_t nrec = sch.size() / SCHED_REC;
    const long wgs = sc.nstreams ? side_wgs() : SUM_WGS;
    hipStream_t str[3] = {st, nullptr, nullptr};
    if (sc.nstreams && (rc = strassen_sum_streams(st, sc.nstreams, str + 1))) return rc;
    // events: [0 .. nstreams) entry and exit, 2 + i behind record i where a record of another stream waits for it
    std::vector<char> needs(nrec, 0);
    for (size_t i = 0; i < nrec; ++i) {
        const long long *q = &sch[i * SCHED_REC];
        for (int j = 0; j < (int)q[20]; ++j)
            if (sch[(size_t)q[21 + j] * SCHED_REC + 17] != q[17]) needs[(size_t)q[21 + j]] = 1;
    }
    Join join{st, 0, {str[1], str[2]}, {nullptr, nullptr}};
    if (sc.nstreams) {
        if ((rc = s.event(0)) || (rc = s.event(1))) return rc;
        SGPR_HIP(hipEventRecord(s.pool[0], st));
        for (int t = 1; t <= sc.nstreams; ++t) SGPR_HIP(hipStreamWaitEvent(str[t], s.pool[0], 0));
        join.n = sc.nstreams; join.ev[0] = s.pool[0]; join.ev[1] = s.pool[1];
    }
    auto at = [&](int rg, long long b) { return s.p + sc.off[rg][b < 0 ? 0 : b]; };
    const long long *hd = nullptr;      // the outer product whose inner records are running
    for (size_t i = 0; i < nrec; ++i) {
        const long long *q = &sch[i * SCHED_REC];
        hipStream_t me = str[q[17]];
        for (int j = 0; j < (int)q[20]; ++j) {
            const size_t w = (size_t)q[21 + j];
            if (sch[w * SCHED_REC + 17] != q[17]) SGPR_HIP(hipStreamWaitEvent(me, s.pool[2 + w], 0));
        }
        if (q[0] == PLAN2_PROD) {
            hd = q;
            continue;
        }
        // a sum's [18] is the buffer it writes, a product's [18] / [19] the buffers it reads
        double *const SA = at(0, q[0] == PLAN_SUM && q[1] ? 0 : q[18]), *const SB = at(1, q[0] == PLAN_SUM ? q[18] : q[19]);
        if (q[0] == PLAN2_SUM) {
            rc = sum_into(q, A, B, at(2 + (int)q[1], q[18]), me, wgs);
        } else if (q[16] == 0) {
            rc = run_plan(q, 1, alpha, A, B, beta, C, ldc, 0.0, nullptr, 0, SA, SB, me, wgs);
        } else {
            // a record of the inner plan of hd: its operands and its destination pair are that product's
            const Dests d = dests_of(hd + 10, alpha, C, ldc);
            rc = run_plan(q, 1, d.a1, operand_of(hd, 0, A, at(2, hd[18])), operand_of(hd, 1, B, at(3, hd[19])), 1.0, d.C1, ldc, d.a2, d.C2, ldc,
                          SA, SB, me, wgs);
        }
        if (rc) return rc;
        if (needs[i]) {
            if ((rc = s.event(2 + i))) return rc;
            SGPR_HIP(hipEventRecord(s.pool[2 + i], me));
        }
    }
    return 0;
}

// Execute a top list.  Serial form: every record on the caller's stream in list order.  Overlapped form: the sums, the zeroing
// and the accumulations go to the library's low-priority top stream `sd` (one stream: they run in the order they are enqueued,
// so the accumulations of a C block stay in list order); the half-size calls and the pass-through calls stay on the caller's.
// With two buffer sets the accumulation of M_i is enqueued BEHIND the sums and the zeroing of M_i+1:
//     sd:  S0 Z0 S1 Z1 | A0 S2 Z2 | A1 S3 Z3 | ...          caller:  P0 | P1 | P2 ...
// P_i waits for the event behind Z_i, A_i for the event behind P_i; S_i+2 / Z_i+2 overwrite the set of M_i behind A_i, which has
// waited for P_i.  So the passes of M_i and the preparation of M_i+2 run under P_i+1.  With one set the accumulation goes in front
// of the next sums (list order): correct, and nothing overlaps.  sd waits for the caller's stream at entry (the operands may come
// from the launches just before), the caller's stream waits for sd in front of every pass-through call and on EVERY return.
int run_top(const std::vector<long long> &plan, const Need3 &nd, double alpha, Mat A, Mat B, double *C, size_t ldc, Scratch &s, hipStream_t st)
{
    Use use(s, st);
    int rc = use.begin();
    if (rc) return rc;
    const size_t need = nd.total();
    const bool overlap = tune("rec_strassen3_overlap", 1) != 0;
    const int nbuf = (top_buffers_wanted() >= 2 && s.cap >= 2 * need) ? 2 : 1;
    const long wgs = overlap ? side_wgs() : SUM_WGS;
    hipStream_t sd = st;
    if (overlap && (rc = strassen_top_stream(st, &sd))) return rc;
    auto at = [&](int region, int b) { return s.p + (size_t)b * need + (region == 0 ? 0 : (region == 1 ? nd.v[0] : nd.v[0] + nd.v[1])); };
    // events: 0 entry, 1 exit / joins, 2 + 2 p behind the zeroing of product p, 3 + 2 p behind product p
    auto join = [&]() {     // the caller's stream waits for everything on sd
        if (!overlap) return 0;
        SGPR_HIP(hipEventRecord(s.pool[1], sd));
        SGPR_HIP(hipStreamWaitEvent(st, s.pool[1], 0));
        return 0;
    };
    if ((rc = s.event(0)) || (rc = s.event(1))) return rc;
    if (overlap) {
        SGPR_HIP(hipEventRecord(s.pool[0], st));
        SGPR_HIP(hipStreamWaitEvent(sd, s.pool[0], 0));
    }
    Join at_exit{st, overlap ? 1 : 0, {sd, nullptr}, {s.pool[1], nullptr}};
    struct Pend { const long long *r; int b; size_t p; };
    std::vector<Pend> pending;
    size_t p = 0;       // the top product the records belong to; its buffer set: p % nbuf
    auto flush = [&]() {
        for (const Pend &q : pending) {
            if (overlap) SGPR_HIP(hipStreamWaitEvent(sd, s.pool[3 + 2 * q.p], 0));
            const Dests d = dests_of(q.r + 3, alpha, C, ldc);
            const int e = block_acc((int)q.r[1], (int)q.r[2], at(0, q.b), d.C1, d.a1, d.C2, d.a2, ldc, sd, wgs);
            if (e) return e;
        }
        pending.clear();
        return 0;
    };
    for (size_t i = 0; i + STRASSEN_REC <= plan.size(); i += STRASSEN_REC) {
        const long long *r = &plan[i];
        const int b = (int)(p % (size_t)nbuf);
        if (r[0] == PLAN3_SUM) {
            if (nbuf == 1 && (rc = flush())) return rc;
            rc = sum_into(r, A, B, at(1 + (int)r[1], b), sd, wgs);
        } else if (r[0] == PLAN3_ZERO) {
            if (nbuf == 1 && (rc = flush())) return rc;
            SGPR_HIP(hipMemsetAsync(at(0, b), 0, (size_t)r[1] * (size_t)r[2] * sizeof(double), sd));
        } else if (r[0] == PLAN3_PROD) {
            const int m = (int)r[7], n = (int)r[8], k = (int)r[9];
            if (overlap) {
                if ((rc = s.event(2 + 2 * p)) || (rc = s.event(3 + 2 * p))) return rc;
                SGPR_HIP(hipEventRecord(s.pool[2 + 2 * p], sd));
                SGPR_HIP(hipStreamWaitEvent(st, s.pool[2 + 2 * p], 0));
            }
            const Mat X = operand_of(r, 0, A, at(1, b)), Y = operand_of(r, 1, B, at(2, b));
            rc = gemm_nt_strassen_cfg(m, n, k, 1.0, X.p, X.ld, Y.p, Y.ld, 1.0, at(0, b), (size_t)m, 0, cfg_of_words(r + 10), st);
            if (rc) return rc;
            if (overlap) SGPR_HIP(hipEventRecord(s.pool[3 + 2 * p], st));
            rc = flush();       // the accumulations of the products before this one: behind its sums, under it
        } else if (r[0] == PLAN3_ACC) {
            pending.push_back(Pend{r, b, p});
            ++p;
        } else if (r[0] == PLAN3_PASS) {
            if ((rc = flush()) || (rc = join())) return rc;
            rc = gemm_nt_strassen_cfg((int)r[6], (int)r[7], (int)r[8], alpha, block(A.p, A.ld, r[2], r[3]), A.ld, block(B.p, B.ld, r[4], r[5]), B.ld,
                                      1.0, block(C, ldc, r[9], r[10]), ldc, (int)r[1], cfg_of_words(r + 11), st);
        } else {
            set_error("run_top: unknown record");
            rc = SGPR_E_ARG;
        }
        if (rc) return rc;
    }
    return flush();
}
}  // namespace

// make room for calls that need up to `both` doubles of scratch on st's device (potrf: once, before the first product);
// if that much cannot be had, `one` (what one level needs): the outer level is then skipped call by call
void strassen_reserve(size_t both, size_t one, hipStream_t st)
{
    const int dev = device_of(st);
    if (dev < 0 || !strassen_levels()) return;
    Scratch &s = g_scratch[0][dev];
    std::lock_guard<std::mutex> lock(s.mu);
    if (both > one && !outer_noscratch() && ensure(s, both, 1, lower_noscratch())) return;
    if (one) (void)ensure(s, one, 1, lower_noscratch());
}
// ... and for the top level's calls of one factorisation: two buffer sets if they can be had, else one; if not even that, the
// top level is off call by call and nothing else changes
void strassen_top_reserve(size_t need, hipStream_t st)
{
    const int dev = device_of(st);
    if (dev < 0 || !need) return;
    Scratch &s = g_scratch[1][dev];
    std::lock_guard<std::mutex> lock(s.mu);
    if (s.cap >= need * (size_t)top_buffers_wanted()) return;
    if (s.cap >= need && s.failed && need * 2 >= s.failed) return;      // the second set has been refused before
    scratch_free(s);
    (void)ensure(s, need, top_buffers_wanted(), top_noscratch());
}
int strassen_trim()
{
    for (int level = 1; level >= 0; --level)
        for (Scratch &s : g_scratch[level]) {
            std::lock_guard<std::mutex> lock(s.mu);
            scratch_free(s);
            if (s.ev) (void)hipEventDestroy(s.ev);
            for (hipEvent_t e : s.pool) if (e) (void)hipEventDestroy(e);
            s.pool.clear();
            s.ev = nullptr; s.failed = 0; s.last = nullptr;
        }
    (void)hipGetLastError();
    return 0;
}

// C = beta C + alpha A B^T (lower: on and below the diagonal of a square C only) through the lists of the two lower levels.
// Whatever does not qualify -- sizes, alignment, beta != 1, no scratch, SGPR_GEMM_STRASSEN=0 -- is the classical launch, bit for
// bit; without room for the outer pair (or with SGPR_GEMM_STRASSEN=1) the call is the one-level call, bit for bit.
int gemm_nt_strassen(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb, double beta,
                     double *C, size_t ldc, int lower, hipStream_t st)
{
    return gemm_nt_strassen_cfg(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, lower, StrassenCfg{}, st);
}
int gemm_nt_strassen_rec(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb, double beta,
                         double *C, size_t ldc, int lower, hipStream_t st)
{
    return gemm_nt_strassen_cfg(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, lower, strassen_rec_cfg(strassen_rec_values(), k, lower), st);
}
// ... with the thresholds of this one call (the recursive factorisation's calls: chol.hip)
int gemm_nt_strassen_cfg(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb, double beta,
                         double *C, size_t ldc, int lower, const StrassenCfg &cfg, hipStream_t st)
{
    const Plan2Cfg c2 = cfg2_of(cfg, ~(size_t)0);
    const bool aligned = ((((uintptr_t)A | (uintptr_t)B) & 15) == 0) && (((lda | ldb) & 1) == 0);
    // (the size test first: the short products of the panel solves come through here by the thousand)
    if (std::min(m, n) / 2 < std::min(c2.in.smin, under_of(c2).smin) || !strassen_levels() || !aligned || beta != 1.0 || (lower && m != n))
        return gemm_nt(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, lower, 0, st);
    std::vector<long long> plan;
    int rc = 0;
    const int dev = device_of(st);
    const bool overlap = tune("gemm_strassen_overlap", 1) != 0;     // the sums on a side stream under the products; 0: the serial form
    const Mat Am{A, lda}, Bm{B, ldb};
    // both levels, where a product is large enough for the outer one and its scratch can be had
    if (strassen_levels() >= 2 && dev >= 0 && !outer_noscratch() && std::min(lower ? m / 2 : m, lower ? n / 2 : n) / 2 >= c2.smin2) {
        outer_plan_of(m, n, k, lower, c2, plan);
        const Need2 nd = plan_need(plan, c2);
        if (nd.v[2] + nd.v[3]) {
            Scratch &s = g_scratch[0][dev];
            std::lock_guard<std::mutex> lock(s.mu);
            if (ensure(s, nd.total(), 1, lower_noscratch())) return run_schedule(plan, c2, nd, overlap, alpha, Am, Bm, beta, C, ldc, s, st);
        }
    }
    auto unscratched = [&] { return run_plan(plan.data(), plan.size() / STRASSEN_REC, alpha, Am, Bm, beta, C, ldc, 0.0, nullptr, 0, nullptr, nullptr, st); };
    rc = strassen_plan(m, n, k, lower, c2.in.smin, c2.in.kslab, ~(size_t)0, plan);
    if (rc) return rc;
    Need2 nd = plan_need(plan, c2);
    if (!nd.total()) return unscratched();
    if (dev < 0) return gemm_nt(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, lower, 0, st);
    Scratch &s = g_scratch[0][dev];
    std::lock_guard<std::mutex> lock(s.mu);
    if (!ensure(s, nd.total(), 1, lower_noscratch())) {
        // plan again with what there is (possibly nothing): smaller products of a SYRK may still fit
        if ((rc = strassen_plan(m, n, k, lower, c2.in.smin, c2.in.kslab, s.cap, plan))) return rc;
        nd = plan_need(plan, c2);
        if (!nd.total()) return unscratched();
    }
    return run_schedule(plan, c2, nd, overlap, alpha, Am, Bm, beta, C, ldc, s, st);
}

// C += alpha A B^T as the recursion issues it, with the top level where it applies.  Whatever does not qualify is exactly the
// call gemm_nt_strassen_cfg(..., strassen_rec_cfg(v, k, lower), st) that stood here before.
int strassen_top_gemm(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb, double beta,
                      double *C, size_t ldc, int lower, const StrassenRec *vp, const StrassenTop *tp, hipStream_t st)
{
    const StrassenRec v = vp ? *vp : strassen_rec_values();
    const StrassenTop t = tp ? *tp : strassen_top_values();
    const StrassenCfg cfg = strassen_rec_cfg(v, k, lower);
    // (the size test first: the short products of the panel solves come through here by the thousand)
    const bool aligned = ((((uintptr_t)A | (uintptr_t)B | (uintptr_t)C) & 15) == 0) && (((lda | ldb | ldc) & 1) == 0);
    const int dev = (!v.on || t.smin3 <= 0 || std::min(lower ? m / 2 : m, lower ? n / 2 : n) / 2 < t.smin3) ? -1 : device_of(st);
    if (dev < 0 || strassen_levels() < 2 || !aligned || beta != 1.0 || (lower && m != n))
        return gemm_nt_strassen_cfg(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, lower, cfg, st);
    std::vector<long long> plan;
    const int rc = strassen_top_plan(m, n, k, lower, &v, &t, ~(size_t)0, plan);
    if (rc) return rc;
    const Need3 nd = top_need(plan);
    if (nd.total()) {
        Scratch &s = g_scratch[1][dev];
        std::lock_guard<std::mutex> lock(s.mu);
        if (ensure(s, nd.total(), top_buffers_wanted(), top_noscratch())) return run_top(plan, nd, alpha, Mat{A, lda}, Mat{B, ldb}, C, ldc, s, st);
    }
    return gemm_nt_strassen_cfg(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, lower, cfg, st);
}

}  // namespace sgpr
