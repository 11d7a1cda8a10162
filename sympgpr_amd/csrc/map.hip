// map.hip -- the symplectic map of a one-pair (d = 1) fit for gfx950 (MI355X): every time step of every orbit on the device,
// for one GP pair (applymap_kernel) and for one GP pair per toroidal section (applymap_sections_kernel).  The two kernels
// share one time step (map_step) and one copy of the per-thread sums (rows_part, guess_part).  The sectioned kernel has a TAN
// instance: the step's Jacobian, the monodromy matrix and the finite-time Lyapunov exponents of every orbit -- mapsec_tan.h sums
// the Hessian on this file's data layout, tangent_core.h (shared with map_nd.hip) has everything that follows from it.
// applymap_sections_inverse_kernel iterates the sectioned map (one section: the one-pair map) backwards, with map_step_inverse.
// The three sectioned kernels read their sections through one SecReader and are launched by one host helper.
#include <atomic>
#include <type_traits>
#include "common.h"
#include "devmath.h"
#include "pair_eval.h"

namespace sgpr {

namespace {

using namespace pairf;

// ---- applymap: the whole symplectic-map iteration of one orbit inside one workgroup ------------
// functions/func.py:216-260 (applymap / applymap_henon) with calcP / calcQ / guessP of
// sympgpr.f90:62-125 inlined: per time step, P_new is the root of f(P) = pGP(q, P) - p + P started
// from the regular-GP guess (the reference runs MINPACK hybrd1, tol 1e-13, per point and step, each
// residual an O(n^2) matmul with Kyinv); here alpha = Kyinv ztrain is cached, a residual is one
// block-wide reduction over the training points, and all nm steps run without leaving the GPU.
constexpr int MAP_T = 256;          // threads of a workgroup that has its orbit to itself
constexpr int MAP_TEAM_T = 256;     // threads of a team member
constexpr int MAP_TEAM_MAX = 16;    // members of a team at most
constexpr int MAP_STAGE = 5;        // rounds of TT training points a member keeps in LDS (7 doubles per point: 70 KB at 256 threads)
struct MapArgs {
    int nm, ntest, n0, n0p, mode, maxiter;
    int S;                                // workgroups per orbit (the team): each sums its share of the training points
    unsigned long long *tw;               // team exchange words: [orbit][member][parity][2] 16-byte granules {value, sequence}, zero on entry
    int *err;                             // set when a team member gave up waiting for another
    double tol;
    const double *xtr, *ytr, *alpha;      // symplectic GP: n0 points, alpha 2 n0
    const double *xtrp, *ytrp, *alphap;   // regular GP (guess): n0p points
    const double *Q0, *P0;
    double *qmap, *pmap, *pdiff;          // [nm][ntest], C order (numpy zeros([nm, Ntest])); pdiff may be null
    KConst kc, kcp;
};

// `sh`: 2 * (TT / 64) doubles that the call before did NOT use (the callers alternate between two: a wave that is still reading
// the sums of call n cannot be overtaken by the writes of call n + 2, because call n + 1's barrier lies between)
template <int TT>
__device__ __forceinline__ void block_sum2(double &a, double &b, double *sh)
{
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o, 64);
        b += __shfl_down(b, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sh[2 * (threadIdx.x >> 6)] = a;
        sh[2 * (threadIdx.x >> 6) + 1] = b;
    }
    __syncthreads();
    double x = 0.0, y = 0.0;
#pragma unroll
    for (int w = 0; w < TT / 64; ++w) { x += sh[2 * w]; y += sh[2 * w + 1]; }
    a = x; b = y;
}

// 16-byte {value, sequence number} granules, written by one write-through store and read by one load that passes the vector L1
// (MI355X_MICROARCH.md, inter-workgroup visibility: 16-byte sc1 halves were observed untorn): the value and the word that says
// which residual it belongs to arrive together, so a member that finds the expected sequence number has the value.
typedef unsigned uint4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void granule_store(unsigned long long *p, double v, unsigned seq)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const uint4_t w = {(unsigned)b, (unsigned)(b >> 32), seq, 0u};
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(w) : "memory");
}
// both granules of a pair in flight together: one memory round trip per look
__device__ __forceinline__ void granule_load2(const unsigned long long *p, uint4_t &u, uint4_t &v)
{
    asm volatile("global_load_dwordx4 %0, %2, off sc1\n\tglobal_load_dwordx4 %1, %2, off offset:16 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(u), "=&v"(v) : "v"(p) : "memory");
}

// One thread's share of Kstar(1,:).alpha and Kstar(2,:).alpha at (q, P): the points j, j + dj, ... < n, added in that order;
// point j + i dj has its x, y and its two weights at index l + i dl of the four arrays (LDS or memory: each call site passes
// one kind, so the address space stays known after inlining)
template <int FAM>
__device__ __forceinline__ void rows_part(const double *x, const double *y, const double *w1, const double *w2, int l, int dl,
                                          int j, int dj, int n, double q, double P, const KConst &kc, double &r1, double &r2)
{
    r1 = 0.0; r2 = 0.0;
    for (; j < n; j += dj, l += dl) {
        double kxx, kxy, kyy;
        pair_eval<FAM, false>(x[l], y[l], q, P, kc, kxx, kxy, kyy);
        const double a1 = w1[l], a2 = w2[l];
        r1 += kxx * a1 + kxy * a2;
        r2 += kxy * a1 + kyy * a2;
    }
}
// ... and of the regular GP's Kstar.alphap at (q, p), the same way
template <int FAM>
__device__ __forceinline__ double guess_part(const double *x, const double *y, const double *w, int l, int dl, int j, int dj,
                                             int n, double q, double p, const KConst &kcp)
{
    double r = 0.0;
    for (; j < n; j += dj, l += dl) r += kcp.sig * kern_eval<FAM, false>(x[l], y[l], q, p, kcp) * w[l];
    return r;
}

// One time step (q, p, pd) -> (q, p, pd) of one orbit, pd the unwrapped momentum; NaN in all three from the step at which the
// orbit is lost.  rows(q, P, r1, r2) leaves the workgroup's (the team's) sums Kstar(1,:).alpha, Kstar(2,:).alpha at (q, P) in
// r1, r2; guess(q, p) returns the regular GP's first guess of P.  Two things must hold for every caller:
//   * call order and count: a rows / guess call contains a workgroup barrier and, with teams, an exchange in which workgroups
//     wait for each other.  So every value that decides a branch here is the block-uniform, team-uniform result of those sums
//     (or a kernel argument), and all threads of all members make the same calls in the same order: guess once, then rows for
//     the two starting residuals, once per secant iteration, and once more for q unless the last residual's r2 can be reused.
//     sgpr_probe_map_calls() counts the rows calls.
//   * order of additions: nothing here adds across threads; the callables add a thread's points in ascending order and reduce
//     with block_sum2 on alternating LDS halves, so a step has the same bits in both kernels.
template <typename Rows, typename Guess>
__device__ __forceinline__ void map_step(int mode, int maxiter, double tol, double &q, double &p, double &pd, Rows &&rows,
                                         Guess &&guess)
{
    const double nan = __builtin_nan("");
    const double twopi = 6.283185307179586477;
    double qn = nan, pn = nan, pdn = nan;
    if (!(q != q) && !(p != p)) {                      // NaN = lost orbit stays lost (func.py:231-232, Split_SympGPR/func.py:199-200)
        double r1, r2, Praw = nan;
        bool have_r2 = false;
        if (mode & SGPR_MAP_EXPLICIT) {
            // explicit map (01_pendulum/explicit/func_expl.py:106-119, 04_standard_map/func.py:174-179):
            // P = p - Kstar(1,:).alpha at (q, p), no implicit equation
            rows(q, p, r1, r2);
            Praw = p - r1;
        } else {
            double P0 = guess(q, p);
            rows(q, P0, r1, r2);
            double f0 = r1 - p + P0;
            double P1 = P0 - f0;                            // f'(P) ~ 1 near the identity map
            rows(q, P1, r1, r2);
            double f1 = r1 - p + P1;
            for (int it = 0; it < maxiter; ++it) {          // secant; every quantity is block-uniform
                if (!(fabs(P1 - P0) > tol * fmax(1.0, fabs(P1))) || !(f1 == f1)) break;
                const double d = f1 - f0;
                if (d == 0.0) break;
                const double Pn = P1 - f1 * (P1 - P0) / d;
                P0 = P1; f0 = f1; P1 = Pn;
                rows(q, P1, r1, r2);
                f1 = r1 - p + P1;
            }
            if ((f1 == f1) && fabs(f1) <= 1e-8 * fmax(1.0, fabs(p))) {
                Praw = P1;
                have_r2 = true;                              // r2 belongs to (q, P1)
            }
        }
        // 05_tokamak/SympGPR/func.py:190-211, sympgpr.f90:128-177 (Split_SympGPR/func.py:215, its P < 0 half): an orbit whose
        // new momentum is negative has left the plasma -- lost from this step on (the flux-surface half of that test needs the
        // out-of-scope fieldlines module and stays with the caller: examples/tokamak.py)
        if ((mode & SGPR_MAP_LOSS_NEGP) && Praw < 0.0) Praw = nan;
        if (Praw == Praw) {
            pdn = pd + (Praw - p);                           // unwrapped momentum (04_standard_map/func.py:234)
            pn = Praw;
            if (mode & SGPR_MAP_WRAP_P) pn -= twopi * floor(pn / twopi);
            if (!have_r2 || pn != Praw) rows(q, pn, r1, r2);
            qn = r2 + q;                                     // Eq. (43)
            if (mode & SGPR_MAP_WRAP_Q) qn -= twopi * floor(qn / twopi);
        }
    }
    q = qn; p = pn; pd = pdn;
}

// One workgroup per (orbit, team member).  With a.S == 1 this is the round-2 kernel: one workgroup runs the whole iteration
// of its orbit.  For large training sets (the drivers use 20 - 80 points; BASELINE config 05 has 16384) S workgroups share an
// orbit: every residual is summed in S parts, exchanged through a.tw and added up in member order by every member alike -- all
// members then hold the same bits, take the same branches and need no leader.  Ntest = 37 orbits no longer mean 37 CUs.
// TT threads: MAP_T for one workgroup per orbit (the drivers' sizes: latency of a few dozen points), MAP_TEAM_T for the teams
template <int FAM, int TT>
__global__ __launch_bounds__(TT) void applymap_kernel(const MapArgs a)
{
    __shared__ double sh[2][2 * (TT / 64)];
    __shared__ double sp[2][2][MAP_TEAM_MAX];           // [parity of the call]
    const int S = a.S, k = blockIdx.x / S, me = blockIdx.x - k * S;
    unsigned seq = 0;
    bool lost = false;                                  // a team member did not answer in time: the orbit is lost (NaN), a.err says why
    // (x, y) := sum over the team of every thread's (x, y), identical bits in every member: the workgroup's own sum first, then
    // ONE pair of granules per member, collected by lanes 0 .. S - 1.  (Tried: every wave publishing its own part, 4 S and 16 S
    // granule pairs to collect -- no gain at 256 threads, 40 instead of 65 G pair evaluations per second at 1024.)
    __shared__ int sh_lost;
    if (threadIdx.x == 0) sh_lost = 0;
    __syncthreads();
    auto team_sum2 = [&](double &x, double &y) {
        ++seq;
        block_sum2<TT>(x, y, sh[seq & 1u]);
        if (S == 1) return;
        if (lost) {                                     // sticky: one timeout ends the orbit, nobody waits 2 s per sum after it
            x = y = __builtin_nan("");
            return;
        }
        if (threadIdx.x == 0) {
            unsigned long long *mine = a.tw + (((size_t)k * S + me) * 2 + (seq & 1u)) * 4;
            granule_store(mine, x, seq);
            granule_store(mine + 2, y, seq);
        }
        if (threadIdx.x < (unsigned)S) {
            const unsigned long long *theirs = a.tw + (((size_t)k * S + threadIdx.x) * 2 + (seq & 1u)) * 4;
            uint4_t u, v;
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
            unsigned it = 0;
            bool ok = true;
            for (;;) {
                granule_load2(theirs, u, v);
                if (u[2] == seq && v[2] == seq) break;
                if ((++it & 255u) == 0 && __builtin_amdgcn_s_memrealtime() - t0 > 200000000ull) { ok = false; break; }    // 2 s
            }
            sp[seq & 1u][0][threadIdx.x] = ok ? __longlong_as_double((long long)(((unsigned long long)u[1] << 32) | u[0])) : __builtin_nan("");
            sp[seq & 1u][1][threadIdx.x] = ok ? __longlong_as_double((long long)(((unsigned long long)v[1] << 32) | v[0])) : __builtin_nan("");
            if (!ok) { atomicExch(a.err, 1); sh_lost = 1; }
        }
        __syncthreads();
        lost = sh_lost != 0;                            // (block-uniform; sh_lost is only ever raised)
        double sx = 0.0, sy = 0.0;
        for (int m = 0; m < S; ++m) { sx += sp[seq & 1u][0][m]; sy += sp[seq & 1u][1][m]; }
        x = sx; y = sy;                                 // (no barrier behind the reads: the next call writes the other halves)
    };
    // This member's training points never change: they are staged in LDS once (a residual is a handful of points per thread, and
    // their loads -- four per point, L2 latency each round -- were two thirds of its time at N0 = 16 384: 1.2 us per point and
    // thread against ~0.4 of arithmetic).  Same points, same order per thread: same bits.  Slices that do not fit stay in memory.
    __shared__ double st[7][MAP_STAGE * TT];            // x, y, alpha (two halves) of the symplectic GP; x, y, alpha of the guess
    auto rounds_of = [&](int n) { return n > me * TT ? (n - me * TT + S * TT - 1) / (S * TT) : 0; };
    const int nr = rounds_of(a.n0), nrp = rounds_of(a.n0p);
    const bool staged = nr <= MAP_STAGE && nrp <= MAP_STAGE;
    if (staged) {
        for (int i = 0; i < nr; ++i) {
            const int j = me * TT + (int)threadIdx.x + i * S * TT;
            if (j < a.n0) {
                st[0][i * TT + threadIdx.x] = a.xtr[j]; st[1][i * TT + threadIdx.x] = a.ytr[j];
                st[2][i * TT + threadIdx.x] = a.alpha[j]; st[3][i * TT + threadIdx.x] = a.alpha[a.n0 + j];
            }
        }
        for (int i = 0; i < nrp; ++i) {
            const int j = me * TT + (int)threadIdx.x + i * S * TT;
            if (j < a.n0p) {
                st[4][i * TT + threadIdx.x] = a.xtrp[j]; st[5][i * TT + threadIdx.x] = a.ytrp[j]; st[6][i * TT + threadIdx.x] = a.alphap[j];
            }
        }
        // (every thread reads back what it wrote itself: no barrier needed)
    }
    unsigned ncalls = 0;                                // residual evaluations of this orbit (measurement aid)
    const int tid = threadIdx.x, j0 = me * TT + tid, dj = S * TT;   // this thread's points: j0, j0 + dj, ...; round i staged at i TT + tid
    auto rows = [&](double q, double P, double &r1, double &r2) {   // Kstar(1,:).alpha, Kstar(2,:).alpha
        ++ncalls;
        if (staged) rows_part<FAM>(st[0], st[1], st[2], st[3], tid, TT, j0, dj, a.n0, q, P, a.kc, r1, r2);
        else        rows_part<FAM>(a.xtr, a.ytr, a.alpha, a.alpha + a.n0, j0, dj, j0, dj, a.n0, q, P, a.kc, r1, r2);
        team_sum2(r1, r2);
    };
    auto guess = [&](double q, double p) {
        double z = 0.0;
        double r = staged ? guess_part<FAM>(st[4], st[5], st[6], tid, TT, j0, dj, a.n0p, q, p, a.kcp)
                          : guess_part<FAM>(a.xtrp, a.ytrp, a.alphap, j0, dj, j0, dj, a.n0p, q, p, a.kcp);
        team_sum2(r, z);
        return r;
    };
    const bool writer = threadIdx.x == 0 && me == 0;
    double q = a.Q0[k], p = a.P0[k], pd = p;
    if (writer) {
        a.qmap[k] = q;
        a.pmap[k] = p;
        if (a.pdiff) a.pdiff[k] = pd;
    }
    for (int i = 0; i + 1 < a.nm; ++i) {
        // some team of this call has given up (a.err): every member of every team sees it at its next step and writes NaN for
        // the rest of its orbit instead of waiting for partners that have diverged
        if (S > 1 && !lost && __hip_atomic_load((__attribute__((address_space(1))) int *)a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) lost = true;
        if (lost) q = p = pd = __builtin_nan("");
        else map_step(a.mode, a.maxiter, a.tol, q, p, pd, rows, guess);
        if (writer) {
            a.qmap[(size_t)(i + 1) * a.ntest + k] = q;
            a.pmap[(size_t)(i + 1) * a.ntest + k] = p;
            if (a.pdiff) a.pdiff[(size_t)(i + 1) * a.ntest + k] = pd;
        }
    }
    if (writer) atomicAdd((unsigned *)(a.err + 1), ncalls);
}

// ---- applymap over sections: 05_tokamak/Split_SympGPR/func.py:184-219 -- nsec independent GP pairs, one per toroidal
// section, applied in turn: step i -> i + 1 of every orbit uses section (first + i) mod nsec.  The step and the sums are
// applymap_kernel's, called with its S == 1 order per thread (j = tid, tid + TT, ...), so a step has the bits of a one-step
// applymap_kernel launch with S == 1 on that section's data.  One workgroup per orbit at every size: sections exist to keep
// each fit small, and a kernel in which no workgroup waits for another has nothing that can hang.
constexpr long MAPSEC_STAGE = 8960;   // doubles of LDS for the staged sections: the 70 KB applymap_kernel reserves (7 * MAP_STAGE * 256)
// One argument block for the three sectioned kernels; the backward one has no guess GPs (n0p = 0, their pointers null) and no pdiff.
struct MapSecArgs {
    int nm, ntest, n0, n0p, mode, maxiter;
    int nsec, first;
    int staged;                           // all sections' points and weights fit into MAPSEC_STAGE doubles of (dynamic) LDS
    double tol;
    const double *xtr, *ytr, *alpha;      // symplectic GPs: n0 x nsec, n0 x nsec, 2 n0 x nsec, column-major, tight
    const double *xtrp, *ytrp, *alphap;   // regular GPs (guess): n0p x nsec each
    const double *Q0, *P0;
    double *qmap, *pmap, *pdiff;          // [nm][ntest], C order; pdiff may be null
};
struct MapSecInvArgs : MapSecArgs {
    int *iters;                           // [nm - 1][ntest] or null
};

#include "tangent_core.h"   // block_sum_n; the step matrix and the monodromy / Benettin step of the TAN instance
#include "mapsec_tan.h"     // MapSecTanArgs; the Hessian sums of the TAN instance

// The sections' points and weights as thread `tid` of an orbit's workgroup (TT threads) reads them: from dynamic LDS
// ([section]{x, y, alpha (two halves): n0 each; guess x, y, alpha: n0p each}, `per` doubles a section) when all sections fit,
// from memory otherwise.  The thread's points are j = tid, tid + TT, ... in that order, staged or not: the same bits.  Every
// call keeps its staged / unstaged branch with one kind of pointer in each (see rows_part).  The sums over the workgroup stay
// with the kernels.
template <int TT>
struct SecReader {
    const MapSecArgs &a;
    double *sec_st;
    int per;                                            // (staged only: nsec * per <= MAPSEC_STAGE)
    bool staged;
    int n0, n0p, tid;
    __device__ __forceinline__ SecReader(const MapSecArgs &args, double *lds)
        : a(args), sec_st(lds), per(4 * args.n0 + 3 * args.n0p), staged(args.staged != 0), n0(args.n0), n0p(args.n0p), tid(threadIdx.x) {}

    __device__ __forceinline__ void stage() const
    {
        if (!staged) return;
        for (int s = 0; s < a.nsec; ++s) {
            double *d = sec_st + s * per;
            const double *x = a.xtr + (size_t)s * n0, *y = a.ytr + (size_t)s * n0, *al = a.alpha + (size_t)s * 2 * n0;
            for (int j = tid; j < n0; j += TT) {
                d[j] = x[j]; d[n0 + j] = y[j];
                d[2 * n0 + j] = al[j]; d[3 * n0 + j] = al[n0 + j];
            }
            const double *xp = a.xtrp + (size_t)s * n0p, *yp = a.ytrp + (size_t)s * n0p, *alp = a.alphap + (size_t)s * n0p;
            for (int j = tid; j < n0p; j += TT) {
                d[4 * n0 + j] = xp[j]; d[4 * n0 + n0p + j] = yp[j]; d[4 * n0 + 2 * n0p + j] = alp[j];
            }
        }
        // (every thread reads back what it wrote itself: no barrier needed)
    }
    // this thread's share of section m's Kstar(1,:).alpha, Kstar(2,:).alpha at (q, P)
    template <int FAM>
    __device__ __forceinline__ void rows(int m, double q, double P, const KConst &kc, double &r1, double &r2) const
    {
        if (staged) {
            const double *d = sec_st + m * per;
            rows_part<FAM>(d, d + n0, d + 2 * n0, d + 3 * n0, tid, TT, tid, TT, n0, q, P, kc, r1, r2);
        } else {
            const double *al = a.alpha + (size_t)m * 2 * n0;
            rows_part<FAM>(a.xtr + (size_t)m * n0, a.ytr + (size_t)m * n0, al, al + n0, tid, TT, tid, TT, n0, q, P, kc, r1, r2);
        }
    }
    // ... of section m's regular GP's Kstar.alphap at (q, p)
    template <int FAM>
    __device__ __forceinline__ double guess(int m, double q, double p, const KConst &kcp) const
    {
        const double *d = sec_st + m * per + 4 * n0;
        return staged ? guess_part<FAM>(d, d + n0p, d + 2 * n0p, tid, TT, tid, TT, n0p, q, p, kcp)
                      : guess_part<FAM>(a.xtrp + (size_t)m * n0p, a.ytrp + (size_t)m * n0p, a.alphap + (size_t)m * n0p,
                                        tid, TT, tid, TT, n0p, q, p, kcp);
    }
    // ... of section m's three Hessian sums at (q, P) (mapsec_tan.h)
    template <int FAM>
    __device__ __forceinline__ void hess(int m, double q, double P, const KConst &kc, double &hA, double &hB, double &hC) const
    {
        if (staged) {
            const double *d = sec_st + m * per;
            sec_hess_part<FAM>(d, d + n0, d + 2 * n0, d + 3 * n0, tid, TT, tid, TT, n0, q, P, kc, hA, hB, hC);
        } else {
            const double *al = a.alpha + (size_t)m * 2 * n0;
            sec_hess_part<FAM>(a.xtr + (size_t)m * n0, a.ytr + (size_t)m * n0, al, al + n0, tid, TT, tid, TT, n0, q, P, kc, hA, hB, hC);
        }
    }
};

// TAN: after every accepted step (new p finite: block-uniform) one more pass over section m's points sums the Hessian of the
// generating function at (q_old, P_new); the step's Jacobian M, the product of the M's and the Benettin sums follow from it
// (tangent_core.h at D = 2, H = {A, B, C}).  The orbit itself makes the same rows / guess calls in the same order as without TAN
// and has the same bits.  A lost orbit's M is NaN from that step on, and with it mono and the exponents.
// kcs, kcps: the sections' constants (make_kconst) in device memory, nsec each; a step reads its pair with block-uniform loads
// (__restrict__: nothing the kernel writes can alias them, so the compiler fetches them with scalar loads, into SGPRs, where
// applymap_kernel has its kernel arguments)
template <int FAM, int TT, bool TAN = false>
__global__ __launch_bounds__(TT) void applymap_sections_kernel(const std::conditional_t<TAN, MapSecTanArgs, MapSecArgs> a,
                                                               const KConst *__restrict__ kcs, const KConst *__restrict__ kcps)
{
    static_assert(TT / 64 <= 4, "block_sum_n<3, TT> gets no `res` half here");
    __shared__ double sh[2][(TAN ? 3 : 2) * (TT / 64)];  // [wave][sum] of block_sum2 / block_sum_n<3>, two alternating halves
    extern __shared__ double sec_st[];
    const int k = blockIdx.x, tid = threadIdx.x;
    const SecReader<TT> rd(a, sec_st);
    rd.stage();
    unsigned seq = 0;
    auto sum2 = [&](double &x, double &y) {
        ++seq;
        block_sum2<TT>(x, y, sh[seq & 1u]);
    };
    double q = a.Q0[k], p = a.P0[k], pd = p;
    if (tid == 0) {
        a.qmap[k] = q;
        a.pmap[k] = p;
        if (a.pdiff) a.pdiff[k] = pd;
    }
    int m = a.first;
    if constexpr (TAN) maptan_init<2>();
    for (int i = 0; i + 1 < a.nm; ++i) {
        const KConst kc = kcs[m];
        const double q_old = q;
        auto rows = [&](double q, double P, double &r1, double &r2) {   // section m's Kstar(1,:).alpha, Kstar(2,:).alpha
            rd.template rows<FAM>(m, q, P, kc, r1, r2);
            sum2(r1, r2);
        };
        auto guess = [&](double q, double p) {
            const KConst kcp = kcps[m];
            double z = 0.0;
            double r = rd.template guess<FAM>(m, q, p, kcp);
            sum2(r, z);
            return r;
        };
        map_step(a.mode, a.maxiter, a.tol, q, p, pd, rows, guess);
        if constexpr (TAN) {                                // section m's Hessian at (q_old, P_new) of the accepted step
            double M[4];
            bool tan_ok = false;
            if (finite_d(p)) {
                double H[3];
                rd.template hess<FAM>(m, q_old, p, kc, H[0], H[1], H[2]);
                ++seq;
                block_sum_n<3, TT>(H, sh[seq & 1u], nullptr);
                tan_ok = maptan_matrix<2>(H, M);
            }
            if (!tan_ok) M[0] = M[1] = M[2] = M[3] = __builtin_nan("");
            maptan_publish<2>(M, a.jac ? a.jac + ((size_t)i * a.ntest + k) * 4 : nullptr);
            maptan_advance<2, true>();
        }
        if (++m == a.nsec) m = 0;
        if (tid == 0) {
            a.qmap[(size_t)(i + 1) * a.ntest + k] = q;
            a.pmap[(size_t)(i + 1) * a.ntest + k] = p;
            if (a.pdiff) a.pdiff[(size_t)(i + 1) * a.ntest + k] = pd;
        }
    }
    if constexpr (TAN) maptan_finish<2>(a.mono, a.lyap, a.nm, k);
}

// ---- the sectioned map BACKWARDS.  The forward step passes through the point (q, P): it solves p = P + r1(q, P) for P and sets
// Q = q + r2(q, P).  The backward step passes through the same point with the roles swapped: P is known, it solves
// g(q) = q + r2(q, P) - Q = 0 for q and sets p = P + r1(q, P).
// One backward step (Q, P) -> (q, p) of one orbit, map_step's twin; NaN in both from the step at which the orbit is lost, `iters`
// the secant updates (the rows calls beyond the two starting residuals), -1 for a lost step.  The same two rules hold as for
// map_step: every value that decides a branch is the block-uniform result of the sums (or a kernel argument), so all threads
// make the same rows calls in the same order -- two starting residuals, then one per secant update --, and nothing here adds
// across threads.  The r1 of the last rows call belongs to (q1, P): no further pass for p.  No first-guess GP: the secant starts
// from q = Q, the identity map's answer.
template <typename Rows>
__device__ __forceinline__ void map_step_inverse(int mode, int maxiter, double tol, double &q, double &p, int &iters, Rows &&rows)
{
    const double nan = __builtin_nan("");
    const double twopi = 6.283185307179586477;
    const double Q = q, P = p;
    double qn = nan, pn = nan;
    int itn = -1;
    if (finite_d(Q) && finite_d(P)) {              // NaN = lost orbit stays lost; an infinite start value is lost as well
        double r1, r2;
        double q0 = Q;
        rows(q0, P, r1, r2);
        double f0 = r2;                                 // g(q0) = q0 + r2 - Q at q0 = Q
        double q1 = q0 - f0;                            // g'(q) ~ 1 near the identity map
        rows(q1, P, r1, r2);
        double f1 = q1 + r2 - Q;
        int it = 0;
        for (; it < maxiter; ++it) {                    // secant; every quantity is block-uniform
            if (!(fabs(q1 - q0) > tol * fmax(1.0, fabs(q1))) || !finite_d(f1)) break;
            const double d = f1 - f0;
            if (d == 0.0) break;
            const double qs = q1 - f1 * (q1 - q0) / d;
            q0 = q1; f0 = f1; q1 = qs;
            rows(q1, P, r1, r2);
            f1 = q1 + r2 - Q;
        }
        if (finite_d(f1) && fabs(f1) <= 1e-8 * fmax(1.0, fabs(Q))) {   // the forward rule with the roles swapped
            const double pp = P + r1;                   // r1 belongs to (q1, P)
            // the backward twin of the forward "new momentum < 0": the preimage has left the plasma
            const bool negp = (mode & SGPR_MAP_LOSS_NEGP) && pp < 0.0;
            if (finite_d(pp) && !negp) {
                pn = pp;
                qn = q1;
                if (mode & SGPR_MAP_WRAP_Q) qn -= twopi * floor(qn / twopi);
                itn = it;
            }
        }
    }
    q = qn; p = pn; iters = itn;
}

// All nm - 1 backward steps of all orbits in one launch: step i (row i -> row i + 1) undoes section (first - i) mod nsec,
// `first` the section whose forward step produced row 0.  applymap_sections_kernel's shape: one workgroup per orbit, the
// sections through the same SecReader (no guess GP: n0p = 0, 4 n0 doubles per section), rows + block_sum2 on alternating LDS
// halves, the sections' constants by block-uniform scalar loads.  No workgroup waits for another.
template <int FAM, int TT>
__global__ __launch_bounds__(TT) void applymap_sections_inverse_kernel(const MapSecInvArgs a, const KConst *__restrict__ kcs)
{
    __shared__ double sh[2][2 * (TT / 64)];
    extern __shared__ double sec_st[];
    const int k = blockIdx.x, tid = threadIdx.x;
    const SecReader<TT> rd(a, sec_st);
    rd.stage();
    unsigned seq = 0;
    auto sum2 = [&](double &x, double &y) {
        ++seq;
        block_sum2<TT>(x, y, sh[seq & 1u]);
    };
    double q = a.Q0[k], p = a.P0[k];
    if (tid == 0) {
        a.qmap[k] = q;
        a.pmap[k] = p;
    }
    int m = a.first;
    for (int i = 0; i + 1 < a.nm; ++i) {
        const KConst kc = kcs[m];
        auto rows = [&](double q, double P, double &r1, double &r2) {   // section m's Kstar(1,:).alpha, Kstar(2,:).alpha
            rd.template rows<FAM>(m, q, P, kc, r1, r2);
            sum2(r1, r2);
        };
        int it;
        map_step_inverse(a.mode, a.maxiter, a.tol, q, p, it, rows);
        if (--m < 0) m = a.nsec - 1;
        if (tid == 0) {
            a.qmap[(size_t)(i + 1) * a.ntest + k] = q;
            a.pmap[(size_t)(i + 1) * a.ntest + k] = p;
            if (a.iters) a.iters[(size_t)i * a.ntest + k] = it;
        }
    }
}

}  // namespace

// Workgroups per orbit: TWO 256-thread members per CU (512 slots) shared out among the ntest orbits, at most 16 per orbit, and no
// more than the training set can feed with a round of 256 points each -- the drivers' own sizes (20 - 80 points) keep one
// workgroup per orbit.  Two members of DIFFERENT orbits per CU is the point: a residual is ~3.5 us of VALU work per CU and ~5 us
// of reduction + exchange with the rest of the team, and with one 512-thread member per CU (the first form: 81 G pair
// evaluations per second at N0 = 16 384, Ntest = 37) the CU idles through the exchange; with two the other orbit computes.
// Every member of a team has to be resident at once (they wait for each other), so two workgroups must fit one CU: 2 waves per
// SIMD (<= 256 VGPRs; families A and D, the largest, have 142) and twice the kernel's LDS within the CU's 160 KB (2 x 72 328 B
// with MAP_STAGE 5; a sixth staged round would not fit).  tests/test_applymap_team_cpu.py holds every instance to this.
int applymap_team(int ntest, int n0)
{
    // resident workgroups the device can hold: two of these per CU (queried once per device; 256 CUs -> 512)
    static const int slots = [] {
        int dev = 0, ncu = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) {
            (void)hipGetLastError();
            return 0;                                    // unknown device: no teams (S = 1 needs no co-residency)
        }
        return 2 * ncu;
    }();
    int S = ntest > 0 ? slots / ntest : 1;
    S = std::min(S, (n0 + MAP_TEAM_T - 1) / MAP_TEAM_T);
    return std::max(1, std::min(S, MAP_TEAM_MAX));
}
size_t applymap_team_ws(int ntest, int n0)
{
    return ((size_t)ntest * applymap_team(ntest, n0) * 2 * 4 + 2) * sizeof(unsigned long long);    // granules + the error word
}

// team_ws: applymap_team_ws(ntest, n0) bytes of device scratch (cleared here)
int applymap(int family, int mode, int nm, int ntest, int n0, const double *xtr, const double *ytr,
             const KConst &kc, const double *alpha, int n0p, const double *xtrp, const double *ytrp,
             const KConst &kcp, const double *alphap, const double *Q0, const double *P0, double *qmap,
             double *pmap, double *pdiff, void *team_ws, hipStream_t st)
{
    if (nm <= 0 || ntest <= 0) return 0;
    const int S = applymap_team(ntest, n0);
    SGPR_HIP(hipMemsetAsync(team_ws, 0, applymap_team_ws(ntest, n0), st));
    unsigned long long *tw = static_cast<unsigned long long *>(team_ws);
    int *err = reinterpret_cast<int *>(tw + (size_t)ntest * S * 2 * 4);
    MapArgs a{nm, ntest, n0, n0p, mode, 60, S, tw, err, 1e-13, xtr, ytr, alpha, xtrp, ytrp, alphap, Q0, P0, qmap, pmap, pdiff, kc, kcp};
    return dispatch_family(family, [&](auto fam) {
        constexpr int F = decltype(fam)::value;
        if (S == 1) hipLaunchKernelGGL((applymap_kernel<F, MAP_T>), dim3(ntest), dim3(MAP_T), 0, st, a);
        else        hipLaunchKernelGGL((applymap_kernel<F, MAP_TEAM_T>), dim3(ntest * S), dim3(MAP_TEAM_T), 0, st, a);
        SGPR_CHECK_LAUNCH();
        return 0;
    });
}
static std::atomic<unsigned> g_last_map_calls{0};
unsigned applymap_last_calls() { return g_last_map_calls.load(); }    // measurement aid (libsympgpr_probe.so): K*-row evaluations of the last map

// after the stream has been waited for: did a team member give up on another (never a property of the data)?
int applymap_status(const void *team_ws, int ntest, int n0)
{
    const unsigned long long *tw = static_cast<const unsigned long long *>(team_ws);
    int hh[2] = {0, 0};
    SGPR_HIP(hipMemcpy(hh, tw + (size_t)ntest * applymap_team(ntest, n0) * 2 * 4, sizeof(hh), hipMemcpyDeviceToHost));
    g_last_map_calls.store((unsigned)hh[1]);
    const int h = hh[0];
    if (h) { set_error("applymap: a workgroup of an orbit's team did not answer in time"); return SGPR_E_HIP; }
    return 0;
}

// The sectioned maps: one launch, one 256-thread workgroup per orbit.  Dynamic LDS: exactly what is staged is reserved -- the
// drivers' size (4 sections of 70 points) takes 15.7 KB, not the 70 KB of the limit, so several orbits share a CU.
// The common arguments of the three kernels and, in `lds`, the bytes of dynamic LDS of the launch (0: nothing is staged).
static MapSecArgs mapsec_args(int mode, int nsec, int first, int nm, int ntest, int n0, const double *xtr, const double *ytr,
                              const double *alpha, int n0p, const double *xtrp, const double *ytrp, const double *alphap,
                              const double *Q0, const double *P0, double *qmap, double *pmap, double *pdiff, size_t &lds)
{
    const long need = (long)nsec * (4L * n0 + 3L * n0p);
    const bool staged = need <= MAPSEC_STAGE;
    lds = staged ? (size_t)need * sizeof(double) : 0;
    return MapSecArgs{nm, ntest, n0, n0p, mode, 60, nsec, first, staged ? 1 : 0, 1e-13, xtr, ytr, alpha, xtrp, ytrp, alphap, Q0, P0,
                      qmap, pmap, pdiff};
}
template <typename Kern, typename... Args>
static int mapsec_launch(Kern kern, int ntest, size_t lds, hipStream_t st, const Args &...args)
{
    if (lds > 48 * 1024)
        SGPR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(ntest), dim3(MAP_T), lds, st, args...);
    SGPR_CHECK_LAUNCH();
    return 0;
}

// Forwards.  jac [nm - 1][ntest][2][2], mono [ntest][2][2], lyap [ntest][2], each or null: with `tan` the launch is the TAN
// instance (same staging rule, same LDS, same orbit bits) and fills those of the three that are given.
int applymap_sections(int family, int mode, int nsec, int first, int nm, int ntest, int n0, const double *xtr, const double *ytr,
                      const double *alpha, const KConst *kcs, int n0p, const double *xtrp, const double *ytrp,
                      const double *alphap, const KConst *kcps, const double *Q0, const double *P0, double *qmap, double *pmap,
                      double *pdiff, hipStream_t st, bool tan, double *jac, double *mono, double *lyap)
{
    if (nm <= 0 || ntest <= 0) return 0;
    size_t lds;
    const MapSecTanArgs a{mapsec_args(mode, nsec, first, nm, ntest, n0, xtr, ytr, alpha, n0p, xtrp, ytrp, alphap, Q0, P0, qmap, pmap,
                                      pdiff, lds), jac, mono, lyap};
    return dispatch_family(family, [&](auto fam) {
        constexpr int F = decltype(fam)::value;
        if (tan) return mapsec_launch(applymap_sections_kernel<F, MAP_T, true>, ntest, lds, st, a, kcs, kcps);
        return mapsec_launch(applymap_sections_kernel<F, MAP_T, false>, ntest, lds, st, static_cast<const MapSecArgs &>(a), kcs, kcps);
    });
}

// Backwards.  No guess GPs, so a section takes 4 n0 doubles of the same MAPSEC_STAGE limit.
int applymap_sections_inverse(int family, int mode, int nsec, int first, int nm, int ntest, int n0, const double *xtr,
                              const double *ytr, const double *alpha, const KConst *kcs, const double *Q0, const double *P0,
                              double *qmap, double *pmap, int *iters, hipStream_t st)
{
    if (nm <= 0 || ntest <= 0) return 0;
    size_t lds;
    const MapSecInvArgs a{mapsec_args(mode, nsec, first, nm, ntest, n0, xtr, ytr, alpha, 0, nullptr, nullptr, nullptr, Q0, P0, qmap, pmap,
                                      nullptr, lds), iters};
    return dispatch_family(family, [&](auto fam) {
        return mapsec_launch(applymap_sections_inverse_kernel<decltype(fam)::value, MAP_T>, ntest, lds, st, a, kcs);
    });
}

}  // namespace sgpr
