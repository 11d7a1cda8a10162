// common.h -- internal declarations shared by the HIP translation units of libsympgpr_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/sympgpr_hip.h"

namespace sgpr {

void set_error(const std::string &msg);
// experiment knobs (capi.hip): built-in value unless set through libsympgpr_probe.so before first use
double tune(const char *name, double dflt);
void tune_set(const char *name, double v);
int hip_fail(hipError_t e, const char *what, const char *file, int line);

#define SGPR_HIP(call)                                                          \
    do {                                                                        \
        hipError_t e__ = (call);                                                \
        if (e__ != hipSuccess) return ::sgpr::hip_fail(e__, #call, __FILE__, __LINE__); \
    } while (0)

#define SGPR_CHECK_LAUNCH() SGPR_HIP(hipGetLastError())
#define SGPR_HIP_TYPES 1    // strassen.h: hipStream_t is declared

constexpr int MAX_DEVICES = 64;   // rows of every per-device table of the library (streams, events, queue state, Strassen scratch)
// the device that owns a stream (the null stream: the current device) as an index of the per-device tables, 0 .. MAX_DEVICES - 1; -1: the
// runtime refused (its error state is cleared; *err, where given, holds what it said) or the index is out of range
inline int device_of(hipStream_t st, hipError_t *err = nullptr)
{
    int dev = -1;
    const hipError_t e = st ? hipStreamGetDevice(st, &dev) : hipGetDevice(&dev);
    if (err) *err = e;
    if (e != hipSuccess) { (void)hipGetLastError(); return -1; }
    return (dev >= 0 && dev < MAX_DEVICES) ? dev : -1;
}

// Hyper-parameters split the way the reference does (`l = hyp[:-1]; sig = hyp[-1]`),
// plus the derived constants every Gram kernel uses.
struct KConst {
    double lx, ly, p, sig;
    double lx2, ly2;        // lx^2, ly^2
    double inv_lx2, inv_ly2;
    double cxx, cyy, cxy;   // sig*pp/lx^4, sig/ly^4, -sig*pm/(lx^2 ly^2)
    double hscale;          // 0.5 (family A/B) or p (family D); unused for C
    // length-scale derivatives (build_dK / build_dKreg)
    double inv_lx, inv_ly, inv_lx3, inv_ly3;
    double gxx;             // sig*pp: kxx = gxx (cos2h/lx^2 - sc^2/lx^4) E  (A/D),  gxx (1/lx^2 - u/lx^4) E  (C)
};
enum { DERIV_NONE = 0, DERIV_LX = 1, DERIV_LY = 2 };
int make_kconst(int family, const double *hyp, int nhyp, KConst *out);
bool family_has_p(int family);   // the family's hyp holds a period parameter p between the lengths and sig
int make_kconst_l(int family, const double *l, int nl, KConst *out);  // sig = 1

// f(std::integral_constant<int, family>()) for the kernel family chosen at run time (host side: gram.hip, map.hip)
template <typename F>
int dispatch_family(int family, F &&f)
{
    switch (family) {
    case SGPR_FAM_A: return f(std::integral_constant<int, SGPR_FAM_A>());
    case SGPR_FAM_B: return f(std::integral_constant<int, SGPR_FAM_B>());
    case SGPR_FAM_C: return f(std::integral_constant<int, SGPR_FAM_C>());
    case SGPR_FAM_D: return f(std::integral_constant<int, SGPR_FAM_D>());
    case SGPR_FAM_USER: return f(std::integral_constant<int, SGPR_FAM_USER>());
    }
    set_error("unknown kernel family");
    return SGPR_E_ARG;
}

// ---- gram.hip
int gram_pairs(int family, int mi, int mj, const double *xb, const double *yb, const double *xa,
               const double *ya, const KConst &kc, double *qq, double *Pq, double *qP, double *PP,
               size_t ld, long diag_off, double noise, unsigned flags, hipStream_t st);
int gram_reg(int family, int mi, int mj, const double *xb, const double *yb, const double *xa,
             const double *ya, const KConst &kc, double *G, size_t ld, long diag_off, double noise,
             hipStream_t st, int deriv = DERIV_NONE);
int kernel_eval(int family, int which, int m, const double *xa, const double *ya, const double *xb,
                const double *yb, const KConst &kc, double *out, hipStream_t st);
int predict_rows(int family, int m, const double *q, const double *P, int n0, const double *xtr,
                 const double *ytr, const KConst &kc, const double *alpha, double *out_p,
                 double *out_q, hipStream_t st);
int predict_reg(int family, int m, const double *q, const double *P, int n0, const double *xtr,
                const double *ytr, const KConst &kc, const double *alpha, double *out,
                hipStream_t st);

// ---- map.hip : the d = 1 symplectic map, every time step on the device
int applymap_team(int ntest, int n0);          // workgroups that share one orbit
size_t applymap_team_ws(int ntest, int n0);    // bytes of device scratch applymap needs
int applymap(int family, int mode, int nm, int ntest, int n0, const double *xtr, const double *ytr,
             const KConst &kc, const double *alpha, int n0p, const double *xtrp, const double *ytrp,
             const KConst &kcp, const double *alphap, const double *Q0, const double *P0, double *qmap,
             double *pmap, double *pdiff, void *team_ws, hipStream_t st);
int applymap_status(const void *team_ws, int ntest, int n0);
unsigned applymap_last_calls();                 // K*-row evaluations (all orbits) of the last applymap of this process   // after the stream has been waited for: SGPR_E_HIP if a team gave up
// the sectioned map (Split_SympGPR): step i uses section (first + i) mod nsec.  Device buffers: xtr / ytr n0 x nsec, alpha
// 2 n0 x nsec, the guess GPs' n0p x nsec, column-major and tight; kcs / kcps: nsec constants each, in device memory too
int applymap_sections(int family, int mode, int nsec, int first, int nm, int ntest, int n0, const double *xtr, const double *ytr,
                      const double *alpha, const KConst *kcs, int n0p, const double *xtrp, const double *ytrp,
                      const double *alphap, const KConst *kcps, const double *Q0, const double *P0, double *qmap, double *pmap,
                      double *pdiff, hipStream_t st, bool tan = false, double *jac = nullptr, double *mono = nullptr,
                      double *lyap = nullptr);
// `tan`: the same with the tangent map (mapsec_tan.h, tangent_core.h): jac [nm - 1][ntest][2][2], mono [ntest][2][2], lyap
// [ntest][2], each or null
// the sectioned map backwards: Q0 / P0 hold the images (Q, P), row i of qmap / pmap is the i-th preimage, step i undoes section
// (first - i) mod nsec; no guess GPs; iters [nm - 1][ntest] or null
int applymap_sections_inverse(int family, int mode, int nsec, int first, int nm, int ntest, int n0, const double *xtr,
                              const double *ytr, const double *alpha, const KConst *kcs, const double *Q0, const double *P0,
                              double *qmap, double *pmap, int *iters, hipStream_t st);

// ---- gram_nd.hip : d canonical pairs per point (X: points x 2d, column-major)
int gram_nd(int family, int d, int mi, int mj, const double *Xb, size_t ldxb, const double *Xa, size_t ldxa,
            const double *hyp, int nhyp, double *K, size_t ld, size_t rstride, size_t cstride, long diag_off,
            double noise, hipStream_t st);
int gram_nd_sel(int family, int d, int mi, int mj, const double *Xb, size_t ldxb, const double *Xa, size_t ldxa,
                const double *hyp, int nhyp, double *K, size_t ld, const long *roff, const long *coff, hipStream_t st);
int predict_nd(int family, int d, int m, const double *Xt, size_t ldxt, int n0, const double *Xtr, size_t ldxtr,
               const double *hyp, int nhyp, const double *alpha, double *out, hipStream_t st);
bool family_is_sum(int family);   // k = sum of the factors (family B, or a USER sum kernel): the explicit maps

// ---- map_nd.hip : the symplectic map of those fits, forwards, with its tangent map and backwards, and its periodic orbits
// nm steps of the d-pair symplectic map for ntest orbits, one workgroup per orbit (device buffers: Xtr n0 x 2d, alpha 2 d n0,
// Q0 / P0 ntest x d with leading dimension ntest, qmap / pmap [nm][ntest][d], iters [nm - 1][ntest] or null)
int applymap_nd(int family, int d, int mode, int nm, int ntest, int n0, const double *Xtr, size_t ldxtr, const double *hyp,
                int nhyp, const double *alpha, const double *Q0, const double *P0, double *qmap, double *pmap, int *iters,
                hipStream_t st);
// the backward orbit with the same buffers: Q0 / P0 hold the images (Q, P), row i of qmap / pmap is the i-th preimage
int applymap_nd_inverse(int family, int d, int mode, int nm, int ntest, int n0, const double *Xtr, size_t ldxtr, const double *hyp,
                        int nhyp, const double *alpha, const double *Q0, const double *P0, double *qmap, double *pmap, int *iters,
                        hipStream_t st);
// the same with the tangent map (maptan.h): jac [nm - 1][ntest][2d][2d], mono [ntest][2d][2d], lyap [ntest][2d], each or null
int applymap_nd_tangent(int family, int d, int mode, int nm, int ntest, int n0, const double *Xtr, size_t ldxtr, const double *hyp,
                        int nhyp, const double *alpha, const double *Q0, const double *P0, double *qmap, double *pmap, int *iters,
                        double *jac, double *mono, double *lyap, hipStream_t st);
// periodic orbits of that map (periodic_nd.h): Newton on the n-fold map from the guesses Q0 / P0 with the winding numbers wind
// (ntest x d ints, leading dimension ntest, or null), all passes in one launch; z [ntest][2d], resid [ntest], its [ntest], mono
// [ntest][2d][2d] or null, qorb / porb [n][ntest][d] or both null
int periodic_nd(int family, int d, int mode, int n, int ntest, int n0, const double *Xtr, size_t ldxtr, const double *hyp, int nhyp,
                const double *alpha, const int *wind, const double *Q0, const double *P0, double tol, int maxit, double *z,
                double *resid, int *its, double *mono, double *qorb, double *porb, hipStream_t st);

// ---- genfun_nd.hip : the generating function of those fits
// the generating function F itself at m device-resident test points (has_ref: row m of Xt is a reference point, F has m + 1
// entries and F[t] := F(x_t) - F(x_0)); one chunk of its variance: the cross-covariance columns V (2 d n0 x mc) and the prior
int genfun_nd(int family, int d, int m, const double *Xt, size_t ldxt, bool has_ref, int n0, const double *Xtr, size_t ldxtr,
              const double *hyp, int nhyp, const double *alpha, double *F, hipStream_t st);
int genfun_cross_nd(int family, int d, int mc, const double *Xt, size_t ldxt, const double *x0, size_t ldx0, int n0,
                    const double *Xtr, size_t ldxtr, const double *hyp, int nhyp, double *V, size_t ldv, double *prior,
                    size_t prior_stride, hipStream_t st);

// ---- gemm_f64.hip : C = beta C + alpha A B^T on fp64 MFMA tiles
int gemm_nt(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B,
            size_t ldb, double beta, double *C, size_t ldc, int lower, long diag_off,
            hipStream_t st);
int gemm_nt_bc(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B,
               size_t ldb, double beta, double *C, size_t ldc, int lower, const int *bc5,
               hipStream_t st);
int gemm_nn(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb,
            double beta, double *C, size_t ldc, hipStream_t st);
// two destinations from one product: C = beta C + alpha A B^T, C2 += alpha2 A B^T
int gemm_nt_two(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb, double beta,
             double *C, size_t ldc, double alpha2, double *C2, size_t ldc2, hipStream_t st);
// up to four destinations from one product (disjoint blocks): C[0] = beta C[0] + alpha[0] A B^T, C[d] += alpha[d] A B^T
int gemm_nt_multi(int m, int n, int k, const double *A, size_t lda, const double *B, size_t ldb, double beta, int count,
                  double *const *C, const size_t *ldc, const double *alpha, hipStream_t st);
int gemm_profile_begin();
int gemm_profile_end(double *out12);
int gemm_profile_launches(double *buf, int max_records);
void gemm_set_overlap(int on);   // look-ahead driver: launches from here on share the device (thread-local)
// diagnostics (libsympgpr_probe.so only): per-workgroup clock stamps, tile-shape / staging switches
int gemm_nt_diag(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb,
                 double beta, double *C, size_t ldc, int lower, unsigned long long *stamps, int dbg, hipStream_t st);

// ---- chol.hip : recursion, look-ahead driver, potrf(), the batched panels (kernels: panel.hip; host arithmetic: chol_plan.hip)
constexpr int LEAF = 128;  // order of the diagonal block factored in LDS by one workgroup
// value left in *dinfo when a hand-off inside the persistent panel kernel timed out (a bug or a
// device problem, never a property of the matrix); info_status() turns it into SGPR_E_HIP
constexpr int POTRF_HANDOFF_TIMEOUT = -1000001;
constexpr int SOLVE_HANDOFF_TIMEOUT = -1000002;   // the same for the strip solves of a batch (batch.hip)
inline int info_status(int info)
{
    if (info >= 0) return info;
    set_error(info == POTRF_HANDOFF_TIMEOUT ? "potrf: a hand-off inside the panel kernel timed out"
              : info == SOLVE_HANDOFF_TIMEOUT ? "solve: a hand-off between the strips of a triangular solve timed out" : "potrf: internal error");
    return SGPR_E_HIP;
}
size_t potrf_workspace(int n);
int potrf(int n, double *A, size_t lda, void *work, size_t lwork, int *dinfo, hipStream_t st);
// batch.hip's mid-size path: nbatch factorisations of order npad (multiple of 128, <= potrf_batch_max_order()) in one launch
size_t potrf_batch_flag_bytes(int nbatch);
int potrf_batch_max_order();
int leaf_probe(double *A, size_t lda, double *inv, int *dinfo, unsigned long long *stamps, hipStream_t st);
int potrf_batch(int nbatch, int npad, double *A, size_t stride_a, size_t lda, double *inv, size_t stride_inv, int *flags,
                int *info, hipStream_t st);
// one panel (columns k0 .. k0 + 128 Wd, rows down to npad) of every problem; flags: potrf_batch_flag_bytes(nbatch) bytes per call
int potrf_batch_panel(int nbatch, int npad, int k0, int Wd, double *A, size_t stride_a, size_t lda, double *inv, size_t stride_inv,
                      int *flags, int *info, hipStream_t st);
// ---- cholq.hip
bool potrf_queue_mark_failed(hipStream_t st);   // a queue factorisation gave up: the look-ahead driver from now on (true: the queue was in use)
// ---- streams.hip
int release_device_streams(int dev);   // drain + destroy the streams potrf created on `dev` (they come back on demand)
// ---- solve.hip : the triangular solves against a factor (its leaf inverses in `work`)
int trsm_rlt(int m, int n, const double *L, size_t ldl, double *B, size_t ldb, const void *work,
             hipStream_t st);
// One-right-hand-side solves keep their hand-off words (tickets, progress, the published segments) IN the workspace: one
// solve per workspace at a time (two solves against one factor from two streams need two copies of the workspace).
int potrs_vec(int n, const double *L, size_t ldl, void *work, double *b, hipStream_t st);
int solve_status(int n, const double *L, size_t ldl, const void *work, hipStream_t st);   // syncs st; SGPR_E_HIP if a strip solve gave up
int trsm_rl(int m, int n, const double *L, size_t ldl, double *B, size_t ldb, const void *work, hipStream_t st);  // B := B L^-1
// the same two against the trailing block L[off:, off:] (L points at it, n its order, off a multiple of 128)
int trsm_rlt_off(int m, int n, const double *L, size_t ldl, double *B, size_t ldb, const void *work, int off, hipStream_t st);
int trsm_rl_off(int m, int n, const double *L, size_t ldl, double *B, size_t ldb, const void *work, int off, hipStream_t st);
int potrs_mat(int n, const double *L, size_t ldl, const void *work, double *B, size_t ldb, int nrhs, double *scratch,
              hipStream_t st);  // B (n x nrhs) := L^-T L^-1 B; scratch: potrs_mat_scratch(n, nrhs, L, ldl) bytes
int potrs_mat_fwd(int n, const double *L, size_t ldl, const void *work, double *B, size_t ldb, int nrhs, double *scratch,
                  hipStream_t st);  // B := L^-1 B (the forward half of potrs_mat, same path, same scratch)
size_t potrs_mat_scratch(int n, int nrhs, const double *L, size_t ldl);
bool potrs_mat_uses_strips(int n, int nrhs, const double *L, size_t ldl);   // the one-launch block solves of trsm.hip (hand-off words in `work`: solve_status)
int trsv(int n, const double *L, size_t ldl, void *work, double *b, int trans, hipStream_t st);
bool trsv_uses_strips(int n, const double *L, size_t ldl);      // potrs_vec / trsv take the one-launch strip kernels
const int *trsv_state(int n, const void *work);                 // their 8 state words: [2], [6] != 0 = a hand-off timed out
int leaf_inverses(int n, const double *L, size_t ldl, void *work, int *dinfo, hipStream_t st);

// ---- trsv.hip : one-right-hand-side triangular solve as one launch (strips + progress counter)
bool trsv_strips_ok(int n, const double *L, size_t ldl);
int trsv_strips(int n, const double *L, size_t ldl, const double *inv, double *b, int trans, int *state /* 4 ints, zero */,
                double *pub /* n doubles, all bytes 0xFF */, hipStream_t st);
// `nbatch` independent systems of one order in one launch: problem p at L + p sL, inv + p sInv, b / pub + p sB, state + p sState
int trsv_strips_batch(int nbatch, int n, const double *L, size_t sL, size_t ldl, const double *inv, size_t sInv, double *b, size_t sB,
                      int trans, int *state, int sState, double *pub, hipStream_t st);

// ---- trsm.hip : triangular solves with a block of right-hand sides, one launch per solve (strips + progress counter)
constexpr int TRSM_YLD = 80;                                      // row stride of the right-hand-side images [k][64 + 16]
constexpr int TRSM_FOLD = 5;                                      // tiles next to the diagonal folded into the leaf inverse
constexpr int TRSM_STATE_INTS = 16;                               // hand-off words of one forward + backward pair
bool trsm_strips_ok(int n, const double *L, size_t ldl);
void trsm_piece_of(int u, int C, int T, int out[5]);                      // the stream tickets as the host sees them (tests)
void trsm_piece_counts(int T, int C, size_t out[2]);
size_t trsm_strips_scratch(int n);                                // bytes
int potrs_strips(int n, const double *L, size_t ldl, const double *inv, double *B, size_t ldb, int nrhs, int *state /* TRSM_STATE_INTS ints */,
                 double *scratch, hipStream_t st);
int trsm_strips_fwd(int n, const double *L, size_t ldl, const double *inv, double *B, size_t ldb, int nrhs, int *state,
                    double *scratch, hipStream_t st);   // B := L^-1 B: potrs_strips' passes without the backward launch

// ---- postcov.hip : posterior covariance blocks from V = L^-1 K*^T (two-stage deterministic reduction)
constexpr int POSTCOV_COLS = 256;                                 // right-hand-side columns of one chunk at most
size_t postcov_partial_doubles(int n, int D, int mc);             // stage-1 scratch of a chunk of mc points
int postcov(int D, int n, int mc, const double *V, size_t ldv, const double *Kss, size_t ldk, double *part, double *cov,
            hipStream_t st);

// ---- nllgrad.hip : the NLL gradient in all hyperparameters from Ky^-1 by row panels (sgpr_fit_nll_grad_full)
size_t nll_grad_full_scratch(int n, int N, int nacc);             // bytes: one panel of Ky^-1 + the partial sums
int nll_grad_full(int family, int d, bool reg, int N, int n, const double *L, size_t ldl, const void *work, const double *X,
                  const double *alpha, const double *l, const double *pp, int nacc, double *scratch, double *out,
                  hipStream_t st);

// a row panel of Ky^-1 from the cached factor: memset, identity, the two recursive panel solves on L[J:, J:]
int kyinv_panel_width(int n, const char *knob);                   // 2048 rows up to n = 8192, 4096 above; tunable `knob` overrides
int kyinv_row_panel(int n, int J, int rows, const double *L, size_t ldl, const void *work, double *R, size_t ldr, hipStream_t st);

// the contraction for loograd.hip: the workgroups of one panel of ldr rows; one launch with the rank-2 weight
// Mp - (beta alpha^T + alpha beta^T) on Mp = M[J:J+rows, J:] (partials as nll_grad_full's, workgroup wg0 on); the fold
size_t grad_contract_wgs(int ldr, int N);
int grad_contract_rank2(int family, int d, bool reg, int N, int J, int rows, const double *Mp, size_t ldr, const double *alpha,
                        const double *beta, const double *X, const double *l, const double *pp, double *part, size_t nwg,
                        size_t wg0, hipStream_t st);
int grad_fold(const double *part, size_t nwg, int nacc, double *out, hipStream_t st);   // out[k] = sum_w part[k nwg + w]

// ---- loo.hip : leave-one-point-out cross-validation of a solved fit from the same row panels (sgpr_fit_loo)
struct LooLayout { size_t panel, blocks, part, resid, cov, lpd, sums, total; };   // offsets in doubles into the scratch
LooLayout loo_layout(int n, int N, int D);
// D = 2d (pair fits, d = 1 .. 3) or 1 (reg); scratch: loo_layout(n, N, D).total doubles.  Leaves {loo, press} at
// scratch + sums, the residuals (n, the layout of z) at + resid, the covariances (N x D x D) at + cov, lpd (N) at + lpd.
int fit_loo(int D, int N, int n, const double *L, size_t ldl, const void *work, const double *alpha, double *scratch,
            hipStream_t st);

// ---- loograd.hip : the gradient of loo / press in all hyperparameters from the dense Ky^-1 (sgpr_fit_loo_grad)
struct LooGradLayout {   // offsets in doubles into the scratch; nb / ldr: the rows of a panel of M and its leading dimension
    size_t kinv, y, panel, w, v, beta, part, part_obj, sums, total, nwg, nwg_points;
    int nb, ldr;
};
LooGradLayout loo_grad_layout(int n, int N, int D, int nacc);
// scratch: loo_grad_layout(...).total doubles.  Leaves the nacc raw sums of nll_grad_full's layout at scratch + sums and the
// objective's raw sum (sum lpd = -loo, or press) behind them; the caller scales them.  `work`: the factor's workspace (potrs_vec)
int fit_loo_grad(int family, int d, bool reg, int which, int N, int n, const double *L, size_t ldl, void *work, const double *X,
                 const double *alpha, const double *l, const double *pp, int nacc, double *scratch, hipStream_t st);

// ---- batch.hip : many small fits (order <= 256 each) in one launch, one workgroup per problem
int fit_batch_max_order();
int fit_batch_trim();                            // release the calling thread's batch arena (device + pinned host)
int potrf_trim();                                // ... and its pooled events
// The arena layout of one batched call: byte offsets into its input block (one H2D copy), its output block (one D2H copy) and the
// device scratch behind them, every region a multiple of 256 bytes.  Host arithmetic only, no device call.  mid: the path of orders
// above 256 (in chunks of problems), else the one-launch path (one chunk); mode: 0 fit, 1 nll gradient, 2 loo, 3 loo gradient;
// d: 0 for points as x | y, else the canonical pairs per point.
struct BatchLayout {
    int chunk;                                       // problems per pass over the arena
    int npad, W, ggx, ggy, lnwg;                     // mid path: padded order, 128-strips, contraction grid, loo workgroups per problem
    size_t nacc;                                     // doubles behind nll per problem (raw sums)
    size_t const_bytes, flag_bytes;                  // per-problem constants; potrf_batch_flag_bytes(chunk) (mid path)
    size_t o_x, o_y, o_z, o_kc, o_no, in_bytes;      // x | y | z | consts | noise
    size_t o_al, o_nll, o_info, out_bytes;           // alpha | nll [+ sums] | info
    size_t o_A, o_inv, o_fl, o_fl2, o_r, o_pub, o_st, o_part, scr_bytes;     // mid path's scratch regions; the total of either path
    size_t o_lpart, o_wt, o_v, o_beta, o_zero;       // mid path's loo gradient: the point pass's partials, W~, v, beta, zeros (behind o_part)
};
BatchLayout batch_layout(int mid, int mode, int d, int reg, int nbatch, int npts, int nhyp);

// One batched call, as the C entries (capi.hip) describe it and the drivers take it.  The mode is the set of outputs asked for: grad
// (nbatch x (nhyp + 1)) the nll gradient, loo (nbatch x 2) the {loo, press} rows, value (nbatch) beside grad the loo objective
// `which` (SGPR_LOO_LPD / SGPR_LOO_PRESS) and its gradient, rows in sgpr_fit_nll_grad_full's order.
enum { MODE_FIT = 0, MODE_GRAD = 1, MODE_LOO = 2, MODE_LOOGRAD = 3 };
struct BatchCall {
    int family, d, reg, nbatch, npts, n, nhyp;      // d = 0: points as x | y; d > 0: d canonical pairs per point, x = X (nbatch x 2d x npts)
    const double *x, *y, *z, *hyp, *sig2n;
    double *alpha, *nll;                            // alpha may be null
    int *info;
    double *grad, *loo, *value;
    int which;
    int mode() const { return value ? MODE_LOOGRAD : grad ? MODE_GRAD : loo ? MODE_LOO : MODE_FIT; }
};
// The one driver: the one-launch path up to fit_batch_grad_max_order(), the mid path above.  The arguments have been checked and
// nbatch > 0.  The order decides alone because check_batch_args (capi.hip) has held every entry to its own range before the call
// -- above fit_batch_grad_max_order() for the _mid entries, at most that for the one-launch gradients, up to fit_batch_max_order()
// for the rest -- so this choice is the one each entry used to make for itself.
int fit_batch_run(const BatchCall &c);
int fit_batch_grad_max_order();                  // 256: one workgroup holds the whole problem

// the raw sums of a gradient (nll_grad_full's layout: lengths, periods, sig, sig2n) into the gradient: the lengths and periods by
// sig / 2 (the kernels differentiate k without sig), sig by 1/2, sig2n by sign(sig2n) / 2
inline void scale_grad_sums(const double *raw, int nhyp, double sig, double sig2n, double *grad)
{
    for (int k = 0; k < nhyp - 1; ++k) grad[k] = 0.5 * sig * raw[k];
    grad[nhyp - 1] = 0.5 * raw[nhyp - 1];
    grad[nhyp] = (sig2n < 0.0 ? -0.5 : 0.5) * raw[nhyp];
}

// ---- blas_small.hip
int zero_strict_upper(int n, double *A, size_t lda, hipStream_t st);
int sym_fill_upper(int n, double *A, size_t lda, hipStream_t st);
int nll_reduce(int n, const double *L, size_t ldl, const double *z, const double *alpha,
               double *dout /* [0]=0.5 z.alpha + sum log diag */, hipStream_t st);
int copy_diag(int n, const double *A, size_t lda, double *d, hipStream_t st);
int dot(int n, const double *a, const double *b, double *out, hipStream_t st);      // out[0] = a.b
constexpr int SUMSQ_SCRATCH = 1024;
// ---- eig.hip
int syev_jacobi(int n, double *A, size_t lda, double *V, size_t ldv, double *w_host, int max_sweeps,
                int *sweeps_done, hipStream_t st);
int sumsq(size_t count, const double *a, double *part, double *out, hipStream_t st);
int trace(int n, const double *A, size_t lda, double *out, hipStream_t st);          // out[0] = sum A_ii
int transpose(int m, int n, const double *A, size_t lda, double *B, size_t ldb, hipStream_t st);
int gemv_n_sub(int m, int k, const double *A, size_t lda, const double *x, double *y,
               hipStream_t st);  // y(m) -= A(m x k) x(k)
int gemv_t_sub(int m, int k, const double *A, size_t lda, const double *x, double *y,
               hipStream_t st);  // y(k) -= A(m x k)^T x(m)

}  // namespace sgpr
