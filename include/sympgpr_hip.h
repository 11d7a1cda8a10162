/*
 * sympgpr_hip.h -- C ABI of libsympgpr_hip.so, the MI355X (gfx950) implementation of
 * SympGPR's GP training core.  Plain C: pointers, sizes, ints; no torch / C++ types.
 *
 * This is the drop-in boundary for the ONE hot path of redmod-team/SympGPR:
 *   build_K / buildKreg            (python/05_tokamak/SympGPR/sympgpr.f90:12-60, the f2py
 *                                   object `sympgpr.build_k`, `sympgpr.buildkreg` that
 *                                   python/functions/func.py:40,50 calls)
 *   Ky = K + |sig2n| I             (python/functions/func.py:183,192)
 *   L  = cholesky(Ky, lower=True)  (python/functions/func.py:166,184,193 -> LAPACK dpotrf)
 *   alpha = L^-T L^-1 y            (python/functions/func.py:174-177       -> LAPACK dtrtrs x2)
 *   nll = y.alpha/2 + sum log L_ii (python/functions/func.py:186,195)
 *   K* rows . alpha                (sympgpr.f90:62-86,112-124: guessP / calcq / calcP target)
 * The reference-side binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - fp64, column-major (Fortran order), leading dimensions in elements.
 *   - `family`: SGPR_FAM_* selects the generated scalar-kernel file of the reference.
 *   - `hyp` / `nhyp`: the reference's hyper-parameter vector: (lx, ly, sig) for A/B/C
 *     (sympgpr.f90:17), (lx, ly, p, sig) for D
 *     (01_pendulum/implicit_period_unknown/func.py:18-19,45-46).  K is scaled by sig.
 *   - return value: 0 = ok; < 0 = SGPR_E_* (argument / HIP error, text via
 *     sgpr_last_error()); > 0 = LAPACK-style info "leading minor of order k is not positive
 *     definite" (the Python layer maps it to numpy.linalg.LinAlgError like SciPy does).
 *   - `*_host` calls take caller-owned host buffers and stage through HBM; `*_dev` calls
 *     take device pointers (hipMalloc / torch tensors) and a hipStream_t passed as void*.
 *   - There is NO CPU fallback: without a usable gfx950 device every compute call
 *     returns SGPR_E_NODEVICE.
 *   - Argument errors (bad extents, leading dimensions, null pointers) of the `*_dev` primitives are
 *     reported as SGPR_E_ARG before any device is looked for, so before SGPR_E_NODEVICE; the message
 *     names the entry point.
 */
#ifndef SYMPGPR_HIP_H
#define SYMPGPR_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SGPR_ABI_VERSION 5   /* 2: solves take a writable workspace, sgpr_solve_status_dev, 12 / 7-double profile records, probes in their own library;
                                3: sgpr_fit_solve_rhs_ms, sgpr_potrf_info_dev, sgpr_trim (entry points added, none changed);
                                4: sgpr_fit_solve_rhs_dev (added);
                                5: sgpr_fit_cond_estimate, sgpr_fit_trim, sgpr_gemm_nn_dev, sgpr_trsm_rl_dev, sgpr_copy_blocks_dev (added) */

enum { SGPR_FAM_A = 0,   /* periodic(q) x SE(P), product : 05_tokamak/SympGPR/kernels.f90      */
       SGPR_FAM_B = 1,   /* periodic(q) + SE(P), sum     : 01_pendulum/explicit/kernels_sum.f90 */
       SGPR_FAM_C = 2,   /* SE x SE                      : 03_henon_heiles/kernels_sq.f90        */
       SGPR_FAM_D = 3,   /* periodic, free period p      : 01_pendulum/implicit_period_unknown/kernels.f90 */
       SGPR_FAM_USER = 4 }; /* the user's kernel: GENERATED code only (tools/gen_kernels.py, USER_FAMILY; the step the
                               reference performs with init_func.py:24-81).  As shipped: SE x SE a second time. */

/* 1 when the family's hyper-parameter vector carries a period p between the lengths and sig -- family D, or a user kernel
 * whose definition uses p: hyp = (lx, ly, p, sig), for d > 1 (lq_1..lq_d, lP_1..lP_d, p_1..p_d, sig); else 0 */
int sgpr_family_has_p(int family);

/* `which` of sgpr_kernel_eval: the four functions of a kernels*.f90 that enter K */
enum { SGPR_K_KERN = 0, SGPR_K_DXDX0 = 1, SGPR_K_DYDY0 = 2, SGPR_K_DXDY0 = 3,
       /* OR-ed in: the derivative of that function with respect to lx / ly (dkdlx_num,
        * d3kdxdx0dlx_num, ... kernels.f90:133-231; product kernels only) */
       SGPR_K_DLX = 4, SGPR_K_DLY = 8,
       /* the seven generated functions no caller of the reference uses (kernels.f90:12-57,95-132):
        * dkdx, dkdy, dkdx0, dkdy0, d3kdxdx0dy0, d3kdydy0dy0, d3kdxdy0dy0 */
       SGPR_K_DX = 16, SGPR_K_DY = 17, SGPR_K_DX0 = 18, SGPR_K_DY0 = 19, SGPR_K_DXDX0DY0 = 20,
       SGPR_K_DYDY0DY0 = 21, SGPR_K_DXDY0DY0 = 22 };

enum { SGPR_E_ARG = -1, SGPR_E_NODEVICE = -2, SGPR_E_HIP = -3, SGPR_E_NOMEM = -4,
       SGPR_E_STATE = -5 };

/* Gram-build part selection / options (sgpr_gram_pairs_dev `flags`) */
enum { SGPR_G_QQ = 1, SGPR_G_PQ = 2, SGPR_G_QP = 4, SGPR_G_PP = 8, SGPR_G_ALL = 15,
       SGPR_G_LOWER = 16,     /* write qq / PP tiles only where they touch row >= col; skip qP */
       SGPR_G_OCML = 32,      /* use the ROCm device-libs exp/sincos instead of the in-house ones */
       SGPR_G_DLX = 64,       /* entries of dK/dlx instead of K (build_dK, functions/func.py:80-129) */
       SGPR_G_DLY = 128 };    /* entries of dK/dly                                                  */

/* fit flags */
enum { SGPR_FIT_LOWER_ONLY = 1,  /* build only the lower triangle (what the factor reads)   */
       SGPR_FIT_REG = 4,         /* scalar-kernel GP (buildKreg, n = n_pts): nll_chol_reg     */
       SGPR_FIT_BLOCK_QQ = 8,    /* only the qq block of build_K (n = n_pts): nll_expl ind=0,  */
       SGPR_FIT_BLOCK_PP = 16 }; /* only the PP block, ind=1 (04_standard_map/func.py:126-141) */

int sgpr_abi_version(void);
const char *sgpr_last_error(void);
/* number of usable HIP devices (0 if none); never fails */
int sgpr_device_count(void);
/* select the device used by this thread's subsequent calls (default 0) */
int sgpr_set_device(int dev);

/* ---- stateless host-buffer calls: mirror the f2py object --------------------------------- */

/* sympgpr.build_k(x, y, x0, y0, hyp, K): K is (2n x 2n0), in/out, column-major.
 * replaces python/05_tokamak/SympGPR/sympgpr.f90:12-38 */
int sgpr_build_k_host(int family, int n, int n0, const double *x, const double *y,
                      const double *x0, const double *y0, const double *hyp, int nhyp,
                      double *K, size_t ldk);
/* sympgpr.buildkreg(x, y, x0, y0, hyp, K): K is (n x n0).  replaces sympgpr.f90:40-60 */
int sgpr_buildkreg_host(int family, int n, int n0, const double *x, const double *y,
                        const double *x0, const double *y0, const double *hyp, int nhyp,
                        double *K, size_t ldk);
/* d canonical pairs per point (BASELINE configs d = 2, 3; SURVEY.md 8 preamble): X (n x 2d), X0
 * (n0 x 2d) column-major, one column per coordinate (q_1..q_d, P_1..P_d), hyp = (lq_1..lq_d,
 * lP_1..lP_d, sig) -- (lq.., lP.., p_1..p_d, sig) for family D.  K is (2 d n x 2 d n0): block (a, b) =
 * sig d^2 k / dx_a dx'_b at rows a n, columns b n0, for the product kernel of family A (periodic q's),
 * C (all SE) or D (a free period per q), or the sum kernel B (only the diagonal blocks are non-zero).
 * d = 1 is sgpr_build_k_host entry for entry; d > 1 has no counterpart in the reference. */
int sgpr_build_k_nd_host(int family, int d, int n, int n0, const double *X, size_t ldx,
                         const double *X0, size_t ldx0, const double *hyp, int nhyp, double *K,
                         size_t ldk);
/* kernels.<name>_num, batched: out[i] = f(xa[i], ya[i], xb[i], yb[i], l...).  `l` holds
 * (lx, ly) or (lx, ly, p).  replaces the f2py `kernels` module (kernels.f90:1-94) */
int sgpr_kernel_eval_host(int family, int which, int m, const double *xa, const double *ya,
                          const double *xb, const double *yb, const double *l, int nl,
                          double *out);
/* build_dK(xin, x0in, hyp)[which] (functions/func.py:80-129; which = 0: d/dlx, 1: d/dly):
 * dK is (2 n0 x 2 n), rows index the "0" points.  Families A, C, D. */
int sgpr_build_dk_host(int family, int which, int n, int n0, const double *x, const double *y,
                       const double *x0, const double *y0, const double *hyp, int nhyp, double *dK,
                       size_t ld);
/* build_dKreg(xin, x0in, hyp)[which] (functions/func.py:52-78): dK is (n x n0) */
int sgpr_build_dkreg_host(int family, int which, int n, int n0, const double *x, const double *y,
                          const double *x0, const double *y0, const double *hyp, int nhyp, double *dK,
                          size_t ld);
/* scipy.linalg.cholesky(A, lower=True) (func.py:166): in place, strict upper zeroed. */
int sgpr_potrf_host(int n, double *A, size_t lda);
/* solve_cholesky(L, B) (func.py:174-177): B (n x nrhs) overwritten by L^-T L^-1 B. */
int sgpr_potrs_host(int n, const double *L, size_t ldl, double *B, size_t ldb, int nrhs);
/* LAPACK dsyev('V','L')-shaped: A (n x n column-major host buffer, lower triangle read) is
 * overwritten by the eigenvectors, w (n) gets the eigenvalues ascending -- the dense equivalent
 * of the drivers' `eigsh(Ky, neig)` fallback (02_pert_pendulum/func.py:199). */
int sgpr_syev_host(int n, double *A, size_t lda, double *w);

/* ---- device-resident fit: the whole nll_chol path without K ever leaving HBM --------------
 * replaces python/functions/func.py:189-196 (nll_chol) / :165-171 (gpsolve) on (x, x). */
typedef struct sgpr_fit *sgpr_fit_t;
/* What a handle holds, and what every entry below needs of it (tests/test_gpu_fit_lifecycle.py keeps this as a table).
 * Three things can be valid: Ky ("built": sgpr_fit_build), the factor L in Ky's place ("factored": sgpr_fit_factor, which
 * ends "built") and alpha with the NLL ("solved": sgpr_fit_solve).  sgpr_fit_set_hyp ends all three, sgpr_fit_set_targets
 * ends "solved" only (the factor does not depend on z: sgpr_fit_solve alone refits), sgpr_fit_build ends "factored" and
 * "solved", a factorisation that fails (info > 0) leaves nothing valid, and neither does sgpr_fit_eig, which overwrites the
 * matrix with eigenvectors.
 *   any state:      set_hyp, set_targets, build, run, eig, trim, stage_ms, solve_rhs_ms (-1 for a stage that has not run),
 *                   device_ptrs, destroy
 *   needs built:    factor;  get_matrix takes built or factored
 *   needs factored: solve, ldiag, solve_rhs, solve_rhs_dev, inverse, cond_estimate
 *   needs solved:   alpha, nll, predict_rows, predict_nd, predict_cov, predict_genfun, nll_grad, nll_grad_terms,
 *                   nll_grad_full, loo, applymap_nd, applymap_nd_tangent, applymap_nd_inverse, periodic_nd
 *                   loo_grad (as nll_grad_full: SGPR_FIT_BLOCK_QQ / _PP fits refused; grows the fit's scratch block)
 * An entry called without what it needs returns SGPR_E_STATE.  So does one called on a kind of fit it is not defined for:
 *   SGPR_FIT_BLOCK_QQ / _PP fits: every "needs solved" entry except alpha and nll, and cond_estimate;
 *   SGPR_FIT_REG fits: predict_nd, applymap_nd, applymap_nd_tangent, applymap_nd_inverse, periodic_nd (predict_genfun: SGPR_E_ARG, see there);
 *   create_nd fits with d > 1: predict_rows, nll_grad, nll_grad_terms.
 * Argument errors (SGPR_E_ARG) are reported first.  Every refusal happens before any device call and leaves the handle, the
 * device buffers and the scratch as they were; its message (sgpr_last_error) begins with the entry's name without "sgpr_"
 * -- "fit_alpha: not solved".  Apart from the stage and scratch changes named with each entry, the "needs factored" and
 * "needs solved" entries only read the handle: their results do not depend on which of them ran before, in which order,
 * or on sgpr_fit_trim / sgpr_trim in between.  (sgpr_fit_get_matrix completes the matrix in place -- the upper triangle of
 * a SGPR_FIT_LOWER_ONLY Ky filled, the strict upper triangle of L zeroed --, which no other entry reads.) */

/* Allocates HBM for an n = 2*n_pts order system (n = n_pts with SGPR_FIT_REG) and uploads
 * x, y (n_pts each), z (n). */
int sgpr_fit_create(int family, int n_pts, const double *x, const double *y, const double *z,
                    const double *hyp, int nhyp, double sig2n, unsigned flags, void *stream,
                    sgpr_fit_t *out);
/* the same fit for d canonical pairs per point: X (n_pts x 2d), z (2 d n_pts), order n = 2 d n_pts */
int sgpr_fit_create_nd(int family, int d, int n_pts, const double *X, size_t ldx, const double *z,
                       const double *hyp, int nhyp, double sig2n, unsigned flags, void *stream,
                       sgpr_fit_t *out);
/* new hyper-parameters / targets for the next run (the optimiser loop of the drivers,
 * 01_pendulum/implicit/main.py:146-151, calls the path ~100x with fixed x) */
int sgpr_fit_set_hyp(sgpr_fit_t f, const double *hyp, int nhyp, double sig2n);
int sgpr_fit_set_targets(sgpr_fit_t f, const double *z);
/* individual stages (asynchronous on the fit's stream) */
int sgpr_fit_build(sgpr_fit_t f);   /* Ky = build_K(x,x) + |sig2n| I                         */
int sgpr_fit_factor(sgpr_fit_t f);  /* L in place; returns info > 0 when not PD (this syncs)  */
int sgpr_fit_solve(sgpr_fit_t f);   /* alpha = L^-T L^-1 z ; nll                              */
/* all three; returns the factor's info */
int sgpr_fit_run(sgpr_fit_t f);
int sgpr_fit_alpha(sgpr_fit_t f, double *alpha_out /* 2*n_pts, host */);
int sgpr_fit_nll(sgpr_fit_t f, double *nll_out);
int sgpr_fit_ldiag(sgpr_fit_t f, double *diag_out /* 2*n_pts, host */);
/* copy the factor (lower, strict upper zeroed) / the matrix as built to a host buffer */
int sgpr_fit_get_matrix(sgpr_fit_t f, double *A, size_t lda);
/* extra right-hand sides with the cached factor: B (n x nrhs, host) overwritten */
int sgpr_fit_solve_rhs(sgpr_fit_t f, double *B, size_t ldb, int nrhs);
/* the same for right-hand sides that already live on the fit's device (n x nrhs, column-major, leading dimension ldb >= n,
 * overwritten with the solution): no host copies, nothing allocated after the first call -- the solve's scratch stays with the
 * fit.  Runs on the fit's stream (the caller makes sure B is complete there) and returns when the solve has finished.  This is
 * the entry a predict path that builds its right-hand sides on the device calls, and the one bench.py's --nrhs leg times. */
int sgpr_fit_solve_rhs_dev(sgpr_fit_t f, double *dB, size_t ldb, int nrhs);
/* K*(2 x 2n_pts) rows . alpha for m test points (sympgpr.f90:75-86,112-124 with alpha cached):
 * out_p[k] = Kstar(1,:).alpha, out_q[k] = Kstar(2,:).alpha */
int sgpr_fit_predict_rows(sgpr_fit_t f, int m, const double *q, const double *P, double *out_p,
                          double *out_q);
/* Ky^-1 (n x n, full symmetric, host buffer) from the cached factor: what the drivers compute with
 * scipy.linalg.inv(K + sig2n I) (01_pendulum/implicit/main.py:161) and hand to calcP / calcQ /
 * applymap as `Kyinv`.  W = L^-T by a panel solve on the identity, Ky^-1 = W W^T by the SYRK
 * kernel; two n x n scratch matrices on the device. */
int sgpr_fit_inverse(sgpr_fit_t f, double *Kyinv, size_t ld);
/* gradient of the nll with respect to (lx, ly) on a solved fit: what nll_grad / nll_grad_reg
 * return as nlp_grad (functions/func.py:132-162) */
int sgpr_fit_nll_grad(sgpr_fit_t f, double *grad2);
/* the pieces the per-example nll_grad variants recombine (03_henon_heiles/func.py:168-192,
 * 05_tokamak/SympGPR/func.py:152-168 add a third component from dK/dsig = K / sig):
 * terms5 = [alpha^T dK_lx alpha, tr(Ky^-1 dK_lx), alpha^T dK_ly alpha, tr(Ky^-1 dK_ly), tr(Ky^-1)] */
int sgpr_fit_nll_grad_terms(sgpr_fit_t f, double *terms5);
/* Eigen-decomposition of Ky = K + |sig2n| I on the device (parallel cyclic Jacobi): the
 * positive-definiteness FAILURE path of the drivers' nll_chol, which falls back to
 * `eigsh(Ky, neig, ...)` when cholesky raises (02_pert_pendulum/func.py:194-203,
 * 01_pendulum/implicit/func.py:99-114, 05_tokamak/Split_SympGPR/func.py:128-166).  Ky is rebuilt
 * (a failed factor has overwritten it) and diagonalised in place; w (n) = eigenvalues ascending,
 * c (n) = Q^T z.  The fit has to be built / run again before any other query.
 * Returns 0, or 1 if the rotations did not converge. */
int sgpr_fit_eig(sgpr_fit_t f, double *w, double *c);
/* K* . alpha for m test points with d pairs each: Xt (m x 2d), out (m x 2d), both column-major.  SGPR_E_STATE before a solve
 * and for SGPR_FIT_REG and SGPR_FIT_BLOCK_QQ / _PP fits (their alpha has n_pts entries, the pair kernel reads 2 d n_pts). */
int sgpr_fit_predict_nd(sgpr_fit_t f, int m, const double *Xt, size_t ldxt, double *out);
/* Posterior mean and covariance at m test points from the cached factor: mean_t = K*_t alpha,
 * cov_t = K**_t - K*_t Ky^-1 K*_t^T (latent prior, no noise).  Xt (m x 2d; (q, P) for d = 1 and reg), column-major,
 * ldxt >= m.  D = 2d outputs per point (1 with SGPR_FIT_REG).  mean (m x D, ld m): the same bits as
 * sgpr_fit_predict_rows / _nd.  cov: point t's D x D matrix, column-major, at cov + t*D*D, exactly symmetric.
 * The values are returned as computed: rounding can leave a diagonal entry slightly negative next to a training point.
 * SGPR_E_STATE before a solve and for SGPR_FIT_BLOCK_QQ / _PP fits; SGPR_E_HIP if a strip solve gave up on a hand-off.
 * Device scratch: the fit's block-solve scratch plus one n x 256 block of doubles and a 256 x 256 one, kept until
 * sgpr_fit_trim.  Added in ABI 5 (an additional entry point). */
int sgpr_fit_predict_cov(sgpr_fit_t f, int m, const double *Xt, size_t ldxt, double *mean, double *cov);
/* The learned generating function F itself (every other prediction entry returns its derivatives) and its variance at m test
 * points.  Xt (m x 2d, column-major, ldxt >= max(m, 1); (q, P) for a d = 1 pair fit).  With dx = x_j - x* per coordinate,
 * g_c = f_c'/f_c and E = sig k (product kernels; E_c = sig f_c for the sum kernels), over the N training points x_j:
 *   F(x*)   = sum_j sum_c E_c g_c alpha[c N + j]                    (dF/dq = sgpr_fit_predict_rows' out_p, dF/dP = its out_q),
 *   v_t     = the same summands without alpha (n entries), kappa(t, s) = sig k(x_t, x_s),
 *   var_t   = kappa(t, t) - |L^-1 v_t|^2                                                       without a reference point,
 *   F_t     = F(x_t) - F(x_0),  var_t = kappa(t, t) - 2 kappa(t, 0) + kappa(0, 0) - |L^-1 (v_t - v_0)|^2    with ref = x_0.
 * ref: 2d doubles or NULL.  Derivative observations do not fix the constant of F: without ref the variance is dominated by
 * that constant and does not vanish with data; the variance of a difference does.  F at a point equal to ref is exactly 0.
 * F (m); var (m) or NULL, which skips the solves.  The variance is the latent posterior (no |sig2n| added) and is returned as
 * computed: rounding can leave it slightly negative.  A point with a coordinate that is not finite gives NaN in its F and var
 * only (status 0); a ref that is not finite gives NaN everywhere.  The results are deterministic, and a point's bits do not
 * depend on the other points of the call.  The factor, alpha, the NLL and the workspace are left as they are.
 * SGPR_E_ARG -- before any device work, the message names predict_genfun -- for a null handle, m < 0, ldxt < max(m, 1), a null
 * Xt or F with m > 0, and for an SGPR_FIT_REG fit (which models F directly: sgpr_fit_predict_rows); SGPR_E_STATE before a solve
 * and for SGPR_FIT_BLOCK_QQ / _PP fits; SGPR_E_HIP if a strip solve gave up on a hand-off.  m = 0 returns 0.
 * Device scratch (var only): as sgpr_fit_predict_cov, kept until sgpr_fit_trim.  ABI 5 (an additional entry point). */
int sgpr_fit_predict_genfun(sgpr_fit_t f, int m, const double *Xt, size_t ldxt, const double *ref, double *F, double *var);
/* Gradient of the fit's NLL (1/2 z^T alpha + sum log L_ii) in every hyperparameter, from the cached factor and alpha:
 * grad_theta = 1/2 sum_ij (Ky^-1 - alpha alpha^T)_ij dKy_ij/dtheta.  ngrad must be nhyp + 1.  grad[0 .. nhyp-1] follow the
 * fit's hyp order -- d = 1 and SGPR_FIT_REG (lx, ly, [p,] sig), create_nd (lq_1..lq_d, lP_1..lP_d, [p_1..p_d,] sig) --, and
 * grad[nhyp] is d/dsig2n: Ky holds |sig2n|, so it is sign(sig2n) 1/2 (tr Ky^-1 - alpha^T alpha), sign(0) = +1.
 * Ky^-1 is formed by panels of 2048 rows (4096 above n = 8192) on the trailing blocks of the factor, 2 n^3 / 3 flop in all,
 * each panel contracted with the derivatives of K evaluated pair by pair; the sums are deterministic.  The factor, alpha
 * and the NLL are left as they are.  SGPR_E_ARG for a null handle or grad or a wrong ngrad (before any device call);
 * SGPR_E_STATE before a solve and for SGPR_FIT_BLOCK_QQ / _PP fits; SGPR_E_HIP if the fit's strip solve gave up on a hand-off.
 * Device scratch, allocated and freed per call: one panel (min(n, 2048 or 4096) x n doubles, 4.3 GB at n = 131 072) and
 * the partial sums (a few MB).  Added in ABI 5 (an additional entry point). */
int sgpr_fit_nll_grad_full(sgpr_fit_t f, double *grad, int ngrad);
/* Leave-one-point-out cross-validation of a solved fit (Rasmussen & Williams 5.4.2, for points): point i owns the D rows
 * B_i = {c N + i, c = 0 .. D-1} of Ky (D = 2d; 1 with SGPR_FIT_REG), and with C_i = (Ky^-1)[B_i, B_i], a_i = alpha[B_i]:
 *   residual r_i = C_i^-1 a_i (the observed rows minus their prediction from the fit without point i), covariance
 *   S_i = C_i^-1 (of that prediction, noise included), lpd_i = -1/2 a_i^T C_i^-1 a_i + 1/2 log det C_i - D/2 log 2 pi.
 * loo2 (required) = {loo = -sum_i lpd_i, press = sum_i |r_i|^2}.  resid (n doubles, the layout of z: entry c N + i is point i,
 * part c), cov (point i's D x D matrix at cov + i*D*D, ordered as sgpr_fit_predict_cov's, exactly symmetric) and lpd (N) may
 * each be NULL.  A point whose block has a pivot that is not positive and finite gives NaN in its r, S and lpd and in loo and
 * press; the call still returns 0.  Ky^-1 is formed by the row panels of sgpr_fit_nll_grad_full (2 n^3 / 3 flop), the
 * blocks are copied out of the panels, one thread per point does the D x D algebra; the sums are deterministic.  The factor,
 * alpha, the NLL and the workspace are left as they are.  SGPR_E_ARG for a null handle or loo2; SGPR_E_STATE before a solve
 * and for SGPR_FIT_BLOCK_QQ / _PP fits; SGPR_E_HIP if the fit's strip solve gave up on a hand-off.  Device scratch: one
 * panel (min(n, 2048 or 4096) x n doubles), 8 N D (D + 1) / 2 bytes of blocks, the outputs and the partial sums, in the
 * fit's own scratch block, kept until sgpr_fit_trim.  ABI 5 (an additional entry point). */
int sgpr_fit_loo(sgpr_fit_t f, double *loo2, double *resid, double *cov, double *lpd);
/* One of sgpr_fit_loo's two objectives and its exact gradient in every hyperparameter.  which = SGPR_LOO_LPD: *value = loo;
 * SGPR_LOO_PRESS: *value = press.  grad, its order and ngrad = nhyp + 1 are those of sgpr_fit_nll_grad_full; the last entry
 * is d/dsig2n and carries sign(sig2n).  With S_i = C_i^-1, r_i = S_i a_i (sgpr_fit_loo's notation):
 *   d value / d theta = 1/2 sum_jk (M - beta alpha^T - alpha beta^T)_jk dKy_jk / d theta,  M = Ky^-1 W Ky^-1,  beta = Ky^-1 v,
 *   loo:   W[B_i, B_i] = r_i r_i^T + S_i,             v[B_i] = r_i;
 *   press: W[B_i, B_i] = 2 (r_i s_i^T + s_i r_i^T),   v[B_i] = 2 s_i,  s_i = S_i r_i;   W is zero outside the N blocks.
 * One weight matrix serves all hyperparameters: Ky^-1 is formed densely on the device (n^3 / 3 + n^3 / 3 flop), M by row
 * panels (n^3 flop), each contracted with dKy evaluated pair by pair; the sums are deterministic.  If a point's block has a
 * pivot that is not positive and finite, *value and every entry of grad are NaN and the call returns 0.  The factor, alpha,
 * the NLL and the workspace are left as they are.  SGPR_E_ARG for a null handle, value or grad, a wrong ngrad or an unknown
 * which (before any device call); SGPR_E_STATE before a solve and for SGPR_FIT_BLOCK_QQ / _PP fits; SGPR_E_NOMEM -- the
 * message names the bytes needed, the handle keeps what it had -- if the scratch does not fit; SGPR_E_HIP if the fit's strip
 * solve gave up on a hand-off.  Device scratch: two n x n blocks, one panel (min(n, 2048 or 4096) x n doubles) and a few
 * vectors, in the fit's own scratch block, kept until sgpr_fit_trim: n <= ~98 304 on one card.  ABI 5 (an additional entry
 * point). */
enum { SGPR_LOO_LPD = 0, SGPR_LOO_PRESS = 1 };
int sgpr_fit_loo_grad(sgpr_fit_t f, int which, double *value, double *grad, int ngrad);
/* cond_2(Ky) estimated from below with the device's own kernels (needs a valid factor): lambda_max by `iters` power iterations on
 * Ky v -- the rows of K re-evaluated from the training points by the prediction kernel, plus |sig2n| v --, lambda_min by `iters`
 * inverse iterations with the cached factor.  out4 = {lambda_max, lambda_min, cond, relative change of the quotients in the last
 * step}.  The reference never computes it; SURVEY.md 7 / 8(d) ask for it beside every parity number (the tolerance on alpha is a
 * multiple of cond * eps).  ABI 5. */
int sgpr_fit_cond_estimate(sgpr_fit_t f, int iters, double *out4);
/* milliseconds of the last build / factor / solve stage (hipEvent timing on the fit's stream) */
int sgpr_fit_stage_ms(sgpr_fit_t f, double *build_ms, double *factor_ms, double *solve_ms);
/* milliseconds of the device part of the last sgpr_fit_solve_rhs / _dev (the two triangular solves with their pack / unpack passes;
 * the host <-> device copies of B are outside): -1 when there has been none */
int sgpr_fit_solve_rhs_ms(sgpr_fit_t f, double *ms);
/* gives back the device scratch the block solves of this fit keep from call to call (sgpr_fit_solve_rhs / _dev: ~0.8 GB at
 * n = 98 304); the next block solve allocates it again.  Waits for the fit's stream.  ABI 5. */
int sgpr_fit_trim(sgpr_fit_t f);
/* device pointers of the fit (for callers that own a torch / HIP context): K/L, alpha */
int sgpr_fit_device_ptrs(sgpr_fit_t f, void **dA, size_t *lda, void **dalpha);
int sgpr_fit_destroy(sgpr_fit_t f);

/* ---- many small independent fits in ONE launch ----------------------------------------------
 * The reference's only batch axis: `nphmap` independent GP pairs (one per toroidal section) and the
 * CMA-ES populations that evaluate nll_chol for many hyper-parameter vectors
 * (python/05_tokamak/Split_SympGPR/main.py:36-41,63-66,96-112), at matrix orders 40 ... 160.
 * Problem b = 0..nbatch-1: the body of nll_chol (python/functions/func.py:189-196; with SGPR_FIT_REG
 * of nll_chol_reg, :180-187) on points x[b*n_pts ..], y[b*n_pts ..], targets z[b*n ..], hyper-parameters
 * hyp[b*nhyp ..], noise |sig2n[b]|;  n = 2 n_pts (n_pts with SGPR_FIT_REG) <= sgpr_fit_batch_max_order().
 * Outputs (host): alpha (nbatch x n, may be NULL), nll (nbatch), info (nbatch; 0 or the LAPACK-style
 * index of the first non-positive pivot of that problem -- the call itself still returns 0). */
int sgpr_fit_batch_max_order(void);
int sgpr_fit_batch(int family, int nbatch, int n_pts, const double *x, const double *y, const double *z,
                   const double *hyp, int nhyp, const double *sig2n, unsigned flags, double *alpha,
                   double *nll, int *info);
/* sgpr_fit_batch for problems with d canonical pairs per point (d = 1, 2, 3; sgpr_fit_create_nd's kernels, block order and hyp):
 * a population of hyper-parameter vectors, or many small data sets, of a d-pair fit in one call.  Order per problem
 * n = 2 d n_pts <= sgpr_fit_batch_max_order() (2048).
 *   X:   nbatch x 2d x n_pts; coordinate m of point i of problem b at X[(b 2d + m) n_pts + i], columns q_1..q_d, P_1..P_d --
 *        sgpr_fit_create_nd's column-major X with ldx = n_pts, problem after problem (d = 1: sgpr_fit_batch's x | y);
 *   z:   nbatch x n in the block order of the matrix (row a n_pts + i), as a d-pair handle takes it;
 *   hyp: nbatch x nhyp, each row (lq_1..lq_d, lP_1..lP_d, sig), nhyp = 2d + 1, or (lq.., lP.., p_1..p_d, sig), nhyp = 3d + 1, for
 *        families with a period; noise |sig2n[b]|.
 * alpha (nbatch x n, may be NULL), nll, info exactly as sgpr_fit_batch: info[b] > 0 is the index of the first non-positive
 * pivot of problem b and the call still returns 0; a NaN target poisons its own problem only.  A problem's bits do not depend on
 * its place in the batch or on the batch size.
 * n <= 256: ONE launch, one workgroup per problem -- each point pair is evaluated once (one exp, d sincos) and feeds its entry
 * of every block of the lower triangle; the factor, solves and nll behind it are sgpr_fit_batch's own code.  Scratch: 512 KiB +
 * 260 KiB per workgroup, at most 1024 workgroups.  256 < n <= 2048: sgpr_fit_batch's mid path with a d-pair build: per chunk of
 * problems one build, one or three factor launches, the right-hand sides, two strip solves and the finish (6 or 8 launches);
 * scratch per chunk: one npad x npad image per problem (npad = n rounded up to 128), at most ~2 GiB, plus the leaf inverses and
 * solve vectors.  All of it lives in the sgpr_fit_batch arena of the calling thread; sgpr_trim gives it back.
 * SGPR_E_ARG (before any device call) for d outside 1..3, an unknown family, a wrong nhyp, flags != 0 (there is no scalar-kernel
 * d-pair fit), nbatch < 0, n_pts <= 0, n above the maximum and a null pointer other than alpha; nbatch == 0 returns 0.  The
 * gradient is sgpr_fit_batch_nd_grad, leave-one-point-out sgpr_fit_batch_nd_loo and its gradient sgpr_fit_batch_nd_loo_grad.  ABI 5
 * (an additional entry point). */
int sgpr_fit_batch_nd(int family, int d, int nbatch, int n_pts, const double *X, const double *z, const double *hyp,
                      int nhyp, const double *sig2n, unsigned flags, double *alpha, double *nll, int *info);
/* sgpr_fit_batch_nd plus d nll / d(hyp, sig2n) per problem, for every order n = 2 d n_pts <= sgpr_fit_batch_max_order() (2048) in
 * one entry.  X, z, hyp, nhyp, sig2n, alpha (may be NULL), nll and info exactly as sgpr_fit_batch_nd.  grad: nbatch x (nhyp + 1),
 * row-major; row b = (d/dlq_1..d/dlq_d, d/dlP_1..d/dlP_d, [d/dp_1..d/dp_d,] d/dsig, d/dsig2n), the order of
 * sgpr_fit_nll_grad_full on an sgpr_fit_create_nd handle.  Ky holds |sig2n[b]|, so the last entry is sign(sig2n[b]) * 1/2 (tr Ky^-1
 * - alpha^T alpha), with sign(0) = +1.  info[b] > 0: nll[b] and the whole row grad[b] are NaN, the other problems are untouched
 * and the call returns 0.  nll, alpha and info are bit-identical to sgpr_fit_batch_nd's (the same Gram stage, factor and solves);
 * a problem's gradient bits do not depend on its place in the batch, the batch size, the chunk it falls into or a repetition of
 * the call (no atomics, no waiting between workgroups in the gradient phase).
 * n <= 256: ONE launch, one workgroup per problem: after the fit it forms L^-T from the leaf inverses and Ky^-1 = L^-T L^-1 over L
 * (the code of sgpr_fit_batch_grad), then thread i takes row i of Ky^-1 - alpha alpha^T -- part i / n_pts of point i % n_pts -- and
 * walks the column points: each point pair is evaluated once, dK from the generated forms, and feeds its 2d entries of the row
 * (W_ii on the diagonal, 2 W_ij below it).  Scratch per workgroup as sgpr_fit_batch_grad: ~1.3 MiB, at most 1024 workgroups.
 * 256 < n <= 2048: sgpr_fit_batch_nd's mid path with both images, then the Ky^-1 stage of sgpr_fit_batch_grad_mid (unchanged) and
 * one contraction launch over rows x column points with a fold per problem; chunks and scratch as sgpr_fit_batch_grad_mid, the
 * partials 16 doubles wide (up to 3d + 2 = 11 sums).  The arena is sgpr_fit_batch's; sgpr_trim gives it back.
 * SGPR_E_ARG (before any device call) for d outside 1..3, an unknown family, a wrong nhyp, flags != 0, nbatch < 0, n_pts <= 0, n
 * above the maximum and a null pointer other than alpha (grad is required); nbatch == 0 returns 0.  ABI 5 (an additional entry
 * point). */
int sgpr_fit_batch_nd_grad(int family, int d, int nbatch, int n_pts, const double *X, const double *z, const double *hyp,
                           int nhyp, const double *sig2n, unsigned flags, double *alpha, double *nll, double *grad, int *info);
/* sgpr_fit_batch_nd plus leave-one-point-out cross-validation of every problem (see sgpr_fit_loo; a point owns its D = 2d rows
 * {c n_pts + i}), for every order n = 2 d n_pts <= sgpr_fit_batch_max_order() (2048) in one entry.  X, z, hyp, nhyp, sig2n, flags
 * (must be 0), alpha (may be NULL), nll and info exactly as sgpr_fit_batch_nd.  loo: nbatch x 2, row-major; row b = {loo, press} by
 * sgpr_fit_loo's definitions.  nll, alpha and info are bit-identical to sgpr_fit_batch_nd's; info[b] > 0: nll[b] and the row loo[b]
 * are NaN, the other problems are untouched and the call returns 0.  A problem's loo bits do not depend on its place in the batch,
 * the batch size, the chunk or a repetition (no atomics).  n <= 256: one launch, one workgroup per problem, which after the fit
 * forms Ky^-1 = L^-T L^-1 over L as sgpr_fit_batch_nd_grad does; then thread i gathers point i's D x D block of Ky^-1 from the lower
 * triangle and takes it through the block algebra of sgpr_fit_loo in registers; the sums fold in a fixed order.  Scratch as
 * sgpr_fit_batch_nd_grad.  Above: the chunks, images and Ky^-1 stage of sgpr_fit_batch_nd_grad's mid path, then one thread per point
 * and a fold per problem in place of the contraction (sgpr_fit_batch_loo's kernels at block size D).  SGPR_E_ARG (before any device
 * call) for d outside 1..3, an unknown family, a wrong nhyp, flags != 0, nbatch < 0, n_pts <= 0, n above the maximum and a null
 * pointer other than alpha (loo is required); nbatch == 0 returns 0.  ABI 5 (an additional entry point). */
int sgpr_fit_batch_nd_loo(int family, int d, int nbatch, int n_pts, const double *X, const double *z, const double *hyp,
                          int nhyp, const double *sig2n, unsigned flags, double *alpha, double *nll, double *loo, int *info);
/* sgpr_fit_batch_nd plus one leave-one-point-out objective and its gradient per problem, for orders n = 2 d n_pts <= 256.  which:
 * SGPR_LOO_LPD (value = loo) or SGPR_LOO_PRESS (value = press), the same for the whole batch; value: nbatch; grad: nbatch x
 * (nhyp + 1), row-major, in sgpr_fit_batch_nd_grad's order, the last entry d/dsig2n with sign(sig2n[b]) (sign(0) = +1); the formulas
 * are sgpr_fit_loo_grad's with D = 2d.  Everything else as sgpr_fit_batch_nd.  nll, alpha and info are bit-identical to
 * sgpr_fit_batch_nd's and value to column `which` of sgpr_fit_batch_nd_loo's (the same code up to the sums).  info[b] > 0: nll[b],
 * value[b] and the whole row grad[b] are NaN, the other problems are untouched and the call returns 0.  A problem's bits do not
 * depend on its place in the batch, the batch size or a repetition.  One launch, one workgroup per problem: behind
 * sgpr_fit_batch_nd_loo's steps each point's weight block W~_i (D (D + 1) / 2 doubles) and v[B_i] go to LDS, Ky^-1 is mirrored to
 * full storage, beta = Ky^-1 v and Y = W~ Ky^-1 (D rows of Ky^-1 per row of Y) follow, then W' = Ky^-1 Y - beta alpha^T - alpha beta^T
 * (n^3 flop, sgpr_fit_batch_loo_grad's code) and its contraction with dK over D x D blocks of point pairs
 * (sgpr_fit_batch_nd_grad's code).  Scratch per workgroup as sgpr_fit_batch_loo_grad: ~1.8 MiB, at most 1024 workgroups (~1.8 GiB),
 * in the sgpr_fit_batch arena, kept until sgpr_trim.  SGPR_E_ARG (before any device call) for d outside 1..3, an unknown family, a
 * wrong nhyp, flags != 0, an unknown which, nbatch < 0, n_pts <= 0, an order above 256 and a null pointer other than alpha;
 * nbatch == 0 returns 0.  ABI 5 (an additional entry point). */
int sgpr_fit_batch_nd_loo_grad(int family, int d, int nbatch, int n_pts, const double *X, const double *z, const double *hyp,
                               int nhyp, const double *sig2n, unsigned flags, int which, double *alpha, double *nll,
                               double *value, double *grad, int *info);
/* sgpr_fit_batch plus d nll / d(hyp, sig2n) per problem.  Order per problem n = 2 n_pts (n_pts with SGPR_FIT_REG) <= 256.
 * grad: nbatch x (nhyp + 1), row-major; row b = (d/dhyp_0 .. d/dhyp_{nhyp-1}, d/dsig2n).  hyp layout and nhyp as
 * sgpr_fit_batch: (lx, ly, sig), or (lx, ly, p, sig) for families with a period.  Ky holds |sig2n[b]|, so the last entry is
 * sign(sig2n[b]) * 1/2 (tr Ky^-1 - alpha^T alpha), with sign(0) = +1.  info[b] > 0: nll[b] and the whole row grad[b] are NaN.
 * nll, alpha and info are bit-identical to sgpr_fit_batch's (the same factor and solves); the gradient of a problem is
 * deterministic and does not depend on its place in the batch.  One launch, one workgroup per problem: after the fit it
 * forms L^-1 from the leaf inverses, Ky^-1 = L^-T L^-1 and contracts Ky^-1 - alpha alpha^T with dK pair by pair.  SGPR_E_ARG
 * (before any device call) for an unknown family, a wrong nhyp, an unknown flag, nbatch < 0, n_pts <= 0, an order above 256
 * and a null pointer other than alpha; nbatch == 0 returns 0.  Device scratch: the sgpr_fit_batch arena grows to ~1.3 MiB per
 * workgroup (up to 1024 workgroups: ~1.3 GiB), kept until sgpr_trim.  Added in ABI 5 (an additional entry point). */
int sgpr_fit_batch_grad(int family, int nbatch, int n_pts, const double *x, const double *y, const double *z,
                        const double *hyp, int nhyp, const double *sig2n, unsigned flags, double *alpha,
                        double *nll, double *grad, int *info);
/* The same for 256 < n <= sgpr_fit_batch_max_order() (2048): arguments, hyp layout, the SGPR_FIT_REG flag and the layout of grad
 * exactly as sgpr_fit_batch_grad -- grad: nbatch x (nhyp + 1), row-major, the last entry sign(sig2n[b]) * 1/2 (tr Ky^-1 -
 * alpha^T alpha), sign(0) = +1; info[b] > 0: nll[b] and the whole row grad[b] are NaN, the other problems are untouched.  nll,
 * alpha and info are bit-identical to sgpr_fit_batch's (the same build, factor and solves); a problem's gradient bits do not
 * depend on its place in the batch, the batch size, the chunk it falls into or a repetition of the call (no atomics, no waiting
 * between workgroups in the gradient phase).  Per chunk of problems, behind the solves: U = L^-T in a second npad x npad image
 * (npad = n rounded up to 128) from the leaf inverses by doubling the block size, at most 2 ceil(log2(npad / 128)) launches of
 * 128 x 128 fp64 MFMA tiles; Ky^-1 = U U^T (lower tiles) over L; one contraction launch with dK pair by pair and a fold per
 * problem.  SGPR_E_ARG (before any device call) for an order <= 256 (sgpr_fit_batch_grad's range) or above the maximum, an
 * unknown family, a wrong nhyp, an unknown flag, nbatch < 0, n_pts <= 0 and a null pointer other than alpha; nbatch == 0
 * returns 0.  Device scratch per chunk: two images of 8 npad^2 bytes per problem, chunks sized to ~2 GiB of images (32
 * problems of order 2048; sgpr_fit_batch: one image, 64), plus the leaf inverses (8 * 128 npad bytes per problem) and the solve
 * vectors; it lives in the sgpr_fit_batch arena and sgpr_trim gives it back.  ABI 5 (an additional entry point). */
int sgpr_fit_batch_grad_mid(int family, int nbatch, int n_pts, const double *x, const double *y, const double *z,
                            const double *hyp, int nhyp, const double *sig2n, unsigned flags, double *alpha,
                            double *nll, double *grad, int *info);
/* sgpr_fit_batch plus leave-one-point-out cross-validation of every problem (see sgpr_fit_loo; D = 2, 1 with SGPR_FIT_REG), for
 * every order n = 2 n_pts (n_pts with SGPR_FIT_REG) <= sgpr_fit_batch_max_order().  loo: nbatch x 2, row-major; row b = {loo,
 * press}.  hyp layout and nhyp as sgpr_fit_batch; the noise enters as |sig2n[b]|.  nll, alpha (may be NULL) and info are
 * bit-identical to sgpr_fit_batch's; info[b] > 0: nll[b] and the row loo[b] are NaN, the other problems are untouched.  A
 * problem's loo bits do not depend on its place in the batch, the batch size, the chunk or a repetition (no atomics).  n <= 256:
 * one launch, one workgroup per problem, which after the fit forms Ky^-1 = L^-T L^-1 as sgpr_fit_batch_grad does and then
 * takes one thread per point.  Above: the chunks, images and Ky^-1 of sgpr_fit_batch_grad_mid, then one thread per point and a
 * fold per problem in place of the contraction.  SGPR_E_ARG (before any device call) for an unknown family, a wrong nhyp, an
 * unknown flag, nbatch < 0, n_pts <= 0, an order above the maximum and a null pointer other than alpha; nbatch == 0 returns 0.
 * Device scratch: that of sgpr_fit_batch_grad (n <= 256) or sgpr_fit_batch_grad_mid, in the sgpr_fit_batch arena, kept until
 * sgpr_trim.  ABI 5 (an additional entry point). */
int sgpr_fit_batch_loo(int family, int nbatch, int n_pts, const double *x, const double *y, const double *z,
                       const double *hyp, int nhyp, const double *sig2n, unsigned flags, double *alpha,
                       double *nll, double *loo, int *info);
/* sgpr_fit_batch plus one of sgpr_fit_batch_loo's two objectives and its exact gradient in (hyp, sig2n) per problem.  Order per
 * problem n = 2 n_pts (n_pts with SGPR_FIT_REG) <= 256.  Arguments, hyp layout and flags as sgpr_fit_batch_grad; which =
 * SGPR_LOO_LPD: value[b] = loo, SGPR_LOO_PRESS: value[b] = press (value: nbatch doubles).  grad: nbatch x (nhyp + 1), row-major;
 * row b = (d/dhyp_0 .. d/dhyp_{nhyp-1}, d/dsig2n) of value[b], by the formulas of sgpr_fit_loo_grad (D = 2; 1 with SGPR_FIT_REG).
 * The noise enters as |sig2n[b]|, so the last entry carries sign(sig2n[b]), with sign(0) = +1.  nll, alpha (may be NULL) and info
 * are bit-identical to sgpr_fit_batch's; value[b] is bit-identical to the `which` column of sgpr_fit_batch_loo's row b (the same
 * code); a problem's value and gradient bits do not depend on its place in the batch, the batch size or a repetition (no atomics,
 * no waiting between workgroups).  info[b] > 0: nll[b], value[b] and the whole row grad[b] are NaN, nothing is computed for that
 * problem and the others are untouched.  A point whose block has a pivot that is not positive and finite makes value[b] and the
 * whole row grad[b] NaN through the arithmetic; the call still returns 0.  One launch, one workgroup per problem: after the fit
 * it forms Ky^-1 as sgpr_fit_batch_grad does, takes one thread per point as sgpr_fit_batch_loo does and keeps the point's weight
 * block and v in LDS, then beta = Ky^-1 v (n^2 flop), Y = W Ky^-1 over L^-T, M = Ky^-1 Y (lower triangle, n^3 flop) and
 * the contraction of M - beta alpha^T - alpha beta^T with dKy pair by pair, the code of sgpr_fit_batch_grad's last step.
 * SGPR_E_ARG (before any device call) for an unknown family, a wrong nhyp, an unknown flag, an unknown which, nbatch < 0,
 * n_pts <= 0, an order above 256 and a null pointer other than alpha; nbatch == 0 returns 0.  Device scratch: the sgpr_fit_batch
 * arena grows to three 256 x 256 blocks (Ky^-1, L^-T / Y, M) beside the leaf inverses, ~1.8 MiB per workgroup (up to 1024
 * workgroups: ~1.8 GiB), kept until sgpr_trim.  ABI 5 (an additional entry point). */
int sgpr_fit_batch_loo_grad(int family, int nbatch, int n_pts, const double *x, const double *y, const double *z,
                            const double *hyp, int nhyp, const double *sig2n, unsigned flags, int which, double *alpha,
                            double *nll, double *value, double *grad, int *info);
/* sgpr_fit_batch_loo_grad for orders 256 < n <= sgpr_fit_batch_max_order() (2048): arguments, outputs, the sign of the last entry
 * and the NaN rows exactly as there.  nll, alpha and info are bit-identical to sgpr_fit_batch's and value[b] to the `which` column of
 * sgpr_fit_batch_loo's row b (the same code up to the sums); a problem's bits do not depend on its place in the batch, the batch
 * size, the chunking or a repetition (no atomics, no waiting between workgroups).  Per chunk of problems, behind sgpr_fit_batch's mid
 * path and the Ky^-1 stage of sgpr_fit_batch_grad_mid: one thread per point (sgpr_fit_batch_loo's pass, which also keeps the weight
 * block W~_i and v), the mirror of Ky^-1 to full storage, beta = Ky^-1 v, Z = Ky^-1 W~ over the L^-T image, M = Ky^-1 Z^T (lower
 * 128 x 128 tiles, n^3 flop per problem on the fp64 matrix cores) into a third npad x npad image, and sgpr_fit_batch_grad_mid's
 * contraction with the weight M - beta alpha^T - alpha beta^T.  Scratch per chunk: three images per problem, at most ~2 GiB (21
 * problems of order 2048), plus W~, v, beta and the partials, in the sgpr_fit_batch arena, kept until sgpr_trim.  SGPR_E_ARG (before any
 * device call) for an order <= 256 or above the maximum (the message names the order and the limit), an unknown family, a wrong nhyp,
 * an unknown flag, an unknown which, nbatch < 0, n_pts <= 0 and a null pointer other than alpha; nbatch == 0 returns 0.  ABI 5 (an
 * additional entry point). */
int sgpr_fit_batch_loo_grad_mid(int family, int nbatch, int n_pts, const double *x, const double *y, const double *z,
                                const double *hyp, int nhyp, const double *sig2n, unsigned flags, int which, double *alpha,
                                double *nll, double *value, double *grad, int *info);
/* The same for problems with d canonical pairs per point: sgpr_fit_batch_nd_loo_grad for orders 256 < n = 2 d n_pts <=
 * sgpr_fit_batch_max_order(), arguments and outputs as there, over 2d x 2d point blocks; nll, alpha and info are bit-identical to
 * sgpr_fit_batch_nd's and value to column `which` of sgpr_fit_batch_nd_loo's.  SGPR_E_ARG as above, and for d outside 1..3 and
 * flags != 0.  ABI 5 (an additional entry point). */
int sgpr_fit_batch_nd_loo_grad_mid(int family, int d, int nbatch, int n_pts, const double *X, const double *z, const double *hyp,
                                   int nhyp, const double *sig2n, unsigned flags, int which, double *alpha, double *nll,
                                   double *value, double *grad, int *info);

/* Gives back what the CALLING thread's earlier calls keep for re-use: the device arena and page-locked staging block of
 * sgpr_fit_batch and sgpr_fit_batch_grad (up to ~2 GiB after a large batch of order-2048 problems, ~1.3 GiB after a gradient batch
 * of 1024 problems or more, ~1.8 GiB after such a batch of sgpr_fit_batch_loo_grad; they also shrink by themselves when a much smaller batch
 * follows) and the pooled events of its factorisations.  Never needed for correctness; call it between a hyper-parameter search
 * over small problems and a fit that wants the whole HBM.  No call of this thread may be in flight. */
int sgpr_trim(void);

/* ---- device-pointer primitives (the tiles a distributed driver composes) ------------------ */

/* Pair-tile Gram build.  For pair rows i = 0..mi-1 (row point b = (xb[i], yb[i])) and pair
 * columns j = 0..mj-1 (column point a = (xa[j], ya[j])) writes, for each selected part,
 *   qq[i + j*ld] = sig d2k/dxdx0,  Pq / qP = sig d2k/dxdy0,  PP = sig d2k/dydy0
 * (the four K(...) assignments of sympgpr.f90:27-34).  `diag_off`: global_row - global_col of
 * element (0,0); |noise| is added on qq / PP where i + diag_off == j (func.py:192). */
int sgpr_gram_pairs_dev(int family, int mi, int mj, const double *xb, const double *yb,
                        const double *xa, const double *ya, const double *hyp, int nhyp,
                        double *qq, double *Pq, double *qP, double *PP, size_t ld,
                        long diag_off, double noise, unsigned flags, void *stream);
/* scalar-kernel Gram tile: G[i + j*ld] = sig k(a_j, b_i)  (sympgpr.f90:54-59) */
int sgpr_gram_reg_dev(int family, int mi, int mj, const double *xb, const double *yb,
                      const double *xa, const double *ya, const double *hyp, int nhyp,
                      double *G, size_t ld, long diag_off, double noise, void *stream);

/* Pair-tile Gram build for d canonical pairs per point: Xb (mi x 2d), Xa (mj x 2d) column-major;
 * block (a, b) of the output at K + a*rstride + b*cstride*ld, each mi x mj. */
int sgpr_gram_nd_dev(int family, int d, int mi, int mj, const double *Xb, size_t ldxb,
                     const double *Xa, size_t ldxa, const double *hyp, int nhyp, double *K, size_t ld,
                     size_t rstride, size_t cstride, long diag_off, double noise, void *stream);
/* The same pairs, but only the blocks (a, b) with roff[a] >= 0 and coff[b] >= 0 (2d entries each, host arrays), block
 * (a, b) at K + roff[a] + coff[b] * ld: for a block-cyclic rank whose coordinate blocks hold DIFFERENT points (N / nb not a
 * multiple of the process grid), one call per pair of distinct point selections. */
int sgpr_gram_nd_sel_dev(int family, int d, int mi, int mj, const double *Xb, size_t ldxb,
                         const double *Xa, size_t ldxa, const double *hyp, int nhyp, double *K, size_t ld,
                         const long *roff, const long *coff, void *stream);
/* workspace (bytes) sgpr_potrf_dev / sgpr_trsm_rlt_dev need for order n */
size_t sgpr_potrf_workspace(int n);
/* The workspace BEGINS with the inverses of the 128 x 128 diagonal leaves of L (ceil(n / 128) blocks of 128 x 128
 * doubles): these bytes, with L itself, are all sgpr_trsm_rlt_dev / sgpr_trsv_dev read of what sgpr_potrf_dev leaves
 * there -- what a distributed driver has to send along with a diagonal block.  The rest is scratch. */
size_t sgpr_potrf_inverses_bytes(int n);
/* sgpr_potrf_dev keeps, per device, one high-priority side stream shared by all callers (every panel kernel of the device
 * runs on it, one at a time, whatever number of handles / host threads factor at once) and, for the orders the task-queue
 * driver takes (13312 .. 28672 unless SGPR_POTRF_Q=0), a pair of CU-masked streams.  They are created on first use and live until this call drains and destroys them (they come
 * back on demand).  Call it with no factorisation being enqueued on `device`; never needed for correctness -- but do call
 * it before the process ends when a profiler is attached: with the masked streams left to the runtime's own teardown a run
 * under rocprofv3 crashed in an exit handler (after its output was written).  The Python binding does so in an atexit hook.
 * Touches `device` only if this library has streams on it. */
int sgpr_release_device_streams(int device);
/* lower Cholesky in place; only the lower triangle of A is read or written.
 * dinfo: device int, 0 or the 1-based failing minor. */
int sgpr_potrf_dev(int n, double *A, size_t lda, void *work, size_t lwork, int *dinfo,
                   void *stream);
/* What the value a caller has read back from `dinfo` means: 0 and LAPACK-style positive values come back unchanged; a negative
 * value is an internal give-up (a bounded wait between the persistent kernels of the factorisation ran out: A is NOT factored,
 * restore it and call sgpr_potrf_dev again) -> SGPR_E_HIP, and the task-queue driver is switched off on `stream`'s device, so the
 * retry takes the launch-per-step driver.  (The fit handle and sgpr_potrf_host do this retry themselves.) */
int sgpr_potrf_info_dev(int info, void *stream);
/* B (m x n) := B L^-T with L (n x n) lower, its diagonal-leaf inverses in `work` as left by
 * sgpr_potrf_dev on that L (the panel solve of a right-looking step). */
int sgpr_trsm_rlt_dev(int m, int n, const double *L, size_t ldl, double *B, size_t ldb,
                      const void *work, void *stream);
/* C (m x n) := beta C + alpha A (m x k) B(n x k)^T ; lower != 0: only tiles touching
 * row >= col (+ diag_off) are computed (SYRK-style trailing update). */
int sgpr_gemm_nt_dev(int m, int n, int k, double alpha, const double *A, size_t lda,
                     const double *B, size_t ldb, double beta, double *C, size_t ldc, int lower,
                     long diag_off, void *stream);
/* SYRK-style update of a LOCAL piece of a 2-D block-cyclic matrix: as sgpr_gemm_nt_dev with
 * lower != 0, but a tile is computed iff it touches a block on/below the GLOBAL diagonal:
 * (row / blk) * pr + pi >= (col / blk) * pc + pj   (blk = block size, (pr, pc) = process grid,
 * (pi, pj) = this rank's grid coordinates plus the block offsets of C's first row / column). */
int sgpr_gemm_nt_bc_dev(int m, int n, int k, double alpha, const double *A, size_t lda,
                        const double *B, size_t ldb, double beta, double *C, size_t ldc, int blk,
                        int pr, int pi, int pc, int pj, void *stream);
/* b (n) := L^-1 b (trans = 0) or L^-T b (trans != 0); `work` as left by sgpr_potrf_dev on L.
 * The one-launch strip solves keep their tickets, progress counters and published segments IN the workspace: ONE solve
 * per workspace at a time (a second stream solving against the same factor needs its own copy of `work`). */
int sgpr_trsv_dev(int n, const double *L, size_t ldl, void *work, double *b, int trans,
                  void *stream);
/* Waits for `stream`, then: 0, or SGPR_E_HIP when a strip solve on this workspace gave up on a hand-off between two
 * workgroups (a bounded wait ran out: a device problem, never a property of the matrix).  Call it after the last
 * sgpr_trsv_dev / sgpr_potrs_vec_dev of a solve before trusting b. */
int sgpr_solve_status_dev(int n, const double *L, size_t ldl, const void *work, void *stream);
/* C (m x n) := beta C + alpha A (m x k) B (k x n)   (ABI 5; the backward half of a block of right-hand sides stored as rows) */
int sgpr_gemm_nn_dev(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb,
                     double beta, double *C, size_t ldc, void *stream);
/* B (m x n) := B L^-1 with L (n x n) lower and `work` as left by sgpr_potrf_dev on it: with the right-hand sides of L^T X = Y stored
 * as the ROWS of B this is the backward solve (sgpr_trsm_rlt_dev, B := B L^-T, is the forward one).  ABI 5. */
int sgpr_trsm_rl_dev(int m, int n, const double *L, size_t ldl, double *B, size_t ldb, const void *work, void *stream);
/* cnt blocks of rows x cols doubles: block i is copied from src + i * sstep (leading dimension lds) to dst + i * dstep (ldd).
 * The packing / regrouping copies of a block-cyclic panel exchange as one launch on the caller's stream.  ABI 5. */
int sgpr_copy_blocks_dev(int rows, int cols, int cnt, const double *src, size_t lds, size_t sstep, double *dst, size_t ldd,
                         size_t dstep, void *stream);
/* y -= A x (trans = 0: A m x k, x k, y m) or y -= A^T x (trans != 0: x m, y k) */
int sgpr_gemv_sub_dev(int trans, int m, int k, const double *A, size_t lda, const double *x,
                      double *y, void *stream);
/* K*(2 x 2 n0) . alpha for m test points, everything device-resident (sympgpr.f90:75-86 calcq,
 * :112-124 target of calcP, with alpha = Kyinv ztrain cached): out_p = row 1, out_q = row 2 */
int sgpr_predict_rows_dev(int family, int m, const double *q, const double *P, int n0,
                          const double *xtrain, const double *ytrain, const double *hyp, int nhyp,
                          const double *alpha, double *out_p, double *out_q, void *stream);
/* the same for d canonical pairs: Xt (m x 2d), Xtrain (n0 x 2d), alpha (2 d n0), out (m x 2d),
 * all column-major device buffers */
int sgpr_predict_nd_dev(int family, int d, int m, const double *Xt, size_t ldxt, int n0,
                        const double *Xtrain, size_t ldxtr, const double *hyp, int nhyp,
                        const double *alpha, double *out, void *stream);
/* Kstar(1 x n0) . alpha with the scalar kernel (sympgpr.f90:62-73 guessP) */
int sgpr_predict_reg_dev(int family, int m, const double *q, const double *P, int n0,
                         const double *xtrain, const double *ytrain, const double *hyp, int nhyp,
                         const double *alpha, double *out, void *stream);
/* applymap / applymap_henon (functions/func.py:216-260; calcP / calcQ / guessP of sympgpr.f90:62-125
 * inlined) for all Ntest orbits with every time step on the device: one workgroup per orbit, the
 * implicit equation for P solved by a secant iteration from the regular-GP guess (tol 1e-13 like
 * hybrd1).  alpha = Kyinv ztrain, alphap = Kyinvp ztrainp.
 * mode bits select the per-example variants of the same recurrence:
 *   SGPR_MAP_WRAP_Q    q mod 2 pi                 (applymap; not applymap_henon, func.py:239-260)
 *   SGPR_MAP_WRAP_P    P mod 2 pi before the q update (04_standard_map/func.py:218-254)
 *   SGPR_MAP_EXPLICIT  P = p - Kstar(1,:).alpha at (q, p), no implicit solve and no first-guess GP
 *                      (01_pendulum/explicit/func_expl.py:106-128, 04_standard_map/func.py:174-179,
 *                      256-285); hypp / xtrainp / ytrainp / alphap are ignored
 *   SGPR_MAP_LOSS_NEGP P < 0 after the implicit solve ends the orbit (the tokamak maps)
 * qmap, pmap: [nm][ntest] C-ordered; a NaN marks a lost orbit from that step on.  pdiff (may be
 * NULL): the unwrapped momentum, pdiff[i+1] = pdiff[i] + (P_new - p_i) (04_standard_map/func.py:234). */
#define SGPR_MAP_WRAP_Q 1
#define SGPR_MAP_WRAP_P 2
#define SGPR_MAP_EXPLICIT 4
#define SGPR_MAP_LOSS_NEGP 8   /* implicit map: an orbit whose new momentum P is negative is lost (NaN) from that step on -- the
                                * tokamak drivers' loss test (05_tokamak/SympGPR/func.py:190-211, sympgpr.f90:128-177) without
                                * its flux-surface half (fieldlines.compute_r stays with the caller).  ABI 5. */
int sgpr_applymap_host(int family, int mode, int nm, int ntest, const double *hyp, int nhyp, int n0,
                       const double *xtrain, const double *ytrain, const double *alpha,
                       const double *hypp, int nhypp, int n0p, const double *xtrainp,
                       const double *ytrainp, const double *alphap, const double *Q0,
                       const double *P0, double *qmap, double *pmap, double *pdiff);
/* The SECTIONED map (05_tokamak/Split_SympGPR/func.py:184-219): nsec independent GP pairs of one size, one per toroidal
 * section, applied in turn -- step i -> i + 1 of every orbit uses section (first + i) mod nsec -- with all nm - 1 steps of all
 * ntest orbits in ONE launch.  The step is sgpr_applymap_host's (same secant, tol, maxiter, acceptance rule, mode bits, pdiff,
 * NaN for a lost orbit), and with nsec == 1 the outputs have that entry's bits wherever it runs one workgroup per orbit.  One
 * 256-thread workgroup per orbit at every n0; no workgroup waits for another.  An orbit's bits depend on nothing but its own
 * start point, `first` and the sections: a map continued from row i with first' = (first + i) mod nsec repeats the bits of
 * the uninterrupted one.
 * Layout (host arrays, column-major and tight, one column per section):
 *   hyp      nhyp x nsec: section s at hyp + s * nhyp, (lx, ly, sig) -- (lx, ly, p, sig) for family D
 *   xtrain, ytrain  n0 x nsec;  alpha  2 n0 x nsec (column s = Ky_s^-1 ztrain_s: what sgpr_fit_batch returns, stacked)
 *   hypp     nhypp x nsec;  xtrainp, ytrainp, alphap  n0p x nsec: the regular GPs of the first guess.  With
 *            SGPR_MAP_EXPLICIT they are ignored (n0p treated as 0) and may be NULL
 *   Q0, P0   ntest;  qmap, pmap, pdiff (may be NULL)  [nm][ntest] C-ordered, row 0 = the start points
 * Checked before any device call (SGPR_E_ARG): nsec < 1, first outside [0, nsec), nm < 1, negative ntest / n0 / n0p, an
 * unknown mode bit, SGPR_MAP_EXPLICIT | SGPR_MAP_LOSS_NEGP, a null required pointer, an unknown family, a wrong nhyp / nhypp
 * for the family.  Then SGPR_E_NODEVICE without a device; ntest == 0 returns 0; nm == 1 writes the start row only.
 * Added in ABI 5 (additional entry point). */
int sgpr_applymap_sections_host(int family, int mode, int nsec, int first, int nm, int ntest,
                                const double *hyp, int nhyp, int n0, const double *xtrain, const double *ytrain,
                                const double *alpha, const double *hypp, int nhypp, int n0p, const double *xtrainp,
                                const double *ytrainp, const double *alphap, const double *Q0, const double *P0,
                                double *qmap, double *pmap, double *pdiff);
/* The sectioned map WITH ITS TANGENT MAP: the same orbits -- qmap, pmap and pdiff are bit-identical to
 * sgpr_applymap_sections_host, whose arguments, layout and checks this entry shares -- and the derivative of every step.  After
 * each accepted step (new P finite) one more pass over the section's training points sums the Hessian of its generating function
 * at (q, P): A = H_qq, B = H_qP, C = H_PP, three sums in one reduction.  With T = 1 / (1 + B) the Jacobian of the step
 * (q, p) -> (Q, P) is
 *     M = [ 1 + B - C T A    C T ]      rows (Q, P), columns (q, p),
 *         [     - T A         T  ]
 * of determinant 1 for any A, B, C; wrapping q does not change it.  The outputs have the layout of
 * sgpr_applymap_nd_tangent_host at d = 1:
 * jac  (may be NULL): [nm-1][ntest][2][2] doubles, C order: M of every step (step i belongs to section (first + i) mod nsec).
 * mono (may be NULL): [ntest][2][2] = M_{nm-1} ... M_1, the identity for nm = 1 (Greene's residue (2 - tr mono) / 4 of a
 *      periodic field line).
 * lyap (may be NULL): [ntest][2] finite-time Lyapunov exponents by Benettin's method (Z = M Qmat, modified Gram-Schmidt in column
 *      order, log |r_cc| summed per column, divided by nm - 1).  The orthonormal basis lives inside one call: a run split into
 *      several calls takes its exponents from the calls' jac (maps.tangent_from_jac).
 * From the step at which an orbit is lost its jac rows are NaN, and so are its mono and lyap; so is the jac row of a step whose
 * 1 + B is 0 or not finite, with mono and lyap (the orbit itself goes on).  An orbit's outputs depend on nothing but its own
 * start point, `first` and the sections.
 * On top of the plain entry's checks (SGPR_E_ARG before any device call): SGPR_MAP_WRAP_P (the implicit half and the q half
 * would sit at different points and need two Hessians; no driver of the sectioned map wraps P); SGPR_MAP_EXPLICIT with a
 * product family (accepted for the sum kernels -- family B, or a USER sum kernel -- where B = 0, A depends on q and C on P
 * only); lyap != NULL with nm < 2.  Then SGPR_E_NODEVICE without a device; ntest == 0 returns 0; nm == 1 writes the start row
 * and mono = identity.
 * Added in ABI 5 (additional entry point). */
int sgpr_applymap_sections_tangent_host(int family, int mode, int nsec, int first, int nm, int ntest,
                                        const double *hyp, int nhyp, int n0, const double *xtrain, const double *ytrain,
                                        const double *alpha, const double *hypp, int nhypp, int n0p, const double *xtrainp,
                                        const double *ytrainp, const double *alphap, const double *Q0, const double *P0,
                                        double *qmap, double *pmap, double *pdiff, double *jac, double *mono, double *lyap);
/* The sectioned map BACKWARDS (with nsec == 1: the one-pair map of sgpr_applymap_host backwards): row 0 of qmap / pmap is a point
 * (Q, P), row i its i-th preimage, all nm - 1 backward steps of all ntest orbits in ONE launch.  The forward step of a section
 * passes through the point (q, P): with r1, r2 = Kstar(1,:).alpha, Kstar(2,:).alpha at (q, P) it solves p = P + r1 for P and sets
 * Q = q + r2.  The backward step passes through the same point with the roles swapped: P is known, it solves
 *     g(q) = q + r2(q, P) - Q = 0   for q,   then   p = P + r1(q, P),
 * by the forward map's secant without a first-guess GP: q0 = Q, q1 = q0 - g(q0), at most 60 updates, stopped when
 * |q1 - q0| <= 1e-13 max(1, |q1|), when g(q1) is not finite or when g(q1) == g(q0).  The step is accepted when g(q1) is finite
 * and |g(q1)| <= 1e-8 max(1, |Q|) (the forward rule with the roles swapped); the r1 of the last residual gives p.  Otherwise the
 * orbit is lost: NaN in q and p from that row on.  A NaN or infinite start value loses that orbit and no other.
 * Section order: step i (row i -> row i + 1) undoes section (first - i) mod nsec; `first` is the section whose forward step
 * produced row 0 -- from the last row of a forward call of nm rows that began with `first_f`, first = (first_f + nm - 2) mod nsec.
 * A run continued from row i with first' = (first - i) mod nsec repeats the bits of the uninterrupted one.
 * mode: SGPR_MAP_WRAP_Q (the solved q mod 2 pi: the preimage of a wrapped orbit) | SGPR_MAP_LOSS_NEGP (a step whose solved p < 0
 * loses the orbit: the backward twin of the forward "new momentum < 0"; row 0 is not tested).
 * Layout as sgpr_applymap_sections_host without the guess GPs and without pdiff (SGPR_MAP_WRAP_P is refused, so the unwrapped
 * momentum is pmap itself): hyp nhyp x nsec, xtrain / ytrain n0 x nsec, alpha 2 n0 x nsec, column-major and tight; Q0, P0 ntest;
 * qmap, pmap [nm][ntest] C-ordered, row 0 = the start points.  iters (may be NULL): [nm-1][ntest] ints, the secant updates of each
 * step (the residual evaluations beyond the two starting ones), -1 for a lost step.
 * One 256-thread workgroup per orbit at every n0; no workgroup waits for another.  The sections are staged in LDS when
 * nsec * 4 n0 <= 8960 doubles and read from memory otherwise, with the same bits either way.  An orbit's bits depend on nothing
 * but its own start point, `first` and the sections.
 * Checked before any device call (SGPR_E_ARG): nsec < 1, first outside [0, nsec), nm < 1, negative ntest / n0, an unknown mode
 * bit, SGPR_MAP_WRAP_P (the two halves of a wrapped step sit at different P), SGPR_MAP_EXPLICIT (as for the d-pair inverse), a
 * null required pointer, an unknown family, a wrong nhyp for the family.  Then SGPR_E_NODEVICE without a device; ntest == 0
 * returns 0; nm == 1 writes the start row only.  There is no tangent form: the Jacobian of a backward step is the symplectic
 * inverse of the forward step matrix at the same (q, P), which sgpr_applymap_sections_tangent_host returns for one step from the
 * preimage.
 * Added in ABI 5 (additional entry point). */
int sgpr_applymap_sections_inverse_host(int family, int mode, int nsec, int first, int nm, int ntest,
                                        const double *hyp, int nhyp, int n0, const double *xtrain, const double *ytrain,
                                        const double *alpha, const double *Q0, const double *P0, double *qmap, double *pmap,
                                        int *iters);
/* The symplectic map of a fit with d canonical pairs (d = 1, 2, 3), nm - 1 steps for ntest orbits with every step on the
 * device: one workgroup per orbit, no workgroup waits on another.  With x = (q_1..q_d, P_1..P_d) and G(x) = K*(x) alpha (what
 * sgpr_fit_predict_nd returns: G_q = dF/dq = p - P, G_P = dF/dP = Q - q) a step solves
 *     f(P) = G_q(q, P) - p + P = 0   for P in R^d,   then   Q = q + G_P(q, P),
 * by Newton from P = p with the ANALYTIC Jacobian I + dG_q/dP (one pass over the training points sums G and the Jacobian
 * together; the d x d system in closed form).  It stops when max|dP| <= 1e-13 max(1, max|P|) or after 60 iterations (the
 * d = 1 map's tol and maxiter); one more pass at the final P gives G_P and the residual, and the step is accepted when
 * max|f| <= 1e-8 max(1, max|p|) (the d = 1 rule).  Otherwise -- also on a non-finite value or a singular Jacobian -- the orbit
 * is lost: NaN from that step on; an orbit that starts NaN stays NaN.
 * mode: SGPR_MAP_WRAP_Q (every q_i mod 2 pi after the update) | SGPR_MAP_EXPLICIT (P = p - G_q(q, p), no solve; the sum
 * kernels' maps); any other bit is SGPR_E_ARG.
 * Q0, P0: ntest x d column-major host arrays (ldq, ldp >= ntest).  qmap, pmap: [nm][ntest][d] doubles, C order, row 0 = the
 * start points.  iters (may be NULL): [nm-1][ntest], the Newton iterations of each solve, 0 in explicit mode, -1 for a lost
 * orbit.  An orbit's bits depend on nothing but its own start point: not on ntest, its index, or a repeated call.
 * 256 threads per orbit with the training points and alpha staged in LDS up to n0 = 1024, 512 threads reading them from
 * memory beyond.  One workgroup per orbit at every n0: the d = 1 kernel's teams of workgroups per orbit do not exist here.
 * Checked before any device call (SGPR_E_ARG): null handle or pointers (iters excepted), nm < 1, ntest < 0, ldq / ldp < ntest,
 * unknown mode bits -- and for the host form an unknown family, d outside 1..3, nhyp != 2d + 1 (3d + 1 with periods), n0 < 0,
 * ldx < n0.  ntest == 0 returns 0; nm == 1 writes the start row only.
 * sgpr_fit_applymap_nd: the training points and alpha of a solved sgpr_fit_create_nd / sgpr_fit_create fit (d = 1 fits run
 * the same kernel with D = 2); SGPR_E_STATE for an unsolved fit, a SGPR_FIT_REG fit and a SGPR_FIT_BLOCK_* fit.
 * sgpr_applymap_nd_host: the same from caller-supplied training points X (n0 x 2d column-major, ldx >= n0), alpha (2 d n0,
 * block by block like the rows of K) and hyp as sgpr_fit_create_nd takes it -- the counterpart of sgpr_applymap_host.
 * Added in ABI 5 (additional entry points). */
int sgpr_fit_applymap_nd(sgpr_fit_t f, int mode, int nm, int ntest, const double *Q0, size_t ldq,
                         const double *P0, size_t ldp, double *qmap, double *pmap, int *iters);
int sgpr_applymap_nd_host(int family, int d, int mode, int nm, int ntest, const double *hyp, int nhyp, int n0,
                          const double *X, size_t ldx, const double *alpha, const double *Q0, size_t ldq,
                          const double *P0, size_t ldp, double *qmap, double *pmap, int *iters);
/* The d-pair map WITH ITS TANGENT MAP: the same orbits -- qmap, pmap and iters are bit-identical to sgpr_fit_applymap_nd /
 * sgpr_applymap_nd_host, whose arguments and checks these entries share -- and the derivative of every step.  After each
 * accepted step one more pass over the training points sums the Hessian H = dG/dx of the generating function at (q, P), one sum
 * per unordered pair of coordinates (H is symmetric by construction); with A = H_qq, B = H_qP, C = H_PP and T = (I + B)^-1 (d x d,
 * closed form) the Jacobian of the step (q, p) -> (Q, P) is
 *     M = [ I + B^T - C T A    C T ]      rows (Q_1..Q_d, P_1..P_d), columns (q_1..q_d, p_1..p_d),
 *         [      - T A          T  ]
 * symplectic (M^T J M = J) for any symmetric A and C; wrapping q does not change it.
 * jac  (may be NULL): [nm-1][ntest][2d][2d] doubles, C order: M of every step.
 * mono (may be NULL): [ntest][2d][2d] = M_{nm-1} ... M_1, the identity for nm = 1 (linear stability of a periodic orbit: Greene's
 *      residue (2 - tr mono) / 4 at d = 1).
 * lyap (may be NULL): [ntest][2d] finite-time Lyapunov exponents by Benettin's method: Z = M Qmat, modified Gram-Schmidt on the
 *      columns of Z in column order, log |r_cc| summed per column, divided by nm - 1 (per step of the map, Gram-Schmidt order).
 * From the step at which an orbit is lost its jac rows are NaN, and so are its mono and lyap; so is the jac row of a step whose
 * I + B is singular, with mono and lyap (the orbit itself goes on).  An orbit's outputs depend on nothing but its own start point.
 * SGPR_MAP_EXPLICIT is accepted for the sum kernels only (family B, or a USER sum kernel: B = 0, A depends on q and C on P
 * only); with a product family it is SGPR_E_ARG here, as is lyap != NULL with nm < 2.  Everything else as for the plain
 * entries: the same SGPR_E_ARG checks before any device call, SGPR_E_STATE in the same cases, ntest == 0 returns 0.
 * Added in ABI 5 (additional entry points). */
int sgpr_fit_applymap_nd_tangent(sgpr_fit_t f, int mode, int nm, int ntest, const double *Q0, size_t ldq,
                                 const double *P0, size_t ldp, double *qmap, double *pmap, int *iters,
                                 double *jac, double *mono, double *lyap);
int sgpr_applymap_nd_tangent_host(int family, int d, int mode, int nm, int ntest, const double *hyp, int nhyp, int n0,
                                  const double *X, size_t ldx, const double *alpha, const double *Q0, size_t ldq,
                                  const double *P0, size_t ldp, double *qmap, double *pmap, int *iters,
                                  double *jac, double *mono, double *lyap);
/* The d-pair map BACKWARDS: row 0 of qmap / pmap is a point (Q, P), row i its i-th preimage under the map of sgpr_fit_applymap_nd /
 * sgpr_applymap_nd_host (mode without SGPR_MAP_EXPLICIT).  The forward step passes through x = (q, P); so does the backward
 * one, with P known and q unknown: it solves
 *     f(q) = q + G_P(q, P) - Q = 0   for q in R^d,   then   p = P + G_q(q, P),
 * by Newton from q = Q with the analytic Jacobian I + dG_P/dq.  G is the gradient of the generating function, so dG_P/dq is the
 * TRANSPOSE of the dG_q/dP block the forward solve uses: the same pass over the training points, the same 2d + d^2 sums, the same
 * closed-form d x d solve on the transposed block.  It stops when max|dq| <= 1e-13 max(1, max|q|) or after 60 iterations; one
 * more pass at the final q gives G_q and the residual, and the step is accepted when max|f| <= 1e-8 max(1, max|Q|) (the forward
 * rule with the roles swapped).  Otherwise -- also on a non-finite value or a singular Jacobian -- the orbit is lost: NaN from
 * that step on; an orbit that starts NaN stays NaN.  The sum kernels' G_P does not depend on q: one exact Newton step.
 * mode: SGPR_MAP_WRAP_Q (every solved q_i mod 2 pi: the preimage of a wrapped orbit, as the forward map wraps Q) or 0.
 * SGPR_MAP_EXPLICIT is SGPR_E_ARG for every family: the explicit product-family map P = p - G_q(q, p) evaluates G at (q, p),
 * not at (q, P), so its inverse needs a second solve (in p) that is not built; the sum kernels' explicit and implicit maps
 * coincide, so mode 0 inverts them already.  Any other bit is SGPR_E_ARG as well.
 * Arguments, shapes, checks, states and thread counts as the forward pair: Q0, P0 ntest x d column-major (ldq, ldp >= ntest);
 * qmap, pmap [nm][ntest][d]; iters (may be NULL) [nm-1][ntest], -1 for a lost orbit; ntest == 0 returns 0, nm == 1 writes the
 * start row only; an orbit's bits depend on nothing but its own start point.  There is no tangent form: the Jacobian of a
 * backward step is the symplectic inverse -J M^T J of the forward step matrix M at the same (q, P), which
 * sgpr_*_applymap_nd_tangent returns for one step from the preimage.
 * Added in ABI 5 (additional entry points). */
int sgpr_fit_applymap_nd_inverse(sgpr_fit_t f, int mode, int nm, int ntest, const double *Q0, size_t ldq,
                                 const double *P0, size_t ldp, double *qmap, double *pmap, int *iters);
int sgpr_applymap_nd_inverse_host(int family, int d, int mode, int nm, int ntest, const double *hyp, int nhyp, int n0,
                                  const double *X, size_t ldx, const double *alpha, const double *Q0, size_t ldq,
                                  const double *P0, size_t ldp, double *qmap, double *pmap, int *iters);
/* PERIODIC ORBITS of the d-pair map: for each of ntest guesses z = (q, p) = row of (Q0, P0), a period n >= 1 and d integer
 * winding numbers w, find z* with
 *     r(z) = ( q_n - q_0 - 2 pi w,  p_n - p_0 ) = 0,      (q_n, p_n) the n-th image of z under the map of sgpr_fit_applymap_nd /
 * sgpr_applymap_nd_host in lifted (unwrapped) coordinates, by plain Newton on the n-fold map, z <- z - (mono(z) - I)^-1 r(z) with
 * mono = M_n ... M_1 from the tangent map (sgpr_*_applymap_nd_tangent); no damping, no line search.  One workgroup per guess
 * runs ALL passes of that guess inside one launch: a pass is the n steps of the map -- the step of the map entries itself, not a
 * copy -- with the Hessian pass and the monodromy product of the tangent entries, then the 2d x 2d solve by Gaussian elimination
 * with partial pivoting.  A guess is CONVERGED when the pass that started from the current z has
 * max|r| <= tol max(1, max|z|); that z is returned, so resid is the residual evaluated at the returned point.  A guess FAILS
 * when maxit passes go by without convergence, when its orbit is lost (the map's NaN rule), when a step's I + B is singular, when
 * mono - I is singular (a zero or non-finite pivot) or the update is not finite.  A failed guess, and one that starts non-finite,
 * has NaN in every floating output and its = -1; the other guesses are not affected.
 * mode: as the tangent entries -- SGPR_MAP_WRAP_Q, and SGPR_MAP_EXPLICIT for the sum kernels only.  With SGPR_MAP_WRAP_Q the turns
 * the map takes out of every Q are counted and the q-residual is (Q_n - q_0) + 2 pi (turns - w); every updated q_0 is wrapped
 * into [0, 2 pi) (a first guess that converges at once is returned as given).  Without it the residual is Q_n - q_0 - 2 pi w: a
 * periodic family run unwrapped is a legitimate lifted map.  There is nothing for SGPR_MAP_WRAP_P.
 * wind (may be NULL = all 0): ntest x d ints, column-major, leading dimension ntest.  Q0, P0: ntest x d column-major (ldq, ldp >=
 * ntest).  z: [ntest][2d] = (q*, p*).  resid: [ntest] = max|r(z*)|.  its: [ntest], the passes run, the converged one included
 * (1 = the guess was a periodic orbit already).  mono (may be NULL): [ntest][2d][2d], the monodromy of the returned orbit
 * (rows (Q, P), columns (q, p)).  qorb, porb (both or neither NULL): [n][ntest][d], rows 0 .. n-1 of the returned orbit, row 0 =
 * z; they have the bits sgpr_*_applymap_nd returns from z.  A guess's bits depend on nothing but its own inputs: not on ntest,
 * its index, or a repeated call.  Threads per workgroup as the map entries (256 staged in LDS up to n0 = 1024, 512 beyond).
 * HAZARD: far from the training data the GP returns its prior mean, the learned map is the identity, and every far point is a
 * "fixed point" with mono = I to rounding; Newton can walk there from a poor guess and report convergence.  Discard results whose
 * mono - I is negligible.
 * Checked before any device call (SGPR_E_ARG): everything the map entries check (n in the place of nm), n < 1, maxit < 1, tol
 * not positive or not finite, null z, resid or its, one of qorb / porb without the other, SGPR_MAP_EXPLICIT with a product
 * family.  SGPR_E_STATE as sgpr_fit_applymap_nd_tangent: an unsolved fit, a SGPR_FIT_REG fit, a SGPR_FIT_BLOCK_* fit.
 * ntest == 0 returns 0.  Added in ABI 5 (additional entry points). */
int sgpr_fit_periodic_nd(sgpr_fit_t f, int mode, int n, int ntest, const int *wind, const double *Q0, size_t ldq,
                         const double *P0, size_t ldp, double tol, int maxit, double *z, double *resid, int *its,
                         double *mono, double *qorb, double *porb);
int sgpr_periodic_nd_host(int family, int d, int mode, int n, int ntest, const double *hyp, int nhyp, int n0,
                          const double *X, size_t ldx, const double *alpha, const int *wind, const double *Q0, size_t ldq,
                          const double *P0, size_t ldp, double tol, int maxit, double *z, double *resid, int *its,
                          double *mono, double *qorb, double *porb);
/* alpha-solve on device with the factor and its leaf inverses: b (n) := L^-T L^-1 b */
int sgpr_potrs_vec_dev(int n, const double *L, size_t ldl, void *work, double *b,
                       void *stream);

/* Per-launch HIP-event timing of the MFMA GEMM kernel between begin and end (measurement
 * aid for bench.py's roofline pass; not part of the reference's interface).  Events come from a
 * fixed pool (8192 launches per window; further launches are counted, not timed).
 * out12: [0..2] launches / algorithmic flop / ms of the 256x128-tile kernel for launches that had
 * the device to themselves, [3..5] all launches of the smaller tile shapes, [6..7] flop / ms of the
 * single largest launch, [8..10] 256x128-tile launches issued by the look-ahead driver (two streams
 * share the chip, their durations overlap), [11] launches beyond the pool. */
int sgpr_profile_begin(void);
int sgpr_profile_end(double *out12);
/* per-launch records of the window closed by the last sgpr_profile_end: 7 doubles each
 * (m, n, k, lower, big-tile flag, ms, overlap flag); returns the number of records available */
int sgpr_profile_launches(double *buf, int max_records);

#ifdef __cplusplus
}
#endif
#endif
