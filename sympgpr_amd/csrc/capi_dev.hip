// capi_dev.hip -- the device-pointer primitives of libsympgpr_hip.so (*_dev), their argument checks and the size queries
#include <algorithm>
#include <cmath>
#include "capi_util.h"

using namespace sgpr;

// Shape / pointer checks of the *_dev entries, answered before need_device(): an argument error is SGPR_E_ARG on any
// machine, with or without a device, and the message names the entry point.
static int dev_arg_error(const char *entry, const char *what)
{
    set_error(std::string(entry) + ": " + what);
    return SGPR_E_ARG;
}

// the leading-dimension rules gemm_launch (gemm_f64.hip) enforces, for an (m x k) A, B (n x k) or, transb, (k x n), C (m x n)
static int gemm_args(const char *entry, int m, int n, int k, const double *A, size_t lda, const double *B, size_t ldb,
                     const double *C, size_t ldc, int transb)
{
    if (m < 0 || n < 0 || k < 0) return dev_arg_error(entry, "negative extent");
    if (m == 0 || n == 0) return 0;
    if (lda < (size_t)m || ldb < (size_t)(transb ? k : n) || ldc < (size_t)m) return dev_arg_error(entry, "leading dimension too small");
    if (!C || (k > 0 && (!A || !B))) return dev_arg_error(entry, "null pointer");
    return 0;
}

// triangular solves against an (n x n) factor: B (m x n), ld >= extent, no null pointer behind a non-zero extent
static int trsm_args(const char *entry, int m, int n, const double *L, size_t ldl, const double *B, size_t ldb, const void *work)
{
    if (m < 0 || n < 0) return dev_arg_error(entry, "negative extent");
    if (m == 0 || n == 0) return 0;
    if (ldl < (size_t)n) return dev_arg_error(entry, "ldl < n");
    if (ldb < (size_t)m) return dev_arg_error(entry, "ldb < m");
    if (!L || !B || !work) return dev_arg_error(entry, "null pointer");
    return 0;
}

static int vec_solve_args(const char *entry, int n, const double *L, size_t ldl, const void *work, const double *b, bool need_b)
{
    if (n < 0) return dev_arg_error(entry, "n < 0");
    if (n == 0) return 0;
    if (ldl < (size_t)n) return dev_arg_error(entry, "ldl < n");
    if (!L || !work || (need_b && !b)) return dev_arg_error(entry, "null pointer");
    return 0;
}

extern "C" {

int sgpr_gram_pairs_dev(int family, int mi, int mj, const double *xb, const double *yb,
                        const double *xa, const double *ya, const double *hyp, int nhyp, double *qq,
                        double *Pq, double *qP, double *PP, size_t ld, long diag_off, double noise,
                        unsigned flags, void *stream)
{
    int rc = need_device();
    if (rc) return rc;
    KConst kc;
    if ((rc = make_kconst(family, hyp, nhyp, &kc))) return rc;
    return gram_pairs(family, mi, mj, xb, yb, xa, ya, kc, qq, Pq, qP, PP, ld, diag_off, std::fabs(noise),
                      flags, static_cast<hipStream_t>(stream));
}

int sgpr_gram_reg_dev(int family, int mi, int mj, const double *xb, const double *yb, const double *xa,
                      const double *ya, const double *hyp, int nhyp, double *G, size_t ld,
                      long diag_off, double noise, void *stream)
{
    int rc = need_device();
    if (rc) return rc;
    KConst kc;
    if ((rc = make_kconst(family, hyp, nhyp, &kc))) return rc;
    return gram_reg(family, mi, mj, xb, yb, xa, ya, kc, G, ld, diag_off, std::fabs(noise),
                    static_cast<hipStream_t>(stream));
}

int sgpr_gram_nd_dev(int family, int d, int mi, int mj, const double *Xb, size_t ldxb, const double *Xa,
                     size_t ldxa, const double *hyp, int nhyp, double *K, size_t ld, size_t rstride,
                     size_t cstride, long diag_off, double noise, void *stream)
{
    if (mi > 0 && mj > 0) {
        if (ld < (size_t)mi) return dev_arg_error("sgpr_gram_nd_dev", "ld < mi");
        if (ldxb < (size_t)mi) return dev_arg_error("sgpr_gram_nd_dev", "ldxb < mi");
        if (ldxa < (size_t)mj) return dev_arg_error("sgpr_gram_nd_dev", "ldxa < mj");
    }
    int rc = need_device();
    if (rc) return rc;
    return gram_nd(family, d, mi, mj, Xb, ldxb, Xa, ldxa, hyp, nhyp, K, ld, rstride, cstride, diag_off,
                   std::fabs(noise), static_cast<hipStream_t>(stream));
}

int sgpr_gram_nd_sel_dev(int family, int d, int mi, int mj, const double *Xb, size_t ldxb, const double *Xa,
                         size_t ldxa, const double *hyp, int nhyp, double *K, size_t ld, const long *roff,
                         const long *coff, void *stream)
{
    if (mi > 0 && mj > 0) {
        if (ld < (size_t)mi) return dev_arg_error("sgpr_gram_nd_sel_dev", "ld < mi");
        if (ldxb < (size_t)mi) return dev_arg_error("sgpr_gram_nd_sel_dev", "ldxb < mi");
        if (ldxa < (size_t)mj) return dev_arg_error("sgpr_gram_nd_sel_dev", "ldxa < mj");
    }
    int rc = need_device();
    if (rc) return rc;
    return gram_nd_sel(family, d, mi, mj, Xb, ldxb, Xa, ldxa, hyp, nhyp, K, ld, roff, coff, static_cast<hipStream_t>(stream));
}

size_t sgpr_potrf_workspace(int n) { return potrf_workspace(n); }
size_t sgpr_potrf_inverses_bytes(int n) { return n <= 0 ? 0 : (size_t)((n + LEAF - 1) / LEAF) * LEAF * LEAF * sizeof(double); }

int sgpr_family_has_p(int family) { return family_has_p(family) ? 1 : 0; }

int sgpr_potrf_dev(int n, double *A, size_t lda, void *work, size_t lwork, int *dinfo, void *stream)
{
    if (n < 0 || (n > 0 && lda < (size_t)n)) return dev_arg_error("sgpr_potrf_dev", "bad n / lda");
    if (lwork < potrf_workspace(n)) return dev_arg_error("sgpr_potrf_dev", "workspace too small");
    if (!work || !dinfo || (n > 0 && !A)) return dev_arg_error("sgpr_potrf_dev", "null pointer");
    int rc = need_device();
    if (rc) return rc;
    return potrf(n, A, lda, work, lwork, dinfo, static_cast<hipStream_t>(stream));
}

int sgpr_potrf_info_dev(int info, void *stream)
{
    if (info >= 0) return info;
    if (info == POTRF_HANDOFF_TIMEOUT) (void)potrf_queue_mark_failed(static_cast<hipStream_t>(stream));
    return info_status(info);
}

int sgpr_trsm_rlt_dev(int m, int n, const double *L, size_t ldl, double *B, size_t ldb,
                      const void *work, void *stream)
{
    int rc = trsm_args("sgpr_trsm_rlt_dev", m, n, L, ldl, B, ldb, work);
    if (rc || (rc = need_device())) return rc;
    return trsm_rlt(m, n, L, ldl, B, ldb, work, static_cast<hipStream_t>(stream));
}

int sgpr_gemm_nt_dev(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B,
                     size_t ldb, double beta, double *C, size_t ldc, int lower, long diag_off,
                     void *stream)
{
    int rc = gemm_args("sgpr_gemm_nt_dev", m, n, k, A, lda, B, ldb, C, ldc, 0);
    if (rc || (rc = need_device())) return rc;
    return gemm_nt(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, lower, diag_off,
                   static_cast<hipStream_t>(stream));
}

int sgpr_gemm_nt_bc_dev(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B,
                        size_t ldb, double beta, double *C, size_t ldc, int blk, int pr, int pi, int pc,
                        int pj, void *stream)
{
    if (blk < 1 || pr < 1 || pc < 1) return dev_arg_error("sgpr_gemm_nt_bc_dev", "bad block-cyclic descriptor");
    int rc = gemm_args("sgpr_gemm_nt_bc_dev", m, n, k, A, lda, B, ldb, C, ldc, 0);
    if (rc || (rc = need_device())) return rc;
    const int bc[5] = {blk, pr, pi, pc, pj};
    return gemm_nt_bc(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, 1, bc, static_cast<hipStream_t>(stream));
}

int sgpr_trsv_dev(int n, const double *L, size_t ldl, void *work, double *b, int trans, void *stream)
{
    int rc = vec_solve_args("sgpr_trsv_dev", n, L, ldl, work, b, true);
    if (rc || (rc = need_device())) return rc;
    return trsv(n, L, ldl, work, b, trans, static_cast<hipStream_t>(stream));
}

int sgpr_gemv_sub_dev(int trans, int m, int k, const double *A, size_t lda, const double *x, double *y,
                      void *stream)
{
    if (m < 0 || k < 0 || (m > 0 && lda < (size_t)m)) return dev_arg_error("sgpr_gemv_sub_dev", "bad shape");
    if (m > 0 && k > 0 && (!A || !x || !y)) return dev_arg_error("sgpr_gemv_sub_dev", "null pointer");
    int rc = need_device();
    if (rc) return rc;
    return trans ? gemv_t_sub(m, k, A, lda, x, y, static_cast<hipStream_t>(stream))
                 : gemv_n_sub(m, k, A, lda, x, y, static_cast<hipStream_t>(stream));
}

int sgpr_gemm_nn_dev(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb,
                     double beta, double *C, size_t ldc, void *stream)
{
    int rc = gemm_args("sgpr_gemm_nn_dev", m, n, k, A, lda, B, ldb, C, ldc, 1);
    if (rc || (rc = need_device())) return rc;
    return gemm_nn(m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, static_cast<hipStream_t>(stream));
}

int sgpr_trsm_rl_dev(int m, int n, const double *L, size_t ldl, double *B, size_t ldb, const void *work, void *stream)
{
    int rc = trsm_args("sgpr_trsm_rl_dev", m, n, L, ldl, B, ldb, work);
    if (rc || (rc = need_device())) return rc;
    return trsm_rl(m, n, L, ldl, B, ldb, work, static_cast<hipStream_t>(stream));
}

namespace sgpr { namespace {
// cnt blocks of rows x cols doubles, block i from src + i * sstep (leading dimension lds) to dst + i * dstep (ldd): the panel
// packing / regrouping copies of the block-cyclic driver in one launch (rows fastest: 512-byte runs per wave)
__global__ __launch_bounds__(256) void copy_blocks_kernel(int rows, int cols, int cnt, const double *src, size_t lds, size_t sstep,
                                                          double *dst, size_t ldd, size_t dstep)
{
    const int i = blockIdx.z;
    const double *s = src + (size_t)i * sstep;
    double *d = dst + (size_t)i * dstep;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    for (int c = blockIdx.y; c < cols; c += gridDim.y) d[(size_t)r + (size_t)c * ldd] = s[(size_t)r + (size_t)c * lds];
}
} }

int sgpr_copy_blocks_dev(int rows, int cols, int cnt, const double *src, size_t lds, size_t sstep, double *dst, size_t ldd,
                         size_t dstep, void *stream)
{
    if (rows < 0 || cols < 0 || cnt < 0 || (rows > 0 && (lds < (size_t)rows || ldd < (size_t)rows)))
        return dev_arg_error("sgpr_copy_blocks_dev", "bad shape");
    const bool empty = rows == 0 || cols == 0 || cnt == 0;
    if (!empty && cnt > 65535) return dev_arg_error("sgpr_copy_blocks_dev", "more than 65535 blocks");
    if (!empty && (!src || !dst)) return dev_arg_error("sgpr_copy_blocks_dev", "null pointer");
    int rc = need_device();
    if (rc) return rc;
    if (empty) return 0;
    const dim3 grid((unsigned)((rows + 255) / 256), (unsigned)std::min(cols, 1024), (unsigned)cnt);
    hipLaunchKernelGGL(sgpr::copy_blocks_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), rows, cols, cnt, src, lds, sstep,
                       dst, ldd, dstep);
    SGPR_CHECK_LAUNCH();
    return 0;
}

int sgpr_predict_rows_dev(int family, int m, const double *q, const double *P, int n0, const double *xtrain,
                          const double *ytrain, const double *hyp, int nhyp, const double *alpha,
                          double *out_p, double *out_q, void *stream)
{
    int rc = need_device();
    if (rc) return rc;
    KConst kc;
    if ((rc = make_kconst(family, hyp, nhyp, &kc))) return rc;
    return predict_rows(family, m, q, P, n0, xtrain, ytrain, kc, alpha, out_p, out_q,
                        static_cast<hipStream_t>(stream));
}

int sgpr_predict_nd_dev(int family, int d, int m, const double *Xt, size_t ldxt, int n0, const double *Xtrain,
                        size_t ldxtr, const double *hyp, int nhyp, const double *alpha, double *out, void *stream)
{
    if (m > 0 && ldxt < (size_t)m) return dev_arg_error("sgpr_predict_nd_dev", "ldxt < m");
    if (m > 0 && n0 > 0 && ldxtr < (size_t)n0) return dev_arg_error("sgpr_predict_nd_dev", "ldxtr < n0");
    int rc = need_device();
    if (rc) return rc;
    return predict_nd(family, d, m, Xt, ldxt, n0, Xtrain, ldxtr, hyp, nhyp, alpha, out, static_cast<hipStream_t>(stream));
}

int sgpr_predict_reg_dev(int family, int m, const double *q, const double *P, int n0, const double *xtrain,
                         const double *ytrain, const double *hyp, int nhyp, const double *alpha,
                         double *out, void *stream)
{
    int rc = need_device();
    if (rc) return rc;
    KConst kc;
    if ((rc = make_kconst(family, hyp, nhyp, &kc))) return rc;
    return predict_reg(family, m, q, P, n0, xtrain, ytrain, kc, alpha, out, static_cast<hipStream_t>(stream));
}

int sgpr_potrs_vec_dev(int n, const double *L, size_t ldl, void *work, double *b, void *stream)
{
    int rc = vec_solve_args("sgpr_potrs_vec_dev", n, L, ldl, work, b, true);
    if (rc || (rc = need_device())) return rc;
    return potrs_vec(n, L, ldl, work, b, static_cast<hipStream_t>(stream));
}

int sgpr_solve_status_dev(int n, const double *L, size_t ldl, const void *work, void *stream)
{
    int rc = vec_solve_args("sgpr_solve_status_dev", n, L, ldl, work, nullptr, false);
    if (rc || (rc = need_device())) return rc;
    return solve_status(n, L, ldl, work, static_cast<hipStream_t>(stream));
}

}  // extern "C"
