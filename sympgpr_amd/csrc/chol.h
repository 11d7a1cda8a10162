// chol.h -- internal: what the pieces of the Cholesky factorisation need of each other.  chol.hip: recursion, look-ahead
// driver, potrf(); cholq.hip: the task-queue driver; solve.hip: the triangular solves; panel.hip / panel.h: the leaf kernel and
// the persistent panel kernel; streams.hip / streams.h: streams and events; chol_plan.hip / chol_plan.h: the host arithmetic.
#pragma once
#include "common.h"
#include "strassen.h"
#include "chol_plan.h"

namespace sgpr {

static_assert(cplan::LEAF_ORDER == LEAF, "the planner's leaf order is the kernels'");

struct Ctx {
    double *inv;   // leaf inverses: leaf t at inv + t * LEAF * LEAF
    int *dinfo;
    hipStream_t st;
    int la_max = 0;   // potrf_rec hands blocks of order <= la_max to the look-ahead driver (0: never)
    int *flags = nullptr;   // hand-off flags of the panel kernel: PFLAG_STRIDE ints per leaf column, zeroed by potrf()
    void *qws = nullptr;    // the task-queue driver's part of the workspace (cholq.h), or null
    bool strassen = false;  // the deep products of the recursion go through gemm_nt_strassen (potrf() only: the solves' do not)
    StrassenRec rec;        // ... each with thresholds of its own, chosen per call from these (strassen_rec_cfg)
    StrassenTop top;        // ... and the two largest with a third level on top (strassen_top_gemm)
};

// ---- chol.hip
int potrf_lookahead(int n, double *A, size_t lda, const Ctx &c, int nb, int off0);
// B (m x n) := B L^-T through the leaf inverses (off: global index of L's first row, a multiple of LEAF)
int trsm_rec(int m, int n, const double *L, size_t ldl, double *B, size_t ldb, int off, const Ctx &c);
void potrf_clear_queue_mark();   // cholq.hip: every potrf() clears the calling thread's "went through the queue" mark

// ---- cholq.hip: returns 1 when the queue form cannot be used here (the caller falls back to the look-ahead driver), < 0 on errors
int potrf_queue(int n, double *A, size_t lda, const Ctx &c, int off0);

}  // namespace sgpr
