/*
 * sympgpr_probe.h -- C ABI of libsympgpr_probe.so: roofline calibration probes and kernel
 * diagnostics for the MI355X build of SympGPR's training core.  MEASUREMENT AIDS ONLY: nothing
 * here replaces an interface of the reference, a maintainer binding include/sympgpr_hip.h never
 * loads this library, and no product path calls it (tools/ and bench.py's calibration do).
 * Same conventions as sympgpr_hip.h (0 = ok, < 0 = SGPR_E_*).
 */
#ifndef SYMPGPR_PROBE_H
#define SYMPGPR_PROBE_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* a register-only fp64 MFMA issue loop with
 * `waves_per_simd` waves on every SIMD, and a streaming 16-B/lane write of `bytes` bytes. */
int sgpr_probe_mfma_f64(int waves_per_simd, int iters, double *tflops);
int sgpr_probe_hbm_write(size_t bytes, int reps, double *gbs);
/* out3: TFLOP/s, shader cycles per MFMA per SIMD, shader clock (GHz) held during the loop */
int sgpr_probe_mfma_clock(int nacc, int waves_per_simd, int iters, double *out3);
/* one synthetic C -= A B^T with per-workgroup stamps: TFLOP/s, median k-loop cycles per
 * workgroup, median shader clock (GHz), k-steps per workgroup */
int sgpr_probe_gemm(int m, int n, int k, int lower, double *out4);
/* switches for the following sgpr_probe_gemm calls OF THIS THREAD (nothing in the product library
 * changes): 8 = 128x128 tile shape, 16 = register-staged body; 0 = normal */
int sgpr_probe_gemm_debug(int bits);
/* shader cycles per phase of one 128x128 leaf factorisation: load, diag block, panel rows,
 * trailing update, write-back, inverse diag, inverse rows, final store */
int sgpr_probe_leaf(double *out8);
/* cycles per step of eight dependent micro-sequences on one wave (the building blocks of the leaf's diagonal-block step) */
int sgpr_probe_lat(double *out8);
/* HW_REG_XCC_ID of each workgroup of a 1-D grid of 512-thread blocks (checks the tile map's `id % 8`) */
int sgpr_probe_xcc(int nblocks, int *host_out);
/* the same on a stream restricted by a CU mask (hipExtStreamCreateWithCUMask): out[2b] = XCC id, out[2b+1] = HW_ID */
int sgpr_probe_cumask(const unsigned *mask_words, int nwords, int nblocks, int *host_out);

/* The OUTPUT OF THE CODE GENERATOR (tools/gen_kernels.py -> csrc/generated/pair_generated.h), evaluated as
 * it stands: out[i] = f(xa[i], ya[i], xb[i], yb[i], l...) without the sig factor; `which` as in
 * sgpr_kernel_eval_host (0..3 = k, d2k/dxdx0, d2k/dydy0, d2k/dxdy0; | 4: d/dlx; | 8: d/dly).  The product
 * library's hand-optimised kernels are diffed against this in tests/test_gpu_generated.py. */
int sgpr_probe_generated_eval(int family, int which, int m, const double *xa, const double *ya,
                              const double *xb, const double *yb, const double *l, int nl, double *out);

/* The task-queue Cholesky (csrc/cholq.h).  Host only: the ordered task list the worker grid would run for order n
 * with `nworkers` workers: counts[0] = panels, counts[1] = tasks, counts[2] = the planner's estimate of the time in
 * us; starts_out (panels + 1 boundaries) and tasks_out (TWO words per task, cholq.h: word 0 = [31:30] type 0 = update
 * / 1 = rows-below solve, [29:21] panel, [20:11] row tile of 256, [10:0] column tile of 128; word 1 = [31:16] first,
 * [15:0] one-past-last 128-column block of L an update applies) are filled up to the given capacities (max_tasks in
 * tasks).  tests/test_queue_plan.py replays the list on the CPU. */
int sgpr_probe_queue_plan(int n, int nworkers, int *starts_out, int max_starts, unsigned *tasks_out, int max_tasks,
                          int *counts);
/* ... with the hand-over point: the queue factors panels 0 .. nq-1 only and leaves the block behind them (all their updates
 * applied) to the look-ahead driver; nq < 0: the default of this order (SGPR_Q_TAIL).  counts has FOUR entries here:
 * counts[3] = nq used. */
int sgpr_probe_queue_plan_partial(int n, int nworkers, int nq, int *starts_out, int max_starts, unsigned *tasks_out,
                                  int max_tasks, int *counts);
/* per-task time stamps of the queue factorisations that follow in this process (8 words per ticket: 100 MHz real
 * time at ticket drawn / inputs ready / published, then task word 1 << 32 | task word 0); _end copies them out and
 * switches the recording off again.  (words 4..7: ticket of the next task returned, out of the products, stores drained, write-back through.)  Behind the 8 * max_tasks ticket words: 2 words per worker workgroup (1024: place
 * = XCC id << 32 | HW_ID, start) and 4 per workgroup of every panel kernel (512 panels x 32: place, start, end, strip);
 * `out` holds 8 * max_tasks + 2048 + 65536 words.  Returns the capacity / the number of words copied. */
int sgpr_probe_queue_trace_begin(int max_tasks);
int sgpr_probe_queue_trace_end(unsigned long long *out, int max_tasks);
int sgpr_probe_queue_trace_clear(void);   /* zero the stamps between two factorisations */
/* state words of the last task-queue factorisation of this process on stderr (ticket head, abort word, the first
 * task / panel strip that gave up waiting, version counters); returns the abort word */
int sgpr_probe_queue_postmortem(int always);
/* TESTS ONLY: while on, every task-queue factorisation of this process gives up before it starts (the give-up word is raised and
 * the factor's info word set as by a hand-off that timed out) -- to exercise the callers' retry with the other driver */
int sgpr_probe_queue_force_giveup(int on);
/* Experiment knobs of the product library (they were SGPR_* environment variables up to round 3): set BEFORE the code that reads
 * them runs for the first time in the process; each is read once.  Task-queue Cholesky: q_w (panel width, 512), q_tail (rows left
 * to the look-ahead driver, 0), q_kcap, q_leaf_us / q_pair_us / q_fixed_us / q_band0_us (planner's cost model), q_pollcap (2),
 * q_slack (CUs left empty, 0), q_nosync, q_debug.  Look-ahead driver: la_panel (3 = persistent panel kernel, 1 / 2 / 0 the
 * multi-launch panels), la_t0 / la_t1 / la_t2 (width thresholds).  GEMM: gemm_small_tile, gemm_small_mb.  Batched fits:
 * batch_two_min (512), batch_below (workgroups for the strips below a panel's diagonal block, 0 = one per strip; read per call).
 * Block solves: trsm_chain (workgroups of the chain class, 0 = built-in), trsm_piece (tiles per stream ticket, 0 = built-in: 16 up
 * to 128 strips, 128 above; read per call). */
int sgpr_probe_tune(const char *name, double value);
/* The Strassen front end of the fp64 NT product (csrc/strassen.h: the record layouts; csrc/strassen_plan.hip: the planner; csrc/strassen.hip: the device path).  Host only: the list of operations one call
 * C -= A B^T (m x n x k; lower: the lower triangle of a square C) turns into, for a threshold `smin` (smallest half-size of m and n
 * that qualifies; k: half of it), a k slab `kslab` (< 0: the built-in values / tunables gemm_strassen_min, gemm_strassen_kslab)
 * and `scratch_doubles` of scratch.  16 words per record, word 0 = kind:
 *   1 sum:      [1] side (0: A, 1: B) [2] rows [3] cols [4] xr [5] xc [6] yr [7] yc [8] sign    scratch[side] = X + sign Y
 *   2 product:  [1] a_src (0: block of A at row [2], k column [3]; 1: the A scratch) [4] b_src [5] [6] likewise [7] m [8] n [9] k
 *               [10] [11] row, column of the first destination block of C [12] its sign [13] [14] [15] the second (sign 0: none)
 *   3 classical launch: [1] lower [2] ar [3] ac [4] br [5] bc [6] m [7] n [8] k [9] cr [10] cc
 * tests/test_strassen_plan_cpu.py replays the list in numpy.  *count = records of the plan; `out` is filled up to max_records. */
int sgpr_probe_strassen_plan(int m, int n, int k, int lower, long smin, long kslab, long scratch_doubles, long long *out,
                             int max_records, int *count);
/* the front end itself and the two-destination product (C = beta C + alpha A B^T, C2 += alpha2 A B^T) on device pointers.
 * Tunables: gemm_strassen_min (8192), gemm_strassen_kslab (16384), gemm_strassen_noscratch (1: the scratch allocation is
 * treated as failed, every product runs classically), la_max (orders above it take the recursive Cholesky driver). */
int sgpr_probe_gemm_strassen_dev(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb,
                                 double beta, double *C, size_t ldc, int lower, void *stream);
int sgpr_probe_gemm_nt2_dev(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb,
                            double beta, double *C, size_t ldc, double alpha2, double *C2, size_t ldc2, void *stream);
/* The outer Strassen level (csrc/strassen_plan.hip).  Host only: the list of one call with both levels.  Records of the inner level
 * (kinds 1 - 3 above, unchanged: a call the outer level does not apply to gives exactly sgpr_probe_strassen_plan's list) and
 *   4 outer sum:     layout of kind 1; the result goes to the OUTER scratch of that side
 *   5 outer product: layout of kind 2; operands are raw blocks or the outer scratch, [7] [8] [9] the half-size extents.  Not a
 *                    launch: the inner plan of an m x n x k product (sgpr_probe_strassen_plan) runs on these operands, each of its
 *                    products going to BOTH destination blocks (offsets inside them as the inner plan says, signs multiplied)
 * `smin2`: smallest half-size of m and n that takes the outer level; `kslab2`: its k slab -- whole slabs of exactly that many
 * columns take it, a shorter remainder of k goes through the inner level alone (< 0: the tunables gemm_strassen2_min (16384),
 * gemm_strassen2_kslab (32768)).  `scratch_doubles` covers the inner and the outer pair together.  Tunable
 * gemm_strassen2_noscratch: the outer pair's allocation is treated as failed (one level).  tools/strassen2_plan.py replays it. */
int sgpr_probe_strassen2_plan(int m, int n, int k, int lower, long smin, long kslab, long smin2, long kslab2, long scratch_doubles,
                              long long *out, int max_records, int *count);
/* count = 2 .. 4 destinations from one product (disjoint blocks, device pointers; the arrays themselves are host memory):
 * C[0] = beta C[0] + alpha[0] A B^T, C[d] += alpha[d] A B^T */
int sgpr_probe_gemm_nt4_dev(int m, int n, int k, const double *A, size_t lda, const double *B, size_t ldb, double beta, int count,
                            double *const *C, const size_t *ldc, const double *alpha, void *stream);
/* the last sgpr_applymap_host of this process: K*-row evaluations (residuals of the implicit equation + q updates) summed over
 * its orbits, and the number of workgroups that share one orbit for ntest orbits on n0 training points */
/* The recursive factorisation (potrf_rec / trsm_rec) gives each of its products thresholds of its own: tunables
 * rec_strassen_min_gemm / rec_strassen_min_syrk (inner threshold of trsm_rec's products / of the lower updates),
 * rec_strassen2_min_gemm / rec_strassen2_min_syrk (outer threshold), rec_strassen2_kslab_short (outer k slab of a call whose k is
 * below the long outer slab and at least this; 0: none); rec_strassen_kslab / rec_strassen2_kslab (inner and long outer k slab:
 * gemm_strassen_kslab / gemm_strassen2_kslab unless set).  Read at
 * every factorisation.  With SGPR_GEMM_STRASSEN set in the environment the recursion uses the library's values instead.
 * sgpr_probe_strassen_rec_plan: the list of ONE call (m x n x k, lower) under the thresholds the recursion gives it, in the record
 * format above; cfg_out (may be null): smin, kslab, smin2, kslab2 and the inner threshold that holds under an outer product
 * (= min(smin, smin2 / 2): the inner plan of a kind-5 record is sgpr_probe_strassen_plan with THAT smin).
 * sgpr_probe_strassen_rec_scratch: doubles of operand-sum scratch potrf() reserves at order n: out[0] both levels, out[1] one.
 * sgpr_probe_gemm_strassen_rec_dev: one product on device pointers as the recursion would issue it.
 * tools/strassen_rec_plan.py replays the list. */
int sgpr_probe_strassen_rec_plan(int m, int n, int k, int lower, long scratch_doubles, long cfg_out[5], long long *out,
                                 int max_records, int *count);
int sgpr_probe_strassen_rec_scratch(int n, unsigned long long out[2]);
int sgpr_probe_gemm_strassen_rec_dev(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb,
                                     double beta, double *C, size_t ldc, int lower, void *stream);
/* The operand sums beside the products.  Tunables, read at every call: gemm_strassen_overlap (1, the built-in value: a call's sums run on
 * low-priority side streams under the products before the ones that need them; 0: everything on the caller's stream in list
 * order), gemm_strassen_overlap_slack (doubles of the scratch beyond the call's need that second buffers may take; < 0: all, 0: none),
 * gemm_strassen_overlap_streams (1, or 2 = the B side's sums on a side stream of their own), gemm_strassen_sum_wgs (most workgroups
 * of a side-stream sum, 256 = one per CU).
 * sgpr_probe_strassen_schedule: the schedule of ONE call (planned like sgpr_probe_strassen_rec_plan, with the scratch it needs) for
 * a scratch buffer of capacity_doubles (< 0: exactly the need; below the need: an error).  32 words per record: [0 .. 15] the list's
 * record, the inner plan of every kind-5 record expanded behind it; [16] level (0: the list's record, 1: a record of the inner plan
 * of the kind-5 record before it); [17] stream (0: the caller's, 1 / 2: a side stream; sums only); [18] a sum: the buffer (0 / 1) of
 * its region it writes; kinds 2 / 5: the buffer of the A-side scratch (inner / outer region) it reads, -1 a raw block; [19] kinds
 * 2 / 5: likewise for the B side; [20] number of waits; [21 ...] the records (indices into the schedule, all earlier) it waits for.
 * Under a kind-5 record the inner records' operands "A" / "B" are its operands: the raw block or the outer buffer [18] / [19].
 * info: [0 .. 3] doubles per region (inner A, inner B, outer A, outer B: the pinned layout; second buffers lie behind it in the
 * same order), [4 .. 7] buffers per region, [8] side streams, [9] the capacity.  tools/strassen_schedule.py replays it. */
int sgpr_probe_strassen_schedule(int m, int n, int k, int lower, long capacity_doubles, long long info[12], long long *out,
                                 int max_records, int *count);
/* The arena layout of a batched fit as the drivers compute it (csrc/batch.hip: batch_layout), without a device call.  path: 0 the
 * one-launch path (order <= 256), 1 the mid path (256 < order <= 2048); mode: 0 fit, 1 nll gradient, 2 loo, 3 loo gradient (path 0
 * only); d: 0 for sgpr_fit_batch's x | y, 1 .. 3 for sgpr_fit_batch_nd[_grad] (mode 0 or 1, reg 0).  The tunable batch_gradmid_chunk applies.
 * out: [0] problems per chunk, [1] doubles behind nll per problem; byte offsets [2 .. 6] x, y, z, consts, noise of the input block
 * and [7] its size; [8 .. 10] alpha, nll, info of the output block and [11] its size; [12 .. 19] the mid path's scratch regions L / U
 * images, leaf inverses, flags of panel 1, of panel 2, solve vectors, publication buffers, state words, partials (0 on path 0) and
 * [20] the scratch size; [21] sizeof KConst, [22] sizeof NdConst, [23] the flag bytes of one panel for a chunk (0 on path 0).
 * tests/test_batch_layout_cpu.py checks it against the formulas. */
int sgpr_probe_batch_layout(int path, int mode, int d, int reg, int nbatch, int n_pts, int nhyp, unsigned long long out[24]);
/* The same for sgpr_fit_batch_nd_loo (mode 2, both paths) and sgpr_fit_batch_nd_loo_grad (mode 3, path 0 only), d = 1 .. 3: the modes
 * sgpr_probe_batch_layout refuses for d > 0.  out as above.  tests/test_batch_pairs_loo_cpu.py checks it against the formulas. */
int sgpr_probe_batch_layout_nd_loo(int path, int mode, int d, int nbatch, int n_pts, int nhyp, unsigned long long out[24]);
/* The mid path's layout for the loo gradient (sgpr_fit_batch_loo_grad_mid: d = 0, reg 0 or 1; sgpr_fit_batch_nd_loo_grad_mid: d = 1 .. 3,
 * reg 0), which the two probes above refuse; 256 < order <= 2048.  out[0 .. 23] as above ([12] the L / U / M images); [24 .. 27] the
 * regions behind the contraction's partials: the point pass's partials, W~, v, beta, and [28] the contraction's vector of zeros; [29] the padded order, [30] images per problem;
 * [31] zero.  tests/test_batch_loo_grad_mid_cpu.py checks it against the formulas. */
int sgpr_probe_batch_layout_loograd_mid(int d, int reg, int nbatch, int n_pts, int nhyp, unsigned long long out[32]);
unsigned sgpr_probe_map_calls(void);
int sgpr_probe_map_team(int ntest, int n0);

/* the block solve's stream tickets as the host computes them (csrc/trsm.hip: piece_of): ticket of a solve with `strips` strips ->
 * {strip, piece, pieces of the strip, slot of the strip's first partial sum, 0 or the tile f whose fold the ticket is} for pieces
 * of at most `cap` tiles (strip = strips: past the end); and for `strips` strips {tickets, partial sums} */
int sgpr_probe_trsm_piece(int ticket, int cap, int strips, int out[5]);
int sgpr_probe_trsm_counts(int strips, int cap, unsigned long long out[2]);

/* co-residency census of two concurrent kernels (A: na workgroups of threads_a threads with lds_a bytes of LDS spinning
 * spin_a us on one stream, B likewise on a second, high-priority stream; optional CU masks): per workgroup XCC id,
 * HW_ID, start and end in 100 MHz ticks.  Answers "how many CUs must a persistent grid leave free, and where". */
int sgpr_probe_census(int na, int threads_a, int lds_a, int spin_a, const unsigned *mask_a, int nwords_a,
                      int nb, int threads_b, int lds_b, int spin_b, const unsigned *mask_b, int nwords_b,
                      unsigned long long *host_out);

/* A third Strassen level on top of the front end, for the recursion's largest products (csrc/strassen_plan.hip: strassen_top_plan).
 * Tunables, read at every factorisation: rec_strassen3_min (smallest half-size of m and n that takes it; 0: off),
 * rec_strassen3_kslab / rec_strassen3_kslab_short (top k slab of a call whose k reaches the long one / of a shorter call; 0: none),
 * rec_strassen3_overlap (1: the top passes run on a low-priority stream of their own under the next product; 0: on the caller's
 * stream in list order), rec_strassen3_buffers (2: a second buffer set for that), rec_strassen3_noscratch (tests: the buffer's
 * allocation is reported as failed -> the level is off).  With SGPR_GEMM_STRASSEN set in the environment the level is never taken.
 * sgpr_probe_strassen_top_plan: the list of ONE call (m x n x k, lower), 16 words per record, [0] = kind:
 *   6 top sum:    layout of kind 1; the result goes to the TOP scratch of that side
 *   7 zero:       [1] rows [2] cols                       the temporary T = 0
 *   8 top product [1] a_src (0: block of A at ([2], [3]), 1: the top A scratch) [4] b_src, ([5], [6]) likewise [7] m [8] n [9] k
 *                 [10 .. 14] thresholds (smin, kslab, smin2, kslab2, smin_under) of the half-size call T += X Y^T, whose list is
 *                 sgpr_probe_strassen_cfg_plan(m, n, k, 0, those)
 *   9 accumulate  [1] rows [2] cols [3] [4] first destination (row, column of C) [5] its sign [6] [7] [8] the second (sign 0: none):
 *                 C1 += alpha sign1 T, C2 += alpha sign2 T
 *  10 pass-through: layout of kind 3 ([1] lower [2] ar [3] ac [4] br [5] bc [6] m [7] n [8] k [9] cr [10] cc), [11 .. 15] thresholds:
 *                 that block through the front end as before (sgpr_probe_strassen_cfg_plan(m, n, k, lower, those)).  A call that
 *                 does not qualify is this record alone.
 * sgpr_probe_strassen_cfg_plan: the list (kinds 1 - 5) of one call under explicit thresholds.
 * sgpr_probe_strassen_top_scratch: doubles of top-level scratch potrf() reserves at order n: out[0] one buffer set (T, A side,
 * B side), out[1] with the second set.  sgpr_probe_gemm_strassen_top_dev: one product on device pointers as the recursion issues it.
 * tools/strassen_top_plan.py replays the list. */
int sgpr_probe_strassen_top_plan(int m, int n, int k, int lower, long scratch_doubles, long long *out, int max_records, int *count);
int sgpr_probe_strassen_cfg_plan(int m, int n, int k, int lower, const long cfg[5], long long *out, int max_records, int *count);
int sgpr_probe_strassen_top_scratch(int n, unsigned long long out[2]);
int sgpr_probe_gemm_strassen_top_dev(int m, int n, int k, double alpha, const double *A, size_t lda, const double *B, size_t ldb,
                                     double beta, double *C, size_t ldc, int lower, void *stream);

#ifdef __cplusplus
}
#endif
#endif
