// batch.hip -- many small independent fits in ONE launch.
//
// The reference's only batch axis: `nphmap` independent GP pairs, one per toroidal section, and the
// CMA-ES populations that evaluate nll_chol for a set of hyper-parameter vectors over the same data
// (python/05_tokamak/Split_SympGPR/main.py:36-41,63-66,96-112), at matrix orders n = 40 ... 160.  At
// those sizes one nll_chol through a device-resident handle is pure set-up (create / upload / five
// launches / download: 0.2 - 1 ms, tools/nll_call_cost.py); here one workgroup runs the whole body of
// nll_chol (python/functions/func.py:189-196) for one problem -- Gram build, Cholesky, both triangular
// solves, the negative log-likelihood -- and a launch covers the batch.
//
// Per problem (order n <= 256 = two leaves): Ky -> scratch (global, L2-resident, 512 KiB per
// workgroup);  L11 = leaf(A11) in LDS (leaf.h), X11 = inv(L11);  L21 = A21 X11^T;  A22 -= L21 L21^T;
// L22 = leaf(A22);  y = L^-1 z and alpha = L^-T y through the leaf inverses.  Latency-bound by
// construction: throughput comes from the number of problems in flight, not from the matrix cores.
// Problems with d canonical pairs per point (sgpr_fit_batch_nd) take the same path behind a Gram stage of their own: the entry
// formulas of nd_eval.h, fit_batch_nd_kernel / mid_build_nd_kernel.  Their nll gradient (sgpr_fit_batch_nd_grad) is that path with the
// Ky^-1 stage of the d = 1 gradient and a contraction over D x D blocks of point pairs: contract_rows_nd / mid_grad_nd_kernel.
// Their leave-one-point-out sums (sgpr_fit_batch_nd_loo) take one thread per point behind the same Ky^-1 stage, with D x D blocks
// (loo_point_nd; mid_loo_kernel<D> above order 256), and the gradient of one of them (sgpr_fit_batch_nd_loo_grad, orders up to 256)
// the phases (L1) - (L4) of the d = 1 loo gradient over those blocks (grad_problem_nd); above order 256 both layouts take the mid
// path's loo gradient stage (sgpr_fit_batch_loo_grad_mid, sgpr_fit_batch_nd_loo_grad_mid: mid_loograd).
// The device code is in batch_small.h (n <= 256) and batch_mid.h (256 < n <= 2048), included here and only here: one translation
// unit.  This file holds the arena, its one layout function, the staging of a call, the two host drivers and, last, the one
// exported runner fit_batch_run, which takes a BatchCall (common.h) filled by the C entry (capi.hip) and chooses the driver.
#include <cmath>
#include <cstring>

#include "common.h"
#include "gemm_tile.h"
#include "leaf.h"
#include "loo_block.h"
#include "nllgrad_pair.h"
#include "nd_eval.h"
#include "pair_eval.h"
#include "batch_small.h"
#include "batch_mid.h"

namespace sgpr {

namespace {

// Device + pinned-host staging of one calling thread, grown on demand and kept: a call is then one H2D copy,
// one launch and one D2H copy (nine hipMalloc / hipFree pairs and eight small pageable copies per call were
// most of a single small fit's 230 us through a handle).
struct Arena {
    char *dev = nullptr, *host = nullptr;
    size_t cap_dev = 0, cap_host = 0;
    int device = -1;
    // no destructor: at thread / process exit the HIP runtime may already be gone; the OS reclaims
    void release()
    {
        if (dev) (void)hipFree(dev);
        if (host) (void)hipHostFree(host);
        dev = host = nullptr;
        cap_dev = cap_host = 0;
    }
    int reserve(size_t need_dev, size_t need_host)
    {
        int cur = 0;
        SGPR_HIP(hipGetDevice(&cur));
        if (cur != device) { release(); device = cur; }
        // grown for a large batch once, asked for a small one now: give the difference back (a CMA-ES population at order 2048
        // must not keep gigabytes pinned under the full-size fit that follows it)
        if (cap_dev > (256ull << 20) && need_dev * 4 < cap_dev) { if (dev) (void)hipFree(dev); dev = nullptr; cap_dev = 0; }
        if (need_dev > cap_dev) {
            if (dev) (void)hipFree(dev);
            dev = nullptr; cap_dev = 0;
            SGPR_HIP(hipMalloc((void **)&dev, need_dev));
            cap_dev = need_dev;
        }
        if (need_host > cap_host) {
            if (host) (void)hipHostFree(host);
            host = nullptr; cap_host = 0;
            SGPR_HIP(hipHostMalloc((void **)&host, need_host, hipHostMallocDefault));
            cap_host = need_host;
        }
        return 0;
    }
};
thread_local Arena t_arena;

// the arena of the calling thread, cut by a layout: pinned input | output blocks, device input | output | scratch
struct Blocks {
    char *hin, *hout, *din, *dout, *dscr;
};

template <class T>
T *at(char *base, size_t off) { return reinterpret_cast<T *>(base + off); }

int reserve_blocks(const BatchLayout &l, Blocks &m)
{
    Arena &ar = t_arena;
    const int rc = ar.reserve(l.in_bytes + l.out_bytes + l.scr_bytes, l.in_bytes + l.out_bytes);
    if (rc) return rc;
    m = Blocks{ar.host, ar.host + l.in_bytes, ar.dev, ar.dev + l.in_bytes, ar.dev + l.in_bytes + l.out_bytes};
    return 0;
}

// problems b0 .. b0 + nb into the pinned input block -- points, z, one KConst (d = 0) or NdConst per problem, |sig2n| -- and the
// block to the device in one copy
int stage_in(const BatchCall &c, const BatchLayout &l, const Blocks &m, int b0, int nb, hipStream_t st)
{
    const size_t B = (size_t)nb, N = (size_t)c.npts, D = 2 * (size_t)c.d;
    if (c.d) memcpy(m.hin + l.o_x, c.x + (size_t)b0 * D * N, B * D * N * 8);
    else {
        memcpy(m.hin + l.o_x, c.x + (size_t)b0 * N, B * N * 8);
        memcpy(m.hin + l.o_y, c.y + (size_t)b0 * N, B * N * 8);
    }
    memcpy(m.hin + l.o_z, c.z + (size_t)b0 * c.n, B * c.n * 8);
    KConst *kcs = at<KConst>(m.hin, l.o_kc);
    nd::NdConst *ncs = at<nd::NdConst>(m.hin, l.o_kc);
    double *noise = at<double>(m.hin, l.o_no);
    for (int b = 0; b < nb; ++b) {
        const double *hyp = c.hyp + (size_t)(b0 + b) * c.nhyp;
        const int rc = c.d ? nd::fill_consts(c.family, c.d, hyp, c.nhyp, ncs[b]) : make_kconst(c.family, hyp, c.nhyp, &kcs[b]);
        if (rc) return rc;
        noise[b] = std::fabs(c.sig2n[b0 + b]);
    }
    SGPR_HIP(hipMemcpyAsync(m.din, m.hin, l.in_bytes, hipMemcpyHostToDevice, st));
    return 0;
}

// the output block back in one copy (without alpha only its tail), the wait, and alpha, nll, info into the caller's rows b0 ..
int fetch_out(const BatchCall &c, const BatchLayout &l, const Blocks &m, int b0, int nb, hipStream_t st)
{
    const size_t B = (size_t)nb, from = c.alpha ? 0 : l.o_nll;
    SGPR_HIP(hipMemcpyAsync(m.hout + from, m.dout + from, l.out_bytes - from, hipMemcpyDeviceToHost, st));
    SGPR_HIP(hipStreamSynchronize(st));
    if (c.alpha) memcpy(c.alpha + (size_t)b0 * c.n, m.hout + l.o_al, B * c.n * 8);
    memcpy(c.nll + b0, m.hout + l.o_nll, B * 8);
    memcpy(c.info + b0, m.hout + l.o_info, B * sizeof(int));
    return 0;
}

// The sums behind nll (problem b's at nll + chunk + b nacc) into the caller's rows b0 ..: the raw gradient sums scaled (sig from the
// problem's staged KConst, or NdConst for d > 0), {loo, press} and the loo gradient's value copied out, NaN rows where the
// factorisation failed.
void finish_rows(const BatchCall &c, const BatchLayout &l, const Blocks &m, int b0, int nb)
{
    const double *raw = at<const double>(m.hout, l.o_nll) + l.chunk;
    const KConst *kcs = at<const KConst>(m.hin, l.o_kc);
    const nd::NdConst *ncs = at<const nd::NdConst>(m.hin, l.o_kc);
    const size_t B = (size_t)nb, nacc = l.nacc, ngrad = (size_t)c.nhyp + 1;
    if (c.grad) {
        for (size_t b = 0; b < B; ++b) {
            const size_t row = (size_t)b0 + b;
            const double *r = raw + b * nacc + (c.value ? 2 : 0);
            double *g = c.grad + row * ngrad;
            if (c.info[row] != 0) {
                c.nll[row] = std::nan("");
                if (c.value) c.value[row] = std::nan("");
                for (size_t k = 0; k < ngrad; ++k) g[k] = std::nan("");
                continue;
            }
            scale_grad_sums(r, c.nhyp, c.d ? ncs[b].sig : kcs[b].sig, c.sig2n[row], g);
            if (c.value) c.value[row] = raw[b * nacc + (c.which == SGPR_LOO_PRESS ? 1 : 0)];
        }
    }
    if (c.loo) {
        for (size_t b = 0; b < B; ++b) {
            const size_t row = (size_t)b0 + b;
            const bool bad = c.info[row] != 0;
            if (bad) c.nll[row] = std::nan("");
            for (int k = 0; k < 2; ++k) c.loo[row * 2 + k] = bad ? std::nan("") : raw[b * 2 + k];
        }
    }
}

}  // namespace

int fit_batch_max_order() { return potrf_batch_max_order(); }
int fit_batch_trim() { t_arena.release(); return 0; }     // the calling thread's device arena and pinned staging block
int fit_batch_grad_max_order() { return BMAX; }

// Every offset of the arena is computed here and nowhere else (common.h: BatchLayout; tests/test_batch_layout_cpu.py checks it
// through sgpr_probe_batch_layout).  Each region is rounded up to 256 bytes.
BatchLayout batch_layout(int mid, int mode, int d, int reg, int nbatch, int npts, int nhyp)
{
    auto up256 = [](size_t b) { return (b + 255) / 256 * 256; };
    BatchLayout l{};
    const int n = d ? 2 * d * npts : reg ? npts : 2 * npts;
    const bool kinv = mode != MODE_FIT;      // the mid path forms Ky^-1 behind the solves
    const size_t xb = d ? 2 * (size_t)d * npts * 8 : (size_t)npts * 8, yb = d ? 0 : (size_t)npts * 8;
    l.const_bytes = d ? sizeof(nd::NdConst) : sizeof(KConst);
    l.chunk = nbatch;
    l.nacc = mode == MODE_GRAD ? (size_t)nhyp + 1 : mode == MODE_LOO ? 2 : mode == MODE_LOOGRAD ? (size_t)nhyp + 3 : 0;
    size_t img = 0, nimg = 0;
    if (mid) {
        l.npad = (n + (int)LEAF - 1) / (int)LEAF * (int)LEAF;
        l.W = l.npad / (int)LEAF;
        l.ggx = (n + GT - 1) / GT;
        l.ggy = (npts + GCJ - 1) / GCJ;
        l.lnwg = (npts + GT - 1) / GT;
        img = (size_t)l.npad * l.npad * 8;
        nimg = mode == MODE_LOOGRAD ? 3 : kinv ? 2 : 1;
        // at most ~2 GiB of images per chunk (64 problems of order 2048, 32 with the gradient's second image: 2 x 32 MiB each, 21 with
        // the loo gradient's third; round 3: 6 GiB), at least one chip-full of strips (256 workgroups)
        l.chunk = (int)std::min<size_t>((size_t)nbatch, std::max<size_t>((256 + l.W - 1) / l.W, (2ull << 30) / (nimg * img)));
        if (l.chunk > 16384) l.chunk = 16384;      // grid.z of the build launch
        if (kinv) {                                // tunable "batch_gradmid_chunk" > 0 caps it (tests: several chunks of few problems)
            const int cap = (int)tune("batch_gradmid_chunk", 0);
            if (cap > 0 && l.chunk > cap) l.chunk = cap;
        }
        l.flag_bytes = potrf_batch_flag_bytes(l.chunk);
    }
    const size_t C = (size_t)l.chunk;
    // input block (one H2D): x | y | z | consts | noise ; output block (one D2H): alpha | nll [| sums: nacc per problem] | info
    l.o_x = 0;
    l.o_y = l.o_x + up256(C * xb);
    l.o_z = l.o_y + up256(C * yb);
    l.o_kc = l.o_z + up256(C * n * 8);
    l.o_no = l.o_kc + up256(C * l.const_bytes);
    l.in_bytes = l.o_no + up256(C * 8);
    l.o_al = 0;
    l.o_nll = l.o_al + up256(C * n * 8);
    l.o_info = l.o_nll + up256(C * (1 + l.nacc) * 8);
    l.out_bytes = l.o_info + up256(C * sizeof(int));
    if (!mid) {
        // per workgroup (at most 1024 of them): PER_WG doubles [+ BMAX^2 (U) for the gradient and loo] [+ BMAX^2 (M) for the loo gradient]
        const size_t per_wg = PER_WG + (mode != MODE_FIT ? (size_t)BMAX * BMAX : 0) + (mode == MODE_LOOGRAD ? (size_t)BMAX * BMAX : 0);
        l.scr_bytes = (size_t)std::min(nbatch, 1024) * per_wg * 8;
        return l;
    }
    // the images (with a Ky^-1 phase the U images directly behind the L images), the leaf inverses, the flags of the two panels, the
    // solves' right-hand sides / solutions padded to npad, their two publication buffers and 8 state words per problem; last the
    // partials of the contraction or of the loo sums
    l.o_A = 0;
    l.o_inv = l.o_A + nimg * up256(C * img);
    l.o_fl = l.o_inv + up256(C * l.W * LEAF * LEAF * 8);
    l.o_fl2 = l.o_fl + up256(l.flag_bytes);
    l.o_r = l.o_fl2 + up256(l.flag_bytes);
    l.o_pub = l.o_r + up256(C * l.npad * 8);
    l.o_st = l.o_pub + up256(2 * C * l.npad * 8);
    l.o_part = l.o_st + up256(C * 8 * sizeof(int));
    // (GPART doubles per partial; GPART_ND for d > 0, whose sums number up to 11)
    const size_t gpart_bytes = up256(C * l.ggx * l.ggy * (d ? GPART_ND : GPART) * 8), lpart_bytes = up256(C * l.lnwg * 2 * 8);
    l.scr_bytes = l.o_part + (mode == MODE_GRAD ? gpart_bytes : mode == MODE_LOO ? lpart_bytes : 0);
    if (mode == MODE_LOOGRAD) {
        // the loo gradient: both sets of partials, then per problem W~ (T = D (D + 1) / 2 doubles per point, D the rows per point),
        // v, beta and a vector of zeros (npad doubles each)
        const size_t D = d ? 2 * (size_t)d : reg ? 1 : 2;
        l.o_lpart = l.o_part + gpart_bytes;
        l.o_wt = l.o_lpart + lpart_bytes;
        l.o_v = l.o_wt + up256(C * (D * (D + 1) / 2) * npts * 8);
        l.o_beta = l.o_v + up256(C * l.npad * 8);
        l.o_zero = l.o_beta + up256(C * l.npad * 8);
        l.scr_bytes = l.o_zero + up256(C * l.npad * 8);
    }
    return l;
}

namespace {

// ---- problems of order n <= BMAX: one launch, one workgroup per problem (fit_batch_kernel in the mode of the call, or
// fit_batch_nd_kernel for d canonical pairs per point); the whole batch is one chunk
int fit_batch_small(const BatchCall &c)
{
    const int mode = c.mode();
    const BatchLayout l = batch_layout(0, mode, c.d, c.reg, c.nbatch, c.npts, c.nhyp);
    Blocks m;
    int rc = reserve_blocks(l, m);
    if (rc) return rc;
    hipStream_t st = nullptr;
    if ((rc = stage_in(c, l, m, 0, c.nbatch, st))) return rc;
    SGPR_HIP(hipMemsetAsync(m.dout + l.o_info, 0, (size_t)c.nbatch * sizeof(int), st));
    const dim3 g(std::min(c.nbatch, 1024)), t(LT);
    if (c.d) {
        const BatchNdArgs a{c.nbatch, c.npts, c.n, at<double>(m.din, l.o_x), at<double>(m.din, l.o_z), at<nd::NdConst>(m.din, l.o_kc),
                            at<double>(m.din, l.o_no), at<double>(m.dscr, 0), c.alpha ? at<double>(m.dout, l.o_al) : nullptr,
                            at<double>(m.dout, l.o_nll), at<int>(m.dout, l.o_info), c.which};
        if ((rc = nd::dispatch_nd(c.family, c.d, [&](auto fam, auto dd) {
                auto launch = [&](auto md) {
                    hipLaunchKernelGGL((fit_batch_nd_kernel<decltype(fam)::value, decltype(dd)::value, decltype(md)::value>), g, t, 0, st, a);
                    return 0;
                };
                switch (mode) {
                case MODE_LOOGRAD: return launch(std::integral_constant<int, MODE_LOOGRAD>());
                case MODE_GRAD:    return launch(std::integral_constant<int, MODE_GRAD>());
                case MODE_LOO:     return launch(std::integral_constant<int, MODE_LOO>());
                default:           return launch(std::integral_constant<int, MODE_FIT>());
                }
            })))
            return rc;
    } else {
        // alpha is never null here, even when the caller's is (the kernel writes it; it is only not copied back)
        const BatchArgs a{c.nbatch, c.npts, c.n, c.reg, at<double>(m.din, l.o_x), at<double>(m.din, l.o_y), at<double>(m.din, l.o_z),
                          at<KConst>(m.din, l.o_kc), at<double>(m.din, l.o_no), at<double>(m.dscr, 0), at<double>(m.dout, l.o_al),
                          at<double>(m.dout, l.o_nll), at<int>(m.dout, l.o_info), c.which};
        auto launch = [&](auto fam, auto md) {
            hipLaunchKernelGGL((fit_batch_kernel<decltype(fam)::value, decltype(md)::value>), g, t, 0, st, a);
            return 0;
        };
        (void)dispatch_family(c.family, [&](auto fam) {         // the family has been checked
            switch (mode) {
            case MODE_LOOGRAD: return launch(fam, std::integral_constant<int, MODE_LOOGRAD>());
            case MODE_GRAD:    return launch(fam, std::integral_constant<int, MODE_GRAD>());
            case MODE_LOO:     return launch(fam, std::integral_constant<int, MODE_LOO>());
            default:           return launch(fam, std::integral_constant<int, MODE_FIT>());
            }
        });
    }
    SGPR_CHECK_LAUNCH();
    if ((rc = fetch_out(c, l, m, 0, c.nbatch, st))) return rc;
    finish_rows(c, l, m, 0, c.nbatch);
    return 0;
}

// ---- problems of order 256 < n <= 2048 (batch_mid.h): chunks of problems share the scratch images; every chunk runs the stages
// below on the stream, in this order.  With grad or loo (the Ky^-1 phase) a second image per problem (U = L^-T) stands behind the L
// images, and the sums come back behind nll in the chunk's one device-to-host copy.  d > 0: X in place of x | y, one NdConst per
// problem, mid_build_nd_kernel in place of mid_build_kernel and mid_grad_nd_kernel in place of mid_grad_kernel; the loo phase is
// mid_loo_kernel at 2 d rows per point.  The loo gradient (value and grad) takes a third image per problem behind the U images and
// the stage mid_loograd in place of the two before it.

// the device pointers of one chunk of nb problems
struct MidChunk {
    int nb;
    MidArgs a;                            // the solves' kernels (and the d = 0 build)
    double *A, *U, *M, *inv;              // L images, U images, the loo gradient's M images, leaf inverses
    int *fl, *fl2;                        // the flags of the first and the second panel
    double *r, *pub;                      // right-hand sides / solutions, publication buffers
    int *state;
    double *part, *sums;                  // the partials; the sums behind nll
    double *lpart, *wt, *v, *beta, *zero; // the loo gradient: the point pass's partials, W~, v, beta, zeros
    int *info;
    size_t stride, stride_inv;            // doubles per image, per problem's leaf inverses
};

MidChunk mid_chunk(const BatchCall &c, const BatchLayout &l, const Blocks &m, int nb)
{
    MidChunk k{};
    const size_t C = (size_t)l.chunk;
    k.nb = nb;
    k.stride = (size_t)l.npad * l.npad;
    k.stride_inv = (size_t)l.W * LEAF * LEAF;
    k.A = at<double>(m.dscr, l.o_A);
    k.U = k.A + C * k.stride;
    k.M = k.U + C * k.stride;
    k.inv = at<double>(m.dscr, l.o_inv);
    k.fl = at<int>(m.dscr, l.o_fl);
    k.fl2 = at<int>(m.dscr, l.o_fl2);
    k.r = at<double>(m.dscr, l.o_r);
    k.pub = at<double>(m.dscr, l.o_pub);
    k.state = at<int>(m.dscr, l.o_st);
    k.part = at<double>(m.dscr, l.o_part);
    k.lpart = at<double>(m.dscr, l.o_lpart);
    k.wt = at<double>(m.dscr, l.o_wt);
    k.v = at<double>(m.dscr, l.o_v);
    k.beta = at<double>(m.dscr, l.o_beta);
    k.zero = at<double>(m.dscr, l.o_zero);
    k.sums = at<double>(m.dout, l.o_nll) + C;
    k.info = at<int>(m.dout, l.o_info);
    k.a = MidArgs{nb, c.npts, c.n, l.npad, c.reg, at<double>(m.din, l.o_x), at<double>(m.din, l.o_y), at<double>(m.din, l.o_z),
                  at<KConst>(m.din, l.o_kc), at<double>(m.din, l.o_no), k.A, k.inv, c.alpha ? at<double>(m.dout, l.o_al) : nullptr,
                  at<double>(m.dout, l.o_nll), k.info};
    return k;
}

// every Ky_b, lower triangle, into its npad x npad image
int mid_build(hipStream_t st, const BatchCall &c, const BatchLayout &l, const MidChunk &k)
{
    const size_t B = (size_t)k.nb, img = k.stride * 8;
    if (c.grad || c.loo) {
        // both images (all three of the loo gradient), unconditionally: the zeros the gradient phase reads above L's diagonal, below
        // U's and in the images of a problem whose factorisation stops early come from here (and the leaf inverses of such a
        // problem are defined)
        SGPR_HIP(hipMemsetAsync(k.A, 0, ((c.value ? 2 : 1) * (size_t)l.chunk + B) * img, st));
        SGPR_HIP(hipMemsetAsync(k.inv, 0, B * k.stride_inv * 8, st));
    } else if (l.npad != c.n) SGPR_HIP(hipMemsetAsync(k.A, 0, B * img, st));
    const dim3 grid((c.npts + MT - 1) / MT, (c.npts + MJ - 1) / MJ, k.nb);
    if (c.d) {
        const MidNdArgs an{c.npts, c.n, l.npad, k.a.x, reinterpret_cast<const nd::NdConst *>(k.a.kc), k.a.noise, k.A};
        const int rc = nd::dispatch_nd(c.family, c.d, [&](auto fam, auto dd) {
            hipLaunchKernelGGL((mid_build_nd_kernel<decltype(fam)::value, decltype(dd)::value>), grid, dim3(MT), 0, st, an);
            return 0;
        });
        if (rc) return rc;
    } else
        (void)dispatch_family(c.family, [&](auto fam) {         // the family has been checked
            hipLaunchKernelGGL(mid_build_kernel<decltype(fam)::value>, grid, dim3(MT), 0, st, k.a);
            return 0;
        });
    SGPR_CHECK_LAUNCH();
    return 0;
}

// panel.hip's panel_batch_kernel (through potrf_batch_panel, chol.hip): W = npad / 128 workgroups per problem run the leaf chain on their own matrix
int mid_factor(hipStream_t st, const BatchLayout &l, const MidChunk &k)
{
    const int npad = l.npad, W = l.W;
    const size_t ld = (size_t)npad;
    static const int two_min = (int)tune("batch_two_min", 512);
    if (npad <= two_min) return potrf_batch(k.nb, npad, k.A, k.stride, ld, k.inv, k.stride_inv, k.fl, k.info, st);
    // two panels above order 512 (SGPR_BATCH_TWO_MIN): in ONE panel the last strip alone has ~W^2 / 2 products of 128^3 to
    // do in a row (n = 2048: 3.0 ms for the launch); as W/2 + W/2 leaf columns (at most 8 first) with the update of the
    // second half on the matrix cores between them it is ~2 ms (per fit at 16 per batch: n = 2048 947 -> 326 us,
    // n = 1024 85 -> 75 us)
    const int W1 = std::min(8, (W + 1) / 2), k1 = W1 * (int)LEAF, m2 = npad - k1;
    SGPR_HIP(hipMemsetAsync(k.info, 0, (size_t)k.nb * sizeof(int), st));
    int rc = potrf_batch_panel(k.nb, npad, 0, W1, k.A, k.stride, ld, k.inv, k.stride_inv, k.fl, k.info, st);
    if (rc) return rc;
    const int t2 = m2 / (int)LEAF;
    hipLaunchKernelGGL(mid_syrk_kernel, dim3((unsigned)(t2 * (t2 + 1) / 2), (unsigned)k.nb), dim3(256), 0, st,
                       MidSyrk{k.A, k.stride, ld, k1, m2});
    SGPR_CHECK_LAUNCH();
    return potrf_batch_panel(k.nb, npad, k1, W - W1, k.A, k.stride, ld, k.inv, k.stride_inv, k.fl2, k.info, st);
}

// y = L^-1 z, alpha = L^-T y for every problem: the strip solve of trsv.hip, W x nb workgroups per launch; then nll and alpha
int mid_solve(hipStream_t st, const BatchLayout &l, const MidChunk &k)
{
    const int npad = l.npad, nb = k.nb;
    const size_t B = (size_t)nb, ld = (size_t)npad;
    SGPR_HIP(hipMemsetAsync(k.state, 0, B * 8 * sizeof(int), st));
    SGPR_HIP(hipMemsetAsync(k.pub, 0xFF, 2 * B * npad * 8, st));
    hipLaunchKernelGGL(mid_rhs_kernel, dim3((unsigned)((npad + 255) / 256), (unsigned)nb), dim3(256), 0, st, k.a, k.r);
    SGPR_CHECK_LAUNCH();
    int rc = trsv_strips_batch(nb, npad, k.A, k.stride, ld, k.inv, k.stride_inv, k.r, ld, 0, k.state, 8, k.pub, st);
    if (rc) return rc;
    if ((rc = trsv_strips_batch(nb, npad, k.A, k.stride, ld, k.inv, k.stride_inv, k.r, ld, 1, k.state + 4, 8, k.pub + B * npad, st)))
        return rc;
    hipLaunchKernelGGL(mid_finish_kernel, dim3(nb), dim3(ST), 0, st, k.a, (const double *)k.r, (const int *)k.state, k.info);
    SGPR_CHECK_LAUNCH();
    return 0;
}

// Ky^-1 (lower) over every L image: steps (a) and (b) of batch_mid.h
int mid_kinv(hipStream_t st, const BatchLayout &l, const MidChunk &k)
{
    const int W = l.W;
    // (a) U = L^-T: the diagonal tiles, then two launches per doubling of the block size
    MidInv mi{k.A, k.U, k.inv, k.stride, (size_t)l.npad, k.stride_inv, W, 1};
    hipLaunchKernelGGL(mid_udiag_kernel, dim3((unsigned)W, (unsigned)k.nb), dim3(256), 0, st, mi);
    SGPR_CHECK_LAUNCH();
    for (int S = 1; S < W; S *= 2) {
        mi.S = S;
        const dim3 gl((unsigned)((W - S + 2 * S - 1) / (2 * S) * S * S), (unsigned)k.nb);
        hipLaunchKernelGGL(mid_inv_level_kernel<0>, gl, dim3(256), 0, st, mi);
        SGPR_CHECK_LAUNCH();
        hipLaunchKernelGGL(mid_inv_level_kernel<1>, gl, dim3(256), 0, st, mi);
        SGPR_CHECK_LAUNCH();
    }
    // (b) Ky^-1 = U U^T over L
    hipLaunchKernelGGL(mid_kinv_kernel, dim3((unsigned)(W * (W + 1) / 2), (unsigned)k.nb), dim3(256), 0, st, mi);
    SGPR_CHECK_LAUNCH();
    return 0;
}

// {loo, press} of every problem from Ky^-1 and alpha, behind nll
int mid_loo(hipStream_t st, const BatchCall &c, const BatchLayout &l, const MidChunk &k)
{
    const MidLoo ml{c.npts, l.lnwg, (size_t)l.npad, k.A, k.r, k.part, k.info, k.sums};
    const dim3 g((unsigned)l.lnwg, 1, (unsigned)k.nb);
    switch (c.d ? 2 * c.d : c.reg ? 1 : 2) {              // the rows per point
    case 1:  hipLaunchKernelGGL(mid_loo_kernel<1>, g, dim3(GT), 0, st, ml); break;
    case 2:  hipLaunchKernelGGL(mid_loo_kernel<2>, g, dim3(GT), 0, st, ml); break;
    case 4:  hipLaunchKernelGGL(mid_loo_kernel<4>, g, dim3(GT), 0, st, ml); break;
    default: hipLaunchKernelGGL(mid_loo_kernel<6>, g, dim3(GT), 0, st, ml); break;
    }
    SGPR_CHECK_LAUNCH();
    hipLaunchKernelGGL(mid_loo_fold_kernel, dim3(k.nb), dim3(64), 0, st, ml);
    SGPR_CHECK_LAUNCH();
    return 0;
}

// (c) the contraction of Ky^-1 - alpha alpha^T with dK and its fold: the raw gradient sums behind nll
int mid_grad(hipStream_t st, const BatchCall &c, const BatchLayout &l, const MidChunk &k)
{
    const MidGrad mg{c.npts, c.n, c.reg, l.ggx * l.ggy, (int)l.nacc, c.d ? GPART_ND : GPART, (size_t)l.npad, k.a.x, k.a.y, k.a.kc, k.A, k.r,
                     k.part, k.info, k.sums};
    const dim3 gg((unsigned)l.ggx, (unsigned)l.ggy, (unsigned)k.nb);
    if (c.d) {
        const MidGradNd mn{c.npts, c.n, mg.nwg, mg.ld, k.a.x, reinterpret_cast<const nd::NdConst *>(k.a.kc), k.A, k.r, k.part};
        const int rc = nd::dispatch_nd(c.family, c.d, [&](auto fam, auto dd) {
            hipLaunchKernelGGL((mid_grad_nd_kernel<decltype(fam)::value, decltype(dd)::value>), gg, dim3(GT), 0, st, mn);
            return 0;
        });
        if (rc) return rc;
    } else
        (void)dispatch_family(c.family, [&](auto fam) {         // the family has been checked
            hipLaunchKernelGGL(mid_grad_kernel<decltype(fam)::value>, gg, dim3(GT), 0, st, mg);
            return 0;
        });
    SGPR_CHECK_LAUNCH();
    hipLaunchKernelGGL(mid_grad_fold_kernel, dim3(k.nb), dim3(64), 0, st, mg);
    SGPR_CHECK_LAUNCH();
    return 0;
}

// The loo gradient behind Ky^-1, steps (p) - (c) of batch_mid.h: {loo, press} and the raw gradient sums of the objective c.which
// behind nll
int mid_loograd(hipStream_t st, const BatchCall &c, const BatchLayout &l, const MidChunk &k)
{
    const int D = c.d ? 2 * c.d : c.reg ? 1 : 2, W = l.W, npad = l.npad;
    const size_t ld = (size_t)npad;
    const unsigned nb = (unsigned)k.nb, rowb = (unsigned)((npad + GT - 1) / GT);
    // (p) the point pass
    const MidLooW lw{c.npts, c.n, l.lnwg, c.which, ld, k.A, k.r, k.lpart, k.wt, k.v};
    const dim3 gp((unsigned)l.lnwg, 1, nb);
    // (z) beta and Z: ZP points per workgroup, the padding columns behind them
    const MidZ mz{c.npts, c.n, ld, k.A, k.wt, k.v, k.beta, k.U};
    const dim3 gz(rowb, (unsigned)((c.npts + ZP - 1) / ZP + 1), nb);
    auto point_pass = [&](auto dd) { hipLaunchKernelGGL(mid_loow_kernel<decltype(dd)::value>, gp, dim3(GT), 0, st, lw); };
    auto z_pass = [&](auto dd) { hipLaunchKernelGGL(mid_z_kernel<decltype(dd)::value>, gz, dim3(GT), 0, st, mz); };
    auto by_rows = [&](auto f) {
        switch (D) {
        case 1:  f(std::integral_constant<int, 1>()); break;
        case 2:  f(std::integral_constant<int, 2>()); break;
        case 4:  f(std::integral_constant<int, 4>()); break;
        default: f(std::integral_constant<int, 6>()); break;
        }
    };
    by_rows(point_pass);
    SGPR_CHECK_LAUNCH();
    // (m) the mirror
    const int T64 = npad / MB;
    hipLaunchKernelGGL(mid_mirror_kernel, dim3((unsigned)(T64 * (T64 + 1) / 2), nb), dim3(256), 0, st,
                       MidInv{k.A, k.U, k.inv, k.stride, ld, k.stride_inv, W, 1});
    SGPR_CHECK_LAUNCH();
    hipLaunchKernelGGL(mid_beta_kernel, dim3(rowb, nb), dim3(GT), 0, st, mz);
    SGPR_CHECK_LAUNCH();
    by_rows(z_pass);
    SGPR_CHECK_LAUNCH();
    // (M) M = Ky^-1 Z^T, lower tiles, into the third image
    hipLaunchKernelGGL(mid_m_kernel, dim3((unsigned)(W * (W + 1) / 2), nb), dim3(256), 0, st, MidM{k.A, k.U, k.M, k.stride, ld, npad});
    SGPR_CHECK_LAUNCH();
    // (w) W' over M's lower triangle
    hipLaunchKernelGGL(mid_wprime_kernel, dim3(rowb, (unsigned)((c.n + WC - 1) / WC), nb), dim3(GT), 0, st, MidWp{c.n, ld, k.r, k.beta, k.M});
    SGPR_CHECK_LAUNCH();
    // (c) the contraction of W' with dK -- the nll gradient's kernels on the M image with zeros for alpha -- and the fold of both sets
    // of partials
    SGPR_HIP(hipMemsetAsync(k.zero, 0, (size_t)k.nb * ld * 8, st));
    const MidGrad mg{c.npts, c.n, c.reg, l.ggx * l.ggy, (int)l.nacc, c.d ? GPART_ND : GPART, ld, k.a.x, k.a.y, k.a.kc, k.M, k.zero,
                     k.part, k.info, k.sums};
    const dim3 gg((unsigned)l.ggx, (unsigned)l.ggy, nb);
    if (c.d) {
        const MidGradNd mn{c.npts, c.n, mg.nwg, ld, k.a.x, reinterpret_cast<const nd::NdConst *>(k.a.kc), k.M, k.zero, k.part};
        const int rc = nd::dispatch_nd(c.family, c.d, [&](auto fam, auto dd) {
            hipLaunchKernelGGL((mid_grad_nd_kernel<decltype(fam)::value, decltype(dd)::value>), gg, dim3(GT), 0, st, mn);
            return 0;
        });
        if (rc) return rc;
    } else
        (void)dispatch_family(c.family, [&](auto fam) {         // the family has been checked
            hipLaunchKernelGGL(mid_grad_kernel<decltype(fam)::value>, gg, dim3(GT), 0, st, mg);
            return 0;
        });
    SGPR_CHECK_LAUNCH();
    hipLaunchKernelGGL(mid_loograd_fold_kernel, dim3(nb), dim3(64), 0, st, mg, (const double *)k.lpart, l.lnwg);
    SGPR_CHECK_LAUNCH();
    return 0;
}

int fit_batch_mid(const BatchCall &c)
{
    const bool kinv = c.grad || c.loo;
    const BatchLayout l = batch_layout(1, c.mode(), c.d, c.reg, c.nbatch, c.npts, c.nhyp);
    Blocks m;
    int rc = reserve_blocks(l, m);
    if (rc) return rc;
    hipStream_t st = nullptr;
    for (int b0 = 0; b0 < c.nbatch; b0 += l.chunk) {
        const int nb = std::min(l.chunk, c.nbatch - b0);
        if ((rc = stage_in(c, l, m, b0, nb, st))) return rc;
        const MidChunk k = mid_chunk(c, l, m, nb);
        if ((rc = mid_build(st, c, l, k))) return rc;
        if ((rc = mid_factor(st, l, k))) return rc;
        if ((rc = mid_solve(st, l, k))) return rc;
        if (kinv && (rc = mid_kinv(st, l, k))) return rc;
        if (c.loo && (rc = mid_loo(st, c, l, k))) return rc;
        if (c.value) { if ((rc = mid_loograd(st, c, l, k))) return rc; }
        else if (c.grad && (rc = mid_grad(st, c, l, k))) return rc;
        if ((rc = fetch_out(c, l, m, b0, nb, st))) return rc;
        for (int b = 0; b < nb; ++b)
            if (c.info[b0 + b] < 0) return info_status(c.info[b0 + b]);     // a hand-off timed out: an error of the call
        finish_rows(c, l, m, b0, nb);
    }
    return 0;
}

}  // namespace

// host buffers in, host buffers out (common.h); see include/sympgpr_hip.h, sgpr_fit_batch and the entries that follow it
int fit_batch_run(const BatchCall &c) { return c.n > BMAX ? fit_batch_mid(c) : fit_batch_small(c); }

}  // namespace sgpr
