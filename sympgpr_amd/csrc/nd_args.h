// nd_args.h -- what the single-problem d-pair units share beside the entry formulas (nd_eval.h): the argument block of one call
// and one small helper.  Included by gram_nd.hip (Gram build, prediction), map_nd.hip (the symplectic map) and genfun_nd.hip
// (the generating function); the batched kernels (batch.hip) read one NdConst per problem instead and do not use it.
#pragma once
#include "nd_eval.h"

namespace sgpr {
namespace nd {

constexpr int NT = 256;     // threads per workgroup of the Gram, prediction and generating-function kernels

// the geometry of one call and, last, the constants of the fit (nd_eval.h)
struct NdArgs {
    int mi, mj;
    const double *Xb, *Xa;   // row points (mi x D), column points (mj x D), column-major
    size_t ldxb, ldxa;
    double *K;
    size_t ld, rstride, cstride;   // element distance between consecutive row / column blocks
    int sel;                       // 1: block (a, b) goes to K + roff[a] + coff[b] * ld instead, skipped when either is < 0
    long roff[6], coff[6];
    long diag_off;
    double noise;
    NdConst c;
};

// the hyper-parameters of the call into the constants of its argument block (nd_eval.h)
inline int fill_args(int family, int d, const double *hyp, int nhyp, NdArgs &a) { return fill_consts(family, d, hyp, nhyp, a.c); }

}  // namespace nd
}  // namespace sgpr
