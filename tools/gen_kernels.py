"""sympy -> HIP code generator for the scalar kernels (build container only; sympy never ships).

The reference derives every kernel function from ONE symbolic definition and emits Fortran
(python/01_pendulum/implicit/init_func.py:24-52 symbolic part, :55-81 codegen; the variants in
01_pendulum/explicit, 03_henon_heiles, 01_pendulum/implicit_period_unknown).  This is the same step for
the device: define k(x_a, y_a, x_b, y_b; lx, ly[, p]), differentiate, common-subexpression-eliminate,
print C -- one device function per family for the four functions that enter K (k, d2k/dx_a dx_b,
d2k/dy_a dy_b, d2k/dx_a dy_b) and one each for their lx- and ly-derivatives (the dkdl*, d3k..dl*
functions build_dK / build_dKreg need, functions/func.py:52-129), plus their derivatives by the period p (zero for the
families without one; sgpr_fit_nll_grad_full).

    python tools/gen_kernels.py            # rewrites sympgpr_amd/csrc/generated/pair_generated.h

The hand-optimised forms in pair_eval.h (one exp + one sincos per pair) are checked against the generated
ones on the device (tests/test_gpu_generated.py); family B's length-scale derivatives, which the
hand-written file never had, are served by the generated code directly.

The fifth slot, SGPR_FAM_USER, has NO hand-written form anywhere: Gram build (d = 1 and d > 1), batched fits, predictors,
maps, nll_grad and the 19-function `kernels` module all run the code printed here.  Its definition is USER_FAMILY below
(as shipped: the Henon-Heiles kernel, 03_henon_heiles/init_func.py:24-28, a second time -- so that every path can be held
against the hand-written family C).  To use another kernel: edit USER_FAMILY, run this script, `make`.

    python tools/gen_kernels.py            # rewrites csrc/generated/pair_generated.h and tests/golden/user_family.npz

The .npz is the oracle side of the USER slot: sympy's own numerical evaluation (lambdify) of the same expressions at
random points -- the 19 functions, a d = 1 Gram matrix, a d = 2 Gram matrix -- written by this script, data only.
"""
import os
import sys

import sympy as sp
from sympy.printing.c import C99CodePrinter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "sympgpr_amd", "csrc", "generated", "pair_generated.h")
NPZ_OUT = os.path.join(ROOT, "tests", "golden", "user_family.npz")   # (both destinations are module attributes: the up-to-date test redirects them)

x_a, y_a, x_b, y_b = sp.symbols("x_a y_a x_b y_b", real=True)
lx, ly, p = sp.symbols("lx ly p", positive=True)


per = sp.exp(-sp.sin((x_a - x_b) / 2) ** 2 / (2 * lx ** 2))          # periodic in q, period 2 pi
perp = sp.exp(-sp.sin(p * (x_a - x_b)) ** 2 / (2 * lx ** 2))          # free period
sex = sp.exp(-(x_a - x_b) ** 2 / (2 * lx ** 2))
sey = sp.exp(-(y_a - y_b) ** 2 / (2 * ly ** 2))

# The user's kernel: (factor in the q's, factor in the P's, "prod" | "sum").  Factors are functions of (x_a - x_b; lx[, p])
# resp. (y_a - y_b; ly); with d > 1 pairs per point the same factor is used for every q_m resp. P_m with its own length.
USER_FAMILY = (sex, sey, "prod")


def families():
    """name -> (enum, q-factor, P-factor, mode).  The definitions of the four init_func.py variants + the user slot."""
    return {
        "A": ("SGPR_FAM_A", per, sey, "prod"),     # 01_pendulum/implicit/init_func.py:24-29 (and 02, 04, 05)
        "B": ("SGPR_FAM_B", per, sey, "sum"),      # 01_pendulum/explicit/init_func.py:24-29 (sum kernel)
        "C": ("SGPR_FAM_C", sex, sey, "prod"),     # 03_henon_heiles/init_func.py:24-28
        "D": ("SGPR_FAM_D", perp, sey, "prod"),    # 01_pendulum/implicit_period_unknown/init_func.py:25-30
        "USER": ("SGPR_FAM_USER",) + USER_FAMILY,
    }


def kernel_of(fq, fP, mode):
    return fq * fP if mode == "prod" else fq + fP


# the seven functions of a kernels*.f90 that no caller of the reference uses (kernels.f90:12-57,95-132), by SGPR_K_* code
EXTRA = [(16, "dkdx_num", (x_a,)), (17, "dkdy_num", (y_a,)), (18, "dkdx0_num", (x_b,)), (19, "dkdy0_num", (y_b,)),
         (20, "d3kdxdx0dy0_num", (x_a, x_b, y_b)), (21, "d3kdydy0dy0_num", (y_a, y_b, y_b)), (22, "d3kdxdy0dy0_num", (x_a, y_b, y_b))]


class Printer(C99CodePrinter):
    """integer powers as products (pow() in fp64 on the device is a libm call)"""

    def _print_Pow(self, e):
        b, ex = e.as_base_exp()
        if ex.is_Integer and 2 <= abs(int(ex)) <= 6:
            s = "(" + "*".join(["(%s)" % self._print(b)] * abs(int(ex))) + ")"
            return s if ex > 0 else "(1.0/%s)" % s
        return super()._print_Pow(e)


def emit(exprs, names):
    """C statements computing out[i] = exprs[i] through common sub-expressions"""
    pr = Printer()
    repl, red = sp.cse(exprs, symbols=sp.numbered_symbols("t"), optimizations="basic")
    lines = ["    const double %s = %s;" % (pr.doprint(s), pr.doprint(e)) for s, e in repl]
    lines += ["    out[%d] = %s;   // %s" % (i, pr.doprint(e), names[i]) for i, e in enumerate(red)]
    return "\n".join(lines)


def emit_ret(expr, name):
    """C statements returning expr through common sub-expressions"""
    pr = Printer()
    repl, red = sp.cse([expr], symbols=sp.numbered_symbols("t"), optimizations="basic")
    lines = ["    const double %s = %s;" % (pr.doprint(s), pr.doprint(e)) for s, e in repl]
    lines.append("    return %s;   // %s" % (pr.doprint(red[0]), name))
    return "\n".join(lines)


def main():
    fams = families()
    head = '''// pair_generated.h -- GENERATED by tools/gen_kernels.py from the sympy kernel definitions; do not edit.
//
// For each kernel family of the reference (the init_func.py variants): the four functions that enter the
// Gram matrix and their length-scale derivatives, differentiated symbolically and printed as C.  All values
// WITHOUT the sig factor; argument order as in the generated Fortran (x_a, y_a, x_b, y_b, lx, ly[, p]).
//   gen::pair<FAM>(...,    out): out = { k, d2k/dx_a dx_b, d2k/dy_a dy_b, d2k/dx_a dy_b }
//   gen::pair_dlx<FAM>(..., out), gen::pair_dly<FAM>(..., out): the same four differentiated by lx / ly
//     (dkdlx_num, d3kdxdx0dlx_num, d3kdydy0dlx_num, d3kdxdy0dlx_num and the ly set).
#pragma once
#include "../common.h"

namespace sgpr {
namespace gen {

template <int FAM> __device__ __forceinline__ void pair(double x_a, double y_a, double x_b, double y_b, double lx, double ly, double p, double *out);
template <int FAM> __device__ __forceinline__ void pair_dlx(double x_a, double y_a, double x_b, double y_b, double lx, double ly, double p, double *out);
template <int FAM> __device__ __forceinline__ void pair_dly(double x_a, double y_a, double x_b, double y_b, double lx, double ly, double p, double *out);
//   gen::pair_dp<FAM>(..., out): the same four differentiated by the period p (all zero for a family without one)
template <int FAM> __device__ __forceinline__ void pair_dp(double x_a, double y_a, double x_b, double y_b, double lx, double ly, double p, double *out);
//   gen::extra<FAM>(which, ...): the seven functions no caller of the reference uses, by SGPR_K_* code (16 .. 22): with pair,
//     pair_dlx and pair_dly all 19 functions of a kernels*.f90
//   gen::factor<FAM, Q>(dx, l, p, out): one coordinate's factor f of the d > 1 product / sum kernel (Q = 1: a q, Q = 0: a P):
//     out = { log f, f'/f, -f''/f };  gen::factor_dl<FAM, Q>: the same three differentiated by the length l
//     gen::factor_dp<FAM, Q>: the same three differentiated by the period p (all zero for a factor without one)
template <int FAM> __device__ double extra(int which, double x_a, double y_a, double x_b, double y_b, double lx, double ly, double p);
template <int FAM, int Q> __device__ __forceinline__ void factor(double dx, double l, double p, double *out);
template <int FAM, int Q> __device__ __forceinline__ void factor_dl(double dx, double l, double p, double *out);
template <int FAM, int Q> __device__ __forceinline__ void factor_dp(double dx, double l, double p, double *out);
//   gen::factor3<FAM, Q>(dx, l, p): f(3)/f, the third derivative of the same factor over f -- with f'/f and -f''/f all that the
//     Hessian of K*(x) alpha needs
//     (the tangent map of the d-pair symplectic map, maptan.h)
template <int FAM, int Q> __device__ __forceinline__ double factor3(double dx, double l, double p);
'''
    body = []
    names = ["k", "d2k/dx_a dx_b", "d2k/dy_a dy_b", "d2k/dx_a dy_b"]
    dx = sp.Symbol("dx", real=True)
    l = sp.Symbol("l", positive=True)
    for fam, (enum, fq, fP, mode) in fams.items():
        k = kernel_of(fq, fP, mode)
        four = [k, sp.diff(k, x_a, x_b), sp.diff(k, y_a, y_b), sp.diff(k, x_a, y_b)]
        for fn, var in (("pair", None), ("pair_dlx", lx), ("pair_dly", ly), ("pair_dp", p)):
            ex = four if var is None else [sp.diff(e, var) for e in four]
            nm = names if var is None else ["d/d%s %s" % (var, n) for n in names]
            body.append("// family %s: k = %s\ntemplate <> __device__ __forceinline__ void %s<%s>(double x_a, double y_a, double x_b, "
                        "double y_b, double lx, double ly, double p, double *out)\n{\n    (void)p;\n%s\n}\n"
                        % (fam, sp.sstr(k), fn, enum, emit(ex, nm)))
        # the seven extra functions
        pr = Printer()
        cases = "\n".join("    case %d: return %s;   // %s" % (code, pr.doprint(sp.diff(k, *wrt)), name) for code, name, wrt in EXTRA)
        body.append("template <> __device__ inline double extra<%s>(int which, double x_a, double y_a, double x_b, double y_b, "
                    "double lx, double ly, double p)\n{\n    (void)p;\n    switch (which) {\n%s\n    }\n    return 0.0;\n}\n"
                    % (enum, cases))
        # one coordinate's factor: f(dx; l[, p]) with dx = x_a - x_b  ->  log f, f'/f, -f''/f  and their l-derivatives
        for Q, f, lsym, a, b in ((1, fq, lx, x_a, x_b), (0, fP, ly, y_a, y_b)):
            fd = f.subs({a: dx, b: 0, lsym: l})
            three = [sp.simplify(sp.log(fd)), sp.simplify(sp.diff(fd, dx) / fd), sp.simplify(-sp.diff(fd, dx, 2) / fd)]
            nm3 = ["log f", "f'/f", "-f''/f"]
            for fn, ex, nm in (("factor", three, nm3), ("factor_dl", [sp.diff(e, l) for e in three], ["d/dl " + n for n in nm3]),
                               ("factor_dp", [sp.diff(e, p) for e in three], ["d/dp " + n for n in nm3])):
                body.append("template <> __device__ __forceinline__ void %s<%s, %d>(double dx, double l, double p, double *out)\n"
                            "{\n    (void)p;\n%s\n}\n" % (fn, enum, Q, emit(ex, nm)))
    # the third logarithmic derivative of every factor, after everything else: what was printed before it keeps its text
    for fam, (enum, fq, fP, mode) in fams.items():
        for Q, f, lsym, a, b in ((1, fq, lx, x_a, x_b), (0, fP, ly, y_a, y_b)):
            fd = f.subs({a: dx, b: 0, lsym: l})
            body.append("template <> __device__ __forceinline__ double factor3<%s, %d>(double dx, double l, double p)\n"
                        "{\n    (void)p;\n%s\n}\n" % (enum, Q, emit_ret(sp.simplify(sp.diff(fd, dx, 3) / fd), "f(3)/f")))
    ufq, ufP, umode = USER_FAMILY
    body.append("// the user slot's shape: sum or product of its two factors; does its q-factor take the extra parameter p\n"
                "// (then hyp = (lx, ly, p, sig) like family D, and (lq.., lP.., p_1..p_d, sig) for d > 1)\n"
                "constexpr bool user_is_sum = %s;\nconstexpr bool user_has_p = %s;\n"
                "// k is the sum of its factors, not their product (family B, or a user slot of that shape)\n"
                "template <int FAM> constexpr bool is_sum() { return FAM == SGPR_FAM_B || (FAM == SGPR_FAM_USER && user_is_sum); }\n"
                % ("true" if umode == "sum" else "false", "true" if p in kernel_of(ufq, ufP, umode).free_symbols else "false"))
    tail = "\n}  // namespace gen\n}  // namespace sgpr\n"
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(head + "\n" + "\n".join(body) + tail)
    print("wrote", os.path.relpath(OUT, ROOT), "(%d functions)" % len(body))
    write_user_fixture()


FUNCS19 = [("kern_num", ()), ("dkdx_num", (x_a,)), ("dkdy_num", (y_a,)), ("dkdx0_num", (x_b,)), ("dkdy0_num", (y_b,)),
           ("d2kdxdx0_num", (x_a, x_b)), ("d2kdydy0_num", (y_a, y_b)), ("d2kdxdy0_num", (x_a, y_b)),
           ("d3kdxdx0dy0_num", (x_a, x_b, y_b)), ("d3kdydy0dy0_num", (y_a, y_b, y_b)), ("d3kdxdy0dy0_num", (x_a, y_b, y_b)),
           ("dkdlx_num", (lx,)), ("dkdly_num", (ly,)), ("d3kdxdx0dlx_num", (x_a, x_b, lx)), ("d3kdydy0dlx_num", (y_a, y_b, lx)),
           ("d3kdxdy0dlx_num", (x_a, y_b, lx)), ("d3kdxdx0dly_num", (x_a, x_b, ly)), ("d3kdydy0dly_num", (y_a, y_b, ly)),
           ("d3kdxdy0dly_num", (x_a, y_b, ly))]          # the 19 functions of init_func.py:55-76, by name


def write_user_fixture():
    """tests/golden/user_family.npz: the oracle side of SGPR_FAM_USER -- sympy's own numerical evaluation (lambdify ->
    numpy) of the expressions the device code above was printed from.  Data only."""
    import numpy as np
    fq, fP, mode = USER_FAMILY
    k = kernel_of(fq, fP, mode)
    has_p = p in k.free_symbols
    rng = np.random.default_rng(2718)
    m = 96
    pts = dict(xa=rng.uniform(0, 2 * np.pi, m), ya=rng.uniform(-3, 3, m), xb=rng.uniform(0, 2 * np.pi, m), yb=rng.uniform(-3, 3, m))
    lv, pv = np.array([0.7, 1.3]), 0.6
    out = dict(pts, l=lv, p=pv, has_p=has_p, is_sum=(mode == "sum"), definition=sp.sstr(k))
    args = (x_a, y_a, x_b, y_b, lx, ly, p)
    for name, wrt in FUNCS19:
        f = sp.lambdify(args, sp.diff(k, *wrt) if wrt else k, "numpy")
        out["f_" + name] = np.broadcast_to(f(pts["xa"], pts["ya"], pts["xb"], pts["yb"], lv[0], lv[1], pv), (m,)).astype(float)
    # d = 1 Gram matrix as build_K lays it out (sympgpr.f90:12-38): rows = points (x, y), columns = points (x0, y0),
    # every entry f(x0(j), y0(j), x(i), y(i)) -- the COLUMN point is "a"
    n, n0, sig = 12, 9, 1.7
    x, y, x0, y0 = rng.uniform(0, 6, n), rng.uniform(-2, 2, n), rng.uniform(0, 6, n0), rng.uniform(-2, 2, n0)
    fxx, fyy, fxy = (sp.lambdify(args, sp.diff(k, *w), "numpy") for w in ((x_a, x_b), (y_a, y_b), (x_a, y_b)))
    A = lambda f: np.broadcast_to(f(x0[None, :], y0[None, :], x[:, None], y[:, None], lv[0], lv[1], pv), (n, n0))
    K1 = sig * np.block([[A(fxx), A(fxy)], [A(fxy), A(fyy)]])
    out.update(g1_x=x, g1_y=y, g1_x0=x0, g1_y0=y0, g1_sig=sig, g1_K=K1)
    # d = 2: x = (q_1, q_2, P_1, P_2), k = prod (or sum) of the factors, each coordinate with its own length (and period);
    # K block (r, c) = d2k / d(row point)_r d(column point)_c
    d = 2
    u = sp.symbols("u0:%d" % (2 * d), real=True)       # row point
    v = sp.symbols("v0:%d" % (2 * d), real=True)       # column point
    ls = sp.symbols("l0:%d" % (2 * d), positive=True)
    ps = sp.symbols("p0:%d" % d, positive=True)
    facs = [fq.subs({x_a: v[mm], x_b: u[mm], lx: ls[mm], p: ps[mm]}, simultaneous=True) for mm in range(d)] + \
           [fP.subs({y_a: v[d + mm], y_b: u[d + mm], ly: ls[d + mm]}, simultaneous=True) for mm in range(d)]
    kd = sp.Mul(*facs) if mode == "prod" else sp.Add(*facs)
    nn, nn0, sig2 = 7, 5, 0.9
    X, X0 = rng.uniform(-1.5, 1.5, (nn, 2 * d)), rng.uniform(-1.5, 1.5, (nn0, 2 * d))
    lvals, pvals = np.array([0.8, 1.1, 0.9, 1.4]), np.array([0.6, 0.45])
    K2 = np.empty((2 * d * nn, 2 * d * nn0))
    for r in range(2 * d):
        for c in range(2 * d):
            f = sp.lambdify(u + v + ls + ps, sp.diff(kd, u[r], v[c]), "numpy")
            cols = [X[:, i][:, None] for i in range(2 * d)] + [X0[:, i][None, :] for i in range(2 * d)]
            K2[r * nn:(r + 1) * nn, c * nn0:(c + 1) * nn0] = sig2 * np.broadcast_to(f(*cols, *lvals, *pvals), (nn, nn0))
    out.update(g2_X=X, g2_X0=X0, g2_l=lvals, g2_p=pvals, g2_sig=sig2, g2_K=K2)
    dst = NPZ_OUT
    np.savez_compressed(dst, **out)
    print("wrote", os.path.relpath(dst, ROOT) if dst.startswith(ROOT) else dst)


if __name__ == "__main__":
    sys.exit(main())
