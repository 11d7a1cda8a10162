"""Device checks of the outer Strassen level (csrc/strassen.hip), one mode per process because the tunables are read once:
    python tools/strassen2_check.py four   OUT.json   the product with 2 .. 4 destinations against separate classical launches
    python tools/strassen2_check.py front  OUT.json   the front end against the classical kernel on the same operands
    python tools/strassen2_check.py potrf  OUT.npz    factor + solve through the recursive driver (order 4096, la_max = 1024)
Environment: STRASSEN_MIN / STRASSEN_KSLAB / STRASSEN2_MIN / STRASSEN2_KSLAB / STRASSEN_NOSCRATCH / STRASSEN2_NOSCRATCH /
STRASSEN_LA_MAX set the tunables before the first call; STRASSEN2_SAVE=1 makes `front` store every result beside OUT.json; SGPR_GEMM_STRASSEN (0: classical, 1: one level) and SGPR_GEMM_KMAX are
read by the library itself.  tests/test_gpu_strassen2.py runs each mode under its own time limit."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from strassen_check import dev, host, p  # noqa: E402

TUNABLES = (("STRASSEN_MIN", "gemm_strassen_min"), ("STRASSEN_KSLAB", "gemm_strassen_kslab"),
            ("STRASSEN2_MIN", "gemm_strassen2_min"), ("STRASSEN2_KSLAB", "gemm_strassen2_kslab"),
            ("STRASSEN_NOSCRATCH", "gemm_strassen_noscratch"), ("STRASSEN2_NOSCRATCH", "gemm_strassen2_noscratch"),
            ("STRASSEN_LA_MAX", "la_max"))


def setup():
    import torch
    from sympgpr_amd import _lib as L
    lib, probe = L.load_library(), L.load_probe_library()
    L.check(lib.sgpr_set_device(0))
    for env, name in TUNABLES:
        if os.environ.get(env):
            L.check(probe.sgpr_probe_tune(name.encode(), float(os.environ[env])))
    return torch, L, lib, probe


def four(out):
    """destinations = blocks of ONE array at different offsets; (m, n, k, alphas, beta): len(alphas) destinations"""
    torch, L, lib, probe = setup()
    res = []
    shapes = [tuple(int(v) for v in s.split("x")) for s in os.environ["STRASSEN2_SHAPES"].split(",")]
    cases = [((-1.0, 1.0, -1.0, 1.0), 1.0), ((1.0, -1.0, 1.0), 1.0), ((-1.0, 1.0), 1.0), ((0.7, -0.3, 1.0, 2.5), 0.5)]
    for (m, n, k) in shapes:
        for alphas, beta in cases:
            cnt = len(alphas)
            rng = np.random.default_rng(m + n + k + cnt)
            A, B = rng.uniform(-1, 1, (m, k)), rng.uniform(-1, 1, (n, k))
            # one array of 2 x 2 blocks with a margin around each; block d at (row, column) offs[d], leading dimension ld
            ld, cols = 2 * m + 6, 2 * n + 3
            offs = [(2, 1), (m + 4, 1), (2, n + 2), (m + 4, n + 2)][:cnt]
            W = rng.uniform(-1, 1, (ld, cols))
            dA, dB, ref, got = dev(torch, A), dev(torch, B), dev(torch, W), dev(torch, W)
            torch.cuda.synchronize()
            size = ref.element_size()
            addr = lambda t, o: t.data_ptr() + size * (o[0] + o[1] * ld)  # noqa: E731
            for d, o in enumerate(offs):
                L.check(lib.sgpr_gemm_nt_dev(m, n, k, alphas[d], p(dA), m, p(dB), n, beta if d == 0 else 1.0, C.c_void_p(addr(ref, o)), ld, 0, 0, None))
            cs = (C.c_void_p * cnt)(*[addr(got, o) for o in offs])
            ls = (C.c_size_t * cnt)(*([ld] * cnt))
            al = (C.c_double * cnt)(*alphas)
            L.check(probe.sgpr_probe_gemm_nt4_dev(m, n, k, p(dA), m, p(dB), n, beta, cnt, cs, ls, al, None))
            torch.cuda.synchronize()
            h_ref, h_got = host(ref), host(got)
            blocks = []
            mask = np.ones_like(W, dtype=bool)
            for d, (r0, c0) in enumerate(offs):
                a, b = h_ref[r0:r0 + m, c0:c0 + n], h_got[r0:r0 + m, c0:c0 + n]
                mask[r0:r0 + m, c0:c0 + n] = False
                blocks.append({"alpha": alphas[d], "bitwise": bool(np.array_equal(a.view(np.uint64), b.view(np.uint64))),
                               "max_diff": float(np.abs(a - b).max()), "max": float(np.abs(a).max()),
                               "changed": bool(not np.array_equal(a, W[r0:r0 + m, c0:c0 + n]))})
            res.append({"m": m, "n": n, "k": k, "count": cnt, "beta": beta, "blocks": blocks,
                        "outside_untouched": bool(np.array_equal(h_got[mask], W[mask])),
                        "operands_untouched": bool(np.array_equal(host(dA), A) and np.array_equal(host(dB), B))})
    json.dump(res, open(out, "w"))


def front(out):
    """every shape through the front end (levels as the environment says) and through the classical kernel"""
    torch, L, lib, probe = setup()
    res = []
    shapes = [tuple(int(v) for v in s.split("x")) for s in os.environ["STRASSEN2_SHAPES"].split(",")]
    for (m, n, k, lower) in shapes:
        rng = np.random.default_rng(m + 3 * n + 7 * k + lower)
        A = rng.uniform(-1, 1, (m, k))
        B = A if lower else rng.uniform(-1, 1, (n, k))
        C0 = rng.uniform(-1, 1, (m, n))
        dA, dB = dev(torch, A), dev(torch, B)
        c_cl, c_st = dev(torch, C0), dev(torch, C0)
        torch.cuda.synchronize()
        L.check(lib.sgpr_gemm_nt_dev(m, n, k, -1.0, p(dA), m, p(dB), n, 1.0, p(c_cl), m, lower, 0, None))
        L.check(probe.sgpr_probe_gemm_strassen_dev(m, n, k, -1.0, p(dA), m, p(dB), n, 1.0, p(c_st), m, lower, None))
        torch.cuda.synchronize()
        h_cl, h_st = host(c_cl), host(c_st)
        ref = C0 - A @ B.T
        if lower:
            h_cl, h_st, ref = np.tril(h_cl), np.tril(h_st), np.tril(ref)
        if os.environ.get("STRASSEN2_SAVE"):       # the result itself, for a bitwise comparison between two processes
            np.save("%s.%dx%dx%d_%d.npy" % (out, m, n, k, lower), h_st)
        res.append({"m": m, "n": n, "k": k, "lower": lower, "max_diff": float(np.abs(h_cl - h_st).max()),
                    "bitwise": bool(np.array_equal(h_cl.view(np.uint64), h_st.view(np.uint64))),
                    "max_a": float(np.abs(A).max()), "max_b": float(np.abs(B).max()), "max_c0": float(np.abs(C0).max()),
                    "classical_vs_numpy": float(np.abs(h_cl - ref).max()), "strassen_vs_numpy": float(np.abs(h_st - ref).max()),
                    "operands_untouched": bool(np.array_equal(host(dA), A) and np.array_equal(host(dB), B))})
    L.check(lib.sgpr_trim())
    json.dump(res, open(out, "w"))


def potrf(out):
    import strassen_check
    strassen_check.setup = setup          # the same factor + solve, with this file's tunables
    strassen_check.potrf(out)


if __name__ == "__main__":
    {"four": four, "front": front, "potrf": potrf}[sys.argv[1]](sys.argv[2])
