"""Device checks of the Strassen front end (csrc/strassen.hip), one mode per process because the tunables are read once:
    python tools/strassen_check.py front  OUT.json   front end against the classical kernel on the same operands
    python tools/strassen_check.py two    OUT.json   the two-destination product against two classical launches
    python tools/strassen_check.py potrf  OUT.npz    factor + solve through the recursive driver (order 4096, la_max = 1024)
Environment: STRASSEN_MIN / STRASSEN_KSLAB / STRASSEN_NOSCRATCH set the tunables before the first call; SGPR_GEMM_STRASSEN=0
and SGPR_GEMM_KMAX are read by the library itself.  tests/test_gpu_strassen.py runs each mode under its own time limit."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def setup():
    import torch
    from sympgpr_amd import _lib as L
    lib, probe = L.load_library(), L.load_probe_library()
    L.check(lib.sgpr_set_device(0))
    for env, name in (("STRASSEN_MIN", "gemm_strassen_min"), ("STRASSEN_KSLAB", "gemm_strassen_kslab"),
                      ("STRASSEN_NOSCRATCH", "gemm_strassen_noscratch"), ("STRASSEN_LA_MAX", "la_max")):
        if os.environ.get(env):
            L.check(probe.sgpr_probe_tune(name.encode(), float(os.environ[env])))
    return torch, L, lib, probe


def dev(torch, a):
    """(rows, cols) numpy -> column-major device buffer (a contiguous (cols, rows) tensor)"""
    return torch.from_numpy(np.ascontiguousarray(a.T)).to("cuda")


def host(t):
    return t.cpu().numpy().T.copy()


def p(t):
    return C.c_void_p(t.data_ptr())


def front(out):
    torch, L, lib, probe = setup()
    res = []
    shapes = [tuple(int(v) for v in s.split("x")) for s in os.environ["STRASSEN_SHAPES"].split(",")]
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
            # a lower update works tile by tile: what the tiles on the diagonal leave above it is not part of the result
            h_cl, h_st, ref = np.tril(h_cl), np.tril(h_st), np.tril(ref)
        res.append({"m": m, "n": n, "k": k, "lower": lower, "max_diff": float(np.abs(h_cl - h_st).max()),
                    "bitwise": bool(np.array_equal(h_cl.view(np.uint64), h_st.view(np.uint64))),
                    "max_a": float(np.abs(A).max()), "max_b": float(np.abs(B).max()),
                    "classical_vs_numpy": float(np.abs(h_cl - ref).max()), "strassen_vs_numpy": float(np.abs(h_st - ref).max()),
                    "operands_untouched": bool(np.array_equal(host(dA), A) and np.array_equal(host(dB), B))})
    L.check(lib.sgpr_trim())
    json.dump(res, open(out, "w"))


def two(out):
    torch, L, lib, probe = setup()
    res = []
    for (m, n, k, a1, beta, a2) in [(4096, 2048, 512, -1.0, 1.0, 1.0), (4096, 2048, 1040, 1.0, 1.0, -1.0),
                                    (4100, 2050, 520, -1.0, 0.5, 0.3), (4096, 2048, 256, 2.0, 0.0, -1.0)]:
        rng = np.random.default_rng(m + n + k)
        A, B = rng.uniform(-1, 1, (m, k)), rng.uniform(-1, 1, (n, k))
        C1, C2 = rng.uniform(-1, 1, (m, n)), rng.uniform(-1, 1, (m, n))
        dA, dB = dev(torch, A), dev(torch, B)
        r1, r2, t1, t2 = dev(torch, C1), dev(torch, C2), dev(torch, C1), dev(torch, C2)
        torch.cuda.synchronize()
        L.check(lib.sgpr_gemm_nt_dev(m, n, k, a1, p(dA), m, p(dB), n, beta, p(r1), m, 0, 0, None))
        L.check(lib.sgpr_gemm_nt_dev(m, n, k, a2, p(dA), m, p(dB), n, 1.0, p(r2), m, 0, 0, None))
        L.check(probe.sgpr_probe_gemm_nt2_dev(m, n, k, a1, p(dA), m, p(dB), n, beta, p(t1), m, a2, p(t2), m, None))
        torch.cuda.synchronize()
        h1, h2, g1, g2 = host(r1), host(r2), host(t1), host(t2)
        res.append({"m": m, "n": n, "k": k, "alpha2": a2,
                    "first_bitwise": bool(np.array_equal(h1.view(np.uint64), g1.view(np.uint64))),
                    "second_bitwise": bool(np.array_equal(h2.view(np.uint64), g2.view(np.uint64))),
                    "second_max_diff": float(np.abs(h2 - g2).max()), "second_max": float(np.abs(h2).max())})
    json.dump(res, open(out, "w"))


def potrf(out):
    torch, L, lib, probe = setup()
    n = 4096
    rng = np.random.default_rng(11)
    G = rng.standard_normal((n, n))
    A = G @ G.T / n + np.eye(n)
    z = rng.standard_normal(n)
    dA = dev(torch, np.tril(A))
    work = torch.zeros(((lib.sgpr_potrf_workspace(n) + 7) // 8,), dtype=torch.float64, device="cuda")
    info = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    b = torch.from_numpy(z.copy()).to("cuda")
    torch.cuda.synchronize()
    L.check(lib.sgpr_potrf_dev(n, p(dA), n, p(work), 8 * work.numel(), p(info), None))
    torch.cuda.synchronize()
    L.check(lib.sgpr_potrf_info_dev(int(info.item()), None))
    L.check(lib.sgpr_potrs_vec_dev(n, p(dA), n, p(work), p(b), None))
    torch.cuda.synchronize()
    Lf = np.tril(host(dA))
    x = b.cpu().numpy()
    np.savez(out, L=Lf, x=x, A=A, z=z)
    L.check(lib.sgpr_trim())


if __name__ == "__main__":
    {"front": front, "two": two, "potrf": potrf}[sys.argv[1]](sys.argv[2])
