"""Device checks of the top Strassen level (csrc/strassen.hip: strassen_top_gemm), one mode per process because the library's
tunables are read once:
    python tools/strassen_top_check.py front OUT.json   one product through the recursion's entry with the top level (twice), through
                                                        the entry it replaced (gemm_nt_strassen_rec) and through the classical kernel
    python tools/strassen_top_check.py potrf OUT.npz    factor + solve through potrf_rec (tools/strassen_rec_check.py)
Environment: TOP_SHAPE="m,n,k,lower" (front); REC_N (potrf); REC_TUNE="name=value,..." sets tunables through sgpr_probe_tune before
the first call; SGPR_GEMM_STRASSEN is read by the library itself.  tests/test_gpu_strassen_top.py runs each configuration under
its own time limit."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from strassen_check import dev, host, p  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def front(out):
    import torch
    from sympgpr_amd import _lib as L
    lib, probe = L.load_library(), L.load_probe_library()
    L.check(lib.sgpr_set_device(0))
    for item in filter(None, os.environ.get("REC_TUNE", "").split(",")):
        name, v = item.split("=")
        L.check(probe.sgpr_probe_tune(name.encode(), float(v)))
    m, n, k, lower = (int(v) for v in os.environ["TOP_SHAPE"].split(","))
    rng = np.random.default_rng(m + 3 * n + 7 * k + lower)
    A = rng.uniform(-1, 1, (m, k))
    B = A if lower else rng.uniform(-1, 1, (n, k))
    C0 = rng.uniform(-1, 1, (m, n))
    dA = dev(torch, A)
    dB = dA if lower else dev(torch, B)
    c_cl, c_top, c_again, c_rec = (dev(torch, C0) for _ in range(4))
    torch.cuda.synchronize()
    L.check(lib.sgpr_gemm_nt_dev(m, n, k, -1.0, p(dA), m, p(dB), n, 1.0, p(c_cl), m, lower, 0, None))
    L.check(probe.sgpr_probe_gemm_strassen_top_dev(m, n, k, -1.0, p(dA), m, p(dB), n, 1.0, p(c_top), m, lower, None))
    L.check(probe.sgpr_probe_gemm_strassen_top_dev(m, n, k, -1.0, p(dA), m, p(dB), n, 1.0, p(c_again), m, lower, None))
    L.check(probe.sgpr_probe_gemm_strassen_rec_dev(m, n, k, -1.0, p(dA), m, p(dB), n, 1.0, p(c_rec), m, lower, None))
    torch.cuda.synchronize()
    h_cl, h_top, h_again, h_rec = host(c_cl), host(c_top), host(c_again), host(c_rec)
    ref = C0 - A @ B.T
    if lower:      # (the diagonal tiles are written whole: what lies above the diagonal is not part of the result)
        h_cl, h_top, h_again, h_rec, ref = (np.tril(x) for x in (h_cl, h_top, h_again, h_rec, ref))
    res = {"m": m, "n": n, "k": k, "lower": lower, "sha": sha(h_top), "again_same": sha(h_again) == sha(h_top),
           "same_as_replaced_entry": sha(h_rec) == sha(h_top), "same_as_classical": sha(h_cl) == sha(h_top),
           "max_diff": float(np.abs(h_cl - h_top).max()), "max_a": float(np.abs(A).max()), "max_b": float(np.abs(B).max()),
           "max_c0": float(np.abs(C0).max()), "classical_vs_numpy": float(np.abs(h_cl - ref).max()),
           "top_vs_numpy": float(np.abs(h_top - ref).max()), "replaced_vs_numpy": float(np.abs(h_rec - ref).max()),
           "operands_untouched": bool(np.array_equal(host(dA), A) and np.array_equal(host(dB), B))}
    L.check(lib.sgpr_trim())
    json.dump(res, open(out, "w"))


def potrf(out):
    import strassen_rec_check
    strassen_rec_check.main(out)


if __name__ == "__main__":
    {"front": front, "potrf": potrf}[sys.argv[1]](sys.argv[2])
