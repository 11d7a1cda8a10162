"""Device check of the recursive factorisation's own Strassen thresholds (csrc/chol.hip, csrc/strassen.hip): factor + solve of one
SPD matrix through potrf_rec, one process per configuration because the library's tunables are read once:
    python tools/strassen_rec_check.py OUT.npz
Environment: REC_N (order, 4096); REC_TUNE="name=value,..." sets tunables through sgpr_probe_tune before the first call (the
recursion's rec_strassen_*, the library's gemm_strassen*, la_max); SGPR_GEMM_STRASSEN is read by the library itself.
tests/test_gpu_strassen_rec.py runs each configuration under its own time limit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from strassen_check import dev, host, p  # noqa: E402


def matrix(n):
    rng = np.random.default_rng(11 + n)
    G = rng.standard_normal((n, n))
    return G @ G.T / n + np.eye(n), rng.standard_normal(n)


def main(out):
    import torch
    from sympgpr_amd import _lib as L
    lib, probe = L.load_library(), L.load_probe_library()
    L.check(lib.sgpr_set_device(0))
    for item in filter(None, os.environ.get("REC_TUNE", "").split(",")):
        name, v = item.split("=")
        L.check(probe.sgpr_probe_tune(name.encode(), float(v)))
    n = int(os.environ.get("REC_N", "4096"))
    A, z = matrix(n)
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
    np.savez(out, L=np.tril(host(dA)), x=b.cpu().numpy())
    L.check(lib.sgpr_trim())


if __name__ == "__main__":
    main(sys.argv[1])
