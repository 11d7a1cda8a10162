"""The Strassen front end with its operand sums on side streams beside the products (sympgpr_amd/csrc/strassen.hip: run_schedule,
tunable gemm_strassen_overlap), inside the recursive factorisation with the recursion's tunables and la_max scaled down by 32 as in
tests/test_gpu_strassen_rec.py: at order 4096 trsm_rec's products and the lower update take both levels, at 4096 + 384 some products
fall through to classical launches beside the ones that qualify.  potrf() reserves the scratch of the largest call, so the smaller
calls find slack for second buffers (gemm_strassen_overlap_slack = -1) -- or none (0: single buffers, the "other side is free"
overlap alone).

The arithmetic and the order of accumulation into C are those of the serial execution, so L and x must be the SAME BITS with the
overlap on and off, and the same again in a second run: any difference is a race.  Nothing here loops or retries.

Every device step is a child process (tools/strassen_rec_check.py) under its own time limit, one per configuration, shared by the
tests."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tests/test_gpu_strassen_rec.py: the recursion's own values scaled by 1 / 32
REC = {"rec_strassen_min_gemm": 128, "rec_strassen_min_syrk": 128, "rec_strassen2_min_gemm": 256, "rec_strassen2_min_syrk": 256,
       "rec_strassen_kslab": 512, "rec_strassen2_kslab": 1024, "rec_strassen2_kslab_short": 512, "la_max": 1024}
OFF = dict(REC, gemm_strassen_overlap=0)
ON = dict(REC, gemm_strassen_overlap=1, gemm_strassen_overlap_slack=-1)
ON_SINGLE = dict(REC, gemm_strassen_overlap=1, gemm_strassen_overlap_slack=0)
_runs = {}


def run(tmp_path_factory, name, n, tune, strassen=None):
    """factor + solve in a child process; one run per name"""
    if name not in _runs:
        out = tmp_path_factory.mktemp("overlap") / (name + ".npz")
        env = dict(os.environ)
        for k in ("SGPR_GEMM_STRASSEN", "SGPR_GEMM_KMAX", "SGPR_LA_MAX", "SGPR_POTRF"):
            env.pop(k, None)
        env.update({"REC_N": str(n), "REC_TUNE": ",".join("%s=%d" % kv for kv in tune.items())})
        if strassen is not None:
            env["SGPR_GEMM_STRASSEN"] = strassen
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tools", "strassen_rec_check.py"), str(out)]
        r = subprocess.run(cmd, env=env, cwd=ROOT, timeout=300, capture_output=True, text=True)
        assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        _runs[name] = np.load(out)
    return _runs[name]


def same_bits(a, b):
    return (np.array_equal(a["L"].view(np.uint64), b["L"].view(np.uint64)) and
            np.array_equal(a["x"].view(np.uint64), b["x"].view(np.uint64)))


@pytest.mark.parametrize("which,tune", [("on", ON), ("single", ON_SINGLE)], ids=["slack-1", "slack0"])
@pytest.mark.parametrize("n", [4096, 4096 + 384])
def test_overlap_gives_the_serial_bits(tmp_path_factory, n, which, tune):
    """second buffers out of the slack (-1) and single buffers (0) against the serial execution"""
    off = run(tmp_path_factory, "off%d" % n, n, OFF)
    assert np.isfinite(off["L"]).all() and np.isfinite(off["x"]).all()
    assert same_bits(run(tmp_path_factory, "%s%d" % (which, n), n, tune), off)


@pytest.mark.parametrize("n", [4096, 4096 + 384])
def test_second_run_gives_the_same_bits(tmp_path_factory, n):
    assert same_bits(run(tmp_path_factory, "again%d" % n, n, ON), run(tmp_path_factory, "on%d" % n, n, ON))


def test_two_side_streams_give_the_serial_bits(tmp_path_factory):
    two = run(tmp_path_factory, "two4096", 4096, dict(ON_SINGLE, gemm_strassen_overlap_streams=2))
    assert same_bits(two, run(tmp_path_factory, "off4096", 4096, OFF))


def test_one_level_alone(tmp_path_factory):
    """SGPR_GEMM_STRASSEN=1: the inner level only (the library's thresholds at the same scale), its two regions"""
    lib = {"gemm_strassen_min": 256, "gemm_strassen_kslab": 512, "la_max": 1024}
    on = run(tmp_path_factory, "env1on", 4096, dict(lib, gemm_strassen_overlap=1, gemm_strassen_overlap_slack=-1), strassen="1")
    off = run(tmp_path_factory, "env1off", 4096, dict(lib, gemm_strassen_overlap=0), strassen="1")
    assert same_bits(on, off)
    both = run(tmp_path_factory, "off4096", 4096, OFF)
    assert not np.array_equal(off["L"], both["L"]), "one level must differ from two"


def test_without_the_outer_pair(tmp_path_factory):
    on = run(tmp_path_factory, "noouter_on", 4096, dict(ON, gemm_strassen2_noscratch=1))
    off = run(tmp_path_factory, "noouter_off", 4096, dict(OFF, gemm_strassen2_noscratch=1))
    assert same_bits(on, off)
