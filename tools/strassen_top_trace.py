"""What a kernel trace of a step (rocprofv3 --kernel-trace, the *_kernel_trace.csv) says about the passes of the top Strassen
level: per kernel class launches and total time, and for the streaming passes (block_sum_kernel, block_acc_kernel, the fill kernel
of the memsets) the part that lies inside the interval of some product kernel.
    python tools/strassen_top_trace.py TRACE.csv [STEPS]
STEPS: factorisations the trace covers (totals are divided by it)."""
import csv
import sys

from strassen_overlap_trace import covered, merged

CLASSES = (("gemm_nt_kernel<256,128>", lambda n: "gemm_nt_kernel" in n and "256" in n), ("gemm_nt2_kernel", lambda n: "gemm_nt2_kernel" in n),
           ("gemm_nt4_kernel", lambda n: "gemm_nt4_kernel" in n), ("block_sum_kernel", lambda n: "block_sum_kernel" in n),
           ("block_acc_kernel", lambda n: "block_acc_kernel" in n), ("memset (fill kernel)", lambda n: "fillBuffer" in n))

if __name__ == "__main__":
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    ivs = {name: [] for name, _ in CLASSES}
    with open(sys.argv[1], newline="") as f:
        for row in csv.DictReader(f):
            for name, match in CLASSES:
                if match(row["Kernel_Name"]):
                    ivs[name].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
                    break
    prod = merged(sorted(ivs["gemm_nt_kernel<256,128>"] + ivs["gemm_nt2_kernel"] + ivs["gemm_nt4_kernel"]))
    print("product kernels together: %.1f ms per step (union of their intervals %.1f ms)"
          % (sum(b - a for k in list(ivs)[:3] for a, b in ivs[k]) / 1e6 / steps, sum(b - a for a, b in prod) / 1e6 / steps))
    for i, (name, _) in enumerate(CLASSES):
        v = sorted(ivs[name])
        t = sum(b - a for a, b in v)
        line = "%-24s %5d launches %9.1f ms per step" % (name, len(v) // steps, t / 1e6 / steps)
        if i >= 3:
            inside = covered(v, prod)
            line += ", %8.1f ms (%.1f %%) inside a product kernel's interval" % (inside / 1e6 / steps, 100.0 * inside / max(t, 1))
        print(line)
