"""What a kernel trace of a step (rocprofv3 --kernel-trace, the *_kernel_trace.csv) says about the operand sums of the Strassen
front end: total time of the product kernels (gemm_nt_kernel<256,128>, gemm_nt2_kernel, gemm_nt4_kernel), total time of
block_sum_kernel, and the part of the latter that lies inside the interval of some product kernel.
    python tools/strassen_overlap_trace.py TRACE.csv [STEPS]
STEPS: factorisations the trace covers (totals are divided by it)."""
import csv
import sys


def intervals(path):
    prod, sums = [], []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            iv = (int(row["Start_Timestamp"]), int(row["End_Timestamp"]))
            if "block_sum_kernel" in name:
                sums.append(iv)
            elif "gemm_nt2_kernel" in name or "gemm_nt4_kernel" in name or ("gemm_nt_kernel" in name and "256" in name):
                prod.append(iv)
    return sorted(prod), sorted(sums)


def merged(ivs):
    out = []
    for a, b in ivs:
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def covered(ivs, cover):
    """ns of the intervals ivs that lie inside the (merged, sorted) intervals cover"""
    total, j = 0, 0
    for a, b in ivs:
        while j < len(cover) and cover[j][1] <= a:
            j += 1
        i = j
        while i < len(cover) and cover[i][0] < b:
            total += max(0, min(b, cover[i][1]) - max(a, cover[i][0]))
            i += 1
    return total


if __name__ == "__main__":
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    prod, sums = intervals(sys.argv[1])
    tp, ts = sum(b - a for a, b in prod), sum(b - a for a, b in sums)
    inside = covered(sums, merged(prod))
    print("product kernels: %d launches, %.1f ms per step" % (len(prod) // steps, tp / 1e6 / steps))
    print("block_sum_kernel: %d launches, %.1f ms per step, %.1f ms (%.1f %%) inside a product kernel's interval"
          % (len(sums) // steps, ts / 1e6 / steps, inside / 1e6 / steps, 100.0 * inside / max(ts, 1)))
