"""Launches per kernel and grid size, from a rocprofv3 kernel trace:
    python tools/kernel_grid_counts.py OUT_kernel_trace.csv > grids.csv

Reads the trace that `rocprofv3 --kernel-trace --output-format csv` writes and prints one CSV row per (kernel, workgroup size, workgroups) with
the number of launches.  The kernel name is the demangled name without its return type and parameter list (`void (anonymous namespace)::k<1>(...)`
-> `(anonymous namespace)::k<1>`).  profiles/launch_geometry_knob_grids.csv was made this way (profiles/README.md)."""
import collections
import csv
import sys


def kernel_name(demangled):
    """strip `void ` and the trailing parameter list (the parenthesis that closes the name, matched from the end)"""
    s = demangled.strip()
    if s.startswith("void "):
        s = s[5:]
    if s.endswith(")"):
        depth = 0
        for i in range(len(s) - 1, -1, -1):
            depth += {")": 1, "(": -1}.get(s[i], 0)
            if depth == 0:
                return s[:i]
    return s


def main(path, out=sys.stdout):
    counts = collections.Counter()
    for r in csv.DictReader(open(path)):
        wg = int(r["Workgroup_Size_X"]) * int(r["Workgroup_Size_Y"]) * int(r["Workgroup_Size_Z"])
        grid = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
        counts[(kernel_name(r["Kernel_Name"]), wg, grid // wg)] += 1
    w = csv.writer(out, lineterminator="\n")
    w.writerow(["kernel", "workgroup_size", "workgroups", "launches"])
    for (k, wg, n), c in sorted(counts.items()):
        w.writerow([k, wg, n, c])


if __name__ == "__main__":
    main(sys.argv[1])
