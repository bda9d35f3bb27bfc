"""Condense rocprofv3 csv output (-f csv) of scratch/wgrad3x3_bench.py run: the dispatches of the backward-weight main
kernels in launch order, cut into runs of `repetitions` (one run per call and switch position): per run the kernel, its
grid, the median / min duration of a kernel trace, or the per-launch mean of every counter of a counter collection.

    python scratch/wgrad3x3_summary.py DIR repetitions"""
import csv
import glob
import os
import re
import sys
from collections import defaultdict

d, reps = sys.argv[1], int(sys.argv[2])
pat = re.compile("conv_wgrad_mfma_kernel|wgrad3x3_kernel")


def short(n):
    n = re.sub(r"\(anonymous namespace\)::", "", n)
    n = re.sub(r"^void ", "", n)
    return n.split("(")[0][:48]


def runs(rows):
    rows.sort(key=lambda r: r[0])
    return [rows[i:i + reps] for i in range(0, len(rows), reps)]


for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
    rows = [(int(r["Start_Timestamp"]), short(r["Kernel_Name"]), r.get("Grid_Size_X", ""), r.get("Workgroup_Size_X", ""),
             (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
            for r in csv.DictReader(open(f)) if pat.search(r["Kernel_Name"])]
    for i, run in enumerate(runs(rows)):
        v = sorted(r[4] for r in run)
        print("TRACE run %2d %-44s grid %7s wg %s  n %d  median %.1f us  min %.1f" % (
            i, run[0][1], run[0][2], run[0][3], len(v), v[len(v) // 2], v[0]))
for f in sorted(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)):
    disp = defaultdict(dict)
    meta = {}
    for r in csv.DictReader(open(f)):
        if pat.search(r["Kernel_Name"]):
            k = int(r["Dispatch_Id"])
            disp[k][r["Counter_Name"]] = disp[k].get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
            meta[k] = (short(r["Kernel_Name"]), r.get("Grid_Size", ""), r.get("VGPR_Count", ""), r.get("Accum_VGPR_Count", ""),
                       r.get("LDS_Block_Size", ""), r.get("Scratch_Size", ""))
    for i, run in enumerate(runs([(k, v) for k, v in disp.items()])):
        print("PMC run %2d %-44s grid %s vgpr %s agpr %s lds %s scratch %s" % ((i,) + meta[run[0][0]]))
        for c in sorted(run[0][1]):
            print("      %-28s mean %.6g  (n %d)" % (c, sum(r[1].get(c, 0.0) for r in run) / len(run), len(run)))
