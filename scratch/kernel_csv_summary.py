"""Condense rocprofv3 csv output (-f csv) under a directory: per kernel (short name + grid) the median / min / mean
duration of every *kernel_trace.csv and the per-launch mean of every counter of every *counter_collection.csv.

    python scratch/kernel_csv_summary.py DIR [regex of kernel names]"""
import csv
import glob
import os
import re
import sys
from collections import defaultdict

d, want = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "conv_mfma_kernel<4, 6|gemm1x1|mask1x1")
pat = re.compile(want)


def short(n):
    n = re.sub(r"\(anonymous namespace\)::", "", n)
    n = re.sub(r"^void ", "", n)
    return n.split("(")[0][:60]


for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
    agg = defaultdict(list)
    for r in csv.DictReader(open(f)):
        k = short(r["Kernel_Name"])
        if pat.search(k):
            agg[(k, r.get("Grid_Size_X", ""), r.get("Grid_Size_Y", ""))].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for k, v in sorted(agg.items()):
        v2 = sorted(v)
        print("TRACE %-50s grid %s,%s  n %d  median %.1f us  min %.1f  mean %.1f" % (k[0], k[1], k[2], len(v), v2[len(v2) // 2], v2[0], sum(v) / len(v)))
for f in sorted(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)):
    agg = defaultdict(lambda: defaultdict(list))
    for r in csv.DictReader(open(f)):
        k = short(r["Kernel_Name"])
        if pat.search(k):
            agg[(k, r.get("Grid_Size", ""), r.get("VGPR_Count", ""), r.get("Accum_VGPR_Count", ""), r.get("LDS_Block_Size", ""), r.get("Scratch_Size", ""))][r["Counter_Name"]].append(float(r["Counter_Value"]))
    for k, cs in sorted(agg.items()):
        print("PMC %-50s grid %s vgpr %s agpr %s lds %s scratch %s" % k)
        for c, v in sorted(cs.items()):
            print("      %-28s mean %.6g  (n %d)" % (c, sum(v) / len(v), len(v)))
