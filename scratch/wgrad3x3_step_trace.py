"""Condense a rocprofv3 kernel trace (-f csv) of bench.py: the launches of the backward-weight main kernels
(conv_wgrad_mfma_kernel, wgrad1x1_kernel, wgrad3x3_kernel) per position in the step -- the step's sequence of them is found
as the period of the trace's tail, so launches of one kernel and grid but different layers stay apart, and position p of a
parent's trace is position p of this tree's -- and the medians of five kernels no change here touches (the drift).

    python scratch/wgrad3x3_step_trace.py DIR [steps to use, default 8]"""
import csv
import glob
import os
import re
import sys

d, steps = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 8
pat = re.compile("conv_wgrad_mfma_kernel|wgrad1x1_kernel|wgrad3x3_kernel")
DRIFT = (("gemm1x1_kernel<2", None), ("wgrad1x1_kernel", None), ("wino_conv_kernel<6, 0, 1", None),
         ("unrot_act_bwd64_kernel", None), ("wino_wgrad_kernel<3", "131072"))


def short(n):
    n = re.sub(r"\(anonymous namespace\)::", "", n)
    n = re.sub(r"^void ", "", n)
    return n.split("(")[0][:48]


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
    rows = sorted((int(r["Start_Timestamp"]), short(r["Kernel_Name"]), r.get("Grid_Size_X", ""),
                   (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in csv.DictReader(open(f)))
    main = [r for r in rows if pat.search(r[1])]
    # kernel names differ between the two trees, grids do not: the period is looked for in the grids
    gs = [r[2] for r in main]
    period = next(m for m in range(1, len(gs) // 3) if gs[-m:] == gs[-2 * m:-m] == gs[-3 * m:-2 * m] and len(set(gs[-m:])) > 1)
    use = min(steps, len(gs) // period - 1)
    tail = main[-use * period:]
    print("%s: %d launches, period %d, %d steps used" % (os.path.basename(f), len(main), period, use))
    for p in range(period):
        v = [tail[s * period + p][3] for s in range(use)]
        print("POS %2d %-44s grid %7s  median %.1f us  min %.1f" % (p, tail[p][1], tail[p][2], med(v), min(v)))
    for name, grid in DRIFT:
        v = [r[3] for r in rows if name in r[1] and (grid is None or r[2] == grid)]
        if v:
            print("DRIFT %-44s grid %7s  n %d  median %.1f us" % (name, grid or "any", len(v), med(v)))
