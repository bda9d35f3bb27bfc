"""Condense rocprofv3 csv output (-f csv) for the Winograd backward-weight kernels (wino_wgrad_kernel,
wino_wgrad_stream_kernel).

    python scratch/wino_wgrad_summary.py calls DIR repetitions
        output of scratch/wino_wgrad_bench.py: the dispatches in launch order, cut into one block per call and switch
        position (a call launches one or two kernels, `repetitions` times each): per block and kernel the median / min
        duration of a kernel trace, or the per-launch mean of every counter of a counter collection
    python scratch/wino_wgrad_summary.py step DIR [steps to use, default 8]
        a kernel trace of bench.py: the launches per position in the step (the step's sequence of them is the period of the
        trace's tail, so position p of a parent's trace is position p of this tree's), and the medians of five kernels the
        change does not touch (the drift)"""
import csv
import glob
import os
import re
import sys
from collections import defaultdict

mode, d, n = sys.argv[1], sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 8
pat = re.compile("wino_wgrad_kernel|wino_wgrad_stream_kernel")
DRIFT = ("gemm1x1_kernel<2", "wgrad1x1_kernel", "wino_conv_kernel<6, 0, 1", "unrot_act_bwd64_kernel", "wgrad3x3_kernel<")


def short(name):
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"^void ", "", name)
    return name.split("(")[0][:48]


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def blocks(rows, reps):
    """rows (order, key, value) -> [{key: [values]}]: a block ends where a kernel has had its `reps` launches"""
    out, cur = [], {}
    for _, key, val in sorted(rows, key=lambda r: r[0]):
        if cur and all(len(v) == reps for v in cur.values()):
            out.append(cur)
            cur = {}
        cur.setdefault(key, []).append(val)
    return out + ([cur] if cur else [])


def grid(r):
    return "%s x %s" % (r.get("Grid_Size_X", r.get("Grid_Size", "")), r.get("Grid_Size_Y", ""))


traces = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
if mode == "calls":
    for f in traces:
        rows = [(int(r["Start_Timestamp"]), (short(r["Kernel_Name"]), grid(r)),
                 (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in csv.DictReader(open(f)) if pat.search(r["Kernel_Name"])]
        for i, b in enumerate(blocks(rows, n)):
            for (name, g), v in b.items():
                print("TRACE block %2d %-34s grid %-12s n %d  median %.1f us  min %.1f" % (i, name, g, len(v), med(v), min(v)))
    for f in sorted(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)):
        disp, meta = defaultdict(dict), {}
        for r in csv.DictReader(open(f)):
            if pat.search(r["Kernel_Name"]):
                k = int(r["Dispatch_Id"])
                disp[k][r["Counter_Name"]] = disp[k].get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
                meta[k] = (short(r["Kernel_Name"]), r.get("Grid_Size", ""), r.get("VGPR_Count", ""), r.get("Scratch_Size", ""))
        for i, b in enumerate(blocks([(k, meta[k], v) for k, v in disp.items()], n)):
            for (name, g, vg, sc), v in b.items():
                print("PMC block %2d %-34s grid %s vgpr %s scratch %s" % (i, name, g, vg, sc))
                for c in sorted(v[0]):
                    print("      %-28s mean %.6g  (n %d)" % (c, sum(x.get(c, 0.0) for x in v) / len(v), len(v)))
else:
    for f in traces:
        rows = sorted((int(r["Start_Timestamp"]), short(r["Kernel_Name"]), grid(r),
                       (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in csv.DictReader(open(f)))
        main = [r for r in rows if pat.search(r[1])]
        gs = [r[2] for r in main]   # kernel names differ between the two trees, grids do not
        period = next(m for m in range(1, len(gs) // 3) if gs[-m:] == gs[-2 * m:-m] == gs[-3 * m:-2 * m] and len(set(gs[-m:])) > 1)
        use = min(n, len(gs) // period - 1)
        tail = main[-use * period:]
        print("%s: %d launches, period %d, %d steps used" % (os.path.basename(f), len(main), period, use))
        for p in range(period):
            v = [tail[s * period + p][3] for s in range(use)]
            print("POS %2d %-34s grid %-12s median %.1f us  min %.1f" % (p, tail[p][1], tail[p][2], med(v), min(v)))
        print("SUM of the medians %.1f us" % sum(med([tail[s * period + p][3] for s in range(use)]) for p in range(period)))
        for name in DRIFT:
            by = defaultdict(list)
            for r in rows:
                if name in r[1]:
                    by[r[2]].append(r[3])
            for g, v in sorted(by.items(), key=lambda kv: -med(kv[1]))[:1]:
                print("DRIFT %-34s grid %-12s n %d  median %.1f us" % (name, g, len(v), med(v)))
