"""The two wide 1x1 backward-weight calls of the fp32 batch-32 step, each alone: timed by events with the
WGRAD1X1 stage off and on (sprk_wgrad1x1_enable), results compared bit for bit.  Under rocprofv3 (--kernel-trace -f csv,
or one --pmc set per run) scratch/kernel_csv_summary.py condenses the csv files: profiles/r07_wgrad1x1_*_counters.txt.

    PYTHONPATH=. python scratch/wgrad1x1_bench.py [repetitions] [384 | 96: that call only]"""
import ctypes
import statistics
import sys

import torch

from spr_pick_amd import _lib, ops

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
only = int(sys.argv[2]) if len(sys.argv) > 2 else 0
L = _lib.lib()
S = torch.ops.sprk
dev = torch.device("cuda:0")
have = "sprk_wgrad1x1_enable" in _lib.EXPORTS   # (a parent build beside the tree has no switch: one pass)
g = torch.Generator().manual_seed(1)


def timed(fn):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return ts


def record():
    out = (ctypes.c_int32 * 24)()
    L.sprk_conv2d_last_variant(2, out)
    return out[0], out[14]


for name, N, K, Cout, HW in (("wgrad 384->384", 64, 384, 384, 64), ("wgrad 384->96", 64, 384, 96, 64)):
    if only and Cout != only:
        continue
    x = torch.randn(N, K, HW, HW, generator=g).to(dev)
    gy = torch.randn(N, Cout, HW, HW, generator=g).to(dev)
    gw = torch.empty(Cout, K, 1, 1, device=dev)
    geom = ops.geom_list(ops.make_geom(x, None, gw, False, 1, 1, (0, 0, 0, 0)))
    fn = lambda: S.conv2d_bwd_weight(x, None, gy, geom, gw, False)   # the main kernel and the reduction of its slabs
    res = {}
    for on in ((0, 1) if have else (None,)):
        if on is not None:
            L.sprk_wgrad1x1_enable(on)
        fn()
        torch.cuda.synchronize()
        ts = timed(fn)
        res[on] = gw.clone()
        stage, tiles = record()
        print("%-16s switch %-4s stage %d tiles/group %d  median %.1f us  min %.1f  max %.1f  (%.1f TF at median, reduction included)" % (
            name, on, stage, tiles, statistics.median(ts), min(ts), max(ts),
            2.0 * N * HW * HW * K * Cout / statistics.median(ts) * 1e-6), flush=True)
    if have:
        print("    on == off: %s" % torch.equal(res[0].view(torch.int32), res[1].view(torch.int32)), flush=True)
    del x, gy, gw, res
    torch.cuda.empty_cache()
