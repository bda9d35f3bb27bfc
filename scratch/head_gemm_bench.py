"""The three wide 1x1 head GEMMs of the fp32 batch-32 step, each alone: timed by events with the GEMM1X1 stage
off and on (sprk_gemm1x1_enable), results compared bit for bit.  Under rocprofv3 (--kernel-trace -f csv, one --pmc set per
run) scratch/kernel_csv_summary.py condenses the csv files: profiles/r06_gemm1x1_*_counters.txt.

    python scratch/head_gemm_bench.py [repetitions]"""
import ctypes
import statistics
import sys

import torch

from spr_pick_amd import _lib, ops

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
shapes = sys.argv[2] if len(sys.argv) > 2 else "main"
L = _lib.lib()
S = torch.ops.sprk
dev = torch.device("cuda:0")
have = "sprk_gemm1x1_enable" in _lib.EXPORTS   # (a parent build beside the tree has no switch: one pass)
g = torch.Generator().manual_seed(1)


def timed(fn):
    ts = []
    out = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return out, ts


def stage(which):
    out = (ctypes.c_int32 * 24)()
    L.sprk_conv2d_last_variant(which, out)
    return out[0]


CASES = {"main": [("fwd 384->384", 64, 384, 384, 64, False), ("fwd 384->96", 64, 384, 96, 64, False),
                  ("bwd 384->384", 64, 384, 384, 64, True)],
         # the sigma-net's and other head candidates
         "more": [("fwd 192->192", 64, 192, 192, 64, False), ("fwd 192->96", 64, 192, 96, 64, False),
                  ("bwd 192->192", 64, 192, 192, 64, True), ("fwd 384->384 N32", 32, 384, 384, 64, False)]}

for name, N, K, Cout, HW, bwd in CASES[shapes]:
    x = torch.randn(N, K, HW, HW, generator=g).to(dev)
    w = (torch.randn(Cout, K, 1, 1, generator=g) / K ** 0.5).to(dev)
    b = torch.randn(Cout, generator=g).to(dev)
    if bwd:
        xin = torch.empty(N, Cout, HW, HW, device=dev)
        wl = (torch.randn(K, Cout, 1, 1, generator=g) / K ** 0.5).to(dev)   # layer Cout(=K reduced) -> gin channels Cout
        geom = ops.make_geom(xin, None, wl, False, 1, 1, (0, 0, 0, 0))
        fn = lambda: S.conv2d_bwd_data(x, wl, ops.geom_list(geom), None, ops.ACT_NONE, None)
    else:
        geom = ops.make_geom(x, None, w, False, 1, 1, (0, 0, 0, 0))
        fn = lambda: ops.conv2d_forward(x, None, w, geom, bias=b, act=ops.ACT_LEAKY)
    res = {}
    for on in ((0, 1) if have else (None,)):
        if on is not None:
            L.sprk_gemm1x1_enable(on)
        fn()
        torch.cuda.synchronize()
        out, ts = timed(fn)
        res[on] = out
        print("%-18s switch %-4s stage %d  median %.1f us  min %.1f  max %.1f  (%.1f TF at median)" % (
            name, on, stage(1 if bwd else 0), statistics.median(ts), min(ts), max(ts),
            2.0 * N * HW * HW * K * Cout / statistics.median(ts) * 1e-6), flush=True)
    if have:
        print("    on == off: %s" % torch.equal(res[0], res[1]), flush=True)
    del x, w, res, out
    torch.cuda.empty_cache()
