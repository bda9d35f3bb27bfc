"""The 3x3 fp32 backward-weight calls of the batch-32 step that run on conv_wgrad_mfma_kernel in MODE 2,
each alone, through sprk_conv2d_bwd_weight with random tensors.

    PYTHONPATH=. python scratch/wgrad3x3_bench.py list FILE.json
        one eager batch-32 step; every backward-weight call's geometry, the 16-byte alignment of its tensors and the
        record sprk_conv2d_last_variant(2) leaves behind it go to FILE.json (nothing is guessed)
    PYTHONPATH=. python scratch/wgrad3x3_bench.py run FILE.json [repetitions] [indices, comma separated]
        the MODE 2 3x3 calls of FILE.json (or those of the given indices into that list), `repetitions` times each, one
        geometry after the other: under rocprofv3 (--kernel-trace -f csv, or one --pmc set per run) the main kernel's
        dispatches come in that order, and scratch/wgrad3x3_summary.py cuts them into runs of `repetitions`.  With the
        WGRAD3X3 stage in the library the calls are made with it off, then on, and the results compared bit for bit."""
import ctypes
import json
import statistics
import sys

import torch

from spr_pick_amd import _lib, ops

GEOM = ("N", "C1", "C2", "Hin", "Win", "up1", "Cout", "Hout", "Wout", "KH", "KW", "stride", "dil", "pad_top", "pad_left", "dtype")


def last_record(L):
    out = (ctypes.c_int32 * 24)()
    L.sprk_conv2d_last_variant(2, out)
    return list(out)


def do_list(path):
    sys.path.insert(0, ".")
    from bench import make_cfg
    from spr_pick_amd import Denoiser, graph_step, synthetic
    L = _lib.lib()
    calls = []

    def wrap(name, igeom):
        real = getattr(L, name)

        def f(*a):
            rc = real(*a)
            g = a[igeom]._obj
            calls.append({"geom": [int(getattr(g, k)) for k in GEOM],
                          "aligned16": [(ctypes.cast(p, ctypes.c_void_p).value or 0) % 16 == 0 for p in a[:3]],
                          "record": last_record(L)})
            return rc
        setattr(L, name, f)

    wrap("sprk_conv2d_bwd_weight", 4)
    wrap("sprk_conv2d_bwd_weight_partial", 4)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    den = Denoiser(make_cfg(), device=dev, mode="joint")
    den.train()
    st = graph_step.GraphedTrainStep(den, 32, 64, 0.75, 0.01, graph=False)
    inp, tgt = synthetic.patch_batches(1, 32, [synthetic.micrograph(i) for i in range(2)], seed=100, device=dev)[0]
    st(inp, tgt, eager=True)
    torch.cuda.synchronize()
    calls.clear()
    st(inp, tgt, eager=True)
    torch.cuda.synchronize()
    json.dump({"geom_fields": GEOM, "calls": calls}, open(path, "w"), indent=0)
    for i, c in enumerate(calls):
        g, r = dict(zip(GEOM, c["geom"])), c["record"]
        print("%3d N%4d C%3d+%3d %3dx%-3d up%d -> %3d k%d s%d d%d pad %d,%d  stage %d IT %d NT %d WJ %d MODE %d chunks %d groups %d c2 %d tiles %d" % (
            i, g["N"], g["C1"], g["C2"], g["Hin"], g["Win"], g["up1"], g["Cout"], g["KH"], g["stride"], g["dil"], g["pad_top"],
            g["pad_left"], r[0], r[1], r[2], r[3], r[4], r[10], r[11], r[13], r[14]))


def do_run(path, reps, only):
    L, S, dev = _lib.lib(), torch.ops.sprk, torch.device("cuda:0")
    have = "sprk_wgrad3x3_enable" in _lib.EXPORTS
    calls = [c for c in json.load(open(path))["calls"]
             if c["record"][0] == 5 and c["record"][4] == 2 and c["geom"][9] == 3 and c["geom"][10] == 3]
    seen, uniq = set(), []
    for c in calls:
        if tuple(c["geom"]) not in seen:
            seen.add(tuple(c["geom"]))
            uniq.append(c)
    gen = torch.Generator().manual_seed(1)
    for i, c in enumerate(uniq):
        if only and i not in only:
            continue
        g = dict(zip(GEOM, c["geom"]))
        x = torch.randn(g["N"], g["C1"], g["Hin"], g["Win"], generator=gen).to(dev)
        x2 = torch.randn(g["N"], g["C2"], g["Hin"], g["Win"], generator=gen).to(dev) if g["C2"] else None
        gy = torch.randn(g["N"], g["Cout"], g["Hout"], g["Wout"], generator=gen).to(dev)
        gw = torch.empty(g["Cout"], g["C1"] + g["C2"], 3, 3, device=dev)
        geom = [g[k] for k in GEOM]
        res = {}
        for on in ((0, 1) if have else (None,)):
            if on is not None:
                L.sprk_wgrad3x3_enable(on)
            ts = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                S.conv2d_bwd_weight(x, x2, gy, geom, gw, False)
                b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            res[on] = gw.clone()
            r = last_record(L)
            print("CALL %d switch %s N %d C %d+%d %dx%d -> %d pad %d,%d  stage %d IT %d NT %d chunks %d groups %d tiles %d  "
                  "median %.1f us min %.1f (reduction included; %.1f TF)" % (
                      i, on, g["N"], g["C1"], g["C2"], g["Hin"], g["Win"], g["Cout"], g["pad_top"], g["pad_left"], r[0], r[1],
                      r[2], r[10], r[11], r[14], statistics.median(ts), min(ts),
                      18.0 * g["N"] * g["Hout"] * g["Wout"] * (g["C1"] + g["C2"]) * g["Cout"] / statistics.median(ts) * 1e-6),
                  flush=True)
        if have:
            print("    on == off: %s" % torch.equal(res[0].view(torch.int32), res[1].view(torch.int32)), flush=True)
        del x, x2, gy, gw, res
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if sys.argv[1] == "list":
        do_list(sys.argv[2])
    else:
        do_run(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5,
               [int(t) for t in sys.argv[4].split(",")] if len(sys.argv) > 4 else [])
