"""The backward-weight calls of the batch-32 step that take the Winograd stage, each alone, through
sprk_conv2d_bwd_weight with random tensors.

    PYTHONPATH=. python scratch/wino_wgrad_bench.py FILE.json [repetitions] [switch positions, default 0,1]
        the calls of FILE.json (scratch/wgrad3x3_bench.py list; profiles/r08_wgrad3x3_calls.json) whose record says stage 3,
        `repetitions` times each, one geometry after the other, with sprk_wino_wgrad_stream_enable at each of the given
        positions in turn (a library without the switch: once): under rocprofv3 (--kernel-trace, or one --pmc set per run)
        the dispatches of wino_wgrad_kernel / wino_wgrad_stream_kernel come in that order.  Event times include the
        reduction; the results of the positions are compared bit for bit."""
import json
import statistics
import sys

import torch

from spr_pick_amd import _lib

GEOM = ("N", "C1", "C2", "Hin", "Win", "up1", "Cout", "Hout", "Wout", "KH", "KW", "stride", "dil", "pad_top", "pad_left", "dtype")


def main(path, reps, positions):
    L, S, dev = _lib.lib(), torch.ops.sprk, torch.device("cuda:0")
    have = "sprk_wino_wgrad_stream_enable" in _lib.EXPORTS
    seen, uniq = set(), []
    for c in json.load(open(path))["calls"]:
        if c["record"][0] == 3 and tuple(c["geom"]) not in seen:
            seen.add(tuple(c["geom"]))
            uniq.append(c)
    gen = torch.Generator(device=dev).manual_seed(1)
    for i, c in enumerate(uniq):
        g = dict(zip(GEOM, c["geom"]))
        x = torch.randn(g["N"], g["C1"], g["Hin"], g["Win"], generator=gen, device=dev)
        x2 = torch.randn(g["N"], g["C2"], g["Hin"], g["Win"], generator=gen, device=dev) if g["C2"] else None
        gy = torch.randn(g["N"], g["Cout"], g["Hout"], g["Wout"], generator=gen, device=dev)
        gw = torch.empty(g["Cout"], g["C1"] + g["C2"], 3, 3, device=dev)
        geom = [g[k] for k in GEOM]
        res = []
        for on in (positions if have else (None,)):
            if on is not None:
                L.sprk_wino_wgrad_stream_enable(on)
            ts = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                S.conv2d_bwd_weight(x, x2, gy, geom, gw, False)
                b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            res.append(gw.clone())
            print("CALL %d switch %s N %d C %d+%d %dx%d -> %d pad %d,%d  median %.1f us min %.1f (reduction included; %.1f TF)" % (
                i, on, g["N"], g["C1"], g["C2"], g["Hin"], g["Win"], g["Cout"], g["pad_top"], g["pad_left"],
                statistics.median(ts), min(ts),
                18.0 * g["N"] * g["Hout"] * g["Wout"] * (g["C1"] + g["C2"]) * g["Cout"] / statistics.median(ts) * 1e-6), flush=True)
        if len(res) > 1:
            print("    equal bits: %s" % all(torch.equal(res[0].view(torch.int32), r.view(torch.int32)) for r in res[1:]), flush=True)
        del x, x2, gy, gw, res
        torch.cuda.empty_cache()
    if have:
        L.sprk_wino_wgrad_stream_enable(1)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 5,
         [int(t) for t in sys.argv[3].split(",")] if len(sys.argv) > 3 else [0, 1])
