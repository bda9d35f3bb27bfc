"""Device time of sprk_align_warp per frame at 4096^2 and 1024^2 against its traffic bound, 12 ny nx bytes at 6.29 TB/s (src
read, y read and written; `first` calls read no y: 8 ny nx), and `joint align` with and without --patch 5,5 on one 40-frame
4096^2 int16 movie, in one process (profiles/r15_localmotion_bench.txt).
A timed window is 40 calls through the C ABI on one stream between two HIP events, over four source frames in turn (a
movie's frames differ) into one running sum; the figure is the window over 40.
usage: python scratch/localmotion_bench.py [OUT.json]"""
import ctypes, json, os, shutil, struct, sys, tempfile, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from spr_pick_amd import _lib, align
from extract_model import write_raw_mrc

BW = 6.29e12
CALLS, SETS = 40, 4
res = {}
L = _lib.lib()

def window(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        out.append(a.elapsed_time(b) / CALLS)
    return {"median_ms": float(np.median(out)), "min_ms": float(min(out)), "max_ms": float(max(out)), "runs": out}

def report(key, t, nbytes):
    t["bytes"] = nbytes
    t["bound_ms"] = nbytes / BW * 1e3
    t["x_bound"] = t["median_ms"] / t["bound_ms"]
    t["TB_per_s"] = nbytes / (t["median_ms"] * 1e-3) / 1e12
    print("%s: median %.4f ms (%.4f .. %.4f), bound %.4f ms, %.2f x, %.2f TB/s" % (
        key, t["median_ms"], t["min_ms"], t["max_ms"], t["bound_ms"], t["x_bound"], t["TB_per_s"]), flush=True)
    res[key] = t
    if len(sys.argv) > 1:
        json.dump(res, open(sys.argv[1], "w"), indent=1)

rng = np.random.RandomState(0)
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
six = ctypes.c_float * 6
# no field; the field of a movie (a few pixels, smooth); one that reaches the clamp in the corners
fields = {"zero": (six(), six()), "smooth": (six(0.3, 1.5, -2.0, 3.0, -2.5, 4.0), six(-0.2, -2.5, 1.0, -4.0, 3.0, 2.0)),
          "clamped": (six(0.3, 25.0, 18.0, 6.0, -9.0, 4.0), six(-0.7, -30.0, 22.0, -5.0, 8.0, 3.0))}
for N in (4096, 1024):
    srcs = [torch.from_numpy((rng.randn(N, N) * 100).astype(np.float32)).cuda() for _ in range(SETS)]
    total = torch.zeros(N, N, device="cuda")
    for name, (cy, cx) in fields.items():
        for first in (False, True):
            def fn():
                for k in range(CALLS):
                    rc = L.sprk_align_warp(srcs[k % SETS].data_ptr(), N, N, cy, cx, total.data_ptr(), 1 if first or k == 0 else 0,
                                           stream)
                    assert rc == 0, L.sprk_last_error()
            report("warp_%d_%s_%s" % (N, name, "first" if first else "add"), window(fn), N * N * (8 if first else 12))
    def op():                                                     # the operator as localmotion.LocalMovie calls it
        for k in range(CALLS):
            torch.ops.sprk.align_warp(srcs[k % SETS], list(fields["smooth"][0]), list(fields["smooth"][1]), total, True)
    report("warp_%d_smooth_first_operator" % N, window(op), N * N * 8)
    del srcs, total

# joint align on one movie of 40 frames, with and without the local field
N = 4096
tmp = tempfile.mkdtemp()
try:
    os.makedirs(os.path.join(tmp, "movies"))
    path = os.path.join(tmp, "movies", "mov.mrc")
    write_raw_mrc(path, np.zeros((2, 2, 2), dtype=np.int16))     # a header to re-pack: nx, ny, nz
    img = rng.randint(500, 1500, size=(N, N)).astype(np.int16)
    with open(path, "r+b") as f:
        f.write(struct.pack("<3i", N, N, 40))
        f.seek(1024)
        for k in range(40):
            f.write(np.roll(img, (k // 4, -(k // 5)), axis=(0, 1)).tobytes())
        f.truncate()
    for kw in ({}, {"patch": (5, 5)}, {}, {"patch": (5, 5)}):
        out = os.path.join(tmp, "out")
        torch.cuda.synchronize()
        t = time.time()
        r = align.align_dataset(os.path.join(tmp, "movies"), out, **kw)
        torch.cuda.synchronize()
        dt = time.time() - t
        shutil.rmtree(out)
        key = "joint_align_40x4096_%s_s" % ("patch_5x5" if kw else "plain")
        res.setdefault(key, []).append(dt)
        local = r["mov"].get("local")
        print("%s: %.2f s %s" % (key, dt, "" if local is None else "(%d local iterations, %d dropped, largest |q| %.3f)" % (
            local["iterations"], local["dropped"], max(np.abs(local["qx"]).max(), np.abs(local["qy"]).max()))), flush=True)
        if len(sys.argv) > 1:
            json.dump(res, open(sys.argv[1], "w"), indent=1)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
