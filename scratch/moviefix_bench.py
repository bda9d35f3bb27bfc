"""Device time of sprk_movie_correct per 4096^2 frame against its traffic bound, ny nx (sample + 4 + 4 + 1 + 4 [+ 8]) bytes
at 6.29 TB/s (gain, dark, fix map and out, and the sum read and written), and `joint align` with and without --gain --dark
--defects --hot_sigma on one 40-frame 4096^2 int16 movie (profiles/r14_moviefix_bench.txt).
A timed window is 40 calls through the C ABI on one stream between two HIP events, over four raw frames and four outputs in
turn (a movie's frames differ, its references do not); the figure is the window over 40.
usage: python scratch/moviefix_bench.py [OUT.json]"""
import ctypes, json, os, shutil, struct, sys, tempfile, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from spr_pick_amd import _lib, align, moviefix
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

N = 4096
rng = np.random.RandomState(0)
gain = torch.from_numpy(rng.uniform(0.5, 1.5, size=(N, N)).astype(np.float32)).cuda()
dark = torch.from_numpy(rng.uniform(0, 50, size=(N, N)).astype(np.float32)).cuda()
maps = {}
for name, frac in (("1e-4", 1e-4), ("1e-3", 1e-3), ("1e-2", 1e-2)):
    maps[name] = moviefix.build_fix(torch.from_numpy(rng.rand(N, N) < frac).cuda())
column = torch.zeros(N, N, dtype=torch.bool, device="cuda")
column[:, 1777] = True
maps["column"] = moviefix.build_fix(column)
maps["1e-3+column"] = moviefix.build_fix(column | (maps["1e-3"] > 0))
maps["none"] = torch.zeros(N, N, dtype=torch.uint8, device="cuda")
outs = [torch.empty(N, N, device="cuda") for _ in range(SETS)]
total = torch.zeros(N, N, device="cuda")
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

def run(raws, mode, fix, with_sum):
    def fn():
        for k in range(CALLS):
            rc = L.sprk_movie_correct(raws[k % SETS].data_ptr(), mode, N, N, gain.data_ptr(), dark.data_ptr(),
                                      None if fix is None else fix.data_ptr(), outs[k % SETS].data_ptr(),
                                      total.data_ptr() if with_sum else None, 1 if k == 0 else 0, stream)
            assert rc == 0, L.sprk_last_error()
    return fn

for mode, dtype, label in ((1, np.int16, "int16"), (0, np.int8, "int8"), (2, np.float32, "float32")):
    item = np.dtype(dtype).itemsize
    if dtype == np.float32:
        frames = [(rng.randn(N, N) * 100).astype(np.float32) for _ in range(SETS)]
    else:
        info = np.iinfo(dtype)
        frames = [rng.randint(max(info.min, -3000), min(info.max, 3000) + 1, size=(N, N)).astype(dtype) for _ in range(SETS)]
    raws = [torch.from_numpy(np.frombuffer(f.tobytes(), dtype=np.uint8).copy()).cuda() for f in frames]
    for name in (("1e-3", "none", "1e-4", "1e-2", "column", "1e-3+column") if mode == 1 else ("1e-3",)):
        for with_sum in (False, True):
            nbytes = N * N * (item + 4 + 4 + 1 + 4 + (8 if with_sum else 0))
            report("%s_fix_%s%s" % (label, name, "_sum" if with_sum else ""), window(run(raws, mode, maps[name], with_sum)), nbytes)
    if mode == 1:                                                 # the operator as moviefix.CorrectedMovie calls it
        def op():
            for k in range(CALLS):
                torch.ops.sprk.movie_correct(raws[k % SETS], 1, N, N, gain, dark, maps["1e-3"], outs[k % SETS], None, True)
        report("int16_fix_1e-3_operator", window(op), N * N * (item + 13))
    del raws, frames
del outs, total, maps

# joint align on one movie of 40 frames, with and without the correction
tmp = tempfile.mkdtemp()
try:
    os.makedirs(os.path.join(tmp, "movies"))
    path = os.path.join(tmp, "movies", "mov.mrc")
    write_raw_mrc(path, np.zeros((2, 2, 2), dtype=np.int16))     # a header to re-pack: nx, ny, nz
    img = rng.randint(500, 1500, size=(N, N)).astype(np.int16)
    hot = rng.rand(N, N) < 1e-4
    with open(path, "r+b") as f:
        f.write(struct.pack("<3i", N, N, 40))
        f.seek(1024)
        for k in range(40):
            frame = np.roll(img, (k // 4, -(k // 5)), axis=(0, 1))
            frame[hot] = 30000
            f.write(frame.tobytes())
        f.truncate()
    g = gain.cpu().numpy()
    g[:, 1777] = 0.0
    write_raw_mrc(os.path.join(tmp, "gain.mrc"), g)
    write_raw_mrc(os.path.join(tmp, "dark.mrc"), dark.cpu().numpy())
    open(os.path.join(tmp, "defects.txt"), "w").write("100 200 6 4\n3000 12 2 40\n")
    flags = {"gain": os.path.join(tmp, "gain.mrc"), "dark": os.path.join(tmp, "dark.mrc"),
             "defects": os.path.join(tmp, "defects.txt"), "hot_sigma": 6.0}
    del gain, dark
    for kw in ({}, flags, {}, flags):
        out = os.path.join(tmp, "out")
        torch.cuda.synchronize()
        t = time.time()
        r = align.align_dataset(os.path.join(tmp, "movies"), out, **kw)
        dt = time.time() - t
        shutil.rmtree(out)
        key = "joint_align_40x4096_%s_s" % ("corrected" if kw else "plain")
        res.setdefault(key, []).append(dt)
        print("%s: %.2f s %s" % (key, dt, r["mov"].get("defects", "")), flush=True)
        if len(sys.argv) > 1:
            json.dump(res, open(sys.argv[1], "w"), indent=1)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
