"""Device time of sprk_align_spectrum per frame (4096^2 int16 -> 4096^2 and -> 2048^2) against its MFMA bound
(2 ny nx 2Hs + 2 2Ku 2ny Hs FLOP / 157.3 TF) with sprk_align_accumulate beside it, of sprk_align_synthesize once per movie,
of the per-frame filter g built with torch, and `joint align` with and without --dose on one 40-frame 4096^2 int16 movie
(profiles/r13_dose_bench.txt).
usage: python scratch/dose_bench.py [OUT.json]"""
import json, os, shutil, struct, sys, tempfile, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from spr_pick_amd import align, dose
from extract_model import write_raw_mrc

PEAK = 157.3e12
res = {}

def timed(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(out)), "min_ms": float(min(out)), "max_ms": float(max(out)), "runs": out}

def report(key, t, flop=None):
    if flop is not None:
        t["bound_ms"] = flop / PEAK * 1e3
        t["x_bound"] = t["median_ms"] / t["bound_ms"]
        print("%s: median %.3f ms (%.3f .. %.3f), bound %.3f ms, %.2f x" % (key, t["median_ms"], t["min_ms"], t["max_ms"],
                                                                           t["bound_ms"], t["x_bound"]), flush=True)
    else:
        print("%s: median %.3f ms (%.3f .. %.3f)" % (key, t["median_ms"], t["min_ms"], t["max_ms"]), flush=True)
    res[key] = t
    if len(sys.argv) > 1:
        json.dump(res, open(sys.argv[1], "w"), indent=1)

N = 4096
rng = np.random.RandomState(0)
img = rng.randint(-3000, 3000, size=(N, N)).astype(np.int16)
raw = torch.from_numpy(np.frombuffer(img.tobytes(), dtype=np.uint8).copy()).cuda()
for B in (4096, 2048):
    t0 = time.time()
    W1, W2, W3, W4 = dose.spectrum_matrices(N, N, B, B, "cuda")
    torch.cuda.synchronize()
    print("spectrum_matrices(4096, 4096, %d, %d): %.2f s, once per geometry" % (B, B, time.time() - t0), flush=True)
    filters = dose.FrameFilters(N, N, B, B, 40, "cuda", apix=1.0, dose=1.5)
    Ku, Hs = filters.Ku, filters.Hs
    g = filters.g(3, 1.37, -2.6)
    F = torch.zeros_like(g)
    report("spectrum_4096_%d" % B, timed(lambda: torch.ops.sprk.align_spectrum(raw, 1, N, N, W1, W2, g, 0.0, F, False)),
           2.0 * N * N * 2 * Hs + 2.0 * 2 * Ku * 2 * N * Hs)
    my, mx = align.shift_matrix(N, B, 1.37, "cuda"), align.shift_matrix(N, B, -2.6, "cuda")
    y = torch.zeros(B, B, device="cuda")
    report("accumulate_4096_%d" % B, timed(lambda: torch.ops.sprk.align_accumulate(raw, 1, N, N, B, B, my, mx, 0.0, y, False)),
           2.0 * N * N * B + 2.0 * B * N * B)
    F.normal_()
    report("synthesize_%d" % B, timed(lambda: torch.ops.sprk.align_synthesize(F, B, B, W3, W4)),
           2.0 * 2 * B * 2 * Ku * Hs + 2.0 * B * 2 * Hs * B)
    report("filter_g_4096_%d" % B, timed(lambda: filters.g(3, 1.37, -2.6)))
    del W1, W2, W3, W4, my, mx, y, F, g, filters
    dose._matrices.clear()
del raw

# joint align on one movie of 40 frames, with and without --dose
tmp = tempfile.mkdtemp()
try:
    os.makedirs(os.path.join(tmp, "movies"))
    path = os.path.join(tmp, "movies", "mov.mrc")
    write_raw_mrc(path, np.zeros((2, 2, 2), dtype=np.int16))     # a header to re-pack: nx, ny, nz
    with open(path, "r+b") as f:
        f.write(struct.pack("<3i", N, N, 40))
        f.seek(1024)
        for k in range(40):
            f.write(np.roll(img, (3 * k, -2 * k), axis=(0, 1)).tobytes())
        f.truncate()
    for kw in ({}, {"dose": 1.5, "apix": 1.0}, {}, {"dose": 1.5, "apix": 1.0}):
        out = os.path.join(tmp, "out")
        torch.cuda.synchronize()
        t = time.time()
        align.align_dataset(os.path.join(tmp, "movies"), out, **kw)
        dt = time.time() - t
        shutil.rmtree(out)
        key = "joint_align_40x4096_%s_s" % ("dose" if kw else "plain")
        res.setdefault(key, []).append(dt)
        print("%s: %.2f s" % (key, dt), flush=True)
        if len(sys.argv) > 1:
            json.dump(res, open(sys.argv[1], "w"), indent=1)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
