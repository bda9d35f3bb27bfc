"""Device time of sprk_align_corr (40 frames of 1024^2, R = 16) and of sprk_align_accumulate per frame (4096^2 int16 ->
4096^2 and -> 2048^2), each against its MFMA bound (FLOP / 157.3 TF), beside sprk_ingest_resample at the same sizes, and
`joint align` on one 40-frame 4096^2 int16 movie (profiles/r12_align_bench.txt).
usage: python scratch/align_bench.py [OUT.json]"""
import json, os, shutil, struct, sys, tempfile, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from spr_pick_amd import align, ingest
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

def report(key, t, flop):
    t["bound_ms"] = flop / PEAK * 1e3
    t["x_bound"] = t["median_ms"] / t["bound_ms"]
    res[key] = t
    print("%s: median %.3f ms, bound %.3f ms, %.2f x" % (key, t["median_ms"], t["bound_ms"], t["x_bound"]), flush=True)
    if len(sys.argv) > 1:
        json.dump(res, open(sys.argv[1], "w"), indent=1)

# align_corr: Z = 40, 1024^2, R = 16; the bound counts the 63 x 63 window the kernel's largest tile would hold
Z, S, R = 40, 1024, 16
a = torch.randn(Z, S, S, device="cuda")
r = torch.randn(Z, S, S, device="cuda")
for tile in (0, 16, 32, 64):
    report("corr_Z40_1024_R16_tile%d" % tile, timed(lambda: torch.ops.sprk.align_corr(a, r, R, tile), reps=5, warm=1),
           2.0 * 63 * 63 * S * S * Z)
del a, r

# align_accumulate per frame, with ingest_resample beside it
rng = np.random.RandomState(0)
img = rng.randint(-3000, 3000, size=(4096, 4096)).astype(np.int16)
raw = torch.from_numpy(np.frombuffer(img.tobytes(), dtype=np.uint8).copy()).cuda()
for B in (4096, 2048):
    my, mx = align.shift_matrix(4096, B, 1.37, "cuda"), align.shift_matrix(4096, B, -2.6, "cuda")
    y = torch.zeros(B, B, device="cuda")
    flop = 2.0 * 4096 * 4096 * B + 2.0 * B * 4096 * B
    report("accumulate_4096_%d" % B, timed(lambda: torch.ops.sprk.align_accumulate(raw, 1, 4096, 4096, B, B, my, mx, 0.0, y, False)),
           flop)
    report("resample_4096_%d" % B, timed(lambda: torch.ops.sprk.ingest_resample(raw, 1, 4096, 4096, B, B, my, mx)), flop)
    res["shift_matrix_4096_%d" % B] = timed(lambda: align.shift_matrix(4096, B, 1.37, "cuda"))      # torch, float64: no bound
    print("shift_matrix_4096_%d: median %.3f ms" % (B, res["shift_matrix_4096_%d" % B]["median_ms"]), flush=True)
del raw, my, mx, y

# joint align on one movie of 40 frames
tmp = tempfile.mkdtemp()
try:
    os.makedirs(os.path.join(tmp, "movies"))
    path = os.path.join(tmp, "movies", "mov.mrc")
    write_raw_mrc(path, np.zeros((2, 2, 2), dtype=np.int16))     # a header to re-pack: nx, ny, nz
    with open(path, "r+b") as f:
        f.write(struct.pack("<3i", 4096, 4096, 40))
        f.seek(1024)
        for k in range(40):
            f.write(np.roll(img, (3 * k, -2 * k), axis=(0, 1)).tobytes())
        f.truncate()
    for ftbin in (1, 2, 1, 2):
        out = os.path.join(tmp, "out")
        torch.cuda.synchronize()
        t = time.time()
        got = align.align_dataset(os.path.join(tmp, "movies"), out, ftbin=ftbin)
        dt = time.time() - t
        shutil.rmtree(out)
        res.setdefault("joint_align_40x4096_ftbin%d_s" % ftbin, []).append(dt)
        res["joint_align_iterations"] = got["mov"]["iterations"]
        print("joint align, 40 frames of 4096^2, ftbin %d: %.2f s, %d iteration(s)" % (ftbin, dt, got["mov"]["iterations"]),
              flush=True)
        if len(sys.argv) > 1:
            json.dump(res, open(sys.argv[1], "w"), indent=1)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
