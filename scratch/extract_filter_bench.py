"""Device time of sprk_extract_filter for 1000 boxes of 256^2 from a 4096^2 int16 micrograph, beside sprk_extract_scale, and
extract_dataset on 16 such micrographs with and without --ctf_correct (profiles/r10_extract_filter_bench.txt).
usage: python scratch/extract_filter_bench.py [OUT.json]"""
import json, os, shutil, sys, tempfile, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from spr_pick_amd import ctf, extract
from extract_model import write_raw_mrc
import types

res = {}
rng = np.random.RandomState(0)
img = rng.randint(-3000, 3000, size=(4096, 4096)).astype(np.int16)
raw = torch.from_numpy(np.frombuffer(img.tobytes(), dtype=np.uint8).copy()).cuda()
header = types.SimpleNamespace(mode=1, ny=4096, nx=4096)
xy_np = rng.randint(128, 4096 - 128 + 1, size=(1000, 2)).astype(np.int32)
xy = torch.from_numpy(xy_np).cuda()

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

for S in (256, 64):
    phi = torch.from_numpy(ctf.correction_filter(256, S, 1.0, 15000.0, 14000.0, 30.0, 300.0, 2.7, 0.07, "flip")).cuda()
    for normalize in (True, False):
        res["filter_256_%d_%s" % (S, "norm" if normalize else "nonorm")] = timed(
            lambda: extract.extract_particles((raw, header), xy, 256, normalize=normalize, scale=S, ctf_filter=phi))
    res["scale_256_%d_norm" % S] = timed(lambda: extract.extract_particles((raw, header), xy, 256, scale=S))
print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "runs"} for k, v in res.items()}, indent=1), flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)

# extract_dataset on 16 micrographs
tmp = tempfile.mkdtemp()
try:
    lines, star = ["image_name\tpath"], [ctf.CTF_STAR_HEADER]
    os.makedirs(os.path.join(tmp, "picks"))
    for m in range(16):
        name = "mic%02d" % m
        path = os.path.join(tmp, name + ".mrc")
        write_raw_mrc(path, np.roll(img, 37 * m, axis=1))
        lines.append("%s\t%s" % (name, path))
        star.append(ctf.star_row(name + ".mrc", 15000.0 + 100 * m, 0.5, 1.0, 300.0, 2.7, 0.07, 14000.0, 30.0))
        open(os.path.join(tmp, "picks", name + "_scores_unbinned.txt"), "w").write(
            "image_name\tx_coord\ty_coord\tscore\n" + "".join("%s\t%d\t%d\t0.9\n" % (name, x, y) for x, y in xy_np))
    open(os.path.join(tmp, "raw.txt"), "w").write("\n".join(lines) + "\n")
    open(os.path.join(tmp, "ctf.star"), "w").write("".join(star))
    for S in (64, 256):
        for flag in (None, "flip", None, "flip"):
            out = os.path.join(tmp, "out")
            t = time.time()
            counts = extract.extract_dataset(os.path.join(tmp, "raw.txt"), os.path.join(tmp, "picks"), out, 256,
                                             scale=None if (S == 256 and flag is None) else S, ctf=os.path.join(tmp, "ctf.star"),
                                             ctf_correct=flag)
            dt = time.time() - t
            assert sum(c["written"] for c in counts.values()) == 16000
            shutil.rmtree(out)
            res.setdefault("dataset_256_%d_%s" % (S, flag or "plain"), []).append(dt)
            print("dataset 256 -> %d %s: %.2f s" % (S, flag or "plain", dt), flush=True)
            if len(sys.argv) > 1:
                json.dump(res, open(sys.argv[1], "w"), indent=1)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
