"""Device time of sprk_ingest_resample and sprk_psd_tiles on the workloads DESIGN 4.3c / 4.3e quote, with their method: the
stream is kept busy by a matrix product while the host enqueues eight calls between two HIP events, median of nine spans.
For A/B runs of two builds select the library with SPRK_LIB and alternate whole runs of this script
(profiles/r11_mfma_pipeline_refactor.txt).
usage: python scratch/mfma_pipeline_bench.py [OUT.json]"""
import json, os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
from spr_pick_amd import ctf, ingest, torch_ops  # noqa: F401  (torch_ops registers torch.ops.sprk)

CALLS, SPANS = 8, 9
busy_a = torch.randn(8192, 8192, device="cuda")


def upload(img):
    return torch.from_numpy(np.frombuffer(img.tobytes(), dtype=np.uint8).copy()).cuda()


def image(ny, nx):
    rng = np.random.RandomState(ny + nx)
    return np.clip(rng.normal(1000.0, 200.0, size=(ny, nx)), -32768, 32767).astype(np.int16)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    spans = []
    for _ in range(SPANS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        busy_a @ busy_a                              # the host runs ahead of the device while it enqueues the span
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        b.synchronize()
        spans.append(a.elapsed_time(b) * 1000.0 / CALLS)
    return {"median_us": float(np.median(spans)), "min_us": float(min(spans)), "max_us": float(max(spans))}


res = {"lib": os.environ.get("SPRK_LIB", "libsprk.so")}
for ny, nx, by, bx in ((4096, 4096, 512, 512), (8192, 8192, 1024, 1024), (5760, 4092, 598, 424)):
    raw = upload(image(ny, nx))
    my, mx = ingest.resample_matrix(ny, by, "cuda"), ingest.resample_matrix(nx, bx, "cuda")
    res["resample_%dx%d_to_%dx%d" % (ny, nx, by, bx)] = timed(
        lambda: torch.ops.sprk.ingest_resample(raw, 1, ny, nx, by, bx, my, mx))
raw = upload(image(4096, 4096))
for T in (512, 256, 1024):
    w1, w2 = ctf.dft_matrices(T, "cuda")
    res["psd_4096x4096_T%d" % T] = timed(lambda: torch.ops.sprk.psd_tiles(raw, 1, 4096, 4096, T, w1, w2, 0))
print(json.dumps(res, indent=1), flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
