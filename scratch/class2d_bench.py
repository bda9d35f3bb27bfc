"""Device time of the three kernels of `joint class2d` and of the correlation step at the sizes of a 16 000-particle run
(64^2 boxes, 16 classes x 72 angles), sprk_class_score against its MFMA bound (2 N Mb D FLOP / 157.3 TF) with
sprk_ingest_resample beside it in the same process, then `class2d.classify` on 16 000 planted particles to K = 16
(profiles/r16_class2d_bench.txt).  HIP events around the operator call, ten runs after three.
usage: python scratch/class2d_bench.py [OUT.json]
       rocprofv3 --pmc COUNTERS -d DIR -o NAME -f csv -- python scratch/class2d_bench.py --score-only"""
import json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from spr_pick_amd import align, class2d, torch_ops
import class2d_model as model

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
    res[key] = t
    print("%s: median %.3f ms (%.3f .. %.3f)%s" % (key, t["median_ms"], t["min_ms"], t["max_ms"],
          "" if flop is None else ", bound %.3f ms, %.2f x" % (t["bound_ms"], t["x_bound"])), flush=True)
    if len(sys.argv) > 1:
        json.dump(res, open(sys.argv[1], "w"), indent=1)

N, S, K, A_n, R = 16000, 64, 16, 72, 3
radius = class2d.default_radius(S, R)
ops = torch.ops.sprk
i32 = dict(dtype=torch.int32, device="cuda")

Mb = K * A_n
if "--score-only" in sys.argv:                   # five calls of class_score at the packed K and nothing else: for a counter run
    D = (len(class2d.packed_pixels(S, radius)) + 3) & ~3
    Q, B = torch.randn(N, D, device="cuda"), torch.randn(Mb, D, device="cuda")
    bs, bi = torch.empty(N, device="cuda"), torch.empty(N, **i32)
    for _ in range(5):
        ops.class_score(Q, B, D, None, bs, bi)
    torch.cuda.synchronize()
    sys.exit(0)

# class_score: the packed K (the pixels of the mask, padded to a multiple of 4) and the whole image
for D in ((len(class2d.packed_pixels(S, radius)) + 3) & ~3, S * S):
    Q, B = torch.randn(N, D, device="cuda"), torch.randn(Mb, D, device="cuda")
    bs, bi = torch.empty(N, device="cuda"), torch.empty(N, **i32)
    report("score_N%d_Mb%d_D%d" % (N, Mb, D), timed(lambda: ops.class_score(Q, B, D, None, bs, bi)), 2.0 * N * Mb * D)
    full = torch.empty(N, Mb, device="cuda")
    report("score_N%d_Mb%d_D%d_full_matrix" % (N, Mb, D), timed(lambda: ops.class_score(Q, B, D, full, bs, bi)), 2.0 * N * Mb * D)
    del Q, B, full

# ingest_resample in the same process: the distance from the bound that the pipeline reaches elsewhere
rng = np.random.RandomState(0)
img = rng.randint(-3000, 3000, size=(4096, 4096)).astype(np.int16)
raw = torch.from_numpy(np.frombuffer(img.tobytes(), dtype=np.uint8).copy()).cuda()
my, mx = align.shift_matrix(4096, 4096, 1.37, "cuda"), align.shift_matrix(4096, 4096, -2.6, "cuda")
report("resample_4096_4096", timed(lambda: ops.ingest_resample(raw, 1, 4096, 4096, 4096, 4096, my, mx)), 4.0 * 4096 ** 3)
del raw, my, mx

# the transforms, the averages and the shift search
P = torch.randn(N, S, S, device="cuda")
avgs = torch.randn(K, S, S, device="cuda")
cs = torch.as_tensor(class2d.angle_table(A_n), device="cuda")
pix = torch.as_tensor(class2d.packed_pixels(S, radius), device="cuda")
ldo = (pix.numel() + 3) & ~3
bank, bank_images, Qp = torch.empty(Mb, ldo, device="cuda"), torch.empty(Mb, S, S, device="cuda"), torch.empty(N, ldo, device="cuda")
src = torch.arange(K, **i32).repeat_interleave(A_n)
angles = torch.arange(A_n, **i32).repeat(K)
flags = torch_ops.CLASS_MASK | torch_ops.CLASS_NORMALIZE
report("transform_bank_packed_%d" % Mb, timed(lambda: ops.class_transform(avgs, src, angles, torch.zeros(Mb, 2, **i32), cs, radius, flags, pix, bank)))
report("transform_bank_images_%d" % Mb, timed(lambda: ops.class_transform(avgs, src, angles, torch.zeros(Mb, 2, **i32), cs, radius, flags, None, bank_images)))
everyone, zeros = torch.arange(N, **i32), torch.zeros(N, **i32)
shift = torch.randint(-R, R + 1, (N, 2), **i32)
report("transform_Q_packed_%d" % N, timed(lambda: ops.class_transform(P, everyone, zeros, shift, cs, radius, 0, pix, Qp)))
ang = torch.randint(0, A_n, (N,), **i32)
for classes in (K, 1):
    cls = torch.randint(0, classes, (N,), device="cuda")
    members = torch.argsort(cls, stable=True).to(torch.int32)
    offsets = torch.zeros(classes + 1, **i32)
    offsets[1:] = torch.cumsum(torch.bincount(cls, minlength=classes), 0).to(torch.int32)
    out = torch.empty(classes, S, S, device="cuda")
    report("average_N%d_K%d" % (N, classes), timed(lambda: ops.class_average(P, ang, shift, cs, members, offsets, out)))
best = torch.randint(0, Mb, (N,), device="cuda")
report("gather_refs_Z%d" % N, timed(lambda: bank_images[best]))
refs = bank_images[best]
report("align_corr_Z%d_64_R%d" % (N, R), timed(lambda: ops.align_corr(P, refs, R, 0)), 2.0 * N * (2 * R + 1) ** 2 * S * S)
del P, refs, Qp

# the whole loop on planted data
t = time.time()
data, labels = model.planted(S, N, 1, 1.0, R)
print("planted %d particles in %.1f s" % (N, time.time() - t), flush=True)
P = torch.as_tensor(data, device="cuda")
for run in range(2):
    torch.cuda.synchronize()
    t = time.time()
    out = class2d.classify(P, K, 360.0 / A_n, R)
    torch.cuda.synchronize()
    dt = time.time() - t
    res.setdefault("classify_N%d_K%d_s" % (N, K), []).append(dt)
    res["classify_levels"] = [list(l) for l in out["levels"]]
    res["classify_purity"] = float(model.purity(out["cls"], labels, K))
    print("classify, %d particles of %d^2 to K = %d: %.2f s, levels %s, purity %.4f, members %s" % (
        N, S, K, dt, out["levels"], res["classify_purity"], np.bincount(out["cls"], minlength=K).tolist()), flush=True)
    if len(sys.argv) > 1:
        json.dump(res, open(sys.argv[1], "w"), indent=1)
