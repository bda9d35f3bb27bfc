"""Device time of the three kernels of `joint class2d --ctf_weight` at the sizes of a 16 000-particle run (64^2 boxes):
sprk_class_spectrum against its MFMA bound (2 N (S S 2Hs + 2Ku 2S Hs) FLOP / 157.3 TF), sprk_class_wiener at K = 16 and K = 1
against its traffic (the spectra and the tables once), sprk_class_synthesize, sprk_class_average beside them, then
`class2d.classify` on 16 000 planted particles seen through six CTFs to K = 16 with and without the weighting, alternated
(profiles/r19_classctf_bench.txt).  HIP events around the operator call, ten runs after three.
usage: python scratch/classctf_bench.py [OUT.json]"""
import json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from spr_pick_amd import class2d, ctf, extract, torch_ops
import class2d_model
import classctf_model as model

PEAK, HBM = 157.3e12, 8.0e12                     # fp32 MFMA FLOP/s and bytes/s of the data sheet
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

def report(key, t, flop=None, nbytes=None):
    extra = ""
    if flop is not None:
        t["bound_ms"] = flop / PEAK * 1e3
        t["x_bound"] = t["median_ms"] / t["bound_ms"]
        extra = ", MFMA bound %.3f ms, %.2f x" % (t["bound_ms"], t["x_bound"])
    if nbytes is not None:
        t["bytes"] = nbytes
        t["gb_per_s"] = nbytes / t["median_ms"] / 1e6
        extra += ", %.1f MB once through: %.0f GB/s" % (nbytes / 1e6, t["gb_per_s"])
    res[key] = t
    print("%s: median %.3f ms (%.3f .. %.3f)%s" % (key, t["median_ms"], t["min_ms"], t["max_ms"], extra), flush=True)
    if len(sys.argv) > 1:
        json.dump(res, open(sys.argv[1], "w"), indent=1)

N, S, K, A_n, R = 16000, 64, 16, 72, 3
Hs, Ku = S // 2 + 1, S + 1
ops = torch.ops.sprk
i32 = dict(dtype=torch.int32, device="cuda")
w1, w2, w3, w4 = extract.filter_matrices(S, S, "cuda")
shapes = torch_ops.class_spectrum_shapes(S)
rows = model.micrograph_rows()
wn, wd = ctf.weight_tables(S, rows, "flip", "cuda")

P = torch.randn(N, S, S, device="cuda")
spec = torch.empty((N,) + shapes[4], device="cuda")
report("spectrum_N%d_%d" % (N, S), timed(lambda: ops.class_spectrum(P, w1, w2, 0, spec)),
       2.0 * N * (S * S * 2 * Hs + 2 * Ku * 2 * S * Hs), 4.0 * (P.numel() + N * 2 * Ku * Hs))
group = (torch.arange(N, device="cuda") % len(rows)).to(torch.int32)
cs = torch.as_tensor(class2d.angle_table(A_n), device="cuda")
ang, shift = torch.randint(0, A_n, (N,), **i32), torch.randint(-R, R + 1, (N, 2), **i32)
for classes in (K, 1):
    cls = torch.randint(0, classes, (N,), device="cuda")
    members = torch.argsort(cls, stable=True).to(torch.int32)
    offsets = torch.zeros(classes + 1, **i32)
    offsets[1:] = torch.cumsum(torch.bincount(cls, minlength=classes), 0).to(torch.int32)
    fsum = torch.empty((classes,) + shapes[4], device="cuda")
    # the bins it reads: Re, Im and the two tables' values per member and bin (the tables stay in cache: six of them)
    report("wiener_N%d_K%d" % (N, classes), timed(lambda: ops.class_wiener(spec, S, wn, wd, group, members, offsets, 1.0, fsum)),
           None, 4.0 * (N * 2 * Ku * Hs + 2 * len(rows) * Ku * Hs))
    out = torch.empty(classes, S, S, device="cuda")
    report("synthesize_K%d" % classes, timed(lambda: ops.class_synthesize(fsum, S, w3, w4, out)))
    report("average_N%d_K%d" % (N, classes), timed(lambda: ops.class_average(P, ang, shift, cs, members, offsets, out)))
aligned = torch.empty_like(P)
everyone = torch.arange(N, **i32)
report("transform_images_%d" % N, timed(lambda: ops.class_transform(P, everyone, ang, shift, cs, 0, 0, None, aligned)))
report("weight_tables_G%d" % len(rows), timed(lambda: ctf.weight_tables(S, rows, "flip", "cuda")))
many = np.repeat(rows, 72, axis=0)
report("weight_tables_G%d" % len(many), timed(lambda: ctf.weight_tables(S, many, "flip", "cuda")))
del P, spec, aligned

# the whole loop on planted data: the shapes of class2d_model.planted, filtered by |c| of micrograph n mod 6 and the noise
# added on the device (16 000 FFTs on the host are a minute)
t = time.time()
rng = np.random.default_rng(1)
radius = S // 2 - R - 2
labels = rng.integers(0, 3, N)
shapes_ = np.empty((N, S, S), dtype=np.float32)
for n in range(N):
    s = class2d_model.unit_shape(labels[n], S, rng.uniform(0, 2 * np.pi), radius)
    shapes_[n] = np.roll(s, tuple(rng.integers(-R, R + 1, 2)), (0, 1))
absc = torch.as_tensor(np.stack([model.plane_abs_ctf(S, row) for row in rows]), device="cuda")
mic = np.arange(N) % len(rows)
seen = torch.fft.ifft2(absc[torch.as_tensor(mic, device="cuda")] * torch.fft.fft2(torch.as_tensor(shapes_, device="cuda").double())).real
P = (seen + 0.5 * torch.randn(N, S, S, device="cuda", dtype=torch.float64, generator=torch.Generator("cuda").manual_seed(1))).float()
print("planted %d particles in %.1f s" % (N, time.time() - t), flush=True)
weighting = (mic, rows, "flip", 1.0)
for run in range(2):
    for name, arg in (("plain", None), ("ctf_weight", weighting)):
        torch.cuda.synchronize()
        t = time.time()
        out = class2d.classify(P, K, 360.0 / A_n, R, ctf=arg)
        torch.cuda.synchronize()
        dt = time.time() - t
        res.setdefault("classify_%s_N%d_K%d_s" % (name, N, K), []).append(dt)
        res["classify_%s_levels" % name] = [list(l) for l in out["levels"]]
        res["classify_%s_purity" % name] = float(class2d_model.purity(out["cls"], labels, K))
        print("classify %s, %d particles of %d^2 to K = %d: %.2f s, levels %s, purity %.4f, members %s" % (
            name, N, S, K, dt, out["levels"], res["classify_%s_purity" % name], np.bincount(out["cls"], minlength=K).tolist()),
            flush=True)
        if len(sys.argv) > 1:
            json.dump(res, open(sys.argv[1], "w"), indent=1)
