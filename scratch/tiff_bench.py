"""Device time of sprk_tiff_decode per 4096^2 frame against its traffic bound (compressed bytes in plus decoded bytes out at
6.29 TB/s), and `joint align` on one 40-frame 4096^2 movie as LZW TIFF and as the MRC of the same values, alternated in one
process (profiles/r20_tiff_bench.txt).  The TIFFs are written by PIL's libtiff (`strip_size` sets the rows per
strip), parsed by tiffio; every decoded frame is compared with what was encoded before it is timed.
A timed window is CALLS calls through the C ABI on one stream between two HIP events, over SETS frames and outputs in turn.
usage: python scratch/tiff_bench.py [OUT.json] [--side N] [--frames Z] [--dry] [--kernels-only]   (--dry: build and parse the
files only; --kernels-only: stop before the movie; SPRK_LIB=<path> times another build of the library)"""
import ctypes, json, os, shutil, sys, tempfile, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
from PIL import Image
from spr_pick_amd import tiffio

args = sys.argv[1:]
DRY = "--dry" in args
N = int(args[args.index("--side") + 1]) if "--side" in args else 4096
Z = int(args[args.index("--frames") + 1]) if "--frames" in args else 40
OUT = args[0] if args and not args[0].startswith("--") else None
BW = 6.29e12
SETS = 4
res = {}
rng = np.random.RandomState(0)


def save(key, value):
    res[key] = value
    if OUT:
        json.dump(res, open(OUT, "w"), indent=1)


def write_tiff(path, frames, rows):
    pages = [Image.fromarray(f) for f in frames]
    pages[0].save(path, save_all=True, append_images=pages[1:], compression="tiff_lzw",
                  strip_size=rows * frames[0].shape[1] * frames[0].dtype.itemsize)
    with open(path, "rb") as f:
        t = tiffio.read_tiff_movie(path, f)
    assert t.rows_per_strip == rows and t.frames == len(frames) and t.compression == 5, (t.rows_per_strip, rows)
    return t


def frame_inputs(path, t, k):
    """frame k -> (its byte span, offsets within it, lengths, decoded bytes per strip)"""
    off, length = t.strip_offsets[k], t.strip_lengths[k]
    lo, hi = int(off.min()), int((off + length).max())
    with open(path, "rb") as f:
        f.seek(lo)
        span = f.read(hi - lo)
    return span, off - lo, length, tiffio.strip_bytes(t)


tmp = tempfile.mkdtemp()
try:
    counts8 = [rng.poisson(1.0, size=(N, N)).astype(np.uint8) for _ in range(SETS)]
    counts16 = [f.astype(np.uint16) for f in counts8]
    noise8 = [rng.randint(0, 256, size=(N, N)).astype(np.uint8) for _ in range(SETS)]
    CASES = [("uint8_counts_rows1", counts8, 1, False), ("uint8_counts_rows8", counts8, 8, False),
             ("uint8_counts_rows8_widen", counts8, 8, True), ("uint8_counts_rows64", counts8, 64, False),
             ("uint16_counts_rows8", counts16, 8, False), ("uint8_noise_rows8", noise8, 8, False),
             ("uint8_counts_one_strip", counts8[:1], N, False)]
    prepared = []
    for key, frames, rows, widen in CASES:
        path = os.path.join(tmp, key + ".tif")
        frames = frames + frames[:1] if len(frames) == 1 else frames             # a movie has two frames at least
        t = write_tiff(path, frames, rows)
        prepared.append((key, frames, widen, t, [frame_inputs(path, t, k) for k in range(len(frames))]))
        print("%s: %d strips a frame, %d -> %d bytes a frame" % (key, len(t.strip_rows), frames[0].nbytes,
                                                                 int(t.strip_lengths[0].sum())), flush=True)
    if DRY:
        sys.exit(0)

    import torch
    from spr_pick_amd import _lib, align
    from extract_model import write_raw_mrc
    L = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def window(fn, calls, reps, warm):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            out.append(a.elapsed_time(b) / calls)
        return {"median_ms": float(np.median(out)), "min_ms": float(min(out)), "max_ms": float(max(out)), "runs": out}

    for key, frames, widen, t, inputs in prepared:
        one = key.endswith("one_strip")
        item = 2 if widen else 1
        dev = []
        for (span, off, length, size), frame in zip(inputs, frames):
            src = torch.from_numpy(np.frombuffer(span, dtype=np.uint8).copy()).cuda()
            tabs = [torch.from_numpy(np.ascontiguousarray(v, dtype=np.int64)).cuda() for v in (off, length, size)]
            out = torch.empty(frame.nbytes * item, dtype=torch.uint8, device="cuda")
            status = torch.empty(len(off), dtype=torch.int32, device="cuda")
            dev.append((src, tabs, out, status))

        def call(k):
            src, tabs, out, status = dev[k % len(dev)]
            rc = L.sprk_tiff_decode(src.data_ptr(), src.numel(), tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(),
                                    tabs[0].numel(), 5, 1 if widen else 0, out.data_ptr(), out.numel() // item,
                                    status.data_ptr(), stream)
            assert rc == 0, L.sprk_last_error()

        calls, reps, warm = (1, 2, 1) if one else (20, 5, 2)
        for k in range(1 if one else len(dev)):                                  # results first: every frame, every byte
            call(k)
            src, tabs, out, status = dev[k]
            want = frames[k].astype(np.uint16) if widen else frames[k]
            assert not bool(status.any()) and out.cpu().numpy().tobytes() == want.tobytes(), key
        r = window(lambda: [call(k) for k in range(calls)], calls, reps, 0 if one else warm)
        comp = float(np.mean([len(i[0]) for i in inputs]))
        r["compressed_bytes"], r["decoded_bytes"] = comp, frames[0].nbytes * item
        r["strips"] = len(t.strip_rows)
        r["bound_ms"] = (comp + frames[0].nbytes * item) / BW * 1e3
        r["x_bound"] = r["median_ms"] / r["bound_ms"]
        print("%s: median %.3f ms (%.3f .. %.3f) a frame, %d strips, %.2f MB in, bound %.4f ms, %.0f x" % (
            key, r["median_ms"], r["min_ms"], r["max_ms"], r["strips"], comp / 1e6, r["bound_ms"], r["x_bound"]), flush=True)
        save(key, r)
        del dev
    del prepared
    torch.cuda.empty_cache()
    if "--kernels-only" in args:
        sys.exit(0)

    # joint align on one movie of Z frames: uint8 counts as LZW TIFF (libtiff's own 64 KiB strips) and as the mode-6 MRC
    os.makedirs(os.path.join(tmp, "tif"))
    os.makedirs(os.path.join(tmp, "mrc"))
    movie = [np.roll(counts8[k % SETS], (k // 4, -(k // 5)), axis=(0, 1)) for k in range(Z)]
    tpath, mpath = os.path.join(tmp, "tif", "mov.tiff"), os.path.join(tmp, "mrc", "mov.mrc")
    t0 = time.time()
    tm = write_tiff(tpath, movie, 65536 // N)
    save("movie_libtiff_encode_s", time.time() - t0)
    write_raw_mrc(mpath, np.zeros((2, 2, 2), dtype=np.uint16))
    import struct
    with open(mpath, "r+b") as f:
        f.write(struct.pack("<3i", N, N, Z))
        f.seek(1024)
        for fr in movie:
            f.write(fr.astype(np.uint16).tobytes())
        f.truncate()
    save("movie_bytes", {"tiff": os.path.getsize(tpath), "mrc": os.path.getsize(mpath), "rows_per_strip": tm.rows_per_strip})
    print("movie: %d frames, TIFF %d bytes (%d rows a strip), MRC %d bytes" % (Z, os.path.getsize(tpath), tm.rows_per_strip,
                                                                              os.path.getsize(mpath)), flush=True)
    t0 = time.time()
    with Image.open(tpath) as im:
        for k in range(Z):
            im.seek(k)
            a = np.array(im)
    save("movie_libtiff_decode_host_s", time.time() - t0)
    print("libtiff on the host decodes the movie in %.2f s" % res["movie_libtiff_decode_host_s"], flush=True)
    sums = {}
    for kind in ("mrc", "tif", "mrc", "tif", "mrc", "tif"):
        out = os.path.join(tmp, "out")
        torch.cuda.synchronize()
        t0 = time.time()
        align.align_dataset(os.path.join(tmp, kind), out)
        torch.cuda.synchronize()
        dt = time.time() - t0
        total = open(os.path.join(out, "mov.mrc"), "rb").read()
        assert sums.setdefault("sum", total) == total                           # the same bytes from both, every time
        shutil.rmtree(out)
        res.setdefault("joint_align_%s_s" % kind, []).append(dt)
        print("joint align, %s: %.2f s" % (kind, dt), flush=True)
        save("joint_align_%s_s" % kind, res["joint_align_%s_s" % kind])
finally:
    shutil.rmtree(tmp, ignore_errors=True)
