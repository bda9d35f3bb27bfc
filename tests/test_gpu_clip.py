"""GPU: the percentile clip of the micrograph ingest (sprk_ingest_clip in csrc/ingest.hip, ``torch.ops.sprk.ingest_clip``,
``--clip``) bit for bit against the NumPy model of its contract (tests/clip_model.py): the two order
statistics, the clamped image, and through files the closure between ``joint bin --clip`` and ``joint eval --bin N
--clip``.  Every comparison is on the uint32 views of the floats; none needs a tolerance."""
import glob
import io
import os
import struct

import numpy as np
import pytest
import torch

import clip_model
from clip_model import bits

pytestmark = pytest.mark.gpu

CLIPS = ((0, 0), (0.5, 0.5), (1.0, 0.1), (49.9, 49.9))


def device_bin(img, mode=2, N=1):
    """-> (binned, range) as sprk_ingest_bin leaves them for the image (float32: mode 2, N = 1 is a plain copy)"""
    from spr_pick_amd import torch_ops  # noqa: F401
    ny, nx = img.shape
    raw = torch.from_numpy(np.frombuffer(np.ascontiguousarray(img).tobytes(), dtype=np.uint8).copy()).cuda()
    return torch.ops.sprk.ingest_bin(raw, mode, ny, nx, N)


def check_clip(binned, rng, k_lo, k_hi):
    """One call against the model; -> (clamped, range) on the device."""
    src = binned.cpu().numpy()
    src_rng = rng.cpu().numpy()
    want, want_rng = clip_model.clip(src, k_lo, k_hi)
    out, rng2 = torch.ops.sprk.ingest_clip(binned, rng, k_lo, k_hi)
    got, got_rng = out.cpu().numpy(), rng2.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32 and got_rng.shape == (2,)
    assert np.array_equal(bits(got_rng), bits(want_rng)), (k_lo, k_hi, got_rng, want_rng)
    assert np.array_equal(bits(got), bits(want)), (k_lo, k_hi, int((bits(got) != bits(want)).sum()))
    # functional: neither argument was written
    assert np.array_equal(bits(binned.cpu().numpy()), bits(src)) and np.array_equal(bits(rng.cpu().numpy()), bits(src_rng))
    return out, rng2


@pytest.mark.parametrize("shape", [(40, 96), (70, 17), (33, 33)])
def test_selection_and_clamp(shape):
    """N(100, 5) with hot and black samples and both zeros: n a multiple of 4, n = 4m + 2 and n = 4m + 1."""
    from spr_pick_amd import ingest, micrograph_io
    img = clip_model.outlier_image(shape, seed=shape[0])
    binned, rng = device_bin(img)
    assert np.array_equal(bits(binned.cpu().numpy()), bits(img))
    for clip in CLIPS:
        k_lo, k_hi = ingest.clip_ranks(img.size, clip)
        out, rng2 = check_clip(binned, rng, k_lo, k_hi)
        if clip == (0, 0):                                           # the identity: same image, same range
            assert np.array_equal(bits(out.cpu().numpy()), bits(img))
            assert np.array_equal(bits(rng2.cpu().numpy()), bits(rng.cpu().numpy()))
        # sprk_ingest_finish on the clamped image with this range == the host loader on the clamped image
        u8, _ = torch.ops.sprk.ingest_finish(out, rng2, True, False)
        assert np.array_equal(u8.cpu().numpy(), micrograph_io.minmax_uint8(out.cpu().numpy()))


def test_int16_through_ingest_bin():
    from spr_pick_amd import ingest
    rng = np.random.RandomState(5)
    img = rng.randint(-3000, 6000, size=(67, 131)).astype(np.int16)
    img[3, 7], img[40, 100], img[66, 130] = 32767, 32767, -32768
    binned, r = device_bin(img, 1, 2)
    assert tuple(binned.shape) == (33, 65)
    for clip in CLIPS:
        check_clip(binned, r, *ingest.clip_ranks(binned.numel(), clip))


def test_many_workgroups_and_a_ragged_tail():
    """257 x 259 = 66563 = 4 * 16640 + 3 elements: 17 workgroups of the histogram kernel, the last one part empty, and a
    three-element tail."""
    from spr_pick_amd import _lib, ingest
    L = _lib.lib()
    assert L.sprk_ingest_clip_ws_bytes(257, 259) - L.sprk_ingest_clip_ws_bytes(1, 4) == 16 * 2 * 2048 * 4
    img = clip_model.outlier_image((257, 259), seed=2)
    binned, rng = device_bin(img)
    for clip in ((0.5, 0.5), (1.0, 0.1), (0.001, 0.001)):
        check_clip(binned, rng, *ingest.clip_ranks(img.size, clip))


@pytest.mark.parametrize("name", ["low bits", "high bits", "full range"])
def test_every_pass_decides(name):
    """The span of the keys in the lowest 10 bits only, from bit 21 up only, and over all 32: ranks in the interior."""
    img = clip_model.pass_images()[name]
    binned, rng = device_bin(img)
    n = img.size
    for k_lo, k_hi in ((n // 7, n - n // 5), (1, n - 2), (n // 2 - 1, n // 2), (n // 3, n // 3)):
        check_clip(binned, rng, k_lo, k_hi)


def test_degenerate_histograms():
    from spr_pick_amd import micrograph_io
    # constant: lo == hi, and the normalised image is all zeros (as min-max gives for it)
    const = np.full((40, 50), 7.25, dtype=np.float32)
    binned, rng = device_bin(const)
    out, rng2 = check_clip(binned, rng, 10, 1900)
    assert rng2.tolist() == [7.25, 7.25]
    u8, net = torch.ops.sprk.ingest_finish(out, rng2, True, True)
    assert int(u8.max()) == 0 and float(net.abs().max()) == 0.0
    # two values: every wave counts into one or two bins
    r = np.random.RandomState(9)
    two = np.where(r.rand(128, 128) < 0.3, np.float32(-1.5), np.float32(2.0)).astype(np.float32)
    binned, rng = device_bin(two)
    n, low = two.size, int((two == -1.5).sum())
    for k_lo, k_hi in ((0, n - 1), (low - 1, low), (low, n - 1), (0, low - 1), (5, n - 6)):
        check_clip(binned, rng, k_lo, k_hi)
    # both ranks inside one long run of equal values; and k_lo == k_hi
    run = (100.0 + 5.0 * r.randn(64, 96)).astype(np.float32)
    run.reshape(-1)[1000:4000] = 101.5
    binned, rng = device_bin(run)
    below = int((run < 101.5).sum())
    out, rng2 = check_clip(binned, rng, below + 10, below + 2900)
    assert rng2.tolist() == [101.5, 101.5]
    for k in (0, below - 1, below, run.size // 2, run.size - 1):
        check_clip(binned, rng, k, k)
    assert np.array_equal(micrograph_io.minmax_uint8(out.cpu().numpy()), np.zeros(run.shape, dtype=np.uint8))


def test_in_place_through_the_c_entry_point():
    """binned_out may be binned_in and range_out may be range_in."""
    from spr_pick_amd import _lib, ingest, torch_ops
    img = clip_model.outlier_image((70, 17), seed=4)
    binned, rng = device_bin(img)
    k_lo, k_hi = ingest.clip_ranks(img.size, (1.0, 1.0))
    want, want_rng = clip_model.clip(img, k_lo, k_hi)
    L = _lib.lib()
    ws = torch.empty(L.sprk_ingest_clip_ws_bytes(70, 17), dtype=torch.uint8, device="cuda")
    p = torch_ops._p
    _lib.check(L.sprk_ingest_clip(p(binned), p(binned), 70, 17, k_lo, k_hi, p(rng), p(rng), p(ws), ws.numel(),
                                  torch_ops._stream(binned)), "sprk_ingest_clip")
    assert np.array_equal(bits(binned.cpu().numpy()), bits(want)) and np.array_equal(bits(rng.cpu().numpy()), bits(want_rng))


def test_clipping_restores_the_levels():
    """The point of the feature: outliers leave min-max a handful of the 256 levels, the clipped path gives them back."""
    from spr_pick_amd import ingest
    img = clip_model.outlier_image((40, 96), seed=40)
    binned, rng = device_bin(img)
    plain, _ = torch.ops.sprk.ingest_finish(binned, rng, True, False)
    out, rng2 = torch.ops.sprk.ingest_clip(binned, rng, *ingest.clip_ranks(img.size, (0.5, 0.5)))
    clipped, _ = torch.ops.sprk.ingest_finish(out, rng2, True, False)
    n_plain, n_clipped = clip_model.levels(plain.cpu().numpy()), clip_model.levels(clipped.cpu().numpy())
    print("levels: min-max %d, clipped at 0.5 %% %d" % (n_plain, n_clipped))
    assert n_plain <= 8
    assert n_clipped >= 200


# ---- through files: joint bin --clip, joint eval --bin N --clip ----------------------------------------------------------
def write_raw_mrc(path, array, mode):
    """An int16 (mode 1) MRC file: write_mrc's header with the mode field (bytes 12..15) re-packed."""
    from spr_pick_amd import micrograph_io
    buf = io.BytesIO()
    micrograph_io.write_mrc(buf, np.asarray(array, dtype=np.float32))
    head = bytearray(buf.getvalue()[:1024])
    struct.pack_into("<i", head, 12, mode)
    with open(path, "wb") as f:
        f.write(bytes(head))
        f.write(np.ascontiguousarray(array, dtype=np.int16).tobytes())


def _raw_set(root, n, size, up, seed=0):
    """n synthetic micrographs as int16 MRC files of size*up pixels a side (each synthetic pixel an up x up block plus
    noise), with hot and black pixels planted — whole up x up blocks and single samples — and their table."""
    from spr_pick_amd import synthetic
    rng = np.random.RandomState(seed)
    os.makedirs(root, exist_ok=True)
    lines = ["image_name\tpath"]
    for k in range(n):
        q, _, _ = synthetic.micrograph(k, size=size, blobs=14, seed=seed)
        raw = np.kron(q.astype(np.int16), np.ones((up, up), dtype=np.int16)) * 37 - 3000
        raw = (raw + rng.randint(-40, 41, size=raw.shape)).astype(np.int16)
        for j in range(6):
            y, x = rng.randint(0, size, size=2) * up
            raw[y:y + up, x:x + up] = 32767 if j % 2 == 0 else -32768
        ys, xs = rng.randint(0, size * up, size=(2, 8))
        raw[ys, xs] = 32767
        path = os.path.join(root, "mic%d.mrc" % k)
        write_raw_mrc(path, raw, 1)
        lines.append("mic%d\t%s" % (k, path))
    imgs = os.path.join(root, "raw.txt")
    open(imgs, "w").write("\n".join(lines) + "\n")
    return imgs


def _write_set(root, n=2, size=320, seed=0):
    from spr_pick_amd import micrograph_io, synthetic
    lines, labels = ["image_name\tpath"], ["image_name\tx_coord\ty_coord"]
    for k in range(n):
        q, centres, _ = synthetic.micrograph(k, size=size, blobs=14, seed=seed)
        path = os.path.join(root, "mic%d.mrc" % k)
        with open(path, "wb") as f:
            micrograph_io.write_mrc(f, q.astype(np.float32))
        lines.append("mic%d\t%s" % (k, path))
        for cy, cx in centres:
            labels.append("mic%d\t%d\t%d" % (k, cx, cy))
        labels += ["mic%d\t%d\t%d" % (k, 80 + 9 * j, 82 + 7 * j) for j in range(8)]   # inside the sampler's margin window
    imgs, lab = os.path.join(root, "imgs.txt"), os.path.join(root, "labels.txt")
    open(imgs, "w").write("\n".join(lines) + "\n")
    open(lab, "w").write("\n".join(labels) + "\n")
    return imgs, lab


COMPARED = ("*_nsy.png", "*_out.png", "*_pred_tar.png", "*_scores.txt")


def _outputs(evaluator):
    out_dir = os.path.join(evaluator.run_dir_path, "eval_imgs")
    files = {}
    for pattern in COMPARED:
        for p in glob.glob(os.path.join(out_dir, pattern)):
            files[os.path.basename(p)] = open(p, "rb").read()
    return files


def test_closure_through_files(tmp_path):
    """`joint bin --bin 4 --clip 0.5` writes what `binned_uint8(raw, 4, clip)` normalises, and `joint eval --bin 4 --clip
    0.5` on the raw files writes the bytes plain `joint eval` writes on that output."""
    from spr_pick_amd import cli, ingest, micrograph_io
    raw_imgs = _raw_set(str(tmp_path / "raw"), 2, 320, 4)
    binned = cli.start(["bin", "--dataset", raw_imgs, "--bin", "4", "--out", str(tmp_path / "bin4"), "--clip", "0.5"])
    plain = cli.start(["bin", "--dataset", raw_imgs, "--bin", "4", "--out", str(tmp_path / "bin4_plain")])
    assert binned["geometry"] == plain["geometry"] == {"mic0": (320, 320, 0, 0), "mic1": (320, 320, 0, 0)}
    for k in range(2):
        raw = str(tmp_path / "raw" / ("mic%d.mrc" % k))
        written = str(tmp_path / "bin4" / ("mic%d.mrc" % k))
        arr, header, _ = micrograph_io.parse_mrc(open(written, "rb").read())
        block_means = micrograph_io.parse_mrc(open(str(tmp_path / "bin4_plain" / ("mic%d.mrc" % k)), "rb").read())[0]
        assert header.mode == 2 and arr.shape == (320, 320)
        want, _ = clip_model.clip(block_means, *ingest.clip_ranks(arr.size, (0.5, 0.5)))
        assert np.array_equal(bits(arr), bits(want)) and not np.array_equal(arr, block_means)
        u8 = micrograph_io.load_image(written)
        assert np.array_equal(u8, ingest.binned_uint8(raw, 4, clip=(0.5, 0.5)))
        assert np.array_equal(ingest.binned_uint8(raw, 4, clip=(0, 0)), ingest.binned_uint8(raw, 4))     # --clip 0: no change
        # unclipped, the planted blocks at +-32768 set the range: the micrograph itself (255 * 37 + 80 = 9515 of 65535
        # wide) gets at most 39 levels, the 8 blocks with one hot sample and the two extremes one each
        assert clip_model.levels(ingest.binned_uint8(raw, 4)) <= 49 and clip_model.levels(u8) >= 200

    imgs, lab = _write_set(str(tmp_path))
    runs = str(tmp_path / "runs")
    argv = ("train start -a ssdn -n gaussian --noise_value var -t %s -l %s -ap 0.75 -tau 0.01 "
            "-iter 64 --train_batch_size 16 --print_interval 32 --checkpoint_interval 64 "
            "--nms 18 --bb 24 --runs_dir %s" % (imgs, lab, runs)).split()
    trainer = cli.start(argv)
    model = os.path.join(trainer.run_dir_path, "training_jt", "model_00000064.training")

    def evaluate(dataset, *extra):
        return cli.start(["eval", "-m", model, "-d", dataset, "--runs_dir", runs, "--nms", "18", "--num", "2", *extra])

    host = _outputs(evaluate(binned["images"]))
    dev = _outputs(evaluate(raw_imgs, "--bin", "4", "--clip", "0.5"))
    assert sorted(host) == sorted("mic%d_%s" % (k, d) for k in range(2) for d in ("nsy.png", "out.png", "pred_tar.png",
                                                                                  "scores.txt"))
    assert dev == host
    unclipped = _outputs(evaluate(raw_imgs, "--bin", "4"))
    assert unclipped["mic0_nsy.png"] != dev["mic0_nsy.png"]              # the flag is not a no-op on this set
