"""GPU: the background flattening of the micrograph ingest (sprk_ingest_flatten in csrc/ingest.hip,
``torch.ops.sprk.ingest_flatten``, ``--flatten R``) bit for bit against the NumPy model of its contract
(tests/flatten_model.py): the flattened image and its range, and through files the closure between ``joint bin --clip
--flatten`` and ``joint eval --bin N --clip --flatten``.  The window sums are integers, so every comparison is on the
uint32 views of the floats; none needs a tolerance."""
import os

import numpy as np
import pytest
import torch

import clip_model
import flatten_model
from clip_model import bits
from test_flatten_cpu import SHAPES
from test_gpu_clip import _outputs, _write_set, device_bin, write_raw_mrc

pytestmark = pytest.mark.gpu


def check_flatten(binned, rng, R):
    """One call against the model; -> (flat, range) on the device."""
    src, src_rng = binned.cpu().numpy(), rng.cpu().numpy()
    want, want_rng = flatten_model.flatten(src, R, src_rng)
    out, rng2 = torch.ops.sprk.ingest_flatten(binned, rng, R)
    got, got_rng = out.cpu().numpy(), rng2.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32 and got_rng.shape == (2,)
    assert np.array_equal(bits(got), bits(want)), (R, int((bits(got) != bits(want)).sum()))
    assert np.array_equal(bits(got_rng), bits(want_rng)), (R, got_rng, want_rng)
    # functional: neither argument was written
    assert np.array_equal(bits(binned.cpu().numpy()), bits(src)) and np.array_equal(bits(rng.cpu().numpy()), bits(src_rng))
    return out, rng2


def _full_range(shape, seed):
    """clip_model.pass_images()["full range"] at any shape: values over the whole float range"""
    rs = np.random.RandomState(seed)
    return (rs.randn(*shape) * np.exp(rs.uniform(-40, 40, size=shape))).astype(np.float32)


@pytest.mark.parametrize("shape,R", SHAPES)
def test_small_shapes(shape, R):
    """A window larger than the image, R = 1, a single row, a single column, a ragged size."""
    for img in (clip_model.outlier_image(shape, seed=shape[0]), _full_range(shape, shape[0])):
        binned, rng = device_bin(img)
        check_flatten(binned, rng, R)


def test_full_range_image():
    img = clip_model.pass_images()["full range"]
    binned, rng = device_bin(img)
    for R in (1, 8, 100):
        check_flatten(binned, rng, R)


@pytest.mark.parametrize("shape,R", [((257, 259), 16),        # several workgroups in both passes, ragged edges
                                     ((3, 5000), 300),        # five row segments: windows reach across their boundaries
                                     ((2100, 3), 700),        # three chunks of rows, each priming its window in the others
                                     ((262500, 1), 1)])       # more segments and tiles than the grids hold: their strides
def test_segments_and_chunks(shape, R):
    binned, rng = device_bin(clip_model.outlier_image(shape, seed=2))
    check_flatten(binned, rng, R)


def test_a_wider_range_than_the_image():
    """range_in only has to bound the image (after a clip it does; so does any wider pair)."""
    img = clip_model.outlier_image((70, 17), seed=6)
    binned, _ = device_bin(img)
    wide = torch.tensor([-1000.0, 70000.0], device="cuda")
    check_flatten(binned, wide, 5)


def test_constant_image():
    binned, rng = device_bin(np.full((40, 50), 7.25, dtype=np.float32))
    out, rng2 = check_flatten(binned, rng, 4)
    assert np.array_equal(bits(out.cpu().numpy()), np.zeros((40, 50), dtype=np.uint32))       # +0.0f everywhere
    assert np.array_equal(bits(rng2.cpu().numpy()), np.zeros(2, dtype=np.uint32))
    u8, net = torch.ops.sprk.ingest_finish(out, rng2, True, True)
    assert int(u8.max()) == 0 and float(net.abs().max()) == 0.0


def test_int16_through_ingest_bin():
    rs = np.random.RandomState(5)
    img = rs.randint(-3000, 6000, size=(67, 131)).astype(np.int16)
    img[3, 7], img[40, 100], img[66, 130] = 32767, 32767, -32768
    binned, r = device_bin(img, 1, 2)
    assert tuple(binned.shape) == (33, 65)
    for R in (5, 40):
        check_flatten(binned, r, R)


def test_in_place_through_the_c_entry_point():
    """binned_out may be binned_in and range_out may be range_in."""
    from spr_pick_amd import _lib, torch_ops
    img = clip_model.outlier_image((70, 17), seed=4)
    binned, rng = device_bin(img)
    want, want_rng = flatten_model.flatten(img, 5)
    L = _lib.lib()
    ws = torch.empty(L.sprk_ingest_flatten_ws_bytes(70, 17, 5), dtype=torch.uint8, device="cuda")
    p = torch_ops._p
    _lib.check(L.sprk_ingest_flatten(p(binned), p(binned), 70, 17, 5, p(rng), p(rng), p(ws), ws.numel(),
                                     torch_ops._stream(binned)), "sprk_ingest_flatten")
    assert np.array_equal(bits(binned.cpu().numpy()), bits(want)) and np.array_equal(bits(rng.cpu().numpy()), bits(want_rng))


def test_finish_on_the_flattened_image():
    """sprk_ingest_finish with range_out == the host loader's min-max on the flattened image."""
    from spr_pick_amd import micrograph_io
    for img, R in ((flatten_model.ramp_image(3), 8), (clip_model.outlier_image((70, 17), seed=8), 5)):
        binned, rng = device_bin(img)
        out, rng2 = torch.ops.sprk.ingest_flatten(binned, rng, R)
        u8, _ = torch.ops.sprk.ingest_finish(out, rng2, True, False)
        assert np.array_equal(u8.cpu().numpy(), micrograph_io.minmax_uint8(out.cpu().numpy()))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_level_counts(seed):
    """The point of the feature, on the device: a ramp takes the levels and the flattened image has them back; with
    outliers it takes clip -> flatten -> clip."""
    from spr_pick_amd import ingest

    def levels(binned, rng):
        return flatten_model.crop_levels(torch.ops.sprk.ingest_finish(binned, rng, True, False)[0].cpu().numpy())

    binned, rng = device_bin(flatten_model.ramp_image(seed))
    n_plain, n_flat = levels(binned, rng), levels(*torch.ops.sprk.ingest_flatten(binned, rng, 8))
    out = flatten_model.ramp_image(seed, outliers=True)
    ranks = ingest.clip_ranks(out.size, (0.1, 0.1))
    binned, rng = torch.ops.sprk.ingest_clip(*device_bin(out), *ranks)
    flat, frng = torch.ops.sprk.ingest_flatten(binned, rng, 8)
    n_cf, n_cfc = levels(flat, frng), levels(*torch.ops.sprk.ingest_clip(flat, frng, *ranks))
    print("levels in the crop: ramp %d, flattened %d; outliers: clip+flatten %d, clip+flatten+clip %d"
          % (n_plain, n_flat, n_cf, n_cfc))
    assert n_plain <= 80 and n_flat >= 120
    assert n_cf <= 40 and n_cfc >= 150


# ---- through files: joint bin --clip --flatten, joint eval --bin N --clip --flatten --------------------------------------
def _raw_set(root, n, size, up, seed=0):
    """n synthetic micrographs as int16 MRC files of size*up pixels a side (each synthetic pixel an up x up block plus
    noise) under an intensity ramp about twice as wide as the micrograph's own signal, with hot and black pixels
    planted — whole up x up blocks and single samples — and their table."""
    from spr_pick_amd import synthetic
    rs = np.random.RandomState(seed)
    os.makedirs(root, exist_ok=True)
    lines = ["image_name\tpath"]
    side = size * up
    yy, xx = np.mgrid[0:side, 0:side]
    for k in range(n):
        q, _, _ = synthetic.micrograph(k, size=size, blobs=14, seed=seed)
        raw = np.kron(q.astype(np.int32), np.ones((up, up), dtype=np.int32)) * 37 - 3000          # -3000 .. 6435
        raw = raw + rs.randint(-40, 41, size=raw.shape) + (14000 * xx) // (side - 1) + (6000 * yy) // (side - 1)
        raw = raw.astype(np.int16)                                                               # below 26476
        for j in range(6):
            y, x = rs.randint(0, size, size=2) * up
            raw[y:y + up, x:x + up] = 32767 if j % 2 == 0 else -32768
        ys, xs = rs.randint(0, side, size=(2, 8))
        raw[ys, xs] = 32767
        path = os.path.join(root, "mic%d.mrc" % k)
        write_raw_mrc(path, raw, 1)
        lines.append("mic%d\t%s" % (k, path))
    imgs = os.path.join(root, "raw.txt")
    open(imgs, "w").write("\n".join(lines) + "\n")
    return imgs


def test_closure_through_files(tmp_path):
    """`joint bin --bin 4 --clip 0.5 --flatten 16` writes what the models give for clip -> flatten -> clip of the block
    means, `load_image` of it equals `binned_uint8(raw, 4, clip, flatten)`, and `joint eval --bin 4 --clip 0.5 --flatten
    16` on the raw files writes the bytes plain `joint eval` writes on that output."""
    from spr_pick_amd import cli, ingest, micrograph_io
    raw_imgs = _raw_set(str(tmp_path / "raw"), 2, 320, 4)
    flags = ["--clip", "0.5", "--flatten", "16"]
    binned = cli.start(["bin", "--dataset", raw_imgs, "--bin", "4", "--out", str(tmp_path / "bin4")] + flags)
    plain = cli.start(["bin", "--dataset", raw_imgs, "--bin", "4", "--out", str(tmp_path / "bin4_plain")])
    assert binned["geometry"] == plain["geometry"] == {"mic0": (320, 320, 0, 0), "mic1": (320, 320, 0, 0)}
    for k in range(2):
        raw = str(tmp_path / "raw" / ("mic%d.mrc" % k))
        written = str(tmp_path / "bin4" / ("mic%d.mrc" % k))
        arr, header, _ = micrograph_io.parse_mrc(open(written, "rb").read())
        block_means = micrograph_io.parse_mrc(open(str(tmp_path / "bin4_plain" / ("mic%d.mrc" % k)), "rb").read())[0]
        assert header.mode == 2 and arr.shape == (320, 320)
        ranks = ingest.clip_ranks(arr.size, (0.5, 0.5))
        clamped, crng = clip_model.clip(block_means, *ranks)
        flat, _ = flatten_model.flatten(clamped, 16, crng)
        want, _ = clip_model.clip(flat, *ranks)
        assert np.array_equal(bits(arr), bits(want))
        u8 = micrograph_io.load_image(written)
        assert np.array_equal(u8, ingest.binned_uint8(raw, 4, clip=(0.5, 0.5), flatten=16))
        only_flat = ingest.binned_uint8(raw, 4, flatten=16)
        assert np.array_equal(only_flat, micrograph_io.minmax_uint8(flatten_model.flatten(block_means, 16)[0]))
        assert not np.array_equal(u8, only_flat) and not np.array_equal(u8, ingest.binned_uint8(raw, 4, clip=(0.5, 0.5)))

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
    dev = _outputs(evaluate(raw_imgs, "--bin", "4", *flags))
    assert sorted(host) == sorted("mic%d_%s" % (k, d) for k in range(2) for d in ("nsy.png", "out.png", "pred_tar.png",
                                                                                  "scores.txt"))
    assert dev == host
    clipped_only = _outputs(evaluate(raw_imgs, "--bin", "4", "--clip", "0.5"))
    assert clipped_only["mic0_nsy.png"] != dev["mic0_nsy.png"]           # the flag is not a no-op on this set
