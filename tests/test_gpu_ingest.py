"""GPU: the device-side micrograph ingest (csrc/ingest.hip, spr_pick_amd/ingest.py) bit for bit against
a NumPy oracle of its contract — strided-slice block sums in the stated order, then the host path's own
``minmax_uint8``, ``to_unit_float`` and ``pad_to_network_size`` — and the two command-line entry points that use it
(``joint bin``, ``joint eval --bin N``) against the host path on the same pixels.  Every comparison is exact."""
import glob
import io
import os
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {0: np.int8, 1: np.int16, 2: np.float32, 6: np.uint16}


def bin_oracle(img, N):
    """Mean of every N x N block of the centred area.  Integer modes: exact integer sum, one float32 division;
    float32: float32 adds from 0 in row-major order within the block, one float32 division."""
    ny, nx = img.shape
    by, bx, oy, ox = ny // N, nx // N, (ny % N) // 2, (nx % N) // 2
    acc = np.zeros((by, bx), dtype=np.float32 if img.dtype == np.float32 else np.int64)
    for i in range(N):
        for j in range(N):
            acc = acc + img[oy + i:oy + by * N:N, ox + j:ox + bx * N:N]
    assert acc.dtype == (np.float32 if img.dtype == np.float32 else np.int64)
    return acc.astype(np.float32) / np.float32(N * N)


def net_oracle(u8):
    from spr_pick_amd import feed, micrograph_io
    return np.ascontiguousarray(feed.pad_to_network_size(micrograph_io.to_unit_float(u8).T[None]))[0]


def make_image(mode, ny, nx, seed=0):
    rng = np.random.RandomState(seed + 17 * mode)
    if mode == 2:
        return (rng.randn(ny, nx) * 100).astype(np.float32)
    info = np.iinfo(DTYPES[mode])
    img = rng.randint(info.min, info.max + 1, size=(ny, nx)).astype(DTYPES[mode])
    img[0, 0], img[-1, -1] = info.min, info.max
    return img


def device_bin(img, mode, N):
    ny, nx = img.shape
    raw = torch.from_numpy(np.frombuffer(img.tobytes(), dtype=np.uint8).copy()).cuda()
    binned, rng = torch.ops.sprk.ingest_bin(raw, mode, ny, nx, N)
    return binned, rng


def check_bin(img, mode, N):
    binned, rng = device_bin(img, mode, N)
    want = bin_oracle(img, N)
    got = binned.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(got, want), (mode, N, np.abs(got - want).max())
    lo, hi = rng.cpu().numpy()
    assert lo == want.min() and hi == want.max(), (mode, N, lo, hi, want.min(), want.max())
    return binned, rng, want


@pytest.mark.parametrize("N", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("mode", [0, 1, 2, 6])
def test_binning_and_range(mode, N):
    """67 x 131: remainders in both axes, odd offsets, int16 rows that are only 2-byte aligned."""
    from spr_pick_amd import torch_ops  # noqa: F401
    check_bin(make_image(mode, 67, 131), mode, N)


@pytest.mark.parametrize("mode,shape,N", [(2, (64, 256), 4), (1, (64, 512), 8), (1, (64, 512), 16), (0, (48, 256), 16),
                                          (2, (64, 256), 2), (1, (37, 40), 4), (1, (1, 2051), 1)])
def test_aligned_vector_paths(mode, shape, N):
    """Row pitch, offset and chunk all multiples of the load width: the 16-byte loads (fp32 N=4, int16 N=8), two of
    them per chunk (int16 N=16), the 8-byte ones, and the flat N=1 conversion with a tail."""
    from spr_pick_amd import torch_ops  # noqa: F401
    check_bin(make_image(mode, *shape, seed=3), mode, N)


def test_exact_sum_at_the_bound():
    from spr_pick_amd import torch_ops  # noqa: F401
    img = np.full((32, 32), 65535, dtype=np.uint16)
    binned, rng = device_bin(img, 6, 16)
    assert binned.shape == (2, 2) and bool((binned == 65535.0).all())
    assert rng.tolist() == [65535.0, 65535.0]


@pytest.mark.parametrize("shape,N", [((96, 40), 1), ((70, 17), 1), ((40, 96), 1), ((64, 64), 1), ((67, 131), 2)])
def test_normalise_and_layout(shape, N):
    from spr_pick_amd import micrograph_io, torch_ops  # noqa: F401
    for mode in (2, 1):
        binned, rng, want = check_bin(make_image(mode, *shape, seed=5), mode, N)
        u8_want = micrograph_io.minmax_uint8(want)
        net_want = net_oracle(u8_want)
        u8, net = torch.ops.sprk.ingest_finish(binned, rng, True, True)        # both in one launch
        assert u8.dtype == torch.uint8 and np.array_equal(u8.cpu().numpy(), u8_want)
        assert np.array_equal(net.cpu().numpy(), net_want)
        u8_only, none = torch.ops.sprk.ingest_finish(binned, rng, True, False)
        assert none.numel() == 0 and torch.equal(u8_only, u8)
        none, net_only = torch.ops.sprk.ingest_finish(binned, rng, False, True)
        assert none.numel() == 0 and torch.equal(net_only, net)


def test_constant_image_is_all_zeros():
    from spr_pick_amd import torch_ops  # noqa: F401
    img = np.full((40, 50), 7.25, dtype=np.float32)
    binned, rng = device_bin(img, 2, 2)
    u8, net = torch.ops.sprk.ingest_finish(binned, rng, True, True)
    assert tuple(u8.shape) == (20, 25) and tuple(net.shape) == (32, 32)
    assert int(u8.max()) == 0 and float(net.abs().max()) == 0.0


def write_raw_mrc(path, array, mode, extended_header=b""):
    """An MRC file of any supported mode: write_mrc's header with the mode field (bytes 12..15) re-packed."""
    from spr_pick_amd import micrograph_io
    buf = io.BytesIO()
    micrograph_io.write_mrc(buf, np.asarray(array, dtype=np.float32), extended_header)
    head = bytearray(buf.getvalue()[:1024 + len(extended_header)])
    struct.pack_into("<i", head, 12, mode)
    with open(path, "wb") as f:
        f.write(bytes(head))
        f.write(np.ascontiguousarray(array, dtype=DTYPES[mode]).tobytes())


def host_input(path):
    """What load_image + MicrographFeed hand to the network for this file."""
    from spr_pick_amd import micrograph_io
    return torch.from_numpy(net_oracle(micrograph_io.load_image(path)))[None, None]


def test_files_match_the_host_path(tmp_path):
    from spr_pick_amd import ingest, micrograph_io
    f32 = make_image(2, 70, 45, seed=7)
    p32 = str(tmp_path / "f32.mrc")
    with open(p32, "wb") as f:
        micrograph_io.write_mrc(f, f32, extended_header=b"0123456789")    # samples start at byte 1034
    i16 = make_image(1, 45, 70, seed=8)
    p16 = str(tmp_path / "i16.mrc")
    write_raw_mrc(p16, i16, 1, b"0123456789")
    assert micrograph_io.parse_mrc(open(p16, "rb").read())[0].dtype == np.int16
    for path, src in ((p32, f32), (p16, i16), (p32, f32)):               # the third read re-uses a pinned slot
        net, (by, bx), geometry = ingest.ingest(path, 1)
        assert (by, bx) == src.shape and geometry == (by, bx, 0, 0)
        assert net.is_cuda and torch.equal(net.cpu(), host_input(path))
        assert np.array_equal(ingest.binned_uint8(path, 1), micrograph_io.load_image(path))
    assert np.array_equal(ingest.binned_uint8(p16, 3), micrograph_io.minmax_uint8(bin_oracle(i16, 3)))

    stack = str(tmp_path / "stack.mrc")
    with open(stack, "wb") as f:
        micrograph_io.write_mrc(f, np.zeros((2, 8, 8), dtype=np.float32))
    with pytest.raises(ValueError):
        micrograph_io.load_image(stack)
    with pytest.raises(ValueError):
        ingest.ingest(stack, 1)
    with pytest.raises(ValueError):
        ingest.ingest(str(tmp_path / "image.png"), 1)


def _raw_set(root, n, size, up, seed=0):
    """n synthetic micrographs as int16 MRC files of size*up pixels a side (each synthetic pixel an up x up block plus
    noise) and their table."""
    from spr_pick_amd import synthetic
    rng = np.random.RandomState(seed)
    os.makedirs(root, exist_ok=True)
    lines = ["image_name\tpath"]
    for k in range(n):
        q, _, _ = synthetic.micrograph(k, size=size, blobs=14, seed=seed)
        raw = np.kron(q.astype(np.int16), np.ones((up, up), dtype=np.int16)) * 37 - 3000
        raw = (raw + rng.randint(-40, 41, size=raw.shape)).astype(np.int16)
        path = os.path.join(root, "mic%d.mrc" % k)
        write_raw_mrc(path, raw, 1)
        lines.append("mic%d\t%s" % (k, path))
    imgs = os.path.join(root, "raw.txt")
    open(imgs, "w").write("\n".join(lines) + "\n")
    return imgs


def test_joint_bin_closure(tmp_path):
    """`joint bin` output read by the host loader is the device's own uint8 image; labels follow to_binned."""
    import pandas as pd
    from spr_pick_amd import cli, ingest, micrograph_io
    rng = np.random.RandomState(11)
    root = str(tmp_path)
    paths, lines = [], ["image_name\tpath"]
    for k in range(2):
        raw = rng.randint(-2000, 9000, size=(320, 324)).astype(np.int16)
        paths.append(os.path.join(root, "mic%d.mrc" % k))
        write_raw_mrc(paths[-1], raw, 1)
        lines.append("mic%d\t%s" % (k, paths[-1]))
    open(os.path.join(root, "raw.txt"), "w").write("\n".join(lines) + "\n")
    pts = [("mic0", 0, 0), ("mic0", 323, 319), ("mic0", 101, 7), ("mic0", -1, 50), ("mic0", 50, 320), ("mic1", 324, 5),
           ("mic1", 13, 14), ("mic1", 200, -3), ("mic1", 322, 318), ("micX", 10, 10)]      # micX: not in the dataset
    lab = os.path.join(root, "raw_labels.txt")
    open(lab, "w").write("image_name\tx_coord\ty_coord\tnote\n" + "".join("%s\t%d\t%d\tn%d\n" % (n, x, y, i)
                                                                            for i, (n, x, y) in enumerate(pts)))
    out = str(tmp_path / "binned")
    res = cli.start(["bin", "--dataset", os.path.join(root, "raw.txt"), "--bin", "4", "--out", out, "--labels", lab])
    assert res["geometry"] == {"mic0": (80, 81, 0, 0), "mic1": (80, 81, 0, 0)}
    assert micrograph_io.read_image_table(res["images"]) == [(0, "mic%d" % k, os.path.join(out, "mic%d.mrc" % k))
                                                             for k in range(2)]
    for k in range(2):
        written = os.path.join(out, "mic%d.mrc" % k)
        arr, header, _ = micrograph_io.parse_mrc(open(written, "rb").read())
        assert header.mode == 2 and arr.shape == (80, 81)
        assert np.array_equal(arr, bin_oracle(micrograph_io.parse_mrc(open(paths[k], "rb").read())[0], 4))
        assert np.array_equal(micrograph_io.load_image(written), ingest.binned_uint8(paths[k], 4))
    table = pd.read_csv(res["labels"], sep="\t")
    want = []
    for i, (n, x, y) in enumerate(pts):
        xb, yb, inside = ingest.to_binned(x, y, 4, 0, 0, 81, 80)
        if inside and n != "micX":
            want.append((n, int(xb), int(yb), "n%d" % i))
    assert len(want) == 5
    assert res["label_rows"] == {"kept": 5, "outside": 4, "unknown_image": 1}
    assert [tuple(r) for r in table[["image_name", "x_coord", "y_coord", "note"]].itertuples(index=False)] == want


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
    return out_dir, files


def test_cli_eval_bin_matches_the_host_path(tmp_path):
    from spr_pick_amd import cli, ingest, picks
    imgs, lab = _write_set(str(tmp_path))
    runs = str(tmp_path / "runs")
    argv = ("train start -a ssdn -n gaussian --noise_value var -t %s -l %s -ap 0.75 -tau 0.01 "
            "-iter 64 --train_batch_size 16 --print_interval 32 --checkpoint_interval 64 "
            "--nms 18 --bb 24 --runs_dir %s" % (imgs, lab, runs)).split()
    trainer = cli.start(argv)
    model = os.path.join(trainer.run_dir_path, "training_jt", "model_00000064.training")

    def evaluate(dataset, *extra):
        return cli.start(["eval", "-m", model, "-d", dataset, "--runs_dir", runs, "--nms", "18", "--num", "2", *extra])

    # --bin 1 on the files the host loader reads: the same bytes in every compared output
    _, host = _outputs(evaluate(imgs))
    dir1, dev1 = _outputs(evaluate(imgs, "--bin", "1"))
    assert sorted(host) == sorted("mic%d_%s" % (k, d) for k in range(2) for d in ("nsy.png", "out.png", "pred_tar.png",
                                                                                  "scores.txt"))
    assert dev1 == host
    assert not glob.glob(os.path.join(dir1, "*_scores_unbinned.txt"))

    # --bin 2 on 640^2 int16 raw files == the host path on the `joint bin --bin 2` copy of them
    raw_imgs = _raw_set(str(tmp_path / "raw"), 2, 320, 2)
    binned = cli.start(["bin", "--dataset", raw_imgs, "--bin", "2", "--out", str(tmp_path / "bin2")])
    _, host2 = _outputs(evaluate(binned["images"]))
    dir2, dev2 = _outputs(evaluate(raw_imgs, "--bin", "2"))
    assert len(host2) == 8 and dev2 == host2
    counts = []
    for k in range(2):
        names, xy, scores = picks.read_scores(os.path.join(dir2, "mic%d_scores.txt" % k))
        names_u, xy_u, scores_u = picks.read_scores(os.path.join(dir2, "mic%d_scores_unbinned.txt" % k))
        assert names_u == names and np.array_equal(scores_u, scores)
        counts.append(len(names))
        x, y = ingest.to_unbinned(xy[:, 0], xy[:, 1], 2, 0, 0)
        assert np.array_equal(xy_u, np.stack([x, y], axis=1).reshape(-1, 2))
        assert open(os.path.join(dir2, "mic%d_scores_unbinned.txt" % k)).readline() == "image_name\tx_coord\ty_coord\tscore\n"
    print("picks per micrograph:", counts)
    assert sum(counts) > 0                  # the coordinate comparison above is not vacuous
