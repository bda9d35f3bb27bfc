"""GPU: the Fourier-cropped micrograph ingest (csrc/resample.hip, ``torch.ops.sprk.ingest_resample``) bit
for bit against the NumPy model of its contract (tests/resample_model.py: two fp32 fma chains in a fixed order), within
the a-priori bound of the float64 product, its range and padding rules, the C ABI's refusals, and the two command-line
entry points (``joint bin --ftbin F``, ``joint eval --ftbin F``)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import resample_model
from test_gpu_ingest import _outputs, _raw_set, _write_set, host_input, write_raw_mrc
from test_resample_cpu import MODES_SHAPE, SHAPES, make_image, matrices

pytestmark = pytest.mark.gpu


def upload(img):
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(img).tobytes(), dtype=np.uint8).copy()).cuda()


def device_resample(img, out_shape):
    from spr_pick_amd import ingest
    ny, nx = img.shape
    by, bx = out_shape
    out, rng = torch.ops.sprk.ingest_resample(upload(img), resample_model.MODE_OF[img.dtype], ny, nx, by, bx,
                                              ingest.resample_matrix(ny, by, "cuda"), ingest.resample_matrix(nx, bx, "cuda"))
    return out.cpu().numpy(), rng.cpu().numpy()


def check_case(img, out_shape):
    My, Mx = matrices(img.shape, out_shape)
    got, rng = device_resample(img, out_shape)
    want, want_rng = resample_model.resample(img, My, Mx)
    assert got.shape == want.shape == tuple(out_shape) and got.dtype == np.float32
    differ = int((got != want).sum())
    ratio = resample_model.check_bound(got, img, My, Mx)
    print("%s %s -> %s: %d of %d pixels differ from the model, worst error / a-priori bound %.3g"
          % (img.dtype, img.shape, tuple(out_shape), differ, got.size, ratio))
    assert np.array_equal(got, want), (differ, float(np.abs(got - want).max()))
    assert rng[0] == got.min() and rng[1] == got.max() and np.array_equal(rng, want_rng)


@pytest.mark.parametrize("mode", [0, 1, 2, 6])
def test_every_mode_matches_the_model(mode):
    shape, out_shape = MODES_SHAPE
    check_case(make_image(mode, *shape), out_shape)


@pytest.mark.parametrize("shape,out_shape", SHAPES, ids=["%dx%d-%dx%d" % (s + o) for s, o in SHAPES])
def test_int16_shapes_match_the_model(shape, out_shape):
    check_case(make_image(1, *shape, seed=shape[0]), out_shape)


def test_large_image_within_the_apriori_bound():
    """1024 x 1536 -> 128 x 192: four workgroup tiles of stage 2 in each direction, sixteen by three of stage 1, K chunks
    in the double-buffered steady state.  The chain model is too slow here: the float64 product and the bound only."""
    img = make_image(1, 1024, 1536, seed=5)
    My, Mx = matrices(img.shape, (128, 192))
    got, rng = device_resample(img, (128, 192))
    ratio = resample_model.check_bound(got, img, My, Mx)
    print("1024x1536 -> 128x192: worst error / a-priori bound %.3g" % ratio)
    assert rng[0] == got.min() and rng[1] == got.max()


def test_both_stage_two_tilings_give_the_same_bits():
    """A 1024 x 1024 output is 256 tiles of 64 x 64, one per compute unit of an MI355X: stage 2 takes its large tile on
    four waves there and the 32 x 32 one on two for every smaller output (the other tests).  Tiling is free under the
    contract, so the large call must give the bits of eight calls on 128 of its rows of My each (the operator takes any
    matrix of the right shape), which run on the small tile."""
    from spr_pick_amd import ingest
    ny, nx, by, bx = 1030, 1040, 1024, 1024
    img = make_image(1, ny, nx, seed=9)
    raw, my, mx = upload(img), ingest.resample_matrix(ny, by, "cuda"), ingest.resample_matrix(nx, bx, "cuda")
    whole, rng = torch.ops.sprk.ingest_resample(raw, 1, ny, nx, by, bx, my, mx)
    parts = [torch.ops.sprk.ingest_resample(raw, 1, ny, nx, 128, bx, my[i:i + 128].contiguous(), mx)[0]
             for i in range(0, by, 128)]
    assert torch.equal(whole, torch.cat(parts))
    assert float(rng[0]) == float(whole.min()) and float(rng[1]) == float(whole.max())
    ratio = resample_model.check_bound(whole.cpu().numpy(), img, *matrices((ny, nx), (by, bx)))
    print("1030x1040 -> 1024x1024: worst error / a-priori bound %.3g" % ratio)


def test_poisoned_workspace_leaves_the_output_finite():
    """The padding rule: U lives in uninitialised memory, so every padded K position is a zero on both operands.  The
    caching allocator may hand the freed NaN block to the operator's workspace; the second half owns its workspace."""
    shape, out_shape = MODES_SHAPE
    img = make_image(1, *shape)
    want, _ = resample_model.resample(img, *matrices(shape, out_shape))
    from spr_pick_amd import _lib
    need = _lib.lib().sprk_ingest_resample_ws_bytes(*shape, *out_shape)
    for _ in range(2):
        poison = torch.full((max(need, 16) // 4 + 1024,), float("nan"), device="cuda")
        del poison
        got, rng = device_resample(img, out_shape)
        assert np.isfinite(got).all() and np.isfinite(rng).all()
        assert np.array_equal(got, want)

    # and through the C ABI, with a workspace this test owns and has filled with NaN
    from spr_pick_amd import ingest
    L = _lib.lib()
    (ny, nx), (by, bx) = shape, out_shape
    raw, my, mx = upload(img), ingest.resample_matrix(ny, by, "cuda"), ingest.resample_matrix(nx, bx, "cuda")
    ws = torch.full((need // 4 + 4096,), float("nan"), device="cuda")     # NaN well past the end of U as well
    out, rng = torch.empty(by, bx, device="cuda"), torch.empty(2, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.sprk_ingest_resample(raw.data_ptr(), 1, ny, nx, by, bx, my.data_ptr(), my.shape[1], mx.data_ptr(), mx.shape[1],
                                out.data_ptr(), rng.data_ptr(), ws.data_ptr(), need, s)
    assert rc == 0, L.sprk_last_error()
    assert np.array_equal(out.cpu().numpy(), want) and float(rng[0]) == want.min() and float(rng[1]) == want.max()


def test_c_abi_refusals_launch_nothing():
    from spr_pick_amd import _lib, ingest
    L = _lib.lib()
    EINVAL, EWORKSPACE = -1, -2
    ny, nx, by, bx = 70, 90, 23, 31
    img = make_image(1, ny, nx)
    raw, my, mx = upload(img), ingest.resample_matrix(ny, by, "cuda"), ingest.resample_matrix(nx, bx, "cuda")
    out, rng = torch.zeros(by, bx, device="cuda"), torch.zeros(2, device="cuda")
    need = L.sprk_ingest_resample_ws_bytes(ny, nx, by, bx)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(raw=raw.data_ptr(), mode=1, ny=ny, nx=nx, by=by, bx=bx, my=my.data_ptr(), ldmy=my.shape[1], mx=mx.data_ptr(),
                ldmx=mx.shape[1], out=out.data_ptr(), range=rng.data_ptr(), ws=ws.data_ptr(), ws_bytes=need)

    def call(**change):
        a = dict(good, **change)
        return L.sprk_ingest_resample(a["raw"], a["mode"], a["ny"], a["nx"], a["by"], a["bx"], a["my"], a["ldmy"], a["mx"],
                                      a["ldmx"], a["out"], a["range"], a["ws"], a["ws_bytes"], s)

    torch.cuda.synchronize()
    before = L.sprk_launch_count()
    cases = [(dict(mode=3), EINVAL, b"mode"), (dict(mode=-1), EINVAL, b"mode"),
             (dict(by=1), EINVAL, b"resampled"), (dict(bx=91), EINVAL, b"resampled"), (dict(by=71), EINVAL, b"resampled"),
             (dict(ny=16385), EINVAL, b"resampled"), (dict(nx=16388, ldmx=16388), EINVAL, b"resampled"),
             (dict(ldmy=68), EINVAL, b"ldmy"), (dict(ldmy=74), EINVAL, b"ldmy"), (dict(ldmx=88), EINVAL, b"ldmx"),
             (dict(ldmx=93), EINVAL, b"ldmx"),
             (dict(raw=None), EINVAL, b"null"), (dict(out=None), EINVAL, b"null"), (dict(range=None), EINVAL, b"null"),
             (dict(raw=raw.data_ptr() + 2), EINVAL, b"aligned"), (dict(my=my.data_ptr() + 4), EINVAL, b"aligned"),
             (dict(mx=mx.data_ptr() + 8), EINVAL, b"aligned"), (dict(out=out.data_ptr() + 4), EINVAL, b"aligned"),
             (dict(ws=ws.data_ptr() + 8), EINVAL, b"aligned"),
             (dict(ws_bytes=need - 1), EWORKSPACE, b"workspace"), (dict(ws=None, ws_bytes=0), EWORKSPACE, b"workspace")]
    for change, code, word in cases:
        assert call(**change) == code, (change, L.sprk_last_error())
        assert word in L.sprk_last_error(), (change, L.sprk_last_error())
    assert L.sprk_launch_count() == before
    assert not out.any() and not rng.any()                       # nothing was written either
    assert call() == 0, L.sprk_last_error()
    assert L.sprk_launch_count() == before + 3                   # the two stages and the range
    want, _ = resample_model.resample(img, *matrices((ny, nx), (by, bx)))
    assert np.array_equal(out.cpu().numpy(), want)


def test_joint_bin_ftbin_closure(tmp_path):
    """`joint bin --ftbin 2.6 [--clip 0.5 --flatten 4]` output read by the host loader is what `ingest(..., ftbin=2.6, ...)`
    makes of the raw files, byte for byte; the written pixels are the model's; labels follow the model's to_scaled."""
    import pandas as pd
    from spr_pick_amd import cli, ingest, micrograph_io
    rng = np.random.RandomState(11)
    root = str(tmp_path)
    paths, raws, lines = [], [], ["image_name\tpath"]
    for k in range(2):
        raws.append(rng.randint(-2000, 9000, size=(200, 260)).astype(np.int16))
        paths.append(os.path.join(root, "mic%d.mrc" % k))
        write_raw_mrc(paths[-1], raws[-1], 1)
        lines.append("mic%d\t%s" % (k, paths[-1]))
    open(os.path.join(root, "raw.txt"), "w").write("\n".join(lines) + "\n")
    pts = [("mic0", 0, 0), ("mic0", 259, 199), ("mic0", 101, 7), ("mic0", -1, 50), ("mic0", 50, 200), ("mic1", 260, 5),
           ("mic1", 13, 14), ("mic1", 200, -3), ("mic1", 258, 198), ("micX", 10, 10)]      # micX: not in the dataset
    lab = os.path.join(root, "raw_labels.txt")
    open(lab, "w").write("image_name\tx_coord\ty_coord\tnote\n" + "".join("%s\t%d\t%d\tn%d\n" % (n, x, y, i)
                                                                            for i, (n, x, y) in enumerate(pts)))
    by, bx = resample_model.geometry(200, 260, "2.6")
    assert (by, bx) == (77, 100)
    for flags, kwargs in (([], {}), (["--clip", "0.5", "--flatten", "4"], dict(clip=(0.5, 0.5), flatten=4))):
        out = str(tmp_path / ("ft" + str(len(flags))))
        res = cli.start(["bin", "--dataset", os.path.join(root, "raw.txt"), "--ftbin", "2.6", "--out", out, "--labels", lab]
                        + flags)
        assert res["geometry"] == {"mic0": (77, 100, 200, 260), "mic1": (77, 100, 200, 260)}
        for k in range(2):
            written = os.path.join(out, "mic%d.mrc" % k)
            arr, header, _ = micrograph_io.parse_mrc(open(written, "rb").read())
            assert header.mode == 2 and arr.shape == (77, 100)
            if not flags:
                assert np.array_equal(arr, resample_model.resample(raws[k], *matrices((200, 260), (77, 100)))[0])
            assert np.array_equal(micrograph_io.load_image(written), ingest.binned_uint8(paths[k], None, ftbin="2.6", **kwargs))
            net, shape, geometry = ingest.ingest(paths[k], None, ftbin="2.6", **kwargs)
            assert shape == (77, 100) and geometry == (77, 100, 200, 260)
            assert torch.equal(net.cpu(), host_input(written))
        table = pd.read_csv(res["labels"], sep="\t")
        want = []
        for i, (n, x, y) in enumerate(pts):
            (xs, inx), (ys, iny) = resample_model.to_scaled(x, 260, 100), resample_model.to_scaled(y, 200, 77)
            if inx and iny and n != "micX":
                want.append((n, xs, ys, "n%d" % i))
        assert len(want) == 5 and want[1] == ("mic0", 99, 76, "n1")
        assert res["label_rows"] == {"kept": 5, "outside": 4, "unknown_image": 1}
        assert [tuple(r) for r in table[["image_name", "x_coord", "y_coord", "note"]].itertuples(index=False)] == want


def test_cli_eval_ftbin(tmp_path):
    """`joint eval --ftbin 2` on 640^2 int16 raw files: the bytes plain `joint eval` writes on the `joint bin --ftbin 2` copy
    of them, plus {name}_scores_unbinned.txt = {name}_scores.txt through to_raw; --ftbin 1 writes no second table."""
    import glob
    from spr_pick_amd import cli, picks
    imgs, lab = _write_set(str(tmp_path))
    runs = str(tmp_path / "runs")
    argv = ("train start -a ssdn -n gaussian --noise_value var -t %s -l %s -ap 0.75 -tau 0.01 "
            "-iter 64 --train_batch_size 16 --print_interval 32 --checkpoint_interval 64 "
            "--nms 18 --bb 24 --runs_dir %s" % (imgs, lab, runs)).split()
    trainer = cli.start(argv)
    model = os.path.join(trainer.run_dir_path, "training_jt", "model_00000064.training")

    def evaluate(dataset, *extra):
        return cli.start(["eval", "-m", model, "-d", dataset, "--runs_dir", runs, "--nms", "18", "--num", "2", *extra])

    raw_imgs = _raw_set(str(tmp_path / "raw"), 2, 320, 2)
    copy = cli.start(["bin", "--dataset", raw_imgs, "--ftbin", "2", "--out", str(tmp_path / "ft2")])
    assert copy["geometry"] == {"mic0": (320, 320, 640, 640), "mic1": (320, 320, 640, 640)}
    _, host = _outputs(evaluate(copy["images"]))
    out_dir, dev = _outputs(evaluate(raw_imgs, "--ftbin", "2"))
    assert len(host) == 8 and dev == host
    counts = []
    for k in range(2):
        names, xy, scores = picks.read_scores(os.path.join(out_dir, "mic%d_scores.txt" % k))
        names_u, xy_u, scores_u = picks.read_scores(os.path.join(out_dir, "mic%d_scores_unbinned.txt" % k))
        assert names_u == names and np.array_equal(scores_u, scores)
        counts.append(len(names))
        want = [(resample_model.to_raw(int(x), 640, 320), resample_model.to_raw(int(y), 640, 320)) for x, y in xy]
        assert np.array_equal(xy_u, np.asarray(want, dtype=np.int64).reshape(-1, 2))
    print("picks per micrograph:", counts)
    assert sum(counts) > 0                  # the coordinate comparison above is not vacuous

    dir1, same = _outputs(evaluate(raw_imgs, "--ftbin", "1"))
    _, bin1 = _outputs(evaluate(raw_imgs, "--bin", "1"))
    assert same == bin1                     # F = 1 is the identity: the pixels of --bin 1
    assert not glob.glob(os.path.join(dir1, "*_scores_unbinned.txt"))
