"""CPU: the Fourier-cropped micrograph ingest (`--ftbin F`) without a GPU — the closed-form resampling
matrix against ``extract.crop_matrix64`` and an FFT, the geometry and the coordinate maps, properties of the NumPy model
of the kernel's contract (tests/resample_model.py), the command line, the operator's fake-tensor shapes and the
registrations."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import resample_model

# (ny, nx) -> (by, bx) of the bit-exact GPU comparison (tests/test_gpu_resample.py), int16: identity on one and on both
# axes, the K tails mod 4 and mod 64, odd row pitch, several workgroup tiles in both directions, a long chain in either stage
SHAPES = [((64, 64), (16, 16)), ((96, 96), (96, 96)), ((130, 67), (130, 20)), ((2, 2), (2, 2)), ((5, 7), (3, 2)),
          ((65, 129), (17, 65)), ((300, 260), (150, 100)), ((257, 515), (129, 258)), ((20, 4100), (9, 33)),
          ((4100, 20), (33, 9))]
MODES_SHAPE = ((70, 90), (23, 31))


def make_image(mode, ny, nx, seed=0):
    rng = np.random.RandomState(seed + 17 * mode)
    if mode == 2:
        return (rng.randn(ny, nx) * 100).astype(np.float32)
    info = np.iinfo(resample_model.DTYPES[mode])
    img = rng.randint(info.min, info.max + 1, size=(ny, nx)).astype(resample_model.DTYPES[mode])
    img[-1, -1], img[0, -1] = info.min, info.max
    return img


def matrices(shape, out):
    from spr_pick_amd import ingest
    return ingest.resample_matrix(shape[0], out[0]), ingest.resample_matrix(shape[1], out[1])


@pytest.mark.parametrize("B,S", [(50, 21), (64, 16), (97, 96), (200, 130), (1000, 250), (33, 2), (5, 3), (4100, 33)])
def test_matrix_is_the_crop_operator(B, S):
    from spr_pick_amd import extract, ingest
    m = ingest.resample_matrix64(B, S)
    assert m.shape == (S, B) and m.dtype == np.float64
    err = np.abs(m - extract.crop_matrix64(B, S)).max()
    print("resample_matrix64(%d, %d) - crop_matrix64: %.3g" % (B, S, err))
    assert err <= 1e-12
    assert np.abs(m.sum(axis=1) - 1).max() <= 1e-12
    x = np.random.RandomState(B + S).randn(B)
    spec = np.fft.rfft(x)[:S // 2 + 1]                          # the kept band; irfft takes the real part of an even S's end
    assert np.abs(m @ x - np.fft.irfft(spec, S) * S / B).max() <= 1e-12 * np.abs(x).sum()


def test_matrix_identity_layout_and_refusals():
    from spr_pick_amd import ingest
    assert np.array_equal(ingest.resample_matrix64(96, 96), np.eye(96))
    m = ingest.resample_matrix(50, 21)
    assert m.dtype == np.float32 and m.shape == (21, 50)
    assert np.array_equal(m, ingest.resample_matrix64(50, 21).astype(np.float32))
    assert ingest.resample_matrix(50, 21) is m                   # cached
    t = ingest.resample_matrix(50, 21, "cpu")
    assert t.dtype == torch.float32 and tuple(t.shape) == (32, 52) and t.is_contiguous()
    assert np.array_equal(t.numpy()[:21, :50], m)
    assert not t.numpy()[21:].any() and not t.numpy()[:, 50:].any()
    assert ingest.resample_matrix(50, 21, "cpu") is t
    for B, S in ((5, 1), (5, 6), (1, 1)):
        with pytest.raises(ValueError):
            ingest.resample_matrix64(B, S)


def test_geometry():
    from spr_pick_amd import ingest
    g = ingest.resample_geometry
    assert g(4096, 4096, 1) == (4096, 4096) and g(77, 31, 1) == (77, 31)
    assert g(4096, 4096, 8) == (512, 512)
    assert g(5760, 4092, "9.64") == (598, 424) == resample_model.geometry(5760, 4092, "9.64")
    assert g(5760, 4092, 9.64) == (598, 424)                     # a float goes through its decimal text
    assert g(200, 260, "2.6") == (77, 100)
    assert g(97, 96, "1.5") == g(97, 96, Fraction(3, 2)) == (65, 64)
    assert g(3, 9, 2) == (2, 5)                                  # halves go up: 1.5 -> 2, 4.5 -> 5
    assert g(16384, 16384, 64) == (256, 256)
    assert ingest.check_ftbin("9.64") == Fraction(241, 25) and ingest.check_ftbin(np.int64(3)) == 3
    for bad in (0, "0.99", Fraction(1, 2), 65, "64.01", "abc", None, float("nan"), True):
        with pytest.raises(ValueError):
            g(100, 100, bad)
    with pytest.raises(ValueError):
        g(5, 100, 4)                                             # floor(1.25 + 0.5) = 1 row
    with pytest.raises(ValueError):
        g(16385, 100, 2)
    with pytest.raises(ValueError):
        g(100, 16385, 2)


@pytest.mark.parametrize("n,b", [(4096, 533), (90, 31), (7, 2), (96, 96), (5, 4), (11520, 1440)])
def test_coordinate_maps(n, b):
    from spr_pick_amd import ingest
    x = np.arange(b)
    xr, yr = ingest.to_raw(x, x, n, n, b, b)
    assert np.array_equal(xr, yr) and np.array_equal(xr, [resample_model.to_raw(int(v), n, b) for v in x])
    assert xr.min() >= 0 and xr.max() < n
    assert np.abs(xr - x * n / b).max() <= 0.5                   # the nearest sample to the pixel's position
    xs, ys, inside = ingest.to_scaled(xr, yr, n, n, b, b)
    assert inside.all() and np.array_equal(xs, x) and np.array_equal(ys, x)              # the round trip
    every = np.arange(-2, n + 2)
    xs, _, inside = ingest.to_scaled(every, np.zeros_like(every), n, n, b, b)
    want = [resample_model.to_scaled(int(v), n, b) for v in every]
    assert np.array_equal(inside, [w[1] for w in want])
    assert np.array_equal(xs[inside], [w[0] for w in want if w[1]])
    assert xs[inside].min() == 0 and xs[inside].max() == b - 1 and (np.diff(xs[inside]) >= 0).all()
    assert ingest.unscaled_map(2 * n, n, 2 * b, b)(b - 1, 0) == (int(xr[-1]), 0)


def test_coordinates_keep_x_and_y_apart():
    from spr_pick_amd import ingest
    assert ingest.to_raw(10, 20, 300, 400, 100, 200) == (20, 60)            # x along nx, y along ny
    xs, ys, inside = ingest.to_scaled(20, 60, 300, 400, 100, 200)
    assert (int(xs), int(ys), bool(inside)) == (10, 20, True)
    assert ingest.unscaled_map(300, 400, 100, 200)(np.int64(10), np.int64(20)) == (20, 60)
    assert not ingest.to_scaled(400, 0, 300, 400, 100, 200)[2] and not ingest.to_scaled(0, -1, 300, 400, 100, 200)[2]


def test_model_constant_integer_image_is_constant():
    img = np.full((37, 45), -1234, dtype=np.int16)
    out, rng = resample_model.resample(img, *matrices((37, 45), (12, 17)))
    assert out.shape == (12, 17) and (out == np.float32(-1234)).all() and tuple(rng) == (-1234.0, -1234.0)


def test_model_removes_what_the_block_mean_folds_back():
    """A unit cosine of 20 x 25 cycles on 96 x 120, reduced 3 x: above the new Nyquist frequency (16, 20).  The block mean
    keeps a quarter of it as an alias; the Fourier crop leaves rounding noise."""
    ny, nx = 96, 120
    y, x = np.mgrid[:ny, :nx]
    img = (np.cos(2 * np.pi * 20 * y / ny) * np.cos(2 * np.pi * 25 * x / nx)).astype(np.float32)
    out, _ = resample_model.resample(img, *matrices((ny, nx), (32, 40)))
    block = img.reshape(32, 3, 40, 3).mean(axis=(1, 3))
    print("amplitude left: Fourier crop %.3g, block mean %.3g" % (np.abs(out).max(), np.abs(block).max()))
    assert np.abs(out).max() < 1e-6 and np.abs(block).max() > 0.2


def test_model_keeps_the_band_and_the_mean():
    ny, nx = 96, 120
    y, x = np.mgrid[:ny, :nx]
    img = (50 + 7 * np.cos(2 * np.pi * 5 * y / ny + 0.3) * np.cos(2 * np.pi * 11 * x / nx)).astype(np.float32)
    out, _ = resample_model.resample(img, *matrices((ny, nx), (32, 40)))
    ys, xs = np.mgrid[:32, :40]
    want = 50 + 7 * np.cos(2 * np.pi * 5 * ys / 32 + 0.3) * np.cos(2 * np.pi * 11 * xs / 40)     # pixel s at s * B / S
    assert np.abs(out - want).max() < 1e-4


@pytest.mark.parametrize("mode", [0, 1, 2, 6])
def test_model_within_the_apriori_bound(mode):
    shape, out_shape = MODES_SHAPE
    img = make_image(mode, *shape)
    My, Mx = matrices(shape, out_shape)
    out, rng = resample_model.resample(img, My, Mx)
    assert out.shape == out_shape and rng[0] == out.min() and rng[1] == out.max()
    ratio = resample_model.check_bound(out, img, My, Mx)
    print("mode %d: worst error / bound %.3g" % (mode, ratio))
    assert ratio < 1


def test_parser():
    from spr_pick_amd import cli
    p = cli.build_parser()
    base = ["eval", "--model", "m.wt", "--dataset", "d.txt"]
    assert vars(p.parse_args(base))["ftbin"] is None
    assert vars(p.parse_args(base + ["--ftbin", "9.64"]))["ftbin"] == Fraction(241, 25)
    a = vars(p.parse_args(base + ["--ftbin", "2", "--clip", "0.5", "--flatten", "4"]))
    assert a["ftbin"] == 2 and a["bin"] is None and a["clip"] == (0.5, 0.5) and a["flatten"] == 4
    b = vars(p.parse_args(["bin", "-d", "raw", "--ftbin", "1.5", "-o", "out", "--clip", "1", "--flatten", "8"]))
    assert b["ftbin"] == Fraction(3, 2) and b["bin"] is None and b["clip"] == (1.0, 1.0) and b["flatten"] == 8
    assert vars(p.parse_args(["bin", "-d", "raw", "--bin", "4", "-o", "out"]))["ftbin"] is None
    for bad in (base + ["--bin", "2", "--ftbin", "2"], base + ["--clip", "0.5"], base + ["--flatten", "4"],
                base + ["--ftbin", "0.5"], base + ["--ftbin", "65"], base + ["--ftbin", "x"],
                ["bin", "-d", "raw", "-o", "out"], ["bin", "-d", "raw", "-o", "out", "--bin", "2", "--ftbin", "2"],
                ["bin", "-d", "raw", "-o", "out", "--ftbin", "0"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_python_api_refuses_bin_with_ftbin():
    from spr_pick_amd import ingest
    rows = [(0, "a", "a.mrc")]
    with pytest.raises(ValueError):
        ingest.RawMicrographFeed(rows, 2, device="cpu", ftbin=2)
    with pytest.raises(ValueError):
        ingest.bin_dataset("nowhere", 4, "out", ftbin="1.5")
    with pytest.raises(ValueError):
        ingest.binned("a.mrc", 2, ftbin=2)


def test_fake_tensor_shapes_and_registration():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from spr_pick_amd import _lib, torch_ops
    assert "ingest_resample" in torch_ops.registered()
    assert {"sprk_ingest_resample", "sprk_ingest_resample_ws_bytes"} <= set(_lib.EXPORTS)
    with FakeTensorMode():
        raw = torch.empty(70 * 90 * 2, dtype=torch.uint8, device="cuda")
        my, mx = torch.empty(32, 72, device="cuda"), torch.empty(32, 92, device="cuda")
        out, rng = torch.ops.sprk.ingest_resample(raw, 1, 70, 90, 23, 31, my, mx)
        assert tuple(out.shape) == (23, 31) and out.dtype == torch.float32 and tuple(rng.shape) == (2,)
        for args in ((raw, 3, 70, 90, 23, 31, my, mx), (raw, 1, 70, 90, 1, 31, my, mx), (raw, 1, 70, 90, 23, 91, my, mx),
                     (raw, 2, 70, 90, 23, 31, my, mx), (raw, 1, 70, 90, 23, 31, mx, my),
                     (raw, 1, 70, 90, 23, 31, my, torch.empty(31, 90, device="cuda"))):
            with pytest.raises(_lib.SprkError):
                torch.ops.sprk.ingest_resample(*args)
        with pytest.raises(_lib.SprkError):
            torch.ops.sprk.ingest_resample(torch.empty(8, dtype=torch.uint8, device="cuda"), 1, 16385, 2, 2, 2, my, mx)


def test_library_refuses_bad_sizes_without_a_gpu():
    from spr_pick_amd import _lib
    L = _lib.lib()
    assert L.sprk_ingest_resample_ws_bytes(70, 90, 23, 31) >= 70 * 32 * 4 + 8
    for bad in ((70, 90, 1, 31), (70, 90, 23, 91), (70, 90, 71, 31), (16385, 90, 23, 31), (70, 16385, 23, 31)):
        assert L.sprk_ingest_resample_ws_bytes(*bad) == 0
