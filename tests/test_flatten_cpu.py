"""CPU: the background flattening of the micrograph ingest without a GPU — the NumPy model of its contract
(tests/flatten_model.py) against a brute-force window loop, the level counts the feature is for, the flag's checking in
spr_pick_amd/ingest.py and on the command line, the operator's fake implementation and the argument checking of the C
entry points."""
import os
import re

import numpy as np
import pytest
import torch

import clip_model
import flatten_model
from clip_model import bits
from conftest import ROOT

SHAPES = [((5, 7), 8), ((33, 33), 1), ((1, 40), 3), ((40, 1), 3), ((70, 17), 5)]      # (shape, R): shared with the GPU tests


@pytest.mark.parametrize("shape,R", SHAPES)
def test_model_equals_the_window_loop(shape, R):
    rs = np.random.RandomState(shape[0])
    images = {"outliers": clip_model.outlier_image(shape, seed=shape[0]),
              "full range": (rs.randn(*shape) * np.exp(rs.uniform(-40, 40, size=shape))).astype(np.float32),
              "integers": rs.randint(-3000, 6000, size=shape).astype(np.float32) / 4}
    for name, img in images.items():
        got, got_rng = flatten_model.flatten(img, R)
        want, want_rng = flatten_model.flatten_brute(img, R)
        assert got.dtype == np.float32 and got.shape == img.shape and np.isfinite(got).all(), name
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got_rng), bits(want_rng)), name
        assert got_rng[0] == got.min() and got_rng[1] == got.max()
        # a wider range than the image's own (as after a clip of other data) is part of the contract
        wide = (np.float32(img.min() - abs(img.min()) * 0.5 - 1), np.float32(img.max() * 2 + 1))
        assert np.array_equal(bits(flatten_model.flatten(img, R, wide)[0]), bits(flatten_model.flatten_brute(img, R, wide)[0]))


def test_model_edges():
    const = np.full((7, 9), 7.25, dtype=np.float32)
    flat, rng = flatten_model.flatten(const, 3)
    assert np.array_equal(bits(flat), np.zeros((7, 9), dtype=np.uint32)) and np.array_equal(bits(rng), [0, 0])
    # a window that covers the whole image subtracts the global mean of the fixed-point values
    img = clip_model.outlier_image((5, 7))
    flat, _ = flatten_model.flatten(img, 8)
    d, t, e = flatten_model.fixed(img, (img.min(), img.max()))
    mean = np.ldexp(np.float64(int(t.sum())) / np.float64(35), e - 30)
    assert np.array_equal(bits(flat), bits((d - mean).astype(np.float32)))
    # the fixed-point step: 31 bits, the maximum maps to at least 2^30
    assert 2 ** 30 <= int(t.max()) < 2 ** 31 and int(t.min()) == 0
    # a plane is removed exactly in the interior (the mean of a symmetric window of a linear function is its centre)
    yy, xx = np.mgrid[0:40, 0:50]
    plane = (3.0 * xx + 2.0 * yy).astype(np.float32)
    flat, _ = flatten_model.flatten(plane, 4)
    assert np.abs(flat[4:-4, 4:-4]).max() <= 2.0 ** -20 and np.abs(flat).max() > 1.0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_level_counts(seed):
    """The point of the feature, on the issue's image: a ramp takes the levels, the flattened image has them back; with
    outliers only clip -> flatten -> clip does."""
    from spr_pick_amd import ingest, micrograph_io
    levels = lambda img: flatten_model.crop_levels(micrograph_io.minmax_uint8(img))
    ramp = flatten_model.ramp_image(seed)
    n_plain, n_flat = levels(ramp), levels(flatten_model.flatten(ramp, 8)[0])
    out = flatten_model.ramp_image(seed, outliers=True)
    ranks = ingest.clip_ranks(out.size, (0.1, 0.1))
    clamped, crng = clip_model.clip(out, *ranks)
    flat, _ = flatten_model.flatten(clamped, 8, crng)
    n_cf, n_cfc = levels(flat), levels(clip_model.clip(flat, *ranks)[0])
    print("levels in the crop: ramp %d, flattened %d; outliers: clip+flatten %d, clip+flatten+clip %d"
          % (n_plain, n_flat, n_cf, n_cfc))
    assert n_plain <= 80 and n_flat >= 120
    assert n_cf <= 40 and n_cfc >= 150


def test_check_flatten():
    from spr_pick_amd import ingest
    assert ingest.MAX_FLATTEN == flatten_model.MAX_R == 1023
    assert ingest.check_flatten(1) == 1 and ingest.check_flatten(np.int64(1023)) == 1023
    for bad in (0, -1, 1024, 1.5, "8", None, True):
        with pytest.raises(ValueError):
            ingest.check_flatten(bad)


def test_command_line():
    from spr_pick_amd import cli
    p = cli.build_parser()
    base = ["eval", "-m", "x.wt", "-d", "t.txt"]
    assert vars(p.parse_args(base))["flatten"] is None
    assert vars(p.parse_args(base + ["--bin", "2"]))["flatten"] is None
    assert vars(p.parse_args(base + ["--bin", "2", "--flatten", "16"]))["flatten"] == 16
    args = vars(p.parse_args(base + ["--flatten", "1023", "--clip", "1,0.1", "--bin", "1"]))
    assert args["flatten"] == 1023 and args["clip"] == (1.0, 0.1)
    with pytest.raises(SystemExit) as e:
        p.parse_args(base + ["--flatten", "8"])              # --flatten without --bin
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        cli.start(base + ["--flatten", "8"])
    assert e.value.code == 2
    args = vars(p.parse_args(["bin", "-d", "raw", "--bin", "4", "-o", "d", "--flatten", "8", "--clip", "0.5"]))
    assert args["flatten"] == 8 and args["clip"] == (0.5, 0.5) and args["bin"] == 4
    assert vars(p.parse_args(["bin", "-d", "raw", "--bin", "4", "-o", "d"]))["flatten"] is None
    for bad in ("0", "-3", "1024", "x", "1.5", ""):
        with pytest.raises(SystemExit):
            p.parse_args(base + ["--bin", "2", "--flatten", bad])
        with pytest.raises(SystemExit):
            p.parse_args(["bin", "-d", "raw", "--bin", "4", "-o", "d", "--flatten", bad])


def test_flatten_is_refused_without_bin():
    from spr_pick_amd.train import DenoiserTrainer
    with pytest.raises(ValueError, match="bin"):
        DenoiserTrainer({}, "joint", flatten=8)


def test_fake_shapes_of_the_flatten_operator():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from spr_pick_amd import _lib, torch_ops
    assert "ingest_flatten" in torch_ops.registered()
    with FakeTensorMode():
        raw = torch.empty(67 * 131 * 2, dtype=torch.uint8, device="cuda")
        binned, rng = torch.ops.sprk.ingest_bin(raw, 1, 67, 131, 2)
        out, rng2 = torch.ops.sprk.ingest_flatten(binned, rng, 5)
        assert tuple(out.shape) == (33, 65) and out.dtype == torch.float32 and out.device == binned.device
        assert tuple(rng2.shape) == (2,) and rng2.dtype == torch.float32
        out, rng3 = torch.ops.sprk.ingest_clip(out, rng2, 10, 2000)
        u8, net = torch.ops.sprk.ingest_finish(out, rng3, True, True)
        assert tuple(u8.shape) == (33, 65) and tuple(net.shape) == (96, 96)
        for R in (0, -1, 1024):
            with pytest.raises(_lib.SprkError):
                torch.ops.sprk.ingest_flatten(binned, rng, R)
        with pytest.raises(_lib.SprkError):
            torch.ops.sprk.ingest_flatten(binned.double(), rng, 5)
        with pytest.raises(_lib.SprkError):
            torch.ops.sprk.ingest_flatten(binned, torch.empty(3, device="cuda"), 5)
        with pytest.raises(_lib.SprkError):
            torch.ops.sprk.ingest_flatten(binned[0], rng, 5)


def test_header_and_exports():
    from spr_pick_amd import _lib
    text = open(os.path.join(ROOT, "include", "sprk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"size_t\s+sprk_ingest_flatten_ws_bytes\s*\(\s*int by,\s*int bx,\s*int R\s*\)\s*;", code)
    assert re.search(r"int\s+sprk_ingest_flatten\s*\(\s*const float \*binned_in,\s*float \*binned_out,\s*int by,\s*int bx,"
                     r"\s*int R,\s*const float \*range_in,\s*float \*range_out,\s*void \*ws,\s*size_t ws_bytes,"
                     r"\s*void \*stream\s*\)\s*;", code)
    assert re.search(r"#define\s+SPRK_INGEST_MAX_FLATTEN\s+1023\b", code)
    assert "#define SPRK_ABI_VERSION 430" in text
    assert {"sprk_ingest_flatten_ws_bytes", "sprk_ingest_flatten"} <= set(_lib.EXPORTS)


def test_c_entry_points_check_their_arguments():
    from spr_pick_amd import _lib
    L = _lib.lib()
    A = 0x100000                                   # never dereferenced: every call below is refused before a launch
    need = L.sprk_ingest_flatten_ws_bytes(64, 64, 8)
    assert need >= 64 * 64 * 8 and L.sprk_ingest_flatten_ws_bytes(64, 64, 1023) == need
    assert L.sprk_ingest_flatten_ws_bytes(4096, 4096, 8) - need == (4096 * 4096 - 64 * 64) * 8      # the uint64 row sums
    assert L.sprk_ingest_flatten_ws_bytes(0, 64, 8) == 0 and L.sprk_ingest_flatten_ws_bytes(64, -1, 8) == 0
    assert L.sprk_ingest_flatten_ws_bytes(65536, 32768, 8) == 0                            # n = 2^31
    assert L.sprk_ingest_flatten_ws_bytes(64, 64, 0) == 0 and L.sprk_ingest_flatten_ws_bytes(64, 64, 1024) == 0
    for k, name in enumerate(("binned_in", "binned_out", "range_in", "range_out")):
        ptrs = [A, A, A, A]
        ptrs[k] = None
        rc = L.sprk_ingest_flatten(ptrs[0], ptrs[1], 64, 64, 8, ptrs[2], ptrs[3], A, need, None)
        assert rc == -1 and b"null" in L.sprk_last_error(), name
    for R in (0, -5, 1024, 2 ** 20):
        assert L.sprk_ingest_flatten(A, A, 64, 64, R, A, A, A, need, None) == -1 and b"radius" in L.sprk_last_error()
    assert L.sprk_ingest_flatten(A, A, 0, 64, 8, A, A, A, need, None) == -1 and b"image size" in L.sprk_last_error()
    assert L.sprk_ingest_flatten(A, A, 65536, 32768, 8, A, A, A, need, None) == -1 and b"image size" in L.sprk_last_error()
    assert L.sprk_ingest_flatten(A, A, 64, 64, 8, A, A, A, need - 1, None) == -2           # SPRK_EWORKSPACE
    assert b"workspace" in L.sprk_last_error()
    assert L.sprk_ingest_flatten(A, A, 64, 64, 8, A, A, None, need, None) == -2
    assert L.sprk_ingest_flatten(A, A, 64, 64, 8, A, A, A + 4, need, None) == -1 and b"aligned" in L.sprk_last_error()
