"""CPU: the percentile clip of the micrograph ingest without a GPU — the NumPy model of its selection
(tests/clip_model.py) against a sort, the ranks and the flag parsing of spr_pick_amd/ingest.py, the command line, the
operator's fake implementation and the argument checking of the C entry points."""
import os
import re

import numpy as np
import pytest
import torch

import clip_model
from conftest import ROOT


def _cases():
    rng = np.random.RandomState(3)
    out = {"outliers 40x96": clip_model.outlier_image((40, 96)), "outliers 33x33": clip_model.outlier_image((33, 33), 1),
           "constant": np.full((7, 9), 7.25, dtype=np.float32),
           "two values": np.where(rng.rand(64, 64) < 0.3, np.float32(-1.5), np.float32(2.0)).astype(np.float32),
           "ties": rng.randint(-3, 4, size=(50, 41)).astype(np.float32),
           "zeros": np.array([[0.0, -0.0, 0.0, -0.0, 1e-30, -1e-30, 5.0]], dtype=np.float32),
           "integers": (rng.randint(0, 300, size=(64, 64)) * 4096 - 500000).astype(np.float32)}
    out.update(clip_model.pass_images())
    return out


def test_the_key_orders_floats_and_both_zeros():
    x = np.array([-np.inf, -3e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3e38, np.inf], dtype=np.float32)
    k = clip_model.key(x)
    assert np.all(k[1:] > k[:-1])
    assert np.array_equal(clip_model.bits(clip_model.unkey(k)), clip_model.bits(x))


@pytest.mark.parametrize("name", sorted(_cases()))
def test_model_selection_is_a_sort_on_keys(name):
    img = _cases()[name]
    keys = clip_model.key(img.ravel())
    order = np.sort(keys)
    n = keys.size
    ranks = sorted({0, 1, n // 200, n // 3, n // 2, n - 1 - n // 200, n - 2 if n > 1 else 0, n - 1})
    for k in ranks:
        got = clip_model.radix_select(keys, k)
        assert got == order[k], (name, k)
        # np.partition orders by value: equal to the key order except that it does not tell -0.0 from +0.0
        assert clip_model.unkey(got) == np.partition(img.ravel(), k)[k], (name, k)
    lo, hi = clip_model.order_statistics(img, ranks[1], ranks[-2])
    clamped, rng = clip_model.clip(img, ranks[1], ranks[-2])
    assert clamped.dtype == np.float32 and clamped.min() == lo and clamped.max() == hi
    inside = (img >= lo) & (img <= hi)
    assert np.array_equal(clip_model.bits(clamped[inside]), clip_model.bits(img[inside]))      # signed zeros included
    same, rng0 = clip_model.clip(img, 0, n - 1)
    assert np.array_equal(clip_model.bits(same), clip_model.bits(img))
    assert rng0[0] == img.min() and rng0[1] == img.max()


def test_clipping_restores_the_levels():
    """The point of the feature on the issue's image: a handful of outliers leaves min-max a few of the 256 levels."""
    from spr_pick_amd import ingest, micrograph_io
    img = clip_model.outlier_image((40, 96))
    assert clip_model.levels(micrograph_io.minmax_uint8(img)) <= 8
    clamped, _ = clip_model.clip(img, *ingest.clip_ranks(img.size, (0.5, 0.5)))
    assert clip_model.levels(micrograph_io.minmax_uint8(clamped)) >= 200


def test_clip_ranks():
    from spr_pick_amd import ingest
    assert ingest.clip_ranks(3840, (0.5, 0.5)) == (19, 3820)
    assert ingest.clip_ranks(3840, (1.0, 0.1)) == (38, 3836)
    assert ingest.clip_ranks(3840, (0, 0)) == (0, 3839)
    assert ingest.clip_ranks(1, (49.9, 49.9)) == (0, 0)
    for n in (1, 2, 3, 100, 4096 * 4096, 2 ** 31 - 1):
        for clip in ((0, 0), (0.5, 0.5), (49.9, 49.9), (99.9, 0), (0, 99.9), (33.3, 66.6)):
            k_lo, k_hi = ingest.clip_ranks(n, clip)
            assert 0 <= k_lo <= k_hi <= n - 1, (n, clip)


def test_parse_clip():
    from spr_pick_amd import ingest
    assert ingest.parse_clip("0.5") == (0.5, 0.5)
    assert ingest.parse_clip("1.0,0.1") == (1.0, 0.1)
    assert ingest.parse_clip("0") == (0.0, 0.0)
    assert ingest.parse_clip("99,0.5") == (99.0, 0.5)
    for bad in ("-1", "1,-0.5", "50", "50,50", "99.5,0.5", "100", "x", "", "1,2,3", "1,", "nan", "inf", "1;2"):
        with pytest.raises(ValueError):
            ingest.parse_clip(bad)
    for bad in ((50, 50), (-1, 0), (1,), "ab", (float("nan"), 0)):
        with pytest.raises(ValueError):
            ingest.check_clip(bad)


def test_command_line():
    from spr_pick_amd import cli
    p = cli.build_parser()
    base = ["eval", "-m", "x.wt", "-d", "t.txt"]
    assert vars(p.parse_args(base))["clip"] is None
    assert vars(p.parse_args(base + ["--bin", "2"]))["clip"] is None
    assert vars(p.parse_args(base + ["--bin", "2", "--clip", "0.5"]))["clip"] == (0.5, 0.5)
    assert vars(p.parse_args(base + ["--clip", "1,0.1", "--bin", "1"]))["clip"] == (1.0, 0.1)
    with pytest.raises(SystemExit) as e:
        p.parse_args(base + ["--clip", "1"])                 # --clip without --bin
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        cli.start(base + ["--clip", "1"])
    assert e.value.code == 2
    args = vars(p.parse_args(["bin", "-d", "raw", "--bin", "4", "-o", "d", "--clip", "0.5,0.25"]))
    assert args["clip"] == (0.5, 0.25) and args["bin"] == 4
    assert vars(p.parse_args(["bin", "-d", "raw", "--bin", "4", "-o", "d"]))["clip"] is None
    for bad in ("-1", "60", "x", "1,2,3"):
        with pytest.raises(SystemExit):
            p.parse_args(base + ["--bin", "2", "--clip", bad])
        with pytest.raises(SystemExit):
            p.parse_args(["bin", "-d", "raw", "--bin", "4", "-o", "d", "--clip", bad])


def test_clip_is_refused_without_bin():
    from spr_pick_amd.train import DenoiserTrainer
    with pytest.raises(ValueError, match="bin"):
        DenoiserTrainer({}, "joint", clip=(0.5, 0.5))


def test_fake_shapes_of_the_clip_operator():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from spr_pick_amd import _lib, torch_ops
    assert "ingest_clip" in torch_ops.registered()
    with FakeTensorMode():
        raw = torch.empty(67 * 131 * 2, dtype=torch.uint8, device="cuda")
        binned, rng = torch.ops.sprk.ingest_bin(raw, 1, 67, 131, 2)
        out, rng2 = torch.ops.sprk.ingest_clip(binned, rng, 10, 2000)
        assert tuple(out.shape) == (33, 65) and out.dtype == torch.float32 and out.device == binned.device
        assert tuple(rng2.shape) == (2,) and rng2.dtype == torch.float32
        u8, net = torch.ops.sprk.ingest_finish(out, rng2, True, True)
        assert tuple(u8.shape) == (33, 65) and tuple(net.shape) == (96, 96)
        for k_lo, k_hi in ((-1, 5), (6, 5), (0, 33 * 65)):
            with pytest.raises(_lib.SprkError):
                torch.ops.sprk.ingest_clip(binned, rng, k_lo, k_hi)
        with pytest.raises(_lib.SprkError):
            torch.ops.sprk.ingest_clip(binned.double(), rng, 0, 5)
        with pytest.raises(_lib.SprkError):
            torch.ops.sprk.ingest_clip(binned, torch.empty(3, device="cuda"), 0, 5)


def test_header_and_exports():
    from spr_pick_amd import _lib
    text = open(os.path.join(ROOT, "include", "sprk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"size_t\s+sprk_ingest_clip_ws_bytes\s*\(\s*int by,\s*int bx\s*\)\s*;", code)
    assert re.search(r"int\s+sprk_ingest_clip\s*\(\s*const float \*binned_in,\s*float \*binned_out,\s*int by,\s*int bx,"
                     r"\s*long long k_lo,\s*long long k_hi,\s*const float \*range_in,\s*float \*range_out,\s*void \*ws,"
                     r"\s*size_t ws_bytes,\s*void \*stream\s*\)\s*;", code)
    assert "#define SPRK_ABI_VERSION 430" in text
    assert {"sprk_ingest_clip_ws_bytes", "sprk_ingest_clip"} <= set(_lib.EXPORTS)


def test_c_entry_points_check_their_arguments():
    from spr_pick_amd import _lib
    L = _lib.lib()
    A = 0x100000                                   # never dereferenced: every call below is refused before a launch
    need = L.sprk_ingest_clip_ws_bytes(64, 64)
    assert need > 0 and L.sprk_ingest_clip_ws_bytes(4096, 4096) > need
    assert L.sprk_ingest_clip_ws_bytes(0, 64) == 0 and L.sprk_ingest_clip_ws_bytes(64, -1) == 0
    assert L.sprk_ingest_clip_ws_bytes(65536, 32768) == 0                                  # n = 2^31
    for k, name in enumerate(("binned_in", "binned_out", "range_in", "range_out")):
        ptrs = [A, A, A, A]
        ptrs[k] = None
        rc = L.sprk_ingest_clip(ptrs[0], ptrs[1], 64, 64, 0, 4095, ptrs[2], ptrs[3], A, need, None)
        assert rc == -1 and b"null" in L.sprk_last_error(), name
    for k_lo, k_hi in ((-1, 10), (11, 10), (0, 4096), (0, 2 ** 40)):
        assert L.sprk_ingest_clip(A, A, 64, 64, k_lo, k_hi, A, A, A, need, None) == -1 and b"ranks" in L.sprk_last_error()
    assert L.sprk_ingest_clip(A, A, 0, 64, 0, 0, A, A, A, need, None) == -1 and b"image size" in L.sprk_last_error()
    assert L.sprk_ingest_clip(A, A, 64, 64, 0, 4095, A, A, A, need - 1, None) == -2        # SPRK_EWORKSPACE
    assert L.sprk_ingest_clip(A, A, 64, 64, 0, 4095, A, A, None, need, None) == -2
    assert L.sprk_ingest_clip(A, A, 64, 64, 0, 4095, A, A, A + 4, need, None) == -1 and b"aligned" in L.sprk_last_error()
