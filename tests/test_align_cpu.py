"""CPU: whole-frame motion correction (`joint align`) without a GPU — the closed-form shift-and-crop matrix
against ``ingest.resample_matrix64`` and np.fft, the geometry of the reduced frames, the movie header, the peak fit, the
command line, the registrations, properties of the NumPy models (tests/align_model.py) and the float64 estimation loop
recovering planted drifts."""
import io
import struct

import numpy as np
import pytest
import torch

import align_model

# (B, S): odd / even on either side, S == B, a strong and a slight crop
PAIRS = [(16, 16), (17, 17), (20, 8), (21, 9), (20, 9), (21, 8), (97, 96), (64, 16), (130, 70)]


@pytest.mark.parametrize("B,S", PAIRS)
def test_shift_matrix_properties(B, S):
    from spr_pick_amd import align, ingest
    zero = align.shift_matrix64(B, S, 0.0)
    assert zero.shape == (S, B) and zero.dtype == np.float64
    assert np.abs(zero - ingest.resample_matrix64(B, S)).max() <= 1e-12
    if S == B:
        assert np.array_equal(zero, np.eye(B))
    x = np.random.RandomState(B + S).randn(B)
    for delta in (0.0, 0.37, -2.6, 0.5, 1.0, B / 2.0, 3 * B + 0.25, -1e-3):
        m = align.shift_matrix64(B, S, delta)
        assert np.abs(m.sum(axis=1) - 1).max() <= 1e-12, delta
        err = np.abs(m @ x - align_model.fft_shift_crop(x, S, delta)).max()
        assert err <= 1e-10, (delta, err)
    # a whole number of samples, no crop: a roll
    if S == B:
        assert np.abs(align.shift_matrix64(B, B, 3.0) @ x - np.roll(x, 3)).max() <= 1e-12
    m32 = align.shift_matrix(B, S, 0.37)
    assert m32.dtype == np.float32 and np.array_equal(m32, align.shift_matrix64(B, S, 0.37).astype(np.float32))


def test_shift_matrix_layout_and_refusals():
    from spr_pick_amd import align
    t = align.shift_matrix(50, 21, -1.75, "cpu")
    assert t.dtype == torch.float32 and tuple(t.shape) == (32, 52) and t.is_contiguous()
    assert not t.numpy()[21:].any() and not t.numpy()[:, 50:].any()
    d64 = align.shift_matrix_device64(50, 21, -1.75, "cpu").numpy()
    assert np.abs(d64 - align.shift_matrix64(50, 21, -1.75)).max() <= 1e-14      # the same operations, torch's sines
    assert np.array_equal(t.numpy()[:21, :50], d64.astype(np.float32))
    for B, S in ((5, 1), (5, 6), (1, 1)):
        with pytest.raises(ValueError):
            align.shift_matrix64(B, S, 0.0)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            align.shift_matrix64(8, 8, bad)


def test_geometry():
    from spr_pick_amd import align
    g = align.align_geometry
    assert g(4096, 4096) == (1024, 1024) and g(4096, 4096, 512) == (512, 512)
    assert g(5760, 4092) == (991, 704)              # 4092 * 1024 / 5760 = 727.5: 704 is the nearest multiple of 64; then
    assert g(4092, 5760) == (727, 1024)             # round(5760 * 704 / 4092) = 991
    assert g(256, 320) == (256, 320)                # never larger than the frame: the multiple of 64 at or below nx
    assert g(300, 100) == (192, 64) and g(2, 64) == (2, 64)
    assert g(16384, 16384, 16384) == (16384, 16384)
    Sy, Sx = g(3838, 3710)
    assert Sx % 64 == 0 and (Sy, Sx) == (993, 960)
    for bad in ((100, 63), (1, 64), (16385, 64), (64, 16385)):
        with pytest.raises(ValueError):
            g(*bad)
    with pytest.raises(ValueError):
        g(4096, 4096, 63)
    assert align.check_align_args(1024, 16, 6) == (1024, 16, 6)
    for bad in ((63, 16, 6), (1024, 0, 6), (1024, 32, 6), (1024, 16, 0), (1024.0, 16, 6), (1024, True, 6)):
        with pytest.raises(ValueError):
            align.check_align_args(*bad)


def _header(nz, ny, nx, mode, next_=0):
    from spr_pick_amd import micrograph_io
    buf = io.BytesIO()
    micrograph_io.write_mrc(buf, np.zeros((1, 1, 1), dtype=np.float32))
    head = bytearray(buf.getvalue()[:1024])
    struct.pack_into("<4i", head, 0, nx, ny, nz, mode)
    struct.pack_into("<i", head, 92, next_)
    return bytes(head)


def test_movie_header_accepts_stacks_and_refuses_single_images():
    from spr_pick_amd import align, ingest
    header, start = align.read_movie_header("m.mrc", io.BytesIO(_header(8, 256, 320, 1, next_=64)))
    assert (header.nz, header.ny, header.nx, header.mode, start) == (8, 256, 320, 1, 1024 + 64)
    with pytest.raises(ValueError, match="single 2-D micrograph"):
        ingest.read_header("m.mrc", io.BytesIO(_header(8, 256, 320, 1)))         # what the device half could not open
    for nz in (1, 0):
        with pytest.raises(ValueError, match="movie"):
            align.read_movie_header("m.mrc", io.BytesIO(_header(nz, 256, 320, 1)))
    with pytest.raises(ValueError, match="mode"):
        align.read_movie_header("m.mrc", io.BytesIO(_header(8, 256, 320, 4)))
    with pytest.raises(ValueError, match="shorter"):
        align.read_movie_header("m.mrc", io.BytesIO(b"\0" * 100))
    with pytest.raises(ValueError, match="bad MRC header"):
        align.read_movie_header("m.mrc", io.BytesIO(_header(8, 0, 320, 1)))
    with pytest.raises(ValueError, match="larger"):
        align.read_movie_header("m.mrc", io.BytesIO(_header(8, 16385, 320, 1)))
    with pytest.raises(ValueError, match="MRC files only"):
        align.Movie("movie.tiff", "cpu")


def test_peak_fit_on_an_analytic_paraboloid():
    from spr_pick_amd import align
    R = 5
    d = np.arange(-R, R + 1, dtype=np.float64)
    centres = [(0.0, 0.0), (1.25, -2.4), (-3.5, 3.49), (4.0, -4.0), (0.3, 0.0)]
    cc = np.stack([7.0 - 0.8 * (d[:, None] - cy) ** 2 - 0.3 * (d[None, :] - cx) ** 2 for cy, cx in centres])
    py, px, edge = align.fit_peaks(cc)
    assert np.abs(py - [c[0] for c in centres]).max() <= 1e-12 and np.abs(px - [c[1] for c in centres]).max() <= 1e-12
    assert not edge.any()
    mpy, mpx, medge = align_model.fit_peaks(cc)                  # the model's fit is the same function
    assert np.allclose(mpy, py, atol=1e-12) and np.allclose(mpx, px, atol=1e-12) and not medge.any()
    # a peak outside the window: the arg-max sits on the border, it is reported and the clamped position is used
    out = np.stack([-(d[:, None] - 7.0) ** 2 - (d[None, :] + 1.0) ** 2])
    py, px, edge = align.fit_peaks(out)
    assert edge.all() and py[0] == R - 1 + 0.5 and abs(px[0] + 1.0) <= 1e-12
    flat = np.zeros((1, 5, 5))                                   # no curvature: the arg-max itself
    assert align.fit_peaks(flat)[0][0] == -1.0                   # index 0 clamped to 1
    for bad in (np.zeros((1, 4, 4)), np.zeros((1, 5, 7)), np.zeros((1, 1, 1))):
        with pytest.raises(ValueError):
            align.fit_peaks(bad)


def test_parser():
    from fractions import Fraction
    from spr_pick_amd import cli
    p = cli.build_parser()
    a = vars(p.parse_args(["align", "--movies", "movies", "--out", "sums"]))
    assert (a["ftbin"], a["align_size"], a["max_shift"], a["iters"], a["no_align"]) == (1, 1024, 16, 6, False)
    a = vars(p.parse_args(["align", "--movies", "m.txt", "--out", "o", "--ftbin", "1.5", "--align_size", "512", "--max_shift",
                           "31", "--iters", "3", "--no_align"]))
    assert (a["ftbin"], a["align_size"], a["max_shift"], a["iters"], a["no_align"]) == (Fraction(3, 2), 512, 31, 3, True)
    base = ["align", "--movies", "m", "--out", "o"]
    for bad in (["align", "--movies", "m"], ["align", "--out", "o"], base + ["--ftbin", "0.5"], base + ["--ftbin", "65"],
                base + ["--max_shift", "0"], base + ["--max_shift", "32"], base + ["--align_size", "32"],
                base + ["--align_size", "20000"], base + ["--iters", "0"], base + ["--iters", "x"], base + ["--bin", "2"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    text = p._subparsers._group_actions[0].choices["align"].format_help()
    text = " ".join(text.split())
    for word in ("gain", "dose weighting", "local", "TIFF", "EER"):          # the help says what is out of scope
        assert word in text, word


def test_names_in_header_binding_and_torch_library():
    import os
    import re
    from conftest import ROOT
    from torch._subclasses.fake_tensor import FakeTensorMode
    from spr_pick_amd import _lib, torch_ops
    names = {"sprk_align_corr", "sprk_align_accumulate", "sprk_align_accumulate_ws_bytes"}
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sprk.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(sprk_[a-z0-9_]+)\s*\(", text))
    assert re.search(r"#define SPRK_ABI_VERSION 430\b", text) and _lib.ABI_VERSION == 430
    assert names <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names) and L.sprk_version() == 430
    assert {"align_corr", "align_accumulate"} <= set(torch_ops.registered())
    assert L.sprk_align_accumulate_ws_bytes(70, 90, 23, 31) == 70 * 32 * 4
    for bad in ((70, 90, 1, 31), (70, 90, 23, 91), (16385, 90, 23, 31)):
        assert L.sprk_align_accumulate_ws_bytes(*bad) == 0
    # refusals come before anything touches the device
    assert L.sprk_align_corr(0x1000, 0x1000, 0, 1, 0, 64, 3, 0, 0x1000, None) == -1 and b"multiple of 64" in L.sprk_last_error()
    assert L.sprk_align_corr(0x1000, 0x1000, 0, 1, 64, 96, 3, 0, 0x1000, None) == -1
    assert L.sprk_align_corr(0x1000, 0x1000, 0, 1, 64, 64, 32, 0, 0x1000, None) == -1 and b"radius" in L.sprk_last_error()
    assert L.sprk_align_corr(0x1000, 0x1000, 0, 1, 64, 64, 3, 48, 0x1000, None) == -1 and b"tile" in L.sprk_last_error()
    assert L.sprk_align_corr(0x1000, 0x1000, 100, 2, 64, 64, 3, 0, 0x1000, None) == -1 and b"stride" in L.sprk_last_error()
    assert L.sprk_align_corr(0x1004, 0x1000, 0, 1, 64, 64, 3, 0, 0x1000, None) == -1 and b"aligned" in L.sprk_last_error()
    with FakeTensorMode():
        a, r = torch.empty(3, 70, 128, device="cuda"), torch.empty(70, 128, device="cuda")
        assert tuple(torch.ops.sprk.align_corr(a, r, 4).shape) == (3, 9, 9)
        assert tuple(torch.ops.sprk.align_corr(a, torch.empty(3, 70, 128, device="cuda"), 31, 64).shape) == (3, 63, 63)
        for args in ((a, r, 0), (a, r, 32), (a, r, 4, 48), (a, torch.empty(2, 70, 128, device="cuda"), 4),
                     (torch.empty(3, 70, 96, device="cuda"), torch.empty(70, 96, device="cuda"), 4)):
            with pytest.raises(_lib.SprkError):
                torch.ops.sprk.align_corr(*args)
        raw = torch.empty(70 * 90 * 2, dtype=torch.uint8, device="cuda")
        my, mx = torch.empty(32, 72, device="cuda"), torch.empty(32, 92, device="cuda")
        y = torch.empty(23, 31, device="cuda")
        assert torch.ops.sprk.align_accumulate(raw, 1, 70, 90, 23, 31, my, mx, 5.0, y, True) is None
        for args in ((raw, 3, 70, 90, 23, 31, my, mx, 0.0, y, True), (raw, 1, 70, 90, 23, 31, mx, my, 0.0, y, True),
                     (raw, 1, 70, 90, 23, 31, my, mx, 0.0, torch.empty(23, 32, device="cuda"), True)):
            with pytest.raises(_lib.SprkError):
                torch.ops.sprk.align_accumulate(*args)


def test_model_corr_finds_a_rolled_frame():
    """the sign convention of the window: a frame whose content is displaced by d against its reference (a = roll(r, d))
    has its peak at shift -d, and there the window holds sum(r * r)"""
    rng = np.random.RandomState(3)
    r = rng.randn(9, 64).astype(np.float32)
    a = np.stack([np.roll(r, (2, -3), axis=(0, 1)), r])
    cc = align_model.corr(a, r, 4)
    assert cc.shape == (2, 9, 9) and cc.dtype == np.float32
    assert np.unravel_index(cc[0].argmax(), (9, 9)) == (4 - 2, 4 + 3) and np.unravel_index(cc[1].argmax(), (9, 9)) == (4, 4)
    want = align_model.window(a[0].astype(np.float64), r.astype(np.float64), 4)
    assert np.abs(cc[0] - want).max() <= 1e-4 * np.abs(want).max()
    assert np.array_equal(align_model.corr(a, np.stack([r, r]), 4), cc)       # a shared reference is a stride of zero


def test_model_accumulate_is_one_chain_and_within_the_bound():
    from spr_pick_amd import align
    rng = np.random.RandomState(5)
    ny, nx, by, bx, Z = 37, 45, 12, 17, 3
    frames = [rng.randint(-3000, 3000, size=(ny, nx)).astype(np.int16) for _ in range(Z)]
    Mys = [align.shift_matrix(ny, by, d) for d in (0.4, -1.3, 2.0)]
    Mxs = [align.shift_matrix(nx, bx, d) for d in (-0.7, 0.0, 5.5)]
    anchor = float(frames[0][0, 0])
    y = align_model.accumulate(frames, Mys, Mxs, anchor)
    assert y.shape == (by, bx) and y.dtype == np.float32
    ratio = align_model.check_bound(y, frames, Mys, Mxs, anchor)
    print("worst error / a-priori bound %.3g" % ratio)
    assert ratio < 1
    # not the sum of the frames' own chains: the order of the roundings is part of the contract
    each = sum(align_model.accumulate([f], [a], [b], anchor).astype(np.float64) for f, a, b in zip(frames, Mys, Mxs))
    assert np.abs(y - each).max() <= 3 * 2.0 ** -24 * np.abs(each).max() * Z
    # constant frames through matrices whose rows sum to 1: the anchor term restores the sum exactly
    const = [np.full((ny, nx), 1234, dtype=np.int16)] * Z
    assert not align_model.accumulate(const, Mys, Mxs, 1234.0).any()


@pytest.fixture(scope="module")
def model_errors():
    ny, nx = align_model.MOVIE_SHAPE
    errs = []
    for seed, noise in align_model.MOVIE_CASES:
        movie, _, drift = align_model.make_movie(ny, nx, align_model.MOVIE_FRAMES, seed, noise)
        assert movie.dtype == np.int16 and np.abs(drift).max() <= 5.0 + 1e-9 and np.abs(drift.mean(axis=0)).max() < 1e-9
        est = align_model.estimate_movie(movie, ny, nx)
        errs.append(float(np.abs(est - drift).max()))
        print("seed %d, noise %.1f x signal: worst |estimated - planted| = %.4f raw pixels" % (seed, noise, errs[-1]))
    return errs


def test_model_loop_recovers_planted_drifts(model_errors):
    from spr_pick_amd import align
    assert align.align_geometry(*align_model.MOVIE_SHAPE) == align_model.MOVIE_SHAPE      # these movies are not reduced
    assert max(model_errors) <= align_model.MODEL_WORST
    assert 1.5 * align_model.MODEL_WORST < 0.5
    assert min(model_errors) < 0.1                               # and at low noise the parabola's bias is all there is
