"""CPU: the tiled power spectrum (`joint ctf`) without a GPU — the DFT matrices against their float64
definition, the tile geometry, the NumPy model of the kernel's contract (tests/psd_model.py) inside its a-priori bound of
np.fft.rfft2, the operator's fake-tensor shapes, its refusals and the registrations."""
import functools

import numpy as np
import pytest
import torch

import psd_model
from test_resample_cpu import make_image

# (ny, nx, T) of the bit-exact GPU comparison (tests/test_gpu_psd.py), int16: one tile; margins on both axes; T not a power
# of two; a wide image; K of several chunks, several output tiles and the ragged 2H = 130; 511 tiles
# (160, 241, 160): stage 1 with K = 160 (three chunks of 64, a tail of 32), stage 2 with K = 320 (five chunks), three row
# blocks with the last one half inactive, 2H = 162 ragged, two tiles on an odd pitch
SHAPES = [(32, 32, 32), (100, 70, 32), (97, 131, 48), (64, 200, 64), (130, 257, 128), (160, 241, 160), (17, 4100, 16)]
MODES_SHAPE = (45, 61, 16)                       # odd pitch, margins on both axes, 24 tiles


def matrices(T):
    from spr_pick_amd import ctf
    return ctf.dft_matrices(T)


@functools.lru_cache(maxsize=None)
def model_case(mode, ny, nx, T, seed=0):
    """-> (img, the model's P): computed once, shared by the CPU and the GPU tests, never written to"""
    img = make_image(mode, ny, nx, seed=seed)
    P = psd_model.psd(img, *matrices(T), T)
    img.setflags(write=False)
    P.setflags(write=False)
    return img, P


@pytest.mark.parametrize("T", [16, 48, 128, 1024])
def test_dft_matrices_against_the_float64_definition(T):
    from spr_pick_amd import ctf
    H = T // 2 + 1
    W1, W2 = ctf.dft_matrices64(T)
    assert W1.shape == (2 * H, T) and W2.shape == (2 * T, 2 * T) and W1.dtype == W2.dtype == np.float64
    # the DFT matrix by its definition, the product NOT reduced: its angle of up to 2 pi T carries a rounding error of up
    # to 2 pi T 2^-53 = 7e-16 T, which is all this comparison can ask for (and why the matrices reduce mod T first)
    F = np.exp(-2j * np.pi * np.outer(np.arange(T), np.arange(T)) / T)
    tol = 1e-15 * T
    assert np.abs(W1[:H] - F[:H].real).max() <= tol and np.abs(W1[H:] + F[:H].imag).max() <= tol
    assert np.abs(W2[:T, :T] - F.real).max() <= tol and np.abs(W2[T:, :T] + F.imag).max() <= tol
    assert np.array_equal(W2[:T, T:], -W2[T:, :T]) and np.array_equal(W2[T:, T:], W2[:T, :T])
    # reduced mod T first: the entries at multiples of a quarter turn are exact to the last bit of sin(pi) in float64
    assert W1[1, 0] == 1 and W1[H + 1, 0] == 0 and abs(W1[1, T // 4]) <= 2e-16 and W2[T // 2, 1] == -1
    # the transform they state, against an FFT
    x = np.random.RandomState(T).randn(T, T)
    U = x @ W1.T
    V = np.concatenate([U[:, :H], U[:, H:]])
    f = np.fft.rfft2(x)
    assert np.abs(W2[:T] @ V - f.real).max() <= 1e-12 * np.abs(x).sum()
    assert np.abs(W2[T:] @ V + f.imag).max() <= 1e-12 * np.abs(x).sum()


def test_dft_matrices_layout_cache_and_refusals():
    from spr_pick_amd import ctf
    W1, W2 = ctf.dft_matrices(48)
    assert W1.dtype == W2.dtype == np.float32 and W1.shape == (50, 48) and W2.shape == (96, 96)
    w64 = ctf.dft_matrices64(48)
    assert np.array_equal(W1, w64[0].astype(np.float32)) and np.array_equal(W2, w64[1].astype(np.float32))
    assert ctf.dft_matrices(48)[0] is W1
    t1, t2 = ctf.dft_matrices(48, "cpu")
    assert t1.dtype == torch.float32 and tuple(t1.shape) == (64, 48) and tuple(t2.shape) == (96, 96)
    assert t1.is_contiguous() and t2.is_contiguous() and t1.shape[1] % 4 == 0 and t2.shape[1] % 4 == 0
    assert np.array_equal(t1.numpy()[:50], W1) and not t1.numpy()[50:].any() and np.array_equal(t2.numpy(), W2)
    assert ctf.dft_matrices(48, "cpu")[0] is t1
    for bad in (8, 24, 1040, 0, -16, 16.0):
        with pytest.raises(ValueError):
            ctf.dft_matrices64(bad)


def test_tile_counts_and_origins():
    from spr_pick_amd import ctf
    want = {(45, 61, 16): (4, 6), (32, 32, 32): (1, 1), (100, 70, 32): (5, 3), (97, 131, 48): (3, 4)}
    for (ny, nx, T), (ty, tx) in want.items():
        assert ctf.tile_geometry(ny, nx, T) == (ty, tx) == psd_model.geometry(ny, nx, T)
        org = psd_model.origins(ny, nx, T)
        assert len(org) == ty * tx and org[0] == (0, 0) and org[-1] == ((ty - 1) * T // 2, (tx - 1) * T // 2)
        assert org[1 % len(org)] == ((0, T // 2) if tx > 1 else ((T // 2, 0) if ty > 1 else (0, 0)))
        # every tile inside; the margin left over is shorter than half a tile
        assert 0 <= ny - (org[-1][0] + T) < T // 2 and 0 <= nx - (org[-1][1] + T) < T // 2
    assert psd_model.origins(97, 131, 48)[5] == (24, 24)
    with pytest.raises(ValueError):
        ctf.tile_geometry(31, 64, 32)


@pytest.mark.parametrize("mode", [0, 1, 2, 6])
def test_model_within_the_apriori_bound(mode):
    ny, nx, T = MODES_SHAPE
    img, P = model_case(mode, ny, nx, T)
    assert P.shape == (T, T // 2 + 1) and P.dtype == np.float32 and (P >= 0).all()
    ratio = psd_model.check_bound(P, img, *matrices(T), T)
    print("mode %d: worst error / bound %.3g" % (mode, ratio))
    assert ratio < 1


def test_model_properties():
    ny, nx, T = 100, 70, 32
    img, P = model_case(1, ny, nx, T, seed=ny)
    W1, W2 = matrices(T)
    ratio = psd_model.check_bound(P, img, W1, W2, T)
    print("int16 100x70 T 32: worst error / bound %.3g" % ratio)
    # a subset of columns gives the bits of those columns
    cols = [0, 1, 7, 16]
    assert np.array_equal(psd_model.psd(img, W1, W2, T, cols=cols), P[:, cols])
    # only x - x[0,0] enters, and the margin does not
    small = (img // 4).astype(np.int16)
    assert np.array_equal(psd_model.psd(small + np.int16(1000), W1, W2, T), psd_model.psd(small, W1, W2, T))
    cut = np.ascontiguousarray(img[:96, :64])
    assert np.array_equal(psd_model.psd(cut, W1, W2, T), P)
    # fma32 rounds once: a product that a separately rounded multiply gets wrong
    a, b, c = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(-1)
    assert float(psd_model.fma32(np.array([a]), np.array([b]), np.array([c]))[0]) == 2.0 ** -11 + 2.0 ** -24


def test_fake_tensor_shapes_and_registration():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from spr_pick_amd import _lib, torch_ops
    assert "psd_tiles" in torch_ops.registered() and hasattr(torch.ops.sprk, "psd_tiles")
    assert {"sprk_psd_tiles", "sprk_psd_tiles_ws_bytes"} <= set(_lib.EXPORTS) and _lib.ABI_VERSION == 430
    with FakeTensorMode():
        raw = torch.empty(97 * 131 * 2, dtype=torch.uint8, device="cuda")
        w1, w2 = torch.empty(64, 48, device="cuda"), torch.empty(96, 96, device="cuda")
        P = torch.ops.sprk.psd_tiles(raw, 1, 97, 131, 48, w1, w2, 0)
        assert tuple(P.shape) == (48, 25) and P.dtype == torch.float32
        for args in ((raw, 3, 97, 131, 48, w1, w2, 0), (raw, 1, 97, 131, 40, w1, w2, 0), (raw, 1, 47, 131, 48, w1, w2, 0),
                     (raw, 1, 97, 47, 48, w1, w2, 0), (raw, 2, 97, 131, 48, w1, w2, 0), (raw, 1, 97, 131, 48, w2, w1, 0),
                     (raw, 1, 97, 131, 48, w1, w2, -1), (raw, 1, 97, 131, 48, torch.empty(50, 48, device="cuda"), w2, 0),
                     (raw, 1, 97, 131, 48, w1.double(), w2, 0), (raw, 1, 97, 131, 1040, w1, w2, 0),
                     (raw.view(-1, 2), 1, 97, 131, 48, w1, w2, 0)):
            with pytest.raises(_lib.SprkError):
                torch.ops.sprk.psd_tiles(*args)
        with pytest.raises(_lib.SprkError):
            torch.ops.sprk.psd_tiles(torch.empty(8, dtype=torch.uint8, device="cuda"), 1, 16385, 48, 48, w1, w2, 0)


def test_library_sizes_the_workspace_and_refuses_without_a_gpu():
    from spr_pick_amd import _lib
    L = _lib.lib()
    per_tile = (2 * 48 * 28 + 48 * 25) * 4                       # V [2T, roundup(H, 4)] and Q [T, H]
    assert L.sprk_psd_tiles_ws_bytes(97, 131, 48, 0) == 12 * per_tile
    assert L.sprk_psd_tiles_ws_bytes(97, 131, 48, 5) == 5 * per_tile
    assert L.sprk_psd_tiles_ws_bytes(97, 131, 48, 100) == 12 * per_tile
    # the library's own choice stays near 256 MiB however many tiles there are
    assert L.sprk_psd_tiles_ws_bytes(8192, 8192, 512, 0) <= 256 << 20
    assert L.sprk_psd_tiles_ws_bytes(16384, 16384, 16, 0) <= 256 << 20
    for bad in ((97, 131, 40, 0), (97, 131, 8, 0), (2048, 2048, 1040, 0), (47, 131, 48, 0), (97, 47, 48, 0),
                (16385, 131, 48, 0), (97, 16385, 48, 0), (97, 131, 48, -1)):
        assert L.sprk_psd_tiles_ws_bytes(*bad) == 0
    EINVAL = -1
    assert L.sprk_psd_tiles(None, 1, 97, 131, 48, None, 48, None, 96, 0, None, None, 0, None) == EINVAL
    assert b"null" in L.sprk_last_error()
    assert L.sprk_psd_tiles(None, 4, 97, 131, 48, None, 48, None, 96, 0, None, None, 0, None) == EINVAL
    assert b"mode" in L.sprk_last_error()
    assert L.sprk_psd_tiles(None, 1, 97, 131, 40, None, 48, None, 96, 0, None, None, 0, None) == EINVAL
    assert b"tile" in L.sprk_last_error()
