"""CPU: dose-weighted movie sums (`joint align --dose`) without a GPU — the four-stage Fourier form against
``align.shift_matrix64`` and np.fft, the exposure filter's properties, the operand layouts, the NumPy models of the two
device contracts (tests/dose_model.py) inside their own a-priori bound, the command line, the registrations and the gain
of the float64 model on the end-to-end movies."""
import numpy as np
import pytest
import torch

import dose_model

# (ny -> by, nx -> bx): odd / even on either side, uncropped and cropped, the shared +-h rows with and without a crop
PAIRS = [((16, 16), (20, 8)), ((17, 17), (21, 9)), ((20, 9), (21, 8)), ((97, 96), (64, 16)), ((20, 20), (17, 9)),
         ((18, 10), (16, 16))]


@pytest.mark.parametrize("rows,cols", PAIRS)
def test_four_stages_with_unit_filter_are_the_shift_matrices(rows, cols):
    from spr_pick_amd import align, dose
    (ny, by), (nx, bx) = rows, cols
    rng = np.random.RandomState(ny + nx)
    Z = 3
    Ds = [rng.randn(ny, nx) for _ in range(Z)]
    shifts = rng.uniform(-4, 4, size=(Z, 2))
    W = dose.spectrum_matrices64(ny, nx, by, bx)
    k, weights = dose.kept_rows(ny, by)
    Ku, Hs = len(k), bx // 2 + 1
    assert Ku == (by + 1 if by % 2 == 0 else by) and (k[0], k[-1]) == (-(by // 2), by // 2)
    assert [m.shape for m in W] == [(2 * Hs, nx), (2 * Ku, 2 * ny), (2 * by, 2 * Ku), (bx, 2 * Hs)]
    Gs = [dose.frame_filter64(1.0, ny, nx, by, bx, dy, dx) for dy, dx in shifts]
    got = dose_model.product64(Ds, W, Gs)
    want = sum(align.shift_matrix64(ny, by, dy) @ D @ align.shift_matrix64(nx, bx, dx).T for D, (dy, dx) in zip(Ds, shifts))
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-11 * max(1.0, scale)
    # and np.fft: fft2 -> phase -> crop -> ifft2, per axis as align_model.fft_shift_crop does it
    import align_model
    fft = 0.0
    for D, (dy, dx) in zip(Ds, shifts):
        half = np.stack([align_model.fft_shift_crop(col, by, dy) for col in D.T], axis=1)        # [by, nx]
        fft = fft + np.stack([align_model.fft_shift_crop(row, bx, dx) for row in half])           # [by, bx]
    assert np.abs(got - fft).max() <= 1e-11 * max(1.0, scale)


def test_kept_rows_and_column_weights():
    from spr_pick_amd import dose
    k, w = dose.kept_rows(20, 8)
    assert k.tolist() == list(range(-4, 5)) and w.tolist() == [0.5] + [1.0] * 7 + [0.5]
    k, w = dose.kept_rows(21, 9)
    assert k.tolist() == list(range(-4, 5)) and w.tolist() == [1.0] * 9
    k, w = dose.kept_rows(16, 16)                                # uncropped and even: the rows +-8 are one frequency, kept twice
    assert len(k) == 17 and w[0] == w[-1] == 0.5
    assert dose.column_weights(8).tolist() == [1, 2, 2, 2, 1] and dose.column_weights(9).tolist() == [1, 2, 2, 2, 2]
    for bad in ((5, 1), (5, 6)):
        with pytest.raises(ValueError):
            dose.kept_rows(*bad)


def test_critical_dose_and_filter_properties():
    from spr_pick_amd import dose
    for q in (0.01, 0.1, 0.25, 0.4):
        assert dose.critical_dose(q, 300.0) == pytest.approx(0.245 * q ** -1.665 + 2.81, rel=1e-14)
        assert dose.critical_dose(q, 200.0) == pytest.approx(0.8 * (0.245 * q ** -1.665 + 2.81), rel=1e-14)
        assert dose.critical_dose(q, 250.0) == pytest.approx(0.9 * (0.245 * q ** -1.665 + 2.81), rel=1e-14)
    assert np.isinf(dose.critical_dose(0.0))
    for kv in (199.9, 300.1, 120.0):
        with pytest.raises(ValueError):
            dose.critical_dose(0.1, kv)
    ny, nx, by, bx, Z = 40, 52, 21, 30, 7
    phi = dose.dose_filter64(ny, nx, by, bx, 1.2, 1.5, 2.0, 300.0, Z)
    k, _ = dose.kept_rows(ny, by)
    assert phi.shape == (Z, len(k), bx // 2 + 1)
    q = dose.frequencies(ny, nx, by, bx, 1.2)
    origin = (by // 2, 0)
    assert q[origin] == 0 and (phi[(slice(None),) + origin] == 1.0).all()          # exactly
    assert np.abs((phi * phi).sum(axis=0) - Z).max() <= 1e-12
    assert (np.diff(phi, axis=0)[:, q > 0] < 0).all()                              # later frames weigh less wherever q > 0
    # the formula itself, at one frequency
    kk, v = 3, 5
    qq = np.hypot(k[kk] / (ny * 1.2), v / (nx * 1.2))
    w = np.exp(-(2.0 + (np.arange(Z) + 1) * 1.5) / (2 * (0.245 * qq ** -1.665 + 2.81)))
    assert np.abs(phi[:, kk, v] - w * np.sqrt(Z / (w * w).sum())).max() <= 1e-14
    # the dose to 0: the plain sum
    assert np.abs(dose.dose_filter64(ny, nx, by, bx, 1.2, 1e-9, 0.0, 300.0, Z) - 1).max() <= 1e-8
    for bad in (dict(dose=0.0), dict(dose=-1.0), dict(pre_dose=-0.1), dict(kv=199.0), dict(kv=301.0), dict(apix=0.0),
                dict(dose=float("nan")), dict(dose="3")):
        with pytest.raises(ValueError):
            dose.check_dose_args(**dict(dict(dose=1.0, pre_dose=0.0, kv=300.0, apix=1.0), **bad))
    assert dose.check_dose_args(2, 1, 200, None) == (2.0, 1.0, 200.0, None)


def test_device_operands_layout_and_values():
    """the float32 operands built with torch (here on the CPU) are the float64 matrices rounded once, padded with zeros"""
    from spr_pick_amd import dose, torch_ops
    ny, nx, by, bx = 37, 45, 12, 17
    W = dose.spectrum_matrices(ny, nx, by, bx, "cpu")
    assert dose.spectrum_matrices(ny, nx, by, bx, "cpu") is W                     # cached
    Ku, Hs = 13, 9
    shapes = torch_ops.align_spectrum_shapes(ny, nx, by, bx, Ku)
    assert shapes == ((18, 48), (26, 76), (24, 28), (17, 20), (26, 12))
    for m, shape, m64 in zip(W, shapes, dose.spectrum_matrices64(ny, nx, by, bx)):
        assert m.dtype == torch.float32 and tuple(m.shape) == shape and m.is_contiguous()
        a = m.numpy()
        assert not a[:, m64.shape[1]:].any()
        ulp = np.spacing(np.abs(m64).astype(np.float32)).astype(np.float64)
        assert (np.abs(a[:, :m64.shape[1]] - m64) <= 0.5 * ulp + 1e-15).all()
    # the blocks: a block size below one matrix gives the same operands
    old, dose._BLOCK = dose._BLOCK, 100
    try:
        dose._matrices.clear()
        for a, b in zip(dose.spectrum_matrices(ny, nx, by, bx, "cpu"), W):
            assert torch.equal(a, b)
    finally:
        dose._BLOCK = old
    # the per-frame filter: torch float64 against NumPy float64, and the layout of g
    Z = 4
    filters = dose.FrameFilters(ny, nx, by, bx, Z, "cpu", apix=1.3, dose=2.0, pre_dose=1.0, kv=250.0)
    phi = dose.dose_filter64(ny, nx, by, bx, 1.3, 2.0, 1.0, 250.0, Z)
    for f, (dy, dx) in enumerate([(0.0, 0.0), (1.25, -3.5), (-7.0, 0.3), (40.0, -50.0)]):
        want = dose.frame_filter64(phi[f], ny, nx, by, bx, dy, dx)
        gr, gi = filters.filter64(f, dy, dx)
        assert np.abs(gr.numpy() - want.real).max() <= 1e-13 and np.abs(gi.numpy() - want.imag).max() <= 1e-13
        g = filters.g(f, dy, dx).numpy()
        assert g.shape == (2 * Ku, 12) and g.dtype == np.float32 and not g[:, Hs:].any()
        assert g[by // 2, 0] == 1.0 and g[Ku + by // 2, 0] == 0.0                  # the origin: exactly 1
    with pytest.raises(ValueError, match="pixel size"):
        dose.FrameFilters(ny, nx, by, bx, Z, "cpu", apix=None, dose=2.0)


BOUND_CASES = [(1, 37, 45, 12, 17, 3), (2, 16, 16, 16, 16, 2)]


@pytest.mark.parametrize("mode,ny,nx,by,bx,Z", BOUND_CASES)
def test_model_lies_inside_its_own_bound(mode, ny, nx, by, bx, Z):
    from spr_pick_amd import dose
    rng = np.random.RandomState(ny)
    frames = [rng.randint(-3000, 3000, size=(ny, nx)).astype(np.int16) if mode == 1
              else (rng.randn(ny, nx) * 100).astype(np.float32) for _ in range(Z)]
    anchor = float(frames[0][0, 0]) if mode == 1 else 0.0
    W = [m.astype(np.float32) for m in dose.spectrum_matrices64(ny, nx, by, bx)]
    phi = dose.dose_filter64(ny, nx, by, bx, 1.5, 3.0, 0.0, 300.0, Z)
    gs = [dose.pack_filter(dose.frame_filter64(phi[f], ny, nx, by, bx, *rng.uniform(-5, 5, 2)))[:, :bx // 2 + 1] for f in range(Z)]
    Y = dose_model.synthesize(dose_model.spectrum(frames, W[0], W[1], gs, anchor), W[2], W[3])
    assert Y.shape == (by, bx) and Y.dtype == np.float32
    ref, bound = dose_model.apriori_bound([dose_model.operand(f, anchor) for f in frames], W, gs)
    ratio = float((np.abs(Y - ref) / bound).max())
    print("%dx%d -> %dx%d, %d frames: worst error / a-priori bound %.3g" % (ny, nx, by, bx, Z, ratio))
    assert ratio < 1
    # constant frames: nothing but the anchor is left, and the spectrum is empty
    const = [np.full((ny, nx), 77, dtype=np.int16)] * Z
    assert not dose_model.spectrum(const, W[0], W[1], gs, 77.0).any()


def test_parser():
    from spr_pick_amd import cli
    p = cli.build_parser()
    base = ["align", "--movies", "m", "--out", "o"]
    a = vars(p.parse_args(base))
    assert (a["dose"], a["pre_dose"], a["kv"], a["apix"]) == (None, None, None, None)
    a = vars(p.parse_args(base + ["--dose", "1.25"]))
    assert (a["dose"], a["pre_dose"], a["kv"], a["apix"]) == (1.25, None, None, None)
    a = vars(p.parse_args(base + ["--dose", "1.25", "--pre_dose", "3", "--kv", "200", "--apix", "0.83"]))
    assert (a["dose"], a["pre_dose"], a["kv"], a["apix"]) == (1.25, 3.0, 200.0, 0.83)
    for bad in (base + ["--pre_dose", "1"], base + ["--kv", "300"], base + ["--apix", "1.0"], base + ["--dose", "0"],
                base + ["--dose", "-2"], base + ["--dose", "x"], base + ["--dose", "1", "--pre_dose", "-1"],
                base + ["--dose", "1", "--kv", "199"], base + ["--dose", "1", "--kv", "301"], base + ["--dose", "1", "--apix", "0"],
                base + ["--dose", "nan"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    text = " ".join(p._subparsers._group_actions[0].choices["align"].format_help().split())
    for word in ("--dose", "--pre_dose", "--kv", "--apix", "dose weighting", "_DW.mrc", "images_DW.txt", "joint ctf", "joint eval",
                 "joint extract", "interpolated", "gain", "local", "TIFF", "EER"):
        assert word in text, word
    not_covered = text[text.index("Not covered"):].split(".")[0]
    assert "dose" not in not_covered


def test_library_refuses_dose_arguments_without_a_dose():
    from spr_pick_amd import align
    for kw in (dict(pre_dose=1.0), dict(kv=200.0), dict(apix=1.0)):
        with pytest.raises(ValueError, match="dose"):
            align.align_dataset("nowhere", "nowhere", **kw)


def test_names_in_header_binding_and_torch_library():
    import os
    import re
    from conftest import ROOT
    from torch._subclasses.fake_tensor import FakeTensorMode
    from spr_pick_amd import _lib, torch_ops
    names = {"sprk_align_spectrum", "sprk_align_spectrum_ws_bytes", "sprk_align_synthesize", "sprk_align_synthesize_ws_bytes"}
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sprk.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(sprk_[a-z0-9_]+)\s*\(", text))
    assert re.search(r"#define SPRK_ABI_VERSION 430\b", text) and _lib.ABI_VERSION == 430
    assert names <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names) and L.sprk_version() == 430
    assert {"align_spectrum", "align_synthesize"} <= set(torch_ops.registered())
    assert L.sprk_align_spectrum_ws_bytes(70, 90, 16) == 2 * 70 * 16 * 4
    assert L.sprk_align_spectrum_ws_bytes(37, 45, 9) == 2 * 37 * 12 * 4
    for bad in ((1, 90, 16), (70, 1, 1), (16385, 90, 16), (70, 16385, 16), (70, 90, 0), (70, 90, 47)):
        assert L.sprk_align_spectrum_ws_bytes(*bad) == 0, bad
    assert L.sprk_align_synthesize_ws_bytes(23, 16) == 23 * 32 * 4 and L.sprk_align_synthesize_ws_bytes(12, 9) == 12 * 20 * 4
    for bad in ((1, 16), (16385, 16), (23, 0), (23, 8194)):
        assert L.sprk_align_synthesize_ws_bytes(*bad) == 0, bad
    # refusals come before anything touches the device
    p = 0x1000
    assert L.sprk_align_spectrum(p, 3, 70, 90, 24, 16, p, p, p, 0.0, p, 1, p, 1 << 30, None) == -1 and b"mode" in L.sprk_last_error()
    assert L.sprk_align_spectrum(p, 1, 70, 90, 72, 16, p, p, p, 0.0, p, 1, p, 1 << 30, None) == -1 and b"kept" in L.sprk_last_error()
    assert L.sprk_align_spectrum(p, 1, 70, 90, 24, 47, p, p, p, 0.0, p, 1, p, 1 << 30, None) == -1 and b"kept" in L.sprk_last_error()
    assert L.sprk_align_spectrum(p, 1, 70, 90, 24, 16, p, p, p, 0.5, p, 1, p, 1 << 30, None) == -1 and b"anchor" in L.sprk_last_error()
    assert L.sprk_align_spectrum(p, 1, 70, 90, 24, 16, p, p, None, 0.0, p, 1, p, 1 << 30, None) == -1 and b"null" in L.sprk_last_error()
    assert L.sprk_align_spectrum(p, 1, 70, 90, 24, 16, p, p, p + 4, 0.0, p, 1, p, 1 << 30, None) == -1 and b"aligned" in L.sprk_last_error()
    assert L.sprk_align_spectrum(p, 1, 70, 90, 24, 16, p, p, p, 0.0, p, 1, p, 100, None) == -2 and b"workspace" in L.sprk_last_error()
    assert L.sprk_align_synthesize(p, 25, 16, 23, 31, p, p, p, p, 1 << 30, None) == -1 and b"kept" in L.sprk_last_error()
    assert L.sprk_align_synthesize(p, 24, 17, 23, 31, p, p, p, p, 1 << 30, None) == -1 and b"kept" in L.sprk_last_error()
    assert L.sprk_align_synthesize(None, 24, 16, 23, 31, p, p, p, p, 1 << 30, None) == -1 and b"null" in L.sprk_last_error()
    assert L.sprk_align_synthesize(p, 24, 16, 23, 31, p, p, p + 8, p, 1 << 30, None) == -1 and b"aligned" in L.sprk_last_error()
    assert L.sprk_align_synthesize(p, 24, 16, 23, 31, p, p, p, p, 100, None) == -2 and b"workspace" in L.sprk_last_error()
    with FakeTensorMode():
        ny, nx, by, bx, Ku = 70, 90, 23, 31, 23
        s1, s2, s3, s4, sf = torch_ops.align_spectrum_shapes(ny, nx, by, bx, Ku)
        assert (s1, s2, s3, s4, sf) == ((32, 92), (46, 140), (46, 48), (31, 32), (46, 16))
        e = lambda s: torch.empty(*s, device="cuda")   # noqa: E731
        raw = torch.empty(ny * nx * 2, dtype=torch.uint8, device="cuda")
        w1, w2, w3, w4, g, F = e(s1), e(s2), e(s3), e(s4), e(sf), e(sf)
        assert torch.ops.sprk.align_spectrum(raw, 1, ny, nx, w1, w2, g, 5.0, F, True) is None
        for args in ((raw, 3, ny, nx, w1, w2, g, 0.0, F, True), (raw, 1, ny, nx, w2, w1, g, 0.0, F, True),
                     (raw, 1, ny, nx, w1, w2, e((46, 20)), 0.0, F, True), (raw, 1, ny, nx, w1, w2, g, 0.0, e((44, 16)), True),
                     (raw[:100], 1, ny, nx, w1, w2, g, 0.0, F, True), (raw, 1, ny, nx, e((31, 92)), w2, g, 0.0, F, True),
                     (raw, 1, ny, 20, e((32, 20)), w2, g, 0.0, F, True)):
            with pytest.raises(_lib.SprkError):
                torch.ops.sprk.align_spectrum(*args)
        y = torch.ops.sprk.align_synthesize(F, by, bx, w3, w4)
        assert tuple(y.shape) == (by, bx) and y.dtype == torch.float32
        for args in ((F, by, bx, w4, w3), (F, by, 33, w3, w4), (F, 21, bx, w3, w4), (e((45, 16)), by, bx, w3, w4),
                     (F, 1, bx, w3, w4)):
            with pytest.raises(_lib.SprkError):
                torch.ops.sprk.align_synthesize(*args)


@pytest.fixture(scope="module")
def gains():
    ny, nx = dose_model.MOVIE_SHAPE
    out = []
    for seed, noise in dose_model.MOVIE_CASES:
        movie, spec, drift = dose_model.make_movie(ny, nx, dose_model.MOVIE_FRAMES, seed, noise)
        assert movie.dtype == np.int16 and movie.shape == (dose_model.MOVIE_FRAMES, ny, nx)
        plain, weighted = dose_model.model_gain(movie, spec, drift)
        print("seed %d, noise %.1f x signal: correlation with the specimen, plain %.4f, dose-weighted %.4f" % (seed, noise, plain, weighted))
        out.append((plain, weighted))
    return out


def test_float64_model_gains_on_the_end_to_end_movies(gains):
    for plain, weighted in gains:
        assert weighted > plain > 0


def test_model_sums_agree_with_the_four_stage_form():
    """the np.fft model of the end-to-end test and the matrix form are the same operator (uncropped, both sides even)"""
    from spr_pick_amd import dose
    ny, nx, Z = 16, 24, 3
    movie, _, drift = dose_model.make_movie(ny, nx, Z, 5, 1.0)
    plain, weighted = dose_model.model_sums(movie, drift)
    W = dose.spectrum_matrices64(ny, nx, ny, nx)
    phi = dose.dose_filter64(ny, nx, ny, nx, dose_model.APIX, dose_model.DOSE, 0.0, dose_model.KV, Z)
    Ds = [f.astype(np.float64) for f in movie]
    for want, p in ((plain, np.ones_like(phi)), (weighted, phi)):
        Gs = [dose.frame_filter64(p[f], ny, nx, ny, nx, -drift[f, 1], -drift[f, 0]) for f in range(Z)]
        assert np.abs(dose_model.product64(Ds, W, Gs) - want).max() <= 1e-9 * np.abs(want).max()
