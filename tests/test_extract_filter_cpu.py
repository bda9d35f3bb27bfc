"""CPU: the CTF-corrected extraction (`joint extract --ctf_correct`) without a GPU: the four matrices and the
filter against their definitions, the four-stage form against ``crop_matrix64`` and against an independent full-plane
``np.fft.fft2`` reference, the float32 model of the device chains within its a-priori bound, the planted cases in float64,
the command line's refusals, and the C entry point's argument checks."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from extract_filter_model import (AC, CS, FLAT, KV, OK, OUTSIDE, PLANTED, apriori_bound, correlation, filter_model,
                                  filter_product, planted, product64)
from extract_model import write_raw_mrc

SHAPES = [(64, 64), (64, 32), (48, 16), (96, 50)]
CTF_ARGS = (2.0, 9000.0, 7000.0, 30.0, KV, CS, AC)              # apix, DefocusU, DefocusV, angle, kV, Cs, ac


def fft_reference(D, S, phi):
    """IDFT_S(Phi . crop(DFT_B(D))) over the full plane: half weights on k = +-h and v = +-h, Phi at (k, v < 0) taken from
    (-k, -v), a direct inverse sum; -> (real part [S, S], largest |imaginary part|)"""
    B, h = D.shape[0], S // 2
    F = np.fft.fft2(D)
    i = np.arange(S)
    acc = np.zeros((S, S), dtype=np.complex128)
    for k in range(-h, h + 1):
        for v in range(-h, h + 1):
            weight = (0.5 if abs(k) == h else 1.0) * (0.5 if abs(v) == h else 1.0)
            f = phi[k + h, v] if v >= 0 else phi[h - k, -v]
            acc += weight * f * F[k % B, v % B] * np.exp(2j * np.pi * (k * i[:, None] + v * i[None, :]) / S)
    return acc.real / B ** 2, float(np.abs(acc.imag).max()) / B ** 2


@pytest.mark.parametrize("B,S", SHAPES + [(16, 16), (66, 34)])
def test_matrices_against_their_definition(B, S):
    from spr_pick_amd import extract, torch_ops
    W1, W2, W3, W4 = extract.filter_matrices64(B, S)
    h, Hs, Ku = S // 2, S // 2 + 1, S + 1
    assert W1.shape == (2 * Hs, B) and W2.shape == (2 * Ku, 2 * B) and W3.shape == (2 * S, 2 * Ku) and W4.shape == (S, 2 * Hs)
    k, v = np.arange(-h, h + 1)[:, None], np.arange(Hs)[:, None]
    c, r, i, j = (np.arange(n)[None, :] for n in (B, B, S, S))
    a = np.where(np.abs(k) == h, 0.5, 1.0)
    w = np.where((v == 0) | (v == h), 1.0, 2.0) / B ** 2
    t1, t2, t3, t4 = 2 * np.pi * v * c / B, 2 * np.pi * k * r / B, 2 * np.pi * k * i / S, 2 * np.pi * v * j / S
    assert np.abs(W1 - np.concatenate([np.cos(t1), np.sin(t1)])).max() < 1e-12
    assert np.abs(W2 - np.block([[np.cos(t2), -np.sin(t2)], [-np.sin(t2), -np.cos(t2)]])).max() < 1e-12
    assert np.abs(W3 - np.block([[(a * np.cos(t3)).T, -(a * np.sin(t3)).T], [(a * np.sin(t3)).T, (a * np.cos(t3)).T]])).max() < 1e-12
    assert np.abs(W4 - np.concatenate([(w * np.cos(t4)).T, -(w * np.sin(t4)).T], axis=1)).max() < 1e-15
    # the reduced phase: the quarter-period entries are exact
    assert W1[1, 0] == 1 and W2[h, :B].tolist() == [1.0] * B and not W2[h, B:].any()
    W32 = extract.filter_matrices(B, S)
    assert all(m32.dtype == np.float32 and np.array_equal(m32, m.astype(np.float32)) for m32, m in zip(W32, (W1, W2, W3, W4)))
    assert extract.filter_matrices(B, S) is W32                                            # cached
    shapes = torch_ops.extract_filter_shapes(B, S)
    assert [s[0] for s in shapes[:4]] == [m.shape[0] for m in W32]
    assert all(s[1] % 4 == 0 and 0 <= s[1] - m.shape[1] < 4 for s, m in zip(shapes[:4], W32)) and shapes[4] == (Ku, Hs)
    for bad in ((63, 32), (64, 31), (64, 14), (64, 66), (1026, 64)):
        with pytest.raises(ValueError, match="even"):
            extract.filter_matrices64(*bad)


@pytest.mark.parametrize("B,S", SHAPES)
def test_four_stages_against_crop_matrix_and_full_plane_fft(B, S):
    from spr_pick_amd import ctf, extract
    W64 = extract.filter_matrices64(B, S)
    D = np.random.RandomState(B + S).randn(B, B)
    M = extract.crop_matrix64(B, S)
    err = np.abs(product64(D, W64, np.ones((S + 1, S // 2 + 1))) - M @ D @ M.T).max()
    assert err < 1e-12, err
    for which in ctf.CORRECTION_MODES:
        phi = ctf.correction_filter(B, S, *CTF_ARGS, which).astype(np.float64)
        ref, imag = fft_reference(D, S, phi)
        err = np.abs(product64(D, W64, phi) - ref).max()
        print("%d -> %d, %s: %.2e from the full-plane reference (its imaginary part %.1e)" % (B, S, which, err, imag))
        assert err < 1e-11 and imag < 1e-11


@pytest.mark.parametrize("B,S", [(64, 64), (96, 50), (66, 34)])
def test_float32_model_within_its_bound(B, S):
    from spr_pick_amd import ctf, extract
    W = extract.filter_matrices(B, S)
    D = (100.0 + 7.0 * np.random.RandomState(B).randn(B, B)).astype(np.float32)
    for which in ctf.CORRECTION_MODES:
        phi = ctf.correction_filter(B, S, *CTF_ARGS, which)
        Y = filter_product(D, W, phi)
        ref, bound = apriori_bound(D, W, phi)
        ratio = float((np.abs(Y - ref) / bound).max())
        print("%d -> %d, %s: the model at %.2e of its a-priori bound" % (B, S, which, ratio))
        assert Y.dtype == np.float32 and 0 < ratio <= 1


def test_filter_values_and_evenness():
    from spr_pick_amd import ctf
    B, S, apix = 96, 50, 1.5
    h = S // 2
    k, v = np.arange(-h, h + 1)[:, None], np.arange(h + 1)[None, :]
    for du, dv, angle in ((12000.0, 12000.0, 0.0), (12000.0, 10000.0, 120.0)):
        mult = ctf.correction_filter(B, S, apix, du, dv, angle, KV, CS, AC, "multiply")
        flip = ctf.correction_filter(B, S, apix, du, dv, angle, KV, CS, AC, "flip")
        assert mult.dtype == flip.dtype == np.float32 and mult.shape == flip.shape == (S + 1, h + 1)
        assert set(np.unique(flip)) == {-1.0, 1.0} and flip[h, 0] == 1 and mult[h, 0] == np.float32(AC)
        assert np.array_equal(flip, np.where(mult >= 0, 1, -1)) or (mult == 0).any()
        # even: the column v = 0 holds both (k, 0) and (-k, 0)
        assert np.array_equal(mult[:, 0], mult[::-1, 0]) and np.array_equal(flip[:, 0], flip[::-1, 0])
        if du == dv:                                                                       # a function of the ring alone
            s = np.sqrt(k * k + v * v) / (B * apix)
            assert np.array_equal(mult, (-ctf.ctf(s, du, KV, CS, AC)).astype(np.float32))
            assert np.array_equal(mult[h - 3, 4], mult[h + 4, 3]) and np.array_equal(mult[h + 5, 0], mult[h, 5])
        else:                                                                              # U along the angle, V across it
            along = ctf.correction_filter(B, S, apix, du, du, 0.0, KV, CS, AC, "multiply")
            across = ctf.correction_filter(B, S, apix, dv, dv, 0.0, KV, CS, AC, "multiply")
            full = ctf.correction_filter(B, B, apix, du, dv, 0.0, KV, CS, AC, "multiply")   # angle 0: U along v (phi = 0)
            assert np.allclose(full[B // 2, 1:], ctf.correction_filter(B, B, apix, du, du, 0.0, KV, CS, AC, "multiply")[B // 2, 1:],
                               atol=1e-6)
            assert np.allclose(full[B // 2 + 1:, 0], ctf.correction_filter(B, B, apix, dv, dv, 0.0, KV, CS, AC, "multiply")[B // 2 + 1:, 0],
                               atol=1e-6)
            assert not np.array_equal(mult, along) and not np.array_equal(mult, across)
    for bad in (dict(mode="wiener"), dict(B=63), dict(S=31), dict(apix=0.0)):
        args = dict(B=64, S=32, apix=1.0, defocus_u=1e4, defocus_v=1e4, angle=0.0, kv=KV, cs=CS, ac=AC, mode="flip")
        args.update(bad)
        with pytest.raises(ValueError):
            ctf.correction_filter(**args)


@pytest.mark.parametrize("B,S,apix,du,dv,angle", PLANTED)
def test_planted_ctf_is_undone(B, S, apix, du, dv, angle):
    """The micrograph is an object seen through -CTF.  Flipping brings the correlation with the (cropped) object from
    nothing to about (2 / pi) sqrt 2 = 0.900; multiplying gives the object filtered by CTF^2."""
    from spr_pick_amd import ctf, extract
    obj, obj2, mic = planted(B, apix, du, dv, angle)
    W64, M = extract.filter_matrices64(B, S), extract.crop_matrix64(B, S)
    want, want2 = M @ obj @ M.T, M @ obj2 @ M.T
    D = mic.astype(np.float64)
    plain = product64(D, W64, np.ones((S + 1, S // 2 + 1)))
    flipped = product64(D, W64, ctf.correction_filter(B, S, apix, du, dv, angle, KV, CS, AC, "flip"))
    multiplied = product64(D, W64, ctf.correction_filter(B, S, apix, du, dv, angle, KV, CS, AC, "multiply"))
    r0, r1, r2 = correlation(plain, want), correlation(flipped, want), correlation(multiplied, want2)
    print("%d -> %d: correlation with the object %.3f uncorrected, %.3f flipped; multiplied against obj * CTF^2 %.4f"
          % (B, S, r0, r1, r2))
    assert r0 < 0.2 and r1 > 0.85 and r2 > 0.99
    if (B, S) == (64, 64):                                     # the angle convention is fit_bins': without it nothing is undone
        mean = product64(D, W64, ctf.correction_filter(B, S, apix, 0.5 * (du + dv), 0.5 * (du + dv), 0.0, KV, CS, AC, "flip"))
        r = correlation(mean, want)
        print("64 -> 64 flipped with the mean defocus and no angle: %.3f" % r)
        assert r < 0.5


def test_model_on_small_boxes():
    from spr_pick_amd import ctf, extract
    rng = np.random.RandomState(1)
    img = rng.randint(-3000, 3000, size=(60, 70)).astype(np.int16)
    W = extract.filter_matrices(16, 16)
    ones = np.ones((17, 9), dtype=np.float32)
    xy = [(20, 20), (7, 20), (62, 52), (63, 52)]
    out, status = filter_model(img, xy, 16, W, ones, normalize=False)
    assert status.tolist() == [OK, OUTSIDE, OK, OUTSIDE] and not out[1].any() and not out[3].any()
    assert np.abs(out[0] - img[12:28, 12:28]).max() < 0.05 and np.abs(out[2] - img[44:60, 54:70]).max() < 0.05
    phi = ctf.correction_filter(16, 16, 1.0, 5000.0, 4000.0, 10.0, KV, CS, AC, "multiply")
    out, _ = filter_model(img, xy[:1], 16, W, phi, normalize=False)
    out_i, _ = filter_model(img, xy[:1], 16, W, phi, normalize=False, invert=True)
    assert np.array_equal(out_i, -out)
    norm, status = filter_model(img, xy[:1], 16, W, phi, 4)
    bg = (np.arange(16)[:, None] - 8) ** 2 + (np.arange(16)[None, :] - 8) ** 2 > 16
    assert status.tolist() == [OK] and abs(norm[0][bg].mean()) < 1e-6 and abs(norm[0][bg].std() - 1) < 1e-6
    assert filter_model(img, xy[:1], 16, W, phi, 16)[1].tolist() == [FLAT]             # no background pixel
    flat = np.full((60, 70), 31000, dtype=np.uint16)
    out, status = filter_model(flat, xy[:1], 16, W, phi, normalize=False)
    assert status.tolist() == [OK] and np.array_equal(out[0], np.full((16, 16), phi[8, 0] * np.float32(31000)))
    assert filter_model(flat, xy[:1], 16, W, phi)[1].tolist() == [FLAT]


def test_operator_is_registered_with_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from spr_pick_amd import _lib, torch_ops
    assert "extract_filter" in torch_ops.registered() and hasattr(torch.ops.sprk, "extract_filter")
    with FakeTensorMode():
        raw = torch.empty(301 * 419 * 2, dtype=torch.uint8, device="cuda")
        xy = torch.empty(40, 2, dtype=torch.int32, device="cuda")
        f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device="cuda")
        shapes = torch_ops.extract_filter_shapes(96, 50)
        assert shapes == ((52, 96), (102, 192), (100, 104), (50, 52), (51, 26))
        W = [f32(*s) for s in shapes]
        out, status = torch.ops.sprk.extract_filter(raw, 1, 301, 419, xy, 96, 50, *W, 7, True, False, 0)
        assert tuple(out.shape) == (40, 50, 50) and out.dtype == torch.float32
        assert tuple(status.shape) == (40,) and status.dtype == torch.int32
        out, status = torch.ops.sprk.extract_filter(raw, 6, 301, 419, xy[:0], 96, 50, *W, 0, False, True, 3)
        assert tuple(out.shape) == (0, 50, 50) and tuple(status.shape) == (0,)
        good = dict(mode=1, xy=xy, box=96, side=50, W=W, R=7, max_batch=0)
        for bad in (dict(side=51), dict(box=95), dict(side=14), dict(box=1026), dict(mode=12), dict(mode=2), dict(R=-1),
                    dict(max_batch=-1), dict(xy=xy.to(torch.int64)), dict(xy=xy.reshape(-1)), dict(side=48),
                    dict(W=W[:4] + [f32(51, 25)]), dict(W=[f32(52, 98)] + W[1:]), dict(W=W[:2] + [W[2].to(torch.float64)] + W[3:])):
            a = dict(good, **bad)
            with pytest.raises(_lib.SprkError):
                torch.ops.sprk.extract_filter(raw, a["mode"], 301, 419, a["xy"], a["box"], a["side"], *a["W"], a["R"], True, False,
                                              a["max_batch"])


def test_cpu_tensors_are_refused():
    from spr_pick_amd import _lib, extract
    header = type("H", (), {"mode": 1, "ny": 32, "nx": 32})
    raw = torch.zeros(2048, dtype=torch.uint8)
    phi = np.ones((17, 9), dtype=np.float32)
    with pytest.raises(_lib.SprkError):
        extract.extract_particles((raw, header), [(16, 16)], 16, ctf_filter=phi)
    with pytest.raises(ValueError, match="bin"):
        extract.extract_particles((raw, header), [(16, 16)], 32, bin=2, ctf_filter=phi)
    with pytest.raises(ValueError, match="even"):
        extract.extract_particles((raw, header), [(16, 16)], 17, ctf_filter=phi)
    with pytest.raises(NotImplementedError):
        z = lambda *s: torch.zeros(*s)
        torch.ops.sprk.extract_filter(raw, 1, 32, 32, torch.zeros(1, 2, dtype=torch.int32), 16, 16, z(18, 16), z(34, 32),
                                      z(32, 36), z(16, 20), z(17, 9), 1, True, False, 0)


def test_c_entry_points_are_declared_exported_and_check_their_arguments():
    from spr_pick_amd import _lib
    text = open(os.path.join(ROOT, "include", "sprk.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+sprk_extract_filter\s*\(", header) and re.search(r"\bsize_t\s+sprk_extract_filter_ws_bytes\s*\(", header)
    assert re.search(r"#define\s+SPRK_ABI_VERSION\s+430\b", text)
    assert {"sprk_extract_filter", "sprk_extract_filter_ws_bytes"} <= set(_lib.EXPORTS) and _lib.ABI_VERSION == 430
    L = _lib.lib()
    assert L.sprk_version() == 430
    A = 0x100000                                               # never dereferenced

    def call(mode=1, ny=301, nx=419, P=4, box=96, side=50, R=7, flags=1, max_batch=0, raw=None, xy=None, w=(None,) * 4,
             phi=None, out=None, status=None, ws=None, ws_bytes=0):
        return L.sprk_extract_filter(raw, mode, ny, nx, xy, P, box, side, *w, phi, R, flags, max_batch, out, status, ws, ws_bytes,
                                     None)

    launches = L.sprk_launch_count()
    for kwargs, word in ((dict(mode=12), b"mode"), (dict(mode=3), b"mode"), (dict(side=49), b"even"), (dict(box=97), b"even"),
                         (dict(side=14), b"side"), (dict(side=98), b"side"), (dict(box=1026, side=64), b"box"),
                         (dict(R=-1), b"radius"), (dict(flags=4), b"flags"), (dict(max_batch=-1), b"max_batch"),
                         (dict(P=-1), b"particles"), (dict(ny=0), b"size"), (dict(ny=65536, nx=32768), b"size")):
        assert call(**kwargs) == -1 and word in L.sprk_last_error(), (kwargs, L.sprk_last_error())
    every = dict(raw=A, xy=A, w=(A,) * 4, phi=A, out=A, status=A, ws=A)
    assert call() == -1 and b"null" in L.sprk_last_error()
    assert call(**dict(every, phi=None)) == -1 and b"null" in L.sprk_last_error()
    assert call(**dict(every, w=(A, A, None, A))) == -1 and b"null" in L.sprk_last_error()
    assert call(**dict(every, raw=A + 2)) == -1 and b"aligned" in L.sprk_last_error()
    assert call(**dict(every, w=(A, A + 4, A, A))) == -1 and b"aligned" in L.sprk_last_error()
    assert call(**dict(every, phi=A + 8)) == -1 and b"aligned" in L.sprk_last_error()
    assert call(**dict(every, ws=A + 4)) == -1 and b"aligned" in L.sprk_last_error()
    need = L.sprk_extract_filter_ws_bytes(4, 96, 50, 0)
    # V [2 * 96, 28], F [2 * 51, 28], Z [50, 52] floats per particle
    assert need == 4 * 4 * (192 * 28 + 102 * 28 + 50 * 52) and L.sprk_extract_filter_ws_bytes(4, 96, 50, 3) == need // 4 * 3
    assert L.sprk_extract_filter_ws_bytes(10 ** 6, 1024, 1024, 0) <= 256 << 20
    assert L.sprk_extract_filter_ws_bytes(4, 96, 51, 0) == 0 and L.sprk_extract_filter_ws_bytes(4, 96, 50, -1) == 0
    assert call(**dict(every, ws_bytes=need - 1)) == -2 and b"workspace" in L.sprk_last_error()
    assert call(**dict(every, ws=None, ws_bytes=need)) == -2
    assert call(P=0) == 0 and call(P=0, box=1024, side=1024, R=10 ** 6, flags=3) == 0
    assert L.sprk_launch_count() == launches


def test_command_line_accepts_and_refuses_ctf_correct():
    from spr_pick_amd import cli
    p = cli.build_parser()
    base = ["extract", "--dataset", "t.txt", "--picks", "dir", "--out", "o"]
    assert vars(p.parse_args(base + ["--box", "255"]))["ctf_correct"] is None
    args = vars(p.parse_args(base + ["--box", "256", "--ctf", "m.star", "--ctf_correct", "flip"]))
    assert (args["ctf_correct"], args["scale"], args["bin"]) == ("flip", None, 1)
    args = vars(p.parse_args(base + ["--box", "256", "--scale", "64", "--ctf", "m.star", "--ctf_correct", "multiply", "--invert"]))
    assert (args["ctf_correct"], args["scale"], args["invert"]) == ("multiply", 64, True)
    assert vars(p.parse_args(base + ["--box", "1024", "--scale", "16", "--ctf", "m.star", "--ctf_correct", "flip"]))["scale"] == 16
    assert "--ctf_phase_flipped" in " ".join(p._subparsers._group_actions[0].choices["extract"].format_help().split())
    for bad in (["--box", "256", "--ctf_correct", "flip"],                                         # no --ctf
                ["--box", "256", "--ctf", "m.star", "--ctf_correct", "wiener"],
                ["--box", "256", "--ctf", "m.star", "--ctf_correct", "flip", "--bin", "2"],
                ["--box", "255", "--ctf", "m.star", "--ctf_correct", "flip"],
                ["--box", "256", "--scale", "63", "--ctf", "m.star", "--ctf_correct", "flip"],
                ["--box", "256", "--scale", "14", "--ctf", "m.star", "--ctf_correct", "flip"],
                ["--box", "14", "--ctf", "m.star", "--ctf_correct", "flip"],
                ["--box", "256", "--scale", "258", "--ctf", "m.star", "--ctf_correct", "flip"],
                ["--box", "256", "--ctf", "m.star", "--ctf_correct", "flip", "--bg_radius", "-1"]):
        with pytest.raises(SystemExit):
            p.parse_args(base + bad)
    # the messages name the rule
    ns = p.parse_args(base + ["--box", "256"])
    ns.ctf_correct, ns.ctf = "flip", None
    with pytest.raises(ValueError, match="--ctf STAR"):
        cli._check_extract(ns)
    ns.ctf, ns.bin = "m.star", 2
    with pytest.raises(ValueError, match="--scale"):
        cli._check_extract(ns)
    ns.bin, ns.box = 1, 255
    with pytest.raises(ValueError, match="even"):
        cli._check_extract(ns)


def test_extract_dataset_host_half_with_ctf_correct(tmp_path, monkeypatch):
    """``extract_dataset`` builds one filter per micrograph from its row of the table (the raw pixel size, not the scaled
    one it writes), and without ``ctf_correct`` the new path is never entered."""
    from spr_pick_amd import ctf, extract, micrograph_io
    rng = np.random.RandomState(3)
    imgs = {"micA": rng.randint(-3000, 3000, size=(70, 90)).astype(np.int16),
            "micB": (100 + 5 * rng.randn(66, 101)).astype(np.float32)}
    params = {"micA": (9000.0, 7000.0, 30.0, 1.2), "micB": (15000.0, 15000.0, 0.0, 0.9)}
    lines, star = ["image_name\tpath"], [ctf.CTF_STAR_HEADER]
    for name, img in imgs.items():
        path = str(tmp_path / (name + ".mrc"))
        write_raw_mrc(path, img)
        lines.append("%s\t%s" % (name, path))
        du, dv, angle, apix = params[name]
        star.append(ctf.star_row(name + ".mrc", du, 0.5, apix, KV, CS, AC, dv, angle))
    table, star_path = str(tmp_path / "raw.txt"), str(tmp_path / "micrographs_ctf.star")
    open(table, "w").write("\n".join(lines) + "\n")
    open(star_path, "w").write("".join(star))
    picks = tmp_path / "picks"
    picks.mkdir()
    rows = {"micA": [(40, 30, 0.9), (4, 30, 0.8), (45, 35, 0.7)], "micB": [(50, 33, 0.95), (60, 30, 0.3), (100, 33, 0.6)]}
    for name, r in rows.items():
        open(str(picks / (name + "_scores_unbinned.txt")), "w").write(
            "image_name\tx_coord\ty_coord\tscore\n" + "".join("%s\t%d\t%d\t%s\n" % (name, x, y, s) for x, y, s in r))
    calls = []

    def by_model(path, xy, box, scale, bg_radius, normalize, invert, device, ctf_filter):
        calls.append((os.path.basename(path), box, scale, bg_radius, ctf_filter))
        with open(path, "rb") as f:
            img, _, _ = micrograph_io.parse_mrc(f.read())
        out, status = filter_model(img, xy, box, extract.filter_matrices(box, scale), ctf_filter, bg_radius, normalize, invert)
        return out[status == OK], status

    def other(*a):
        raise AssertionError("ctf_correct given: only _extract_file_filtered may be called")

    monkeypatch.setattr(extract, "_extract_file_filtered", by_model)
    monkeypatch.setattr(extract, "_extract_file_scaled", other)
    monkeypatch.setattr(extract, "_extract_file", other)
    out_dir = str(tmp_path / "out")
    counts = extract.extract_dataset(table, str(picks), out_dir, 32, threshold=0.5, scale=16, ctf=star_path, ctf_correct="multiply")
    assert counts == {"micA": {"written": 2, "outside": 1, "flat": 0}, "micB": {"written": 1, "outside": 1, "flat": 0}}
    assert [c[:4] for c in calls] == [("micA.mrc", 32, 16, 6), ("micB.mrc", 32, 16, 6)]
    for call, (du, dv, angle, apix) in zip(calls, params.values()):
        assert np.array_equal(call[4], ctf.correction_filter(32, 16, apix, du, dv, angle, KV, CS, AC, "multiply"))
    text = open(os.path.join(out_dir, "particles.star")).read().splitlines()
    data = [line.split("\t") for line in text if line[:1].isdigit()]
    assert len(data) == 3 and [row[12] for row in data] == ["2.40000", "2.40000", "1.80000"]       # apix * 32 / 16
    stack, _, _ = micrograph_io.parse_mrc(open(os.path.join(out_dir, "micA.mrcs"), "rb").read())
    assert stack.shape == (2, 16, 16)
    for kwargs, word in ((dict(ctf_correct="flip"), "micrographs_ctf.star"), (dict(ctf=star_path, ctf_correct="wiener"), "one of"),
                         (dict(ctf=star_path, ctf_correct="flip", bin=2), "bin"),
                         (dict(ctf=star_path, ctf_correct="flip", scale=15), "even")):
        with pytest.raises(ValueError, match=word):
            extract.extract_dataset(table, str(picks), out_dir, 32, **kwargs)
    # without the flag the filtered path is not entered
    monkeypatch.setattr(extract, "_extract_file_filtered", other)
    monkeypatch.setattr(extract, "_extract_file_scaled",
                        lambda path, xy, box, scale, *a: (np.zeros((len(xy), scale, scale), np.float32), np.zeros(len(xy), np.int32)))
    extract.extract_dataset(table, str(picks), str(tmp_path / "plain"), 32, threshold=0.5, scale=16, ctf=star_path)
