"""CPU: the parts of the Fourier-crop extraction (`joint extract --scale S`: spr_pick_amd/extract.py, csrc/extract.hip,
DESIGN §4.3d) that need no GPU — the crop matrix against its FFT construction, the NumPy model of the contract
(tests/extract_scale_model.py) with its exact float32 fma and the filter properties that are the reason for the feature,
the operator's registration and fake shapes, the C entry point's argument checking, the command line, and the host half
of ``extract_dataset(..., scale=S)`` with the device call replaced by the model."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import ROOT
from extract_model import write_raw_mrc
from extract_scale_model import (FLAT, OK, OUTSIDE, apriori_bound, crop_product, fma32, model_extract_file_scaled,
                                 scale_model)


def fft_matrix(B, S):
    return np.fft.irfft(np.fft.rfft(np.eye(B), axis=0)[:S // 2 + 1], n=S, axis=0) * S / B


@pytest.mark.parametrize("B,S", [(64, 16), (50, 21), (48, 48), (100, 36), (37, 9), (51, 50), (6, 2), (3, 3)])
def test_crop_matrix(B, S):
    """odd and even S, S = B, B not a multiple of 4"""
    from spr_pick_amd import extract
    M = extract.crop_matrix64(B, S)
    assert M.dtype == np.float64 and M.shape == (S, B)
    assert np.abs(M - fft_matrix(B, S)).max() <= 1e-12
    # the mean passes through.  3e-15 for the shapes it was stated for; elsewhere the a-priori figure: an entry is a sum
    # of h + 1 cosines, each within 2^-52 (argument and cosine), over B, and a row adds B of them with B roundings
    h = S // 2
    tol = 3e-15 if (B, S) in ((64, 16), (50, 21), (48, 48), (100, 36), (37, 9)) else \
        2 * (h + 1) * 2.0 ** -52 + B * 2.0 ** -53 * np.abs(M).sum(axis=1).max()
    assert np.abs(M.sum(axis=1) - 1).max() <= tol
    if S == B:
        assert np.array_equal(M, np.eye(B))
    M32 = extract.crop_matrix(B, S)
    assert M32.dtype == np.float32 and np.array_equal(M32, M.astype(np.float32))
    assert extract.crop_matrix(B, S) is M32                             # cached
    padded = extract.crop_matrix(B, S, "cpu")
    rows, cols = -(-S // 16) * 16, -(-B // 4) * 4
    assert padded.dtype == torch.float32 and tuple(padded.shape) == (rows, cols) and padded.is_contiguous()
    assert np.array_equal(padded[:S, :B].numpy(), M32)
    assert not padded[S:].any() and not padded[:, B:].any()             # exact zeros
    assert extract.crop_matrix(B, S, "cpu") is padded


def test_crop_matrix_refuses_bad_sizes():
    from spr_pick_amd import extract
    for B, S in ((16, 17), (16, 1), (1, 1)):
        with pytest.raises(ValueError):
            extract.crop_matrix64(B, S)
    for box, scale, R in ((16, 17, None), (16, 1, None), (1026, 64, None), (64, 32, -1), (64, 32.0, None)):
        with pytest.raises(ValueError):
            extract.check_scale(box, scale, R)
    assert extract.check_scale(300, 128) == (128, 48) and extract.check_scale(1024, 1024, 0) == (1024, 0)


def exact_fma32(a, b, c):
    """float32(a*b + c), correctly rounded, by rational arithmetic"""
    v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if v == 0:
        return np.float32(0)
    lo = np.float32(float(v))                                           # double rounding may be off by one step: mend it
    cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
    best = min(abs(Fraction(float(x)) - v) for x in cands)
    ties = [x for x in cands if abs(Fraction(float(x)) - v) == best]
    if len(ties) == 1:
        return ties[0]
    return [x for x in ties if (int(np.float32(x).view(np.int32)) & 1) == 0][0]     # a tie goes to the even mantissa


def test_fma32_is_one_rounding():
    """random triples, cancelling triples, and near-ties: c = a float32 midpoint displaced by a product far below the
    float64 sum's last bit — float32(float64(a*b + c)) rounds those twice and gets them wrong"""
    rng = np.random.RandomState(0)
    n = 1500
    a = rng.randn(3 * n).astype(np.float32)
    b = rng.randn(3 * n).astype(np.float32)
    c = rng.randn(3 * n).astype(np.float32)
    c[n:2 * n] = -(a[n:2 * n] * b[n:2 * n])                             # heavy cancellation
    # near-ties: c = 1 + j 2^-23 has the ulp 2^-23, and a*b = +-2^-24 (1 - u^2 2^-46) is 2^-70 short of half of it: the
    # float64 sum (ulp 2^-52) rounds onto the tie, and the second rounding then goes to even instead of towards c
    u = rng.randint(1, 8, size=n).astype(np.float32) * np.float32(2.0 ** -23)
    a[2 * n:] = np.float32(1) + u
    b[2 * n:] = (np.float32(1) - u) * np.float32(2.0 ** -24) * rng.choice([-1, 1], size=n).astype(np.float32)
    c[2 * n:] = np.float32(1) + np.float32(2.0 ** -23) * rng.randint(1, 2 ** 20, size=n).astype(np.float32)
    got = fma32(a, b, c)
    want = np.array([exact_fma32(x, y, z) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert (naive != want).sum() > 0                                    # the cases do tell the two apart


def cosine(B, k0):
    return np.cos(2 * np.pi * k0 * np.arange(B) / B)


@pytest.mark.parametrize("B,S", [(96, 32), (50, 21), (100, 36)])
def test_filter_properties_with_the_float64_matrix(B, S):
    """A cosine with a whole number of cycles per box is reproduced below the new Nyquist frequency and removed above
    it; the block mean leaves a good part of it."""
    from spr_pick_amd import extract
    M = extract.crop_matrix64(B, S)
    for k0 in range(0, (S - 1) // 2 + 1):                               # k0 < S/2
        want = np.cos(2 * np.pi * k0 * np.arange(S) / S)
        assert np.abs(M @ cosine(B, k0) - want).max() <= 1e-13, k0
    for k0 in range(S // 2 + 1, B // 2 + 1):                            # S/2 < k0 <= B/2
        assert np.abs(M @ cosine(B, k0)).max() <= 1e-13, k0
    if B % S == 0:
        N = B // S
        k0 = 20
        assert S / 2 < k0 <= B / 2
        # the block mean's response there is sin(pi k0 N / B) / (N sin(pi k0 / B)) = 0.506; the alias has 12 cycles in 32
        # pixels, eight phases pi/4 apart, so one of its samples is within pi/8 of a crest: 0.506 cos(pi/8) = 0.467
        assert np.abs(cosine(B, k0).reshape(S, N).mean(axis=1)).max() > 0.46
        assert np.abs(M @ cosine(B, k0)).max() <= 1e-13


def test_model_on_small_boxes():
    """S = B: the matrix is the identity and the model returns the box; a constant box stays constant (rows sum to 1)
    up to the rounding of the float32 matrix; outside boxes and flat backgrounds get their status."""
    from spr_pick_amd import extract
    rng = np.random.RandomState(1)
    img = rng.randint(-3000, 3000, size=(40, 50)).astype(np.int16)
    eye = extract.crop_matrix(12, 12)
    out, status = scale_model(img, [(20, 20), (3, 20), (44, 34), (45, 34)], 12, eye, normalize=False)
    assert status.tolist() == [OK, OUTSIDE, OK, OUTSIDE] and not out[1].any() and not out[3].any()
    assert np.array_equal(out[0], img[14:26, 14:26].astype(np.float32))
    assert np.array_equal(out[2], img[28:40, 38:50].astype(np.float32))
    out_i, _ = scale_model(img, [(20, 20)], 12, eye, normalize=False, invert=True)
    assert np.array_equal(out_i[0], -out[0])
    norm, status = scale_model(img, [(20, 20)], 12, eye, 4)
    assert status.tolist() == [OK]
    bg = (np.arange(12)[:, None] - 6) ** 2 + (np.arange(12)[None, :] - 6) ** 2 > 16
    assert abs(norm[0][bg].mean()) < 1e-6 and abs(norm[0][bg].std() - 1) < 1e-6
    assert scale_model(img, [(20, 20)], 12, eye, 12)[1].tolist() == [FLAT]          # no background pixel
    flat = np.full((40, 50), 31000, dtype=np.uint16)
    M = extract.crop_matrix(12, 5)
    out, status = scale_model(flat, [(20, 20)], 12, M, normalize=False)
    assert status.tolist() == [OK] and np.array_equal(out[0], np.full((5, 5), 31000, dtype=np.float32))   # D = 0: the anchor
    assert scale_model(flat, [(20, 20)], 12, M, 1)[1].tolist() == [FLAT]
    fimg = (100 + rng.randn(40, 50)).astype(np.float32)
    Y = crop_product(fimg[14:26, 14:26], M)
    want, bound = apriori_bound(fimg[14:26, 14:26], M)
    assert Y.dtype == np.float32 and (np.abs(Y - want) <= bound).all() and np.abs(Y - want).max() > 0


def test_operator_is_registered_with_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from spr_pick_amd import _lib, torch_ops
    assert "extract_scale" in torch_ops.registered() and hasattr(torch.ops.sprk, "extract_scale")
    with FakeTensorMode():
        raw = torch.empty(301 * 419 * 2, dtype=torch.uint8, device="cuda")
        xy = torch.empty(40, 2, dtype=torch.int32, device="cuda")
        m = torch.empty(32, 52, dtype=torch.float32, device="cuda")                  # 50 -> 21
        out, status = torch.ops.sprk.extract_scale(raw, 1, 301, 419, xy, 50, 21, m, 7, True, False)
        assert tuple(out.shape) == (40, 21, 21) and out.dtype == torch.float32
        assert tuple(status.shape) == (40,) and status.dtype == torch.int32
        out, status = torch.ops.sprk.extract_scale(raw, 6, 301, 419, xy[:0], 50, 21, m, 0, False, True)
        assert tuple(out.shape) == (0, 21, 21) and tuple(status.shape) == (0,)
        # argument checks raise before the library is called
        for bad in ((1, 301, 419, xy, 50, 51, m, 7), (1, 301, 419, xy, 50, 1, m, 0), (1, 301, 419, xy, 1026, 21, m, 0),
                    (12, 301, 419, xy, 50, 21, m, 7), (1, 301, 419, xy, 50, 21, m, -1),
                    (2, 301, 419, xy, 50, 21, m, 7),                                 # float32 needs twice the bytes
                    (1, 301, 419, xy, 50, 21, m[:, :50], 7), (1, 301, 419, xy, 50, 21, m[:21], 7),
                    (1, 301, 419, xy, 50, 21, m.to(torch.float64), 7), (1, 301, 419, xy, 48, 21, m, 7),
                    (1, 301, 419, xy.to(torch.int64), 50, 21, m, 7), (1, 301, 419, xy.reshape(-1), 50, 21, m, 7)):
            with pytest.raises(_lib.SprkError):
                torch.ops.sprk.extract_scale(raw, *bad, True, False)


def test_cpu_tensors_are_refused():
    from spr_pick_amd import _lib, extract
    header = type("H", (), {"mode": 1, "ny": 8, "nx": 8})
    with pytest.raises(_lib.SprkError):
        extract.extract_particles((torch.zeros(128, dtype=torch.uint8), header), [(4, 4)], 4, scale=3)
    with pytest.raises(ValueError):
        extract.extract_particles((torch.zeros(128, dtype=torch.uint8), header), [(4, 4)], 4, bin=2, scale=2)
    with pytest.raises(NotImplementedError):
        torch.ops.sprk.extract_scale(torch.zeros(128, dtype=torch.uint8), 1, 8, 8, torch.zeros(1, 2, dtype=torch.int32),
                                     4, 3, torch.zeros(16, 4), 1, True, False)


def test_c_entry_point_is_declared_exported_and_checks_its_arguments():
    from spr_pick_amd import _lib
    text = open(os.path.join(ROOT, "include", "sprk.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+sprk_extract_scale\s*\(", header)
    assert re.search(r"#define\s+SPRK_ABI_VERSION\s+430\b", text)
    assert "sprk_extract_scale" in _lib.EXPORTS and _lib.ABI_VERSION == 430
    L = _lib.lib()
    assert L.sprk_version() == 430
    A = 0x100000                                               # never dereferenced

    def call(mode=1, ny=301, nx=419, P=4, box=50, side=21, ldm=52, R=7, flags=1, raw=None, xy=None, m=None, out=None,
             status=None):
        return L.sprk_extract_scale(raw, mode, ny, nx, xy, P, box, side, m, ldm, R, flags, out, status, None)

    # null device pointers throughout: each of these is refused for its argument, before a launch
    for kwargs, word in ((dict(mode=12), b"mode"), (dict(mode=3), b"mode"), (dict(side=1), b"side"), (dict(side=51), b"side"),
                         (dict(box=1026, side=64, ldm=1028), b"box"), (dict(box=1, side=1, ldm=4), b"box"),
                         (dict(ldm=48), b"ldm"), (dict(ldm=50), b"ldm"), (dict(ldm=54), b"ldm"), (dict(R=-1), b"radius"),
                         (dict(flags=4), b"flags"), (dict(P=-1), b"particles"), (dict(ny=0), b"size"),
                         (dict(ny=65536, nx=32768), b"size")):
        assert call(**kwargs) == -1 and word in L.sprk_last_error(), (kwargs, L.sprk_last_error())
    launches = L.sprk_launch_count()
    assert call() == -1 and b"null" in L.sprk_last_error()
    assert call(raw=A, xy=A, out=A, status=A) == -1 and b"null" in L.sprk_last_error()          # no matrix
    assert call(raw=A, xy=A, m=A, out=A) == -1 and b"null" in L.sprk_last_error()
    assert call(raw=A + 2, xy=A, m=A, out=A, status=A) == -1 and b"aligned" in L.sprk_last_error()
    assert call(raw=A, xy=A, m=A + 4, out=A, status=A) == -1 and b"aligned" in L.sprk_last_error()
    assert call(P=0) == 0 and call(P=0, box=1024, side=1024, ldm=1024, R=10 ** 6, flags=3) == 0
    assert L.sprk_launch_count() == launches


def test_command_line_accepts_scale():
    from spr_pick_amd import cli
    p = cli.build_parser()
    base = ["extract", "--dataset", "t.txt", "--picks", "dir", "--out", "o"]
    args = vars(p.parse_args(base + ["--box", "256"]))
    assert args["scale"] is None and args["bin"] == 1
    args = vars(p.parse_args(base + ["--box", "300", "--scale", "128"]))
    assert (args["box"], args["scale"], args["bin"], args["bg_radius"]) == (300, 128, 1, None)
    args = vars(p.parse_args(base + ["--box", "300", "--scale", "96", "--bin", "1", "--picks_bin", "8", "--bg_radius", "30",
                                     "--threshold", "0.25", "--invert", "--no_norm"]))
    assert (args["scale"], args["bin"], args["picks_bin"], args["bg_radius"], args["threshold"], args["invert"],
            args["no_norm"]) == (96, 1, 8, 30, 0.25, True, True)
    assert vars(p.parse_args(base + ["--box", "1024", "--scale", "1024"]))["scale"] == 1024
    assert vars(p.parse_args(base + ["--box", "37", "--scale", "2"]))["scale"] == 2
    for bad in (["--box", "300", "--scale", "100", "--bin", "3"], ["--box", "300", "--scale", "75", "--bin", "2"],
                ["--box", "300", "--scale", "1"], ["--box", "300", "--scale", "0"], ["--box", "300", "--scale", "-4"],
                ["--box", "300", "--scale", "301"], ["--box", "300", "--scale", "x"], ["--box", "300", "--scale", "64.5"],
                ["--box", "1026", "--scale", "64"], ["--box", "300", "--scale", "64", "--bg_radius", "-1"]):
        with pytest.raises(SystemExit):
            p.parse_args(base + bad)


def test_extract_dataset_host_half_with_scale(tmp_path, monkeypatch):
    from spr_pick_amd import extract, ingest, micrograph_io
    rng = np.random.RandomState(3)
    imgs = {"micA": rng.randint(-3000, 3000, size=(70, 90)).astype(np.int16),
            "micB": rng.randint(20000, 26000, size=(66, 101)).astype(np.uint16)}
    lines = ["image_name\tpath"]
    for name, img in imgs.items():
        path = str(tmp_path / (name + ".mrc"))
        write_raw_mrc(path, img)
        lines.append("%s\t%s" % (name, path))
    table = str(tmp_path / "raw.txt")
    open(table, "w").write("\n".join(lines) + "\n")
    picks = tmp_path / "picks"
    picks.mkdir()
    rows = {"micA": [(10, 8, 0.9), (1, 8, 0.8), (11, 9, 0.2), (20, 8, 0.7), (12, 5, 0.51)],     # (x, y, score), bin-4 frame
            "micB": [(3, 3, 0.3), (12, 8, 0.95), (13, 13, 0.6), (24, 8, 0.99)]}
    for name, r in rows.items():
        open(str(picks / (name + "_scores.txt")), "w").write(
            "image_name\tx_coord\ty_coord\tscore\n" + "".join("%s\t%d\t%d\t%s\n" % (name, x, y, s) for x, y, s in r))
    calls = []

    def by_model(path, xy, box, scale, bg_radius, normalize, invert, device):
        calls.append((os.path.basename(path), np.array(xy), box, scale, bg_radius, normalize, invert))
        return model_extract_file_scaled(path, xy, box, scale, bg_radius, normalize, invert)

    def unbinned(*a):
        raise AssertionError("scale given: _extract_file must not be called")

    monkeypatch.setattr(extract, "_extract_file_scaled", by_model)
    monkeypatch.setattr(extract, "_extract_file", unbinned)
    out_dir = str(tmp_path / "out")
    counts = extract.extract_dataset(table, str(picks), out_dir, 18, picks_bin=4, threshold=0.5, scale=7)
    assert sorted(counts) == ["micA", "micB"] and [c[0] for c in calls] == ["micA.mrc", "micB.mrc"]
    assert all(c[2:] == (18, 7, 2, True, False) for c in calls)                 # default radius 3 * 7 // 8

    star = open(os.path.join(out_dir, "particles.star")).read()
    head = ("# version 30001\n\ndata_\n\nloop_\n_rlnCoordinateX #1\n_rlnCoordinateY #2\n_rlnImageName #3\n"
            "_rlnMicrographName #4\n_rlnAutopickFigureOfMerit #5\n")
    assert star.startswith(head)
    got_rows = [line.split("\t") for line in star[len(head):].splitlines()]
    want_rows = []
    M = extract.crop_matrix(18, 7)
    for (name, img), call in zip(imgs.items(), calls):
        kept = [(x, y, s) for x, y, s in rows[name] if s > 0.5]
        _, _, oy, ox = ingest.binned_geometry(img.shape[0], img.shape[1], 4)
        xy = np.array([ingest.to_unbinned(x, y, 4, ox, oy) for x, y, _ in kept])
        assert np.array_equal(call[1], xy)                                      # raw-frame coordinates
        want, status = scale_model(img, xy, 18, M, 2)
        assert counts[name] == {"written": int((status == OK).sum()), "outside": int((status == OUTSIDE).sum()),
                                "flat": int((status == FLAT).sum())}
        assert counts[name]["written"] >= 2 and counts[name]["outside"] >= 1
        stack, header, _ = micrograph_io.parse_mrc(open(os.path.join(out_dir, name + ".mrcs"), "rb").read())
        assert header.mode == 2 and (header.nz, header.ny, header.nx) == (counts[name]["written"], 7, 7)
        assert np.array_equal(stack, want[status == OK])
        for k, i in enumerate(np.flatnonzero(status == OK)):
            want_rows.append([str(xy[i, 0]), str(xy[i, 1]), "%06d@%s.mrcs" % (k + 1, name), name + ".mrc", str(kept[i][2])])
    assert got_rows == want_rows and len(want_rows) >= 4

    for kwargs in (dict(scale=19), dict(scale=1), dict(scale=7, bin=2), dict(scale=7, bg_radius=-1)):
        with pytest.raises(ValueError):
            extract.extract_dataset(table, str(picks), out_dir, 18, picks_bin=4, **kwargs)
