"""GPU: the particle extraction (csrc/extract.hip, spr_pick_amd/extract.py) against the NumPy model of its
contract (tests/extract_model.py).  Integer modes and every not-normalised output are compared bit for bit: their sums
are exact integers, and int64 -> double, the double division and the double square root are correctly rounded on both
sides, so both sides round the same double to float32.  float32 normalised output is held to one float32 ulp: the
double sums of the two sides differ in their order of adds, by O(n * 2^-53) relative — nine orders below a float32 ulp —
so only a value that sits on a float32 rounding boundary can move, and by one step."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
from extract_model import DTYPES, FLAT, MODE_OF, OK, OUTSIDE, extract_model, write_raw_mrc

pytestmark = pytest.mark.gpu


def make_image(mode, ny, nx, seed=0):
    rng = np.random.RandomState(seed + 17 * mode)
    if mode == 2:
        return (100.0 + 7.0 * rng.randn(ny, nx)).astype(np.float32)       # mean^2 / var near 200
    if mode == 6:
        return rng.randint(30000, 34000, size=(ny, nx)).astype(np.uint16)  # counts on a large offset
    info = np.iinfo(DTYPES[mode])
    return rng.randint(info.min, info.max + 1, size=(ny, nx)).astype(DTYPES[mode])


def upload(img):
    """-> the (raw, header) pair ingest.read_raw returns for a file holding img"""
    raw = torch.from_numpy(np.frombuffer(img.tobytes(), dtype=np.uint8).copy()).cuda()
    return raw, types.SimpleNamespace(mode=MODE_OF[img.dtype], ny=img.shape[0], nx=img.shape[1])


def device_extract(img, xy, box, bin=1, bg_radius=None, normalize=True, invert=False, raw=None):
    from spr_pick_amd import extract
    out, status = extract.extract_particles(raw or upload(img), xy, box, bin, bg_radius, normalize, invert)
    b = box // bin
    assert tuple(out.shape) == (len(xy), b, b) and out.dtype == torch.float32 and status.dtype == torch.int32
    return out.cpu().numpy(), status.cpu().numpy()


def ulp_distance(a, b):
    """distance of two float32 arrays in representable values"""
    def ordered(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(ordered(a) - ordered(b))


def check(img, xy, box, bin=1, bg_radius=None, normalize=True, invert=False, raw=None):
    """Device against model: status exact; output exact, or within one ulp for normalised float32 data."""
    got, status = device_extract(img, xy, box, bin, bg_radius, normalize, invert, raw)
    want, want_status = extract_model(img, xy, box, bin, bg_radius, normalize, invert)
    assert np.array_equal(status, want_status), (status, want_status)
    assert not got[status != OK].any()                                  # outside and flat boxes: exactly zero
    if img.dtype == np.float32 and normalize:
        dist = ulp_distance(got, want)
        print("float32 normalised: %d of %d pixels one ulp from the model, max distance %d"
              % (int((dist == 1).sum()), dist.size, int(dist.max()) if dist.size else 0))
        assert dist.size == 0 or dist.max() <= 1, (int(dist.max()), np.unravel_index(dist.argmax(), dist.shape))
    else:
        bad = np.argwhere(got != want)
        assert np.array_equal(got, want), (len(bad), bad[:1], got[tuple(bad[0])], want[tuple(bad[0])])
    return got, status


@pytest.mark.parametrize("N", [1, 2, 3, 4])
@pytest.mark.parametrize("mode", [0, 1, 2, 6])
def test_modes_and_bins(mode, N):
    """301 x 419: odd nx makes int16 rows only 2-byte aligned; 40 centres in [-5, n+5): boxes start at odd and even x0
    and some fall outside."""
    ny, nx = 301, 419
    img = make_image(mode, ny, nx)
    rng = np.random.RandomState(7)
    xy = np.stack([rng.randint(-5, nx + 5, size=40), rng.randint(-5, ny + 5, size=40)], axis=1)
    x0 = xy[:, 0] - 6 * N
    _, status = check(img, xy, 12 * N, N, 4)
    assert (status == OK).sum() >= 20 and (status == OUTSIDE).sum() >= 1          # not vacuous either way
    assert len(set(x0[status == OK] % 2)) == 2                                    # odd and even row starts
    check(img, xy, 12 * N, N, 4, normalize=False)


@pytest.mark.parametrize("shape,box,N,centres", [
    ((64, 75), 8, 1, [(4, 4), (37, 31), (70, 59), (71, 60)]),                     # b = 8: 64 pixels, idle lanes
    ((64, 75), 16, 2, [(8, 8), (37, 31), (67, 56)]),
    ((150, 201), 64, 1, [(32, 32), (99, 75), (169, 118)]),                        # b = 64: LDS-resident
    ((300, 419), 128, 1, [(64, 64), (355, 236), (201, 101)]),                     # b = 128: the largest resident box
    ((300, 419), 129, 1, [(64, 64), (354, 235), (201, 101)]),                     # b = 129: the first that is not
    ((300, 419), 256, 1, [(128, 128), (291, 172), (201, 150)]),                   # b = 256: re-read from global memory
    ((150, 201), 64, 16, [(32, 32), (99, 75), (169, 118)]),                       # N = 16, b = 4
    ((300, 419), 288, 2, [(144, 144), (275, 156), (201, 150)]),                   # b = 144 with N = 2: not resident
])
def test_lane_and_residency_regimes(shape, box, N, centres):
    img = make_image(6, *shape, seed=2)
    raw = upload(img)
    _, status = check(img, centres, box, N, raw=raw)
    assert (status == OK).all()
    check(img, centres, box, N, 0, raw=raw)
    check(img, centres, box, N, normalize=False, raw=raw)


@pytest.mark.parametrize("mode,N", [(1, 1), (6, 2), (2, 1), (0, 3)])
def test_borders(mode, N):
    ny, nx, B = 61, 83, 6 * N
    h = B // 2
    img = make_image(mode, ny, nx, seed=4)
    touching = [(h, 30), (30, h), (nx - B + h, 30), (30, ny - B + h), (h, h), (nx - B + h, ny - B + h)]
    one_out = [(h - 1, 30), (30, h - 1), (nx - B + h + 1, 30), (30, ny - B + h + 1)]
    far = [(10 ** 6, 30), (30, -10 ** 6), (-10 ** 6, 10 ** 6), (2 ** 31 - 1, 30), (30, -2 ** 31), (-2 ** 31, 2 ** 31 - 1)]
    for normalize in (True, False):
        _, status = check(img, touching + one_out + far, B, N, 1, normalize=normalize)
        assert status.tolist() == [OK] * 6 + [OUTSIDE] * 10


@pytest.mark.parametrize("mode", [1, 2, 6])
def test_degenerate_boxes(mode):
    dtype = DTYPES[mode]
    flat = np.full((40, 50), 37, dtype=dtype)
    _, status = check(flat, [(20, 20), (25, 17)], 16, 2)
    assert status.tolist() == [FLAT, FLAT]                                        # a constant image
    img = make_image(mode, 40, 50, seed=5)
    _, status = check(img, [(20, 20), (25, 17)], 16, 2, 8)                        # R = b: no background pixel
    assert status.tolist() == [FLAT, FLAT]
    _, status = check(img, [(20, 20)], 16, 2, 10 ** 6)
    assert status.tolist() == [FLAT]
    # constant except inside the radius: the box at (20, 20) starts at sample 12, the one at (21, 20) at column 13, so
    # samples 18 .. 22 are at most 3 and 2 pixels from the centre pixel 8: 13 <= R^2 = 16
    inner = flat.copy()
    inner[18:23, 18:23] = img[18:23, 18:23]
    _, status = check(inner, [(20, 20), (21, 20)], 16, 1, 4)
    assert status.tolist() == [FLAT, FLAT]
    _, status = check(inner, [(20, 20)], 16, 1, 2)                                # a smaller radius sees the samples
    assert status.tolist() == [OK]
    _, status = check(flat, [(20, 20)], 16, 2, normalize=False)                   # no statistics, nothing degenerate
    assert status.tolist() == [OK]


@pytest.mark.parametrize("mode", [1, 2])
def test_invert_is_the_exact_negation(mode):
    img = make_image(mode, 64, 75, seed=6)
    raw = upload(img)
    xy = [(20, 20), (41, 33), (3, 3)]
    for normalize in (True, False):
        plain, status = device_extract(img, xy, 16, 2, normalize=normalize, raw=raw)
        inverted, status_i = device_extract(img, xy, 16, 2, normalize=normalize, invert=True, raw=raw)
        assert status.tolist() == status_i.tolist() == [OK, OK, OUTSIDE]
        assert np.array_equal(inverted, -plain) and np.abs(plain[:2]).max() > 0
    check(img, xy, 16, 2, invert=True, raw=raw)


def test_determinism_and_a_grid_larger_than_the_machine():
    """float32, whose sums depend on their order: the same call twice gives the same bytes, and 3000 particles in one
    launch equal the same particles extracted seven at a time."""
    img = make_image(2, 128, 128, seed=8)
    raw = upload(img)
    rng = np.random.RandomState(9)
    xy = torch.from_numpy(rng.randint(0, 128, size=(3000, 2)).astype(np.int32)).cuda()
    from spr_pick_amd import extract
    out, status = extract.extract_particles(raw, xy, 16, 2)
    again, status2 = extract.extract_particles(raw, xy, 16, 2)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)) and torch.equal(status, status2)
    assert int((status == OK).sum()) > 1500 and int((status == OUTSIDE).sum()) > 100
    parts = [extract.extract_particles(raw, xy[k:k + 7], 16, 2) for k in range(0, 3000, 7)]
    assert torch.equal(out.view(torch.int32), torch.cat([p[0] for p in parts]).view(torch.int32))
    assert torch.equal(status, torch.cat([p[1] for p in parts]))
    check(img, xy[:64].cpu().numpy(), 16, 2, raw=raw)


def test_joint_extract_end_to_end(tmp_path):
    """`python -m spr_pick_amd extract` in a fresh process: raw int16 and uint16 micrographs plus pick tables in the
    bin-4 frame in, stacks, STAR table and counts out, all equal to the model."""
    from spr_pick_amd import ingest, micrograph_io
    imgs = {"micA": make_image(1, 256, 384, seed=10), "micB": make_image(6, 258, 383, seed=11)}   # micB: offsets (1, 1)
    imgs["micB"][96:144, 96:144] = 31000                                                    # a flat patch
    lines = ["image_name\tpath"]
    for name, img in imgs.items():
        path = str(tmp_path / (name + ".mrc"))
        write_raw_mrc(path, img, b"0123456789")
        lines.append("%s\t%s" % (name, path))
    table = str(tmp_path / "raw.txt")
    open(table, "w").write("\n".join(lines) + "\n")
    picks = tmp_path / "picks"
    picks.mkdir()
    rows = {"micA": [(20, 20, 0.9), (3, 30, 0.8), (48, 31, 0.75), (92, 59, 0.7), (93, 30, 0.65), (50, 5, 0.6), (33, 41, 0.1)],
            "micB": [(29, 29, 0.95), (60, 40, 0.85), (4, 4, 0.8), (70, 60, 0.7), (95, 10, 0.6), (40, 41, 0.05),
                     (50, 20, 0.55)]}
    for name, r in rows.items():
        open(str(picks / (name + "_scores.txt")), "w").write(
            "image_name\tx_coord\ty_coord\tscore\n" + "".join("%s\t%d\t%d\t%s\n" % (name, x, y, s) for x, y, s in r))
    out_dir = str(tmp_path / "particles")
    run = subprocess.run([sys.executable, "-m", "spr_pick_amd", "extract", "--dataset", table, "--picks", str(picks),
                          "--box", "32", "--out", out_dir, "--picks_bin", "4", "--bin", "2", "--threshold", "0.5"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    counts = json.loads(run.stdout.strip().splitlines()[-1])["micrographs"]
    want_rows, seen = [], set()
    for name, img in imgs.items():
        kept = [(x, y, s) for x, y, s in rows[name] if s > 0.5]
        _, _, oy, ox = ingest.binned_geometry(img.shape[0], img.shape[1], 4)
        xy = np.array([ingest.to_unbinned(x, y, 4, ox, oy) for x, y, _ in kept])
        want, status = extract_model(img, xy, 32, 2)
        seen |= set(status.tolist())
        assert counts[name] == {"written": int((status == OK).sum()), "outside": int((status == OUTSIDE).sum()),
                                "flat": int((status == FLAT).sum())}
        stack, header, _ = micrograph_io.parse_mrc(open(os.path.join(out_dir, name + ".mrcs"), "rb").read())
        assert header.mode == 2 and stack.shape == (counts[name]["written"], 16, 16)
        assert np.array_equal(stack, want[status == OK])
        for k, i in enumerate(np.flatnonzero(status == OK)):
            want_rows.append("%d\t%d\t%06d@%s.mrcs\t%s.mrc\t%s" % (xy[i, 0], xy[i, 1], k + 1, name, name, kept[i][2]))
    assert seen == {OK, OUTSIDE, FLAT} and len(want_rows) >= 6
    star = open(os.path.join(out_dir, "particles.star")).read().splitlines()
    assert star[:9] == ["# version 30001", "", "data_", "", "loop_", "_rlnCoordinateX #1", "_rlnCoordinateY #2",
                        "_rlnImageName #3", "_rlnMicrographName #4"] and star[9] == "_rlnAutopickFigureOfMerit #5"
    assert star[10:] == want_rows
