"""GPU: the CTF-corrected extraction (csrc/extractfilter.hip, `joint extract --ctf_correct`) against the NumPy
model of its contract (tests/extract_filter_model.py).

Not-normalised output is compared bit for bit: both sides run the same four float32 fma chains in the same order (the MFMA
is a k-ordered fmaf chain), one float32 multiply by the filter and one fma for the anchor.  Normalised output is held to one
float32 ulp, for the reason tests/test_gpu_extract.py gives.  Every bit-for-bit case is also held to the model's a-priori
bound, which guards against nonsense only (the chains sit at some 1e-5 of it).

Shapes: the two of the contract in every mode; the smallest; every K = 2 mod 4 with one column past a tile (66 -> 34);
three row blocks of stage 2 and 3 with Ku = 67 (130 -> 66); several K chunks and tiles (256 -> 64, 200 -> 200); the
largest box."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from extract_filter_model import (AC, CS, FLAT, KV, OK, OUTSIDE, PLANTED, apriori_bound, box_of, correlation, filter_model,
                                  filter_products, operand, planted)
from extract_model import write_raw_mrc
from test_gpu_extract_scale import make_image, ulp_distance, upload

pytestmark = pytest.mark.gpu

MAIN_SHAPES = [(64, 64), (96, 50)]
MORE_SHAPES = [(16, 16), (66, 34), (130, 66), (256, 64), (200, 200), (1024, 96)]
CTF_ARGS = (1.3, 14000.0, 11000.0, 40.0, KV, CS, AC)            # apix, DefocusU, DefocusV, angle, kV, Cs, ac


def device_filter(raw, xy, box, S, phi, bg_radius=None, normalize=True, invert=False, max_batch=0):
    from spr_pick_amd import extract
    out, status = extract.extract_particles(raw, xy, box, 1, bg_radius, normalize, invert, scale=S, ctf_filter=phi,
                                            max_batch=max_batch)
    assert tuple(out.shape) == (len(xy), S, S) and out.dtype == torch.float32 and status.dtype == torch.int32
    return out.cpu().numpy(), status.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(mode, B, S, which="flip"):
    """One image, its centres, the filter and the model's products (the expensive half), shared by the tests of this
    shape: the centres of tests/test_gpu_extract_scale.py — inside centres at both parities of x0 (fewer for the large
    boxes), two corners touching, three outside."""
    from spr_pick_amd import ctf, extract
    ny, nx = (301, 419) if B <= 256 else (1100, 1101)
    img = make_image(mode, ny, nx, seed=B + S)
    rng = np.random.RandomState(B * 7 + S)
    h = B // 2
    inside = 4 if B <= 100 else 2 if B <= 256 else 0                    # besides the corners below
    xs = rng.randint(h, nx - B + h + 1, size=inside)
    if inside:
        xs[1] = xs[0] + 1 if xs[0] + 1 <= nx - B + h else xs[0] - 1      # both parities of x0
    ys = rng.randint(h, ny - B + h + 1, size=inside)
    xy = np.stack([xs, ys], axis=1).reshape(-1, 2).tolist()
    xy[1:1] = [(h - 1, h)]                                              # one sample out on the left
    xy += [(nx - B + h + 1, h), (nx // 2, ny + 5), (nx - B + h, ny - B + h)]   # out, out, a corner touching
    if B <= 256:
        xy += [(h, h)]                                                  # the other corner (the largest box: one box)
    xy = np.array(xy)
    W = extract.filter_matrices(B, S)
    phi = ctf.correction_filter(B, S, *CTF_ARGS, which)
    return dict(img=img, raw=upload(img), xy=xy, W=W, phi=phi, products=filter_products(img, xy, B, W, phi))


def check_bound(c, B, got, status):
    """the a-priori bound for every status-0 box of a not-normalised output -> the worst ratio"""
    worst = 0.0
    for p in np.flatnonzero(status == OK):
        D, anchor = operand(box_of(c["img"], c["xy"][p, 0], c["xy"][p, 1], B))
        ref, bound = apriori_bound(D, c["W"], c["phi"])
        ref = ref + np.float64(c["phi"][c["phi"].shape[0] // 2, 0]) * np.float64(anchor)
        if c["img"].dtype != np.float32:
            bound = bound + 2.0 ** -24 * np.abs(ref)                    # the anchor's fma: half an ulp of the output
        err = np.abs(got[p].astype(np.float64) - ref)
        assert (err <= bound).all(), (p, float((err[bound > 0] / bound[bound > 0]).max()))
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    return worst


def bit_for_bit(c, B, S, least_ok):
    got, status = device_filter(c["raw"], c["xy"], B, S, c["phi"], normalize=False)
    want, want_status = filter_model(c["img"], c["xy"], B, c["W"], c["phi"], normalize=False, products=c["products"])
    assert np.array_equal(status, want_status), (status, want_status)
    assert (status == OK).sum() >= least_ok and (status == OUTSIDE).sum() == 3
    assert not got[status != OK].any()
    worst = check_bound(c, B, got, status)
    dist = ulp_distance(got, want)
    print("%d -> %d: %d of %d pixels differ from the model, largest distance %d ulp; %.2e of the a-priori bound"
          % (B, S, int((dist > 0).sum()), dist.size, int(dist.max()), worst))
    assert np.array_equal(got, want), (int((dist > 0).sum()), int(dist.max()))


@pytest.mark.parametrize("B,S", MAIN_SHAPES)
@pytest.mark.parametrize("mode", [0, 1, 2, 6])
def test_not_normalised_bit_for_bit(mode, B, S):
    bit_for_bit(case(mode, B, S), B, S, 4)


@pytest.mark.parametrize("B,S", MORE_SHAPES)
def test_further_shapes_bit_for_bit(B, S):
    bit_for_bit(case(1, B, S), B, S, 1 if B > 256 else 4)


@pytest.mark.parametrize("B,S", MAIN_SHAPES)
@pytest.mark.parametrize("which", ["flip", "multiply"])
def test_both_filters_bit_for_bit(which, B, S):
    c = case(1, B, S, which)
    assert (np.abs(c["phi"]) == 1).all() == (which == "flip")
    bit_for_bit(c, B, S, 4)


@pytest.mark.parametrize("B,S", MAIN_SHAPES)
@pytest.mark.parametrize("mode", [1, 2])
def test_normalised_within_one_ulp(mode, B, S):
    c = case(mode, B, S)
    for R, invert in ((None, False), (5, True)):
        got, status = device_filter(c["raw"], c["xy"], B, S, c["phi"], R, invert=invert)
        want, want_status = filter_model(c["img"], c["xy"], B, c["W"], c["phi"], R, invert=invert, products=c["products"])
        assert np.array_equal(status, want_status), (status, want_status)
        assert (status == OK).sum() >= 4 and not got[status != OK].any()     # outside boxes: exactly zero
        dist = ulp_distance(got, want)
        print("mode %d, %d -> %d, R %s: %d of %d pixels one ulp from the model, largest distance %d"
              % (mode, B, S, R, int((dist == 1).sum()), dist.size, int(dist.max())))
        assert dist.max() <= 1, (int(dist.max()), np.unravel_index(dist.argmax(), dist.shape))
        bg = (np.arange(S)[:, None] - S // 2) ** 2 + (np.arange(S)[None, :] - S // 2) ** 2 > (3 * S // 8 if R is None else R) ** 2
        ok = got[status == OK][:, bg].astype(np.float64)
        assert np.abs(ok.mean(axis=1)).max() < 1e-6 and np.abs(ok.std(axis=1) - 1).max() < 1e-6


def test_degenerate_boxes():
    from spr_pick_amd import ctf
    flat = np.full((120, 130), 31000, dtype=np.uint16)
    raw = upload(flat)
    phi = ctf.correction_filter(64, 32, *CTF_ARGS, "multiply")
    out, status = device_filter(raw, [(60, 60), (61, 57)], 64, 32, phi)
    assert status.tolist() == [FLAT, FLAT] and not out.any()                      # D = 0: Y = 0, no variance
    out, status = device_filter(raw, [(60, 60)], 64, 32, phi, normalize=False)
    want = np.float32(phi[16, 0]) * np.float32(31000)                              # fma(phi0, anchor, 0): one rounding
    assert status.tolist() == [OK] and np.array_equal(out[0], np.full((32, 32), want, dtype=np.float32))
    c = case(1, 96, 50)
    for R in (50, 10 ** 6):                                                       # no background pixel
        out, status = device_filter(c["raw"], c["xy"], 96, 50, c["phi"], R)
        assert set(status.tolist()) == {OUTSIDE, FLAT} and not out.any()
        assert np.array_equal(status, filter_model(c["img"], c["xy"], 96, c["W"], c["phi"], R, products=c["products"])[1])


def test_far_centres_and_determinism():
    from spr_pick_amd import _lib, extract, torch_ops
    c = case(1, 64, 64)
    far = [(10 ** 6, 100), (100, -10 ** 6), (2 ** 31 - 1, 100), (100, -2 ** 31), (-2 ** 31, 2 ** 31 - 1)]
    xy = np.concatenate([c["xy"], np.array(far, dtype=np.int64)])
    for normalize in (True, False):
        plain, status = device_filter(c["raw"], xy, 64, 64, c["phi"], normalize=normalize)
        inverted, status_i = device_filter(c["raw"], xy, 64, 64, c["phi"], normalize=normalize, invert=True)
        assert np.array_equal(status, status_i) and status[-5:].tolist() == [OUTSIDE] * 5
        assert np.array_equal(inverted, -plain)
        assert (np.abs(plain[status == OK]).max(axis=(1, 2)) > 0).all() and not plain[status != OK].any()
    # the same call twice gives the same bytes; 300 particles in one call equal the same particles seven at a time, and
    # with one particle per batch; a workspace full of NaNs is harmless
    rng = np.random.RandomState(9)
    many = torch.from_numpy(rng.randint(0, 301, size=(300, 2)).astype(np.int32)).cuda()
    run = lambda xy, **kw: extract.extract_particles(c["raw"], xy, 64, ctf_filter=c["phi"], **kw)
    out, status = run(many)
    again, status2 = run(many)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)) and torch.equal(status, status2)
    assert int((status == OK).sum()) > 50 and int((status == OUTSIDE).sum()) > 50
    parts = [run(many[k:k + 7]) for k in range(0, 300, 7)]
    assert torch.equal(out.view(torch.int32), torch.cat([p[0] for p in parts]).view(torch.int32))
    assert torch.equal(status, torch.cat([p[1] for p in parts]))
    single, status1 = run(many, max_batch=1)
    assert torch.equal(out.view(torch.int32), single.view(torch.int32)) and torch.equal(status, status1)
    L = _lib.lib()
    raw, header = c["raw"]
    need = L.sprk_extract_filter_ws_bytes(300, 64, 64, 16)
    assert need == 16 * L.sprk_extract_filter_ws_bytes(1, 64, 64, 0) > 0
    ws = torch.full((need // 4,), float("nan"), device="cuda")
    W = extract.filter_matrices(64, 64, raw.device)
    phi = torch.from_numpy(c["phi"]).cuda()
    got, got_status = torch.full_like(out, float("nan")), torch.full_like(status, -1)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    args = [ptr(raw), header.mode, header.ny, header.nx, ptr(many), 300, 64, 64, *(ptr(w) for w in W), ptr(phi), 24,
            torch_ops.EXTRACT_NORMALIZE, 16, ptr(got), ptr(got_status)]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.sprk_extract_filter(*args, ptr(ws), need, stream) == 0, L.sprk_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), got.view(torch.int32)) and torch.equal(status, got_status)
    assert L.sprk_extract_filter(*args, ptr(ws), need - 16, stream) == -2          # SPRK_EWORKSPACE, nothing launched


def test_planted_ctf_is_undone_on_the_device():
    """tests/test_extract_filter_cpu.py's planted cases at 64 -> 64 and 64 -> 32: the flipped output correlates with the
    object at about (2/pi) sqrt 2, the uncorrected one (sprk_extract_scale) does not."""
    from spr_pick_amd import ctf, extract
    for B, S, apix, du, dv, angle in PLANTED[:2]:
        obj, _, mic = planted(B, apix, du, dv, angle)
        M = extract.crop_matrix64(B, S)
        want = M @ obj @ M.T
        raw, xy = upload(mic), [(B // 2, B // 2)]
        plain, status = extract.extract_particles(raw, xy, B, normalize=False, scale=S)
        assert status.tolist() == [OK]
        flipped, status = device_filter(raw, xy, B, S, ctf.correction_filter(B, S, apix, du, dv, angle, KV, CS, AC, "flip"),
                                        normalize=False)
        assert status.tolist() == [OK]
        r0, r1 = correlation(plain.cpu().numpy()[0], want), correlation(flipped[0], want)
        print("%d -> %d: correlation with the object %.3f uncorrected, %.3f flipped" % (B, S, r0, r1))
        assert r0 < 0.2 and r1 > 0.85


def test_joint_extract_ctf_correct_end_to_end(tmp_path):
    """`python -m spr_pick_amd extract --ctf STAR --ctf_correct flip --scale 32` in a fresh process: raw int16, uint16 and
    float32 micrographs, pick tables and a hand-written micrographs_ctf.star in; stacks within one ulp of the model, STAR
    rows and counts equal to it, the pixel size scaled by B / S."""
    from spr_pick_amd import ctf, extract, micrograph_io
    B, S = 48, 32
    imgs = {"micA": make_image(1, 128, 192, seed=10), "micB": make_image(6, 130, 191, seed=11),
            "micC": make_image(2, 128, 192, seed=12)}
    imgs["micB"][20:110, 30:120] = 31000                                                    # a flat patch
    params = {"micA": (9000.0, 7000.0, 30.0, 1.2), "micB": (15000.0, 15000.0, 0.0, 1.2), "micC": (12000.0, 11000.0, 150.0, 0.9)}
    lines, star = ["image_name\tpath"], [ctf.CTF_STAR_HEADER]
    for name, img in imgs.items():
        path = str(tmp_path / (name + ".mrc"))
        write_raw_mrc(path, img, b"0123456789")
        lines.append("%s\t%s" % (name, path))
        du, dv, angle, apix = params[name]
        star.append(ctf.star_row(name + ".mrc", du, 0.5, apix, KV, CS, AC, dv, angle))
    table, star_path = str(tmp_path / "raw.txt"), str(tmp_path / "micrographs_ctf.star")
    open(table, "w").write("\n".join(lines) + "\n")
    open(star_path, "w").write("".join(star))
    picks = tmp_path / "picks"
    picks.mkdir()
    rows = {"micA": [(40, 40, 0.9), (10, 60, 0.8), (96, 64, 0.75), (167, 103, 0.7), (168, 103, 0.65), (100, 12, 0.6), (64, 80, 0.1)],
            "micB": [(150, 50, 0.95), (75, 65, 0.85), (8, 8, 0.8), (160, 100, 0.7), (24, 24, 0.6), (80, 84, 0.05)],
            "micC": [(48, 48, 0.9), (120, 68, 0.2), (125, 73, 0.6)]}
    for name, r in rows.items():
        open(str(picks / (name + "_scores_unbinned.txt")), "w").write(
            "image_name\tx_coord\ty_coord\tscore\n" + "".join("%s\t%d\t%d\t%s\n" % (name, x, y, s) for x, y, s in r))
    out_dir = str(tmp_path / "particles")
    run = subprocess.run([sys.executable, "-m", "spr_pick_amd", "extract", "--dataset", table, "--picks", str(picks),
                          "--box", str(B), "--out", out_dir, "--scale", str(S), "--threshold", "0.5", "--ctf", star_path,
                          "--ctf_correct", "flip"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    summary = json.loads(run.stdout.strip().splitlines()[-1])
    assert summary["ctf_correct"] == "flip"
    counts = summary["micrographs"]
    W = extract.filter_matrices(B, S)
    want_rows, seen = [], set()
    for name, img in imgs.items():
        kept = [(x, y, s) for x, y, s in rows[name] if s > 0.5]
        xy = np.array([(x, y) for x, y, _ in kept])
        du, dv, angle, apix = params[name]
        apix_star = float("%.5f" % apix)                                                     # as the table states it
        phi = ctf.correction_filter(B, S, apix_star * 1e4 / ctf.MAGNIFICATION, du, dv, angle, KV, CS, AC, "flip")
        want, status = filter_model(img, xy, B, W, phi)
        seen |= set(status.tolist())
        assert counts[name] == {"written": int((status == OK).sum()), "outside": int((status == OUTSIDE).sum()),
                                "flat": int((status == FLAT).sum())}
        stack, header, _ = micrograph_io.parse_mrc(open(os.path.join(out_dir, name + ".mrcs"), "rb").read())
        assert header.mode == 2 and stack.shape == (counts[name]["written"], S, S)
        assert ulp_distance(stack, want[status == OK]).max() <= 1
        tail = ctf.star_row(name + ".mrc", du, 0.5, apix * B / S, KV, CS, AC, dv, angle).rstrip("\n").split("\t", 1)[1]
        for k, i in enumerate(np.flatnonzero(status == OK)):
            want_rows.append("%d\t%d\t%06d@%s.mrcs\t%s.mrc\t%s\t%s" % (xy[i, 0], xy[i, 1], k + 1, name, name, kept[i][2], tail))
    assert seen == {OK, OUTSIDE, FLAT} and len(want_rows) >= 6
    text = open(os.path.join(out_dir, "particles.star")).read().splitlines()
    first = text.index("_rlnAutopickFigureOfMerit #5") + len(ctf.CTF_STAR_COLUMNS)
    assert text[first - 1] == "_rlnCtfFigureOfMerit #14" and text[first:] == want_rows
