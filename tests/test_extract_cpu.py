"""CPU: the parts of the particle extraction (spr_pick_amd/extract.py, csrc/extract.hip) that need no GPU
— the operator's registration and fake shapes, the C entry point's argument checking, the NumPy model of the contract
(tests/extract_model.py) against hand-computed boxes, the command line, and the host half of ``extract_dataset`` with
the device call replaced by the model."""
import logging
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from extract_model import FLAT, OK, OUTSIDE, extract_model, model_extract_file, write_raw_mrc


def test_operator_is_registered_with_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from spr_pick_amd import _lib, torch_ops
    assert "extract_boxes" in torch_ops.registered() and hasattr(torch.ops.sprk, "extract_boxes")
    with FakeTensorMode():
        raw = torch.empty(301 * 419 * 2, dtype=torch.uint8, device="cuda")
        xy = torch.empty(40, 2, dtype=torch.int32, device="cuda")
        out, status = torch.ops.sprk.extract_boxes(raw, 1, 301, 419, xy, 48, 4, 4, True, False)
        assert tuple(out.shape) == (40, 12, 12) and out.dtype == torch.float32
        assert tuple(status.shape) == (40,) and status.dtype == torch.int32
        out, status = torch.ops.sprk.extract_boxes(raw, 6, 301, 419, xy[:0], 256, 1, 0, False, True)
        assert tuple(out.shape) == (0, 256, 256) and tuple(status.shape) == (0,)
        # argument checks raise before the library is called
        for bad in ((1, 301, 419, xy, 50, 4, 4), (1, 301, 419, xy, 1, 1, 0), (1, 301, 419, xy, 1026, 1, 0),
                    (12, 301, 419, xy, 48, 4, 4), (1, 301, 419, xy, 48, 4, -1), (1, 301, 419, xy, 48, 17, 4),
                    (2, 301, 419, xy, 48, 4, 4),                               # float32 needs twice the bytes
                    (1, 301, 419, xy.to(torch.int64), 48, 4, 4), (1, 301, 419, xy.reshape(-1), 48, 4, 4)):
            with pytest.raises(_lib.SprkError):
                torch.ops.sprk.extract_boxes(raw, *bad, True, False)


def test_cpu_tensors_are_refused():
    from spr_pick_amd import _lib, extract
    header = type("H", (), {"mode": 1, "ny": 8, "nx": 8})
    with pytest.raises(_lib.SprkError):
        extract.extract_particles((torch.zeros(128, dtype=torch.uint8), header), [(4, 4)], 4)
    with pytest.raises(NotImplementedError):
        torch.ops.sprk.extract_boxes(torch.zeros(128, dtype=torch.uint8), 1, 8, 8, torch.zeros(1, 2, dtype=torch.int32),
                                     4, 1, 1, True, False)


def test_c_entry_point_is_declared_exported_and_checks_its_arguments():
    from spr_pick_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sprk.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+sprk_extract_boxes\s*\(", header)
    assert "sprk_extract_boxes" in _lib.EXPORTS and _lib.ABI_VERSION == 430
    L = _lib.lib()
    NORM = 1

    def call(mode=1, P=4, box=48, bin=4, R=4, flags=NORM, raw=None, xy=None, out=None, status=None):
        return L.sprk_extract_boxes(raw, mode, 301, 419, xy, P, box, bin, R, flags, out, status, None)

    # null device pointers throughout: each of these is refused for its argument, before a launch
    for kwargs, word in ((dict(box=50, bin=4), b"box"), (dict(box=1, bin=1), b"box"), (dict(box=1026, bin=1), b"box"),
                         (dict(box=2, bin=2), b"box"), (dict(mode=12), b"mode"), (dict(mode=3), b"mode"),
                         (dict(R=-1), b"radius"), (dict(bin=0), b"bin"), (dict(bin=17, box=34), b"bin"),
                         (dict(flags=4), b"flags"), (dict(P=-1), b"particles")):
        assert call(**kwargs) == -1 and word in L.sprk_last_error(), (kwargs, L.sprk_last_error())
    launches = L.sprk_launch_count()
    assert call() == -1 and b"null" in L.sprk_last_error()
    A = 0x100000                                               # never dereferenced
    assert call(raw=A, xy=A, out=A) == -1 and b"null" in L.sprk_last_error()
    assert call(raw=A + 2, xy=A, out=A, status=A) == -1 and b"aligned" in L.sprk_last_error()
    assert call(P=0) == 0 and call(P=0, box=1024, bin=16, R=10 ** 6, flags=3) == 0
    assert L.sprk_launch_count() == launches


# 4 x 4 output, R = 2: the background is (0,0), (0,1), (0,3), (1,0), (3,0) — the pixels with (i-2)^2 + (j-2)^2 > 4
V4 = np.array([[100, 100, 90, 100],
               [100, 120, 130, 110],
               [95, 140, 150, 125],
               [105, 115, 135, 99]])


def test_model_against_hand_computed_boxes():
    # integer: d = v - 100, background d = {0, 0, 0, 0, 5}: mean 1, var 25/5 - 1 = 4 -> out = (v - 101) / 2
    # float32: background v = {100 x 4, 105}: mean 101, var (4*1 + 16)/5 = 4 -> the same
    want = ((V4 - 101) / 2).astype(np.float32)
    for dtype, shift in ((np.int16, 0), (np.uint16, 0), (np.int8, -100), (np.float32, 0)):   # int8: -10 .. 50
        img = np.full((9, 11), 7, dtype=dtype)
        img[3:7, 2:6] = V4 + shift                                 # x0 = 2, y0 = 3 -> centre (4, 5)
        out, status = extract_model(img, [(4, 5)], 4, 1, 2)
        assert status.tolist() == [OK] and out.dtype == np.float32 and np.array_equal(out[0], want), dtype
        out, _ = extract_model(img, [(4, 5)], 4, 1, 2, invert=True)
        assert np.array_equal(out[0], -want)
        out, status = extract_model(img, [(4, 5)], 4, 1, 2, normalize=False)
        assert status.tolist() == [OK] and np.array_equal(out[0], (V4 + shift).astype(np.float32))
    # bin 2: every block holds its value in one sample (the not-normalised output is the block MEAN)
    img = np.zeros((20, 20), dtype=np.uint16)
    img[4:12:2, 6:14:2] = V4 * 100                                 # x0 = 6, y0 = 4, B = 8 -> centre (10, 8)
    out, status = extract_model(img, [(10, 8)], 8, 2, 2)
    assert status.tolist() == [OK] and np.array_equal(out[0], ((V4 * 100 - 10100) / 200).astype(np.float32))
    out, _ = extract_model(img, [(10, 8)], 8, 2, 2, normalize=False)
    assert np.array_equal(out[0], (V4 * 25).astype(np.float32))
    # uint16 on a large offset: the anchor keeps the one-pass variance exact
    img = np.full((9, 11), 65000, dtype=np.uint16)
    img[3:7, 2:6] = V4 + 65000
    assert np.array_equal(extract_model(img, [(4, 5)], 4, 1, 2)[0][0], want)


def test_model_degenerate_and_outside_boxes():
    img = np.arange(10 * 12, dtype=np.int16).reshape(10, 12)
    flat = np.full((10, 12), 3, dtype=np.int16)
    zeros = np.zeros((4, 4), dtype=np.float32)
    out, status = extract_model(flat, [(5, 5)], 4, 1, 1)
    assert status.tolist() == [FLAT] and np.array_equal(out[0], zeros)                 # a flat box
    for R in (4, 5, 100):                                                              # R >= b: no background
        out, status = extract_model(img, [(5, 5)], 4, 1, R)
        assert status.tolist() == [FLAT] and np.array_equal(out[0], zeros)
    assert extract_model(img, [(5, 5)], 4, 1, 2)[1].tolist() == [OK]
    # x0 = x - 2: x = 2 touches the left border, x = 10 the right one (x0 + 4 = 12); y likewise with ny = 10
    inside = [(2, 5), (10, 5), (5, 2), (5, 8), (2, 2), (10, 8)]
    outside = [(1, 5), (11, 5), (5, 1), (5, 9)]                                        # one sample out on each side
    out, status = extract_model(img, inside + outside, 4, 1, 1)
    assert status.tolist() == [OK] * 6 + [OUTSIDE] * 4
    assert all(np.array_equal(o, zeros) for o in out[6:]) and all(np.abs(o).max() > 0 for o in out[:6])
    out, status = extract_model(img, outside, 4, 1, 1, normalize=False)
    assert status.tolist() == [OUTSIDE] * 4 and not out.any()
    assert np.array_equal(extract_model(img, [(2, 2)], 4, 1, 1, normalize=False)[0][0], img[0:4, 0:4].astype(np.float32))


def test_command_line_accepts_extract():
    from spr_pick_amd import cli
    p = cli.build_parser()
    base = ["extract", "--dataset", "t.txt", "--picks", "dir", "--out", "o"]
    args = vars(p.parse_args(base + ["--box", "256"]))
    assert (args["command"], args["dataset"], args["picks"], args["out"], args["box"]) == ("extract", "t.txt", "dir", "o", 256)
    assert (args["bin"], args["picks_bin"], args["bg_radius"], args["threshold"], args["invert"], args["no_norm"]) == \
        (1, 1, None, None, False, False)
    args = vars(p.parse_args(base + ["--box", "96", "--bin", "3", "--picks_bin", "8", "--bg_radius", "10", "--threshold", "0.25",
                                     "--invert", "--no_norm"]))
    assert (args["box"], args["bin"], args["picks_bin"], args["bg_radius"], args["threshold"], args["invert"],
            args["no_norm"]) == (96, 3, 8, 10, 0.25, True, True)
    assert vars(p.parse_args(base + ["--box", "1024", "--bin", "16"]))["box"] == 1024
    for bad in (["--box", "100", "--bin", "3"], ["--box", "1"], ["--box", "1026"], ["--box", "x"], ["--box", "2", "--bin", "2"],
                ["--box", "64", "--bin", "0"], ["--box", "64", "--bin", "17"], ["--box", "64", "--picks_bin", "17"],
                ["--box", "64", "--bg_radius", "-1"], []):
        with pytest.raises(SystemExit):
            p.parse_args(base + bad)
    with pytest.raises(SystemExit):
        p.parse_args(["extract", "--dataset", "t.txt", "--box", "64", "--out", "o"])        # --picks is required


def _dataset(tmp_path):
    """Three raw micrographs (mode 1, mode 6, and one that gets no pick table), pick tables in a bin-4 frame."""
    rng = np.random.RandomState(3)
    imgs = {"micA": rng.randint(-3000, 3000, size=(70, 90)).astype(np.int16),
            "micB": rng.randint(20000, 26000, size=(66, 101)).astype(np.uint16),     # 66 % 4, 101 % 4: offsets 1 and 0
            "micC": rng.randint(0, 100, size=(70, 90)).astype(np.int16)}
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
    return imgs, table, str(picks), rows


def test_extract_dataset_host_half(tmp_path, monkeypatch, caplog):
    from spr_pick_amd import extract, ingest, micrograph_io
    imgs, table, picks, rows = _dataset(tmp_path)
    calls = []

    def by_model(path, xy, box, bin, bg_radius, normalize, invert, device):
        calls.append((os.path.basename(path), np.array(xy), box, bin, bg_radius, normalize, invert))
        return model_extract_file(path, xy, box, bin, bg_radius, normalize, invert)

    monkeypatch.setattr(extract, "_extract_file", by_model)
    out_dir = str(tmp_path / "out")
    with caplog.at_level(logging.WARNING, logger="joint.extract"):
        counts = extract.extract_dataset(table, picks, out_dir, 16, bin=2, picks_bin=4, threshold=0.5)
    assert "micC" in caplog.text and "micA" not in caplog.text                  # the skipped micrograph is named
    assert sorted(counts) == ["micA", "micB"]
    assert [c[0] for c in calls] == ["micA.mrc", "micB.mrc"]                    # one device call per micrograph
    assert all(c[2:] == (16, 2, 3, True, False) for c in calls)                 # default radius 3 * 8 // 8

    star = open(os.path.join(out_dir, "particles.star")).read()
    head = ("# version 30001\n\ndata_\n\nloop_\n_rlnCoordinateX #1\n_rlnCoordinateY #2\n_rlnImageName #3\n"
            "_rlnMicrographName #4\n_rlnAutopickFigureOfMerit #5\n")
    assert star.startswith(head)
    got_rows = [line.split("\t") for line in star[len(head):].splitlines()]
    want_rows = []
    for (name, img), call in zip(list(imgs.items())[:2], calls):
        kept = [(x, y, s) for x, y, s in rows[name] if s > 0.5]                 # the threshold filter, pick order kept
        _, _, oy, ox = ingest.binned_geometry(img.shape[0], img.shape[1], 4)
        xy = np.array([ingest.to_unbinned(x, y, 4, ox, oy) for x, y, _ in kept])
        assert np.array_equal(call[1], xy)                                      # --picks_bin mapping == to_unbinned
        want, status = extract_model(img, xy, 16, 2, 3)
        assert counts[name] == {"written": int((status == OK).sum()), "outside": int((status == OUTSIDE).sum()),
                                "flat": int((status == FLAT).sum())}
        assert counts[name]["written"] >= 2 and counts[name]["outside"] >= 1
        stack, header, _ = micrograph_io.parse_mrc(open(os.path.join(out_dir, name + ".mrcs"), "rb").read())
        assert header.mode == 2 and (header.nz, header.ny, header.nx) == (counts[name]["written"], 8, 8)
        assert np.array_equal(stack, want[status == OK])
        k = 0
        for i in np.flatnonzero(status == OK):
            k += 1                                                              # 1-based place in the stack
            want_rows.append([str(xy[i, 0]), str(xy[i, 1]), "%06d@%s.mrcs" % (k, name), name + ".mrc", str(kept[i][2])])
    assert got_rows == want_rows and len(want_rows) >= 4
    assert not os.path.exists(os.path.join(out_dir, "micC.mrcs"))

    # a threshold nothing survives: tables are read, no device call, no stack, an empty STAR table
    del calls[:]
    out2 = str(tmp_path / "out2")
    counts = extract.extract_dataset(table, picks, out2, 16, picks_bin=4, threshold=2.0)
    assert counts == {n: {"written": 0, "outside": 0, "flat": 0} for n in ("micA", "micB")} and not calls
    assert sorted(os.listdir(out2)) == ["particles.star"] and open(os.path.join(out2, "particles.star")).read() == head

    # explicit files in the raw frame (picks_bin 1): coordinates pass through unchanged
    raw_table = str(tmp_path / "micA_raw.txt")
    open(raw_table, "w").write("image_name\tx_coord\ty_coord\tscore\nmicA\t40\t30\t0.5\nmicA\t45\t35\t0.25\n")
    counts = extract.extract_dataset(table, [raw_table], str(tmp_path / "out3"), 8, normalize=False, invert=True)
    assert counts == {"micA": {"written": 2, "outside": 0, "flat": 0}}
    assert np.array_equal(calls[0][1], [(40, 30), (45, 35)]) and calls[0][2:] == (8, 1, 3, False, True)
    with pytest.raises(ValueError):
        extract.extract_dataset(table, picks, out_dir, 18, bin=4)
    with pytest.raises(ValueError):
        extract.extract_dataset(table, picks, out_dir, 2048)
