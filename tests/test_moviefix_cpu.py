"""CPU: raw detector movies in (`joint align --gain / --dark / --defects / --hot_sigma`) without a GPU — the
command line, the reference and defect files, the fix map and the hot-pixel rule against the loops of
tests/moviefix_model.py, the registrations and refusals of ``sprk_movie_correct``, and the float64 estimation loop of
tests/align_model.py failing on a spoiled movie and recovering on the corrected one."""
import os
import re

import numpy as np
import pytest
import torch

import align_model
import moviefix_model
from extract_model import write_raw_mrc


def test_parser():
    from spr_pick_amd import cli
    p = cli.build_parser()
    base = ["align", "--movies", "m", "--out", "o"]
    a = vars(p.parse_args(base))
    assert all(a[k] is None for k in ("gain", "gain_rot", "gain_flip", "dark", "defects", "hot_sigma"))
    a = vars(p.parse_args(base + ["--gain", "g.mrc", "--gain_rot", "3", "--gain_flip", "lr", "--dark", "d.mrc", "--defects",
                                  "bad.txt", "--hot_sigma", "6"]))
    assert (a["gain"], a["gain_rot"], a["gain_flip"], a["dark"], a["defects"], a["hot_sigma"]) == \
        ("g.mrc", 3, "lr", "d.mrc", "bad.txt", 6.0)
    a = vars(p.parse_args(base + ["--hot_sigma", "4.5"]))                     # hot pixels alone, on gain-corrected movies
    assert a["hot_sigma"] == 4.5 and a["gain"] is None
    for bad in (base + ["--gain_rot", "1"], base + ["--gain_flip", "ud"], base + ["--gain_rot", "0"],
                base + ["--dark", "d.mrc", "--gain_rot", "2"], base + ["--gain", "g", "--gain_rot", "4"],
                base + ["--gain", "g", "--gain_rot", "-1"], base + ["--gain", "g", "--gain_rot", "x"],
                base + ["--gain", "g", "--gain_flip", "both"], base + ["--hot_sigma", "0"], base + ["--hot_sigma", "-3"],
                base + ["--hot_sigma", "nan"], base + ["--hot_sigma", "inf"], base + ["--hot_sigma", "x"], base + ["--gain"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    text = " ".join(p._subparsers._group_actions[0].choices["align"].format_help().split())
    for word in ("--gain", "--gain_rot", "--gain_flip", "--dark", "--defects", "--hot_sigma", "MULTIPLIED", "divided by",
                 "6 is recommended", "_defects.mrc", "x y w h", "local", "TIFF", "EER"):
        assert word in text, word
    not_covered = text[text.index("Not covered"):].split(".")[0]
    assert "gain" not in not_covered and "dark" not in not_covered
    for word in ("local", "TIFF", "EER"):
        assert word in not_covered, word


def test_library_refuses_bad_correction_arguments():
    from spr_pick_amd import align, moviefix
    for kw in (dict(gain_rot=1), dict(gain_flip="ud"), dict(gain="g.mrc", gain_rot=4), dict(gain="g.mrc", gain_flip="x"),
               dict(hot_sigma=0.0), dict(hot_sigma=float("nan")), dict(hot_sigma=float("inf")), dict(hot_sigma=True)):
        with pytest.raises(ValueError):
            align.align_dataset("nowhere", "nowhere", **kw)
        with pytest.raises(ValueError):
            moviefix.check_fix_args(**kw)
    assert moviefix.check_fix_args() is False and moviefix.check_fix_args(hot_sigma=6) is True
    assert moviefix.check_fix_args(dark="d.mrc") is True and moviefix.check_fix_args(gain="g", gain_rot=3, gain_flip="lr") is True


def test_read_reference_orientation_and_refusals(tmp_path):
    from spr_pick_amd import moviefix
    g = np.arange(15, dtype=np.float32).reshape(3, 5) + 1
    path = str(tmp_path / "gain.mrc")
    write_raw_mrc(path, g)
    for rot in (0, 1, 2, 3):
        for flip in (None, "ud", "lr"):
            want = np.rot90(g, rot)
            want = want if flip is None else (np.flipud(want) if flip == "ud" else np.fliplr(want))
            ny, nx = want.shape
            assert (ny, nx) == ((3, 5) if rot % 2 == 0 else (5, 3))
            got = moviefix.read_reference(path, ny, nx, rot, flip)
            assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(got, want), (rot, flip)
            with pytest.raises(ValueError, match="frames are"):
                moviefix.read_reference(path, nx, ny, rot, flip)             # the other orientation
    # written out: one quarter turn counter-clockwise brings the last column to the top row, and "ud" turns that over
    assert np.array_equal(moviefix.read_reference(path, 5, 3, 1)[0], g[:, 4])
    assert np.array_equal(moviefix.read_reference(path, 5, 3, 1, "ud")[4], g[:, 4])
    assert np.array_equal(moviefix.read_reference(path, 3, 5, 0, "lr")[:, 0], g[:, 4])
    for dtype in (np.int8, np.int16, np.uint16):                              # the integer modes come out as float32
        write_raw_mrc(path, g.astype(dtype))
        assert np.array_equal(moviefix.read_reference(path, 3, 5), g)
    for bad in (dict(rot=4), dict(rot=True), dict(flip="x")):
        with pytest.raises(ValueError):
            moviefix.read_reference(path, 3, 5, **bad)
    stack = str(tmp_path / "stack.mrc")
    write_raw_mrc(stack, np.zeros((2, 3, 5), dtype=np.float32))
    with pytest.raises(ValueError, match="single image"):
        moviefix.read_reference(stack, 3, 5)
    with open(path, "r+b") as f:
        f.truncate(1024 + 20)
    with pytest.raises(ValueError):
        moviefix.read_reference(path, 3, 5)


def test_read_defects_and_refusals(tmp_path):
    from spr_pick_amd import moviefix
    path = str(tmp_path / "defects.txt")
    open(path, "w").write("# x y w h\n\n  2 1 3 2  \n0 5 8 1\n#7 7 1 1\n7 0 1 6\n")
    bad = moviefix.read_defects(path, 6, 8)
    want = np.zeros((6, 8), dtype=bool)
    want[1:3, 2:5] = True                                                     # x is the column, y the row
    want[5, :] = True
    want[:, 7] = True
    assert bad.dtype == bool and np.array_equal(bad, want)
    assert np.array_equal(bad, moviefix_model.defect_mask([(2, 1, 3, 2), (0, 5, 8, 1), (7, 0, 1, 6)], 6, 8))
    for text, line in (("2 1 3 2\n6 0 3 1\n", 2), ("# c\n\n0 5 1 2\n", 3), ("-1 0 2 2\n", 1), ("0 0 0 1\n", 1), ("0 0 1 0\n", 1),
                       ("0 -2 1 1\n", 1), ("1 2 3\n", 1), ("1 2 3 4 5\n", 1), ("1 2 3 x\n", 1), ("1.5 2 3 4\n", 1)):
        open(path, "w").write(text)
        with pytest.raises(ValueError, match="line %d" % line):
            moviefix.read_defects(path, 6, 8)


def test_static_bad():
    from spr_pick_amd import moviefix
    gain = np.ones((4, 6), dtype=np.float32)
    gain[0, 0], gain[1, 1], gain[2, 2], gain[3, 3], gain[0, 5] = 0.0, -1.0, np.nan, np.inf, 1e-30
    rects = moviefix_model.defect_mask([(4, 1, 2, 2)], 4, 6)
    want = moviefix_model.static_bad(gain, rects)
    assert want.sum() == 4 + 4 and not want[0, 5]
    got = moviefix.static_bad(torch.from_numpy(gain), torch.from_numpy(rects))
    assert got.dtype == torch.bool and np.array_equal(got.numpy(), want)
    assert np.array_equal(moviefix.static_bad(torch.from_numpy(gain), None).numpy(), moviefix_model.static_bad(gain, None))
    assert np.array_equal(moviefix.static_bad(None, torch.from_numpy(rects)).numpy(), rects)
    assert moviefix.static_bad(None, None) is None


FIX_CASES = moviefix_model.fix_cases()


@pytest.mark.parametrize("name,bad,largest", FIX_CASES, ids=[c[0] for c in FIX_CASES])
def test_build_fix_equals_the_model(name, bad, largest):
    """A w x w blob's centre is (w + 1) / 2 from the nearest good pixel: 15 x 15 is the largest that can be repaired (radius
    8 at its centre); the centre of 17 x 17 has a window of +-8 that is the blob itself, so it raises as 19 x 19 does."""
    from spr_pick_amd import moviefix
    if largest is None:
        with pytest.raises(ValueError) as model_err:
            moviefix_model.build_fix(bad)
        with pytest.raises(ValueError, match=r"\d+ bad pixel\(s\) without a good one within 8 pixels, the first at row 19, column 23"):
            moviefix.build_fix(torch.from_numpy(bad))
        assert "row 19, column 23" in str(model_err.value)
        return
    want = moviefix_model.build_fix(bad)
    got = moviefix.build_fix(torch.from_numpy(bad))
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want)
    assert int(want.max()) == largest and np.array_equal(want > 0, bad)
    if name == "blob5":
        assert sorted(set(want[bad])) == [1, 2, 3]
    if name == "corners":                                                     # the window is clamped to the frame
        assert want[0, 0] == want[-1, -1] == 1


def test_build_fix_refuses_other_tensors():
    from spr_pick_amd import moviefix
    for bad in (torch.zeros(4, 4), torch.zeros(4, dtype=torch.bool), torch.zeros(1, 4, 4, dtype=torch.bool)):
        with pytest.raises(ValueError):
            moviefix.build_fix(bad)
    assert not moviefix.build_fix(torch.zeros(3, 5, dtype=torch.bool)).any()
    with pytest.raises(ValueError, match="6 bad"):                            # nothing good at all
        moviefix.build_fix(torch.ones(2, 3, dtype=torch.bool))


def test_detect_hot_needs_its_second_round():
    """three pixels at 1e4 inflate the first round's sigma to several hundred, which hides five pixels at 9; the second
    round, without the three, finds them; the third finds nothing"""
    from spr_pick_amd import moviefix
    rng = np.random.RandomState(11)
    T = rng.standard_normal((30, 40)).astype(np.float32)
    T = np.clip(T, -3.5, 3.5)
    strong, mild = [(2, 3), (17, 39), (29, 0)], [(0, 0), (5, 20), (14, 14), (22, 31), (29, 39)]
    for p in strong:
        T[p] = 1e4
    for p in mild:
        T[p] = 9.0
    static = np.zeros(T.shape, dtype=bool)
    static[10, :] = True                                                      # a dead row holds a value that must not count
    T[10, :] = 5e5
    want, rounds = moviefix_model.detect_hot(T, static, 6.0)
    assert len(rounds) == 3
    assert 1e4 > rounds[0][0] > 9.0 > rounds[1][0] and rounds[0][1] > 100 and rounds[2][1] < 1.1
    found = want & ~static
    assert sorted(map(tuple, np.argwhere(found))) == sorted(strong + mild)
    for threshold, sd in rounds:                                              # no pixel sits within 1e-6 sigma of a threshold
        assert np.abs(T.astype(np.float64) - threshold)[~static].min() > 1e-6 * sd
    got = moviefix.detect_hot(torch.from_numpy(T), torch.from_numpy(static), 6.0)
    assert got.dtype == torch.bool and np.array_equal(got.numpy(), want)
    assert not static[0, 0]                                                   # the argument is left as it was
    # one round only when nothing stands out, and an all-bad frame is left alone
    calm, rounds = moviefix_model.detect_hot(np.clip(rng.standard_normal((30, 40)), -3, 3), static, 6.0)
    assert len(rounds) == 1 and np.array_equal(calm, static)
    everything = torch.ones(3, 3, dtype=torch.bool)
    assert moviefix.detect_hot(torch.zeros(3, 3), everything, 6.0).all()


def test_names_in_header_binding_and_torch_library():
    from conftest import ROOT
    from torch._subclasses.fake_tensor import FakeTensorMode
    from spr_pick_amd import _lib, moviefix, torch_ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sprk.h")).read(), flags=re.S)
    assert "sprk_movie_correct" in set(re.findall(r"\b(sprk_[a-z0-9_]+)\s*\(", text))
    assert re.search(r"#define SPRK_ABI_VERSION 430\b", text) and _lib.ABI_VERSION == 430
    assert re.search(r"#define SPRK_FIX_MAX_RADIUS 8\b", text)
    assert torch_ops.FIX_MAX_RADIUS == moviefix.FIX_MAX_RADIUS == moviefix_model.FIX_MAX_RADIUS == 8
    assert "sprk_movie_correct" in _lib.EXPORTS
    L = _lib.lib()
    assert hasattr(L, "sprk_movie_correct") and L.sprk_version() == 430
    assert "movie_correct" in torch_ops.registered() and hasattr(torch.ops.sprk, "movie_correct")
    makefile = open(os.path.join(ROOT, "spr_pick_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bmoviefix\.hip\b", makefile, flags=re.M)
    assert re.search(r"moviefix\.o: CXXFLAGS \+= -ffp-contract=off", makefile)

    # refusals come before anything touches the device: the pointers are never dereferenced
    P, Q = 0x10000, 0x20000

    def call(raw=P, mode=1, ny=70, nx=90, gain=0x30000, dark=0x40000, fix=0x50000, out=Q, total=0x60000, first=1):
        return L.sprk_movie_correct(raw, mode, ny, nx, gain, dark, fix, out, total, first, None)

    before = L.sprk_launch_count()
    cases = [(dict(raw=None), b"null"), (dict(out=None), b"null"), (dict(mode=3), b"mode"), (dict(mode=-1), b"mode"),
             (dict(mode=4), b"mode"), (dict(ny=0), b"frame"), (dict(nx=0), b"frame"), (dict(ny=16385), b"frame"),
             (dict(nx=16385), b"frame"), (dict(raw=P + 4), b"aligned"), (dict(gain=0x30008), b"aligned"),
             (dict(dark=0x40004), b"aligned"), (dict(fix=0x50001), b"aligned"), (dict(out=Q + 8), b"aligned"),
             (dict(total=0x60004), b"aligned"), (dict(out=P), b"out must not be"), (dict(out=0x30000), b"out must not be"),
             (dict(out=0x40000), b"out must not be"), (dict(out=0x60000), b"out must not be")]
    for change, word in cases:
        assert call(**change) == -1, change
        err = L.sprk_last_error()
        assert err.startswith(b"movie_correct: ") and word in err, (change, err)
    assert L.sprk_launch_count() == before

    with FakeTensorMode():
        ny, nx = 70, 90
        raw = torch.empty(ny * nx * 2, dtype=torch.uint8, device="cuda")
        f32 = lambda *shape: torch.empty(*shape, device="cuda")              # noqa: E731
        gain, dark, out, total = f32(ny, nx), f32(ny, nx), f32(ny, nx), f32(ny, nx)
        fix = torch.empty(ny, nx, dtype=torch.uint8, device="cuda")
        assert torch.ops.sprk.movie_correct(raw, 1, ny, nx, gain, dark, fix, out, total, True) is None
        assert torch.ops.sprk.movie_correct(raw, 1, ny, nx, None, None, None, out, None, False) is None
        assert torch.ops.sprk.movie_correct(raw, 0, ny, nx, gain, None, fix, out, None, True) is None
        for args in ((raw, 3, ny, nx, gain, dark, fix, out, total, True),               # the mode
                     (raw, 2, ny, nx, gain, dark, fix, out, total, True),               # too few bytes for float32
                     (raw.view(torch.int16), 1, ny, nx, gain, dark, fix, out, total, True),
                     (raw, 1, 0, nx, gain, dark, fix, out, total, True), (raw, 1, ny, 16385, gain, dark, fix, out, total, True),
                     (raw, 1, ny, nx, f32(nx, ny), dark, fix, out, total, True), (raw, 1, ny, nx, gain, f32(ny, nx + 1), fix, out, total, True),
                     (raw, 1, ny, nx, gain, dark, fix.float(), out, total, True), (raw, 1, ny, nx, gain, dark, fix, out.double(), total, True),
                     (raw, 1, ny, nx, gain, dark, fix, f32(ny * nx), total, True), (raw, 1, ny, nx, gain, dark, fix, out, f32(1, ny, nx), True),
                     (raw, 1, ny, nx, gain.cpu(), dark, fix, out, total, True)):
            with pytest.raises(_lib.SprkError):
                torch.ops.sprk.movie_correct(*args)


def test_model_window_by_hand():
    """the contract on numbers small enough to add by hand"""
    raw = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]], dtype=np.int16)
    fix = np.zeros((3, 3), dtype=np.uint8)
    fix[1, 1], fix[0, 0] = 1, 1
    out = moviefix_model.movie_correct(raw, None, None, fix)
    assert out[1, 1] == np.float32(20 + 30 + 40 + 60 + 70 + 80 + 90) / np.float32(7)       # (0, 0) is bad: left out
    assert out[0, 0] == np.float32(20 + 40) / np.float32(2)                                 # the window is clamped
    gain = np.full((3, 3), 0.5, dtype=np.float32)
    dark = np.full((3, 3), 2.0, dtype=np.float32)
    gain[1, 1], dark[0, 0] = np.nan, np.inf                                                 # a bad pixel's own references
    out = moviefix_model.movie_correct(raw, gain, dark, fix)
    assert np.isfinite(out).all() and out[2, 2] == 44.0 and out[0, 0] == np.float32(9 + 19) / np.float32(2)
    fix[:] = 200                                                                            # nothing good anywhere
    assert not moviefix_model.movie_correct(raw, gain, dark, fix).any()
    _, total = moviefix_model.movie_sum([raw, raw, raw], None, None, None)
    assert np.array_equal(total, 3 * raw.astype(np.float32))


def test_a_fixed_pattern_pins_the_model_and_the_correction_frees_it():
    """the float64 loop of align_model on MOVIE_CASES[0]: spoiled by gain, dark, a dead column, a defect rectangle and 40 hot
    pixels, every estimated shift stays at zero (the error is the whole planted drift, 5 pixels); with gain and dark applied
    but the defects left in it still does; corrected by the model it is back at the clean movie's estimate"""
    ny, nx = align_model.MOVIE_SHAPE
    seed, noise = align_model.MOVIE_CASES[0]
    movie, _, drift = align_model.make_movie(ny, nx, align_model.MOVIE_FRAMES, seed, noise)
    s = moviefix_model.spoil(movie, seed)
    assert s["hot"].sum() == moviefix_model.HOT_COUNT and s["raw"].dtype == np.int16
    clean = align_model.estimate_movie(movie, ny, nx)
    spoiled = align_model.estimate_movie(s["raw"], ny, nx)
    half = align_model.estimate_movie(np.stack([moviefix_model.corrected(f, s["gain"], s["dark"]) for f in s["raw"]]), ny, nx)
    defects = moviefix_model.defect_mask(s["rects"], ny, nx)
    static, bad, fix, frames = moviefix_model.prepare(s["raw"], s["gain"], s["dark"], defects, 6.0)
    assert static.sum() == ny + 24 - defects[:, s["column"]].sum()
    assert np.array_equal(bad & ~static, s["hot"])                            # the hot set is the planted one
    assert np.array_equal(frames[:, ~bad], movie.astype(np.float32)[:, ~bad])  # good pixels are M again, exactly
    fixed = align_model.estimate_movie(frames, ny, nx)
    err = lambda est: float(np.abs(est - drift).max())                       # noqa: E731
    print("worst |estimated - planted| in raw pixels: clean %.4f, spoiled %.4f (largest |shift| %.4f), gain and dark only "
          "%.4f, corrected %.4f; |corrected - clean| %.4f" % (err(clean), err(spoiled), float(np.abs(spoiled).max()), err(half),
                                                              err(fixed), float(np.abs(fixed - clean).max())))
    assert err(spoiled) > 4 and err(half) > 4
    assert err(fixed) <= 1.5 * align_model.MODEL_WORST and err(clean) <= align_model.MODEL_WORST
    assert float(np.abs(fixed - clean).max()) <= 0.01 + 0.0004               # the loop's tolerance, as DEVICE_VS_MODEL
