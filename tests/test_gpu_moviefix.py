"""GPU: raw detector movies in (csrc/moviefix.hip, ``torch.ops.sprk.movie_correct``, spr_pick_amd/moviefix.py):
the kernel bit for bit against the NumPy model of its contract (tests/moviefix_model.py) in every sample type, with every
combination of references, on frames whose size is no multiple of four, smaller than a window and larger than a workgroup;
the running sum as one chain; the refusals of the C ABI; and ``joint align --gain --dark --defects --hot_sigma`` end to end
on spoiled movies with planted drift."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

import align_model
import moviefix_model
from extract_model import write_raw_mrc

pytestmark = pytest.mark.gpu

NAN = float("nan")
FRAMES = [(37, 45), (70, 90), (2, 2), (1, 5), (130, 257)]
MODES = [0, 1, 2, 6]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def upload(img):
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(img).tobytes(), dtype=np.uint8).copy()).cuda()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def device_correct(raw, gain=None, dark=None, fix=None, total=None, first=True):
    """through the C ABI, into an output (and, when ``first``, a sum) this test has filled with NaN -> out [, the sum tensor]"""
    from spr_pick_amd import _lib
    L = _lib.lib()
    ny, nx = raw.shape
    out = torch.full((ny, nx), NAN, device="cuda")
    if total is not None and first:
        total.fill_(NAN)
    g, d, f = dev(gain), dev(dark), dev(fix)
    r = upload(raw)
    rc = L.sprk_movie_correct(r.data_ptr(), align_model.MODE_OF[raw.dtype], ny, nx, None if g is None else g.data_ptr(),
                              None if d is None else d.data_ptr(), None if f is None else f.data_ptr(), out.data_ptr(),
                              None if total is None else total.data_ptr(), 1 if first else 0, _stream())
    assert rc == 0, L.sprk_last_error()
    return out.cpu().numpy()


def make_frame(mode, ny, nx, rng):
    if mode == 2:
        return (rng.randn(ny, nx) * 100).astype(np.float32)
    info = np.iinfo(align_model.DTYPES[mode])
    img = rng.randint(info.min, info.max + 1, size=(ny, nx)).astype(align_model.DTYPES[mode])
    img.flat[0], img.flat[-1] = info.min, info.max
    return img


def make_references(ny, nx, rng):
    """a gain in 0.5 .. 1.5 and a dark in 0 .. 50, neither a round number: the subtraction and the product both round"""
    return rng.uniform(0.5, 1.5, size=(ny, nx)).astype(np.float32), rng.uniform(0, 50, size=(ny, nx)).astype(np.float32)


def make_fix(ny, nx, rng):
    """bad pixels at both ends of rows (the first and last of the frame among them: the scalar tail), a run along a row that
    crosses a group of four, a vertical run, and a scatter; hand-set radii 1 .. 8, not the smallest that would do.  The
    frames of a few pixels have their first and last pixel marked, and every window is larger than they are."""
    fix = np.zeros((ny, nx), dtype=np.uint8)
    fix[0, 0] = fix[-1, -1] = 1
    if ny * nx > 8:
        fix[rng.rand(ny, nx) < 0.03] = 1
        fix[0, -1] = fix[-1, 0] = fix[ny // 2, -1] = fix[ny // 2, 0] = 1
    if nx >= 12:
        fix[ny // 3, 3:10] = 1
    if ny >= 12:
        fix[2:11, nx // 2] = 1
    bad = fix > 0
    fix[bad] = rng.randint(1, 9, size=int(bad.sum()))
    return fix


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ny,nx", FRAMES, ids=["%dx%d" % f for f in FRAMES])
def test_movie_correct_matches_the_model(ny, nx, mode):
    rng = np.random.RandomState(100 * ny + nx + mode)
    raw = make_frame(mode, ny, nx, rng)
    gain, dark = make_references(ny, nx, rng)
    fix = make_fix(ny, nx, rng)
    want = moviefix_model.movie_correct(raw, gain, dark, fix)
    got = device_correct(raw, gain, dark, fix)
    differ = int((bits(got) != bits(want)).sum())
    print("mode %d, %dx%d, %d of %d pixels marked: %d differ from the model" % (mode, ny, nx, int((fix > 0).sum()), fix.size, differ))
    assert np.isfinite(got).all() and differ == 0
    # the operator: the same bytes
    out = torch.full((ny, nx), NAN, device="cuda")
    assert torch.ops.sprk.movie_correct(upload(raw), mode, ny, nx, dev(gain), dev(dark), dev(fix), out, None, True) is None
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))


@pytest.mark.parametrize("with_gain,with_dark,with_fix", [(g, d, f) for g in (0, 1) for d in (0, 1) for f in (0, 1)])
def test_every_combination_of_references(with_gain, with_dark, with_fix):
    ny, nx = 70, 90
    rng = np.random.RandomState(7)
    raw = make_frame(1, ny, nx, rng)
    gain, dark = make_references(ny, nx, rng)
    fix = make_fix(ny, nx, rng)
    args = (gain if with_gain else None, dark if with_dark else None, fix if with_fix else None)
    want = moviefix_model.movie_correct(raw, *args)
    got = device_correct(raw, *args)
    assert np.isfinite(got).all() and np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
    if not (with_gain or with_dark or with_fix):
        assert np.array_equal(got, raw.astype(np.float32))                    # a plain decode


FIX_CASES = [c for c in moviefix_model.fix_cases() if c[2] is not None]


@pytest.mark.parametrize("name,bad,largest", FIX_CASES, ids=[c[0] for c in FIX_CASES])
def test_the_maps_of_build_fix(name, bad, largest):
    """the layouts of the CPU list, their maps built on the device by ``moviefix.build_fix``"""
    from spr_pick_amd import moviefix
    ny, nx = bad.shape
    rng = np.random.RandomState(len(name))
    raw = make_frame(1, ny, nx, rng)
    gain, dark = make_references(ny, nx, rng)
    fix = moviefix.build_fix(torch.from_numpy(bad).cuda()).cpu().numpy()
    assert np.array_equal(fix, moviefix_model.build_fix(bad)) and int(fix.max()) == largest
    got = device_correct(raw, gain, dark, fix)
    assert np.isfinite(got).all() and np.array_equal(bits(got), bits(moviefix_model.movie_correct(raw, gain, dark, fix)))


def test_hand_set_radii_the_clamp_and_an_unreachable_pixel():
    ny, nx = moviefix_model.FIX_SHAPE
    rng = np.random.RandomState(21)
    raw = make_frame(6, ny, nx, rng)
    gain, dark = make_references(ny, nx, rng)
    fix = np.zeros((ny, nx), dtype=np.uint8)
    for r in range(1, 9):                                                     # every radius, along a diagonal
        fix[2 + 4 * r, 3 + 5 * r] = r
    fix[20, 4] = 200                                                          # clamped to 8
    got = device_correct(raw, gain, dark, fix)
    assert np.array_equal(bits(got), bits(moviefix_model.movie_correct(raw, gain, dark, fix)))
    clamped = fix.copy()
    clamped[20, 4] = 8
    assert np.array_equal(bits(got), bits(device_correct(raw, gain, dark, clamped)))
    assert got[20, 4] != device_correct(raw, gain, dark, np.where(fix == 200, 7, fix).astype(np.uint8))[20, 4]
    # a 19 x 19 blob marked with radius 1 throughout: inside, no window holds a good pixel, and the output is 0.0f
    blob = next(c[1] for c in moviefix_model.fix_cases() if c[0] == "blob19")
    fix = blob.astype(np.uint8)
    want = moviefix_model.movie_correct(raw, gain, dark, fix)
    got = device_correct(raw, gain, dark, fix)
    assert np.array_equal(bits(got), bits(want))
    assert not got[12:29, 16:33].any() and got[11, 15] != 0 and bits(got)[20, 24] == 0       # +0.0f


def test_nothing_of_a_bad_pixel_reaches_the_output():
    """float32 samples: NaN and Inf samples, and Inf / NaN / 0 gains and NaN darks, on marked pixels only"""
    ny, nx = 70, 90
    rng = np.random.RandomState(31)
    raw = make_frame(2, ny, nx, rng)
    gain, dark = make_references(ny, nx, rng)
    fix = make_fix(ny, nx, rng)
    marked = np.argwhere(fix > 0)
    poison = [np.nan, np.inf, -np.inf]
    for i, (y, x) in enumerate(marked):
        raw[y, x] = poison[i % 3] if i % 2 == 0 else raw[y, x]
        gain[y, x] = [np.inf, np.nan, 0.0, -1.0][i % 4]
        dark[y, x] = np.nan if i % 5 == 0 else dark[y, x]
    want = moviefix_model.movie_correct(raw, gain, dark, fix)
    total = torch.empty((ny, nx), device="cuda")
    got = device_correct(raw, gain, dark, fix, total)
    assert np.isfinite(want).all() and np.isfinite(got).all() and np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(total.cpu().numpy()), bits(want))
    unmarked = device_correct(raw, gain, dark, None)                          # and without the map they do come out
    assert not np.isfinite(unmarked[fix > 0]).all()


@pytest.mark.parametrize("mode,ny,nx", [(1, 37, 45), (2, 70, 90), (0, 1, 5)])
def test_the_sum_is_one_chain(mode, ny, nx):
    rng = np.random.RandomState(41 + mode)
    frames = [make_frame(mode, ny, nx, rng) for _ in range(3)]
    gain, dark = make_references(ny, nx, rng)
    fix = make_fix(ny, nx, rng)
    outs, want = moviefix_model.movie_sum(frames, gain, dark, fix)
    total = torch.empty((ny, nx), device="cuda")
    for k, f in enumerate(frames):
        got = device_correct(f, gain, dark, fix, total, k == 0)
        assert np.array_equal(bits(got), bits(outs[k]))
    assert np.array_equal(bits(total.cpu().numpy()), bits(want))
    # `first` does not read the sum: a second start on a sum full of NaN gives the frame alone
    got = device_correct(frames[1], gain, dark, fix, total, True)
    assert np.array_equal(bits(total.cpu().numpy()), bits(got))


def test_refusals_launch_nothing():
    from spr_pick_amd import _lib
    L = _lib.lib()
    ny, nx = 70, 90
    rng = np.random.RandomState(51)
    img = make_frame(1, ny, nx, rng)
    gain, dark = make_references(ny, nx, rng)
    fix = make_fix(ny, nx, rng)
    raw, g, d, f = upload(img), dev(gain), dev(dark), dev(fix)
    out, total = torch.full((ny, nx), NAN, device="cuda"), torch.full((ny, nx), NAN, device="cuda")
    good = dict(raw=raw.data_ptr(), mode=1, ny=ny, nx=nx, gain=g.data_ptr(), dark=d.data_ptr(), fix=f.data_ptr(),
                out=out.data_ptr(), total=total.data_ptr(), first=1)

    def call(**change):
        a = dict(good, **change)
        return L.sprk_movie_correct(a["raw"], a["mode"], a["ny"], a["nx"], a["gain"], a["dark"], a["fix"], a["out"], a["total"],
                                    a["first"], _stream())

    torch.cuda.synchronize()
    before = L.sprk_launch_count()
    cases = [(dict(raw=None), b"null"), (dict(out=None), b"null"), (dict(mode=3), b"mode"), (dict(mode=7), b"mode"),
             (dict(ny=0), b"frame"), (dict(nx=16385), b"frame"), (dict(raw=raw.data_ptr() + 2), b"aligned"),
             (dict(gain=g.data_ptr() + 4), b"aligned"), (dict(dark=d.data_ptr() + 8), b"aligned"),
             (dict(fix=f.data_ptr() + 1), b"aligned"), (dict(out=out.data_ptr() + 4), b"aligned"),
             (dict(total=total.data_ptr() + 4), b"aligned"), (dict(out=raw.data_ptr()), b"out must not be"),
             (dict(out=g.data_ptr()), b"out must not be"), (dict(out=d.data_ptr()), b"out must not be"),
             (dict(out=total.data_ptr()), b"out must not be")]
    for change, word in cases:
        assert call(**change) == -1, (change, L.sprk_last_error())
        assert L.sprk_last_error().startswith(b"movie_correct: ") and word in L.sprk_last_error(), (change, L.sprk_last_error())
    torch.cuda.synchronize()
    assert L.sprk_launch_count() == before
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(total).all())    # both still hold their fill
    assert torch.equal(g, dev(gain)) and torch.equal(d, dev(dark)) and torch.equal(raw, upload(img))
    assert call() == 0, L.sprk_last_error()
    assert L.sprk_launch_count() == before + 1                                # one launch per frame
    want = moviefix_model.movie_correct(img, gain, dark, fix)
    assert np.array_equal(bits(out.cpu().numpy()), bits(want)) and np.array_equal(bits(total.cpu().numpy()), bits(want))
    # the operator refuses tensors that are not contiguous
    with pytest.raises(_lib.SprkError, match="contiguous"):
        torch.ops.sprk.movie_correct(raw, 1, ny, nx, g, d, f, torch.empty((nx, ny), device="cuda").t(), None, True)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
DEVICE_VS_MODEL = 0.01 + 0.0004                  # tests/test_gpu_align.py: the loop's tolerance plus what was measured there
APIX = 1.5
CASES = [0, 1]


def write_movie(path, movie, apix):
    """an MRC stack of the movie's own sample type whose header states the pixel size"""
    write_raw_mrc(path, movie)
    Z, ny, nx = movie.shape
    with open(path, "r+b") as f:
        f.seek(28)
        f.write(struct.pack("<3i3f", nx, ny, Z, apix * nx, apix * ny, apix * Z))


def read_shifts(path):
    rows = [line.split("\t") for line in open(path).read().splitlines()]
    assert rows[0] == ["frame", "dx", "dy"]
    return np.array([[float(r[1]), float(r[2])] for r in rows[1:]])


def read_bytes(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def movies():
    """per case: the clean movie M, its planted drift, and both spoilings (gain and dark only; with the defects)"""
    ny, nx = align_model.MOVIE_SHAPE
    out = {}
    for case in CASES:
        seed, noise = align_model.MOVIE_CASES[case]
        movie, _, drift = align_model.make_movie(ny, nx, align_model.MOVIE_FRAMES, seed, noise)
        out[case] = (movie, drift, moviefix_model.spoil(movie, seed, defects=False), moviefix_model.spoil(movie, seed))
    return out


def lay_out(root, raw, s):
    """root/movies/mov.mrc, root/refs/{gain,dark}.mrc, root/refs/defects.txt -> the flags that name them"""
    os.makedirs(os.path.join(root, "movies"))
    os.makedirs(os.path.join(root, "refs"))
    write_movie(os.path.join(root, "movies", "mov.mrc"), raw, APIX)
    gain, dark, defects = (os.path.join(root, "refs", n) for n in ("gain.mrc", "dark.mrc", "defects.txt"))
    write_raw_mrc(gain, s["gain"])
    write_raw_mrc(dark, s["dark"].astype(np.int16))                           # a dark reference in an integer mode
    moviefix_model.write_defects(defects, s["rects"])
    return ["align", "--movies", os.path.join(root, "movies")], ["--gain", gain, "--dark", dark], ["--defects", defects]


@pytest.mark.parametrize("case", CASES)
def test_gain_and_dark_give_the_bytes_of_the_clean_movie(case, movies, tmp_path):
    """(a) raw = M / gain + dark exactly, so the corrected frames are M as float32, and the run writes what plain `joint
    align` writes for M stored as a float32 movie"""
    from spr_pick_amd import cli, micrograph_io
    movie, drift, s, _ = movies[case]
    root = str(tmp_path)
    base, refs, _ = lay_out(os.path.join(root, "raw"), s["raw"], s)
    os.makedirs(os.path.join(root, "clean"))
    write_movie(os.path.join(root, "clean", "mov.mrc"), movie.astype(np.float32), APIX)
    want_dir, got_dir, sum_dir = (os.path.join(root, n) for n in ("want", "got", "sum"))
    want = cli.start(["align", "--movies", os.path.join(root, "clean"), "--out", want_dir])
    got = cli.start(base + ["--out", got_dir] + refs)
    assert sorted(os.listdir(want_dir)) == ["images.txt", "mov.mrc", "mov_shifts.txt"]
    assert sorted(os.listdir(got_dir)) == ["images.txt", "mov.mrc", "mov_defects.mrc", "mov_shifts.txt"]
    for name in ("mov.mrc", "mov_shifts.txt"):
        assert read_bytes(os.path.join(got_dir, name)) == read_bytes(os.path.join(want_dir, name)), name
    assert got["mov"]["defects"] == {"static": 0, "hot": 0} and "defects" not in want["mov"]
    assert {k: v for k, v in got["mov"].items() if k != "defects"} == want["mov"]
    fix, header, _ = micrograph_io.parse_mrc(read_bytes(os.path.join(got_dir, "mov_defects.mrc")))
    assert header.mode == 0 and fix.shape == movie.shape[1:] and not fix.any()
    assert float(np.abs(read_shifts(os.path.join(got_dir, "mov_shifts.txt")) - drift).max()) <= 1.5 * align_model.MODEL_WORST
    cli.start(base + ["--out", sum_dir, "--no_align"] + refs)
    total, _, _ = micrograph_io.parse_mrc(read_bytes(os.path.join(sum_dir, "mov.mrc")))
    assert np.array_equal(total, movie.astype(np.float64).sum(axis=0).astype(np.float32))


@pytest.mark.parametrize("case", CASES)
def test_a_spoiled_movie_pins_the_shifts_without_the_flags(case, movies, tmp_path):
    """(b) the failure this repairs: the fixed pattern correlates with itself at shift zero"""
    from spr_pick_amd import cli
    movie, drift, _, s = movies[case]
    base, _, _ = lay_out(str(tmp_path), s["raw"], s)
    out = os.path.join(str(tmp_path), "out")
    res = cli.start(base + ["--out", out])
    got = read_shifts(os.path.join(out, "mov_shifts.txt"))
    miss = float(np.abs(got - drift).max())
    print("case %d without the flags: largest |shift| %.4f, worst |device - planted| %.4f raw pixels" % (case, float(np.abs(got).max()), miss))
    assert sorted(os.listdir(out)) == ["images.txt", "mov.mrc", "mov_shifts.txt"] and "defects" not in res["mov"]
    assert miss > 4


@pytest.mark.parametrize("case", CASES)
def test_the_corrected_movie_aligns(case, movies, tmp_path):
    """(c) --gain --dark --defects --hot_sigma 6, with --dose 1.0 on top"""
    from spr_pick_amd import cli, micrograph_io
    movie, drift, _, s = movies[case]
    Z, ny, nx = movie.shape
    base, refs, defects = lay_out(str(tmp_path), s["raw"], s)
    out = os.path.join(str(tmp_path), "out")
    res = cli.start(base + ["--out", out] + refs + defects + ["--hot_sigma", "6", "--dose", "1.0"])
    assert sorted(os.listdir(out)) == ["images.txt", "images_DW.txt", "mov.mrc", "mov_DW.mrc", "mov_defects.mrc", "mov_shifts.txt"]
    static, bad, fix, frames = moviefix_model.prepare(s["raw"], s["gain"], s["dark"], moviefix_model.defect_mask(s["rects"], ny, nx), 6.0)
    assert np.array_equal(bad & ~static, s["hot"])                            # the model finds the planted set, and so must
    got_fix, header, _ = micrograph_io.parse_mrc(read_bytes(os.path.join(out, "mov_defects.mrc")))       # the device
    assert header.mode == 0 and got_fix.dtype == np.int8 and np.array_equal(got_fix, fix)
    assert np.array_equal((got_fix > 0) & ~static, s["hot"])
    assert res["mov"]["defects"] == {"static": int(static.sum()), "hot": moviefix_model.HOT_COUNT}
    model = align_model.estimate_movie(frames, ny, nx)
    got = read_shifts(os.path.join(out, "mov_shifts.txt"))
    to_model, to_planted = float(np.abs(got - model).max()), float(np.abs(got - drift).max())
    print("case %d corrected: %d iteration(s); worst |device - model| %.4f, |device - planted| %.4f, |model - planted| %.4f raw "
          "pixels" % (case, res["mov"]["iterations"], to_model, to_planted, float(np.abs(model - drift).max())))
    assert got.shape == (Z, 2) and res["mov"]["edge_frames"] == []
    assert to_model <= DEVICE_VS_MODEL
    assert to_planted <= 1.5 * align_model.MODEL_WORST < 0.5
    weighted, _, _ = micrograph_io.parse_mrc(read_bytes(os.path.join(out, "mov_DW.mrc")))
    total, _, _ = micrograph_io.parse_mrc(read_bytes(os.path.join(out, "mov.mrc")))
    assert weighted.shape == total.shape == (ny, nx) and np.isfinite(weighted).all() and np.isfinite(total).all()
    assert total.max() < 8 * 4096                                             # no hot pixel (30000 a frame) is left in the sum
