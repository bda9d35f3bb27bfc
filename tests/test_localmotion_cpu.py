"""CPU: local motion correction (spr_pick_amd/localmotion.py, ``joint align --patch``): the properties of the
NumPy model of ``sprk_align_warp`` (tests/localmotion_model.py), the patch geometry, the fit and its refusals, the parser, the
names in the header, the binding and torch.library, and the float64 model of the whole loop on the end-to-end cases that
tests/test_gpu_localmotion.py runs on the device."""
import os
import re

import numpy as np
import pytest
import torch

import localmotion_model as lm

ZERO = [0.0] * 6


def frame(shape, seed=0):
    return (np.random.RandomState(seed).standard_normal(shape) * 30).astype(np.float32)


# ---- the model of the kernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (37, 45)])
def test_model_identity_and_integer_shift(shape):
    a = frame(shape)
    w = lm.weights(np.zeros(1, dtype=np.float32))
    assert [float(v[0]) for v in w] == [0.0, 1.0, 0.0, 0.0] and np.signbit(w[0][0])       # exactly (-0, 1, 0, 0)
    assert np.array_equal(lm.warp(a, ZERO, ZERO), a)
    assert np.array_equal(lm.warp(a, [3.0] + ZERO[1:], [-2.0] + ZERO[1:]), np.roll(a, (-3, 2), axis=(0, 1)))
    y = frame(shape, 1)
    assert np.array_equal(lm.warp(a, ZERO, ZERO, y, first=False), y + a)


def test_model_weights_sum_to_one():
    t = np.concatenate([np.arange(0, 1, 2.0 ** -17), np.random.RandomState(0).uniform(0, 1, 100000)]).astype(np.float32)
    total = sum(w.astype(np.float64) for w in lm.weights(t))
    worst = np.abs(total - 1.0).max() / 2.0 ** -23
    print("the four weights sum to 1 within %.2f ulp" % worst)
    assert worst <= 2.0


def test_model_clamp():
    s = lm.shifts([0.0, 100.0, 0.0, 0.0, 0.0, 0.0], 4, 64)
    assert s.min() == -16 and s.max() == 16 and s.dtype == np.float32
    # the clamped shift is an integer one: a roll by 16 where it engages
    a = frame((4, 64))
    out = lm.warp(a, ZERO, [0.0, 100.0, 0.0, 0.0, 0.0, 0.0])
    assert np.array_equal(out[:, 60], a[:, (60 + 16) % 64]) and np.array_equal(out[:, 3], a[:, (3 - 16) % 64])
    # an overflow makes a NaN of inf - inf; fmax / fmin turn it into -16
    with np.errstate(all="ignore"):
        assert float(np.fmin(np.fmax(np.float32("nan"), np.float32(-16)), np.float32(16))) == -16.0


def test_model_reproduces_a_quadratic_image():
    """Catmull-Rom reproduces polynomials up to degree two: away from the wrap, a quadratic image pulled by a constant
    fraction is the quadratic at the displaced positions"""
    ny, nx = 40, 48
    i, j = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")

    def quad(i, j):
        return 3.0 - 0.5 * i + 0.25 * j + 0.02 * i * i - 0.03 * i * j + 0.01 * j * j
    out = lm.warp(quad(i, j).astype(np.float32), [0.3] + ZERO[1:], [-0.6] + ZERO[1:])
    want = quad(i + np.float32(0.3), j + np.float32(-0.6))
    inner = (slice(3, ny - 3), slice(3, nx - 3))
    assert np.abs(out[inner] - want[inner]).max() <= 8 * 2.0 ** -24 * np.abs(want).max()       # a few roundings of the largest value
    assert np.abs(lm.warp64(quad(i, j), np.full((ny, nx), 0.3), np.full((ny, nx), -0.6))[inner] - want[inner]).max() < 1e-5


def test_model_strips_are_the_whole():
    a = frame((37, 45))
    cy, cx = [0.3, 25.0, 18.0, 6.0, -9.0, 4.0], [-0.7, -30.0, 22.0, -5.0, 8.0, 3.0]
    whole = lm.warp(a, cy, cx)
    rows, cols = np.array([0, 5, 36]), np.array([44, 2])
    assert np.array_equal(lm.warp(a, cy, cx, rows=rows, cols=cols), whole[np.ix_(rows, cols)])


# ---- geometry, design, fit ---------------------------------------------------------------------------------------------------
def test_patch_geometry_and_its_refusals():
    from spr_pick_amd import localmotion
    g = localmotion.patch_geometry(256, 320, 3, 3, 6)
    assert (g["ph"], g["pw"]) == (85, 128) and g["y0"].tolist() == [0, 86, 171] and g["x0"].tolist() == [0, 96, 192]
    assert np.allclose(g["u"], (np.array([0, 96, 192]) + 63.5) / 320 - 0.5) and np.allclose(g["v"], (g["y0"] + 42.0) / 256 - 0.5)
    for Sy, Sx, PY, PX in ((256, 320, 3, 3), (1024, 1024, 5, 5), (1024, 1024, 16, 16), (720, 1024, 7, 4), (4096, 4096, 5, 7)):
        g = localmotion.patch_geometry(Sy, Sx, PY, PX, 6)
        assert (g["ph"], g["pw"], g["y0"].tolist(), g["x0"].tolist()) == lm.patch_grid(Sy, Sx, PY, PX)
        assert g["pw"] % 64 == 0 and g["y0"][0] == 0 and g["x0"][0] == 0 and g["y0"][-1] + g["ph"] == Sy and g["x0"][-1] + g["pw"] == Sx
        assert np.ptp(np.diff(g["y0"])) <= 1 and np.ptp(np.diff(g["x0"])) <= 1            # evenly spaced, to the pixel
    g = localmotion.patch_geometry(1024, 1024, 5, 5, 6)
    assert (g["ph"], g["pw"]) == (205, 192)
    with pytest.raises(ValueError, match="window"):
        localmotion.patch_geometry(256, 320, 16, 3, 8)           # patches of 16 rows, a window of 17
    assert localmotion.patch_geometry(1024, 1024, 3, 3, 31)["pw"] == 320
    with pytest.raises(ValueError, match="window"):
        localmotion.patch_geometry(150, 64, 3, 3, 31)            # patches of 50 rows, a window of 63
    assert localmotion.patch_geometry(1024, 64, 3, 3, 31)["pw"] == 64                     # 63 columns fit the narrowest patch
    with pytest.raises(ValueError, match="do not fit"):
        localmotion.patch_geometry(256, 32, 3, 3, 2)             # a patch is 64 wide at least
    for bad in ((2, 3), (3, 17), (3,), (3, 3, 3), "3,3", (3.0, 3), (True, 3), None):
        with pytest.raises(ValueError, match="patch"):
            localmotion.check_patch_args(bad)
    for shift, iters in ((0, 4), (32, 4), (6, 0), (6, 101), (6.0, 4), (True, 4)):
        with pytest.raises(ValueError, match="patch_"):
            localmotion.check_patch_args((3, 3), shift, iters)
    assert localmotion.check_patch_args([3, 16]) == ((3, 16), 6, 4)
    assert localmotion.parse_patch("5,7") == (5, 7)
    for text in ("5", "5,7,9", "a,b", "5;7", ""):
        with pytest.raises(ValueError, match="PY,PX"):
            localmotion.parse_patch(text)


def test_design_matrix_and_fit():
    from spr_pick_amd import localmotion
    g = localmotion.patch_geometry(256, 320, 3, 3, 6)
    for Z in (4, 8):
        A = localmotion.design(Z, g["u"], g["v"])
        assert A.shape == (Z * 9, 18 + 9) and np.linalg.matrix_rank(A) == 27            # every unknown is observable
    assert np.linalg.matrix_rank(localmotion.design(3, g["u"], g["v"])) < 27              # a cubic in time needs four frames
    Z = 8
    A = localmotion.design(Z, g["u"], g["v"])
    assert not A[:9, :18].any() and np.array_equal(A[:9, 18:], np.eye(9))                 # frame 0 sees the offsets alone
    rng = np.random.RandomState(0)
    q, offsets = rng.standard_normal((3, 6)), rng.standard_normal(9)
    # row (f, n) is the field of frame f at the centre of patch n, plus that patch's offset
    cf = localmotion.frame_coefficients(q, Z)
    assert not cf[0].any() and np.allclose(cf[-1], q.sum(axis=0))                          # E_0 = 0, t = 1 at the last frame
    centres = localmotion.basis(g["u"][None, :], g["v"][:, None]).reshape(9, 6)
    m = (centres @ cf.T).T + offsets[None, :]
    assert np.allclose(A @ np.concatenate([q.ravel(), offsets]), m.ravel())
    assert np.allclose(cf, lm.frame_quadratics(q, Z)) and np.allclose(centres[4], lm.terms64(g["u"][1], g["v"][1]))
    keep = np.ones(Z * 9, dtype=bool)
    got, fitted = localmotion.fit_field(A, m.ravel(), keep)
    assert np.abs(got - q).max() < 1e-9 and np.abs(fitted - m.ravel()).max() < 1e-9
    spoiled = m.ravel().copy()
    keep[[5, 17, 40]] = False
    spoiled[~keep] = 1e3                                          # a dropped observation does not reach the fit
    got, _ = localmotion.fit_field(A, spoiled, keep)
    assert np.abs(got - q).max() < 1e-9
    assert localmotion.field_extreme(np.zeros((3, 6)), 8) == 0.0
    assert abs(localmotion.field_extreme(np.array([[2.0, 0, 0, 0, 0, 0]] * 3), 8) - 6.0) < 1e-12


def test_report_round_trip(tmp_path):
    from spr_pick_amd import localmotion
    rng = np.random.RandomState(1)
    Z, P = 5, 9
    local = {"geometry": localmotion.patch_geometry(256, 320, 3, 3, 6), "patch": (3, 3), "reduced": (256, 320), "iterations": 3,
             "dropped": 2, "qx": rng.standard_normal((3, 6)), "qy": rng.standard_normal((3, 6)),
             "measured": rng.standard_normal((Z, P, 2)), "fitted": rng.standard_normal((Z, P, 2))}
    path = str(tmp_path / "m_local.txt")
    localmotion.write_local(path, local)
    lines = [line.split("\t") for line in open(path).read().splitlines()]
    assert lines[0][0].startswith("#") and ["patches", "3", "3"] in lines and ["dropped", "2"] in lines
    rows = [row for row in lines if row[0] in "xy" and len(row) == 8]
    assert [(r[0], r[1]) for r in rows] == [("x", "1"), ("x", "2"), ("x", "3"), ("y", "1"), ("y", "2"), ("y", "3")]
    assert np.abs(np.array([[float(v) for v in r[2:]] for r in rows[:3]]) - local["qx"]).max() <= 5e-7
    table = lines[lines.index(["patch", "frame", "measured_dx", "measured_dy", "fitted_dx", "fitted_dy"]) + 1:]
    assert len(table) == Z * P and table[Z + 2][:2] == ["1", "2"]
    assert abs(float(table[Z + 2][2]) - local["measured"][2, 1, 1]) <= 5e-5 and abs(float(table[Z + 2][5]) - local["fitted"][2, 1, 0]) <= 5e-5


# ---- the parser and the library's refusals -------------------------------------------------------------------------------------
def test_parser_and_library_refusals(tmp_path):
    from spr_pick_amd import align, cli
    p = cli.build_parser()
    base = ["align", "--movies", "m", "--out", "o"]
    ns = p.parse_args(base + ["--patch", "3,5", "--patch_shift", "8", "--patch_iters", "2", "--ftbin", "2", "--dose", "1.2"])
    assert (ns.patch, ns.patch_shift, ns.patch_iters) == ("3,5", 8, 2)
    ns = p.parse_args(base)
    assert ns.patch is None and ns.patch_shift is None and ns.patch_iters is None
    for bad in (base + ["--patch", "2,3"], base + ["--patch", "3,17"], base + ["--patch", "3"], base + ["--patch", "3,3,3"],
                base + ["--patch", "a,b"], base + ["--patch"], base + ["--patch", "3,3", "--no_align"],
                base + ["--patch_shift", "6"], base + ["--patch_iters", "4"], base + ["--patch", "3,3", "--patch_shift", "0"],
                base + ["--patch", "3,3", "--patch_shift", "32"], base + ["--patch", "3,3", "--patch_iters", "0"],
                base + ["--patch", "3,3", "--patch_shift", "1.5"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    text = " ".join(p._subparsers._group_actions[0].choices["align"].format_help().split())
    for word in ("--patch PY,PX", "--patch_shift", "--patch_iters", "_local.txt", "Catmull-Rom", "0.88", "--no_align"):
        assert word in text, word
    not_covered = text[text.index("Not covered"):].split(".")[0]
    assert "local motion finer than" in not_covered and "polishing" in not_covered
    # the library refuses before it reads anything
    movies = str(tmp_path / "none")
    for kw, word in ((dict(patch=(3, 3), no_align=True), "no_align"), (dict(patch=(2, 3)), "patch must be"),
                     (dict(patch_shift=6), "give patch"), (dict(patch_iters=4), "give patch"),
                     (dict(patch=(3, 3), patch_shift=40), "patch_shift"), (dict(patch=(3, 3), patch_iters=0), "patch_iters")):
        with pytest.raises(ValueError, match=word):
            align.align_dataset(movies, str(tmp_path / "out"), **kw)
        with pytest.raises(ValueError, match=word):
            align.align_movie(movies, **kw)
    assert not os.path.exists(str(tmp_path / "out"))


def test_names_in_header_binding_and_torch_library():
    from conftest import ROOT
    from torch._subclasses.fake_tensor import FakeTensorMode
    from spr_pick_amd import _lib, localmotion, torch_ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sprk.h")).read(), flags=re.S)
    assert "sprk_align_warp" in set(re.findall(r"\b(sprk_[a-z0-9_]+)\s*\(", text))
    assert re.search(r"#define SPRK_ABI_VERSION 430\b", text) and _lib.ABI_VERSION == 430
    assert re.search(r"#define SPRK_WARP_MAX_SHIFT 16\b", text)
    assert torch_ops.WARP_MAX_SHIFT == localmotion.MAX_FIELD == lm.MAX_SHIFT == 16 and torch_ops.WARP_TERMS == 6
    assert "sprk_align_warp" in _lib.EXPORTS
    L = _lib.lib()
    assert hasattr(L, "sprk_align_warp") and L.sprk_version() == 430
    assert "align_warp" in torch_ops.registered() and hasattr(torch.ops.sprk, "align_warp")
    makefile = open(os.path.join(ROOT, "spr_pick_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bwarp\.hip\b", makefile, flags=re.M)
    assert re.search(r"warp\.o: CXXFLAGS \+= -ffp-contract=off", makefile)

    # refusals come before anything touches the device: the pointers are never dereferenced
    import ctypes
    six = (ctypes.c_float * 6)()
    P, Q = 0x10000, 0x20000

    def call(src=P, ny=70, nx=90, cy=six, cx=six, y=Q, first=1):
        return L.sprk_align_warp(src, ny, nx, cy, cx, y, first, None)
    before = L.sprk_launch_count()
    cases = [(dict(src=None), b"null"), (dict(y=None), b"null"), (dict(cy=None), b"null"), (dict(cx=None), b"null"),
             (dict(ny=0), b"frame"), (dict(nx=0), b"frame"), (dict(ny=16385), b"frame"), (dict(nx=16385), b"frame"),
             (dict(src=P + 2), b"aligned"), (dict(y=Q + 1), b"aligned"), (dict(y=P), b"must not be src"),
             (dict(cy=(ctypes.c_float * 6)(0, float("nan"))), b"finite"), (dict(cx=(ctypes.c_float * 6)(0, 0, 0, 0, 0, float("-inf"))), b"finite")]
    for change, word in cases:
        assert call(**change) == -1, change
        err = L.sprk_last_error()
        assert err.startswith(b"align_warp: ") and word in err, (change, err)
    assert L.sprk_launch_count() == before

    with FakeTensorMode():
        src, y = torch.empty((70, 90), device="cuda"), torch.empty((70, 90), device="cuda")
        assert torch.ops.sprk.align_warp(src, ZERO, ZERO, y, True) is None
        for args, word in (((src, ZERO[:5], ZERO, y, True), "coefficients"), ((src, ZERO, ZERO, torch.empty((70, 91), device="cuda"), True), "y must be"),
                           ((src.double(), ZERO, ZERO, y, True), "float32"), ((src, [float("nan")] + ZERO[1:], ZERO, y, True), "finite"),
                           ((torch.empty((0, 90), device="cuda"), ZERO, ZERO, torch.empty((0, 90), device="cuda"), True), "frame")):
            with pytest.raises(_lib.SprkError, match=word):
                torch.ops.sprk.align_warp(*args)


# ---- the float64 model of the loop ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_runs():
    ny, nx = lm.MOVIE_SHAPE
    runs = []
    for seed, noise in lm.MOVIE_CASES:
        movie, spec, drift, q = lm.make_movie(ny, nx, lm.MOVIE_FRAMES, seed, noise)
        assert movie.dtype == np.int16 and np.abs(drift).max() <= 5.0 + 1e-9 and not q[:, :, 0].any()
        assert abs(np.abs(lm.local_displacement(q, ny, nx, lm.MOVIE_FRAMES)).max() - 3.0) < 1e-9
        est_drift, est_q, dropped, G = lm.estimate_movie(movie, *lm.PATCH)
        planted = lm.total_displacement(drift, q, ny, nx)
        local = lm.total_displacement(est_drift, est_q, ny, nx)
        whole = lm.total_displacement(est_drift, np.zeros_like(est_q), ny, nx)
        stats = (lm.sum_statistic(lm.corrected_sum(G, est_q), spec, local, planted),
                 lm.sum_statistic(lm.corrected_sum(G, None), spec, whole, planted))
        runs.append((lm.gauge_free_error(local, planted), lm.gauge_free_error(whole, planted), dropped, stats))
        print("seed %d, noise %.1f x signal: gauge-free worst error %.4f with the local field, %.4f whole-frame only, raw "
              "pixels; %d dropped; sum statistic %.4f / %.4f" % (seed, noise, *runs[-1][:3], *stats))
    return runs


def test_model_loop_recovers_the_planted_field(model_runs):
    from spr_pick_amd import align
    assert align.align_geometry(*lm.MOVIE_SHAPE) == lm.MOVIE_SHAPE                        # these movies are not reduced
    worst = max(r[0] for r in model_runs)
    assert lm.MODEL_WORST - 0.002 < worst <= lm.MODEL_WORST
    assert lm.GLOBAL_ONLY <= min(r[1] for r in model_runs) < lm.GLOBAL_ONLY + 0.01
    assert 1.5 * lm.MODEL_WORST < 0.5 * lm.GLOBAL_ONLY


def test_model_loop_drops_no_observation(model_runs):
    assert [r[2] for r in model_runs] == [0, 0, 0]


def test_model_sums_separate_local_from_whole_frame(model_runs):
    for (_, _, _, (s_local, s_whole)), (want_local, want_whole) in zip(model_runs, lm.SUM_STATISTIC):
        assert abs(s_local - want_local) < 5e-4 and abs(s_whole - want_whole) < 5e-4
        assert 1.0 - s_local < 0.5 * (1.0 - s_whole)             # the local field removes more than half of what the blur costs
