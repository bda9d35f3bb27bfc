"""GPU: local motion correction (csrc/warp.hip, ``torch.ops.sprk.align_warp``, spr_pick_amd/localmotion.py):
the kernel bit for bit against the NumPy model of its contract (tests/localmotion_model.py), its refusals, and
``joint align --patch`` end to end on synthetic movies with a planted drift and a planted local field."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

import localmotion_model as lm
from extract_model import write_raw_mrc

pytestmark = pytest.mark.gpu
APIX = 1.5

ZERO = [0.0] * 6
# a full quadratic per axis that passes +-16 in opposite corners: the clamp engages with both signs on either axis, and
# the taps wrap over all four edges
WILD_Y, WILD_X = [0.3, 25.0, 18.0, 6.0, -9.0, 4.0], [-0.7, -30.0, 22.0, -5.0, 8.0, 3.0]
FIELDS = {"zero": (ZERO, ZERO), "integer": ([3.0] + ZERO[1:], [-2.0] + ZERO[1:]), "half": ([0.5] + ZERO[1:], [0.5] + ZERO[1:]),
          "wild": (WILD_Y, WILD_X)}
# the taps wrap more than once; ragged tiles; exact tiles; two tiles a side with a ragged second
SHAPES = [(1, 1), (3, 5), (17, 64), (37, 45), (64, 256), (70, 130)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def frame(shape, seed):
    return (np.random.RandomState(seed).standard_normal(shape) * 30).astype(np.float32)


def device_warp(src, cy, cx, y=None):
    """into an output this test has filled with NaN when it is the first call, else on from ``y``"""
    from spr_pick_amd import torch_ops  # noqa: F401  (registers torch.ops.sprk)
    out = torch.full(src.shape, float("nan"), device="cuda") if y is None else torch.from_numpy(y).cuda()
    torch.ops.sprk.align_warp(torch.from_numpy(src).cuda(), cy, cx, out, y is None)
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("field", sorted(FIELDS))
def test_kernel_matches_the_model_bit_for_bit(shape, field):
    cy, cx = FIELDS[field]
    a, b = frame(shape, 1), frame(shape, 2)
    want = lm.warp(a, cy, cx)
    got = device_warp(a, cy, cx)
    assert np.array_equal(bits(got), bits(want))
    if field == "zero":
        assert np.array_equal(got, a)                            # the identity: the weights are (-0, 1, 0, 0)
    if field == "integer":
        assert np.array_equal(got, np.roll(a, (-3, 2), axis=(0, 1)))          # out(i, j) = src(i + 3, j - 2)
    if field == "wild" and min(shape) > 16:
        sy, sx = lm.shifts(cy, *shape), lm.shifts(cx, *shape)
        assert sy.min() == -16 and sy.max() == 16 and sx.min() == -16 and sx.max() == 16
    # a second frame on top: one add per pixel
    second = device_warp(b, cx, cy, got)
    assert np.array_equal(bits(second), bits(lm.warp(b, cx, cy, want, first=False)))


def test_large_indices_cost_no_weight_bits():
    """4100 x 4100: the coordinates reach 4099 and the flat index 2^24; the fraction of a tap comes from the shift alone"""
    n = 4100
    rng = np.random.RandomState(7)
    src = (rng.standard_normal((n, n)) * 30).astype(np.float32)
    cy, cx = (rng.uniform(-1, 1, 6) * [0.5, 2, 2, 4, 4, 4]).tolist(), (rng.uniform(-1, 1, 6) * [0.5, 2, 2, 4, 4, 4]).tolist()
    got = device_warp(src, cy, cx)
    every = np.arange(n)
    for strip in (np.arange(0, 6), np.arange(2045, 2051), np.arange(n - 6, n)):
        assert np.array_equal(bits(got[strip]), bits(lm.warp(src, cy, cx, rows=strip, cols=every)))
        assert np.array_equal(bits(got[:, strip]), bits(lm.warp(src, cy, cx, rows=every, cols=strip)))


def test_refusals_launch_nothing():
    from spr_pick_amd import _lib, torch_ops  # noqa: F401  (registers torch.ops.sprk)
    L = _lib.lib()
    src = torch.from_numpy(frame((20, 70), 3)).cuda()
    y = torch.full((20, 70), float("nan"), device="cuda")
    torch.cuda.synchronize()
    before = L.sprk_launch_count()
    nan, inf = float("nan"), float("inf")
    cases = [((src.double(), ZERO, ZERO, y, True), "float32"), ((src[0], ZERO, ZERO, y[0], True), "float32"),
             ((src, ZERO[:5], ZERO, y, True), "coefficients"), ((src, ZERO, ZERO + [0.0], y, True), "coefficients"),
             ((src, [0.0, nan, 0.0, 0.0, 0.0, 0.0], ZERO, y, True), "finite"),
             ((src, ZERO, [0.0, 0.0, 0.0, 0.0, 0.0, -inf], y, True), "finite"),
             ((src, [1e39, 0.0, 0.0, 0.0, 0.0, 0.0], ZERO, y, True), "finite"),                       # not finite in float32
             ((src, ZERO, ZERO, y[:, :69].contiguous(), True), "y must be"), ((src, ZERO, ZERO, y.cpu(), True), "y must be"),
             ((src, ZERO, ZERO, y.double(), True), "y must be"),
             ((src.t(), ZERO, ZERO, torch.empty((70, 20), device="cuda"), True), "contiguous"),
             ((src, ZERO, ZERO, src, False), "must not be src")]
    for args, word in cases:
        with pytest.raises(_lib.SprkError, match=word):
            torch.ops.sprk.align_warp(*args)
    # the C ABI refuses the same, and sizes the operator cannot state
    six = (ctypes.c_float * 6)()
    bad = (ctypes.c_float * 6)(0, 0, float("inf"), 0, 0, 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for args, word in (((None, 20, 70, six, six, y.data_ptr(), 1), b"null"), ((src.data_ptr(), 20, 70, None, six, y.data_ptr(), 1), b"null"),
                       ((src.data_ptr(), 0, 70, six, six, y.data_ptr(), 1), b"frame"),
                       ((src.data_ptr(), 20, 16385, six, six, y.data_ptr(), 1), b"frame"),
                       ((src.data_ptr(), 20, 70, six, bad, y.data_ptr(), 1), b"finite"),
                       ((src.data_ptr() + 2, 20, 70, six, six, y.data_ptr(), 1), b"aligned"),
                       ((src.data_ptr(), 20, 70, six, six, src.data_ptr(), 1), b"must not be src")):
        assert L.sprk_align_warp(*args, stream) == -1, args
        assert L.sprk_last_error().startswith(b"align_warp: ") and word in L.sprk_last_error(), L.sprk_last_error()
    torch.cuda.synchronize()
    assert L.sprk_launch_count() == before and bool(torch.isnan(y).all())
    torch.ops.sprk.align_warp(src, ZERO, ZERO, y, True)
    assert L.sprk_launch_count() == before + 1 and torch.equal(y, src)        # one launch per frame


# ---- end to end ----------------------------------------------------------------------------------------------------------------
# The device's field against the float64 model's, over all pixels and frames, gauge-free as the recovery error is.  Both
# loops measure the same patches with the same windows and solve the same least squares; the device's warps and
# correlations are fp32 and its whole-frame shifts differ from the model's by about 0.0001 pixel (tests/test_gpu_align.py).
# Measured on an MI355X over lm.MOVIE_CASES: 0.0001 raw pixel in every case, both loops running their four iterations; the
# bound is ten times that.  (A loop that stopped an iteration before the other would move a patch-centre value by up to the
# tolerance of 0.01 pixel; that does not happen on these cases, and the kernels are deterministic.)
DEVICE_FIELD_MEASURED = 0.0001
DEVICE_VS_MODEL_FIELD = 10 * DEVICE_FIELD_MEASURED

_cache = {}


def write_movie(path, movie, apix):
    """an MRC stack of the movie's own sample type whose header states the pixel size"""
    write_raw_mrc(path, movie)
    Z, ny, nx = movie.shape
    with open(path, "r+b") as f:
        f.seek(28)
        f.write(struct.pack("<3i3f", nx, ny, Z, apix * nx, apix * ny, apix * Z))


def read_shifts(path):
    rows = [line.split("\t") for line in open(path).read().splitlines()]
    assert rows[0] == ["frame", "dx", "dy"] and [int(r[0]) for r in rows[1:]] == list(range(len(rows) - 1))
    return np.array([[float(r[1]), float(r[2])] for r in rows[1:]])


def case_data(case):
    """the movie of a case and the float64 model's run on it, computed once"""
    if case not in _cache:
        ny, nx = lm.MOVIE_SHAPE
        movie, spec, drift, q = lm.make_movie(ny, nx, lm.MOVIE_FRAMES, *lm.MOVIE_CASES[case])
        m_drift, m_q, m_dropped, _ = lm.estimate_movie(movie, *lm.PATCH)
        _cache[case] = (movie, spec, drift, q, m_drift, m_q, m_dropped)
    return _cache[case]


def read_local(path):
    """{name}_local.txt -> (q [2, 3, 6] (y, x), {key: [fields]}, rows [[patch, frame, mdx, mdy, fdx, fdy]])"""
    lines = [line.split("\t") for line in open(path).read().splitlines() if not line.startswith("#")]
    at = lines.index(["axis", "k", "c_1", "c_u", "c_v", "c_uu", "c_uv", "c_vv"])
    head = {row[0]: row[1:] for row in lines[:at]}
    q = np.zeros((2, 3, 6))
    for row in lines[at + 1:at + 7]:
        q[{"y": 0, "x": 1}[row[0]], int(row[1]) - 1] = [float(v) for v in row[2:]]
    assert lines[at + 7] == ["patch", "frame", "measured_dx", "measured_dy", "fitted_dx", "fitted_dy"]
    return q, head, np.array([[float(v) for v in row] for row in lines[at + 8:]])


def run_align(tmp_path, movie, *flags):
    from spr_pick_amd import cli
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "movies"), exist_ok=True)
    write_movie(os.path.join(root, "movies", "mov.mrc"), movie, APIX)
    out = os.path.join(root, "out%d" % len(os.listdir(root)))
    return cli.start(["align", "--movies", os.path.join(root, "movies"), "--out", out, *flags]), out


@pytest.mark.parametrize("case", range(len(lm.MOVIE_CASES)))
def test_joint_align_patch_recovers_the_planted_field(case, tmp_path):
    from spr_pick_amd import micrograph_io
    movie, spec, drift, q, m_drift, m_q, m_dropped = case_data(case)
    Z, ny, nx = movie.shape
    res, out = run_align(tmp_path, movie, "--patch", "%d,%d" % lm.PATCH)
    assert sorted(os.listdir(out)) == ["images.txt", "mov.mrc", "mov_local.txt", "mov_shifts.txt"]
    local = res["mov"]["local"]
    got_q, head, rows = read_local(local["path"])
    assert np.abs(got_q - np.array([local["qy"], local["qx"]])).max() <= 5e-7      # the table holds six decimals
    assert head["patches"] == ["3", "3"] and head["dropped"] == ["0"] and local["dropped"] == 0 and m_dropped == 0
    assert local["patch"] == [3, 3] and 1 <= local["iterations"] <= 4 and rows.shape == (9 * Z, 6)
    assert head["patch_size"][:2] == ["85", "128"] and head["patch_rows"] == ["0", "86", "171"]
    assert head["patch_columns"] == ["0", "96", "192"]
    got_drift = read_shifts(os.path.join(out, "mov_shifts.txt"))
    planted = lm.total_displacement(drift, q, ny, nx)
    device = lm.total_displacement(got_drift, got_q, ny, nx)
    model = lm.total_displacement(m_drift, m_q, ny, nx)
    whole_frame = lm.total_displacement(got_drift, np.zeros_like(got_q), ny, nx)
    to_planted, to_model = lm.gauge_free_error(device, planted), lm.gauge_free_error(device, model)
    print("seed %d, noise %.1f: %d local iteration(s); gauge-free worst |device - planted| %.4f, |model - planted| %.4f, "
          "|device - model| %.4f, whole-frame only %.4f raw pixels"
          % (*lm.MOVIE_CASES[case], local["iterations"], to_planted, lm.gauge_free_error(model, planted), to_model,
             lm.gauge_free_error(whole_frame, planted)))
    # what the fit reports of itself: fitted and measured values of the patches agree to a fraction of a pixel
    print("worst |measured - fitted| over the patches %.4f raw pixels" % np.abs(rows[:, 2:4] - rows[:, 4:6]).max())
    total, header, _ = micrograph_io.parse_mrc(open(os.path.join(out, "mov.mrc"), "rb").read())
    assert header.mode == 2 and total.shape == (ny, nx)
    stat = lm.sum_statistic(total, spec, device, planted)
    s_local, s_global = lm.SUM_STATISTIC[case]
    print("sum statistic: device %.4f; model with the local field %.4f, whole-frame only %.4f" % (stat, s_local, s_global))
    assert to_planted <= 1.5 * lm.MODEL_WORST < 0.5 * lm.GLOBAL_ONLY
    assert to_model <= DEVICE_VS_MODEL_FIELD
    assert stat >= 0.5 * (s_local + s_global)
    # the anchor (a sample of about 900) stays out of the interpolation and comes back once, Z times: the mean of the sum is
    # the mean of the frames' sum, up to what a warp that is no rigid shift does to the mean of a texture
    assert abs(total.mean() - movie.astype(np.float64).sum(axis=0).mean()) < 0.5


def test_patch_composes_with_ftbin_and_dose_and_feeds_joint_ctf(tmp_path):
    from spr_pick_amd import cli, micrograph_io
    movie = case_data(0)[0]
    Z, ny, nx = movie.shape
    res, out = run_align(tmp_path, movie, "--patch", "3,3", "--patch_shift", "5", "--patch_iters", "2", "--ftbin", "2",
                         "--dose", "1.2")
    assert sorted(os.listdir(out)) == ["images.txt", "images_DW.txt", "mov.mrc", "mov_DW.mrc", "mov_local.txt", "mov_shifts.txt"]
    assert res["mov"]["shape"] == [ny // 2, nx // 2] and res["mov"]["local"]["iterations"] <= 2
    plain, header, _ = micrograph_io.parse_mrc(open(os.path.join(out, "mov.mrc"), "rb").read())
    weighted, _, _ = micrograph_io.parse_mrc(open(os.path.join(out, "mov_DW.mrc"), "rb").read())
    assert plain.shape == weighted.shape == (ny // 2, nx // 2) and abs(header.xlen / header.mx - 2 * APIX) < 1e-5
    assert np.isfinite(plain).all() and np.isfinite(weighted).all()
    # both sums carry the anchor once: their means are the mean of the frames' sum (the weight is 1 at the origin)
    mean = movie.astype(np.float64).sum(axis=0).mean()
    assert abs(plain.mean() - mean) < 0.5 and abs(weighted.mean() - mean) < 0.5
    fit = cli.start(["ctf", "--dataset", os.path.join(out, "images.txt"), "--out", os.path.join(str(tmp_path), "ctf"),
                     "--tile", "128"])
    assert sorted(fit) == ["mov"]


def test_without_the_flag_nothing_new_runs(tmp_path, monkeypatch):
    """no --patch: the sum and the table are those of the functions the command had before, and localmotion is not entered"""
    from spr_pick_amd import align, localmotion
    movie = case_data(0)[0]
    Z, ny, nx = movie.shape

    def never(*a, **k):
        raise AssertionError("localmotion entered without --patch")
    for name in ("estimate_field", "LocalMovie", "check_patch_args", "write_local"):
        monkeypatch.setattr(localmotion, name, never)
    res, out = run_align(tmp_path, movie)
    assert sorted(os.listdir(out)) == ["images.txt", "mov.mrc", "mov_shifts.txt"] and "local" not in res["mov"]
    path = os.path.join(str(tmp_path), "movies", "mov.mrc")
    with align.Movie(path) as m:
        h = m.header
        my, mx = align.ingest.resample_matrix(ny, ny, "cuda"), align.ingest.resample_matrix(nx, nx, "cuda")
        reduced = torch.empty((Z, ny, nx), dtype=torch.float32, device="cuda")
        for k in range(Z):
            red, _ = torch.ops.sprk.ingest_resample(m.frame(k), h.mode, ny, nx, ny, nx, my, mx)
            reduced[k] = red - red.mean()
        sy, sx, _ = align.estimate_shifts(reduced)
        want = align.sum_frames(m, ny, nx, sy, sx).cpu().numpy()
    align.write_sum(os.path.join(str(tmp_path), "want.mrc"), want, h, ny, nx)
    assert open(os.path.join(out, "mov.mrc"), "rb").read() == open(os.path.join(str(tmp_path), "want.mrc"), "rb").read()
    table = "frame\tdx\tdy\n" + "".join("%d\t%.4f\t%.4f\n" % (k, 0.0 - sx[k], 0.0 - sy[k]) for k in range(Z))
    assert open(os.path.join(out, "mov_shifts.txt")).read() == table
