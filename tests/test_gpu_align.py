"""GPU: whole-frame motion correction (csrc/align.hip, ``torch.ops.sprk.align_corr`` / ``align_accumulate``,
spr_pick_amd/align.py): both kernels bit for bit against the NumPy models of their contracts
(tests/align_model.py), the running sum within its a-priori bound, the padding and refusal rules of the C ABI, the
torch-built matrices against the NumPy ones, and ``joint align`` end to end on synthetic movies with planted drift."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

import align_model
from extract_model import write_raw_mrc

pytestmark = pytest.mark.gpu

EINVAL, EWORKSPACE = -1, -2


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def upload(img):
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(img).tobytes(), dtype=np.uint8).copy()).cuda()


def device_matrix(m):
    """a float32 [S, B] array -> the operand layout of ingest.resample_matrix(B, S, device)"""
    S, B = m.shape
    padded = np.zeros((-(-S // 16) * 16, -(-B // 4) * 4), dtype=np.float32)
    padded[:S, :B] = m
    return torch.from_numpy(padded).cuda()


# ---- align_corr ------------------------------------------------------------------------------------------------------------
def device_corr(a, r, R, tile=0):
    """through the C ABI, into an output this test has filled with NaN"""
    from spr_pick_amd import _lib
    L = _lib.lib()
    Z, Sy, Sx = a.shape
    n = 2 * R + 1
    da, dr = torch.from_numpy(a).cuda(), torch.from_numpy(r).cuda()
    cc = torch.full((Z, n, n), float("nan"), device="cuda")
    rc = L.sprk_align_corr(da.data_ptr(), dr.data_ptr(), Sy * Sx if r.ndim == 3 else 0, Z, Sy, Sx, R, tile, cc.data_ptr(),
                           _stream())
    assert rc == 0, L.sprk_last_error()
    return cc.cpu().numpy()


def corr_inputs(Z, Sy, Sx, shared, seed):
    rng = np.random.RandomState(seed)
    a = (rng.randn(Z, Sy, Sx) * 30).astype(np.float32)
    r = (rng.randn(*((Sy, Sx) if shared else (Z, Sy, Sx))) * 30).astype(np.float32)
    return a, r


# three chunks and every roll wraps; two chunks per row and a window taller than the frame (the rows roll modulo Sy); the
# full 63 x 63 tile on a frame just as tall; a shared reference, three chunks per row
CORR_CASES = [(1, 3, 64, 1, False), (3, 5, 128, 4, False), (2, 63, 64, 31, False), (2, 7, 192, 15, True)]


@pytest.mark.parametrize("Z,Sy,Sx,R,shared", CORR_CASES, ids=["%dx%dx%d-R%d%s" % (c[:4] + ("-shared" if c[4] else "",))
                                                              for c in CORR_CASES])
def test_corr_matches_the_model(Z, Sy, Sx, R, shared):
    a, r = corr_inputs(Z, Sy, Sx, shared, seed=Sy + R)
    want = align_model.corr(a, r, R)
    got = device_corr(a, r, R)
    differ = int((got != want).sum())
    print("%d frames of %dx%d, R %d: %d of %d values differ from the model" % (Z, Sy, Sx, R, differ, got.size))
    assert np.isfinite(got).all() and np.array_equal(got, want), (differ, float(np.abs(got - want).max()))
    op = torch.ops.sprk.align_corr(torch.from_numpy(a).cuda(), torch.from_numpy(r).cuda(), R)
    assert np.array_equal(op.cpu().numpy(), want)


def test_corr_every_tiling_gives_the_same_bytes():
    """a 41 x 41 window: nine tiles of 16 x 16 on one wave, four of 32 x 32 on two, one of 64 x 64 on four, and the choice
    the library makes itself"""
    from spr_pick_amd import torch_ops
    a, r = corr_inputs(2, 41, 64, False, seed=8)
    want = align_model.corr(a, r, 20)
    for tile in torch_ops.ALIGN_TILES:
        got = device_corr(a, r, 20, tile)
        assert np.array_equal(got, want), (tile, int((got != want).sum()))
        op = torch.ops.sprk.align_corr(torch.from_numpy(a).cuda(), torch.from_numpy(r).cuda(), 20, tile)
        assert np.array_equal(op.cpu().numpy(), want)


# ---- align_accumulate --------------------------------------------------------------------------------------------------------
def make_frames(mode, ny, nx, Z, seed):
    rng = np.random.RandomState(seed)
    if mode == 2:
        return [(rng.randn(ny, nx) * 100).astype(np.float32) for _ in range(Z)]
    info = np.iinfo(align_model.DTYPES[mode])
    frames = [rng.randint(info.min, info.max + 1, size=(ny, nx)).astype(align_model.DTYPES[mode]) for _ in range(Z)]
    frames[-1][-1, -1], frames[-1][0, -1] = info.min, info.max
    return frames


def make_matrices(ny, nx, by, bx, Z, seed):
    from spr_pick_amd import align
    d = np.random.RandomState(seed).uniform(-6, 6, size=(Z, 2))
    return [align.shift_matrix(ny, by, dy) for dy, _ in d], [align.shift_matrix(nx, bx, dx) for _, dx in d]


def device_accumulate(frames, Mys, Mxs, anchor, poison_y=True):
    """one call per frame through the C ABI: the workspace is this test's and full of NaN, and so is y before the first"""
    from spr_pick_amd import _lib
    L = _lib.lib()
    mode = align_model.MODE_OF[frames[0].dtype]
    ny, nx = frames[0].shape
    by, bx = Mys[0].shape[0], Mxs[0].shape[0]
    need = L.sprk_align_accumulate_ws_bytes(ny, nx, by, bx)
    assert need == ny * (-(-bx // 4) * 4) * 4
    y = torch.full((by, bx), float("nan") if poison_y else 0.0, device="cuda")
    for k, (img, My, Mx) in enumerate(zip(frames, Mys, Mxs)):
        ws = torch.full((need // 4 + 4096,), float("nan"), device="cuda")    # NaN well past the end of U as well
        raw, my, mx = upload(img), device_matrix(My), device_matrix(Mx)
        rc = L.sprk_align_accumulate(raw.data_ptr(), mode, ny, nx, by, bx, my.data_ptr(), my.shape[1], mx.data_ptr(),
                                     mx.shape[1], anchor, y.data_ptr(), 1 if k == 0 else 0, ws.data_ptr(), need, _stream())
        assert rc == 0, L.sprk_last_error()
    return y.cpu().numpy()


# float32; int16 with ragged K in both stages; uint16, shift only, three K chunks; int8
ACC_CASES = [(2, 16, 16, 16, 16, 2), (1, 37, 45, 12, 17, 3), (6, 70, 130, 70, 130, 2), (0, 66, 34, 20, 34, 2)]


@pytest.mark.parametrize("mode,ny,nx,by,bx,Z", ACC_CASES, ids=["mode%d-%dx%d-%dx%d-Z%d" % c for c in ACC_CASES])
def test_accumulate_matches_the_single_chain(mode, ny, nx, by, bx, Z):
    frames = make_frames(mode, ny, nx, Z, seed=ny)
    Mys, Mxs = make_matrices(ny, nx, by, bx, Z, seed=nx)
    anchor = 0.0 if mode == 2 else float(frames[0][0, 0])
    want = align_model.accumulate(frames, Mys, Mxs, anchor)
    got = device_accumulate(frames, Mys, Mxs, anchor)
    differ = int((got != want).sum())
    ratio = align_model.check_bound(got, frames, Mys, Mxs, anchor)
    print("mode %d, %d frames of %dx%d -> %dx%d: %d of %d pixels differ from the model, worst error / a-priori bound %.3g"
          % (mode, Z, ny, nx, by, bx, differ, got.size, ratio))
    assert np.isfinite(got).all() and np.array_equal(got, want), (differ, float(np.abs(got - want).max()))
    # the operator: the same bytes, y updated in place
    y = torch.full((by, bx), float("nan"), device="cuda")
    for k in range(Z):
        assert torch.ops.sprk.align_accumulate(upload(frames[k]), mode, ny, nx, by, bx, device_matrix(Mys[k]),
                                               device_matrix(Mxs[k]), anchor, y, k == 0) is None
    assert np.array_equal(y.cpu().numpy(), want)


def test_accumulate_first_overwrites_a_poisoned_sum():
    """`first` starts the chain at 0.0f and does not read y: a second call with `first` set on a sum full of NaN gives the
    bytes of that frame alone"""
    mode, ny, nx, by, bx, Z = ACC_CASES[1]
    frames = make_frames(mode, ny, nx, 2, seed=3)
    Mys, Mxs = make_matrices(ny, nx, by, bx, 2, seed=4)
    anchor = float(frames[0][0, 0])
    y = torch.zeros((by, bx), device="cuda")
    torch.ops.sprk.align_accumulate(upload(frames[0]), mode, ny, nx, by, bx, device_matrix(Mys[0]), device_matrix(Mxs[0]),
                                    anchor, y, True)
    y.fill_(float("nan"))
    torch.ops.sprk.align_accumulate(upload(frames[1]), mode, ny, nx, by, bx, device_matrix(Mys[1]), device_matrix(Mxs[1]),
                                    anchor, y, True)
    assert np.array_equal(y.cpu().numpy(), align_model.accumulate(frames[1:], Mys[1:], Mxs[1:], anchor))


def test_accumulate_one_frame_is_ingest_resample():
    """Z = 1, zero shift, float32: the bytes of ingest_resample on the same matrices (70 x 90 -> 23 x 31)"""
    from spr_pick_amd import ingest
    ny, nx, by, bx = 70, 90, 23, 31
    img = make_frames(2, ny, nx, 1, seed=6)[0]
    raw, my, mx = upload(img), ingest.resample_matrix(ny, by, "cuda"), ingest.resample_matrix(nx, bx, "cuda")
    want, _ = torch.ops.sprk.ingest_resample(raw, 2, ny, nx, by, bx, my, mx)
    y = torch.full((by, bx), float("nan"), device="cuda")
    torch.ops.sprk.align_accumulate(raw, 2, ny, nx, by, bx, my, mx, 0.0, y, True)
    assert torch.equal(y, want) and bool(y.abs().sum() > 0)


def test_accumulate_refusals_launch_nothing():
    from spr_pick_amd import _lib, ingest
    L = _lib.lib()
    ny, nx, by, bx = 70, 90, 23, 31
    img = make_frames(1, ny, nx, 1, seed=7)[0]
    raw, my, mx = upload(img), ingest.resample_matrix(ny, by, "cuda"), ingest.resample_matrix(nx, bx, "cuda")
    y = torch.zeros(by, bx, device="cuda")
    need = L.sprk_align_accumulate_ws_bytes(ny, nx, by, bx)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    good = dict(raw=raw.data_ptr(), mode=1, ny=ny, nx=nx, by=by, bx=bx, my=my.data_ptr(), ldmy=my.shape[1], mx=mx.data_ptr(),
                ldmx=mx.shape[1], anchor=float(img[0, 0]), y=y.data_ptr(), first=1, ws=ws.data_ptr(), ws_bytes=need)

    def call(**change):
        a = dict(good, **change)
        return L.sprk_align_accumulate(a["raw"], a["mode"], a["ny"], a["nx"], a["by"], a["bx"], a["my"], a["ldmy"], a["mx"],
                                       a["ldmx"], a["anchor"], a["y"], a["first"], a["ws"], a["ws_bytes"], _stream())

    torch.cuda.synchronize()
    before = L.sprk_launch_count()
    cases = [(dict(ws_bytes=need - 1), EWORKSPACE, b"workspace"), (dict(ws=None, ws_bytes=0), EWORKSPACE, b"workspace"),
             (dict(mode=3), EINVAL, b"mode"), (dict(by=71), EINVAL, b"resampled"), (dict(ldmy=68), EINVAL, b"ldmy"),
             (dict(ldmx=93), EINVAL, b"ldmx"), (dict(anchor=0.5), EINVAL, b"anchor"), (dict(anchor=40000.0), EINVAL, b"anchor"),
             (dict(mode=2, anchor=1.0), EINVAL, b"anchor"), (dict(y=None), EINVAL, b"null"),
             (dict(y=y.data_ptr() + 4), EINVAL, b"aligned"), (dict(ws=ws.data_ptr() + 8), EINVAL, b"aligned")]
    for change, code, word in cases:
        assert call(**change) == code, (change, L.sprk_last_error())
        assert word in L.sprk_last_error(), (change, L.sprk_last_error())
    assert L.sprk_launch_count() == before and not y.any()
    assert call() == 0, L.sprk_last_error()
    assert L.sprk_launch_count() == before + 2                   # the two stages
    assert np.array_equal(y.cpu().numpy(),
                          align_model.accumulate([img], [my.cpu().numpy()[:by, :ny]], [mx.cpu().numpy()[:bx, :nx]], float(img[0, 0])))


# ---- the matrices built on the device ----------------------------------------------------------------------------------------
# What float64 sin and cos on the device differ by from NumPy's, through the quotient of the Dirichlet kernel: measured on an
# MI355X over these cases, the largest |device - NumPy| entry was 1.11e-16 (entries up to 1); the bound is 4 x that.
MATRIX_TOLERANCE = 4.5e-16
MATRIX_CASES = [(1000, 1000, -0.5), (1001, 1001, 17.25), (4096, 1024, 3.37), (997, 331, -2.125), (130, 70, 0.0), (64, 64, 0.0)]


def test_device_matrices_match_numpy():
    from spr_pick_amd import align
    worst = 0.0
    for B, S, delta in MATRIX_CASES:
        want = align.shift_matrix64(B, S, delta)
        got = align.shift_matrix_device64(B, S, delta, "cuda").cpu().numpy()
        err = float(np.abs(got - want).max())
        worst = max(worst, err)
        print("shift_matrix(%d, %d, %g): largest |device - NumPy| = %.3g" % (B, S, delta, err))
        t = align.shift_matrix(B, S, delta, "cuda")
        assert tuple(t.shape) == (-(-S // 16) * 16, -(-B // 4) * 4) and t.dtype == torch.float32
        t = t.cpu().numpy()
        assert not t[S:].any() and not t[:, B:].any()
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert (np.abs(t[:S, :B] - want) <= 0.5 * ulp + MATRIX_TOLERANCE).all()      # the float32 nearest to (nearly) the same number
    assert worst <= MATRIX_TOLERANCE, worst
    assert MATRIX_TOLERANCE < 1e-6 * 2.0 ** -24                  # far below a float32 ulp of entries that matter
    assert np.array_equal(align.shift_matrix(64, 64, 0.0, "cuda").cpu().numpy(), np.eye(64, dtype=np.float32))


# ---- end to end ----------------------------------------------------------------------------------------------------------------
# The device's shifts against the float64 model's: the correlation windows are fp32 chains of 81920 products, the parabola
# divides differences of their values, and either loop may stop one iteration before the other, which moves a component by
# less than the loop's tolerance (0.01 reduced pixel = 0.01 raw pixel here).  Measured on an MI355X over the cases of
# align_model.MOVIE_CASES: at most 0.0001 raw pixel, with the same number of iterations on both sides; the bound is the
# loop's tolerance plus 4 x that.
DEVICE_VS_MODEL = 0.01 + 0.0004
APIX = 1.5


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


def correlation(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


@pytest.fixture(scope="module")
def movies():
    ny, nx = align_model.MOVIE_SHAPE
    out = []
    for seed, noise in align_model.MOVIE_CASES:
        movie, spec, drift = align_model.make_movie(ny, nx, align_model.MOVIE_FRAMES, seed, noise)
        out.append((movie, spec, drift, align_model.estimate_movie(movie, ny, nx)))
    return out


@pytest.mark.parametrize("case", range(len(align_model.MOVIE_CASES)))
def test_joint_align_recovers_the_planted_drift(case, movies, tmp_path):
    from spr_pick_amd import cli, micrograph_io
    movie, spec, drift, model = movies[case]
    Z, ny, nx = movie.shape
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "movies"))
    write_movie(os.path.join(root, "movies", "mov.mrc"), movie, APIX)
    out = os.path.join(root, "sums")
    res = cli.start(["align", "--movies", os.path.join(root, "movies"), "--out", out])
    assert sorted(os.listdir(out)) == ["images.txt", "mov.mrc", "mov_shifts.txt"]
    got = read_shifts(os.path.join(out, "mov_shifts.txt"))
    assert got.shape == (Z, 2) and np.abs(got.mean(axis=0)).max() <= 1e-4
    assert np.abs(got - np.array(res["mov"]["shifts"])).max() <= 5e-5          # the table holds four decimals
    to_model, to_planted = float(np.abs(got - model).max()), float(np.abs(got - drift).max())
    print("seed %d, noise %.1f: %d iteration(s); worst |device - model| %.4f, |device - planted| %.4f, |model - planted| %.4f "
          "raw pixels" % (*align_model.MOVIE_CASES[case], res["mov"]["iterations"], to_model, to_planted,
                          float(np.abs(model - drift).max())))
    assert res["mov"]["edge_frames"] == [] and res["mov"]["frames"] == Z and res["mov"]["shape"] == [ny, nx]
    assert to_model <= DEVICE_VS_MODEL
    assert to_planted <= 1.5 * align_model.MODEL_WORST < 0.5

    total, header, _ = micrograph_io.parse_mrc(open(os.path.join(out, "mov.mrc"), "rb").read())
    assert header.mode == 2 and total.shape == (ny, nx) and (header.mx, header.my) == (nx, ny)
    assert abs(header.xlen / header.mx - APIX) < 1e-5 and abs(header.ylen / header.my - APIX) < 1e-5
    plain = cli.start(["align", "--movies", os.path.join(root, "movies"), "--out", os.path.join(root, "plain"), "--no_align"])
    assert not np.array(plain["mov"]["shifts"]).any() and plain["mov"]["iterations"] == 0
    unaligned, _, _ = micrograph_io.parse_mrc(open(os.path.join(root, "plain", "mov.mrc"), "rb").read())
    # zero shift, no crop: the identity matrices, so the sum is the plain sum of the frames (exact in fp32 at this size)
    assert np.array_equal(unaligned, movie.astype(np.float64).sum(axis=0).astype(np.float32))
    c_aligned, c_plain = correlation(total, spec), correlation(unaligned, spec)
    print("correlation with the specimen: aligned %.4f, unaligned %.4f" % (c_aligned, c_plain))
    assert c_aligned > c_plain + 0.02
    # the aligned sum is the specimen again: every frame laid back on the mean position
    assert abs(total.mean() - movie.astype(np.float64).sum(axis=0).mean()) < 1e-2


def test_the_sum_feeds_the_rest_of_the_chain(movies, tmp_path):
    """`joint align --ftbin 2` writes the cropped sum at twice the pixel size; `joint ctf` (which takes the pixel size from
    that header) and `joint bin --ftbin 2` read the sums"""
    from spr_pick_amd import cli, micrograph_io
    movie = movies[0][0]
    Z, ny, nx = movie.shape
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "movies"))
    for name in ("a", "b"):
        write_movie(os.path.join(root, "movies", name + ".mrc"), movie, APIX)
    table = os.path.join(root, "movies.txt")
    open(table, "w").write("image_name\tpath\n" + "".join("%s\t%s\n" % (n, os.path.join(root, "movies", n + ".mrc")) for n in "ab"))
    out = os.path.join(root, "sums")
    res = cli.start(["align", "--movies", table, "--out", out, "--ftbin", "2", "--max_shift", "8", "--iters", "2"])
    assert sorted(res) == ["a", "b"] and res["a"]["shape"] == [ny // 2, nx // 2] and res["a"]["shifts"] == res["b"]["shifts"]
    assert res["a"]["iterations"] <= 2
    total, header, _ = micrograph_io.parse_mrc(open(os.path.join(out, "a.mrc"), "rb").read())
    assert total.shape == (ny // 2, nx // 2) and abs(header.xlen / header.mx - 2 * APIX) < 1e-5
    fit = cli.start(["ctf", "--dataset", out, "--out", os.path.join(root, "ctf"), "--tile", "128"])
    assert sorted(fit) == ["a", "b"] and os.path.exists(os.path.join(root, "ctf", "micrographs_ctf.star"))
    binned = cli.start(["bin", "--dataset", os.path.join(out, "images.txt"), "--ftbin", "2", "--out", os.path.join(root, "bin")])
    assert binned["geometry"] == {"a": (ny // 4, nx // 4, ny // 2, nx // 2), "b": (ny // 4, nx // 4, ny // 2, nx // 2)}
