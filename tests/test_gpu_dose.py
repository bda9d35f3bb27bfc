"""GPU: dose-weighted movie sums (csrc/alignsum.hip, ``torch.ops.sprk.align_spectrum`` / ``align_synthesize``,
spr_pick_amd/dose.py): both entry points bit for bit against the NumPy models of their contracts
(tests/dose_model.py) and within the a-priori bound, against ``align_accumulate`` with pure phases, the padding and refusal
rules of the C ABI, the torch-built filter against the NumPy one, and ``joint align --dose`` end to end on synthetic movies
of a specimen that the exposure damages."""
import ctypes
import os

import numpy as np
import pytest
import torch

import align_model
import dose_model
from test_gpu_align import device_accumulate, make_frames, upload, write_movie

pytestmark = pytest.mark.gpu

EINVAL, EWORKSPACE = -1, -2


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def padded(m):
    """a float32 array -> the device operand: columns rounded up to a multiple of 4 with zeros"""
    out = np.zeros((m.shape[0], -(-m.shape[1] // 4) * 4), dtype=np.float32)
    out[:, :m.shape[1]] = m
    return torch.from_numpy(out).cuda()


def matrices32(ny, nx, by, bx):
    from spr_pick_amd import dose
    return [m.astype(np.float32) for m in dose.spectrum_matrices64(ny, nx, by, bx)]


def random_filters(Ku, Hs, Z, seed):
    """random complex filters, not only dose weights: float32 [2Ku, Hs] each"""
    rng = np.random.RandomState(seed)
    return [rng.uniform(-1.5, 1.5, size=(2 * Ku, Hs)).astype(np.float32) for _ in range(Z)]


def device_sum(frames, W, gs, anchor, by, bx, poison=True):
    """one align_spectrum call per frame and one align_synthesize through the C ABI: the workspaces are this test's and full
    of NaN, and so are F before the first call and the padding columns of g -> (F [2Ku, Hs], Y [by, bx])"""
    from spr_pick_amd import _lib
    L = _lib.lib()
    mode = align_model.MODE_OF[frames[0].dtype]
    ny, nx = frames[0].shape
    Ku, Hs = W[1].shape[0] // 2, W[0].shape[0] // 2
    ldv = -(-Hs // 4) * 4
    need = L.sprk_align_spectrum_ws_bytes(ny, nx, Hs)
    assert need == 2 * ny * ldv * 4
    w1, w2, w3, w4 = (padded(m) for m in W)
    F = torch.full((2 * Ku, ldv), float("nan") if poison else 0.0, device="cuda")
    for k, (img, g) in enumerate(zip(frames, gs)):
        ws = torch.full((need // 4 + 4096,), float("nan"), device="cuda")      # NaN well past the end of V as well
        dg = torch.full((2 * Ku, ldv), float("nan"), device="cuda")
        dg[:, :Hs] = torch.from_numpy(g).cuda()
        raw = upload(img)
        rc = L.sprk_align_spectrum(raw.data_ptr(), mode, ny, nx, Ku, Hs, w1.data_ptr(), w2.data_ptr(), dg.data_ptr(), anchor,
                                   F.data_ptr(), 1 if k == 0 else 0, ws.data_ptr(), need, _stream())
        assert rc == 0, L.sprk_last_error()
    need = L.sprk_align_synthesize_ws_bytes(by, Hs)
    assert need == by * (-(-2 * Hs // 4) * 4) * 4
    ws = torch.full((need // 4 + 4096,), float("nan"), device="cuda")
    y = torch.full((by, bx), float("nan"), device="cuda")
    rc = L.sprk_align_synthesize(F.data_ptr(), Ku, Hs, by, bx, w3.data_ptr(), w4.data_ptr(), y.data_ptr(), ws.data_ptr(), need,
                                 _stream())
    assert rc == 0, L.sprk_last_error()
    return F.cpu().numpy()[:, :Hs], y.cpu().numpy()


# float32; int16, odd sizes and ragged K in every stage; uint16, even and uncropped (the shared +-h rows), more than one
# 64-tile in every dimension, Hs = 66 and three K chunks in every stage; int8
CASES = [(2, 16, 16, 16, 16, 2), (1, 37, 45, 12, 17, 3), (6, 70, 130, 70, 130, 2), (0, 66, 34, 20, 34, 2)]


@pytest.mark.parametrize("mode,ny,nx,by,bx,Z", CASES, ids=["mode%d-%dx%d-%dx%d-Z%d" % c for c in CASES])
def test_spectrum_and_synthesize_match_the_model(mode, ny, nx, by, bx, Z):
    frames = make_frames(mode, ny, nx, Z, seed=ny)
    W = matrices32(ny, nx, by, bx)
    Ku, Hs = W[1].shape[0] // 2, W[0].shape[0] // 2
    gs = random_filters(Ku, Hs, Z, seed=nx)
    anchor = 0.0 if mode == 2 else float(frames[0][0, 0])
    want_F = dose_model.spectrum(frames, W[0], W[1], gs, anchor)
    want_Y = dose_model.synthesize(want_F, W[2], W[3])
    got_F, got_Y = device_sum(frames, W, gs, anchor, by, bx)
    ref, bound = dose_model.apriori_bound([align_model.operand(f, anchor) for f in frames], W, gs)
    ratio = float((np.abs(got_Y - ref) / bound).max())
    print("mode %d, %d frames of %dx%d -> %dx%d (Ku %d, Hs %d): %d of %d spectrum values and %d of %d pixels differ from the "
          "model, worst error / a-priori bound %.3g" % (mode, Z, ny, nx, by, bx, Ku, Hs, int((got_F != want_F).sum()), got_F.size,
                                                        int((got_Y != want_Y).sum()), got_Y.size, ratio))
    assert np.isfinite(got_F).all() and np.array_equal(got_F, want_F), float(np.abs(got_F - want_F).max())
    assert np.isfinite(got_Y).all() and np.array_equal(got_Y, want_Y), float(np.abs(got_Y - want_Y).max())
    assert ratio < 1
    # the operators: the same bytes, F updated in place
    w1, w2, w3, w4 = (padded(m) for m in W)
    F = torch.full((2 * Ku, -(-Hs // 4) * 4), float("nan"), device="cuda")
    for k in range(Z):
        assert torch.ops.sprk.align_spectrum(upload(frames[k]), mode, ny, nx, w1, w2, padded(gs[k]), anchor, F, k == 0) is None
    assert np.array_equal(F.cpu().numpy()[:, :Hs], want_F)
    assert np.array_equal(torch.ops.sprk.align_synthesize(F, by, bx, w3, w4).cpu().numpy(), want_Y)


def test_first_overwrites_a_poisoned_spectrum():
    """`first` starts F at 0.0f and does not read it: a second call with `first` set on a spectrum full of NaN gives the
    bytes of that frame alone"""
    mode, ny, nx, by, bx, _ = CASES[1]
    frames = make_frames(mode, ny, nx, 2, seed=3)
    W = matrices32(ny, nx, by, bx)
    Ku, Hs = W[1].shape[0] // 2, W[0].shape[0] // 2
    gs = random_filters(Ku, Hs, 2, seed=4)
    anchor = float(frames[0][0, 0])
    w1, w2 = padded(W[0]), padded(W[1])
    F = torch.zeros((2 * Ku, -(-Hs // 4) * 4), device="cuda")
    torch.ops.sprk.align_spectrum(upload(frames[0]), mode, ny, nx, w1, w2, padded(gs[0]), anchor, F, True)
    F.fill_(float("nan"))
    torch.ops.sprk.align_spectrum(upload(frames[1]), mode, ny, nx, w1, w2, padded(gs[1]), anchor, F, True)
    assert np.array_equal(F.cpu().numpy()[:, :Hs], dose_model.spectrum(frames[1:], W[0], W[1], gs[1:], anchor))


@pytest.mark.parametrize("mode,ny,nx,by,bx,Z", CASES[1:3], ids=["mode%d-%dx%d-%dx%d-Z%d" % c for c in CASES[1:3]])
def test_pure_phases_agree_with_align_accumulate(mode, ny, nx, by, bx, Z):
    """g = the phases of the shifts alone: the sum of align_accumulate on the same frames and shifts, each side within its
    own a-priori bound of the same operator"""
    from spr_pick_amd import align, dose
    frames = make_frames(mode, ny, nx, Z, seed=ny + 1)
    shifts = np.random.RandomState(nx).uniform(-6, 6, size=(Z, 2))
    anchor = float(frames[0][0, 0])
    W = matrices32(ny, nx, by, bx)
    Hs = bx // 2 + 1
    gs = [dose.pack_filter(dose.frame_filter64(1.0, ny, nx, by, bx, dy, dx))[:, :Hs] for dy, dx in shifts]
    _, got = device_sum(frames, W, gs, anchor, by, bx)
    Mys, Mxs = [align.shift_matrix(ny, by, dy) for dy, _ in shifts], [align.shift_matrix(nx, bx, dx) for _, dx in shifts]
    acc = device_accumulate(frames, Mys, Mxs, anchor)
    Ds = [align_model.operand(f, anchor) for f in frames]
    _, bound_f = dose_model.apriori_bound(Ds, W, gs)
    bound_a = 0.0
    for D, My, Mx in zip(Ds, Mys, Mxs):
        bound_a = bound_a + np.abs(My.astype(np.float64)) @ np.abs(D.astype(np.float64)) @ np.abs(Mx.astype(np.float64)).T
    bound_a = (Z * ny + nx + 4) * 2.0 ** -24 * bound_a           # align_model.check_bound's
    ratio = float((np.abs(got.astype(np.float64) - acc) / (bound_f + bound_a)).max())
    print("%d frames of %dx%d -> %dx%d: |Fourier path - align_accumulate| at most %.3g of the two bounds' sum"
          % (Z, ny, nx, by, bx, ratio))
    assert ratio < 1


def test_refusals_launch_nothing():
    from spr_pick_amd import _lib
    L = _lib.lib()
    ny, nx, by, bx = 70, 90, 23, 31
    img = make_frames(1, ny, nx, 1, seed=7)[0]
    W = matrices32(ny, nx, by, bx)
    Ku, Hs = 23, 16
    gs = random_filters(Ku, Hs, 1, seed=1)
    raw, (w1, w2, w3, w4), g = upload(img), [padded(m) for m in W], padded(gs[0])
    F = torch.zeros((2 * Ku, 16), device="cuda")
    y = torch.zeros((by, bx), device="cuda")
    need = L.sprk_align_spectrum_ws_bytes(ny, nx, Hs)
    need_s = L.sprk_align_synthesize_ws_bytes(by, Hs)
    ws = torch.zeros(max(need, need_s) + 16, dtype=torch.uint8, device="cuda")
    good = dict(raw=raw.data_ptr(), mode=1, ny=ny, nx=nx, Ku=Ku, Hs=Hs, w1=w1.data_ptr(), w2=w2.data_ptr(), g=g.data_ptr(),
                anchor=float(img[0, 0]), F=F.data_ptr(), first=1, ws=ws.data_ptr(), ws_bytes=need)

    def call(**change):
        a = dict(good, **change)
        return L.sprk_align_spectrum(a["raw"], a["mode"], a["ny"], a["nx"], a["Ku"], a["Hs"], a["w1"], a["w2"], a["g"], a["anchor"],
                                     a["F"], a["first"], a["ws"], a["ws_bytes"], _stream())

    torch.cuda.synchronize()
    before = L.sprk_launch_count()
    cases = [(dict(ws_bytes=need - 1), EWORKSPACE, b"workspace"), (dict(ws=None, ws_bytes=0), EWORKSPACE, b"workspace"),
             (dict(mode=3), EINVAL, b"mode"), (dict(Ku=72), EINVAL, b"kept"), (dict(Ku=0), EINVAL, b"kept"),
             (dict(Hs=47), EINVAL, b"kept"), (dict(Hs=0), EINVAL, b"kept"), (dict(ny=1), EINVAL, b"kept"),
             (dict(nx=16385), EINVAL, b"kept"), (dict(anchor=0.5), EINVAL, b"anchor"), (dict(anchor=40000.0), EINVAL, b"anchor"),
             (dict(mode=2, anchor=1.0), EINVAL, b"anchor"), (dict(F=None), EINVAL, b"null"), (dict(g=None), EINVAL, b"null"),
             (dict(F=F.data_ptr() + 4), EINVAL, b"aligned"), (dict(g=g.data_ptr() + 8), EINVAL, b"aligned"),
             (dict(ws=ws.data_ptr() + 8), EINVAL, b"aligned")]
    for change, code, word in cases:
        assert call(**change) == code, (change, L.sprk_last_error())
        assert word in L.sprk_last_error(), (change, L.sprk_last_error())
    assert L.sprk_launch_count() == before and not F.any()

    good_s = dict(F=F.data_ptr(), Ku=Ku, Hs=Hs, by=by, bx=bx, w3=w3.data_ptr(), w4=w4.data_ptr(), y=y.data_ptr(),
                  ws=ws.data_ptr(), ws_bytes=need_s)

    def call_s(**change):
        a = dict(good_s, **change)
        return L.sprk_align_synthesize(a["F"], a["Ku"], a["Hs"], a["by"], a["bx"], a["w3"], a["w4"], a["y"], a["ws"],
                                       a["ws_bytes"], _stream())

    cases = [(dict(ws_bytes=need_s - 1), EWORKSPACE, b"workspace"), (dict(ws=None, ws_bytes=0), EWORKSPACE, b"workspace"),
             (dict(Ku=25), EINVAL, b"kept"), (dict(Hs=17), EINVAL, b"kept"), (dict(by=1), EINVAL, b"kept"),
             (dict(bx=16385), EINVAL, b"kept"), (dict(y=None), EINVAL, b"null"), (dict(w3=None), EINVAL, b"null"),
             (dict(y=y.data_ptr() + 4), EINVAL, b"aligned"), (dict(ws=ws.data_ptr() + 8), EINVAL, b"aligned")]
    for change, code, word in cases:
        assert call_s(**change) == code, (change, L.sprk_last_error())
        assert word in L.sprk_last_error(), (change, L.sprk_last_error())
    assert L.sprk_launch_count() == before and not y.any()

    assert call() == 0, L.sprk_last_error()
    assert L.sprk_launch_count() == before + 2                   # stages 1 and 2
    assert call_s() == 0, L.sprk_last_error()
    assert L.sprk_launch_count() == before + 4                   # stages 3 and 4
    want_F = dose_model.spectrum([img], W[0], W[1], gs, float(img[0, 0]))
    assert np.array_equal(F.cpu().numpy(), want_F)
    assert np.array_equal(y.cpu().numpy(), dose_model.synthesize(want_F, W[2], W[3]))


# ---- the operands built on the device --------------------------------------------------------------------------------------
# G = Phi e^{i a}, a = -2 pi (k dy / ny + v dx / nx), in float64 on either side.  Each side forms a with three roundings
# (relative 3 x 2^-53 of |a_y| + |a_x|), takes cos and sin (within 2^-52 absolute each, and a change of the argument by da
# moves them by at most da), multiplies the two phases (four products and two sums of numbers at most 1: 6 x 2^-53) and
# multiplies by Phi <= sqrt(Z), itself exp, sum, division and square root away from NumPy's by a few ulps.  So per side
# |dG| <= sqrt(Z) 2^-53 (3 A + 16) with A = 2 pi (|k dy| / ny + |v dx| / nx) at its largest, and the two sides differ by at
# most twice that: FILTER_ULPS x 2^-53 x sqrt(Z) x (A + 6).
FILTER_ULPS = 6
FILTER_CASES = [(128, 192, 128, 192, 8, (4.25, -3.5)), (97, 130, 64, 87, 5, (-31.75, 47.0)), (2048, 1024, 683, 342, 40, (12.3, -7.7))]


def test_device_filters_match_numpy():
    from spr_pick_amd import dose
    worst = 0.0
    for ny, nx, by, bx, Z, (dy, dx) in FILTER_CASES:
        filters = dose.FrameFilters(ny, nx, by, bx, Z, "cuda", apix=1.1, dose=1.5, pre_dose=0.5, kv=300.0)
        phi = dose.dose_filter64(ny, nx, by, bx, 1.1, 1.5, 0.5, 300.0, Z)
        A = 2 * np.pi * ((by // 2) * abs(dy) / ny + (bx // 2) * abs(dx) / nx)
        tol = FILTER_ULPS * 2.0 ** -53 * np.sqrt(Z) * (A + 6)
        for f in (0, Z - 1):
            want = dose.frame_filter64(phi[f], ny, nx, by, bx, dy, dx)
            gr, gi = filters.filter64(f, dy, dx)
            err = max(float(np.abs(gr.cpu().numpy() - want.real).max()), float(np.abs(gi.cpu().numpy() - want.imag).max()))
            worst = max(worst, err / tol)
            print("%dx%d -> %dx%d, frame %d of %d, shift (%g, %g): largest |device - NumPy| = %.3g (bound %.3g)"
                  % (ny, nx, by, bx, f, Z, dy, dx, err, tol))
            assert err <= tol
            g = filters.g(f, dy, dx).cpu().numpy()
            Ku, Hs = want.shape
            assert g.shape == (2 * Ku, -(-Hs // 4) * 4) and not g[:, Hs:].any() and g[by // 2, 0] == 1.0 and g[Ku + by // 2, 0] == 0.0
            ulp = np.spacing(np.abs(want.real).astype(np.float32)).astype(np.float64)
            assert (np.abs(g[:Ku, :Hs] - want.real) <= 0.5 * ulp + tol).all()
    print("worst |device - NumPy| / bound %.3g" % worst)
    # the matrices: one geometry with a crop on both axes, against the float64 ones rounded once
    ny, nx, by, bx = 130, 97, 70, 64
    for m, m64 in zip(dose.spectrum_matrices(ny, nx, by, bx, "cuda"), dose.spectrum_matrices64(ny, nx, by, bx)):
        a = m.cpu().numpy()
        ulp = np.spacing(np.abs(m64).astype(np.float32)).astype(np.float64)
        assert not a[:, m64.shape[1]:].any() and (np.abs(a[:, :m64.shape[1]] - m64) <= 0.5 * ulp + 1e-15).all()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def movies():
    ny, nx = dose_model.MOVIE_SHAPE
    out = []
    for seed, noise in dose_model.MOVIE_CASES:
        movie, spec, drift = dose_model.make_movie(ny, nx, dose_model.MOVIE_FRAMES, seed, noise)
        out.append((movie, spec, drift, dose_model.model_gain(movie, spec, drift)))
    return out


def read_mrc(path):
    from spr_pick_amd import micrograph_io
    image, header, _ = micrograph_io.parse_mrc(open(path, "rb").read())
    return image, header


@pytest.mark.parametrize("case", range(len(dose_model.MOVIE_CASES)))
def test_joint_align_dose_end_to_end(case, movies, tmp_path):
    from spr_pick_amd import cli, dose
    movie, spec, drift, (model_plain, model_weighted) = movies[case]
    Z, ny, nx = movie.shape
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "movies"))
    write_movie(os.path.join(root, "movies", "mov.mrc"), movie, dose_model.APIX)
    base = ["align", "--movies", os.path.join(root, "movies")]
    plain_dir, dw_dir = os.path.join(root, "plain"), os.path.join(root, "dw")
    cli.start(base + ["--out", plain_dir])
    res = cli.start(base + ["--out", dw_dir, "--dose", str(dose_model.DOSE)])
    # (a) today's files are what they are without the flag
    assert sorted(os.listdir(plain_dir)) == ["images.txt", "mov.mrc", "mov_shifts.txt"]
    assert sorted(os.listdir(dw_dir)) == ["images.txt", "images_DW.txt", "mov.mrc", "mov_DW.mrc", "mov_shifts.txt"]
    for name in ("mov.mrc", "mov_shifts.txt"):
        assert open(os.path.join(plain_dir, name), "rb").read() == open(os.path.join(dw_dir, name), "rb").read(), name
    assert open(os.path.join(plain_dir, "images.txt")).read().replace(plain_dir, dw_dir) == open(os.path.join(dw_dir, "images.txt")).read()
    assert res["mov"]["dose_weighted"] == os.path.join(dw_dir, "mov_DW.mrc")
    assert open(os.path.join(dw_dir, "images_DW.txt")).read() == "image_name\tpath\nmov\t%s\n" % res["mov"]["dose_weighted"]
    total, _ = read_mrc(os.path.join(dw_dir, "mov.mrc"))
    weighted, header = read_mrc(res["mov"]["dose_weighted"])
    assert header.mode == 2 and weighted.shape == (ny, nx) and abs(header.xlen / header.mx - dose_model.APIX) < 1e-5
    # (b) within the a-priori bound of the float64 model at the device's own shifts (the sum applies the drift's negative)
    shifts = np.array(res["mov"]["shifts"])
    anchor = float(movie[0, 0, 0])
    phi = dose.dose_filter64(ny, nx, ny, nx, dose_model.APIX, dose_model.DOSE, 0.0, dose_model.KV, Z)
    Gs = [dose.frame_filter64(phi[f], ny, nx, ny, nx, 0.0 - shifts[f, 1], 0.0 - shifts[f, 0]) for f in range(Z)]
    Ds = [align_model.operand(f, anchor).astype(np.float64) for f in movie]
    W64 = dose.spectrum_matrices64(ny, nx, ny, nx)
    ref = dose_model.product64(Ds, W64, Gs) + Z * anchor
    # the bound for operands known to within a float32 ulp, and the one fp32 add of the anchor term
    _, bound = dose_model.apriori_bound(Ds, [m.astype(np.float32) for m in W64], [dose.pack_filter(G)[:, :G.shape[1]] for G in Gs],
                                        exact_operands=10)
    bound = bound + dose_model.EPS * (np.abs(ref) + bound)
    ratio = float((np.abs(weighted - ref) / bound).max())
    # (c) the gain in correlation with the specimen
    c_plain, c_weighted = dose_model.correlation(total, spec), dose_model.correlation(weighted, spec)
    print("seed %d, noise %.1f: correlation with the specimen: plain %.4f, dose-weighted %.4f (float64 model %.4f and %.4f); "
          "worst |DW - float64 model| / a-priori bound %.3g" % (*dose_model.MOVIE_CASES[case], c_plain, c_weighted, model_plain,
                                                                  model_weighted, ratio))
    assert ratio < 1
    assert model_weighted > model_plain
    assert c_weighted - c_plain >= 0.5 * (model_weighted - model_plain)
    assert abs(weighted.mean() - total.mean()) <= 1e-3 * abs(total.mean())         # the weighted sum's mean is the plain sum's


def test_odd_crop_writes_a_sum_the_chain_reads(movies, tmp_path):
    """(d) --ftbin 1.5: odd output sizes; the _DW.mrc has the plain sum's shape and pixel size, and `joint bin` reads it
    through images_DW.txt"""
    from spr_pick_amd import cli
    movie = movies[0][0]
    Z, ny, nx = movie.shape
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "movies"))
    write_movie(os.path.join(root, "movies", "mov.mrc"), movie, dose_model.APIX)
    out = os.path.join(root, "sums")
    res = cli.start(["align", "--movies", os.path.join(root, "movies"), "--out", out, "--ftbin", "1.5", "--dose", "10",
                     "--pre_dose", "2", "--kv", "200", "--max_shift", "8", "--iters", "2"])
    total, h_plain = read_mrc(os.path.join(out, "mov.mrc"))
    weighted, h_dw = read_mrc(res["mov"]["dose_weighted"])
    by, bx = res["mov"]["shape"]
    assert (by, bx) == (85, 128) and total.shape == weighted.shape == (by, bx)
    assert (h_dw.mx, h_dw.my, h_dw.xlen, h_dw.ylen) == (h_plain.mx, h_plain.my, h_plain.xlen, h_plain.ylen)
    assert abs(h_dw.xlen / h_dw.mx - 1.5 * dose_model.APIX) < 1e-4
    assert np.isfinite(weighted).all() and abs(weighted.mean() - total.mean()) <= 1e-3 * abs(total.mean())
    binned = cli.start(["bin", "--dataset", os.path.join(out, "images_DW.txt"), "--ftbin", "2", "--out", os.path.join(root, "bin")])
    assert list(binned["geometry"]) == ["mov"] and tuple(binned["geometry"]["mov"][2:]) == (by, bx)
