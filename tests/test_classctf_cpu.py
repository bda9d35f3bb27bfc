"""`joint class2d --ctf_weight` without a GPU: the NumPy model of the three contracts inside its a-priori bound,
``ctf.weight_tables``, the sign of the rotation rule, every refusal of the C ABI, of the operators and of the command line
(nothing is launched), the fixed-assignment average and the float64 model of the whole loop on planted data."""
import os
import re

import numpy as np
import pytest
import torch

import class2d_model
import classctf_model as model

PURITY_LINE = 0.95                                # test_class2d_cpu's line
f32 = np.float32


def matrices(S):
    from spr_pick_amd import extract
    return extract.filter_matrices(S, S)


def tables(S, rows, mode):
    """``ctf.weight_tables`` without its padded columns"""
    from spr_pick_amd import ctf
    wn, wd = ctf.weight_tables(S, rows, mode)
    return wn[:, :, :S // 2 + 1], wd[:, :, :S // 2 + 1]


# ---- the model ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [16, 34])
def test_model_stays_inside_its_apriori_bound(S):
    rng = np.random.default_rng(S)
    W = matrices(S)
    n = 9
    imgs = rng.standard_normal((n, S, S)).astype(f32)
    for got, ref, bound in model.stage_bounds(imgs[0], W):
        print("S %d: stage error / bound %.3f" % (S, (np.abs(got - ref)[bound > 0] / bound[bound > 0]).max()))
        assert (np.abs(got - ref) <= bound).all()
    # a spectrum is the DFT of its image on the kept half plane; synthesis inverts it
    h = S // 2
    F = np.fft.fft2(imgs[0].astype(np.float64))[np.arange(-h, h + 1) % S][:, :h + 1]
    spec = model.spectrum(imgs[0], W)
    assert np.abs(spec[:S + 1] - F.real).max() < 1e-4 * np.abs(F).max() and np.abs(spec[S + 1:] - F.imag).max() < 1e-4 * np.abs(F).max()
    assert np.abs(model.synthesize(spec, W) - imgs[0]).max() < 1e-4 * np.abs(imgs[0]).max()
    rows = model.micrograph_rows(2000.0)[:3]
    wn, wd = tables(S, rows, "flip")
    group = rng.integers(0, 3, n).astype(np.int32)
    members = np.array([3, 0, 8, 8, 5, 1, 2], dtype=np.int32)
    specs = np.stack([model.spectrum(i, W) for i in imgs])
    out = np.full((2,) + specs.shape[1:], np.nan, f32)
    model.wiener(specs, wn, wd, group, members, np.array([0, 0, 7], np.int32), 1.0, out)
    assert np.isnan(out[0]).all() and np.isfinite(out[1]).all()          # the empty class keeps what it holds
    got = model.synthesize(out[1], W)
    ref, bound = model.apriori_bound(imgs, W, wn, wd, group, members, 1.0)
    print("S %d: composed error / bound %.3f" % (S, (np.abs(got - ref) / bound).max()))
    assert (np.abs(got - ref) <= bound).all()
    # indices outside their arrays behave as their clamped values
    wild = np.full_like(out, np.nan)
    model.wiener(specs, wn, wd, np.where(group == 2, 7, group), np.where(members == 8, 99, members), np.array([-4, 0, 11], np.int32),
                 1.0, wild)
    assert np.isnan(wild[0]).all() and np.array_equal(wild[1], out[1])


# ---- weight_tables ----------------------------------------------------------------------------------------------------------------
def test_weight_tables_relation_to_the_correction_filter():
    from spr_pick_amd import ctf
    S, h = 64, 32
    rows = np.array([(15000.0, 11000.0, 20.0, 300.0, 2.7, 0.07, 4.0), (9000.0, 9000.0, 0.0, 200.0, 2.0, 0.1, 2.5)])
    wn_f, wd_f = ctf.weight_tables(S, rows, "flip")
    wn_m, wd_m = ctf.weight_tables(S, rows, "multiply")
    assert wn_f.dtype == wd_f.dtype == f32 and wn_f.shape == wd_f.shape == wn_m.shape == (2, S + 1, 36)
    assert not wn_f[:, :, h + 1:].any() and not wd_f[:, :, h + 1:].any() and not wn_m[:, :, h + 1:].any()    # exact zeros
    assert np.array_equal(wd_f, wd_m) and np.array_equal(wn_m[:, :, :h + 1], np.ones((2, S + 1, h + 1), f32))
    for g, (u, v, angle, kv, cs, ac, apix) in enumerate(rows):
        mult = ctf.correction_filter(S, S, apix, u, v, angle, kv, cs, ac, "multiply")
        flip = ctf.correction_filter(S, S, apix, u, v, angle, kv, cs, ac, "flip")
        assert np.array_equal(wn_f[g, :, :h + 1], np.abs(mult))          # flip: wn = |the multiply filter|, bit for bit
        # wd is the square in float64 rounded once, not the square of the rounded filter
        s, dz = ctf.filter_grid(np, S, S, apix, u, v, np.radians(angle))
        c = ctf.ctf(s, dz, kv, cs, ac)
        assert np.array_equal(wd_f[g, :, :h + 1], (c * c).astype(f32))
        assert np.abs(wd_f[g, :, :h + 1] - mult.astype(np.float64) ** 2).max() < 2.0 ** -22
        assert np.array_equal(flip, np.where(mult >= 0, 1.0, -1.0).astype(f32))       # and the flip filter its sign
        # even: the table at (-k, -v) equals the one at (k, v); on the stored half plane that is column 0
        assert np.array_equal(wn_f[g, ::-1, 0], wn_f[g, :, 0]) and np.array_equal(wd_f[g, ::-1, 0], wd_f[g, :, 0])
    # U = V: independent of the angle
    iso = [(12000.0, 12000.0, a, 300.0, 2.7, 0.07, 4.0) for a in (0.0, 33.0, 170.0)]
    wn, wd = ctf.weight_tables(S, iso, "flip")
    assert np.array_equal(wn[0], wn[1]) and np.array_equal(wn[0], wn[2]) and np.array_equal(wd[0], wd[2])
    # torch builds the same tables within what the two sines differ by
    tn, td = ctf.weight_tables(S, rows, "flip", device="cpu")
    assert tn.dtype == torch.float32 and tuple(tn.shape) == wn_f.shape
    assert np.abs(tn.numpy() - wn_f).max() < 2.0 ** -22 and np.abs(td.numpy() - wd_f).max() < 2.0 ** -22
    assert not tn.numpy()[:, :, h + 1:].any()
    for bad in ((15, rows, "flip"), (130, rows, "flip"), (64, rows, "wiener"), (64, [], "flip"), (64, [(1, 1, 0, 300, 2.7, 0.07, 0)], "flip"),
                (64, [(np.nan, 1, 0, 300, 2.7, 0.07, 1)], "flip")):
        with pytest.raises(ValueError):
            ctf.weight_tables(*bad)


def test_correction_filter_bits_are_unchanged():
    """the grid moved into ``ctf.filter_grid``; the filter is the expression it was"""
    import math
    from spr_pick_amd import ctf
    for B, S, apix, u, v, angle in ((64, 64, 2.0, 9000.0, 7000.0, 30.0), (96, 48, 1.5, 12000.0, 10000.0, 120.0)):
        h = S // 2
        k = np.arange(-h, h + 1, dtype=np.float64)[:, None]
        w = np.arange(h + 1, dtype=np.float64)[None, :]
        s = np.sqrt(k * k + w * w) / (B * float(apix))
        dz = 0.5 * (u + v) + 0.5 * (u - v) * np.cos(2.0 * (np.arctan2(k, w) - math.radians(angle)))
        c = ctf.ctf(s, dz, 300.0, 2.7, 0.07)
        assert np.array_equal(ctf.correction_filter(B, S, apix, u, v, angle, 300.0, 2.7, 0.07, "multiply"), (-c).astype(f32))
        assert np.array_equal(ctf.correction_filter(B, S, apix, u, v, angle, 300.0, 2.7, 0.07, "flip"),
                              np.where(c <= 0, 1.0, -1.0).astype(f32))


# ---- the rotation sign ------------------------------------------------------------------------------------------------------------
def test_turning_a_particle_turns_its_ctf_the_way_the_groups_say():
    """Measured: correlation 0.9992 with the table at the angle ``class2d.ctf_groups`` gives, 0.9679 at the
    opposite sign."""
    from spr_pick_amd import class2d
    S, h, A_n, a = 64, 32, 12, 1                                 # turned back by index 1 of 12: 30 degrees
    rng = np.random.default_rng(5)
    i, j = np.mgrid[0:S, 0:S]
    obj = np.zeros((S, S))
    for _ in range(40):                                          # smooth: 40 Gaussian blobs of sigma 1
        cy, cx = S // 2 + rng.uniform(-S / 4, S / 4, 2)
        obj += rng.uniform(0.5, 1.5) * np.exp(-((i - cy) ** 2 + (j - cx) ** 2) / 2.0)
    row = np.array([(14000.0, 10000.0, 20.0, model.KV, model.CS, model.AC, model.APIX)])
    seen = np.fft.ifft2(model.plane_ctf(S, model.APIX, 14000.0, 10000.0, 20.0) * np.fft.fft2(obj)).real
    cs = class2d.angle_table(A_n).astype(np.float64)
    turned = class2d_model.rigid64(np.stack([seen, obj]), cs[[a, a], 0], cs[[a, a], 1], np.zeros(2, np.int64), np.zeros(2, np.int64))
    group, extra = class2d.ctf_groups([0], row, [a], A_n)
    assert group.tolist() == [1] and extra.shape == (1, 7) and extra[0, 2] == 50.0 and np.array_equal(extra[0, :2], row[0, :2])
    opposite = extra.copy()
    opposite[0, 2] = 20.0 - 30.0
    half = lambda x: np.abs(np.fft.fft2(x))[np.arange(-h, h + 1) % S][:, :h + 1]      # noqa: E731
    got = []
    for r in (extra, opposite):
        wn, _ = tables(S, r, "flip")                             # |c| at that angle
        got.append(model.correlation(wn[0].astype(np.float64) * half(turned[1]), half(turned[0])))
    print("rotation sign: correlation %.4f with the rule's table, %.4f with the opposite sign" % tuple(got))
    assert got[0] > got[1] and (1 - got[0]) < 0.5 * (1 - got[1])
    # rows with U = V keep their table whatever the angle, and pairs that occur twice share one
    table = np.array([(9000.0, 9000.0, 0.0, 300.0, 2.7, 0.07, 4.0), (9000.0, 8000.0, 10.0, 300.0, 2.7, 0.07, 4.0)])
    group, extra = class2d.ctf_groups([0, 1, 1, 0, 1], table, [5, 3, 0, 2, 3], 36)
    assert group.tolist() == [0, 3, 2, 0, 3] and extra[:, 2].tolist() == [10.0, 40.0]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_names_in_header_binding_and_refusals_launch_nothing():
    from conftest import ROOT
    from spr_pick_amd import _lib, torch_ops
    names = {"sprk_class_spectrum", "sprk_class_spectrum_ws_bytes", "sprk_class_wiener", "sprk_class_synthesize",
             "sprk_class_synthesize_ws_bytes"}
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sprk.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(sprk_[a-z0-9_]+)\s*\(", text)) and names <= set(_lib.EXPORTS)
    assert re.search(r"#define SPRK_ABI_VERSION 430\b", text) and _lib.ABI_VERSION == 430
    assert {"class_spectrum", "class_wiener", "class_synthesize"} <= set(torch_ops.registered())
    L = _lib.lib()
    EINVAL, EWORKSPACE = -1, -2
    p = 0x1000
    before = L.sprk_launch_count()
    # the queries: the geometry of the header, 0 for what would be refused
    for S in (16, 34, 64, 128):
        Hs, ldv, ldz = S // 2 + 1, (S // 2 + 4) & ~3, (S + 5) & ~3
        assert L.sprk_class_spectrum_ws_bytes(5, S, 2) == 2 * (2 * S * ldv * 4) and L.sprk_class_synthesize_ws_bytes(3, S) == 3 * S * ldz * 4
        assert L.sprk_class_spectrum_ws_bytes(5, S, 0) == 5 * (2 * S * ldv * 4) and Hs <= ldv < Hs + 4
    assert L.sprk_class_spectrum_ws_bytes(5, 15, 0) == 0 == L.sprk_class_spectrum_ws_bytes(5, 130, 0)
    assert L.sprk_class_spectrum_ws_bytes(0, 64, 0) == 0 == L.sprk_class_spectrum_ws_bytes(5, 64, -1)
    assert L.sprk_class_synthesize_ws_bytes(0, 64) == 0 == L.sprk_class_synthesize_ws_bytes(3, 66 + 64)

    def spectrum(**kw):
        a = dict(img=p, n=5, side=64, w1=p, w2=p, max_batch=0, spec=p, ws=p, ws_bytes=1 << 30)
        a.update(kw)
        return L.sprk_class_spectrum(*[a[k] for k in ("img", "n", "side", "w1", "w2", "max_batch", "spec", "ws", "ws_bytes")], None)

    need = L.sprk_class_spectrum_ws_bytes(5, 64, 0)
    for change, rc, word in ((dict(side=63), EINVAL, b"side"), (dict(side=14), EINVAL, b"side"), (dict(side=130), EINVAL, b"side"),
                             (dict(n=-1), EINVAL, b"images"), (dict(max_batch=-1), EINVAL, b"max_batch"),
                             (dict(img=None), EINVAL, b"null"), (dict(w1=None), EINVAL, b"null"), (dict(w2=None), EINVAL, b"null"),
                             (dict(spec=None), EINVAL, b"null"), (dict(img=p + 8), EINVAL, b"aligned"),
                             (dict(spec=p + 4), EINVAL, b"aligned"), (dict(ws=p + 8), EINVAL, b"aligned"),
                             (dict(ws=None), EWORKSPACE, b"workspace"), (dict(ws_bytes=need - 1), EWORKSPACE, b"workspace"),
                             (dict(ws_bytes=0), EWORKSPACE, b"workspace")):
        assert spectrum(**change) == rc and word in L.sprk_last_error(), (change, L.sprk_last_error())
    assert ("%d" % need).encode() in L.sprk_last_error()         # the remedy: the bytes the query returns
    assert spectrum(n=0, img=None, spec=None, ws=None, ws_bytes=0) == 0      # nothing to do

    def wiener(**kw):
        a = dict(spec=p, n=9, side=64, wn=p, wd=p, G=3, group=p, members=p, N=7, offsets=p, K=2, tau=1.0, out=2 * p)
        a.update(kw)
        return L.sprk_class_wiener(*[a[k] for k in ("spec", "n", "side", "wn", "wd", "G", "group", "members", "N", "offsets", "K",
                                                    "tau", "out")], None)

    for change, word in ((dict(side=65), b"side"), (dict(side=256), b"side"), (dict(n=-1), b"at least 0"), (dict(N=-2), b"at least 0"),
                         (dict(K=0), b"classes"), (dict(K=65536), b"classes"), (dict(G=0), b"tables"), (dict(tau=0.0), b"tau"),
                         (dict(tau=-1.0), b"tau"), (dict(tau=float("inf")), b"tau"), (dict(tau=float("nan")), b"tau"),
                         (dict(spec=None), b"null"), (dict(wn=None), b"null"), (dict(wd=None), b"null"), (dict(group=None), b"null"),
                         (dict(members=None), b"null"), (dict(offsets=None), b"null"), (dict(out=None), b"null"),
                         (dict(wn=p + 4), b"aligned"), (dict(out=p + 8), b"aligned"), (dict(members=p + 2), b"aligned"),
                         (dict(out=p), b"must not be spec")):
        assert wiener(**change) == EINVAL and word in L.sprk_last_error(), (change, L.sprk_last_error())
    assert wiener(N=0) == 0 and wiener(n=0) == 0                 # every class is empty: nothing to do

    def synthesize(**kw):
        a = dict(f=p, K=3, side=64, w3=p, w4=p, out=p, ws=p, ws_bytes=1 << 30)
        a.update(kw)
        return L.sprk_class_synthesize(*[a[k] for k in ("f", "K", "side", "w3", "w4", "out", "ws", "ws_bytes")], None)

    need = L.sprk_class_synthesize_ws_bytes(3, 64)
    for change, rc, word in ((dict(side=17), EINVAL, b"side"), (dict(side=8), EINVAL, b"side"), (dict(K=0), EINVAL, b"spectra"),
                             (dict(K=-3), EINVAL, b"spectra"), (dict(K=65536), EINVAL, b"spectra"), (dict(f=None), EINVAL, b"null"),
                             (dict(w3=None), EINVAL, b"null"), (dict(w4=None), EINVAL, b"null"), (dict(out=None), EINVAL, b"null"),
                             (dict(f=p + 4), EINVAL, b"aligned"), (dict(w4=p + 8), EINVAL, b"aligned"),
                             (dict(ws=None), EWORKSPACE, b"workspace"), (dict(ws_bytes=need - 16), EWORKSPACE, b"workspace")):
        assert synthesize(**change) == rc and word in L.sprk_last_error(), (change, L.sprk_last_error())
    assert L.sprk_launch_count() == before


def test_fake_tensor_shapes_of_the_three_operators():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from spr_pick_amd import _lib, torch_ops
    assert torch_ops.class_spectrum_shapes(64) == ((66, 64), (130, 128), (128, 132), (64, 68), (130, 36), (65, 36))
    assert torch_ops.class_spectrum_shapes(34) == ((36, 36), (70, 68), (68, 72), (34, 36), (70, 20), (35, 20))
    assert torch_ops.class_spectrum_shapes(64)[:4] == torch_ops.extract_filter_shapes(64, 64)[:4]

    def f(*shape):
        return torch.empty(*shape, device="cuda")

    def i32(*shape):
        return torch.empty(*shape, dtype=torch.int32, device="cuda")

    ops = torch.ops.sprk
    with FakeTensorMode():
        S = 34
        w1, w2, w3, w4 = (f(*s) for s in torch_ops.class_spectrum_shapes(S)[:4])
        img, spec, wn, wd = f(5, S, S), f(5, 70, 20), f(3, 35, 20), f(3, 35, 20)
        out, avg = f(2, 70, 20), f(2, S, S)
        assert ops.class_spectrum(img, w1, w2, 0, spec) is None and ops.class_spectrum(img, w1, w2, 2, spec) is None
        assert ops.class_wiener(spec, S, wn, wd, i32(5), i32(7), i32(3), 1.0, out) is None
        assert ops.class_wiener(spec, S, wn, wd, i32(5), i32(0), i32(3), 0.5, out) is None
        assert ops.class_synthesize(out, S, w3, w4, avg) is None
        bad = [(ops.class_spectrum, (f(5, 33, 33), w1, w2, 0, spec)), (ops.class_spectrum, (f(5, 130, 130), w1, w2, 0, spec)),
               (ops.class_spectrum, (f(5, 14, 14), w1, w2, 0, spec)), (ops.class_spectrum, (f(5, S, S + 2), w1, w2, 0, spec)),
               (ops.class_spectrum, (img, w2, w2, 0, spec)), (ops.class_spectrum, (img, w1, w1, 0, spec)),
               (ops.class_spectrum, (img, w1, w2, -1, spec)), (ops.class_spectrum, (img, w1, w2, 0, f(4, 70, 20))),
               (ops.class_spectrum, (img, w1, w2, 0, f(5, 70, 18))), (ops.class_spectrum, (img.double(), w1, w2, 0, spec)),
               (ops.class_wiener, (spec, 36, wn, wd, i32(5), i32(7), i32(3), 1.0, out)),
               (ops.class_wiener, (spec, S, wn, f(2, 35, 20), i32(5), i32(7), i32(3), 1.0, out)),
               (ops.class_wiener, (spec, S, f(3, 35, 18), f(3, 35, 18), i32(5), i32(7), i32(3), 1.0, out)),
               (ops.class_wiener, (spec, S, wn, wd, i32(4), i32(7), i32(3), 1.0, out)),
               (ops.class_wiener, (spec, S, wn, wd, i32(5), i32(7).long(), i32(3), 1.0, out)),
               (ops.class_wiener, (spec, S, wn, wd, i32(5), i32(7), i32(1), 1.0, out)),
               (ops.class_wiener, (spec, S, wn, wd, i32(5), i32(7), i32(4), 1.0, out)),
               (ops.class_wiener, (spec, S, wn, wd, i32(5), i32(7), i32(3), 0.0, out)),
               (ops.class_wiener, (spec, S, wn, wd, i32(5), i32(7), i32(3), float("inf"), out)),
               (ops.class_wiener, (spec, S, wn, wd, i32(5), i32(7), i32(3), float("nan"), out)),
               (ops.class_synthesize, (out, 36, w3, w4, avg)), (ops.class_synthesize, (out, S, w4, w4, avg)),
               (ops.class_synthesize, (out, S, w3, w3, avg)), (ops.class_synthesize, (out, S, w3, w4, f(3, S, S))),
               (ops.class_synthesize, (f(0, 70, 20), S, w3, w4, f(0, S, S)))]
        for op, args in bad:
            with pytest.raises(_lib.SprkError):
                op(*args)


def _write_star(tmp_path, columns):
    from spr_pick_amd import export
    path = os.path.join(tmp_path, "particles.star")
    with open(path, "w") as f:
        f.write(export.PARTICLES_STAR_HEADER)
        f.write("".join("_rln%s #%d\n" % (c, 6 + k) for k, c in enumerate(columns)))
        for k in range(4):
            f.write("%d\t%d\t%06d@absent.mrcs\tmic.mrc\t0.5%s\n" % (10 * k, 7, k + 1, "\t1.0" * len(columns)))
    return path


def test_command_line_refusals(tmp_path, capsys):
    from spr_pick_amd import _lib, class2d, cli
    p = cli.build_parser()
    base = ["class2d", "--particles", "p.star", "--classes", "4", "--out", "o"]
    a = vars(p.parse_args(base))
    assert a["ctf_weight"] is None and a["wiener"] is None
    a = vars(p.parse_args(base + ["--ctf_weight", "multiply", "--wiener", "0.25"]))
    assert (a["ctf_weight"], a["wiener"]) == ("multiply", 0.25)
    assert class2d.check_ctf_weight(None, None) is None and class2d.check_ctf_weight("flip", None) == 1.0
    for bad, word in ((["--wiener", "2"], "--ctf_weight"), (["--ctf_weight", "flip", "--wiener", "0"], "> 0"),
                      (["--ctf_weight", "flip", "--wiener", "-1"], "> 0"), (["--ctf_weight", "flip", "--wiener", "inf"], "> 0"),
                      (["--ctf_weight", "flip", "--wiener", "nan"], "> 0"), (["--ctf_weight", "wiener"], "ctf_weight")):
        with pytest.raises(SystemExit):
            p.parse_args(base + bad)
        assert word in capsys.readouterr().err, bad
    # the CTF columns: all eight or a refusal that names the remedy, before any stack is opened (there is none) or made
    before = _lib.lib().sprk_launch_count()
    out = os.path.join(str(tmp_path), "cls")
    for columns in ((), class2d.CTF_COLUMNS[:2], class2d.CTF_COLUMNS[:-1]):
        star = _write_star(str(tmp_path), columns)
        with pytest.raises(SystemExit):
            cli.start(["class2d", "--particles", star, "--classes", "2", "--out", out, "--ctf_weight", "flip"])
        err = capsys.readouterr().err
        assert "joint extract --ctf STAR --ctf_correct flip" in err and "_rlnDetectorPixelSize" in err
    assert _lib.lib().sprk_launch_count() == before and not os.path.exists(out)
    # the rows: distinct CTFs in order of appearance, apix = DetectorPixelSize 10^4 / Magnification
    labels = ["ImageName"] + list(class2d.CTF_COLUMNS)
    rows = ["1@a.mrcs 9000 8000 10 300 2.7 0.07 10000 4.0", "2@a.mrcs 12000 12000 0 300 2.7 0.07 20000 4.0",
            "3@a.mrcs 9000 8000 10 300 2.7 0.07 10000 4.0"]
    index, table = class2d.ctf_rows(labels, rows)
    assert index.tolist() == [0, 1, 0] and table.tolist() == [[9000, 8000, 10, 300, 2.7, 0.07, 4.0], [12000, 12000, 0, 300, 2.7, 0.07, 2.0]]


# ---- fixed assignment, float64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", model.ONE_CLASS["seeds"])
def test_wiener_average_recovers_what_the_plain_mean_loses(seed):
    """Measured: Wiener 0.9832 .. 0.9843, plain mean 0.756 .. 0.813 over the three seeds."""
    from spr_pick_amd import extract
    c = model.ONE_CLASS
    P, obj, mic, rows = model.one_class(seed)
    W64 = extract.filter_matrices64(c["S"], c["S"])
    wn, wd = tables(c["S"], rows, "flip")
    members = list(range(c["N"]))
    weighted = model.masked_correlation(model.wiener64(P, W64, wn, wd, mic, members, 1.0), obj, c["radius"])
    plain = model.masked_correlation(P.astype(np.float64).mean(axis=0), obj, c["radius"])
    absc = np.stack([model.plane_abs_ctf(c["S"], rows[k]) for k in mic])
    full = model.masked_correlation(model.wiener_fft(P.astype(np.float64), absc, "flip", 1.0), obj, c["radius"])
    print("seed %d: Wiener %.4f (full-plane FFT %.4f), plain mean %.4f" % (seed, weighted, full, plain))
    assert weighted > 0.95 and plain < 0.90
    assert abs(weighted - full) < 1e-3                           # the half-plane matrices and the FFT tell one story


# ---- the float64 loop with weighting ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise,seed,astigmatism", model.CASES)
def test_model_loop_with_weighting_separates_planted_shapes(noise, seed, astigmatism):
    """Measured: see the table there."""
    P, labels, mic, rows, res = model.planted_case(noise, seed, astigmatism)
    K = model.CASE["K"]
    pur = class2d_model.purity(res["cls"], labels, K)
    print("noise %g seed %d U-V %g: purity %.4f, levels %s, members %s"
          % (noise, seed, astigmatism, pur, res["levels"], np.bincount(res["cls"], minlength=K).tolist()))
    assert pur >= PURITY_LINE
    assert np.abs(res["shift"]).max() <= model.CASE["R"] and [k for k, _ in res["levels"]] == [1, 2, 3]
