"""`joint class2d` without a GPU: the parser, the refusals (nothing is launched), the names in the header,
the binding and torch.library, the split rule and the STAR columns, the properties of the NumPy models
(tests/class2d_model.py) and the float64 model of the whole loop on planted data."""
import os
import re

import numpy as np
import pytest
import torch

import class2d_model as model

PURITY_LINE = 0.95                                # the float64 model alone, on every planted case


def test_parser_defaults_and_errors():
    from spr_pick_amd import cli
    p = cli.build_parser()
    a = vars(p.parse_args(["class2d", "--particles", "particles.star", "--classes", "16", "--out", "cls"]))
    assert (a["classes"], a["angle_step"], a["max_shift"], a["radius"], a["iters"]) == (16, 5.0, 3, None, 8)
    a = vars(p.parse_args(["class2d", "-p", "p.star", "-k", "4", "-o", "o", "--angle_step", "7.5", "--max_shift", "31",
                           "--radius", "20", "--iters", "2"]))
    assert (a["classes"], a["angle_step"], a["max_shift"], a["radius"], a["iters"]) == (4, 7.5, 31, 20, 2)
    base = ["class2d", "--particles", "p.star", "--classes", "4", "--out", "o"]
    for bad in (base[:5], base[:3] + base[5:], base[:1] + base[3:], base[:3] + ["--classes", "0", "--out", "o"],
                base + ["--angle_step", "7"], base + ["--angle_step", "0"], base + ["--angle_step", "0.4"],
                base + ["--max_shift", "0"], base + ["--max_shift", "32"], base + ["--radius", "0"], base + ["--iters", "1"],
                base + ["--iters", "x"], base + ["--bin", "2"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    text = " ".join(p._subparsers._group_actions[0].choices["class2d"].format_help().split())
    tail = text[text.index("Not covered"):]
    for word in ("CTF weighting", "soft", "sub-pixel", "64 or 128"):          # the help says what is out of scope
        assert word in tail, word


def test_argument_and_geometry_refusals_name_the_remedy():
    from spr_pick_amd import class2d
    assert class2d.check_class2d_args(16) == 72
    assert class2d.angle_count(0.5) == 720 and class2d.angle_count(360) == 1
    for step in (0.25, 7, -5, 0):
        with pytest.raises(ValueError, match="angle_step"):
            class2d.angle_count(step)
    assert class2d.check_geometry(64, 300, 3, 3) == 27 and class2d.check_geometry(128, 10, 10, 31) == 31
    assert class2d.check_geometry(64, 300, 3, 3, 20) == 20
    for side in (48, 96, 192, 256):
        with pytest.raises(ValueError, match="--scale 64"):
            class2d.check_geometry(side, 300, 3, 3)
    with pytest.raises(ValueError, match="lower --classes"):
        class2d.check_geometry(64, 5, 6, 3)
    with pytest.raises(ValueError, match="lower --classes"):
        class2d.check_geometry(64, 5, 0, 3)
    with pytest.raises(ValueError, match="lower --radius"):
        class2d.check_geometry(64, 300, 3, 3, 28)
    with pytest.raises(ValueError, match="lower --max_shift"):
        class2d.check_geometry(64, 300, 3, 30)
    with pytest.raises(ValueError, match="CUDA"):                # before anything else: no fallback on the host
        class2d.classify(torch.zeros(4, 64, 64), 2)


def test_names_in_header_binding_and_torch_library():
    from conftest import ROOT
    from torch._subclasses.fake_tensor import FakeTensorMode
    from spr_pick_amd import _lib, torch_ops
    names = {"sprk_class_transform", "sprk_class_score", "sprk_class_average"}
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sprk.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(sprk_[a-z0-9_]+)\s*\(", text))
    assert re.search(r"#define SPRK_ABI_VERSION 430\b", text) and _lib.ABI_VERSION == 430
    assert re.search(r"#define SPRK_CLASS_MASK 1\b", text) and re.search(r"#define SPRK_CLASS_NORMALIZE 2\b", text)
    assert (torch_ops.CLASS_MASK, torch_ops.CLASS_NORMALIZE) == (model.MASK, model.NORMALIZE) == (1, 2)
    assert names <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names) and L.sprk_version() == 430
    assert {"class_transform", "class_score", "class_average"} <= set(torch_ops.registered())
    # refusals come before anything touches the device
    p = 0x1000
    before = L.sprk_launch_count()

    def transform(**kw):
        a = dict(src=p, n_src=2, S=64, idx=p, ang=p, shift=p, M=3, cs=p, A_n=72, radius=27, flags=3, pix=p, D=2291, ldo=2292,
                 out=p)
        a.update(kw)
        return L.sprk_class_transform(*[a[k] for k in ("src", "n_src", "S", "idx", "ang", "shift", "M", "cs", "A_n", "radius",
                                                       "flags", "pix", "D", "ldo", "out")], None)

    for change, word in ((dict(S=130), b"side"), (dict(S=63), b"side"), (dict(M=0), b"at least 1"), (dict(A_n=721), b"angle"),
                         (dict(A_n=0), b"angle"), (dict(flags=4), b"flags"), (dict(radius=65), b"radius"),
                         (dict(radius=-1), b"radius"), (dict(src=None), b"null"), (dict(out=None), b"null"),
                         (dict(src=p + 4), b"aligned"), (dict(idx=p + 2), b"aligned"), (dict(D=0), b"packed"),
                         (dict(D=4097), b"packed"), (dict(ldo=2291), b"packed"), (dict(ldo=2288), b"packed")):
        assert transform(**change) == -1 and word in L.sprk_last_error(), (change, L.sprk_last_error())

    def score(**kw):
        a = dict(Q=p, ldq=2292, N=10, B=p, ldb=2292, Mb=72, D=2292, scores=p, lds=72, best_score=p, best_index=p)
        a.update(kw)
        return L.sprk_class_score(*[a[k] for k in ("Q", "ldq", "N", "B", "ldb", "Mb", "D", "scores", "lds", "best_score",
                                                   "best_index")], None)

    for change, word in ((dict(N=0), b"rows"), (dict(Mb=0), b"bank"), (dict(Mb=65537), b"bank"), (dict(D=0), b"columns"),
                         (dict(D=2290), b"columns"), (dict(D=16388, ldq=16388, ldb=16388), b"columns"),
                         (dict(ldq=2288), b"strides"), (dict(ldb=2294), b"strides"), (dict(Q=None), b"null"),
                         (dict(best_index=None), b"null"), (dict(lds=71), b"score matrix"), (dict(B=p + 8), b"aligned")):
        assert score(**change) == -1 and word in L.sprk_last_error(), (change, L.sprk_last_error())

    def average(**kw):
        a = dict(src=p, n_src=40, S=64, ang=p, shift=p, cs=p, A_n=72, members=p, N=38, offsets=p, K=3, out=2 * p)
        a.update(kw)
        return L.sprk_class_average(*[a[k] for k in ("src", "n_src", "S", "ang", "shift", "cs", "A_n", "members", "N",
                                                     "offsets", "K", "out")], None)

    for change, word in ((dict(S=256), b"side"), (dict(N=0), b"members"), (dict(K=0), b"classes"), (dict(K=65536), b"classes"),
                         (dict(A_n=0), b"angle"), (dict(members=None), b"null"), (dict(out=p), b"must not be src"),
                         (dict(offsets=p + 1), b"aligned")):
        assert average(**change) == -1 and word in L.sprk_last_error(), (change, L.sprk_last_error())
    assert L.sprk_launch_count() == before

    def i32(*shape):
        return torch.empty(*shape, dtype=torch.int32, device="cuda")

    with FakeTensorMode():
        src, cs = torch.empty(5, 64, 64, device="cuda"), torch.empty(72, 2, device="cuda")
        out, packed, pix = torch.empty(7, 64, 64, device="cuda"), torch.empty(7, 2292, device="cuda"), i32(2291)
        assert torch.ops.sprk.class_transform(src, i32(7), i32(7), i32(7, 2), cs, 27, 3, None, out) is None
        assert torch.ops.sprk.class_transform(src, i32(7), i32(7), i32(7, 2), cs, 27, 0, pix, packed) is None
        for args in ((torch.empty(5, 66, 64, device="cuda"), i32(7), i32(7), i32(7, 2), cs, 27, 3, None, out),
                     (torch.empty(5, 130, 130, device="cuda"), i32(7), i32(7), i32(7, 2), cs, 27, 3, None, out),
                     (src, i32(7), i32(6), i32(7, 2), cs, 27, 3, None, out), (src, i32(7), i32(7), i32(7, 2), cs, 65, 1, None, out),
                     (src, i32(7), i32(7), i32(7, 2), cs, 27, 4, None, out), (src, i32(7), i32(7), i32(7, 2), cs, 27, 3, None, packed),
                     (src, i32(7), i32(7), i32(7, 2), cs, 27, 3, pix, torch.empty(7, 2291, device="cuda")),
                     (src, i32(7), i32(7), i32(7, 2), torch.empty(721, 2, device="cuda"), 27, 3, None, out)):
            with pytest.raises(_lib.SprkError):
                torch.ops.sprk.class_transform(*args)
        Q, B = torch.empty(10, 2292, device="cuda"), torch.empty(144, 2292, device="cuda")
        bs, bi = torch.empty(10, device="cuda"), i32(10)
        assert torch.ops.sprk.class_score(Q, B, 2292, None, bs, bi) is None
        assert torch.ops.sprk.class_score(Q, B, 2288, torch.empty(10, 144, device="cuda"), bs, bi) is None
        for args in ((Q, B, 2290, None, bs, bi), (Q, B, 2296, None, bs, bi), (Q, B, 2292, None, bs, i32(9)),
                     (Q, B, 2292, torch.empty(10, 143, device="cuda"), bs, bi),
                     (Q, torch.empty(144, 2290, device="cuda"), 2288, None, bs, bi)):
            with pytest.raises(_lib.SprkError):
                torch.ops.sprk.class_score(*args)
        avg = torch.empty(3, 64, 64, device="cuda")
        assert torch.ops.sprk.class_average(src, i32(5), i32(5, 2), cs, i32(5), i32(4), avg) is None
        for args in ((src, i32(4), i32(5, 2), cs, i32(5), i32(4), avg), (src, i32(5), i32(5, 2), cs, i32(5), i32(5), avg),
                     (src, i32(5), i32(5, 2), cs, i32(0), i32(4), avg)):
            with pytest.raises(_lib.SprkError):
                torch.ops.sprk.class_average(*args)


def test_split_rule_on_a_hand_made_score_vector():
    from spr_pick_amd import class2d
    #      class:  0    0    0    0    1    1    1    2    2    2    2
    cls = np.array([0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2])
    sc = np.array([.9, .1, .5, .5, .3, .2, .1, .4, .8, .6, .7])
    # Kc = 3 -> K = 5: the two largest classes are split; 0 and 2 tie in size, the stable sort takes 0 first
    new, parents = class2d.split_classes(cls, sc, 3, 5)
    assert parents == [0, 2]
    # class 0: median 0.5, members at or above it stay; class 2: median 0.65
    assert new.tolist() == [0, 3, 0, 0, 1, 1, 1, 4, 2, 4, 2]
    assert cls.tolist() == [0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2]    # the input is left alone
    # K - Kc limits the number of splits; a class of one member keeps it and founds an empty class
    new, parents = class2d.split_classes(cls, sc, 3, 4)
    assert parents == [0] and new.tolist() == [0, 3, 0, 0, 1, 1, 1, 2, 2, 2, 2]
    new, parents = class2d.split_classes(np.array([0]), np.array([1.0]), 1, 2)
    assert parents == [0] and new.tolist() == [0]
    for args in ((cls, sc, 3, 5), (cls, sc, 3, 4), (np.zeros(7, int), np.arange(7.0), 1, 3)):
        a, b = class2d.split_classes(*args), model.split_classes(*args)
        assert a[0].tolist() == b[0].tolist() and a[1] == b[1]


def _write_star(tmp_path, ctf, stacks):
    from spr_pick_amd import export, micrograph_io
    extra = ["DefocusU", "DefocusV", "DefocusAngle", "Voltage"] if ctf else []
    rows = []
    for name, images in stacks.items():
        with open(os.path.join(tmp_path, name), "wb") as f:
            micrograph_io.write_mrc(f, images)
        for k in range(len(images)):
            rows.append("%d\t%d\t%06d@%s\tmic.mrc\t0.5%s\n" % (10 * k, 7, k + 1, name, "\t1.0" * len(extra)))
    path = os.path.join(tmp_path, "particles.star")
    with open(path, "w") as f:
        f.write(export.PARTICLES_STAR_HEADER)
        f.write("".join("_rln%s #%d\n" % (c, 6 + k) for k, c in enumerate(extra)))
        f.writelines(rows)
    return path


@pytest.mark.parametrize("ctf", [False, True])
def test_star_columns_continue_the_numbering(tmp_path, ctf):
    from spr_pick_amd import class2d
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((3, 64, 64)).astype(np.float32), rng.standard_normal((2, 64, 64)).astype(np.float32)
    star = _write_star(str(tmp_path), ctf, {"a.mrcs": a, "b.mrcs": b})
    P, head, labels, rows, header = class2d.load_particles(star)
    assert np.array_equal(P, np.concatenate([a, b])) and len(rows) == 5 and (header.nx, header.ny, header.nz) == (64, 64, 3)
    n = 9 if ctf else 5
    assert len(labels) == n and labels[2] == "ImageName"
    assert class2d.star_columns(labels) == ["_rlnClassNumber #%d" % (n + 1), "_rlnAnglePsi #%d" % (n + 2),
                                            "_rlnOriginX #%d" % (n + 3), "_rlnOriginY #%d" % (n + 4)]
    assert "\n".join(head) + "\n" == open(star).read()[:len("\n".join(head)) + 1]      # verbatim
    # stacks of differing sides are refused, with the remedy
    star = _write_star(str(tmp_path), ctf, {"a.mrcs": a, "c.mrcs": np.zeros((2, 48, 48), np.float32)})
    with pytest.raises(ValueError, match="--scale 64"):
        class2d.load_particles(star)
    out = os.path.join(str(tmp_path), "classes.mrcs")
    class2d.write_averages(out, a, header._replace(mx=64, xlen=64 * 1.7))
    from spr_pick_amd import micrograph_io
    back, h, _ = micrograph_io.parse_mrc(open(out, "rb").read())
    assert np.array_equal(back, a) and h.mode == 2 and abs(h.xlen / h.mx - 1.7) < 1e-6


def test_model_angle_zero_is_a_shifted_copy():
    rng = np.random.default_rng(5)
    img = rng.standard_normal((64, 64)).astype(np.float32)
    cs = np.array([[1.0, 0.0]], dtype=np.float32)
    for dy, dx in ((0, 0), (3, -2), (-31, 31), (64, 0)):
        out = model.transform(img[None], [0], [0], [(dy, dx)], cs)[0]
        assert np.array_equal(out, model.shifted_copy(img, dy, dx)), (dy, dx)
    # a quarter turn with an exact table moves pixels: out[i, j] = src[S - j, i], and column 0 comes from beyond the edge
    quarter = model.transform(img[None], [0], [0], [(0, 0)], np.array([[0.0, 1.0]], dtype=np.float32))[0]
    assert np.array_equal(quarter[:, 1:], np.rot90(img, -1)[:, :-1]) and not quarter[:, 0].any()


def test_model_bank_rows_have_zero_mean_and_unit_norm_under_the_mask():
    from spr_pick_amd import class2d
    rng = np.random.default_rng(6)
    S, radius = 64, 27
    src = (rng.standard_normal((2, S, S)) + 3.0).astype(np.float32)
    cs = model.angle_table(72)
    assert np.array_equal(cs, class2d.angle_table(72))
    pix = model.packed_pixels(S, radius)
    assert len(pix) == 2289 and np.array_equal(pix, class2d.packed_pixels(S, radius))
    idx, ang = [0, 1, 1], [0, 7, 50]
    full = model.transform(src, idx, ang, [(0, 0)] * 3, cs, radius, model.MASK | model.NORMALIZE)
    packed = model.transform(src, idx, ang, [(0, 0)] * 3, cs, radius, model.MASK | model.NORMALIZE, pix, 2292)
    inside = model.mask_of(S, radius)
    assert not full[:, ~inside].any() and np.array_equal(packed[:, :2289], full.reshape(3, -1)[:, pix]) and not packed[:, 2289:].any()
    v = full[:, inside].astype(np.float64)
    assert np.abs(v.sum(axis=1)).max() < 2289 * 2.0 ** -24 and np.abs((v ** 2).sum(axis=1) - 1).max() < 1e-5
    flat = model.transform(np.full((1, S, S), 2.5, np.float32), [0], [3], [(0, 0)], cs, 20, model.NORMALIZE)
    assert not flat.any()                                        # a norm that is not > 0 gives zeros


def test_model_lowest_index_wins_a_tie():
    rng = np.random.default_rng(7)
    Q = rng.standard_normal((6, 12)).astype(np.float32)
    B = rng.standard_normal((9, 12)).astype(np.float32)
    B[7], B[2] = B[4], B[4]
    s = model.score(Q, B, 12)
    ref = Q.astype(np.float64) @ B.astype(np.float64).T
    assert np.abs(s - ref).max() < 12 * 2.0 ** -23 * np.abs(Q).max() * np.abs(B).max() * 12
    assert np.array_equal(s[:, 2], s[:, 4]) and np.array_equal(s[:, 7], s[:, 4])
    score, index = model.best(s)
    assert not np.isin(index, (4, 7)).any() and np.array_equal(score, s.max(axis=1))
    score, index = model.best(-np.abs(s) - 1)                    # every score negative: the best is negative
    assert (score < 0).all()


@pytest.mark.parametrize("noise,seed", model.CASES)
def test_model_loop_separates_planted_shapes(noise, seed):
    """Measured: purity 1.00 on all six cases."""
    P, labels, res = model.planted_case(noise, seed)
    K = model.CASE["K"]
    pur = model.purity(res["cls"], labels, K)
    print("noise %g seed %d: purity %.4f, levels %s, members %s" % (noise, seed, pur, res["levels"],
                                                                     np.bincount(res["cls"], minlength=K).tolist()))
    assert pur >= PURITY_LINE
    assert np.abs(res["shift"]).max() <= model.CASE["R"] and [k for k, _ in res["levels"]] == [1, 2, 3]
    assert all(2 <= used <= model.CASE["iters"] for _, used in res["levels"])
