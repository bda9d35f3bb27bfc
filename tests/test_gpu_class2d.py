"""`joint class2d` on the device (csrc/class2d.hip): the three kernels bit for bit against the NumPy models of
tests/class2d_model.py, the refusal rules of the C ABI and of the operators, and ``joint class2d`` end to end through the
command line on planted data, judged against the float64 model of the whole loop."""
import functools
import os

import numpy as np
import pytest
import torch

import class2d_model as model
from spr_pick_amd import torch_ops  # noqa: F401  (registers torch.ops.sprk)

pytestmark = pytest.mark.gpu

f32 = np.float32


def dev(a, dtype=None):
    return torch.as_tensor(np.array(a, dtype=dtype, order="C"), device="cuda")       # a copy: the shared arrays are read-only


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


# ---- class_score -----------------------------------------------------------------------------------------------------------
SCORE_N, SCORE_MB = (1, 17, 65, 130), (1, 5, 63, 65, 200)
SCORE_D = (4, 60, 64, 68, 196, 2292)                             # one chunk, ragged, three or more chunks of 64


@functools.lru_cache(maxsize=None)
def score_case(D):
    """operands of the largest shape and their model scores, computed once: every score is a chain of its own, so the
    smaller shapes are slices"""
    rng = np.random.default_rng(D)
    Q = rng.standard_normal((max(SCORE_N), D)).astype(f32)
    B = rng.standard_normal((max(SCORE_MB), D)).astype(f32)
    s = model.score(Q, B, D)
    for a in (Q, B, s):
        a.setflags(write=False)
    return Q, B, s


def run_score(Q, B, D, full=True):
    N, Mb = len(Q), len(B)
    scores = nan(N, Mb) if full else None
    best_score, best_index = nan(N), torch.full((N,), -7, dtype=torch.int32, device="cuda")
    torch.ops.sprk.class_score(dev(Q), dev(B), D, scores, best_score, best_index)
    return (scores.cpu().numpy() if full else None), best_score.cpu().numpy(), best_index.cpu().numpy()


@pytest.mark.parametrize("D", SCORE_D)
@pytest.mark.parametrize("Mb", SCORE_MB)
@pytest.mark.parametrize("N", SCORE_N)
def test_score_bit_for_bit(N, Mb, D):
    Q, B, s = score_case(D)
    want = s[:N, :Mb]
    got, best_score, best_index = run_score(Q[:N], B[:Mb], D)
    assert same_bits(got, want)
    ws, wi = model.best(want)
    assert same_bits(best_score, ws) and np.array_equal(best_index, wi)
    _, best_score, best_index = run_score(Q[:N], B[:Mb], D, full=False)      # without the score matrix
    assert same_bits(best_score, ws) and np.array_equal(best_index, wi)


def test_score_ties_last_column_negative_rows_and_strides():
    rng = np.random.default_rng(11)
    D = 64
    base = rng.standard_normal(D).astype(f32)
    Q = (base + 0.1 * rng.standard_normal((130, D))).astype(f32)
    # duplicated bank rows in different column tiles: the lowest index wins
    B = rng.standard_normal((200, D)).astype(f32)
    B[150] = B[70] = B[10] = 10 * base
    got, best_score, best_index = run_score(Q, B, D)
    want = model.score(Q, B, D)
    assert same_bits(got, want) and same_bits(got[:, 10], got[:, 150]) and same_bits(got[:, 10], got[:, 70])
    assert (best_index == 10).all() and same_bits(best_score, want[:, 10])
    # the best in the last real column, alone in its column tile
    B = rng.standard_normal((65, D)).astype(f32)
    B[64] = 10 * base
    got, best_score, best_index = run_score(Q, B, D)
    want = model.score(Q, B, D)
    assert same_bits(got, want) and (best_index == 64).all() and same_bits(best_score, want[:, 64])
    # every real score negative: the padding's zeros must not win
    Qp, Bn = np.abs(Q[:17]) + f32(0.5), -np.abs(rng.standard_normal((5, D)).astype(f32)) - f32(0.5)
    got, best_score, best_index = run_score(Qp, Bn, D)
    want = model.score(Qp, Bn, D)
    ws, wi = model.best(want)
    assert same_bits(got, want) and (best_score < 0).all() and same_bits(best_score, ws) and np.array_equal(best_index, wi)
    # row strides beyond D (the columns D .. ld-1 are zeros) and a score matrix wider than the bank
    D = 60
    Qw, Bw = np.zeros((17, D + 4), f32), np.zeros((65, D + 12), f32)
    Qw[:, :D], Bw[:, :D] = rng.standard_normal((17, D)), rng.standard_normal((65, D))
    scores, best_score, best_index = nan(17, 70), nan(17), torch.zeros(17, dtype=torch.int32, device="cuda")
    torch.ops.sprk.class_score(dev(Qw), dev(Bw), D, scores, best_score, best_index)
    want = model.score(Qw, Bw, D)
    scores = scores.cpu().numpy()
    assert same_bits(scores[:, :65], want) and np.isnan(scores[:, 65:]).all()
    ws, wi = model.best(want)
    assert same_bits(best_score.cpu().numpy(), ws) and np.array_equal(best_index.cpu().numpy(), wi)


# ---- class_transform ---------------------------------------------------------------------------------------------------------
def transform_table():
    """rows 0 .. 2: 0, 90 and 180 degrees exactly; rows 3 .. 7: five generic angles of the 5-degree table"""
    exact = np.array([[1, 0], [0, 1], [-1, 0]], dtype=f32)
    return np.concatenate([exact, model.angle_table(72)[[1, 7, 23, 50, 71]]])


@functools.lru_cache(maxsize=None)
def transform_sources(S):
    src = np.random.default_rng(S).standard_normal((3, S, S)).astype(f32)
    src.setflags(write=False)
    return src


TRANSFORM_CALL = dict(idx=[0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1],
                      ang=[0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 3],
                      shift=[(0, 0), (3, -2), (-31, 31), (0, 0), (0, 0), (0, 0), (2, 1), (-3, 3), (1, -1), (0, -2), (-31, 31)])


def run_transform(src, idx, ang, shift, cs, radius, flags, pix=None):
    M, S = len(idx), src.shape[1]
    out = nan(M, S, S) if pix is None else nan(M, (len(pix) + 3) & ~3)
    torch.ops.sprk.class_transform(dev(src), dev(idx, np.int32), dev(ang, np.int32), dev(shift, np.int32), dev(cs), radius, flags,
                                   None if pix is None else dev(pix), out)
    return out.cpu().numpy()


@pytest.mark.parametrize("flags", [0, model.MASK, model.NORMALIZE, model.MASK | model.NORMALIZE])
@pytest.mark.parametrize("S", [64, 128])
def test_transform_bit_for_bit(S, flags):
    src, cs, radius = transform_sources(S), transform_table(), S // 2 - 5
    call = TRANSFORM_CALL
    want = model.transform(src, call["idx"], call["ang"], call["shift"], cs, radius, flags)
    got = run_transform(src, call["idx"], call["ang"], call["shift"], cs, radius, flags)
    assert same_bits(got, want)
    if not flags:
        for m in range(3):                                       # angle 0: the zero-filled shifted copy
            assert same_bits(got[m], model.shifted_copy(src[call["idx"][m]], *call["shift"][m])), m
        disc = model.mask_of(S, S // 2 - 1)
        for m in (3, 4):                                         # 90 and 180 degrees: a permutation of the pixels of the disc
            assert np.array_equal(np.sort(got[m][disc]), np.sort(src[call["idx"][m]][disc])), m
    # the packed form of the same call gives the same values, and zeros in the padding columns
    pix = model.packed_pixels(S, radius)
    packed = run_transform(src, call["idx"], call["ang"], call["shift"], cs, radius, flags, pix)
    assert packed.shape[1] % 4 == 0 and same_bits(packed[:, :len(pix)], want.reshape(len(want), -1)[:, pix])
    assert same_bits(packed[:, len(pix):], np.zeros((len(want), packed.shape[1] - len(pix)), f32))
    if flags:
        assert not want[:, ~model.mask_of(S, radius)].any()


def test_transform_flat_image_normalises_to_zeros():
    src = np.full((1, 64, 64), 2.5, f32)
    got = run_transform(src, [0, 0], [0, 5], [(0, 0), (0, 0)], transform_table(), 20, model.NORMALIZE)
    assert same_bits(got, np.zeros_like(got))
    got = run_transform(src, [0], [0], [(0, 0)], transform_table(), 0, model.NORMALIZE)      # one pixel: the norm is 0
    assert same_bits(got, np.zeros_like(got))


# ---- class_average -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 128])
def test_average_bit_for_bit_and_empty_class_untouched(S):
    rng = np.random.default_rng(S + 1)
    n_src, A_n = 40, 72
    src = rng.standard_normal((n_src, S, S)).astype(f32)
    cs = model.angle_table(A_n)
    ang = rng.integers(0, A_n, n_src).astype(np.int32)
    shift = rng.integers(-3, 4, (n_src, 2)).astype(np.int32)
    order = rng.permutation(n_src)[:38]
    members = np.concatenate([order[:1], np.sort(order[1:])]).astype(np.int32)       # counts 1, 0, 37
    offsets = np.array([0, 1, 1, 38], dtype=np.int32)
    out = nan(3, S, S)
    poison = rng.standard_normal((S, S)).astype(f32)
    out[1] = dev(poison)
    torch.ops.sprk.class_average(dev(src), dev(ang), dev(shift), dev(cs), dev(members), dev(offsets), out)
    want = np.full((3, S, S), np.nan, f32)
    want[1] = poison
    model.average(src, ang, shift, cs, members, offsets, want)
    got = out.cpu().numpy()
    assert same_bits(got, want) and same_bits(got[1], poison) and np.isfinite(got).all()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from spr_pick_amd import _lib
    L = _lib.lib()
    S = 64
    src, cs = torch.zeros(3, S, S, device="cuda"), dev(model.angle_table(8))

    def i32(*shape):
        return torch.zeros(*shape, dtype=torch.int32, device="cuda")

    out, packed, pix = nan(2, S, S), nan(2, 2292), dev(model.packed_pixels(S, 27))
    Q, B, bs, bi = torch.zeros(5, 64, device="cuda"), torch.zeros(7, 64, device="cuda"), nan(5), i32(5)
    avg = nan(2, S, S)
    torch.cuda.synchronize()
    before = L.sprk_launch_count()
    bad = [
        ("class_transform", (torch.zeros(3, 48, 50, device="cuda"), i32(2), i32(2), i32(2, 2), cs, 27, 3, None, out)),
        ("class_transform", (torch.zeros(3, 130, 130, device="cuda"), i32(2), i32(2), i32(2, 2), cs, 27, 3, None, out)),
        ("class_transform", (src, i32(2), i32(3), i32(2, 2), cs, 27, 3, None, out)),
        ("class_transform", (src, i32(2), i32(2), i32(2, 2), cs, 65, 1, None, out)),
        ("class_transform", (src, i32(2), i32(2), i32(2, 2), cs, 27, 8, None, out)),
        ("class_transform", (src, i32(2), i32(2), i32(2, 2), cs, 27, 3, pix, nan(2, 2290))),
        ("class_transform", (src, i32(2), i32(2), i32(2, 2), cs, 27, 3, pix, out)),
        ("class_transform", (src, i32(2).long(), i32(2), i32(2, 2), cs, 27, 3, None, out)),
        ("class_transform", (src, i32(2), i32(2), i32(2, 2), cs, 27, 3, None, nan(2, S, S + 1)[:, :, :S])),
        ("class_score", (Q, B, 62, None, bs, bi)), ("class_score", (Q, B, 0, None, bs, bi)), ("class_score", (Q, B, 68, None, bs, bi)),
        ("class_score", (Q, B, 64, nan(5, 6), bs, bi)), ("class_score", (Q, B, 64, None, bs, i32(4))),
        ("class_score", (Q, torch.zeros(7, 62, device="cuda"), 60, None, bs, bi)),
        ("class_average", (src, i32(2), i32(3, 2), cs, i32(3), i32(3), avg)),
        ("class_average", (src, i32(3), i32(3, 2), cs, i32(0), i32(3), avg)),
        ("class_average", (src, i32(3), i32(3, 2), cs, i32(3), i32(4), avg)),
        ("class_average", (src, i32(3), i32(3, 2), cs, i32(3), i32(3), src[:2])),
    ]
    for name, args in bad:
        with pytest.raises(_lib.SprkError):
            getattr(torch.ops.sprk, name)(*args)
    # the C entry points themselves: a misaligned pointer and a stride the operator would not pass on
    assert L.sprk_class_score(Q.data_ptr() + 4, 64, 5, B.data_ptr(), 64, 7, 64, None, 0, bs.data_ptr(), bi.data_ptr(), None) == -1
    assert b"aligned" in L.sprk_last_error()
    assert L.sprk_class_transform(src.data_ptr(), 3, S, i32(2).data_ptr(), i32(2).data_ptr(), i32(2, 2).data_ptr(), 2,
                                  cs.data_ptr(), 8, 27, 3, pix.data_ptr(), 2289, 2290, packed.data_ptr(), None) == -1
    assert b"packed" in L.sprk_last_error()
    torch.cuda.synchronize()
    assert L.sprk_launch_count() == before
    for t in (out, packed, bs, avg):
        assert torch.isnan(t).all()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape_bank(S, radius, A_n=120):
    """every planted shape at A_n rotations, under the mask, zero mean and unit norm -> [3 * A_n, D]"""
    inside = model.mask_of(S, radius)
    rows = np.stack([model.unit_shape(kind, S, 2 * np.pi * t / A_n, radius)[inside] for kind in range(3) for t in range(A_n)])
    rows = rows - rows.mean(axis=1, keepdims=True)
    return rows / np.sqrt((rows ** 2).sum(axis=1, keepdims=True))


def shape_correlations(averages, S, radius):
    """-> per class average its largest correlation under the mask with any planted shape at any rotation"""
    v = averages[:, model.mask_of(S, radius)].astype(np.float64)
    v = v - v.mean(axis=1, keepdims=True)
    v = v / np.sqrt((v ** 2).sum(axis=1, keepdims=True))
    return (v @ shape_bank(S, radius).T).max(axis=1)


def write_particles(tmp, P, sizes=(170,)):
    """P as stacks beside a particles.star with CTF columns, in the layout of `joint extract --ctf`"""
    from spr_pick_amd import export, micrograph_io
    bounds = [0] + list(np.cumsum(sizes)) + [len(P)]
    rows = []
    for s, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        name = "mic%d.mrcs" % s
        with open(os.path.join(tmp, name), "wb") as f:
            micrograph_io.write_mrc(f, P[a:b])
        rows += ["%d\t%d\t%06d@%s\tmic%d.mrc\t0.5\t15000.0\t14000.0\n" % (k, 2 * k, k + 1, name, s) for k in range(b - a)]
    star = os.path.join(tmp, "particles.star")
    with open(star, "w") as f:
        f.write(export.PARTICLES_STAR_HEADER + "_rlnDefocusU #6\n_rlnDefocusV #7\n")
        f.writelines(rows)
    return star, rows


@pytest.mark.parametrize("noise,seed", model.CASES)
def test_class2d_end_to_end(tmp_path, noise, seed):
    """Measured: see the table there; the fraction of particles whose (class, angle, shift) equals the float64
    model's is printed, not gated."""
    from spr_pick_amd import class2d, cli, micrograph_io
    P, labels, ref = model.planted_case(noise, seed)
    c = model.CASE
    radius = c["S"] // 2 - c["R"] - 2
    star, rows = write_particles(str(tmp_path), P)
    out = os.path.join(str(tmp_path), "cls")
    res = cli.start(["class2d", "--particles", star, "--classes", str(c["K"]), "--out", out, "--angle_step",
                     str(360 // c["A_n"]), "--max_shift", str(c["R"]), "--iters", str(c["iters"])])
    assert res["particles"] == c["N"] and [l[0] for l in res["levels"]] == [1, 2, 3]

    # the files, read back
    avgs, header, _ = micrograph_io.parse_mrc(open(os.path.join(out, "classes.mrcs"), "rb").read())
    assert avgs.shape == (c["K"], c["S"], c["S"]) and avgs.dtype == np.float32 and header.mode == 2 and np.isfinite(avgs).all()
    head, names, table = class2d.read_particles_star(os.path.join(out, "particles_class2d.star"))
    assert names[:7] == ["CoordinateX", "CoordinateY", "ImageName", "MicrographName", "AutopickFigureOfMerit", "DefocusU",
                         "DefocusV"] and names[7:] == list(class2d.STAR_COLUMNS)
    assert [h for h in head if h.startswith("_rln")][-4:] == ["_rln%s #%d" % (n, 8 + k) for k, n in enumerate(class2d.STAR_COLUMNS)]
    assert len(table) == c["N"] and all(t.startswith(r.rstrip("\n") + "\t") for t, r in zip(table, rows))
    fields = np.array([t.split()[7:] for t in table], dtype=np.float64)
    cls, psi, origin = fields[:, 0].astype(int) - 1, fields[:, 1], fields[:, 2:].astype(int)
    assert cls.min() >= 0 and cls.max() < c["K"] and np.abs(origin).max() <= c["R"] and (psi >= 0).all() and (psi < 360).all()
    text = open(os.path.join(out, "class2d.txt")).read()
    assert [int(r["members"]) for r in res["classes"]] == np.bincount(cls, minlength=c["K"]).tolist() and "iterations" in text

    # against the float64 model of the whole loop
    pur, ref_pur = model.purity(cls, labels, c["K"]), model.purity(ref["cls"], labels, c["K"])
    ang = np.rint(psi / (360.0 / c["A_n"])).astype(int)
    equal = (cls == ref["cls"]) & (ang == ref["ang"]) & (-origin[:, 1] == ref["shift"][:, 0]) & (-origin[:, 0] == ref["shift"][:, 1])
    corr, ref_corr = shape_correlations(avgs, c["S"], radius), shape_correlations(ref["averages"], c["S"], radius)
    print("noise %g seed %d: purity %.4f (model %.4f), equal to the model %.4f, levels %s (model %s), correlations %s (model %s)"
          % (noise, seed, pur, ref_pur, equal.mean(), res["levels"], ref["levels"], np.round(corr, 3), np.round(ref_corr, 3)))
    assert pur >= ref_pur - 0.02
    assert (corr >= 0.5 * ref_corr.min()).all()


def test_class2d_refuses_a_side_of_48(tmp_path, capsys):
    from spr_pick_amd import _lib, cli
    star, _ = write_particles(str(tmp_path), np.zeros((6, 48, 48), f32), sizes=(4,))
    before = _lib.lib().sprk_launch_count()
    with pytest.raises(SystemExit):
        cli.start(["class2d", "--particles", star, "--classes", "2", "--out", os.path.join(str(tmp_path), "cls")])
    assert "--scale 64" in capsys.readouterr().err
    assert _lib.lib().sprk_launch_count() == before and not os.path.exists(os.path.join(str(tmp_path), "cls"))
