"""`joint class2d --ctf_weight` on the device (csrc/classctf.hip): the three kernels bit for bit against the NumPy
model of tests/classctf_model.py (outputs and workspaces filled with NaN before every call), the composed path inside its
a-priori bound, the fixed-assignment average, and ``joint class2d --ctf_weight flip`` end to end through the command line on
planted data, judged against the float64 model of the whole loop."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.utils._python_dispatch

import class2d_model
import classctf_model as model
from spr_pick_amd import torch_ops  # noqa: F401  (registers torch.ops.sprk)

pytestmark = pytest.mark.gpu

f32 = np.float32
EPS = model.EPS


def dev(a, dtype=None):
    return torch.as_tensor(np.array(a, dtype=dtype, order="C"), device="cuda")       # a copy: the shared arrays are read-only


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def padded(a, fill=np.nan):
    """[..., Hs] -> [..., roundup(Hs, 4)] on the device, the added columns ``fill`` (nobody may read them)"""
    out = np.full(a.shape[:-1] + ((a.shape[-1] + 3) & ~3,), fill, dtype=f32)
    out[..., :a.shape[-1]] = a
    return dev(out)


def matrices(S):
    from spr_pick_amd import extract
    return extract.filter_matrices(S, S), extract.filter_matrices(S, S, "cuda")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def nan_ws(nbytes):
    return nan(max(int(nbytes), 16) // 4)


# ---- class_spectrum ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def spectrum_case(S):
    """five images and their model spectra, computed once; an image's bits depend on nothing but the image"""
    rng = np.random.default_rng(S)
    imgs = rng.standard_normal((5, S, S)).astype(f32)
    want = np.stack([model.spectrum(i, matrices(S)[0]) for i in imgs])
    imgs.setflags(write=False)
    want.setflags(write=False)
    return imgs, want


def run_spectrum(imgs, S, max_batch):
    """through the C ABI, with a workspace of NaN"""
    from spr_pick_amd import _lib
    L = _lib.lib()
    Hs, Ku, ldv = model.geometry(S)
    W = matrices(S)[1]
    spec, x = nan(len(imgs), 2 * Ku, ldv), dev(imgs)
    ws = nan_ws(L.sprk_class_spectrum_ws_bytes(len(imgs), S, max_batch))
    rc = L.sprk_class_spectrum(ptr(x), len(imgs), S, ptr(W[0]), ptr(W[1]), max_batch, ptr(spec), ptr(ws), ws.numel() * 4, stream())
    assert rc == 0, L.sprk_last_error()
    return spec.cpu().numpy()[:, :, :Hs]


@pytest.mark.parametrize("S", [16, 34, 64, 66, 128])
def test_spectrum_bit_for_bit(S):
    imgs, want = spectrum_case(S)
    for n in (1, 5):
        assert same_bits(run_spectrum(imgs[:n], S, 0), want[:n]), n
    assert same_bits(run_spectrum(imgs, S, 2), want)             # batches of 2, 2 and 1: the same bytes
    # the operator: the same call with a workspace of its own
    Hs, Ku, ldv = model.geometry(S)
    W, spec = matrices(S)[1], nan(5, 2 * Ku, ldv)
    torch.ops.sprk.class_spectrum(dev(imgs), W[0], W[1], 0, spec)
    assert same_bits(spec.cpu().numpy()[:, :, :Hs], want)


# ---- class_wiener ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [(1, 0, 37), (2, 3, 4)])
@pytest.mark.parametrize("S", [16, 64])
def test_wiener_bit_for_bit(S, counts):
    rng = np.random.default_rng(S + sum(counts))
    Hs, Ku, ldv = model.geometry(S)
    n, G, N = 40, 3, sum(counts)
    spec = rng.standard_normal((n, 2 * Ku, Hs)).astype(f32)
    wn = np.abs(rng.standard_normal((G, Ku, Hs))).astype(f32)
    wd = (rng.standard_normal((G, Ku, Hs)) ** 2).astype(f32)
    group = rng.integers(0, G, n).astype(np.int32)
    members = rng.permutation(n)[:N].astype(np.int32)
    members[-1] = members[-2]                                    # a repeated member counts twice
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    tau = 0.75

    def run(group, members, offsets):
        out = nan(3, 2 * Ku, ldv)
        torch.ops.sprk.class_wiener(padded(spec), S, padded(wn), padded(wd), dev(group), dev(members), dev(offsets), tau, out)
        return out.cpu().numpy()[:, :, :Hs]

    want = model.wiener(spec, wn, wd, group, members, offsets, tau, np.full((3, 2 * Ku, Hs), np.nan, f32))
    got = run(group, members, offsets)
    assert same_bits(got, want)
    for k, c in enumerate(counts):
        assert np.isnan(got[k]).all() if c == 0 else np.isfinite(got[k]).all(), k        # the empty class keeps its NaN
    once = members.copy()
    once[-1] = next(m for m in range(n) if m not in members)
    assert not same_bits(run(group, once, offsets)[2], got[2])
    # out-of-range member and group indices behave as their clamped values, offsets past the list as its end
    wild_m, wild_g = members.copy(), group.copy()
    hi, lo = int(np.argmax(members == members.max())), int(np.argmax(members == members.min()))
    clamped_m = members.copy()
    wild_m[hi], clamped_m[hi] = 2 ** 31 - 1, n - 1
    wild_m[lo], clamped_m[lo] = -5, 0
    wild_g[group == G - 1] = 1000
    wild_g[group == 0] = -(2 ** 31)
    wild_o = offsets.copy()
    wild_o[0], wild_o[-1] = -3, N + 100
    assert same_bits(run(wild_g, wild_m, wild_o),
                     model.wiener(spec, wn, wd, group, clamped_m, offsets, tau, np.full((3, 2 * Ku, Hs), np.nan, f32)))


# ---- class_synthesize --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synthesize_case(S):
    rng = np.random.default_rng(S + 7)
    Hs, Ku, _ = model.geometry(S)
    f = rng.standard_normal((3, 2 * Ku, Hs)).astype(f32)
    want = np.stack([model.synthesize(x, matrices(S)[0]) for x in f])
    f.setflags(write=False)
    want.setflags(write=False)
    return f, want


@pytest.mark.parametrize("S", [16, 34, 64, 128])
def test_synthesize_bit_for_bit(S):
    from spr_pick_amd import _lib
    L = _lib.lib()
    f, want = synthesize_case(S)
    W = matrices(S)[1]
    for K in (1, 3):
        x, out = padded(f[:K]), nan(K, S, S)
        ws = nan_ws(L.sprk_class_synthesize_ws_bytes(K, S))
        rc = L.sprk_class_synthesize(ptr(x), K, S, ptr(W[2]), ptr(W[3]), ptr(out), ptr(ws), ws.numel() * 4, stream())
        assert rc == 0, L.sprk_last_error()
        assert same_bits(out.cpu().numpy(), want[:K]), K
    out = nan(3, S, S)
    torch.ops.sprk.class_synthesize(padded(f), S, W[2], W[3], out)
    assert same_bits(out.cpu().numpy(), want)


# ---- composed ----------------------------------------------------------------------------------------------------------------------
def device_average(imgs, S, wn, wd, group, members, offsets, tau, K):
    """images -> the three operators -> averages [K, S, S]; wn, wd [G, Ku, Hs] NumPy"""
    Hs, Ku, ldv = model.geometry(S)
    W = matrices(S)[1]
    spec, fsum, out = nan(len(imgs), 2 * Ku, ldv), nan(K, 2 * Ku, ldv), nan(K, S, S)
    torch.ops.sprk.class_spectrum(dev(imgs), W[0], W[1], 0, spec)
    torch.ops.sprk.class_wiener(spec, S, padded(wn, 0.0), padded(wd, 0.0), dev(group, np.int32), dev(members, np.int32),
                                dev(offsets, np.int32), tau, fsum)
    torch.ops.sprk.class_synthesize(fsum, S, W[2], W[3], out)
    return out.cpu().numpy()


@pytest.mark.parametrize("S", [34, 64])
def test_composed_path_inside_the_apriori_bound_and_equal_to_the_plain_mean(S):
    from spr_pick_amd import ctf
    rng = np.random.default_rng(S + 11)
    Hs = S // 2 + 1
    n = 23
    imgs = rng.standard_normal((n, S, S)).astype(f32)
    wn, wd = (t[:, :, :Hs] for t in ctf.weight_tables(S, model.micrograph_rows(2000.0)[:3], "flip"))
    group = rng.integers(0, 3, n).astype(np.int32)
    members = rng.permutation(n).astype(np.int32)
    got = device_average(imgs, S, wn, wd, group, members, [0, 9, n], 1.0, 2)
    for k, mem in enumerate((members[:9], members[9:])):
        ref, bound = model.apriori_bound(imgs, matrices(S)[0], wn, wd, group, list(mem), 1.0)
        print("S %d class %d: error / bound %.4f" % (S, k, (np.abs(got[k] - ref) / bound).max()))
        assert (np.abs(got[k] - ref) <= bound).all()
    # wn = 1, wd = 0, tau = count: the plain mean, which class_average forms from the same members (angle 0, shift 0: a copy)
    one, zero = np.ones((1, S + 1, Hs), f32), np.zeros((1, S + 1, Hs), f32)
    mem = members[:9]
    got = device_average(imgs, S, one, zero, np.zeros(n, np.int32), mem, [0, 9], 9.0, 1)[0]
    ref, bound = model.apriori_bound(imgs, matrices(S)[0], one, zero, np.zeros(n, np.int32), list(mem), 9.0)
    assert (np.abs(got - ref) <= bound).all()
    plain = nan(1, S, S)
    cs = dev(np.array([[1.0, 0.0]], dtype=f32))
    torch.ops.sprk.class_average(dev(imgs), dev(np.zeros(n, np.int32)), dev(np.zeros((n, 2), np.int32)), cs, dev(mem),
                                 dev(np.array([0, 9], np.int32)), plain)
    mean64 = imgs[mem].astype(np.float64).mean(axis=0)
    plain_bound = (9 + 2) * EPS * np.abs(imgs[mem]).astype(np.float64).mean(axis=0)      # nine adds, the reciprocal, the product
    plain = plain.cpu().numpy()[0]
    assert (np.abs(plain - mean64) <= plain_bound).all()
    # the reference of the Wiener path is the mean up to what the rounded matrices differ from an exact transform pair by,
    # which its bound's slack of 8 roundings holds (four matrices, one rounding each)
    print("S %d: Wiener path against class_average, error / bounds %.4f" % (S, (np.abs(got - plain) / (bound + plain_bound)).max()))
    assert (np.abs(got - plain) <= bound + plain_bound).all()


# ---- fixed assignment ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", model.ONE_CLASS["seeds"])
def test_wiener_average_on_the_device_recovers_what_the_plain_mean_loses(seed):
    """Measured: the CPU case of tests/test_classctf_cpu.py through the three operators."""
    from spr_pick_amd import ctf
    c = model.ONE_CLASS
    S, N = c["S"], c["N"]
    P, obj, mic, rows = model.one_class(seed)
    wn, wd = ctf.weight_tables(S, rows, "flip", "cuda")
    W = matrices(S)[1]
    Hs, Ku, ldv = model.geometry(S)
    spec, fsum, out, plain = nan(N, 2 * Ku, ldv), nan(1, 2 * Ku, ldv), nan(1, S, S), nan(1, S, S)
    members, offsets = dev(np.arange(N, dtype=np.int32)), dev(np.array([0, N], np.int32))
    torch.ops.sprk.class_spectrum(dev(P), W[0], W[1], 0, spec)
    torch.ops.sprk.class_wiener(spec, S, wn, wd, dev(mic, np.int32), members, offsets, 1.0, fsum)
    torch.ops.sprk.class_synthesize(fsum, S, W[2], W[3], out)
    torch.ops.sprk.class_average(dev(P), dev(np.zeros(N, np.int32)), dev(np.zeros((N, 2), np.int32)),
                                 dev(np.array([[1.0, 0.0]], dtype=f32)), members, offsets, plain)
    weighted = model.masked_correlation(out.cpu().numpy()[0].astype(np.float64), obj, c["radius"])
    mean = model.masked_correlation(plain.cpu().numpy()[0].astype(np.float64), obj, c["radius"])
    print("seed %d: Wiener %.4f, plain mean %.4f" % (seed, weighted, mean))
    assert weighted > 0.95 and mean < 0.90


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def write_particles(tmp, P, mic, rows, ctf=True):
    """P as one stack per micrograph beside a particles.star in the layout of `joint extract --ctf` (without the CTF columns:
    of plain `joint extract`) -> (star, the rows in particle order)"""
    from spr_pick_amd import export, micrograph_io
    from spr_pick_amd import ctf as ctf_mod
    lines = [None] * len(P)
    for m in range(len(rows)):
        mem = np.flatnonzero(mic == m)
        name = "mic%d.mrcs" % m
        with open(os.path.join(tmp, name), "wb") as f:
            micrograph_io.write_mrc(f, P[mem])
        u, v, angle, kv, cs, q, apix = (float(x) for x in rows[m])
        cols = "\t%r\t%r\t%r\t%r\t%r\t%r\t%r\t%r\t0.5" % (u, v, angle, kv, cs, q, ctf_mod.MAGNIFICATION, apix) if ctf else ""
        for k, n in enumerate(mem):
            lines[n] = "%d\t%d\t%06d@%s\tmic%d.mrc\t0.5%s\n" % (n, 2 * n, k + 1, name, m, cols)
    star = os.path.join(tmp, "particles.star")
    with open(star, "w") as f:
        f.write(export.PARTICLES_STAR_HEADER)
        if ctf:
            f.write("".join("_rln%s #%d\n" % (c, 6 + k) for k, c in enumerate(ctf_mod.CTF_STAR_COLUMNS[1:])))
        f.writelines(lines)
    return star, lines


@pytest.mark.parametrize("noise,seed,astigmatism", model.CASES)
def test_class2d_ctf_weight_end_to_end(tmp_path, noise, seed, astigmatism):
    """Measured: see the table there; the fraction of particles whose (class, angle, shift) equals the float64
    model's is printed, not gated."""
    from spr_pick_amd import class2d, cli, micrograph_io
    P, labels, mic, rows, ref = model.planted_case(noise, seed, astigmatism)
    c = model.CASE
    star, lines = write_particles(str(tmp_path), P, mic, rows)
    out = os.path.join(str(tmp_path), "cls")
    res = cli.start(["class2d", "--particles", star, "--classes", str(c["K"]), "--out", out, "--angle_step",
                     str(360 // c["A_n"]), "--max_shift", str(c["R"]), "--iters", str(c["iters"]), "--ctf_weight", "flip"])
    assert res["particles"] == c["N"] and [l[0] for l in res["levels"]] == [1, 2, 3]

    # the files, read back
    avgs, header, _ = micrograph_io.parse_mrc(open(os.path.join(out, "classes.mrcs"), "rb").read())
    assert avgs.shape == (c["K"], c["S"], c["S"]) and avgs.dtype == np.float32 and header.mode == 2 and np.isfinite(avgs).all()
    head, names, table = class2d.read_particles_star(os.path.join(out, "particles_class2d.star"))
    assert names[5:14] == ["DefocusU", "DefocusV", "DefocusAngle", "Voltage", "SphericalAberration", "AmplitudeContrast",
                           "Magnification", "DetectorPixelSize", "CtfFigureOfMerit"] and names[14:] == list(class2d.STAR_COLUMNS)
    assert len(table) == c["N"] and all(t.startswith(r.rstrip("\n") + "\t") for t, r in zip(table, lines))
    fields = np.array([t.split()[14:] for t in table], dtype=np.float64)
    cls, psi, origin = fields[:, 0].astype(int) - 1, fields[:, 1], fields[:, 2:].astype(int)
    assert cls.min() >= 0 and cls.max() < c["K"] and np.abs(origin).max() <= c["R"] and (psi >= 0).all() and (psi < 360).all()
    first = open(os.path.join(out, "class2d.txt")).read().split("\n")[0]
    assert first.endswith(", ctf_weight flip, wiener 1.0") and first.startswith("# %d particles of 64x64" % c["N"])
    assert [int(r["members"]) for r in res["classes"]] == np.bincount(cls, minlength=c["K"]).tolist()

    # against the float64 model of the whole loop
    pur, ref_pur = class2d_model.purity(cls, labels, c["K"]), class2d_model.purity(ref["cls"], labels, c["K"])
    ang = np.rint(psi / (360.0 / c["A_n"])).astype(int)
    equal = (cls == ref["cls"]) & (ang == ref["ang"]) & (-origin[:, 1] == ref["shift"][:, 0]) & (-origin[:, 0] == ref["shift"][:, 1])
    print("noise %g seed %d U-V %g: purity %.4f (model %.4f), equal to the model %.4f, levels %s (model %s)"
          % (noise, seed, astigmatism, pur, ref_pur, equal.mean(), res["levels"], ref["levels"]))
    assert pur >= ref_pur - 0.02


class Recorder(torch.utils._python_dispatch.TorchDispatchMode):
    """the names of the sprk operators that run under it"""

    def __init__(self):
        super().__init__()
        self.names = set()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        if name.startswith("sprk."):
            self.names.add(name.split(".")[1])
        return func(*args, **(kwargs or {}))


def test_the_flag_decides_which_operators_run_and_missing_columns_are_refused(tmp_path, capsys):
    from spr_pick_amd import _lib, cli
    new = {"class_spectrum", "class_wiener", "class_synthesize"}
    P, labels, mic, rows = model.planted(64, 48, 2, 0.5)
    os.makedirs(os.path.join(str(tmp_path), "a"))
    star, _ = write_particles(os.path.join(str(tmp_path), "a"), P, mic, rows)
    base = ["class2d", "--particles", star, "--classes", "2", "--iters", "2", "--angle_step", "30"]
    with Recorder() as plain:
        cli.start(base + ["--out", os.path.join(str(tmp_path), "plain")])
    with Recorder() as weighted:
        cli.start(base + ["--out", os.path.join(str(tmp_path), "weighted"), "--ctf_weight", "flip", "--wiener", "0.5"])
    assert not plain.names & new and "class_average" in plain.names
    assert new <= weighted.names and "class_average" not in weighted.names and "class_transform" in weighted.names
    first = open(os.path.join(str(tmp_path), "plain", "class2d.txt")).read().split("\n")[0]
    assert first == "# 48 particles of 64x64, 2 classes, 12 angles, max shift 3, mask radius 27"      # the line it was
    assert open(os.path.join(str(tmp_path), "weighted", "class2d.txt")).read().split("\n")[0] == first + ", ctf_weight flip, wiener 0.5"
    # the stacks of plain `joint extract`: refused with nothing launched and no directory made
    os.makedirs(os.path.join(str(tmp_path), "b"))
    star, _ = write_particles(os.path.join(str(tmp_path), "b"), P, mic, rows, ctf=False)
    out = os.path.join(str(tmp_path), "refused")
    torch.cuda.synchronize()
    before = _lib.lib().sprk_launch_count()
    with pytest.raises(SystemExit):
        cli.start(["class2d", "--particles", star, "--classes", "2", "--out", out, "--ctf_weight", "flip"])
    assert "joint extract --ctf STAR --ctf_correct flip" in capsys.readouterr().err
    assert _lib.lib().sprk_launch_count() == before and not os.path.exists(out)
