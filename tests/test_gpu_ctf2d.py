"""GPU: the scores of the 2-D Thon-ring fit (csrc/ctffit.hip, ``torch.ops.sprk.ctf_score``) against the NumPy
model of their contract (tests/ctf2d_model.py) within the a-priori bound, the same bits on a second call and whatever the
output and the workspace held, the C ABI's refusals, the device fit against the model's on a planted case, and the command
line: ``joint ctf --astigmatism`` and the join into ``joint extract --ctf``."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import ctf2d_model
from test_ctf2d_cpu import CASES, case_bins, case_seed, case_spectrum, check_fit, planted_image
from test_gpu_ingest import write_raw_mrc

pytestmark = pytest.mark.gpu

# (bins, candidates, row stride): one lane of one wave; below and above one 16 x 16 tile; one bin; a ragged chunk and a
# ragged workgroup; four workgroups of candidates; several slices of several chunks; few candidates and many bins (79
# slices); a row stride above n with NaN behind the bins
SIZES = [(1, 1, 4), (15, 17, 16), (17, 1, 20), (63, 300, 64), (1003, 65, 1004), (5000, 1000, 5000), (20011, 16, 20012),
         (1003, 65, 1040)]


@functools.lru_cache(maxsize=None)
def synthetic(n, ncand):
    """bins and candidates in the ranges of a real fit -> (bins float32 [5, n], cand float32 [ncand, 3], the model's S)"""
    rng = np.random.RandomState(n * 31 + ncand)
    p = rng.uniform(2e-4, 0.02, n)
    phi2 = rng.uniform(-np.pi, np.pi, n)
    bins = np.stack([rng.uniform(0, 1, n), p, p * np.cos(phi2), p * np.sin(phi2), 0.3 * rng.randn(n)]).astype(np.float32)
    cand = np.stack([rng.uniform(-600, 600, ncand), rng.uniform(-1050, 1050, ncand), rng.uniform(-1050, 1050, ncand)],
                    axis=1).astype(np.float32)
    want = ctf2d_model.sums(bins, cand)
    for a in (bins, cand, want):
        a.setflags(write=False)
    return bins, cand, want


def ctf_score(bins, cand):
    from spr_pick_amd import torch_ops  # noqa: F401  (registers torch.ops.sprk.*)
    return torch.ops.sprk.ctf_score(bins, cand)


def upload(bins, ldb):
    """-> a [5, n] view of a [5, ldb] device buffer whose other columns hold NaN"""
    buf = torch.full((5, ldb), float("nan"), device="cuda")
    buf[:, :bins.shape[1]] = torch.from_numpy(np.array(bins))
    return buf[:, :bins.shape[1]]


@pytest.mark.parametrize("n,ncand,ldb", SIZES, ids=["%dx%d-ld%d" % s for s in SIZES])
def test_sums_lie_within_the_bound_of_the_model(n, ncand, ldb):
    bins, cand, want = synthetic(n, ncand)
    b, c = upload(bins, ldb), torch.from_numpy(np.array(cand)).cuda()
    got = ctf_score(b, c)
    assert got.dtype == torch.float64 and tuple(got.shape) == (ncand, 3)
    ratio = ctf2d_model.check(got.cpu().numpy(), bins, cand, want)
    print("%d bins x %d candidates, stride %d: worst error / a-priori bound of S1, S2, S3: %.3g %.3g %.3g"
          % (n, ncand, ldb, *ratio))
    again = ctf_score(b, c)
    assert torch.equal(got, again)                               # a fixed order: the same bits
    assert np.array_equal(np.isnan(b._base.cpu().numpy()), np.arange(ldb)[None, :] >= n * np.ones((5, 1)))


def test_output_and_workspace_may_hold_anything():
    """Through the C ABI with an output and a workspace this test owns, both filled with NaN (the workspace well past its
    end): the bits of the operator's result, and nothing written past either."""
    from spr_pick_amd import _lib
    L = _lib.lib()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    slices = []
    for n, ncand, ldb in SIZES[3:]:
        bins, cand, want = synthetic(n, ncand)
        b, c = upload(bins, ldb), torch.from_numpy(np.array(cand)).cuda()
        ref = ctf_score(b, c)
        need = L.sprk_ctf_score_ws_bytes(n, ncand)
        assert need % (ncand * 24) == 0
        slices.append(need // (ncand * 24))
        ws = torch.full((need // 8 + 4096,), float("nan"), device="cuda", dtype=torch.float64)
        out = torch.full((ncand + 64, 3), float("nan"), device="cuda", dtype=torch.float64)
        rc = L.sprk_ctf_score(b.data_ptr(), ldb, n, c.data_ptr(), ncand, out.data_ptr(), ws.data_ptr(), need, s)
        assert rc == 0, L.sprk_last_error()
        assert torch.equal(out[:ncand], ref) and torch.isnan(out[ncand:]).all()
        assert torch.isnan(ws[need // 8:]).all() and not torch.isnan(ws[:need // 8]).any()
        ctf2d_model.check(out[:ncand].cpu().numpy(), bins, cand, want)
    assert slices[0] == 0 and slices[2] >= 4 and slices[3] == 79          # one slice needs no workspace


def test_c_abi_refusals_launch_nothing():
    from spr_pick_amd import _lib
    L = _lib.lib()
    EINVAL, EWORKSPACE = -1, -2
    n, ncand, ldb = SIZES[5]
    bins, cand, want = synthetic(n, ncand)
    b, c = upload(bins, ldb), torch.from_numpy(np.array(cand)).cuda()
    out = torch.zeros(ncand, 3, device="cuda", dtype=torch.float64)
    need = L.sprk_ctf_score_ws_bytes(n, ncand)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(bins=b.data_ptr(), ldb=ldb, n=n, cand=c.data_ptr(), ncand=ncand, out=out.data_ptr(), ws=ws.data_ptr(),
                ws_bytes=need)

    def call(**change):
        a = dict(good, **change)
        return L.sprk_ctf_score(a["bins"], a["ldb"], a["n"], a["cand"], a["ncand"], a["out"], a["ws"], a["ws_bytes"], s)

    torch.cuda.synchronize()
    before = L.sprk_launch_count()
    cases = [(dict(n=0), EINVAL, b"bins"), (dict(n=-1), EINVAL, b"bins"), (dict(n=(1 << 20) + 1, ldb=(1 << 20) + 4), EINVAL, b"bins"),
             (dict(ncand=0), EINVAL, b"candidates"), (dict(ncand=(1 << 24) + 1), EINVAL, b"candidates"),
             (dict(ldb=n - 4), EINVAL, b"ldb"), (dict(ldb=n + 2), EINVAL, b"ldb"),
             (dict(bins=None), EINVAL, b"null"), (dict(cand=None), EINVAL, b"null"), (dict(out=None), EINVAL, b"null"),
             (dict(bins=b.data_ptr() + 4), EINVAL, b"aligned"), (dict(cand=c.data_ptr() + 4), EINVAL, b"aligned"),
             (dict(out=out.data_ptr() + 8), EINVAL, b"aligned"), (dict(ws=ws.data_ptr() + 8), EINVAL, b"aligned"),
             (dict(ws_bytes=need - 1), EWORKSPACE, b"workspace"), (dict(ws=None, ws_bytes=0), EWORKSPACE, b"workspace")]
    for change, code, word in cases:
        assert call(**change) == code, (change, L.sprk_last_error())
        assert word in L.sprk_last_error(), (change, L.sprk_last_error())
    assert L.sprk_launch_count() == before
    assert not out.any()                                         # nothing was written either
    assert call() == 0, L.sprk_last_error()
    assert L.sprk_launch_count() == before + 2                   # the slices and their sum
    ctf2d_model.check(out.cpu().numpy(), bins, cand, want)
    # the operator refuses the same before the library is called
    for bad_b, bad_c in ((b[:4], c), (b.double(), c), (b, c[:, :2]), (b, c.double()), (b[:, :0], c), (b, c[:0]),
                         (torch.zeros(5, n + 2, device="cuda")[:, :n], c), (b[:, 1:], c), (b, c.cpu())):
        with pytest.raises(_lib.SprkError):
            ctf_score(bad_b, bad_c)
    assert L.sprk_launch_count() == before + 2


def score_bound(S, Y, dS):
    """how far the score of sums within dS of S can lie from that of S, to first order in dS (doubled for the rest)"""
    n = Y.size
    sy, syy = Y.sum(), (Y * Y).sum()
    var = S[:, 1] - S[:, 0] ** 2 / n
    cov = np.abs(S[:, 2] - S[:, 0] * sy / n)
    d_cov = dS[2] + dS[0] * abs(sy) / n
    d_var = dS[1] + 2 * np.abs(S[:, 0]) * dS[0] / n
    return 2 * (d_cov / np.sqrt(var * syy) + cov * d_var / (2 * var * np.sqrt(var * syy)))


def test_the_fit_of_a_planted_case_on_the_device_and_by_the_model():
    """The bins of planted (512, 128, 2.0, 20000, 400, 60) with the fit's two grids: every candidate's sums and score
    within the bound of the model's, and the device fit within one fine step (5 Angstrom in each of d0, e1, e2) of the
    model's — near-ties may flip."""
    from spr_pick_amd import ctf
    case = CASES[0]
    _, T, apix = case[:3]
    bins, d_ref = case_bins(case)
    Y = bins[4].astype(np.float64)
    coarse, fine = ctf.astigmatism_grids(1000.0)
    assert len(coarse) == 26397 and len(fine) == 9261
    want = ctf2d_model.sums(bins, coarse.astype(np.float32))
    best = coarse[int(np.argmax(ctf.score(want, Y)))]
    dS = ctf2d_model.bound(bins)
    picks = []
    for name, cand, ref in (("coarse", coarse, want), ("fine", best + fine, None)):
        cand = cand.astype(np.float32)
        ref = ctf2d_model.sums(bins, cand) if ref is None else ref
        got = ctf.device_sums(bins, cand)
        ratio = ctf2d_model.check(got, bins, cand, ref)
        s_dev, s_ref = ctf.score(got, Y), ctf.score(ref, Y)
        tol = score_bound(ref, Y, dS)
        print("%s grid, %d bins x %d candidates: sums at %.3g %.3g %.3g of their bound; scores differ by at most %.3g "
              "(bound %.3g), best %.6f" % (name, bins.shape[1], len(cand), *ratio, np.abs(s_dev - s_ref).max(), tol.max(),
                                           s_ref.max()))
        assert (np.abs(s_dev - s_ref) <= tol).all() and tol.max() < 1e-5
        picks.append((cand[int(np.argmax(s_dev))], cand[int(np.argmax(s_ref))]))
    # the model's fit is the best of its fine grid (the first of equal scores: argmax); the device's runs on its own
    model = picks[1][1].astype(np.float64) + (d_ref, 0.0, 0.0)
    u, v, angle, score = ctf.fit_astigmatism(case_spectrum(case), T, apix)
    d1, a = (u - v) / 2, np.radians(2 * angle)
    device = np.array([(u + v) / 2, d1 * np.cos(a), d1 * np.sin(a)])
    print("device fit (d0, e1, e2) %s score %.6f, model fit %s" % (device, score, model))
    assert np.abs(device - model).max() <= 5.0 + 1e-6
    check_fit(case, u, v, angle, "device sums")


def test_joint_ctf_astigmatism_and_the_join_into_extract(tmp_path):
    """`joint ctf --astigmatism` on two planted 512^2 int16 micrographs (T = 128, 2 Angstrom per pixel): the rows are what
    the host fit makes of the device's spectrum and sums, and meet the conditions of test_ctf2d_cpu; `joint extract --ctf
    --bin 2` carries them through with the pixel size doubled; without the flag the table is the 1-D fit's, as before."""
    from spr_pick_amd import cli, ctf, export
    root, T, apix = str(tmp_path), 128, 2.0
    # the second file: the defocus, astigmatism and angle of CASES[1] at this size.  A 512^2 micrograph gives 49 tiles of
    # 128 and 5158 bins, and e1 and e2 scatter by about 100 Angstrom between noise realisations: the
    # largest d1 of the issue's cases leaves the angle condition the most room (100 / (2 x 800) rad = 3.6 degrees)
    cases = [CASES[0], (512, 128, 2.0, 12000, 800, 150)]
    lines = ["image_name\tpath"]
    for k, case in enumerate(cases):
        path = os.path.join(root, "mic%d.mrc" % k)
        write_raw_mrc(path, planted_image(case[0], apix, *case[3:], seed=case_seed(case)), 1)
        lines.append("mic%d\t%s" % (k, path))
    dataset = os.path.join(root, "raw.txt")
    open(dataset, "w").write("\n".join(lines) + "\n")
    base = ["ctf", "--dataset", dataset, "--tile", "128", "--apix", "2.0"]
    res = cli.start(base + ["--out", str(tmp_path / "astig"), "--astigmatism"])
    plain = cli.start(base + ["--out", str(tmp_path / "plain")])
    want_rows, want_plain = [], []
    for k, case in enumerate(cases):
        Pm = ctf.power_spectrum(os.path.join(root, "mic%d.mrc" % k), T)
        u, v, angle, score = ctf.fit_astigmatism(Pm, T, apix)
        check_fit(case, u, v, angle, "joint ctf --astigmatism")
        r = res["mic%d" % k]
        assert (r["defocus_u"], r["defocus_v"], r["angle"], r["score_2d"]) == (u, v, angle, score)
        want_rows.append(ctf.star_row("mic%d.mrc" % k, u, score, apix, 300.0, 2.7, 0.07, v, angle))
        defocus, score1 = ctf.fit_defocus(ctf.radial_profile(Pm), T, apix)
        assert plain["mic%d" % k] == {"defocus": defocus, "score": score1, "apix": apix, "tiles": 49}
        want_plain.append("mic%d.mrc\t%.2f\t%.2f\t0.00\t300.00\t2.7000\t0.0700\t10000.00\t%.5f\t%.6f\n"
                          % (k, defocus, defocus, apix, score1))
        for suffix in ("_psd.mrc", "_profile.txt"):
            assert open(str(tmp_path / "astig" / ("mic%d%s" % (k, suffix))), "rb").read() == \
                open(str(tmp_path / "plain" / ("mic%d%s" % (k, suffix))), "rb").read()
    star = str(tmp_path / "astig" / "micrographs_ctf.star")
    assert open(star).read() == ctf.CTF_STAR_HEADER + "".join(want_rows)
    assert open(str(tmp_path / "plain" / "micrographs_ctf.star")).read() == ctf.CTF_STAR_HEADER + "".join(want_plain)

    picks = os.path.join(root, "mic0_scores.txt")
    pts = [(100, 120, 0.9), (300, 200, 0.8), (256, 256, 0.6)]
    open(picks, "w").write("image_name\tx_coord\ty_coord\tscore\n" + "".join("mic0\t%d\t%d\t%s\n" % p for p in pts))
    ex = str(tmp_path / "ex")
    cli.start(["extract", "--dataset", dataset, "--picks", picks, "--box", "64", "--out", ex, "--ctf", star, "--bin", "2"])
    text = open(os.path.join(ex, "particles.star")).read()
    header = export.PARTICLES_STAR_HEADER + "".join("_rln%s #%d\n" % (c, 6 + k) for k, c in enumerate(ctf.CTF_STAR_COLUMNS[1:]))
    assert text.startswith(header)
    rows = text[len(header):].splitlines()
    fields = want_rows[0].rstrip("\n").split("\t")
    assert float(fields[1]) > float(fields[2]) and fields[3] != "0.00"
    fields[8] = "%.5f" % (apix * 2)
    assert len(rows) == 3
    for row, p, k in zip(rows, pts, range(3)):
        assert row == "%d\t%d\t%06d@mic0.mrcs\tmic0.mrc\t%s\t" % (p[0], p[1], k + 1, p[2]) + "\t".join(fields[1:])
