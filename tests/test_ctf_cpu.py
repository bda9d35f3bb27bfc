"""CPU: the host half of `joint ctf` (spr_pick_amd/ctf.py) without a GPU — radial bins against an
exact-integer brute force, the defocus fit on planted images (the spectrum by np.fft in place of the device), the command
line's refusals, the pixel-size fallback, the bytes of micrographs_ctf.star and the `joint extract --ctf` join."""
import os

import numpy as np
import pytest

import psd_model

# (side, T, apix, planted defocus, ramp in sigma across x, astigmatism: half the difference of the two defoci)
FIT_CASES = [(1024, 256, 1.0, 8000, 0, 0), (1024, 256, 1.0, 15000, 0, 0), (1024, 256, 1.0, 25000, 0, 0),
             (1024, 256, 1.0, 15000, 3, 0), (768, 128, 1.5, 12000, 0, 0), (512, 128, 2.0, 20000, 0, 0),
             (2048, 512, 0.8, 18000, 0, 0), (1024, 256, 1.0, 15000, 0, 500)]
FIT_LIMIT = 500.0                                # Angstrom: the issue's condition, not a measurement


def planted_image(side, apix, defocus, seed, ramp=0.0, astig=0.0, kv=300.0, cs=2.7, ac=0.07):
    """White noise filtered by the CTF times exp(-40 s^2), scaled to 0.3 of the unit white noise added on top, as int16
    1000 + 100 img.  astig: the defocus is ``defocus + astig cos(2 theta)``; ramp: that many sigma of a linear ramp across x."""
    from spr_pick_amd import ctf
    rng = np.random.RandomState(seed)
    fy, fx = np.fft.fftfreq(side, apix)[:, None], np.fft.rfftfreq(side, apix)[None, :]
    s = np.sqrt(fy * fy + fx * fx)
    dz = defocus + astig * np.cos(2 * np.arctan2(fy, fx))
    lam = ctf.wavelength(kv)
    chi = np.pi * lam * dz * s ** 2 - 0.5 * np.pi * cs * 1e7 * lam ** 3 * s ** 4 + np.arctan2(ac, np.sqrt(1 - ac * ac))
    signal = np.fft.irfft2(np.fft.rfft2(rng.randn(side, side)) * (-np.sin(chi)) * np.exp(-40 * s * s), s=(side, side))
    img = 0.3 * signal / signal.std() + rng.randn(side, side)
    if ramp:
        img = img + ramp * img.std() * np.linspace(-0.5, 0.5, side)[None, :]
    return np.round(1000 + 100 * img).astype(np.int16)


def fft_power(img, T):
    """sum over the tiles of |rfft2(D_t)|^2 in float64 -> (P, ntiles)"""
    Dt = psd_model.tiles(img, T).astype(np.float64)
    F = np.fft.rfft2(Dt)
    return (F.real ** 2 + F.imag ** 2).sum(axis=0), Dt.shape[0]


@pytest.mark.parametrize("T", [16, 48, 128])
def test_radial_bins_against_exact_integers(T):
    from fractions import Fraction
    from spr_pick_amd import ctf
    k = ctf.radial_bins(T)
    assert k.shape == (T, T // 2 + 1)
    rng = np.random.RandomState(T)
    Pm = rng.rand(T, T // 2 + 1)
    sums, counts = [Fraction(0)] * (T // 2 + 1), [0] * (T // 2 + 1)
    for u in range(T):
        us = u if u <= T // 2 else u - T
        for v in range(T // 2 + 1):
            r4 = 4 * (us * us + v * v)
            kk = next(c for c in range(2 * T) if (c == 0 or (2 * c - 1) ** 2 <= r4) and r4 < (2 * c + 1) ** 2)
            assert k[u, v] == kk
            if kk <= T // 2:
                sums[kk] += Fraction(float(Pm[u, v]))
                counts[kk] += 1
    want = np.array([float(s / c) for s, c in zip(sums, counts)])
    got = ctf.radial_profile(Pm)
    assert got.shape == (T // 2 + 1,) and counts[0] == 1
    assert np.abs(got - want).max() <= 1e-14 * want.max()
    with pytest.raises(ValueError):
        ctf.radial_profile(Pm[:, :-1])


@pytest.mark.parametrize("case", FIT_CASES, ids=["%d-T%d-apix%g-dz%d-ramp%d-astig%d" % c for c in FIT_CASES])
def test_fit_recovers_the_planted_defocus(case):
    from spr_pick_amd import ctf
    side, T, apix, dz, ramp, astig = case
    img = planted_image(side, apix, dz, seed=side + dz, ramp=ramp, astig=astig)
    P, ntiles = fft_power(img, T)
    profile = ctf.radial_profile(ctf.mean_power(P, ntiles, T))
    got, score = ctf.fit_defocus(profile, T, apix)
    print("side %d T %d apix %g planted %d ramp %d astig %d: fitted %.0f (error %+.0f A), score %.3f"
          % (side, T, apix, dz, ramp, astig, got, got - dz, score))
    assert abs(got - dz) <= FIT_LIMIT
    assert 0 < score <= 1


def test_fit_is_a_pure_function_of_its_arguments_and_refuses_bad_ones():
    from spr_pick_amd import ctf
    s = np.arange(129) / (256 * 1.5)
    profile = np.exp(-30 * s) * (0.2 + ctf.ctf(s, 17340.0, 300.0, 2.7, 0.07) ** 2) + 0.05
    got, score = ctf.fit_defocus(profile, 256, 1.5)
    assert abs(got - 17340) <= 100 and got % 5 == 0 and 0 < score <= 1
    assert ctf.fit_defocus(profile, 256, 1.5) == (got, score)
    assert ctf.fit_defocus(profile, 256, 1.5, min_defocus=17000, max_defocus=17200)[0] <= 17200
    assert abs(ctf.wavelength(300.0) - 0.019687) < 1e-5 and abs(ctf.wavelength(200.0) - 0.025079) < 1e-5
    for kw in (dict(apix=0), dict(kv=-1), dict(cs=-0.1), dict(ac=1.0), dict(ac=-0.1), dict(min_res=0),
               dict(max_res=40.0), dict(max_res=2.0), dict(min_defocus=6000, max_defocus=5000), dict(min_defocus=0),
               dict(min_res=8.0, max_res=7.5)):
        args = dict(apix=1.5)
        args.update(kw)
        with pytest.raises(ValueError):
            ctf.fit_defocus(profile, 256, **args)
    with pytest.raises(ValueError):
        ctf.fit_defocus(np.zeros(129), 256, 1.5)


def test_parser():
    from spr_pick_amd import cli
    p = cli.build_parser()
    base = ["ctf", "--dataset", "raw", "--out", "o"]
    a = vars(p.parse_args(base))
    assert a["command"] == "ctf" and a["apix"] is None and a["kv"] == 300 and a["cs"] == 2.7 and a["ac"] == 0.07
    assert a["tile"] == 512 and a["min_res"] == 30 and a["max_res"] is None
    assert a["min_defocus"] == 3000 and a["max_defocus"] == 50000
    b = vars(p.parse_args(base + "--apix 1.06 --kv 200 --cs 2.0 --ac 0.1 --tile 256 --min_res 40 --max_res 5 --min_defocus 5000 "
                                 "--max_defocus 30000".split()))
    assert (b["apix"], b["kv"], b["cs"], b["ac"], b["tile"]) == (1.06, 200, 2.0, 0.1, 256)
    assert (b["min_res"], b["max_res"], b["min_defocus"], b["max_defocus"]) == (40, 5, 5000, 30000)
    for bad in (["--tile", "100"], ["--tile", "8"], ["--tile", "2048"], ["--tile", "x"], ["--apix", "0"], ["--apix", "-1"],
                ["--kv", "0"], ["--cs", "-1"], ["--ac", "1"], ["--ac", "-0.2"], ["--min_res", "0"],
                ["--min_res", "5", "--max_res", "6"], ["--apix", "2", "--max_res", "3"],
                ["--min_defocus", "9000", "--max_defocus", "8000"], ["--min_defocus", "-5"]):
        with pytest.raises(SystemExit):
            p.parse_args(base + bad)
    with pytest.raises(SystemExit):
        p.parse_args(["ctf", "--dataset", "raw"])
    ex = ["extract", "-d", "raw", "-p", "picks", "-b", "64", "-o", "out"]
    assert vars(p.parse_args(ex))["ctf"] is None
    assert vars(p.parse_args(ex + ["--ctf", "m.star"]))["ctf"] == "m.star"


def test_apix_fallback_and_its_error():
    from spr_pick_amd import ctf, micrograph_io
    fields = dict(zip(micrograph_io.MRCHeader._fields, [0] * len(micrograph_io.MRCHeader._fields)))
    h = micrograph_io.MRCHeader(**dict(fields, nx=4096, ny=4096, mx=4096, xlen=4341.76))
    assert abs(ctf.header_apix(h) - 1.06) < 1e-12
    for mx, xlen in ((0, 4341.76), (4096, 0.0), (4096, float("nan")), (-1, 10.0), (1, 1.0)):
        assert ctf.header_apix(micrograph_io.MRCHeader(**dict(fields, nx=4096, ny=4096, mx=mx, xlen=xlen))) is None


def test_ctf_dataset_asks_for_apix_when_the_header_has_none(tmp_path, monkeypatch):
    """the error comes before any device work: a header written without a pixel size, and no --apix"""
    from spr_pick_amd import ctf, ingest, micrograph_io
    path = str(tmp_path / "mic0.mrc")
    with open(path, "wb") as f:
        micrograph_io.write_mrc(f, np.zeros((64, 64), dtype=np.float32))

    def read_raw(p, device):
        with open(p, "rb") as f:
            return object(), ingest.read_header(p, f)[0]
    monkeypatch.setattr(ingest, "read_raw", read_raw)
    monkeypatch.setattr(ctf, "psd_sum", lambda *a: pytest.fail("the device was asked for a spectrum"))
    with pytest.raises(ValueError, match="--apix"):
        ctf.ctf_dataset(str(tmp_path), str(tmp_path / "out"), tile=32)
    with pytest.raises(ValueError, match="Nyquist"):
        ctf.ctf_dataset(str(tmp_path), str(tmp_path / "out"), tile=32, apix=3.0, max_res=5.0)


def test_star_bytes_and_reader(tmp_path):
    from spr_pick_amd import ctf
    assert ctf.CTF_STAR_HEADER == (
        "# version 30001\n\ndata_\n\nloop_\n_rlnMicrographName #1\n_rlnDefocusU #2\n_rlnDefocusV #3\n_rlnDefocusAngle #4\n"
        "_rlnVoltage #5\n_rlnSphericalAberration #6\n_rlnAmplitudeContrast #7\n_rlnMagnification #8\n"
        "_rlnDetectorPixelSize #9\n_rlnCtfFigureOfMerit #10\n")
    row = ctf.star_row("mic0.mrc", 15005.0, 0.4321987, 1.06, 300.0, 2.7, 0.07)
    assert row == "mic0.mrc\t15005.00\t15005.00\t0.00\t300.00\t2.7000\t0.0700\t10000.00\t1.06000\t0.432199\n"
    path = str(tmp_path / "m.star")
    open(path, "w").write(ctf.CTF_STAR_HEADER + row + ctf.star_row("mic1.mrc", 8000.0, 0.2, 1.06, 300.0, 2.7, 0.07))
    table = ctf.read_ctf_star(path)
    assert list(table) == ["mic0.mrc", "mic1.mrc"]
    assert table["mic0.mrc"]["DefocusU"] == "15005.00" and table["mic1.mrc"]["DetectorPixelSize"] == "1.06000"
    open(path, "w").write("data_\n\nloop_\n_rlnMicrographName #1\n_rlnDefocusU #2\nmic0.mrc\t1.0\n")
    with pytest.raises(ValueError):
        ctf.read_ctf_star(path)


def _fake_extract(monkeypatch):
    """`extract_dataset` without a device: every box comes back as zeros with status 0"""
    from spr_pick_amd import extract

    def fake(b):
        return lambda path, xy, *a: (np.zeros((len(xy), b, b), dtype=np.float32), np.zeros(len(xy), dtype=np.int32))
    monkeypatch.setattr(extract, "_extract_file", lambda path, xy, box, bin, *a: fake(box // bin)(path, xy))
    monkeypatch.setattr(extract, "_extract_file_scaled", lambda path, xy, box, scale, *a: fake(scale)(path, xy))


def _extract_set(root):
    from spr_pick_amd import ctf, micrograph_io
    lines = ["image_name\tpath"]
    for k in range(2):
        path = os.path.join(root, "mic%d.mrc" % k)
        with open(path, "wb") as f:
            micrograph_io.write_mrc(f, np.zeros((96, 128), dtype=np.float32))
        lines.append("mic%d\t%s" % (k, path))
        open(os.path.join(root, "mic%d_scores.txt" % k), "w").write(
            "image_name\tx_coord\ty_coord\tscore\n" + "".join("mic%d\t%d\t%d\t%s\n" % (k, 40 + 9 * i, 41 + i, 0.5 + 0.1 * i)
                                                               for i in range(3)))
    open(os.path.join(root, "raw.txt"), "w").write("\n".join(lines) + "\n")
    star = os.path.join(root, "micrographs_ctf.star")
    open(star, "w").write(ctf.CTF_STAR_HEADER + ctf.star_row("mic0.mrc", 15005.0, 0.43, 1.06, 300.0, 2.7, 0.07)
                          + ctf.star_row("mic1.mrc", 8000.0, 0.2, 1.06, 300.0, 2.7, 0.07))
    return os.path.join(root, "raw.txt"), star


def test_extract_joins_the_ctf_columns(tmp_path, monkeypatch):
    from spr_pick_amd import ctf, export, extract
    _fake_extract(monkeypatch)
    dataset, star = _extract_set(str(tmp_path))
    plain = str(tmp_path / "plain")
    extract.extract_dataset(dataset, str(tmp_path), plain, 32, device="cpu")
    plain_bytes = open(os.path.join(plain, "particles.star"), "rb").read()
    rows = plain_bytes.decode()[len(export.PARTICLES_STAR_HEADER):].splitlines()
    assert plain_bytes.decode().startswith(export.PARTICLES_STAR_HEADER) and len(rows) == 6
    assert rows[0] == "40\t41\t000001@mic0.mrcs\tmic0.mrc\t0.5"      # today's row, nothing appended

    header = export.PARTICLES_STAR_HEADER + "".join("_rln%s #%d\n" % (c, 6 + k) for k, c in enumerate(ctf.CTF_STAR_COLUMNS[1:]))
    for kwargs, factor in ((dict(), 1.0), (dict(bin=2), 2.0), (dict(scale=20), 32 / 20)):
        out = str(tmp_path / ("o%g" % factor))
        extract.extract_dataset(dataset, str(tmp_path), out, 32, device="cpu", ctf=star, **kwargs)
        text = open(os.path.join(out, "particles.star")).read()
        assert text.startswith(header)
        got = text[len(header):].splitlines()
        assert len(got) == 6
        for k, (line, old) in enumerate(zip(got, rows)):
            dz = "15005.00" if k < 3 else "8000.00"
            fom = "0.430000" if k < 3 else "0.200000"
            assert line == old + "\t%s\t%s\t0.00\t300.00\t2.7000\t0.0700\t10000.00\t%.5f\t%s" % (dz, dz, 1.06 * factor, fom)

    # a micrograph with picks but no row in the table: refused by name before anything is extracted
    open(star, "w").write(ctf.CTF_STAR_HEADER + ctf.star_row("mic0.mrc", 15005.0, 0.43, 1.06, 300.0, 2.7, 0.07))
    calls = []
    monkeypatch.setattr(extract, "_extract_file", lambda *a: calls.append(a))
    with pytest.raises(ValueError, match="mic1"):
        extract.extract_dataset(dataset, str(tmp_path), str(tmp_path / "bad"), 32, device="cpu", ctf=star)
    assert not calls and not os.path.exists(str(tmp_path / "bad" / "particles.star"))
