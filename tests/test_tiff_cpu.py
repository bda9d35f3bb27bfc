"""CPU: TIFF movie input (spr_pick_amd/tiffio.py, tests/tiff_model.py): the model's decoder undoes its encoder
in every sample format and strip layout; what PIL (libtiff) writes decodes through ``tiffio`` and the model to what PIL reads
back; every refusal of the container reader, with its message; classic and BigTIFF parse alike; and nothing of it needs
torch."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tiff_model
from conftest import ROOT
from spr_pick_amd import tiffio

DTYPES = [np.dtype(d) for d in ("u1", "i1", "<u2", "<i2", "<f4")]
NY, NX, Z = 13, 40, 2


def counts(dtype, shape, seed):
    rng = np.random.RandomState(seed)
    if dtype.kind == "f":
        return rng.poisson(1.0, size=shape).astype(dtype) * np.float32(0.37)
    a = rng.poisson(1.0, size=shape)
    if dtype.kind == "i":
        a = a - 1
    a = a.astype(dtype)
    info = np.iinfo(dtype)
    a.flat[0], a.flat[-1] = info.max, info.min
    return a


def decode_file(path):
    """``tiffio`` for the container, the model for the strips -> [Z, ny, nx] in the file's own sample type"""
    with open(path, "rb") as f:
        t = tiffio.read_tiff_movie(path, f)
        content = f.seek(0) or f.read()
    sizes = tiffio.strip_bytes(t)
    frames = []
    for off, length in zip(t.strip_offsets, t.strip_lengths):
        out, status = tiff_model.decode(content, off, length, sizes, t.compression, False)
        assert not status.any(), status
        frames.append(out.tobytes())
    dtype = np.dtype("u1") if t.widen else t.dtype
    return np.frombuffer(b"".join(frames), dtype=dtype).reshape(t.frames, t.ny, t.nx), t


@pytest.mark.parametrize("dtype", DTYPES, ids=[d.name for d in DTYPES])
@pytest.mark.parametrize("rows", [1, 3, 8, NY])
@pytest.mark.parametrize("lzw", [True, False], ids=["lzw", "stored"])
def test_the_model_decoder_undoes_the_model_encoder(dtype, rows, lzw, tmp_path):
    movie = counts(dtype, (Z, NY, NX), 7 + rows)
    path = str(tmp_path / "m.tif")
    tables = tiff_model.write_tiff(path, movie, rows, lzw=lzw, big=(rows == 3))
    got, t = decode_file(path)
    assert got.dtype == movie.dtype and np.array_equal(got.view(np.uint8), movie.view(np.uint8))
    assert (t.ny, t.nx, t.frames, t.rows_per_strip) == (NY, NX, Z, rows) and t.bigtiff == (rows == 3)
    assert t.mode == tiff_model.MODE_OF_TIFF[dtype] and t.widen == (dtype == np.dtype("u1"))
    assert t.compression == (5 if lzw else 1) and t.apix is None
    assert list(t.strip_rows) == [min(rows, NY - r) for r in range(0, NY, rows)]       # NY % rows != 0 for 3 and 8
    assert [list(zip(o, n)) for o, n in zip(t.strip_offsets, t.strip_lengths)] == tables
    assert any(o % 2 for o in t.strip_offsets[0])                               # strips at odd file offsets
    # the product's own host decoder agrees with the model
    with open(path, "rb") as f:
        content = f.read()
    for (o, n), size in zip(tables[1], tiffio.strip_bytes(t)):
        assert tiffio.decode_strip(content[o:o + n], int(size), t.compression) == \
            (tiff_model.lzw_decode(content[o:o + n], int(size)) if lzw else (content[o:o + n], 0))


def test_the_encoder_reaches_every_width_and_clears_a_full_table():
    rng = np.random.RandomState(3)
    data = rng.randint(0, 256, size=12000).astype(np.uint8).tobytes()
    enc = tiff_model.lzw_encode(data)
    # the codes of the stream, read back with the decoder's own widths
    widths, clears, bitpos, nxt, prev = set(), 0, 0, 258, False
    while True:
        w = tiff_model.width_of(nxt)
        code = tiff_model.read_code(enc, bitpos, w)
        bitpos += w
        widths.add(w)
        if code == 257:
            break
        if code == 256:
            clears, nxt, prev = clears + 1, 258, False
            continue
        nxt, prev = nxt + (1 if prev and nxt < 4096 else 0), True
    assert widths == {9, 10, 11, 12} and clears >= 2
    assert tiff_model.lzw_decode(enc, len(data)) == (data, 0) and tiffio.lzw_decode(enc, len(data)) == (data, 0)
    for options in (dict(eoi=False), dict(clear_every=100), dict(clear_every=1)):
        e = tiff_model.lzw_encode(data[:3000], **options)
        assert tiff_model.lzw_decode(e, 3000) == (data[:3000], 0) and tiffio.lzw_decode(e, 3000) == (data[:3000], 0)


def test_the_statuses_and_the_zero_fill():
    data = bytes(range(200)) * 3
    enc = tiff_model.lzw_encode(data)
    for decode in (tiff_model.lzw_decode, tiffio.lzw_decode):
        out, st = decode(enc[:100], len(data))                                  # the input runs out
        assert st == 2 and out[:60] == data[:60] and not any(out[-300:]) and len(out) == len(data)
        assert decode(enc, len(data) + 1) == (data + b"\0", 2)                  # EOI before the bytes are out
        out, st = decode(enc, 500)                                              # a string past the end: cut
        assert st in (0, 3) and out == data[:500]
        assert decode(enc, 201) == (data[:201], 3)                              # the code for (0, 1) is cut after its first byte
        w = tiff_model.BitWriter()
        for code, width in ((256, 9), (65, 9), (66, 9), (300, 9)):               # 300 > next free (259)
            w.put(code, width)
        assert decode(w.done(), 10) == (b"AB" + bytes(8), 1)
        w = tiff_model.BitWriter()
        for code, width in ((256, 9), (258, 9)):                                 # no literal after a Clear
            w.put(code, width)
        assert decode(w.done(), 4) == (bytes(4), 1)
        w = tiff_model.BitWriter()
        for code, width in ((65, 9), (258, 9), (259, 9)):                        # no Clear first; code == next free twice
            w.put(code, width)
        assert decode(w.done(), 6) == (b"AAAAAA", 0)
        assert decode(b"", 3) == (bytes(3), 2) and decode(b"", 0) == (b"", 0)


PIL_CASES = [("u1", "L"), ("<u2", "I;16")]


@pytest.mark.parametrize("dtype,pil_mode", PIL_CASES, ids=["uint8", "uint16"])
def test_what_libtiff_writes_decodes_to_what_it_reads_back(dtype, pil_mode, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from PIL import features
    if not features.check("libtiff"):
        pytest.skip("this PIL has no libtiff, and its own writer knows no LZW")
    rng = np.random.RandomState(11)
    ny, nx = 70, 300
    # counts, with a stretch of noise in frame 1 that takes libtiff's table through its widths to the Clear
    movie = rng.poisson(1.0, size=(3, ny, nx)).astype(dtype)
    movie[1, 10:60] = rng.randint(0, 256 if dtype == "u1" else 65536, size=(50, nx))
    path = str(tmp_path / "pil.tif")
    pages = [Image.fromarray(f) for f in movie]
    pages[0].save(path, save_all=True, append_images=pages[1:], compression="tiff_lzw")
    back = []
    with Image.open(path) as im:
        assert im.n_frames == 3
        for k in range(3):
            im.seek(k)
            back.append(np.array(im))
    back = np.stack(back)
    assert np.array_equal(back, movie)
    got, t = decode_file(path)
    assert t.compression == 5 and (t.frames, t.ny, t.nx) == (3, ny, nx) and t.mode == 6
    assert got.dtype == np.dtype(dtype) and np.array_equal(got, back)
    print("libtiff wrote %d strip(s) a frame, %d rows each; %d -> %d bytes" % (
        len(t.strip_rows), t.rows_per_strip, movie.nbytes, int(sum(n.sum() for n in t.strip_lengths))))


def test_classic_and_bigtiff_parse_to_the_same_description(tmp_path):
    movie = counts(np.dtype("<i2"), (3, NY, NX), 5)
    a, b = str(tmp_path / "a.tif"), str(tmp_path / "b.tif")
    tiff_model.write_tiff(a, movie, 4, apix=1.25)
    tiff_model.write_tiff(b, movie, 4, apix=1.25, big=True)
    with open(a, "rb") as fa, open(b, "rb") as fb:
        ta, tb = tiffio.read_tiff_movie(a, fa), tiffio.read_tiff_movie(b, fb)
        ca, cb = fa.seek(0) or fa.read(), fb.seek(0) or fb.read()
    assert not ta.bigtiff and tb.bigtiff
    for name in ("ny", "nx", "frames", "mode", "dtype", "widen", "compression", "rows_per_strip", "apix"):
        assert getattr(ta, name) == getattr(tb, name), name
    assert abs(ta.apix - 1.25) < 1e-6 and np.array_equal(ta.strip_rows, tb.strip_rows)
    for k in range(3):
        assert np.array_equal(ta.strip_lengths[k], tb.strip_lengths[k])
        for s in range(len(ta.strip_rows)):
            assert ca[ta.strip_offsets[k][s]:][:ta.strip_lengths[k][s]] == cb[tb.strip_offsets[k][s]:][:tb.strip_lengths[k][s]]
    # a resolution without a unit of length states no pixel size
    tiff_model.write_tiff(a, movie, 4, apix=1.25, extra_tags=[(296, 3, [1])])
    with open(a, "rb") as f:
        assert tiffio.read_tiff_movie(a, f).apix is None


def refused(tmp_path, match, movie=None, patch=None, **kw):
    movie = counts(np.dtype("<u2"), (2, NY, NX), 1) if movie is None else movie
    path = str(tmp_path / "bad.tif")
    kw.setdefault("rows_per_strip", 4)
    tiff_model.write_tiff(path, movie, **kw)
    if patch:
        with open(path, "r+b") as f:
            patch(f)
    with open(path, "rb") as f, pytest.raises(ValueError, match=match) as e:
        tiffio.read_tiff_movie(path, f)
    assert path in str(e.value)
    return str(e.value)


def test_every_refusal_names_the_file_the_tag_and_what_to_do(tmp_path):
    S, L = 3, 4
    refused(tmp_path, r"big-endian TIFF.*tiffcp -L", patch=lambda f: f.write(b"MM\x00*"))
    refused(tmp_path, r"no TIFF header", patch=lambda f: f.write(b"\x89PNG"))
    refused(tmp_path, r"tiled \(tag TileWidth\).*strips", extra_tags=[(322, L, [16]), (323, L, [16])])
    refused(tmp_path, r"BitsPerSample is 4 \(packed samples\).*unpack", extra_tags=[(258, S, [4])])
    refused(tmp_path, r"Predictor is 2 \(horizontal differencing\).*without a predictor", extra_tags=[(317, S, [2])])
    refused(tmp_path, r"Predictor is 3 \(floating-point differencing\)", extra_tags=[(317, S, [3])])
    refused(tmp_path, r"Compression is ZSTD \(50000\).*rewrite", compression=50000)
    refused(tmp_path, r"Compression is Deflate \(8\)", compression=8)
    refused(tmp_path, r"Compression is JPEG \(7\)", compression=7)
    refused(tmp_path, r"FillOrder is 2", extra_tags=[(266, S, [2])])
    refused(tmp_path, r"SamplesPerPixel is 3", extra_tags=[(277, S, [3])])
    refused(tmp_path, r"SampleFormat 3 with BitsPerSample 16", extra_tags=[(339, S, [3])])
    refused(tmp_path, r"at least 2 frames.*got 1", movie=counts(np.dtype("u1"), (1, NY, NX), 2))
    assert tiffio.MAX_SIDE == 16384
    refused(tmp_path, r"ImageLength x ImageWidth is 13x16385.*1\.\.16384", extra_tags=[(256, L, [tiffio.MAX_SIDE + 1])])
    refused(tmp_path, r"strip 1 \(StripOffsets \d+, StripByteCounts 1000000\) points outside the file",
            extra_tags=[(279, L, [5, 1000000, 5, 5])])
    refused(tmp_path, r"StripOffsets has 4 and StripByteCounts 4 entries, 13 rows in strips of 5 \(RowsPerStrip\) need 3",
            extra_tags=[(278, L, [5])])
    refused(tmp_path, r"has no StripOffsets tag", extra_tags=[(273, None, None)])

    def second_frame_differs(f):                 # frame 1 of a movie that says uint16 turns int16
        content = f.seek(0) or f.read()
        at = content.rfind(b"\x53\x01\x03\x00\x01\x00\x00\x00\x01\x00")       # tag 339, SHORT, count 1, value 1
        f.seek(at + 8)
        f.write(b"\x02")
    refused(tmp_path, r"frame 1 is 13x40, SampleFormat/BitsPerSample \(2, 16\).*every frame of a movie must be like frame 0",
            patch=second_frame_differs)

    def cut(f):
        f.truncate(os.path.getsize(f.name) - 40)
    refused(tmp_path, r"(runs past the end|outside the file)", patch=cut)


def test_max_side_is_ingests_and_the_module_needs_no_torch():
    # the package's __init__ imports torch; the module itself, loaded from its file, reads and checks a movie without it
    code = ("import importlib.util, sys; spec = importlib.util.spec_from_file_location('tiffio', %r); "
            "m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m); "
            "assert m.lzw_decode(bytes([0x80, 0x10, 0x40]), 1) == (b'A', 0); "
            "assert 'torch' not in sys.modules" % os.path.join(ROOT, "spr_pick_amd", "tiffio.py"))
    subprocess.run([sys.executable, "-c", code], check=True)
    from spr_pick_amd import ingest, torch_ops
    assert tiffio.MAX_SIDE == ingest.MAX_SIDE
    assert "tiff_decode" in torch_ops.registered()
