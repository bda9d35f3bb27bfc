"""TIFF movies for ``joint align``: the container read on the host, the strips decoded on the device.

SerialEM and EPU write K2 / K3 / Falcon movies as multi-page TIFF, one IFD per frame, in strips, LZW-compressed: counting-mode
frames of 0 / 1 / 2 counts shrink 5 to 10 times.  ``read_tiff_movie`` reads the IFDs only, pure Python and NumPy, and returns
where every strip of every frame lies; ``align.TiffMovie`` uploads a frame's strips as they are and ``torch.ops.sprk.tiff_decode``
(csrc/tiff.hip) turns them into the sample block every other kernel takes.

Accepted: little-endian classic TIFF and BigTIFF, stripped, one sample per pixel, stored or LZW, no predictor; uint8, int8,
uint16, int16 and float32 samples.  uint8 becomes the project's mode 6 (uint16): mode 0 is int8 and cannot hold 0..255, and
the device widens every byte as it decodes.  Row r of the TIFF is row r of the frame as stored.  IMOD shows TIFF flipped in Y
against MRC, so a gain reference that IMOD converted to MRC needs ``--gain_flip ud``.

Everything else is refused before any launch, with a ValueError that names the file, the tag and what to do.

``lzw_decode`` is the host form of the device contract (include/sprk.h: sprk_tiff_decode); ``align.TiffMovie`` uses it once per
movie, on the first strip of frame 0, for the anchor.  This module imports neither torch nor the library."""
import struct
from collections import namedtuple

import numpy as np

MAX_SIDE = 16384                                 # ingest.MAX_SIDE (tests/test_tiff_cpu.py holds them together)
STORED, LZW = 1, 5
COMPRESSIONS = {1: "stored", 2: "CCITT RLE", 3: "CCITT Group 3", 4: "CCITT Group 4", 5: "LZW", 6: "old JPEG", 7: "JPEG",
                8: "Deflate", 32773: "PackBits", 32946: "Deflate", 34712: "JPEG 2000", 34925: "LZMA", 50000: "ZSTD",
                50001: "WebP"}
# (SampleFormat, BitsPerSample) -> (the project's mode, the dtype of the decoded samples, widen)
SAMPLES = {(1, 8): (6, np.dtype("<u2"), True), (2, 8): (0, np.dtype("i1"), False), (1, 16): (6, np.dtype("<u2"), False),
           (2, 16): (1, np.dtype("<i2"), False), (3, 32): (2, np.dtype("<f4"), False)}
ANGSTROM_PER_UNIT = {2: 2.54e8, 3: 1.0e8}        # ResolutionUnit: inch, centimetre

_TYPES = {1: "B", 2: "c", 3: "H", 4: "I", 5: "II", 6: "b", 7: "B", 8: "h", 9: "i", 10: "ii", 11: "f", 12: "d", 13: "I",
          16: "Q", 17: "q", 18: "Q"}
_NAMES = {256: "ImageWidth", 257: "ImageLength", 258: "BitsPerSample", 259: "Compression", 266: "FillOrder",
          273: "StripOffsets", 277: "SamplesPerPixel", 278: "RowsPerStrip", 279: "StripByteCounts", 282: "XResolution",
          296: "ResolutionUnit", 317: "Predictor", 322: "TileWidth", 323: "TileLength", 324: "TileOffsets",
          325: "TileByteCounts", 339: "SampleFormat"}

TiffMovie = namedtuple("TiffMovie", "ny nx frames mode dtype widen compression rows_per_strip strip_offsets strip_lengths "
                                    "strip_rows apix bigtiff")
TiffMovie.__doc__ = """ny, nx, frames; mode: the project's sample mode (0 / 1 / 2 / 6) and dtype: the decoded samples';
widen: the file's samples are uint8 and every byte becomes a uint16; compression: 1 or 5; rows_per_strip; strip_offsets,
strip_lengths: per frame, int64 arrays [n_strips] of file offsets and byte counts; strip_rows: int64 [n_strips], the rows of
each strip (the same for every frame); apix: Angstrom per pixel from XResolution / ResolutionUnit, or None; bigtiff."""


def compression_name(c):
    return "%s (%d)" % (COMPRESSIONS.get(c, "unknown"), c)


def _read_at(f, offset, n, path, what):
    f.seek(offset)
    b = f.read(n)
    if len(b) != n:
        raise ValueError("%s: %s at byte %d runs past the end of the file; the file is truncated: copy it again"
                         % (path, what, offset))
    return b


def _read_ifd(f, offset, big, size, path, k):
    """-> ({tag: tuple of values}, offset of the next IFD)"""
    what = "the directory of frame %d" % k
    if offset < 8 or offset >= size:
        raise ValueError("%s: %s lies at byte %d, outside the file of %d bytes; the file is truncated or no TIFF: copy it "
                         "again" % (path, what, offset, size))
    cnt_fmt, ent_fmt, ent_size, inline = ("<Q", "<HHQ8s", 20, 8) if big else ("<H", "<HHI4s", 12, 4)
    n, = struct.unpack(cnt_fmt, _read_at(f, offset, struct.calcsize(cnt_fmt), path, what))
    if n > 4096:
        raise ValueError("%s: %s counts %d entries; this is no TIFF directory: copy the file again" % (path, what, n))
    body = _read_at(f, offset + struct.calcsize(cnt_fmt), n * ent_size + inline, path, what)
    tags = {}
    for i in range(n):
        tag, typ, count, value = struct.unpack_from(ent_fmt, body, i * ent_size)
        if tag not in _NAMES:
            continue                             # no tag of the others changes where the samples lie
        if typ not in _TYPES or typ == 2:
            raise ValueError("%s: frame %d: tag %s has the field type %d, which is not a number; write the movie with "
                             "SerialEM, EPU, IMOD or libtiff" % (path, k, _NAMES[tag], typ))
        fmt = "<" + _TYPES[typ] * count
        nbytes = struct.calcsize(fmt)
        if nbytes > inline:
            at, = struct.unpack("<Q" if big else "<I", value)
            if at + nbytes > size:
                raise ValueError("%s: frame %d: the values of tag %s (%d bytes at %d) lie outside the file of %d bytes; the "
                                 "file is truncated: copy it again" % (path, k, _NAMES[tag], nbytes, at, size))
            value = _read_at(f, at, nbytes, path, "tag %s of frame %d" % (_NAMES[tag], k))
        vals = struct.unpack_from(fmt, value)
        tags[tag] = tuple(vals[0::2][j] / vals[1::2][j] if vals[1::2][j] else 0.0 for j in range(count)) if typ in (5, 10) \
            else vals
    nxt, = struct.unpack("<Q" if big else "<I", body[n * ent_size:])
    return tags, nxt


def _one(tags, tag, default, path, k):
    v = tags.get(tag)
    if v is None:
        if default is None:
            raise ValueError("%s: frame %d has no %s tag; it is needed: write the movie with SerialEM, EPU, IMOD or libtiff"
                             % (path, k, _NAMES[tag]))
        return default
    if len(set(v)) != 1:
        raise ValueError("%s: frame %d: tag %s holds different values %s; one sample per pixel is read: convert the movie"
                         % (path, k, _NAMES[tag], v[:4]))
    return v[0]


def _frame(tags, path, k, size):
    """the checked facts of one IFD -> (ny, nx, (format, bits), compression, rows per strip, offsets, lengths)"""
    if 322 in tags or 323 in tags or 324 in tags or 325 in tags:
        raise ValueError("%s: frame %d is tiled (tag %s); only stripped TIFF is read: rewrite the movie in strips (IMOD: "
                         "newstack; libtiff: tiffcp -s)" % (path, k, _NAMES[min(t for t in (322, 323, 324, 325) if t in tags)]))
    nx, ny = _one(tags, 256, None, path, k), _one(tags, 257, None, path, k)
    spp = _one(tags, 277, 1, path, k)
    if spp != 1:
        raise ValueError("%s: frame %d: SamplesPerPixel is %d; movie frames have 1: convert the movie to grey values"
                         % (path, k, spp))
    bits, fmt = _one(tags, 258, 1, path, k), _one(tags, 339, 1, path, k)
    if bits == 4:
        raise ValueError("%s: frame %d: BitsPerSample is 4 (packed samples); they are not read: unpack the movie to 8 bits "
                         "(IMOD: newstack -mode 0, or clip unpack)" % (path, k))
    if (fmt, bits) not in SAMPLES:
        raise ValueError("%s: frame %d: SampleFormat %d with BitsPerSample %d; read are uint8, int8, uint16, int16 and "
                         "float32: convert the movie" % (path, k, fmt, bits))
    comp = _one(tags, 259, 1, path, k)
    if comp not in (STORED, LZW):
        raise ValueError("%s: frame %d: Compression is %s; read are stored (1) and LZW (5): rewrite the movie (IMOD: newstack; "
                         "libtiff: tiffcp -c lzw)" % (path, k, compression_name(comp)))
    pred = _one(tags, 317, 1, path, k)
    if pred != 1:
        raise ValueError("%s: frame %d: Predictor is %d (%s differencing); only Predictor 1 (none) is read: rewrite the movie "
                         "without a predictor (libtiff: tiffcp -c lzw:1)"
                         % (path, k, pred, {2: "horizontal", 3: "floating-point"}.get(pred, "unknown")))
    fill = _one(tags, 266, 1, path, k)
    if fill != 1:
        raise ValueError("%s: frame %d: FillOrder is %d; only FillOrder 1 (most significant bit first) is read: rewrite the "
                         "movie (libtiff: tiffcp -M)" % (path, k, fill))
    if not (1 <= ny <= MAX_SIDE and 1 <= nx <= MAX_SIDE):
        raise ValueError("%s: frame %d: ImageLength x ImageWidth is %dx%d; joint align takes sides of 1..%d: bin the movie"
                         % (path, k, ny, nx, MAX_SIDE))
    rows = min(_one(tags, 278, 2 ** 32 - 1, path, k), ny)
    if rows < 1:
        raise ValueError("%s: frame %d: RowsPerStrip is 0; rewrite the movie" % (path, k))
    if 273 not in tags or 279 not in tags:
        raise ValueError("%s: frame %d has no %s tag; only stripped TIFF is read: rewrite the movie in strips"
                         % (path, k, _NAMES[273 if 273 not in tags else 279]))
    off, length = np.array(tags[273], dtype=np.int64), np.array(tags[279], dtype=np.int64)
    want = -(-ny // rows)
    if len(off) != want or len(length) != want:
        raise ValueError("%s: frame %d: StripOffsets has %d and StripByteCounts %d entries, %d rows in strips of %d "
                         "(RowsPerStrip) need %d: the file is damaged, write it again"
                         % (path, k, len(off), len(length), ny, rows, want))
    bad = np.nonzero((off < 8) | (length < 0) | (off + length > size))[0]
    if len(bad):
        s = int(bad[0])
        raise ValueError("%s: frame %d: strip %d (StripOffsets %d, StripByteCounts %d) points outside the file of %d bytes: "
                         "the file is truncated, copy it again" % (path, k, s, off[s], length[s], size))
    return ny, nx, (fmt, bits), comp, rows, off, length


def read_tiff_movie(path, f):
    """The IFDs of an open TIFF movie -> ``TiffMovie``.  No sample is read."""
    f.seek(0, 2)
    size = f.tell()
    head = _read_at(f, 0, 16 if size >= 16 else 8, path, "the TIFF header") if size >= 8 else b""
    if head[:4] in (b"MM\x00*", b"MM\x00+"):
        raise ValueError("%s: a big-endian TIFF (byte order MM); only little-endian files (II) are read: rewrite it (libtiff: "
                         "tiffcp -L)" % path)
    if head[:4] == b"II*\x00":
        big, first = False, struct.unpack("<I", head[4:8])[0]
    elif head[:4] == b"II+\x00" and len(head) == 16 and struct.unpack("<HH", head[4:8]) == (8, 0):
        big, first = True, struct.unpack("<Q", head[8:16])[0]
    else:
        raise ValueError("%s: no TIFF header (II*\\0 or II+\\0 in the first four bytes); is this a TIFF movie?" % path)
    offsets, lengths, facts, apix, seen, at = [], [], None, None, set(), first
    while at:
        if at in seen:
            raise ValueError("%s: the directories form a loop at byte %d: the file is damaged, write it again" % (path, at))
        seen.add(at)
        k = len(offsets)
        tags, at = _read_ifd(f, at, big, size, path, k)
        ny, nx, sample, comp, rows, off, length = _frame(tags, path, k, size)
        if facts is None:
            facts = (ny, nx, sample, comp, rows)
            unit, xres = _one(tags, 296, 2, path, k), tags.get(282, (0.0,))[0]
            if unit in ANGSTROM_PER_UNIT and np.isfinite(xres) and xres > 0:
                apix = ANGSTROM_PER_UNIT[unit] / float(xres)
        elif (ny, nx, sample, comp, rows) != facts:
            raise ValueError("%s: frame %d is %dx%d, SampleFormat/BitsPerSample %s, Compression %d, RowsPerStrip %d; frame 0 is "
                             "%dx%d, %s, %d, %d: every frame of a movie must be like frame 0: write the movie again"
                             % ((path, k, ny, nx, sample, comp, rows) + facts))
        offsets.append(off)
        lengths.append(length)
    if len(offsets) < 2:
        raise ValueError("%s: expected a movie, at least 2 frames (one directory each), got %d" % (path, len(offsets)))
    ny, nx, sample, comp, rows = facts
    mode, dtype, widen = SAMPLES[sample]
    n = -(-ny // rows)
    strip_rows = np.full(n, rows, dtype=np.int64)
    strip_rows[-1] = ny - rows * (n - 1)
    return TiffMovie(ny, nx, len(offsets), mode, dtype, widen, comp, rows, offsets, lengths, strip_rows, apix, big)


def strip_bytes(movie):
    """-> int64 [n_strips]: the bytes each strip decodes to in the file's own samples (before a uint8 is widened)"""
    return movie.strip_rows * movie.nx * (1 if movie.widen else movie.dtype.itemsize)


# ---- the decoder on the host ---------------------------------------------------------------------------------------------
def lzw_decode(data, out_len):
    """One LZW strip by the contract of sprk_tiff_decode -> (``out_len`` bytes, status 0 / 1 / 2 / 3).  The table holds
    (start, length) in the output, as the kernel's does."""
    out = bytearray(out_len)
    total = len(data) * 8
    bitpos, n, width, nxt, prev = 0, 0, 9, 258, None
    pos, length = [0] * 4096, [0] * 4096
    while n < out_len:
        if bitpos + width > total:
            return bytes(out), 2
        byte = bitpos >> 3
        code = (int.from_bytes(data[byte:byte + 3].ljust(3, b"\0"), "big") >> (24 - width - (bitpos & 7))) & ((1 << width) - 1)
        bitpos += width
        if code == 256:
            width, nxt, prev = 9, 258, None
            continue
        if code == 257:
            return bytes(out), 2
        if prev is None:
            if code > 255:
                return bytes(out), 1
            s = bytes([code])
        elif code < 256:
            s = bytes([code])
        elif code < nxt:
            s = bytes(out[pos[code]:pos[code] + length[code]])
        elif code == nxt:
            s = bytes(out[prev[0]:prev[0] + prev[1]]) + bytes(out[prev[0]:prev[0] + 1])
        else:
            return bytes(out), 1
        if n + len(s) > out_len:
            out[n:] = s[:out_len - n]
            return bytes(out), 3
        out[n:n + len(s)] = s
        if prev is not None and nxt < 4096:
            pos[nxt], length[nxt] = prev[0], prev[1] + 1
            nxt += 1
            if nxt in (511, 1023, 2047):
                width += 1
        prev = (n, len(s))
        n += len(s)
    return bytes(out), 0


def decode_strip(data, out_len, compression):
    """-> (out_len bytes, status): ``lzw_decode``, or the copy of a stored strip"""
    if compression == LZW:
        return lzw_decode(bytes(data), out_len)
    data = bytes(data[:out_len])
    return data + bytes(out_len - len(data)), (0 if len(data) == out_len else 2)


def first_sample(movie, f):
    """The first sample of frame 0, from the head of its first strip decoded on the host (a few bytes are asked for)."""
    size = 1 if movie.widen else movie.dtype.itemsize
    f.seek(int(movie.strip_offsets[0][0]))
    data = f.read(min(int(movie.strip_lengths[0][0]), 4096))
    out, _ = decode_strip(data, size, movie.compression)
    return float(np.frombuffer(out, dtype=np.uint8 if movie.widen else movie.dtype)[0])
