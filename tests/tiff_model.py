"""The model of TIFF movie input (spr_pick_amd/tiffio.py, csrc/tiff.hip, include/sprk.h: sprk_tiff_decode), the
yardstick of tests/test_tiff_cpu.py and tests/test_gpu_tiff.py, in plain Python over ``bytes``.

* ``lzw_encode``: TIFF 6.0 LZW as libtiff writes it (MSB-first codes of 9..12 bits, early change, a Clear first and another
  when the table reaches 4094 entries, an EOI last), with the options to leave the EOI out and to emit Clears early.
* ``lzw_decode`` / ``decode``: the device contract, statuses and zero fill included.  The table holds the strings themselves,
  not positions in the output as the kernel and ``tiffio.lzw_decode`` do: the three are written independently.
* ``write_tiff``: a multi-page stripped TIFF, classic or BigTIFF, of the five sample formats, stored or LZW."""
import struct

import numpy as np

CLEAR, EOI, FIRST = 256, 257, 258
OK, BAD_CODE, SHORT, LONG = 0, 1, 2, 3


def width_of(nxt):
    """the code width while the decoder's next free code is ``nxt`` (the early change)"""
    return 9 if nxt < 511 else 10 if nxt < 1023 else 11 if nxt < 2047 else 12


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, width):
        self.acc = (self.acc << width) | code
        self.n += width
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1

    def done(self):
        if self.n:
            self.out.append((self.acc << (8 - self.n)) & 255)
            self.acc, self.n = 0, 0
        return bytes(self.out)


def lzw_encode(data, eoi=True, clear_every=None, table_limit=4094):
    """bytes -> one LZW strip.  ``clear_every``: a Clear after every that many codes as well (None: only when the table
    reaches ``table_limit`` entries); ``eoi``: end with the EOI code."""
    w = BitWriter()
    table, emitted = {}, 0                       # (prefix code, byte) -> code; codes out since the last Clear

    def dec_next():                              # the decoder's next free code once it has read what is out
        return FIRST + max(0, emitted - 1)

    w.put(CLEAR, 9)
    cur = None
    for b in data:
        if cur is None:
            cur = b
            continue
        hit = table.get((cur, b))
        if hit is not None:
            cur = hit
            continue
        w.put(cur, width_of(dec_next()))
        emitted += 1
        entry = FIRST + emitted - 1              # the entry the decoder makes when it reads the code after this one
        if entry >= table_limit or (clear_every and emitted >= clear_every):
            w.put(CLEAR, width_of(dec_next()))
            table, emitted = {}, 0
        elif entry < 4096:
            table[(cur, b)] = entry
        cur = b
    if cur is not None:
        w.put(cur, width_of(dec_next()))
        emitted += 1
    if eoi:
        w.put(EOI, width_of(dec_next()))
    return w.done()


def read_code(data, bitpos, width):
    v = 0
    for i in range(bitpos, bitpos + width):
        v = (v << 1) | ((data[i >> 3] >> (7 - (i & 7))) & 1)
    return v


def lzw_decode(data, out_len):
    """-> (out_len bytes, status): the contract of sprk_tiff_decode for one LZW strip"""
    out, strings, prev, width, nxt, bitpos = bytearray(), {}, None, 9, FIRST, 0
    status = OK
    while len(out) < out_len:
        if bitpos + width > 8 * len(data):
            status = SHORT
            break
        code = read_code(data, bitpos, width)
        bitpos += width
        if code == CLEAR:
            strings, prev, width, nxt = {}, None, 9, FIRST
            continue
        if code == EOI:
            status = SHORT
            break
        if prev is None:
            if code > 255:
                status = BAD_CODE
                break
            s = bytes([code])
        elif code < 256:
            s = bytes([code])
        elif code < nxt:
            s = strings[code]
        elif code == nxt:
            s = prev + prev[:1]
        else:
            status = BAD_CODE
            break
        if len(out) + len(s) > out_len:
            out += s[:out_len - len(out)]
            status = LONG
            break
        out += s
        if prev is not None and nxt < 4096:
            strings[nxt] = prev + s[:1]
            nxt += 1
            width = width_of(nxt)
        prev = s
    return bytes(out) + bytes(out_len - len(out)), status


def decode(src, strip_off, strip_len, strip_out, compression, widen, out_elems=None):
    """The whole launch: -> (out as uint8 (uint16 with widen) [sum of strip_out], status int32 [n_strips]); positions past
    ``out_elems`` (default: the sum) are not part of the output, and every value is clamped as the contract states."""
    src = bytes(src)
    total = sum(min(max(int(v), 0), 1 << 62) for v in strip_out)
    cap = total if out_elems is None else out_elems
    out, status, base = bytearray(cap), [], 0
    for off, length, so in zip(strip_off, strip_len, strip_out):
        off, length = int(off), int(length)
        so = min(max(int(so), 0), cap)
        base = min(base, cap)
        so_c = min(so, cap - base, 2 ** 31 - 1)
        lo = min(max(off, 0), len(src))
        hi = lo if length <= 0 else max(min(off + length, len(src)), lo)
        data = src[lo:hi]
        if compression == 1:
            got = data[:so_c]
            piece, st = got + bytes(so_c - len(got)), (OK if len(got) == so_c else SHORT)
        else:
            piece, st = lzw_decode(data, so_c)
        out[base:base + so_c] = piece
        status.append(st)
        base += so
    arr = np.frombuffer(bytes(out), dtype=np.uint8)
    return (arr.astype("<u2") if widen else arr), np.array(status, dtype=np.int32)


# ---- the container ---------------------------------------------------------------------------------------------------------
FORMATS = {np.dtype("u1"): (1, 8), np.dtype("i1"): (2, 8), np.dtype("<u2"): (1, 16), np.dtype("<i2"): (2, 16),
           np.dtype("<f4"): (3, 32)}
MODE_OF_TIFF = {np.dtype("u1"): 6, np.dtype("i1"): 0, np.dtype("<u2"): 6, np.dtype("<i2"): 1, np.dtype("<f4"): 2}


def write_tiff(path, movie, rows_per_strip, lzw=True, big=False, apix=None, extra_tags=(), encode=None, pad_first=1,
               compression=None):
    """movie [Z, ny, nx] of one of the five sample types -> a multi-page TIFF, one IFD per frame, strips of
    ``rows_per_strip`` rows written back to back (``pad_first`` bytes after the header, so that strips start at odd
    offsets).  apix: XResolution / YResolution in pixels per centimetre.  extra_tags: (tag, type, values) per IFD, after
    the standard ones (a repeated tag replaces the standard one).  encode: the strip encoder (default ``lzw_encode``).
    compression: the value of the Compression tag, when it shall differ from what the strips hold.
    -> per frame, the list of (offset, length) of its strips."""
    movie = np.ascontiguousarray(movie)
    Z, ny, nx = movie.shape
    fmt, bits = FORMATS[movie.dtype]
    encode = encode or lzw_encode
    blob = bytearray(b"II+\x00\x08\x00\x00\x00" + bytes(8) if big else b"II*\x00" + bytes(4))
    blob += bytes(pad_first)
    tables = []
    for k in range(Z):
        strips = []
        for r in range(0, ny, rows_per_strip):
            raw = movie[k, r:r + rows_per_strip].tobytes()
            data = encode(raw) if lzw else raw
            strips.append((len(blob), len(data)))
            blob += data
        tables.append(strips)
    link = 8 if big else 4                       # where the offset of the next IFD goes
    T = dict(SHORT=3, LONG=4, RATIONAL=5, LONG8=16)
    for k in range(Z):
        offs, lens = [s[0] for s in tables[k]], [s[1] for s in tables[k]]
        wide = T["LONG8"] if big else T["LONG"]
        tags = {256: (T["LONG"], [nx]), 257: (T["LONG"], [ny]), 258: (T["SHORT"], [bits]),
                259: (T["SHORT"], [compression if compression is not None else (5 if lzw else 1)]),
                262: (T["SHORT"], [1]), 273: (wide, offs), 277: (T["SHORT"], [1]), 278: (T["LONG"], [rows_per_strip]),
                279: (wide, lens), 339: (T["SHORT"], [fmt])}
        if apix is not None:
            num = int(round(1.0e8 / apix * 10))
            tags.update({282: (T["RATIONAL"], [num, 10]), 283: (T["RATIONAL"], [num, 10]), 296: (T["SHORT"], [3])})
        for tag, typ, vals in extra_tags:
            if typ is None:
                tags.pop(tag, None)
            else:
                tags[tag] = (typ, list(vals))
        while len(blob) % 8:
            blob.append(0)
        entries = []
        for tag in sorted(tags):
            typ, vals = tags[tag]
            code = {3: "H", 4: "I", 5: "I", 16: "Q"}[typ]
            count = len(vals) // 2 if typ == 5 else len(vals)
            payload = struct.pack("<%d%s" % (len(vals), code), *vals)
            inline = 8 if big else 4
            if len(payload) > inline:
                while len(blob) % 2:
                    blob.append(0)
                at = len(blob)
                blob += payload
                payload = struct.pack("<Q" if big else "<I", at)
            entries.append(struct.pack("<HHQ" if big else "<HHI", tag, typ, count) + payload.ljust(inline, b"\0"))
        while len(blob) % 8:
            blob.append(0)
        at = len(blob)
        blob[link:link + (8 if big else 4)] = struct.pack("<Q" if big else "<I", at)
        blob += struct.pack("<Q" if big else "<H", len(entries)) + b"".join(entries)
        link = len(blob)
        blob += bytes(8 if big else 4)
    with open(path, "wb") as f:
        f.write(bytes(blob))
    return tables
