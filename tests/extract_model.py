"""NumPy model of the particle-extraction contract (csrc/extract.hip, include/sprk.h), the oracle of
tests/test_extract_cpu.py and tests/test_gpu_extract.py — the reference project has no extraction step.

Particle p of centre (x, y) covers raw rows y0 .. y0+B-1 and columns x0 .. x0+B-1, x0 = x - B//2, y0 = y - B//2; output
pixel (i, j) of its [b, b] image (b = B // N) is the N x N block at (y0 + iN, x0 + jN).  Block value v: integer modes
the exact sum; float32 float32 adds from 0 in row-major order within the block.  A box not entirely inside the image:
status 1, zeros.  Not normalised: float32(v) / float32(N*N).  Normalised: background = {(i - b//2)^2 + (j - b//2)^2 >
R^2}, n pixels (n == 0: status 2, zeros);
  integer modes: d = v - v[0, 0], S1 = sum_bg d and S2 = sum_bg d^2 as Python ints, mean = float(S1) / float(n),
      var = float(S2) / float(n) - mean*mean (two roundings), status 2 and zeros unless var > 0,
      out = float32((float64(d) - mean) / sqrt(var));
  float32: mean = sum_bg v / n, var = sum_bg (v - mean)^2 / n in float64 (NumPy's summation order), same rule,
      out = float32((float64(v) - mean) / sqrt(var));
negated with ``invert``."""
import io
import struct

import numpy as np

DTYPES = {0: np.int8, 1: np.int16, 2: np.float32, 6: np.uint16}
MODE_OF = {np.dtype(v): k for k, v in DTYPES.items()}
OK, OUTSIDE, FLAT = 0, 1, 2


def block_values(sub, N):
    """[B, B] samples -> [b, b] block values: int64 (exact) or float32 (the contract's order of adds)."""
    b = sub.shape[0] // N
    if sub.dtype == np.float32:
        acc = np.zeros((b, b), dtype=np.float32)
        for i in range(N):
            for j in range(N):
                acc = acc + sub[i::N, j::N]
        assert acc.dtype == np.float32
        return acc
    return sub.astype(np.int64).reshape(b, N, b, N).sum(axis=(1, 3))


def background(b, R):
    i, j = np.meshgrid(np.arange(b), np.arange(b), indexing="ij")
    return (i - b // 2) ** 2 + (j - b // 2) ** 2 > R * R


def extract_one(img, x, y, box, bin, bg_radius, normalize, invert):
    """-> (float32 [b, b], status)"""
    ny, nx = img.shape
    b = box // bin
    zeros = np.zeros((b, b), dtype=np.float32)
    x0, y0 = int(x) - box // 2, int(y) - box // 2
    if x0 < 0 or y0 < 0 or x0 + box > nx or y0 + box > ny:
        return zeros, OUTSIDE
    v = block_values(img[y0:y0 + box, x0:x0 + box], bin)
    if not normalize:
        out = v.astype(np.float32) / np.float32(bin * bin)
        return (-out if invert else out), OK
    bg = background(b, bg_radius)
    n = int(bg.sum())
    if n == 0:
        return zeros, FLAT
    if img.dtype == np.float32:
        d = v.astype(np.float64)
        mean = d[bg].sum() / n
        var = ((d[bg] - mean) ** 2).sum() / n
    else:
        d = v - v[0, 0]
        assert np.abs(d).max() < 2 ** 31
        terms = d[bg].astype(object)                       # Python ints from here on
        S1, S2 = int(terms.sum()), int((terms * terms).sum())
        assert abs(S2) < 2 ** 63 and abs(S1) < 2 ** 63
        mean = float(S1) / float(n)
        var = float(S2) / float(n) - mean * mean
        d = d.astype(np.float64)
    if not var > 0:
        return zeros, FLAT
    out = ((d - mean) / np.sqrt(np.float64(var))).astype(np.float32)
    return (-out if invert else out), OK


def extract_model(img, xy, box, bin=1, bg_radius=None, normalize=True, invert=False):
    """img: [ny, nx] array of an MRC sample type; xy: [P, 2] (x along nx, y along ny).
    -> (out float32 [P, b, b], status int32 [P])"""
    assert img.ndim == 2 and img.dtype in MODE_OF
    assert 2 <= box <= 1024 and 1 <= bin <= 16 and box % bin == 0 and box // bin >= 2
    b = box // bin
    if bg_radius is None:
        bg_radius = 3 * b // 8
    assert bg_radius >= 0
    xy = np.asarray(xy).reshape(-1, 2)
    out = np.zeros((len(xy), b, b), dtype=np.float32)
    status = np.zeros(len(xy), dtype=np.int32)
    for p, (x, y) in enumerate(xy):
        out[p], status[p] = extract_one(img, x, y, box, bin, bg_radius, normalize, invert)
    return out, status


def write_raw_mrc(path, array, extended_header=b""):
    """A 2-D MRC file of the array's own sample type (mode 0 / 1 / 2 / 6): write_mrc's header with the mode re-packed."""
    from spr_pick_amd import micrograph_io
    mode = MODE_OF[array.dtype]
    buf = io.BytesIO()
    micrograph_io.write_mrc(buf, np.asarray(array, dtype=np.float32), extended_header)
    head = bytearray(buf.getvalue()[:1024 + len(extended_header)])
    struct.pack_into("<i", head, 12, mode)
    with open(path, "wb") as f:
        f.write(bytes(head))
        f.write(np.ascontiguousarray(array).tobytes())


def model_extract_file(path, xy, box, bin, bg_radius, normalize, invert, device=None):
    """``spr_pick_amd.extract._extract_file`` by the model: (status-0 particles in pick order, status)."""
    from spr_pick_amd import micrograph_io
    with open(path, "rb") as f:
        img, _, _ = micrograph_io.parse_mrc(f.read())
    out, status = extract_model(img, xy, box, bin, bg_radius, normalize, invert)
    return out[status == OK], status
