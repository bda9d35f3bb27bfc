"""Writes tests/golden/contamination.npz: a few small micrographs and, for each, the index set that the
reference's own find_contamination (utils/algorithms.py:24-57) returns for it.

Run by hand on a machine that has the reference tree (pytest does not collect this file):
    python tests/make_contamination_golden.py
The reference module is imported through oracle/ref_shim.py.  cv2 is not installed, so the two cv2 calls the filter
makes are given NumPy stand-ins defined below: cv2.normalize(NORM_MINMAX, CV_8U) and cv2.blur (BORDER_REFLECT_101,
a NumPy view being a whole image to cv2).  They restate OpenCV's arithmetic; the reference's own loop
then produces the set — seed test, disk offsets, clipping and the flat index."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cv2_normalize(src, dst, alpha=0, beta=255, norm_type=32, dtype=0):
    assert dst is None and norm_type == 32 and dtype == 0 and (alpha, beta) == (0, 255)
    x = np.asarray(src, dtype=np.float32)
    lo, hi = float(x.min()), float(x.max())
    s = (beta - alpha) / (hi - lo) if hi - lo > np.finfo(np.float64).eps else 0.0
    a, b = np.float32(s), np.float32(alpha - lo * s)
    y = np.multiply(x, a, dtype=np.float32)
    y = np.add(y, b, dtype=np.float32)
    return np.clip(np.rint(y), 0, 255).astype(np.uint8)


def _border(p, n):
    if 0 <= p < n:
        return p
    if n == 1:
        return 0
    while not 0 <= p < n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def cv2_blur(src, ksize):
    kh, kw = ksize
    src = np.asarray(src)
    h, w = src.shape
    rows = np.array([[_border(i + d, h) for d in range(-(kh // 2), kh // 2 + 1)] for i in range(h)])
    cols = np.array([[_border(j + d, w) for d in range(-(kw // 2), kw // 2 + 1)] for j in range(w)])
    s = src.astype(np.int64)[rows[:, :, None, None], cols[None, None, :, :]].sum(axis=(1, 3))
    n = kh * kw
    return ((s + n // 2) // n).astype(np.uint8)


def micrographs():
    """Noise plus dark and bright blobs; blobs touch every border and a corner so that the clip and the wrap of the
    reference's index arithmetic are exercised."""
    rng = np.random.default_rng(20261016)
    out = []
    for k, (H, W) in enumerate(((256, 320), (200, 176), (96, 128))):
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        img = rng.normal(0.0, 1.0, (H, W)).astype(np.float32)
        blobs = [(0, 0, 14, -6), (H - 1, W // 2, 10, 7), (H // 3, W - 1, 9, -6), (H // 2, 0, 8, 7),
                 (0, W - 2, 7, -6), (H - 2, W - 1, 11, 7), (H // 2 + 7 * k, W // 2 - 5 * k, 6, -6)]
        for cy, cx, rad, amp in blobs:
            img += np.float32(amp) * (((yy - cy) ** 2 + (xx - cx) ** 2) <= rad * rad)
        img = np.round(img * 16) / np.float32(16)     # few mantissa bits: the fixture compresses
        out.append(img.astype(np.float32))
    return out


def main():
    from oracle import ref_shim
    R = ref_shim.load()
    cv2 = sys.modules["cv2"]
    assert isinstance(cv2, types.ModuleType) and not hasattr(cv2, "__file__"), "a real cv2 is installed: use it"
    cv2.NORM_MINMAX, cv2.CV_8U = 32, 0
    cv2.normalize, cv2.blur = cv2_normalize, cv2_blur
    find = sys.modules["spr_pick.utils.algorithms"].find_contamination
    arrays = {}
    for k, img in enumerate(micrographs()):
        got = find(img.copy())
        arrays["img%d" % k] = img
        arrays["set%d" % k] = np.array(sorted(int(v) for v in got), dtype=np.int32)
        print("img%d %s: %d indices" % (k, img.shape, len(got)))
    path = os.path.join(ROOT, "tests", "golden", "contamination.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")
    del R


if __name__ == "__main__":
    main()
