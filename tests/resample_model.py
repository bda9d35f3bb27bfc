"""NumPy model of the Fourier-cropped micrograph ingest (csrc/resample.hip, include/sprk.h: sprk_ingest_resample, DESIGN
§4.3c), the oracle of tests/test_resample_cpu.py and tests/test_gpu_resample.py.

My float32 [by, ny] and Mx float32 [bx, nx] are the matrices the caller passes (``spr_pick_amd.ingest.resample_matrix``).
D = float32(x - x[0,0]) for the integer modes (exact), x for float32.
  U[r, j] = float32 fma chain over c = 0 .. nx-1 ascending of D[r, c] * Mx[j, c], from 0;
  Y[i, j] = float32 fma chain over r = 0 .. ny-1 ascending of My[i, r] * U[r, j], from 0.
out = Y + float32(x[0,0]) (one float32 add) for the integer modes, Y for float32; range = (min, max) of out.

Geometry: by = floor(ny / F + 1/2) in rationals, bx likewise.  Coordinates: output pixel s sits at input position
s * B / S; to_raw rounds that to the nearest sample (halves up), to_scaled is its inverse on the pixels."""
from fractions import Fraction

import numpy as np

from extract_scale_model import fma32

DTYPES = {0: np.int8, 1: np.int16, 2: np.float32, 6: np.uint16}
MODE_OF = {np.dtype(v): k for k, v in DTYPES.items()}


def geometry(ny, nx, F):
    F = Fraction(F)
    return tuple(int((Fraction(n) / F + Fraction(1, 2)).__floor__()) for n in (ny, nx))


def to_raw(x, n, b):
    """pixel x of b -> sample of n"""
    return (2 * x * n + b) // (2 * b)


def to_scaled(xr, n, b):
    """sample xr of n -> (pixel of b, inside)"""
    return min((2 * xr * b + n) // (2 * n), b - 1), 0 <= xr < n


def operand(img):
    """[ny, nx] samples -> (D float32, anchor float32 or None)"""
    if img.dtype == np.float32:
        return img, None
    d = img.astype(np.int64) - int(img[0, 0])
    assert np.abs(d).max() < 2 ** 24
    return d.astype(np.float32), np.float32(img[0, 0])


def product(D, My, Mx):
    """D float32 [ny, nx], My float32 [by, ny], Mx float32 [bx, nx] -> Y float32 [by, bx] by the contract's two chains."""
    ny, nx = D.shape
    by, bx = My.shape[0], Mx.shape[0]
    assert D.dtype == My.dtype == Mx.dtype == np.float32 and My.shape == (by, ny) and Mx.shape == (bx, nx)
    MxT = np.ascontiguousarray(Mx.T)                             # [nx, bx]
    U = np.zeros((ny, bx), dtype=np.float32)
    for c in range(nx):
        U = fma32(D[:, c:c + 1], MxT[c:c + 1, :], U)
    Y = np.zeros((by, bx), dtype=np.float32)
    for r in range(ny):
        Y = fma32(My[:, r:r + 1], U[r:r + 1, :], Y)
    return Y


def resample(img, My, Mx):
    """-> (out float32 [by, bx], range float32 [2])"""
    assert img.ndim == 2 and img.dtype in MODE_OF
    D, anchor = operand(np.ascontiguousarray(img))
    out = product(D, My, Mx)
    if anchor is not None:
        out = out + anchor
    assert out.dtype == np.float32
    return out, np.array([out.min(), out.max()], dtype=np.float32)


def apriori_bound(D, My, Mx):
    """-> (reference float64 [by, bx], bound [by, bx]): |Y - My D Mx^T| <= (nx + ny + 4) 2^-24 (|My| |D| |Mx|^T)
    elementwise for the float32 matrices and D: a chain of nx roundings, then one of ny, each within 2^-24 relative of its
    partial sum, plus slack for the second-order terms."""
    ny, nx = D.shape
    My64, Mx64, D64 = My.astype(np.float64), Mx.astype(np.float64), D.astype(np.float64)
    ref = My64 @ D64 @ Mx64.T
    return ref, (nx + ny + 4) * 2.0 ** -24 * (np.abs(My64) @ np.abs(D64) @ np.abs(Mx64).T)


def check_bound(out, img, My, Mx):
    """``out`` (the device's or the model's) within the a-priori bound of the float64 product; the anchor add of the
    integer modes is one more float32 rounding, within 2^-24 of |out|.  -> the worst error / bound ratio."""
    D, anchor = operand(np.ascontiguousarray(img))
    ref, bound = apriori_bound(D, My, Mx)
    got = out.astype(np.float64)
    if anchor is not None:
        ref = ref + float(anchor)
        bound = bound + 2.0 ** -24 * np.abs(got)
    err = np.abs(got - ref)
    assert (err <= bound).all(), float((err - bound).max())
    return float((err / np.maximum(bound, 1e-300)).max())
