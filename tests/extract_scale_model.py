"""NumPy model of the Fourier-crop extraction contract (csrc/extract.hip: extract_scale_kernel, include/sprk.h:
sprk_extract_scale), the oracle of tests/test_extract_scale_cpu.py and tests/test_gpu_extract_scale.py.

Particle p of centre (x, y) covers raw rows y0 .. y0+B-1 and columns x0 .. x0+B-1, x0 = x - B//2, y0 = y - B//2.  A box
not entirely inside the image: status 1, zeros.  M is the float32 [S, B] matrix the caller passes
(``spr_pick_amd.extract.crop_matrix``).  D = float32(x - x[0,0]) for the integer modes (exact), x for float32.
  U[r, j] = float32 fma chain over c = 0 .. B-1 ascending of D[r, c] * M[j, c], from 0;
  Y[i, j] = float32 fma chain over r = 0 .. B-1 ascending of M[i, r] * U[r, j], from 0.
Not normalised: Y + float32(x[0,0]) (one float32 add) for the integer modes, Y for float32.  Normalised, every mode:
background = {(i - S//2)^2 + (j - S//2)^2 > R^2}, n pixels (n == 0: status 2, zeros); mean = sum_bg Y / n and var =
sum_bg (Y - mean)^2 / n in float64 (NumPy's summation order), status 2 and zeros unless var > 0,
out = float32((float64(Y) - mean) / sqrt(var)).  Negated with ``invert``.

``fma32`` is an exact float32 fused multiply-add in float64 arithmetic: the product of two float32 is exact in float64
(48 significant bits); the sum with c is formed with its TwoSum error term and rounded TO ODD in float64, so that the
final rounding to float32 sees a correctly placed sticky bit — a plain float32(a*b + c) rounds twice and misses ties."""
import numpy as np

from extract_model import DTYPES, FLAT, MODE_OF, OK, OUTSIDE, background  # noqa: F401  (re-exported for the tests)


def fma32(a, b, c):
    """float32 arrays (broadcast) -> float32(a*b + c) with ONE rounding, for finite operands and results."""
    p = a.astype(np.float64) * b.astype(np.float64)              # exact
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    bb = s - p                                                   # TwoSum (Knuth): s + e == p + c exactly
    e = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy()
    fix = (e != 0) & ((bits & 1) == 0)                           # inexact and even: the odd neighbour on e's side
    away = (e > 0) == (s > 0)                                    # e points away from zero: the magnitude grows
    bits[fix & away] += 1
    bits[fix & ~away] -= 1
    return bits.view(np.float64).astype(np.float32)


def crop_product(D, M):
    """D float32 [B, B], M float32 [S, B] -> Y float32 [S, S] by the contract's two chains."""
    B, S = D.shape[0], M.shape[0]
    assert D.dtype == np.float32 and M.dtype == np.float32 and D.shape == (B, B) and M.shape == (S, B)
    Mt = np.ascontiguousarray(M.T)                               # [B, S]
    U = np.zeros((B, S), dtype=np.float32)
    for c in range(B):
        U = fma32(D[:, c:c + 1], Mt[c:c + 1, :], U)
    Y = np.zeros((S, S), dtype=np.float32)
    for r in range(B):
        Y = fma32(M[:, r:r + 1], U[r:r + 1, :], Y)
    return Y


def operand(sub):
    """[B, B] samples -> (D float32, anchor float32)"""
    if sub.dtype == np.float32:
        return sub, np.float32(0)
    d = sub.astype(np.int64) - int(sub[0, 0])
    assert np.abs(d).max() < 2 ** 24
    return d.astype(np.float32), np.float32(sub[0, 0])


def finish(Y, anchor, is_float, bg_radius, normalize, invert):
    """The output stage for one box: Y float32 [S, S] -> (float32 [S, S], status)."""
    S = Y.shape[0]
    zeros = np.zeros((S, S), dtype=np.float32)
    if not normalize:
        out = Y if is_float else Y + anchor
        assert out.dtype == np.float32
        return (-out if invert else out), OK
    bg = background(S, bg_radius)
    n = int(bg.sum())
    if n == 0:
        return zeros, FLAT
    d = Y.astype(np.float64)
    mean = d[bg].sum() / n
    var = ((d[bg] - mean) ** 2).sum() / n
    if not var > 0:
        return zeros, FLAT
    out = ((d - mean) / np.sqrt(np.float64(var))).astype(np.float32)
    return (-out if invert else out), OK


def box_of(img, x, y, box):
    """-> the [box, box] samples of the particle at (x, y), or None when the box is not entirely inside"""
    ny, nx = img.shape
    x0, y0 = int(x) - box // 2, int(y) - box // 2
    if x0 < 0 or y0 < 0 or x0 + box > nx or y0 + box > ny:
        return None
    return img[y0:y0 + box, x0:x0 + box]


def scale_products(img, xy, box, M):
    """The expensive half, to be shared between tests: -> [(Y, anchor) or None per particle]"""
    res = []
    for x, y in np.asarray(xy).reshape(-1, 2):
        sub = box_of(img, x, y, box)
        if sub is None:
            res.append(None)
        else:
            D, anchor = operand(sub)
            res.append((crop_product(D, M), anchor))
    return res


def scale_model(img, xy, box, M, bg_radius=None, normalize=True, invert=False, products=None):
    """img: [ny, nx] array of an MRC sample type; xy: [P, 2] (x along nx, y along ny); M: float32 [S, box].
    -> (out float32 [P, S, S], status int32 [P])"""
    assert img.ndim == 2 and img.dtype in MODE_OF
    S = M.shape[0]
    assert M.shape == (S, box) and 2 <= S <= box <= 1024
    if bg_radius is None:
        bg_radius = 3 * S // 8
    assert bg_radius >= 0
    xy = np.asarray(xy).reshape(-1, 2)
    if products is None:
        products = scale_products(img, xy, box, M)
    out = np.zeros((len(xy), S, S), dtype=np.float32)
    status = np.zeros(len(xy), dtype=np.int32)
    for p, prod in enumerate(products):
        if prod is None:
            status[p] = OUTSIDE
        else:
            out[p], status[p] = finish(prod[0], prod[1], img.dtype == np.float32, bg_radius, normalize, invert)
    return out, status


def model_extract_file_scaled(path, xy, box, scale, bg_radius, normalize, invert, device=None):
    """``spr_pick_amd.extract._extract_file_scaled`` by the model: (status-0 particles in pick order, status)."""
    from spr_pick_amd import extract, micrograph_io
    with open(path, "rb") as f:
        img, _, _ = micrograph_io.parse_mrc(f.read())
    out, status = scale_model(img, xy, box, extract.crop_matrix(box, scale), bg_radius, normalize, invert)
    return out[status == OK], status


def apriori_bound(D, M):
    """-> (reference float64 [S, S], bound [S, S]): |Y - M D M^T| <= (2B + 4) 2^-24 (|M| |D| |M|^T) elementwise, for the
    float32 M and D: two chains of B roundings, each within 2^-24 relative of its partial sum, plus slack for the
    second-order terms."""
    B = D.shape[0]
    M64, D64 = M.astype(np.float64), D.astype(np.float64)
    ref = M64 @ D64 @ M64.T
    return ref, (2 * B + 4) * 2.0 ** -24 * (np.abs(M64) @ np.abs(D64) @ np.abs(M64).T)
