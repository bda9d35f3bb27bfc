"""NumPy model of the tiled power spectrum (csrc/psd.hip, include/sprk.h: sprk_psd_tiles), the oracle of
tests/test_psd_cpu.py and tests/test_gpu_psd.py.

Tiles of T x T at a step of T/2: ty = (ny - T) // (T/2) + 1 rows of tx tiles, tile t = i*tx + j at (i*T/2, j*T/2).
D = float32(x - x[0,0]) for the integer modes (x[0,0] of the micrograph; exact), x for float32.  W1 float32 [2H, T] and W2
float32 [2T, 2T] are the matrices the caller passes (``spr_pick_amd.ctf.dft_matrices``), H = T/2 + 1.
  U[r, q]  = float32 fma chain over c = 0 .. T-1 ascending of D_t[r, c] * W1[q, c], from 0;
  V        = [U[:, :H] ; U[:, H:]]                                                      [2T, H];
  Re[u, v] = float32 fma chain over k = 0 .. 2T-1 ascending of W2[u, k] * V[k, v], from 0; Im with row T+u;
  Q_t      = fma(Im, Im, float32(Re * Re));
  P        = ((0 + Q_0) + Q_1) + ... in ascending tile order, float32 adds.
Every step is vectorised over the tiles (and, with ``cols``, restricted to a few columns v: the chains of different output
elements do not touch one another)."""
import numpy as np

from extract_scale_model import fma32

DTYPES = {0: np.int8, 1: np.int16, 2: np.float32, 6: np.uint16}
MODE_OF = {np.dtype(v): k for k, v in DTYPES.items()}
EPS = 2.0 ** -24


def fma(a, b, c):
    """``fma32`` at a third of its cost.  The product of two float32 is exact in float64, so s = float64(a*b + c) is the
    exact sum rounded once to 53 bits, and float32(s) is the fused result unless s sits exactly half-way between two
    float32 (the low 29 bits of its significand are 1 0...0): only there can the second rounding go the other way, and
    only those elements are redone by ``fma32``.  For results in float32's normal range, or zero."""
    s = a.astype(np.float64) * b.astype(np.float64) + c
    r = s.astype(np.float32)
    tie = (s.view(np.int64) & 0x1FFFFFFF) == 0x10000000
    if tie.any():
        a, b, c = (np.broadcast_to(x, s.shape)[tie] for x in (a, b, c))
        r[tie] = fma32(a, b, c)
    return r


def geometry(ny, nx, T):
    """-> (ty, tx)"""
    assert T % 2 == 0 and ny >= T and nx >= T
    return (ny - T) // (T // 2) + 1, (nx - T) // (T // 2) + 1


def origins(ny, nx, T):
    """-> [(y0, x0)] in tile order"""
    ty, tx = geometry(ny, nx, T)
    return [(i * (T // 2), j * (T // 2)) for i in range(ty) for j in range(tx)]


def operand(img):
    """[ny, nx] samples -> D float32"""
    if img.dtype == np.float32:
        return img
    d = img.astype(np.int64) - int(img[0, 0])
    assert np.abs(d).max() < 2 ** 24
    return d.astype(np.float32)


def tiles(img, T):
    """-> D of every tile, float32 [ntiles, T, T]"""
    D = operand(np.ascontiguousarray(img))
    return np.stack([D[y:y + T, x:x + T] for y, x in origins(*img.shape, T)])


def tile_spectra(Dt, W1, W2, cols=None):
    """Dt float32 [n, T, T] -> (Re, Im) float32 [n, T, len(cols)] by the contract's chains (cols: all H by default)"""
    n, T, _ = Dt.shape
    H = T // 2 + 1
    assert Dt.dtype == W1.dtype == W2.dtype == np.float32 and W1.shape == (2 * H, T) and W2.shape == (2 * T, 2 * T)
    cols = np.arange(H) if cols is None else np.asarray(cols)
    q = np.concatenate([cols, H + cols])
    W1T = np.ascontiguousarray(W1[q].T)                           # [T, 2m]
    U = np.zeros((n, T, len(q)), dtype=np.float32)
    for c in range(T):
        U = fma(Dt[:, :, c:c + 1], W1T[None, c:c + 1, :], U)
    V = np.concatenate([U[:, :, :len(cols)], U[:, :, len(cols):]], axis=1)    # [n, 2T, m]
    out = []
    for rows in (W2[:T], W2[T:]):
        acc = np.zeros((n, T, len(cols)), dtype=np.float32)
        for k in range(2 * T):
            acc = fma(rows[None, :, k:k + 1], V[:, k:k + 1, :], acc)
        out.append(acc)
    return out[0], out[1]


def power(Re, Im):
    """Q = fma(Im, Im, float32(Re * Re))"""
    sq = Re * Re
    assert sq.dtype == np.float32
    return fma(Im, Im, sq)


def psd(img, W1, W2, T, cols=None):
    """img: [ny, nx] array of an MRC sample type -> P float32 [T, len(cols)]"""
    assert img.ndim == 2 and img.dtype in MODE_OF
    Q = power(*tile_spectra(tiles(img, T), W1, W2, cols))
    P = np.zeros(Q.shape[1:], dtype=np.float32)
    for t in range(Q.shape[0]):
        P = P + Q[t]
    assert P.dtype == np.float32
    return P


def apriori_bound(img, W1, W2, T):
    """-> (reference float64 [T, H], bound [T, H]) for P.  The reference is sum_t |rfft2(D_t)|^2 in float64.  Re and Im of a
    tile lie within b = (3T + 4) 2^-24 (|W2| |V|) of the exact ones, |V| = the two halves of |D| |W1|^T: a chain of T
    roundings, then one of 2T, each within 2^-24 relative of its partial sum, the rounding of the two matrices' entries,
    and slack for the second-order terms.  |Q - Q_ref| <= 2 |Re| b_re + b_re^2 + 2 |Im| b_im + b_im^2, and the two roundings
    of Q with the ntiles - 1 adds of the sum (every term is positive) come to (ntiles + 3) 2^-24 relative."""
    H = T // 2 + 1
    Dt = tiles(img, T).astype(np.float64)
    n = Dt.shape[0]
    F = np.fft.rfft2(Dt)                                         # [n, T, H]
    A1, A2 = np.abs(W1.astype(np.float64)), np.abs(W2.astype(np.float64))
    absU = np.abs(Dt) @ A1.T                                     # [n, T, 2H]
    absV = np.concatenate([absU[:, :, :H], absU[:, :, H:]], axis=1)
    b_re, b_im = ((3 * T + 4) * EPS * (A @ absV) for A in (A2[:T], A2[T:]))
    ref = (F.real ** 2 + F.imag ** 2).sum(axis=0)
    dq = (2 * np.abs(F.real) * b_re + b_re ** 2 + 2 * np.abs(F.imag) * b_im + b_im ** 2).sum(axis=0)
    return ref, dq + (n + 3) * EPS * (ref + dq)


def check_bound(P, img, W1, W2, T, ref_bound=None):
    """``P`` (the device's or the model's) within the a-priori bound of the float64 reference -> worst error / bound"""
    ref, bound = apriori_bound(img, W1, W2, T) if ref_bound is None else ref_bound
    err = np.abs(P.astype(np.float64) - ref)
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    return float((err / np.maximum(bound, 1e-300)).max())
