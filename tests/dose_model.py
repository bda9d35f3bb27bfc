"""NumPy models of the dose-weighted sum (csrc/alignsum.hip, include/sprk.h: sprk_align_spectrum / sprk_align_synthesize,
spr_pick_amd/dose.py), the oracle of tests/test_dose_cpu.py and tests/test_gpu_dose.py.

The two device contracts on float32 fma chains (one rounding per product, K ascending from 0, ``extract_filter_model.chain``).
W1 .. W4 are the float32 matrices the caller passes without their padding columns, g_f the float32 [2Ku, Hs] filter of
frame f (real rows over imaginary rows), D_f = float32(x_f - anchor) for the integer modes (exact), x_f for float32:
  spectrum, per frame:  U[r, q]  = chain over c of D[r, c] * W1[q, c];          V = [U[:, :Hs] ; U[:, Hs:]]      [2ny, Hs]
                        A[kk, v] = chain over t of W2[kk, t] * V[t, v];  B with row Ku + kk;
                        Fr = fma(A, Gr, fma(-B, Gi, Fr_old)),  Fi = fma(A, Gi, fma(B, Gr, Fi_old)),  F_old = 0 at first
  synthesize, once:     Zr[i, v] = chain over t of W3[i, t] * F[t, v];  Zi with row by + i;   Z = [Zr, Zi]       [by, 2Hs]
                        Y[i, j]  = chain over t of Z[i, t] * W4[j, t]."""
import numpy as np

from align_model import DTYPES, MODE_OF, drift_curve, operand, shift2, specimen  # noqa: F401
from extract_filter_model import EPS, chain, correlation  # noqa: F401
from psd_model import fma


# ---- the contracts in float32 ----------------------------------------------------------------------------------------------
def spectrum(frames, W1, W2, gs, anchor):
    """frames: Z arrays [ny, nx] of one sample type; W1 float32 [2Hs, nx], W2 float32 [2Ku, 2ny]; gs: Z float32 [2Ku, Hs]
    -> F float32 [2Ku, Hs] after the Z calls (the first with ``first`` set)"""
    Hs, Ku = W1.shape[0] // 2, W2.shape[0] // 2
    F = None
    for img, g in zip(frames, gs):
        D = operand(np.ascontiguousarray(img), anchor)
        ny, nx = D.shape
        assert W1.dtype == W2.dtype == g.dtype == np.float32
        assert W1.shape == (2 * Hs, nx) and W2.shape == (2 * Ku, 2 * ny) and g.shape == (2 * Ku, Hs)
        U = chain(D, np.ascontiguousarray(W1.T))                     # [ny, 2Hs]
        X = chain(W2, np.concatenate([U[:, :Hs], U[:, Hs:]]))        # [2Ku, Hs]: A over B
        A, B, Gr, Gi = X[:Ku], X[Ku:], g[:Ku], g[Ku:]
        old = np.zeros((2 * Ku, Hs), dtype=np.float32) if F is None else F
        F = np.concatenate([fma(A, Gr, fma(-B, Gi, old[:Ku])), fma(A, Gi, fma(B, Gr, old[Ku:]))])
        assert F.dtype == np.float32
    return F


def synthesize(F, W3, W4):
    """F float32 [2Ku, Hs], W3 float32 [2by, 2Ku], W4 float32 [bx, 2Hs] -> Y float32 [by, bx]"""
    by = W3.shape[0] // 2
    assert F.dtype == W3.dtype == W4.dtype == np.float32 and W3.shape[1] == F.shape[0] and W4.shape[1] == 2 * F.shape[1]
    Zs = chain(W3, F)                                                # [2by, Hs]: Zr over Zi
    return chain(np.concatenate([Zs[:by], Zs[by:]], axis=1), np.ascontiguousarray(W4.T))


def unpadded(W, ny, nx, by, bx, Ku):
    """the operands of spr_pick_amd.dose.spectrum_matrices (arrays) without their padding columns, which must be zeros"""
    Hs = bx // 2 + 1
    out = []
    for m, cols in zip(W, (nx, 2 * ny, 2 * Ku, 2 * Hs)):
        m = np.asarray(m)
        assert not m[:, cols:].any()
        out.append(np.ascontiguousarray(m[:, :cols]))
    return out


# ---- the same product in float64 -------------------------------------------------------------------------------------------
def spectrum64(Ds, W1, W2, Gs):
    """Ds: Z float64 [ny, nx]; W1, W2 float64; Gs: Z complex [Ku, Hs] -> F complex [Ku, Hs]"""
    Hs, Ku = W1.shape[0] // 2, W2.shape[0] // 2
    F = 0.0
    for D, G in zip(Ds, Gs):
        U = D @ W1.T
        X = W2 @ np.concatenate([U[:, :Hs], U[:, Hs:]])
        F = F + (X[:Ku] + 1j * X[Ku:]) * G
    return F


def synthesize64(F, W3, W4):
    by = W3.shape[0] // 2
    Zs = W3 @ np.concatenate([F.real, F.imag])
    return np.concatenate([Zs[:by], Zs[by:]], axis=1) @ W4.T


def product64(Ds, W64, Gs):
    """the four stages in float64 -> Y [by, bx]"""
    return synthesize64(spectrum64(Ds, W64[0], W64[1], Gs), W64[2], W64[3])


def complex_of(g):
    """float32 or float64 [2Ku, Hs] -> complex128 [Ku, Hs]"""
    Ku = g.shape[0] // 2
    return g[:Ku].astype(np.float64) + 1j * g[Ku:].astype(np.float64)


def apriori_bound(Ds, W, gs, exact_operands=0):
    """-> (reference float64 [by, bx], bound [by, bx]) for float32 operands W (four matrices) and gs (Z filters [2Ku, Hs]) and
    the frames' operands Ds (float32 or float64 [ny, nx], exact):

        |Y - ref| <= (nx + 2ny + 2Z + 2Ku + 2Hs + 8 + exact_operands) 2^-24  |W4| |W3| sum_f (|G_f| . (|W2| |W1| |D_f|))

    elementwise, the stages composed as ``product64`` composes them and |G| . X standing for the four real products of
    the complex multiply with every sign made positive.  Derivation (the one of extract_filter_model.apriori_bound, made
    before any device output was seen): a chain of K fma roundings is within K 2^-24, relative, of the sum of the absolute
    values of its terms; the four chains have K = nx, 2ny, 2Ku and 2Hs.  The running spectrum takes two fma roundings per
    frame and component, each relative to a partial sum that the absolute sum over the frames bounds: 2Z.  An error made
    in one stage passes through the stages after it multiplied by their absolute values, which is what the product of
    absolute matrices is; the second-order terms (errors of errors) are below (sum of the K)^2 2^-48 of the same product,
    which for K sums up to 2^17 is below 2^-14 of the first-order term, and the constant 8 holds them and the rounding of
    intermediate results read back as operands.  ``exact_operands``: when ``ref`` is to stand for operands known only to
    within one float32 ulp (the float64 matrices and filters, rounded on another device), each of the five operand
    factors W1, W2, G, W3, W4 adds up to 2 x 2^-24, relative, to every term: pass 10."""
    W64 = [np.asarray(m, dtype=np.float64) for m in W]
    Ds = [np.asarray(D, dtype=np.float64) for D in Ds]
    Gs = [complex_of(g) for g in gs]
    ref = product64(Ds, W64, Gs)
    # every sign positive: |A| |Gr| + |B| |Gi| for the real part, |A| |Gi| + |B| |Gr| for the imaginary one
    Wa = [np.abs(m) for m in W64]
    Hs, Ku = Wa[0].shape[0] // 2, Wa[1].shape[0] // 2
    Fr = Fi = 0.0
    for D, G in zip(Ds, Gs):
        U = np.abs(D) @ Wa[0].T
        X = Wa[1] @ np.concatenate([U[:, :Hs], U[:, Hs:]])
        Fr = Fr + X[:Ku] * np.abs(G.real) + X[Ku:] * np.abs(G.imag)
        Fi = Fi + X[:Ku] * np.abs(G.imag) + X[Ku:] * np.abs(G.real)
    absolute = synthesize64(Fr + 1j * Fi, Wa[2], Wa[3])
    ny, nx = Ds[0].shape
    return ref, (nx + 2 * ny + 2 * len(Ds) + 2 * Ku + 2 * Hs + 8 + exact_operands) * EPS * absolute


# ---- the end-to-end movies: a specimen that the exposure damages ------------------------------------------------------------
MOVIE_SHAPE, MOVIE_FRAMES, APIX, DOSE, KV = (128, 192), 8, 1.5, 10.0, 300.0
MOVIE_CASES = [(1, 1.0), (2, 2.0)]                                   # (seed, noise / signal)


def plane_exponent(ny, nx, apix, kv):
    """-1 / (2 Ne) over the full plane of np.fft's frequencies, 0 at the origin"""
    from spr_pick_amd import dose
    fy, fx = np.fft.fftfreq(ny)[:, None] / apix, np.fft.fftfreq(nx)[None, :] / apix
    q = np.sqrt(fy * fy + fx * fx)
    return np.where(q == 0, 0.0, -0.5 / dose.critical_dose(np.where(q == 0, 1.0, q), kv))


def make_movie(ny, nx, Z, seed, noise, apix=APIX, dose=DOSE, kv=KV, signal=60.0, offset=900.0, dtype=np.int16, drift=True):
    """-> (movie [Z, ny, nx] of ``dtype``, specimen float64 [ny, nx], drift [Z, 2] (dx, dy) with mean zero): frame f is the
    specimen (``align_model.specimen`` with cutoff 0.4) damaged by exp(-N_f / (2 Ne)) per frequency, N_f = (f + 1) dose,
    displaced by drift[f], times ``signal``, plus Gaussian noise of ``noise`` x ``signal`` per pixel, plus ``offset``,
    rounded."""
    spec = specimen(ny, nx, seed, cutoff=0.4)
    d = drift_curve(Z, seed) if drift else np.zeros((Z, 2))
    E = plane_exponent(ny, nx, apix, kv)
    rng = np.random.RandomState(2000 + seed)
    S = np.fft.fft2(spec)
    frames = []
    for f, (dx, dy) in enumerate(d):
        damaged = np.fft.ifft2(S * np.exp((f + 1) * dose * E)).real
        frames.append(signal * shift2(damaged, dy, dx) + noise * signal * rng.standard_normal((ny, nx)) + offset)
    return np.rint(np.stack(frames)).astype(dtype), spec, d


def model_sums(movie, drift, apix=APIX, dose=DOSE, pre_dose=0.0, kv=KV):
    """the float64 model on np.fft, full size -> (plain, weighted): every frame laid back by -drift[f] and summed, as it is
    and under Phi_f = w_f sqrt(Z / sum w^2) (1 at the origin)"""
    Z, ny, nx = movie.shape
    E = plane_exponent(ny, nx, apix, kv)
    N = pre_dose + (np.arange(Z) + 1.0) * dose
    w = np.exp(N[:, None, None] * E[None])
    phi = w * np.sqrt(Z / (w * w).sum(axis=0))[None]
    phi[:, E == 0] = 1.0
    plain = weighted = 0.0
    for f in range(Z):
        back = shift2(movie[f].astype(np.float64), -drift[f, 1], -drift[f, 0])
        plain = plain + back
        weighted = weighted + np.fft.ifft2(np.fft.fft2(back) * phi[f]).real
    return plain, weighted


def model_gain(movie, spec, drift, **kw):
    """-> (corr(plain, specimen), corr(weighted, specimen)) of ``model_sums``"""
    plain, weighted = model_sums(movie, drift, **kw)
    return correlation(plain, spec), correlation(weighted, spec)
