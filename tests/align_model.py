"""NumPy models of whole-frame motion correction (csrc/align.hip, include/sprk.h: sprk_align_corr / sprk_align_accumulate,
spr_pick_amd/align.py), the oracle of tests/test_align_cpu.py and tests/test_gpu_align.py.

The two device contracts, on ``fma32`` (one float32 rounding per product, a fixed order):
  corr:        cc[f, i, j] = chain from 0 over y' = 0 .. Sy-1, then x = 0 .. Sx-1 ascending, of
                             a[f, (y' - (i-R)) mod Sy, x] * r[f, y', (x + (j-R)) mod Sx];
  accumulate:  D_f = float32(x_f - anchor) for the integer modes (exact), x_f for float32;
               U_f[r, j] = chain from 0 over c ascending of D_f[r, c] * Mx_f[j, c];
               y[i, j]   = ONE chain from 0 over (f, r) ascending of My_f[i, r] * U_f[r, j]
               (the device takes one frame per call and goes on from the stored sum: the same bits).

The estimate, in float64 on np.fft (``estimate``): what spr_pick_amd.align.estimate_shifts does on the device in float32,
written independently: Fourier shifts by phase ramps, correlation by the product of spectra, the same loop."""
import numpy as np

from extract_scale_model import fma32
from resample_model import DTYPES, MODE_OF  # noqa: F401  (the tests take the modes from here)


# ---- the correlation window ------------------------------------------------------------------------------------------------
def corr(a, r, R):
    """a float32 [Z, Sy, Sx]; r float32 [Z, Sy, Sx] or [Sy, Sx] (one shared reference) -> cc float32 [Z, 2R+1, 2R+1]"""
    Z, Sy, Sx = a.shape
    if r.ndim == 2:
        r = np.broadcast_to(r, a.shape)
    assert a.dtype == r.dtype == np.float32 and r.shape == a.shape and 2 * R + 1 <= Sx
    d = np.arange(-R, R + 1)
    cc = np.zeros((Z, 2 * R + 1, 2 * R + 1), dtype=np.float32)
    for y in range(Sy):
        rows = (y - d) % Sy                                      # [n]: the row of a for every row shift
        for x in range(Sx):
            cols = (x + d) % Sx                                  # [n]: the column of r for every column shift
            cc = fma32(a[:, rows, x][:, :, None], r[:, y, cols][:, None, :], cc)
    return cc


# ---- the running sum -------------------------------------------------------------------------------------------------------
def operand(img, anchor):
    """[ny, nx] samples -> D float32: minus the anchor for the integer modes (exact), as they are for float32"""
    if img.dtype == np.float32:
        assert anchor == 0
        return img
    d = img.astype(np.int64) - int(anchor)
    assert float(anchor) == int(anchor) and np.abs(d).max() < 2 ** 24
    return d.astype(np.float32)


def accumulate(frames, Mys, Mxs, anchor):
    """frames: Z arrays [ny, nx] of one sample type; Mys / Mxs: Z float32 matrices [by, ny] / [bx, nx] -> y float32 [by, bx]
    by the single chain over (frame, row) — without the anchor term the host adds at the end."""
    by, bx = Mys[0].shape[0], Mxs[0].shape[0]
    y = np.zeros((by, bx), dtype=np.float32)
    for img, My, Mx in zip(frames, Mys, Mxs):
        D = operand(np.ascontiguousarray(img), anchor)
        ny, nx = D.shape
        assert My.dtype == Mx.dtype == np.float32 and My.shape == (by, ny) and Mx.shape == (bx, nx)
        MxT = np.ascontiguousarray(Mx.T)
        U = np.zeros((ny, bx), dtype=np.float32)
        for c in range(nx):
            U = fma32(D[:, c:c + 1], MxT[c:c + 1, :], U)
        for r in range(ny):
            y = fma32(My[:, r:r + 1], U[r:r + 1, :], y)
    return y


def check_bound(y, frames, Mys, Mxs, anchor):
    """``y`` (the device's or the model's) within the a-priori bound of the float64 sum of products:
    |y - sum_f My_f D_f Mx_f^T| <= (Z ny + nx + 4) 2^-24 sum_f (|My_f| |D_f| |Mx_f|^T) elementwise: a chain of nx roundings per
    element of U, then one of Z ny, each within 2^-24 relative of its partial sum, plus slack for the second-order terms (the
    bound of resample_model.check_bound with the second chain Z times as long).  -> the worst error / bound ratio."""
    ref, bound = 0.0, 0.0
    for img, My, Mx in zip(frames, Mys, Mxs):
        D = operand(np.ascontiguousarray(img), anchor).astype(np.float64)
        My64, Mx64 = My.astype(np.float64), Mx.astype(np.float64)
        ref = ref + My64 @ D @ Mx64.T
        bound = bound + np.abs(My64) @ np.abs(D) @ np.abs(Mx64).T
    ny, nx = frames[0].shape
    bound = (len(frames) * ny + nx + 4) * 2.0 ** -24 * bound
    err = np.abs(y.astype(np.float64) - ref)
    assert (err <= bound).all(), float((err - bound).max())
    return float((err / np.maximum(bound, 1e-300)).max())


# ---- the operator by np.fft (the reference of shift_matrix64) ----------------------------------------------------------------
def fft_shift_crop(v, S, delta):
    """v float64 [B] -> [S]: fft, phase ramp e^{-2 pi i k delta / B}, crop to S frequencies, ifft, times S / B; for even S
    the +-S/2 terms enter at half weight each (for S == B they are the same bin: its ramp becomes cos(pi delta))."""
    B = len(v)
    X = np.fft.fft(np.asarray(v, dtype=np.float64))
    k = np.fft.fftfreq(S, 1.0 / S).round().astype(int)          # signed frequencies of the output bins; -S/2 for even S
    Y = X[k % B] * np.exp(-2j * np.pi * k * delta / B)
    if S % 2 == 0:
        h = S // 2
        Y[h] = 0.5 * (X[h % B] * np.exp(-2j * np.pi * h * delta / B) + X[(-h) % B] * np.exp(2j * np.pi * h * delta / B))
    out = np.fft.ifft(Y) * (S / B)
    assert np.abs(out.imag).max() <= 1e-9 * max(1.0, np.abs(out.real).max())
    return out.real


# ---- a synthetic movie -------------------------------------------------------------------------------------------------------
def shift2(img, dy, dx):
    """img float64 [ny, nx] displaced by (dy, dx) pixels, periodic: out(p) = img(p - d), by phase ramps (the Nyquist bins
    of even sides get the cosine, which keeps the result real)."""
    ny, nx = img.shape

    def ramp(n, d):
        k = np.fft.fftfreq(n, 1.0 / n)
        w = np.exp(-2j * np.pi * k * d / n)
        if n % 2 == 0:
            w[n // 2] = np.cos(np.pi * d)
        return w
    return np.fft.ifft2(np.fft.fft2(img) * ramp(ny, dy)[:, None] * ramp(nx, dx)[None, :]).real


def specimen(ny, nx, seed, cutoff=0.18):
    """a band-limited random field, unit variance: white noise under a Gaussian low-pass at ``cutoff`` cycles per pixel"""
    rng = np.random.RandomState(seed)
    fy, fx = np.fft.fftfreq(ny)[:, None], np.fft.fftfreq(nx)[None, :]
    s = np.fft.ifft2(np.fft.fft2(rng.standard_normal((ny, nx))) * np.exp(-(fy * fy + fx * fx) / (2 * (cutoff / 2) ** 2))).real
    return (s - s.mean()) / s.std()


def drift_curve(Z, seed, amplitude=5.0):
    """-> [Z, 2] (dx, dy): a random walk with a steady component, scaled so that the largest |component| is ``amplitude``"""
    rng = np.random.RandomState(1000 + seed)
    d = np.cumsum(rng.standard_normal((Z, 2)) + rng.standard_normal(2), axis=0)
    d -= d.mean(axis=0)
    return d * (amplitude / np.abs(d).max())


def make_movie(ny, nx, Z, seed, noise, signal=60.0, offset=900.0, dtype=np.int16):
    """-> (movie [Z, ny, nx] of ``dtype``, specimen float64 [ny, nx], drift [Z, 2] (dx, dy) with mean zero): frame f is the
    specimen displaced by drift[f], times ``signal``, plus Gaussian noise of ``noise`` x ``signal`` per pixel, plus
    ``offset``, rounded."""
    spec, drift = specimen(ny, nx, seed), drift_curve(Z, seed)
    rng = np.random.RandomState(2000 + seed)
    frames = [signal * shift2(spec, dy, dx) + noise * signal * rng.standard_normal((ny, nx)) + offset for dx, dy in drift]
    return np.rint(np.stack(frames)).astype(dtype), spec, drift


# ---- the estimate in float64 -------------------------------------------------------------------------------------------------
def fit_peaks(cc):
    """[Z, n, n] -> (py, px) float64 [Z] from the window's centre, edge [Z]: arg-max clamped to the interior, then the
    vertex of the parabola through three points per axis (within half a pixel)"""
    Z, n, _ = cc.shape
    R = (n - 1) // 2
    py, px, edge = np.zeros(Z), np.zeros(Z), np.zeros(Z, dtype=bool)
    for f in range(Z):
        iy, ix = np.unravel_index(np.argmax(cc[f]), (n, n))
        edge[f] = iy in (0, n - 1) or ix in (0, n - 1)
        iy, ix = min(max(iy, 1), n - 2), min(max(ix, 1), n - 2)
        for axis, (lo, hi) in enumerate(((cc[f, iy - 1, ix], cc[f, iy + 1, ix]), (cc[f, iy, ix - 1], cc[f, iy, ix + 1]))):
            curv = lo - 2 * cc[f, iy, ix] + hi
            off = min(max(0.5 * (lo - hi) / curv, -0.5), 0.5) if curv < 0 else 0.0
            if axis == 0:
                py[f] = iy - R + off
            else:
                px[f] = ix - R + off
    return py, px, edge


def window(a, r, R):
    """the correlation window of ``corr`` for one frame in float64, by the product of spectra"""
    full = np.fft.ifft2(np.conj(np.fft.fft2(a)) * np.fft.fft2(r)).real       # full[d] = sum_q a[q] r[q + d]
    d = np.arange(-R, R + 1)
    return full[np.ix_(d % a.shape[0], d % a.shape[1])]


def estimate(reduced, R, iters, tol=0.01):
    """reduced float64 [Z, Sy, Sx] (means taken out) -> (sy, sx, iterations): the shift that lays each frame on the others"""
    Z = len(reduced)
    sy, sx = np.zeros(Z), np.zeros(Z)
    for it in range(iters):
        shifted = np.stack([shift2(reduced[f], sy[f], sx[f]) for f in range(Z)])
        total = shifted.sum(axis=0)
        py, px, _ = fit_peaks(np.stack([window(reduced[f], total - shifted[f], R) for f in range(Z)]))
        py, px = py - py.mean(), px - px.mean()
        moved = max(np.abs(py - sy).max(), np.abs(px - sx).max())
        sy, sx = py, px
        if moved < tol:
            break
    return sy, sx, it + 1


def estimate_movie(movie, Sy, Sx, R=16, iters=6):
    """movie [Z, ny, nx] -> drift [Z, 2] (dx, dy) in raw pixels, mean zero: frames Fourier-cropped to [Sy, Sx] with the
    float64 matrices of ingest.resample_matrix64, means out, ``estimate``, scaled back and negated (a frame displaced by d is
    laid back by -d)."""
    from spr_pick_amd import ingest
    Z, ny, nx = movie.shape
    My, Mx = ingest.resample_matrix64(ny, Sy), ingest.resample_matrix64(nx, Sx)
    reduced = np.stack([My @ f.astype(np.float64) @ Mx.T for f in movie])
    reduced -= reduced.mean(axis=(1, 2), keepdims=True)
    sy, sx, _ = estimate(reduced, R, iters)
    return np.stack([-sx * (nx / Sx), -sy * (ny / Sy)], axis=1)


# The end-to-end cases of both test files: 256 x 320, Z = 8, int16, drift within +-5 pixels, (seed, noise / signal).
# The model's own worst error |estimated - planted| over them, measured on the CPU (test_align_cpu prints it), is
# MODEL_WORST raw pixels; the recovery condition of both tests is 1.5 times that, and it has to lie below 0.5.
MOVIE_SHAPE, MOVIE_FRAMES = (256, 320), 8
MOVIE_CASES = [(1, 1.0), (2, 2.0), (3, 4.0)]
MODEL_WORST = 0.289                              # case (3, 4.0): 0.2886; (1, 1.0): 0.029, (2, 2.0): 0.050
