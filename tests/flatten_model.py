"""NumPy model of the background flattening of the micrograph ingest (sprk_ingest_flatten, include/sprk.h; DESIGN
§4.3c) and the images its tests share.  The window sums are integers (t = floor((x - lo) * 2^(30 - ilogb(hi - lo))) <
2^31), so this model's prefix sums, the brute-force window loop it is checked against and the device's running sums
all give the same bits; the GPU tests compare the kernels with it without a tolerance."""
import numpy as np

MAX_R = 1023            # SPRK_INGEST_MAX_FLATTEN: 2^31 * 2047^2 < 2^53
CROP = (slice(32, 64), slice(64, 96))          # the central 32 x 32 of the 96 x 160 level-count image


def scale(rng):
    """-> (lo as float64, e = ilogb(double(hi) - double(lo)) or None when hi == lo)"""
    lo, hi = np.float64(np.float32(rng[0])), np.float64(np.float32(rng[1]))
    span = hi - lo
    assert span >= 0
    if span == 0:
        return lo, None
    return lo, int(np.frexp(span)[1]) - 1


def fixed(x, rng):
    """-> (d = double(x) - double(lo), t = floor(d * 2^(30 - e)) as int64, e); the image must lie inside rng"""
    lo, e = scale(rng)
    d = np.asarray(x, dtype=np.float32).astype(np.float64) - lo
    t = np.floor(np.ldexp(d, 30 - e)).astype(np.int64)
    assert t.min() >= 0 and t.max() < 2 ** 31, "the image is not inside its range"
    return d, t, e


def windows(n, R):
    """first and one-past-last index of the clamped window of every position on an axis of n"""
    i = np.arange(n)
    return np.maximum(i - R, 0), np.minimum(i + R, n - 1) + 1


def box_sums(t, R):
    """-> (S int64 [by, bx]: the sum of t over every clamped window, from a 2-D prefix sum; cnt: the windows' sizes)"""
    by, bx = t.shape
    assert t.size < 2 ** 31                      # the prefix sum stays below 2^62
    P = np.zeros((by + 1, bx + 1), dtype=np.int64)
    P[1:, 1:] = np.cumsum(np.cumsum(t, axis=0), axis=1)
    r0, r1 = windows(by, R)
    c0, c1 = windows(bx, R)
    S = P[np.ix_(r1, c1)] - P[np.ix_(r0, c1)] - P[np.ix_(r1, c0)] + P[np.ix_(r0, c0)]
    return S, np.outer(r1 - r0, c1 - c0)


def finish(d, S, cnt, e):
    assert int(S.max()) < 2 ** 53                # double(S) is exact
    bg = np.ldexp(S.astype(np.float64) / cnt.astype(np.float64), e - 30)
    return (d - bg).astype(np.float32)


def flatten(x, R, rng=None):
    """-> (flat float32 [by, bx], float32 [2] = its min and max).  rng = (lo, hi) bounding x; None: its min and max."""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim == 2 and 1 <= R <= MAX_R
    if rng is None:
        rng = (x.min(), x.max())
    if scale(rng)[1] is None:
        return np.zeros(x.shape, dtype=np.float32), np.zeros(2, dtype=np.float32)
    d, t, e = fixed(x, rng)
    S, cnt = box_sums(t, R)
    flat = finish(d, S, cnt, e)
    return flat, np.array([flat.min(), flat.max()], dtype=np.float32)


def flatten_brute(x, R, rng=None):
    """The same by a per-pixel loop over the window: Python integers, no prefix sum."""
    x = np.asarray(x, dtype=np.float32)
    if rng is None:
        rng = (x.min(), x.max())
    d, t, e = fixed(x, rng)
    by, bx = x.shape
    S, cnt = np.zeros((by, bx), dtype=np.int64), np.zeros((by, bx), dtype=np.int64)
    for r in range(by):
        for c in range(bx):
            win = t[max(r - R, 0):min(r + R, by - 1) + 1, max(c - R, 0):min(c + R, bx - 1) + 1]
            S[r, c], cnt[r, c] = sum(int(v) for v in win.ravel()), win.size
    flat = finish(d, S, cnt, e)
    return flat, np.array([flat.min(), flat.max()], dtype=np.float32)


def ramp_image(seed=0, outliers=False, shape=(96, 160)):
    """float32 100 + 5 randn + 200 x/(W-1) + 80 y/(H-1); with ``outliers`` 5 samples at 30000 and 3 at -500"""
    H, W = shape
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = (100 + 5 * rs.randn(H, W) + 200.0 * xx / (W - 1) + 80.0 * yy / (H - 1)).astype(np.float32)
    if outliers:
        img.reshape(-1)[rs.choice(img.size, 8, replace=False)] = [30000] * 5 + [-500] * 3
    return img


def crop_levels(u8):
    """distinct grey levels in the central 32 x 32 crop of the 96 x 160 image"""
    return int(np.unique(np.asarray(u8)[CROP]).size)
