"""Vectorised NumPy model of the contamination mask (csrc/contam.hip): the reference's
find_contamination (utils/algorithms.py:24-57) stated step by step.

* ``normalise``: cv2.normalize(NORM_MINMAX, CV_8U) restated — a = float32(255/(max-min)), b = float32(-min*255/(max-min))
  (quotient in double), u = rint_half_even(float32(float32(x*a) + b)) saturated to [0, 255]; min / max over the finite
  pixels, NaN -> 0, u = 0 everywhere when max - min <= DBL_EPSILON;
* ``blur``: cv2.blur(ksize x ksize) of the crop restated — (sum + K*K//2) // (K*K), BORDER_REFLECT_101 inside the crop;
* ``seeds``: blurred pixel < mean - k_low*std or > mean + k_high*std, mean / std of the whole uint8 image;
* ``contam_set_literal``: the reference's clipped-disk indices, one vectorised scatter per disk offset (small maps);
* ``contam_set_bitmap``: the same set as the dilation of the seeds on the crop grid extended by one row and one column
  (the form the kernel evaluates; any map size);
* ``score_mask``: the set in the score map's frame: f masks (f // Wb + crop, f % Wb + crop).
"""
import numpy as np

CROP, KSIZE, K_LOW, K_HIGH, RADIUS = 3, 5, 1.5, 2.0, 15


def normalise(img):
    x = np.asarray(img, dtype=np.float32)
    fin = np.isfinite(x)
    u = np.zeros(x.shape, dtype=np.uint8)
    if not fin.any():
        return u
    lo, hi = float(x[fin].min()), float(x[fin].max())
    if hi - lo <= np.finfo(np.float64).eps:
        return u
    s = 255.0 / (hi - lo)
    a, b = np.float32(s), np.float32(-lo * s)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint((x * a).astype(np.float32) + b)
    v = np.where(np.isnan(v), 0.0, np.clip(v, 0.0, 255.0))
    return v.astype(np.uint8)


def reflect101(p, n):
    """cv2::borderInterpolate(p, n, BORDER_REFLECT_101) for an integer array p."""
    p = np.array(p, dtype=np.int64)
    if n == 1:
        return np.zeros_like(p)
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))


def blur(u, crop=CROP, ksize=KSIZE):
    H, W = u.shape
    c = u[crop:H - crop, crop:W - crop]
    Hb, Wb = c.shape
    h = ksize // 2
    P = c[reflect101(np.arange(-h, Hb + h), Hb)][:, reflect101(np.arange(-h, Wb + h), Wb)].astype(np.int32)
    rows = sum(P[:, dx:dx + Wb] for dx in range(ksize))          # separable: exact integer sums
    acc = sum(rows[dy:dy + Hb] for dy in range(ksize))
    kk = ksize * ksize
    return ((acc + kk // 2) // kk).astype(np.uint8)


def thresholds(u, k_low=K_LOW, k_high=K_HIGH):
    avg, std = np.mean(u), np.std(u)
    return avg - std * k_low, avg + std * k_high


def seeds(img, crop=CROP, ksize=KSIZE, k_low=K_LOW, k_high=K_HIGH):
    u = normalise(img)
    lo, hi = thresholds(u, k_low, k_high)
    b = blur(u, crop, ksize)
    return (b < lo) | (b > hi)


def disk(r=RADIUS):
    ii, jj = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1))
    keep = ii ** 2 + jj ** 2 <= r * r
    return ii[keep], jj[keep]


def contam_set_literal(img, crop=CROP, ksize=KSIZE, k_low=K_LOW, k_high=K_HIGH, r=RADIUS):
    """The reference's set as a sorted int64 array: clip(i+di, 0, Hb) * Wb + clip(j+dj, 0, Wb) over seeds x disk."""
    S = seeds(img, crop, ksize, k_low, k_high)
    Hb, Wb = S.shape
    si, sj = np.nonzero(S)
    out = np.zeros((Hb + 1) * Wb + 1, dtype=bool)
    for di, dj in zip(*disk(r)):
        out[np.clip(si + di, 0, Hb) * Wb + np.clip(sj + dj, 0, Wb)] = True
    return np.flatnonzero(out)


def _hdilate(rowbits, w):
    """rows of a bool array [n, m] dilated horizontally by w (a 1-D window of 2w+1), via prefix sums."""
    n, m = rowbits.shape
    cs = np.zeros((n, m + 2 * w + 1), dtype=np.int32)
    np.cumsum(rowbits, axis=1, dtype=np.int32, out=cs[:, w + 1:w + 1 + m])
    cs[:, w + 1 + m:] = cs[:, w + m:w + m + 1]
    return cs[:, 2 * w + 1:] > cs[:, :m]


def contam_set_bitmap(img, crop=CROP, ksize=KSIZE, k_low=K_LOW, k_high=K_HIGH, r=RADIUS):
    """bool[(Hb+1)*Wb + 1]: True at every index of the reference's set."""
    S = seeds(img, crop, ksize, k_low, k_high)
    Hb, Wb = S.shape
    E = np.zeros((Hb + 1 + 2 * r, Wb + 1), dtype=bool)       # seeds on the extended grid, r zero rows above and below
    E[r:r + Hb, :Wb] = S
    D = np.zeros((Hb + 1, Wb + 1), dtype=bool)
    for di in range(-r, r + 1):
        w = int(np.floor(np.sqrt(r * r - di * di)))
        while (w + 1) ** 2 + di * di <= r * r:
            w += 1
        while w * w + di * di > r * r:
            w -= 1
        D |= _hdilate(E[r + di:r + di + Hb + 1], w)
    out = np.zeros((Hb + 1) * Wb + 1, dtype=bool)
    out[:(Hb + 1) * Wb] = D[:, :Wb].ravel()
    # the virtual column x = Wb is the flat index (y+1)*Wb: column 0 of the next row
    out[Wb::Wb] |= D[:, Wb]
    return out


def score_mask(bitmap, H, W, crop=CROP):
    """bitmap of the set -> bool [H, W] in the score map's frame."""
    Hb, Wb = H - 2 * crop, W - 2 * crop
    f = np.flatnonzero(bitmap)
    m = np.zeros((H, W), dtype=bool)
    m[f // Wb + crop, f % Wb + crop] = True
    return m


def contam_mask(img, **kw):
    H, W = np.asarray(img).shape
    return score_mask(contam_set_bitmap(img, **kw), H, W, kw.get("crop", CROP))
