"""NumPy model of the percentile clip of the micrograph ingest (sprk_ingest_clip, include/sprk.h) and
the images its tests share.  The selection follows the device's scheme step by step — relative keys, three passes of at
most 11 bits from the highest set bit of the span down, a histogram, a scan and a pick per pass — so that it can be
checked here against a plain sort; the GPU tests then compare the kernels with it bit for bit."""
import numpy as np

PASSES, DIGIT = 3, 11


def key(x):
    """float32 -> uint32, order-preserving (enc of csrc/ingest.hip): -0.0 sorts before +0.0"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def digits(span, p):
    """-> (top, shift) of pass p: it takes bits [shift, top) of the relative key"""
    nbits = int(span).bit_length()
    top = max(nbits - DIGIT * p, 0)
    return top, max(top - DIGIT, 0)


def radix_select(keys, k):
    """The element of the uint32 array ``keys`` with the k-th smallest value (from 0), by the device's passes."""
    keys = np.asarray(keys, dtype=np.uint32).ravel()
    kmin = int(keys.min())
    d = keys.astype(np.int64) - kmin
    span = int(d.max())
    prefix, k = 0, int(k)
    for p in range(PASSES):
        top, shift = digits(span, p)
        if top == shift:
            continue
        live = (d >> top) == prefix
        hist = np.bincount((d[live] >> shift) & ((1 << (top - shift)) - 1), minlength=1 << DIGIT)
        below = np.cumsum(hist) - hist
        b = int(np.searchsorted(below + hist, k, side="right"))          # the bin with below <= k < below + count
        prefix, k = (prefix << (top - shift)) | b, k - int(below[b])
    assert digits(span, PASSES - 1)[1] == 0
    return np.uint32(kmin + prefix)


def order_statistics(img, k_lo, k_hi):
    keys = key(np.asarray(img, dtype=np.float32).ravel())
    assert 0 <= k_lo <= k_hi <= keys.size - 1
    return unkey(radix_select(keys, k_lo))[()], unkey(radix_select(keys, k_hi))[()]


def clamp(img, lo, hi):
    """x < lo ? lo : (x > hi ? hi : x) in float comparisons: signed zeros are left alone"""
    x = np.asarray(img, dtype=np.float32)
    return np.where(x < lo, np.float32(lo), np.where(x > hi, np.float32(hi), x)).astype(np.float32)


def clip(img, k_lo, k_hi):
    """-> (clamped image, float32 [2] = (lo, hi))"""
    lo, hi = order_statistics(img, k_lo, k_hi)
    return clamp(img, lo, hi), np.array([lo, hi], dtype=np.float32)


def outlier_image(shape, seed=0):
    """N(100, 5) float32 with 5 samples at 30000, 3 at -500, one -0.0 and one +0.0"""
    rng = np.random.RandomState(seed)
    img = (100.0 + 5.0 * rng.randn(*shape)).astype(np.float32)
    at = rng.choice(img.size, 10, replace=False)
    flat = img.reshape(-1)
    flat[at[:5]], flat[at[5:8]], flat[at[8]], flat[at[9]] = 30000.0, -500.0, -0.0, 0.0
    return img


def pass_images(seed=3):
    """Three 64 x 64 images, one per way the span of keys can lie: values that differ only in the lowest 10 key bits;
    integers m * 2^e (m in 4..7) whose keys differ only from bit 21 up; a mix over the whole float range."""
    rng = np.random.RandomState(seed)
    low = (np.float32(1.0) + rng.randint(0, 1024, size=(64, 64)) * np.float32(2.0 ** -23)).astype(np.float32)
    high = (rng.randint(4, 8, size=(64, 64)) * 2.0 ** rng.randint(0, 61, size=(64, 64))).astype(np.float32)
    mix = (rng.randn(64, 64) * np.exp(rng.uniform(-40, 40, size=(64, 64)))).astype(np.float32)
    assert int(np.ptp(key(low).astype(np.int64))) < 1024 and not np.any(key(high) & np.uint32((1 << 21) - 1))
    return {"low bits": low, "high bits": high, "full range": mix}


def levels(u8):
    return int(np.unique(u8).size)
