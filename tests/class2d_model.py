"""NumPy models of reference-free 2-D classification (csrc/class2d.hip, include/sprk.h: sprk_class_transform / _score /
_average, spr_pick_amd/class2d.py), the oracle of tests/test_class2d_cpu.py and tests/test_gpu_class2d.py.

The three device contracts on ``fma32`` (one float32 rounding per fmaf, every other operation one float32 rounding):
  transform:  out(i, j) = the bilinear sample of src at the rotated position plus an integer shift, zero beyond the edges,
              then the mask and the normalisation with their fp64 sums in the device's order (``tree_sum``);
  score:      s[n, m] = chain from 0 over d ascending of Q[n, d] * B[m, d]; the lowest index of the maximum;
  average:    the fp32 add chain over a class's members in list order, times float32(1) / float32(count).

The whole loop in float64 (``classify64``), written independently of spr_pick_amd.class2d: plain ``@`` for the scores, FFTs
for the shift search, the same schedule.  ``planted`` makes the data both are judged on."""
import functools

import numpy as np

from extract_scale_model import fma32

MASK, NORMALIZE = 1, 2
THREADS = 256
f32 = np.float32


def angle_table(A_n):
    a = 2.0 * np.pi * np.arange(A_n, dtype=np.float64) / A_n
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(f32)


def mask_of(S, radius):
    c = S // 2
    i, j = np.mgrid[0:S, 0:S]
    return (i - c) ** 2 + (j - c) ** 2 <= radius * radius


def packed_pixels(S, radius):
    return np.flatnonzero(mask_of(S, radius).ravel()).astype(np.int32)


# ---- the rigid transform -------------------------------------------------------------------------------------------------
def value(img, ct, st, dy, dx):
    """img float32 [S, S]; ct, st float32 -> the transform value at every pixel, float32 [S, S]"""
    S = img.shape[0]
    c = S // 2
    assert img.dtype == f32 and img.shape == (S, S)
    ct, st = np.asarray(ct, dtype=f32), np.asarray(st, dtype=f32)
    y = np.broadcast_to((np.arange(S) - c).astype(f32)[:, None], (S, S))
    x = np.broadcast_to((np.arange(S) - c).astype(f32)[None, :], (S, S))
    u = fma32(ct, y, -(st * x))
    v = fma32(st, y, ct * x)
    fu, fv = np.floor(u), np.floor(v)
    tu, tv = u - fu, v - fv
    i0, j0 = fu.astype(np.int64) + c + dy, fv.astype(np.int64) + c + dx

    def tap(i, j):
        ok = (i >= 0) & (i < S) & (j >= 0) & (j < S)
        return np.where(ok, img[np.clip(i, 0, S - 1), np.clip(j, 0, S - 1)], f32(0))

    r = [fma32(tv, tap(i0 + a, j0 + 1), (f32(1) - tv) * tap(i0 + a, j0)) for a in (0, 1)]
    return fma32(tu, r[1], (f32(1) - tu) * r[0])


def tree_sum(v):
    """float64 [n] in linear pixel order -> the device's sum: 256 strided partials, each ascending, then a halving tree"""
    n = -(-len(v) // THREADS) * THREADS
    rows = np.concatenate([v, np.zeros(n - len(v))]).reshape(-1, THREADS)
    part = np.zeros(THREADS)
    for row in rows:
        part = part + row
    h = THREADS // 2
    while h:
        part[:h] = part[:h] + part[h:2 * h]
        h //= 2
    return part[0]


def finish(v, radius, flags):
    """the mask and the normalisation of one transformed image"""
    S = v.shape[0]
    if not flags:
        return v
    inside = mask_of(S, radius)
    v = np.where(inside, v, f32(0))
    if not flags & NORMALIZE:
        return v
    count = int(inside.sum())
    if count == 0:
        return np.zeros_like(v)
    mean = f32(tree_sum(v.ravel().astype(np.float64)) / float(count))
    w = np.where(inside, v - mean, f32(0)).astype(f32)
    norm = np.sqrt(f32(tree_sum(w.ravel().astype(np.float64) ** 2)))
    if not norm > 0:
        return np.zeros_like(v)
    return (w / norm).astype(f32)


def transform(src, idx, ang, shift, cs, radius=0, flags=0, pix=None, ldo=None):
    """-> float32 [M, S, S], or with pix the packed [M, ldo]"""
    out = np.stack([finish(value(src[idx[m]], cs[ang[m], 0], cs[ang[m], 1], int(shift[m][0]), int(shift[m][1])), radius, flags)
                    for m in range(len(idx))])
    if pix is None:
        return out
    packed = np.zeros((len(idx), ldo), dtype=f32)
    packed[:, :len(pix)] = out.reshape(len(idx), -1)[:, pix]
    return packed


def shifted_copy(img, dy, dx):
    """out[i, j] = img[i + dy, j + dx], zeros beyond the edges"""
    S = img.shape[0]
    out = np.zeros_like(img)
    i0, i1 = max(0, -dy), min(S, S - dy)
    j0, j1 = max(0, -dx), min(S, S - dx)
    if i0 < i1 and j0 < j1:
        out[i0:i1, j0:j1] = img[i0 + dy:i1 + dy, j0 + dx:j1 + dx]
    return out


# ---- the scores ------------------------------------------------------------------------------------------------------------
def score(Q, B, D):
    """Q float32 [N, >= D], B float32 [Mb, >= D] -> s float32 [N, Mb]"""
    s = np.zeros((Q.shape[0], B.shape[0]), dtype=f32)
    for d in range(D):
        s = fma32(Q[:, d:d + 1], B[None, :, d], s)
    return s


def best(s):
    """-> (best_score float32 [N], best_index int32 [N]): the lowest index of the maximum"""
    i = np.argmax(s, axis=1)                                     # the first occurrence
    return s[np.arange(len(s)), i], i.astype(np.int32)


# ---- the class sums ----------------------------------------------------------------------------------------------------------
def average(src, ang, shift, cs, members, offsets, out):
    """out float32 [K, S, S] is updated in place as the device does: an empty class keeps what it holds"""
    for k in range(len(offsets) - 1):
        mem = members[offsets[k]:offsets[k + 1]]
        if not len(mem):
            continue
        s = np.zeros(src.shape[1:], dtype=f32)
        for p in mem:
            s = s + value(src[p], cs[ang[p], 0], cs[ang[p], 1], int(shift[p][0]), int(shift[p][1]))
        out[k] = s * (f32(1) / f32(len(mem)))
    return out


# ---- planted data ------------------------------------------------------------------------------------------------------------
def _shape(kind, S, theta):
    """one of three shapes rotated by theta about the centre, float64 [S, S]"""
    c = S // 2
    i, j = np.mgrid[0:S, 0:S]
    y, x = (i - c).astype(np.float64), (j - c).astype(np.float64)
    ct, st = np.cos(theta), np.sin(theta)
    yr, xr = ct * y - st * x, st * y + ct * x                    # the frame of the shape
    sig = S / 20.0

    def blob(cy, cx):
        return np.exp(-((yr - cy) ** 2 + (xr - cx) ** 2) / (2 * sig * sig))

    step = S / 8.0
    if kind == 0:                                                # a bar
        return np.exp(-(yr / (S / 5.0)) ** 2 / 2 - (xr / sig) ** 2 / 2)
    if kind == 1:                                                # a triangle of three blobs
        r = S / 5.0
        return sum(blob(r * np.cos(t), r * np.sin(t)) for t in (0.0, 2 * np.pi / 3, 4 * np.pi / 3))
    pts = [(-2, 0), (-1, 0), (0, 0), (0, 1), (0, 2)]             # an L of five blobs, its centre of mass at the centre
    my, mx = np.mean([p[0] for p in pts]), np.mean([p[1] for p in pts])
    return sum(blob((p[0] - my) * step, (p[1] - mx) * step) for p in pts)


def unit_shape(kind, S, theta, radius):
    """the shape with zero mean and unit standard deviation under the mask"""
    inside = mask_of(S, radius)
    s = _shape(kind, S, theta)
    return (s - s[inside].mean()) / s[inside].std()


def planted(S, N, seed, noise, R=3, kinds=3):
    """-> (P float32 [N, S, S], labels [N]): each particle one of the shapes at a random rotation and integer shift within
    +-R, plus Gaussian noise of ``noise`` times the signal's standard deviation under the mask"""
    rng = np.random.default_rng(seed)
    radius = S // 2 - R - 2
    labels = rng.integers(0, kinds, N)
    P = np.empty((N, S, S), dtype=f32)
    for n in range(N):
        s = unit_shape(labels[n], S, rng.uniform(0, 2 * np.pi), radius)
        dy, dx = rng.integers(-R, R + 1, 2)
        P[n] = (np.roll(s, (dy, dx), (0, 1)) + noise * rng.standard_normal((S, S))).astype(f32)
    return P, labels


def purity(cls, labels, K):
    return sum(np.bincount(labels[cls == k]).max() for k in range(K) if (cls == k).any()) / float(len(labels))


# ---- the whole loop in float64 -----------------------------------------------------------------------------------------------
def rigid64(imgs, ct, st, dy, dx):
    """imgs float64 [M, S, S] with one angle (ct, st [M]) and one shift (dy, dx [M]) each -> [M, S, S]"""
    M, S, _ = imgs.shape
    c = S // 2
    y = (np.arange(S) - c)[None, :, None].astype(np.float64)
    x = (np.arange(S) - c)[None, None, :].astype(np.float64)
    ct, st = ct[:, None, None], st[:, None, None]
    u, v = ct * y - st * x, st * y + ct * x
    fu, fv = np.floor(u), np.floor(v)
    tu, tv = u - fu, v - fv
    i0 = fu.astype(np.int64) + c + dy[:, None, None]
    j0 = fv.astype(np.int64) + c + dx[:, None, None]
    # a border of zeros two pixels wide: taps beyond the edges are clipped into it
    Sp = S + 4
    flat = np.pad(imgs, ((0, 0), (2, 2), (2, 2))).ravel()
    i0, j0 = np.clip(i0, -2, S) + 2, np.clip(j0, -2, S) + 2
    base = (np.arange(M)[:, None, None] * Sp + i0) * Sp + j0
    r0 = tv * flat.take(base + 1) + (1 - tv) * flat.take(base)
    r1 = tv * flat.take(base + Sp + 1) + (1 - tv) * flat.take(base + Sp)
    return tu * r1 + (1 - tu) * r0


def split_classes(cls, scores, Kc, K):
    """the divisive step: the min(Kc, K - Kc) largest classes (ties by a stable sort) are split at the median score"""
    cls = cls.copy()
    sizes = np.bincount(cls, minlength=Kc)
    order = np.argsort(-sizes, kind="stable")[:min(Kc, K - Kc)]
    parents = []
    for t, k in enumerate(order):
        mem = np.flatnonzero(cls == k)
        if len(mem):
            cls[mem[scores[mem] < np.median(scores[mem])]] = Kc + t
        parents.append(int(k))
    return cls, parents


def classify64(P, K, A_n=72, R=3, radius=None, iters=8):
    """-> dict(cls, ang, shift [N, 2], scores, averages float64 [K, S, S], levels [(Kc, iterations)])"""
    N, S, _ = P.shape
    P = P.astype(np.float64)
    radius = S // 2 - R - 2 if radius is None else radius
    inside = mask_of(S, radius)
    pix = np.flatnonzero(inside.ravel())
    a = 2.0 * np.pi * np.arange(A_n) / A_n
    cos, sin = np.cos(a), np.sin(a)
    cls, ang, sh = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros((N, 2), np.int64)
    FP = np.fft.rfft2(P)

    def averages_of(prev, Kc):
        out = prev.copy()
        inv = (A_n - ang) % A_n
        aligned = rigid64(P, cos[inv], sin[inv], sh[:, 0], sh[:, 1])
        for k in range(Kc):
            if (cls == k).any():
                out[k] = aligned[cls == k].mean(axis=0)
        return out

    avgs = P.mean(axis=0)[None]
    Kc, levels, scores = 1, [], np.zeros(N)
    while True:
        used = 0
        for it in range(iters):
            used = it + 1
            kk, aa = np.repeat(np.arange(Kc), A_n), np.tile(np.arange(A_n), Kc)
            bank = rigid64(avgs[kk], cos[aa], sin[aa], np.zeros(Kc * A_n, np.int64), np.zeros(Kc * A_n, np.int64))
            bank = np.where(inside, bank, 0.0)
            bank = np.where(inside, bank - bank.reshape(len(bank), -1)[:, pix].mean(axis=1)[:, None, None], 0.0)
            norm = np.sqrt((bank ** 2).sum(axis=(1, 2)))
            bank = np.where(norm[:, None, None] > 0, bank / np.where(norm > 0, norm, 1.0)[:, None, None], 0.0)
            Q = rigid64(P, np.ones(N), np.zeros(N), sh[:, 0], sh[:, 1]).reshape(N, -1)[:, pix]
            s = Q @ bank.reshape(len(bank), -1)[:, pix].T
            bi = np.argmax(s, axis=1)
            scores = s[np.arange(N), bi]
            new_cls, new_ang = bi // A_n, bi % A_n
            # cc[di, dj] = sum over p of P[p - d] * ref[p], periodic: the peak says which shifted particle fits its reference
            cc = np.fft.irfft2(np.conj(FP) * np.fft.rfft2(bank[bi]), s=(S, S))
            d = np.arange(-R, R + 1)
            win = cc[:, d[:, None] % S, d[None, :] % S].reshape(N, -1)
            peak = np.argmax(win, axis=1)
            new_sh = np.stack([-(peak // (2 * R + 1) - R), -(peak % (2 * R + 1) - R)], axis=1)
            same = (new_cls == cls).all() and (new_ang == ang).all() and (new_sh == sh).all()
            cls, ang, sh = new_cls, new_ang, new_sh
            avgs = averages_of(avgs, Kc)
            if same and used >= 2:
                break
        levels.append((Kc, used))
        if Kc >= K:
            break
        cls, parents = split_classes(cls, scores, Kc, K)
        avgs = np.concatenate([avgs, avgs[parents]])
        Kc += len(parents)
        avgs = averages_of(avgs, Kc)
    return {"cls": cls, "ang": ang, "shift": sh, "scores": scores, "averages": avgs, "levels": levels}


# the cases of the planted-data tests: S, N, K, A_n, R, and (noise, seed) pairs chosen so that the float64 model alone
# reaches the purity line of tests/test_class2d_cpu.py
CASE = {"S": 64, "N": 300, "K": 3, "A_n": 36, "R": 3, "iters": 8}
CASES = [(1.0, 1), (1.0, 2), (1.0, 3), (2.0, 1), (2.0, 2), (2.0, 3)]


@functools.lru_cache(maxsize=None)
def planted_case(noise, seed):
    """-> (P, labels, the float64 model's result); computed once and shared, never modified"""
    P, labels = planted(CASE["S"], CASE["N"], seed, noise, CASE["R"])
    res = classify64(P, CASE["K"], CASE["A_n"], CASE["R"], None, CASE["iters"])
    P.setflags(write=False)
    return P, labels, res

