"""NumPy models of the Wiener-weighted class averages (csrc/classctf.hip, include/sprk.h: sprk_class_spectrum / _wiener /
_synthesize, spr_pick_amd/class2d.py with ``ctf=``), the oracle of tests/test_classctf_cpu.py and
tests/test_gpu_classctf.py.

The three device contracts on fmaf chains (``extract_filter_model.chain``: one float32 rounding per step, from 0, K ascending),
h = S/2, Hs = h + 1, Ku = S + 1, W the four float32 matrices of ``spr_pick_amd.extract.filter_matrices(S, S)``:
  spectrum:    U = chain(img, W1^T);  V = [U[:, :Hs] ; U[:, Hs:]];  spec = chain(W2, V)                 [2Ku, Hs]: Re over Im
  wiener:      nr = fma(wn[g_m], Re_m, nr), ni likewise, d = d + wd[g_m] over the members in list order from 0;
               out = nr / (d + tau), ni / (d + tau)                                                  [2Ku, Hs]
  synthesize:  Zs = chain(W3, f);  Z = [Zs[:S], Zs[S:]];  out = chain(Z, W4^T)                          [S, S]
The model's arrays have Hs columns; the device's have roundup(Hs, 4), the added ones written and read by nobody.

``wiener64`` is the same estimate in float64 with the float64 matrices, ``apriori_bound`` what the float32 path may differ
from it by.  ``classify64`` is ``class2d_model.classify64`` with Wiener averages by plain FFTs over the full plane, written
independently of the device's half-plane layout; ``planted`` and ``one_class`` make the data both are judged on."""
import functools

import numpy as np

import class2d_model
from extract_filter_model import AC, CS, EPS, KV, chain, correlation, plane_ctf  # noqa: F401
from psd_model import fma

f32 = np.float32


def geometry(S):
    """-> (Hs, Ku, ldv)"""
    return S // 2 + 1, S + 1, (S // 2 + 1 + 3) & ~3


# ---- the three contracts ------------------------------------------------------------------------------------------------------
def spectrum(img, W):
    """img float32 [S, S] -> spec float32 [2Ku, Hs]"""
    W1, W2 = W[0], W[1]
    S = img.shape[0]
    Hs, Ku, _ = geometry(S)
    assert img.dtype == f32 and img.shape == (S, S) and W1.shape == (2 * Hs, S) and W2.shape == (2 * Ku, 2 * S)
    U = chain(img, np.ascontiguousarray(W1.T))
    return chain(W2, np.concatenate([U[:, :Hs], U[:, Hs:]]))


def wiener(spec, wn, wd, group, members, offsets, tau, out):
    """spec float32 [n, 2Ku, Hs]; wn, wd float32 [G, Ku, Hs]; out float32 [K, 2Ku, Hs] is updated in place as the device does:
    an empty class keeps what it holds; members, groups and offsets are clamped into their arrays"""
    n, G, N, Ku = len(spec), len(wn), len(members), wn.shape[1]
    tau = f32(tau)
    assert spec.dtype == wn.dtype == wd.dtype == out.dtype == f32
    for k in range(len(offsets) - 1):
        beg, end = (int(np.clip(offsets[k + j], 0, N)) for j in (0, 1))
        if end <= beg:
            continue
        nr, ni, d = (np.zeros(wn.shape[1:], dtype=f32) for _ in range(3))
        for m in members[beg:end]:
            m = int(np.clip(m, 0, n - 1))
            g = int(np.clip(group[m], 0, G - 1))
            nr = fma(wn[g], spec[m, :Ku], nr)
            ni = fma(wn[g], spec[m, Ku:], ni)
            d = d + wd[g]
        den = d + tau
        assert nr.dtype == ni.dtype == den.dtype == f32
        out[k, :Ku], out[k, Ku:] = nr / den, ni / den
    return out


def synthesize(f, W):
    """f float32 [2Ku, Hs] -> float32 [S, S]"""
    W3, W4 = W[2], W[3]
    S = W4.shape[0]
    assert f.dtype == f32 and f.shape == (2 * (S + 1), S // 2 + 1)
    Zs = chain(W3, f)
    return chain(np.concatenate([Zs[:S], Zs[S:]], axis=1), np.ascontiguousarray(W4.T))


# ---- float64 and the a-priori bound ---------------------------------------------------------------------------------------------
def spectrum64(img, W64):
    Hs = W64[0].shape[0] // 2
    U = np.asarray(img, dtype=np.float64) @ W64[0].T
    return W64[1] @ np.concatenate([U[:, :Hs], U[:, Hs:]])


def synthesize64(f, W64):
    S = W64[3].shape[0]
    Zs = W64[2] @ f
    return np.concatenate([Zs[:S], Zs[S:]], axis=1) @ W64[3].T


def wiener64(imgs, W64, wn, wd, group, members, tau):
    """one class: IDFT(sum wn DFT(y) / (sum wd + tau)) in float64 over the members (a list of image indices) -> [S, S]"""
    num = sum(np.concatenate([wn[group[m]], wn[group[m]]]).astype(np.float64) * spectrum64(imgs[m], W64) for m in members)
    den = sum(wd[group[m]].astype(np.float64) for m in members) + float(tau)
    return synthesize64(num / np.concatenate([den, den]), W64)


def apriori_bound(imgs, W, wn, wd, group, members, tau):
    """-> (reference float64 [S, S], bound [S, S]) for one class of the float32 operands, in the form of
    ``extract_filter_model.apriori_bound``: |A - ref| <= (S + 2S + 2 count + 2 + 2Ku + 2Hs + 8) 2^-24 times
    |W4| |W3| (sum wn |W2| |W1| |y|) / (sum wd + tau), the stages composed as ``wiener64`` composes them.  The four chains
    of S, 2S, 2Ku and 2Hs roundings are each within 2^-24 relative of their partial sums of absolute values; the numerator is
    a chain of `count` fmaf over products of what stage 2 left; the denominator is a sum of `count` non-negative terms and tau
    (every partial sum within 2^-24 relative, no cancellation) and the quotient one rounding more: count + 2; 8 of slack for
    the second-order terms."""
    S, count = W[3].shape[0], len(members)
    W64 = [m.astype(np.float64) for m in W]
    ref = wiener64(imgs, W64, wn, wd, group, members, tau)
    absolute = wiener64(np.abs(imgs), [np.abs(m) for m in W64], np.abs(wn), wd, group, members, tau)
    return ref, (S + 2 * S + 2 * count + 2 + 2 * (S + 1) + 2 * (S // 2 + 1) + 8) * EPS * absolute


def stage_bounds(img, W):
    """the spectrum and the synthesis alone against float64, each in the same form -> [(got, ref, bound), ...]: the chains
    of S and 2S roundings, then those of 2Ku and 2Hs on the float32 spectrum the first pair gave"""
    S = img.shape[0]
    W64, A64 = [m.astype(np.float64) for m in W], [np.abs(m.astype(np.float64)) for m in W]
    spec = spectrum(img, W)
    first = (spec, spectrum64(img, W64), (S + 2 * S + 4) * EPS * spectrum64(np.abs(img), A64))
    second = (synthesize(spec, W), synthesize64(spec.astype(np.float64), W64),
              (2 * (S + 1) + 2 * (S // 2 + 1) + 4) * EPS * synthesize64(np.abs(spec).astype(np.float64), A64))
    return [first, second]


# ---- planted data ---------------------------------------------------------------------------------------------------------------
APIX = 4.0
DEFOCI = np.linspace(8000.0, 24000.0, 6)
MICROGRAPHS = len(DEFOCI)


def micrograph_rows(astigmatism=0.0):
    """-> float64 [6, 7]: (DefocusU, DefocusV, DefocusAngle, kV, Cs, Q, apix) of the six micrographs; with ``astigmatism`` =
    U - V the angles are mixed (25 degrees apart from 10)"""
    return np.array([(d + 0.5 * astigmatism, d - 0.5 * astigmatism, (10.0 + 25.0 * m) % 180.0 if astigmatism else 0.0, KV, CS,
                      AC, APIX) for m, d in enumerate(DEFOCI)])


def plane_abs_ctf(S, row):
    """|c| of one row on np.fft.fftfreq's full grid, float64 [S, S]"""
    return np.abs(plane_ctf(S, row[6], row[0], row[1], row[2]))


def through_ctf(img, absc):
    return np.fft.ifft2(absc * np.fft.fft2(img)).real


def planted(S, N, seed, noise, R=3, kinds=3, astigmatism=0.0):
    """``class2d_model.planted`` seen through the CTFs: the same draws in the same order (labels first; per particle the
    angle, the shift, then the noise field); the shifted shape is filtered by |c| of micrograph n mod 6 before the noise is
    added -> (P float32 [N, S, S], labels [N], micrograph [N], rows [6, 7])"""
    rng = np.random.default_rng(seed)
    radius = S // 2 - R - 2
    rows = micrograph_rows(astigmatism)
    absc = [plane_abs_ctf(S, row) for row in rows]
    labels = rng.integers(0, kinds, N)
    P = np.empty((N, S, S), dtype=f32)
    for n in range(N):
        s = class2d_model.unit_shape(labels[n], S, rng.uniform(0, 2 * np.pi), radius)
        dy, dx = rng.integers(-R, R + 1, 2)
        P[n] = (through_ctf(np.roll(s, (dy, dx), (0, 1)), absc[n % MICROGRAPHS]) + noise * rng.standard_normal((S, S))).astype(f32)
    return P, labels, np.arange(N) % MICROGRAPHS, rows


ONE_CLASS = {"S": 64, "N": 240, "radius": 27, "blobs": 12, "noise": 1.0, "seeds": (1, 2, 3)}


@functools.lru_cache(maxsize=None)
def one_class(seed, noise=ONE_CLASS["noise"]):
    """The fixed-assignment case: an object of 12 random Gaussian blobs (centres uniform in the square of +-S/4 about the
    centre, sigma 1.5 .. 3 pixels, amplitudes 0.5 .. 1.5), zero mean and unit standard deviation under the mask of radius 27,
    seen N = 240 times through |c| of micrograph n mod 6 at angle 0 and shift 0, plus ``noise`` times standard normal noise
    -> (P float32 [N, S, S], obj float64 [S, S], micrograph [N], rows [6, 7]); shared, never modified"""
    S, N = ONE_CLASS["S"], ONE_CLASS["N"]
    rng = np.random.default_rng(seed)
    i, j = np.mgrid[0:S, 0:S]
    obj = np.zeros((S, S))
    for _ in range(ONE_CLASS["blobs"]):
        cy, cx = S // 2 + rng.uniform(-S / 4, S / 4, 2)
        sig, amp = rng.uniform(1.5, 3.0), rng.uniform(0.5, 1.5)
        obj += amp * np.exp(-((i - cy) ** 2 + (j - cx) ** 2) / (2 * sig * sig))
    inside = class2d_model.mask_of(S, ONE_CLASS["radius"])
    obj = (obj - obj[inside].mean()) / obj[inside].std()
    rows = micrograph_rows()
    seen = [through_ctf(obj, plane_abs_ctf(S, row)) for row in rows]
    P = np.stack([seen[n % MICROGRAPHS] + noise * rng.standard_normal((S, S)) for n in range(N)]).astype(f32)
    P.setflags(write=False)
    return P, obj, np.arange(N) % MICROGRAPHS, rows


def masked_correlation(a, b, radius):
    inside = class2d_model.mask_of(a.shape[0], radius)
    return correlation(a[inside], b[inside])


def wiener_fft(Y, absc, wn_mode, tau):
    """float64, full plane: IDFT(sum wn DFT(y_i) / (sum c_i^2 + tau)); Y [M, S, S], absc [M, S, S] the members' |c|"""
    wn = absc if wn_mode == "flip" else np.ones_like(absc)
    return np.fft.ifft2((wn * np.fft.fft2(Y)).sum(axis=0) / ((absc * absc).sum(axis=0) + tau)).real


# ---- the whole loop in float64 --------------------------------------------------------------------------------------------------
def classify64(P, K, micrograph, rows, mode="flip", tau=1.0, A_n=72, R=3, radius=None, iters=8):
    """``class2d_model.classify64`` with every average a Wiener sum: the same schedule, scores, shift search and splits.
    A particle turned back by the angle index a has its CTF turned with it: |c| of its micrograph at DefocusAngle + 360 a /
    A_n (rows with U = V: one plane per micrograph)."""
    from class2d_model import mask_of, rigid64, split_classes
    N, S, _ = P.shape
    P = P.astype(np.float64)
    radius = S // 2 - R - 2 if radius is None else radius
    inside = mask_of(S, radius)
    pix = np.flatnonzero(inside.ravel())
    a = 2.0 * np.pi * np.arange(A_n) / A_n
    cos, sin = np.cos(a), np.sin(a)
    cls, ang, sh = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros((N, 2), np.int64)
    FP = np.fft.rfft2(P)
    planes = {}

    def plane(m, ai):
        row = rows[m]
        key = (m, ai if row[0] != row[1] else 0)
        if key not in planes:
            planes[key] = plane_abs_ctf(S, tuple(row[:2]) + (row[2] + 360.0 * key[1] / A_n,) + tuple(row[3:]))
        return planes[key]

    def averages_of(prev, Kc):
        out = prev.copy()
        inv = (A_n - ang) % A_n
        aligned = rigid64(P, cos[inv], sin[inv], sh[:, 0], sh[:, 1])
        for k in range(Kc):
            mem = np.flatnonzero(cls == k)
            if len(mem):
                out[k] = wiener_fft(aligned[mem], np.stack([plane(micrograph[n], inv[n]) for n in mem]), mode, tau)
        return out

    avgs = averages_of(np.zeros((1, S, S)), 1)
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


# the cases of the planted-data tests (DESIGN §4.3n lists every seed tried): (noise, seed, U - V)
CASE = class2d_model.CASE
CASES = [(0.5, 1, 0.0), (0.5, 3, 0.0), (0.25, 3, 0.0), (0.5, 1, 2000.0)]


@functools.lru_cache(maxsize=None)
def planted_case(noise, seed, astigmatism=0.0):
    """-> (P, labels, micrograph, rows, the float64 model's result with Wiener weighting); computed once and shared"""
    P, labels, mic, rows = planted(CASE["S"], CASE["N"], seed, noise, CASE["R"], astigmatism=astigmatism)
    res = classify64(P, CASE["K"], mic, rows, "flip", 1.0, CASE["A_n"], CASE["R"], None, CASE["iters"])
    P.setflags(write=False)
    return P, labels, mic, rows, res
