"""NumPy model of the scores of the 2-D Thon-ring fit (csrc/ctffit.hip, include/sprk.h: sprk_ctf_score), the
oracle of tests/test_ctf2d_cpu.py and tests/test_gpu_ctf2d.py and the ``sums`` a test without a GPU hands to
``spr_pick_amd.ctf.fit_astigmatism``.

bins float32 [5, n]: rows b, p, q, r, Y; cand float32 [ncand, 3]: (d0, e1, e2).  Per bin and candidate
  t  = fma(r, e2, fma(q, e1, fma(p, d0, b)))   in float32, bit for bit the device's chain (``psd_model.fma``);
  c* = cos(2 pi t)                             in float64 (the device's float32 cosine lies within EPS of it);
  S1 = sum c*, S2 = sum c*^2, S3 = sum Y c*    in float64 over the bins.
The device differs from these sums by no more than ``bound``: its cosine error, and the roundings of two float64 sums of n
terms each (the device's, in its own fixed order, and NumPy's pairwise one)."""
import numpy as np

from psd_model import fma

EPS = 2.0 ** -22                                 # |cospif(2 t) - cos(2 pi t)| in float32: 4 ulp of a value of at most 1
MAX_BINS, MAX_CAND = 1 << 20, 1 << 24
BLOCK = 1 << 22                                  # bin x candidate pairs evaluated at a time


def phase(bins, cand):
    """-> t float32 [ncand, n]"""
    assert bins.dtype == cand.dtype == np.float32 and bins.ndim == 2 and bins.shape[0] == 5 and cand.ndim == 2 and cand.shape[1] == 3
    b, p, q, r = (bins[k][None, :] for k in range(4))
    # the inner links of the chain depend on d0, and on (d0, e1), alone: on a grid they are shared by many candidates and
    # are evaluated once per distinct value (an elementwise function gives the same bits either way)
    u1, i1 = np.unique(cand[:, 0], return_inverse=True)
    t1 = fma(p, u1[:, None], np.broadcast_to(b, (len(u1), bins.shape[1])))
    u2, i2 = np.unique(np.stack([i1.ravel().astype(np.float32), cand[:, 1]], axis=1), axis=0, return_inverse=True)
    t2 = fma(q, u2[:, 1:2], t1[u2[:, 0].astype(np.int64)])
    t = fma(r, cand[:, 2:3], t2[i2.ravel()])
    assert t.dtype == np.float32 and t.shape == (len(cand), bins.shape[1])
    return t


def sums(bins, cand):
    """-> S float64 [ncand, 3]"""
    bins, cand = np.ascontiguousarray(bins), np.ascontiguousarray(cand)
    n, ncand = bins.shape[1], cand.shape[0]
    assert 1 <= n <= MAX_BINS and 1 <= ncand <= MAX_CAND
    Y = bins[4].astype(np.float64)
    S = np.empty((ncand, 3))
    step = max(1, BLOCK // n)
    for c0 in range(0, ncand, step):
        c = np.cos(2.0 * np.pi * phase(bins, cand[c0:c0 + step]).astype(np.float64))
        S[c0:c0 + step, 0] = c.sum(axis=1)
        S[c0:c0 + step, 1] = (c * c).sum(axis=1)
        S[c0:c0 + step, 2] = c @ Y
    return S


def bound(bins):
    """-> float64 [3]: the a-priori bound of |S - S*| for S1, S2, S3.  With |c - c*| <= EPS per term: n EPS, n (2 EPS +
    EPS^2) and EPS sum |Y|; gamma = n^2 2^-53 covers the roundings of both float64 sums (each partial sum is at most n, max
    |Y| n for S3, and is rounded to within 2^-53 of itself, n times over, on either side)."""
    n = bins.shape[1]
    Y = np.abs(bins[4].astype(np.float64))
    gamma = float(n) ** 2 * 2.0 ** -53
    return np.array([n * EPS + gamma, n * (2 * EPS + EPS * EPS) + gamma, EPS * Y.sum() + gamma * Y.max()])


def check(S, bins, cand, want=None):
    """the device's S within ``bound`` of the model's -> worst error / bound of the three sums"""
    want = sums(bins, cand) if want is None else want
    assert S.shape == want.shape and S.dtype == np.float64
    bd = bound(bins)
    err = np.abs(S - want).max(axis=0)
    ratio = err / np.maximum(bd, 1e-300)
    assert np.isfinite(S).all() and (err <= bd).all(), (err, bd)
    return ratio
