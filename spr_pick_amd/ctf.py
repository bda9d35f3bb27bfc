"""CTF estimation from raw micrographs: ``joint ctf`` writes, per micrograph, the summed power spectrum of
overlapping tiles and its radial profile, fits one defocus value to the Thon rings and collects the fits in
``micrographs_ctf.star`` — the columns 2-D classification needs next to the coordinates of ``joint extract`` (which joins
them into ``particles.star`` with ``--ctf``), and a screen for drifted or thick-ice micrographs before picking.

The device part is ``torch.ops.sprk.psd_tiles`` (csrc/psd.hip): a file's sample block uploaded once by
``ingest.read_raw``, T x T tiles at a step of T/2, each tile's half-plane DFT as two real fp32 GEMMs on MFMA with the
matrices of ``dft_matrices``, the squared magnitudes summed over the tiles in a fixed order.  The trailing margin of fewer
than T/2 samples on either axis is not covered; nothing is tapered and no mean is taken out, so the DC bin and its
nearest neighbours carry the image's offset and are not used.  Everything after that is NumPy float64 on the T x (T/2+1)
numbers of the spectrum and needs no GPU.

By default astigmatism is not fitted: the table carries DefocusU = DefocusV and an angle of 0.  With ``astigmatism=True``
(``joint ctf --astigmatism``) ``fit_astigmatism`` fits DefocusU, DefocusV and the angle to the 2-D spectrum
around the 1-D fit: the host prepares five numbers per bin (``fit_bins``) and the candidates, ``torch.ops.sprk.ctf_score``
(csrc/ctffit.hip) evaluates cos 2 chi of every bin for every candidate and returns three float64 sums each, and the host
turns them into a Pearson correlation (``score``).  Phase plates, per-particle defocus and CTF correction are out of
scope."""
import logging
import math
import os

import numpy as np
import torch

from . import _lib, fourier, ingest, micrograph_io, torch_ops

logger = logging.getLogger("joint.ctf")

CTF_STAR_COLUMNS = ("MicrographName", "DefocusU", "DefocusV", "DefocusAngle", "Voltage", "SphericalAberration",
                    "AmplitudeContrast", "Magnification", "DetectorPixelSize", "CtfFigureOfMerit")
CTF_STAR_HEADER = "# version 30001\n\ndata_\n\nloop_\n" + "".join("_rln%s #%d\n" % (c, k + 1)
                                                                   for k, c in enumerate(CTF_STAR_COLUMNS))
MAGNIFICATION = 10000.0                          # with it _rlnDetectorPixelSize (micrometres) is the pixel size in Angstrom
COARSE_STEP, FINE_STEP = 100.0, 5.0              # Angstrom: the two grids of fit_defocus
MAX_ASTIGMATISM = 1000.0                         # Angstrom: the default radius of fit_astigmatism's search in (e1, e2)
ASTIG_STEP, ASTIG_RANGE = 50.0, 500.0            # fit_astigmatism's coarse grid: the step of all three, the range of d0 - D_ref


# ---- the device part ---------------------------------------------------------------------------------------------------
def check_tile(T):
    """-> T or ValueError: a multiple of 16 in 16..1024"""
    if not isinstance(T, (int, np.integer)):
        raise ValueError("tile must be an integer, got %r" % (T,))
    try:
        return torch_ops.psd_tile(int(T))
    except _lib.SprkError as e:
        raise ValueError(str(e)) from None


def tile_geometry(ny, nx, T):
    """-> (ty, tx): rows and columns of tiles at a step of T/2; tile t = i*tx + j starts at (i*T/2, j*T/2)"""
    if ny < T or nx < T:
        raise ValueError("a %dx%d image is smaller than one tile of %d" % (ny, nx, T))
    return (ny - T) // (T // 2) + 1, (nx - T) // (T // 2) + 1


def dft_matrices64(T):
    """-> (W1 [2H, T], W2 [2T, 2T]) in float64, H = T/2 + 1.  W1: row v cos(2 pi ((v c) mod T) / T), row H+v the sine of
    the same angle.  W2 = [[C, -S], [S, C]] with C[u, r] = cos(2 pi ((u r) mod T) / T), S the sine.  The integer product is
    reduced mod T before the division, so the angle is as exact as float64 can hold it whatever the size."""
    T = check_tile(T)
    n = np.arange(T, dtype=np.int64)
    a2 = fourier.phase(n, n, T)
    C, S = np.cos(a2), np.sin(a2)
    return fourier.half_plane64(T // 2 + 1, T), np.block([[C, -S], [S, C]])


def dft_matrices(T, device=None):
    """``dft_matrices64`` rounded to float32.  Without a device: the two arrays.  With one: the operands of
    ``torch.ops.sprk.psd_tiles``, contiguous tensors [roundup(2H, 16), T] and [2T, 2T] on that device whose added rows
    are exact zeros (T is a multiple of 16, so no column is added), built once per (T, device)."""
    T = check_tile(T)
    return fourier.operands(dft_matrices64, (T,), torch_ops.psd_matrix_shapes(T), device)


def psd_sum(path_or_raw, tile, device="cuda", max_batch=0):
    """path_or_raw: an MRC file, or the ``(raw, header)`` pair ``ingest.read_raw`` returns for one.
    -> (P float32 CUDA [T, T/2 + 1], the un-normalised sum over the tiles; ntiles); nothing is synchronised."""
    T = check_tile(tile)
    if isinstance(path_or_raw, (str, os.PathLike)):
        raw, header = ingest.read_raw(os.fspath(path_or_raw), device)
    else:
        raw, header = path_or_raw
    if not raw.is_cuda:
        raise _lib.SprkError("the power spectrum runs on the GPU only (raw samples on %s)" % raw.device)
    ty, tx = tile_geometry(header.ny, header.nx, T)
    w1, w2 = dft_matrices(T, raw.device)
    return torch.ops.sprk.psd_tiles(raw, header.mode, header.ny, header.nx, T, w1, w2, int(max_batch)), ty * tx


def mean_power(P, ntiles, T):
    """the float64 mean power per tile and sample: P / (ntiles T^2)"""
    return np.asarray(P, dtype=np.float64) / (float(ntiles) * T * T)


def power_spectrum(path_or_raw, tile, device="cuda"):
    """-> the float64 mean power spectrum [T, T/2 + 1] of the micrograph's tiles: P / (ntiles T^2)"""
    P, ntiles = psd_sum(path_or_raw, tile, device)
    return mean_power(P.cpu().numpy(), ntiles, int(tile))


# ---- the host part: float64 on the spectrum ----------------------------------------------------------------------------
def radial_bins(T):
    """-> int64 [T, T/2 + 1]: the ring k = round(sqrt(u'^2 + v^2)) of every stored bin, u' the signed frequency of row u
    (u - T past T/2).  The rounding is decided in integers: k is the one with (2k - 1)^2 <= 4 r^2 < (2k + 1)^2."""
    u = np.arange(T, dtype=np.int64)
    u = np.where(u > T // 2, u - T, u)
    r4 = 4 * (u[:, None] ** 2 + np.arange(T // 2 + 1, dtype=np.int64)[None, :] ** 2)
    m = np.sqrt(r4.astype(np.float64)).astype(np.int64)          # floor(sqrt(4 r^2)), put right in integers below
    m -= (m * m > r4)
    m += ((m + 1) * (m + 1) <= r4)
    return (m + 1) // 2


def radial_profile(Pm):
    """Pm [T, T/2 + 1] -> float64 [T/2 + 1]: the mean of the stored (half-plane) bins of every ring k <= T/2, each stored
    bin counting once."""
    Pm = np.asarray(Pm, dtype=np.float64)
    T = Pm.shape[0]
    if Pm.ndim != 2 or T % 2 or Pm.shape[1] != T // 2 + 1:
        raise ValueError("a half-plane spectrum [T, T/2 + 1] is expected, got %s" % (Pm.shape,))
    k = radial_bins(T)
    keep = k <= T // 2
    count = np.bincount(k[keep], minlength=T // 2 + 1)
    return np.bincount(k[keep], weights=Pm[keep], minlength=T // 2 + 1) / count


def wavelength(kv):
    """the relativistic electron wavelength in Angstrom at kv kilovolts"""
    v = kv * 1e3
    return 12.2643247 / math.sqrt(v * (1.0 + 0.978466e-6 * v))


def ctf(s, defocus, kv, cs, ac):
    """CTF(s) = -sin(pi lambda dz s^2 - pi/2 Cs lambda^3 s^4 + atan2(ac, sqrt(1 - ac^2))); s in 1/Angstrom, dz in
    Angstrom (positive: underfocus), Cs in millimetres.  ``defocus`` may be an array [n, 1] against s [m]."""
    lam, cs = wavelength(kv), cs * 1e7
    s2 = np.asarray(s, dtype=np.float64) ** 2
    return -np.sin(np.pi * lam * defocus * s2 - 0.5 * np.pi * cs * lam ** 3 * s2 * s2 + math.atan2(ac, math.sqrt(1 - ac * ac)))


CORRECTION_MODES = ("flip", "multiply")


def correction_filter(B, S, apix, defocus_u, defocus_v, angle, kv, cs, ac, mode):
    """The filter of ``torch.ops.sprk.extract_filter`` for boxes of B raw samples cropped to S (both even): float32
    [S + 1, S/2 + 1], computed in float64 and rounded once, over the kept frequencies k = -S/2 .. S/2 (rows) and v = 0 ..
    S/2 (columns) in cycles per box.  s^2 = (k^2 + v^2) / (B apix)^2 with ``apix`` the RAW pixel size in Angstrom, phi =
    atan2(k, v) (``fit_bins``' convention: k the row frequency), dz = d0 + d1 cos(2 (phi - angle)) with d0 = (U + V) / 2,
    d1 = (U - V) / 2 and ``angle`` in degrees, c = ``ctf``(s, dz).  mode "flip": +1 where c <= 0, else -1; "multiply": -c.
    Both leave the low-resolution contrast as it was (ctf(0) = -ac < 0), and both are even: Phi(-k, -v) = Phi(k, v)."""
    if mode not in CORRECTION_MODES:
        raise ValueError("ctf correction mode %r (one of %s)" % (mode, ", ".join(CORRECTION_MODES)))
    B, S = int(B), int(S)
    if B % 2 or S % 2 or not 2 <= S <= B:
        raise ValueError("ctf correction needs an even box and an even output side, 2 <= S <= B; got B = %d, S = %d" % (B, S))
    if not (apix > 0 and np.isfinite(apix)):
        raise ValueError("apix must be positive, got %r" % (apix,))
    s, dz = filter_grid(np, B, S, float(apix), float(defocus_u), float(defocus_v), math.radians(float(angle)))
    c = ctf(s, dz, kv, cs, ac)
    if mode == "flip":
        return np.where(c <= 0, 1.0, -1.0).astype(np.float32)
    return (-c).astype(np.float32)


def filter_grid(xp, B, S, apix, defocus_u, defocus_v, angle_rad, **where):
    """The grid and the dz(phi) rule of ``correction_filter``, for NumPy or torch (``xp``; torch with ``device=``): ->
    (s, dz) float64 over rows k = -S/2 .. S/2 and columns v = 0 .. S/2.  The four parameters are floats, or arrays [G, 1, 1]
    for G filters at once (``angle_rad`` in radians)."""
    h = S // 2
    k = xp.arange(-h, h + 1, dtype=xp.float64, **where)[:, None]
    v = xp.arange(h + 1, dtype=xp.float64, **where)[None, :]
    s = xp.sqrt(k * k + v * v) / (B * apix)
    d0, d1 = 0.5 * (defocus_u + defocus_v), 0.5 * (defocus_u - defocus_v)
    dz = d0 + d1 * xp.cos(2.0 * (xp.arctan2(k, v) - angle_rad))
    return s, dz


def weight_tables(S, rows, mode, device=None):
    """The weights of the Wiener class sums (``torch.ops.sprk.class_wiener``) for a stack of side S whose
    particles went through ``correction_filter(.., mode)``: -> (wn, wd) float32 [G, S + 1, roundup(S/2 + 1, 4)], one table per
    row of ``rows`` = (DefocusU, DefocusV, DefocusAngle in degrees, kV, Cs, Q, apix of the STACK), formed in float64 and
    rounded once, the padded columns exact zeros.  c is ``ctf`` on the grid of ``correction_filter(S, S, apix, ..)``.
    "flip" (data -|c| S + n): wn = |c|, wd = c^2; "multiply" (data -c^2 S - c n): wn = 1, wd = c^2.  Without a device: NumPy
    arrays.  With one: tensors there, built there in one batch (what torch's sine differs from NumPy's is what they differ
    by)."""
    if mode not in CORRECTION_MODES:
        raise ValueError("ctf weighting mode %r (one of %s: what `joint extract --ctf_correct` was given)"
                         % (mode, ", ".join(CORRECTION_MODES)))
    try:
        S = torch_ops.class_ctf_side("weight_tables", int(S))
    except _lib.SprkError as e:
        raise ValueError(str(e)) from None
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 7)
    if not len(rows) or not np.isfinite(rows).all() or not (rows[:, 6] > 0).all() or not (rows[:, 3] > 0).all():
        raise ValueError("weight_tables: at least one row of seven finite numbers with kV > 0 and apix > 0")
    # per row, in the operations of ``ctf``: the phase is a dz s^2 - b s^4 + shift
    lam = np.array([wavelength(kv) for kv in rows[:, 3]])
    a = np.array([np.pi * l for l in lam])
    b = np.array([0.5 * np.pi * (cs * 1e7) * l ** 3 for cs, l in zip(rows[:, 4], lam)])
    shift = np.array([math.atan2(q, math.sqrt(1 - q * q)) for q in rows[:, 5]])
    if device is None:
        xp, where, col = np, {}, lambda x: x[:, None, None]
    else:
        xp, where = torch, {"device": device}
        col = lambda x: torch.as_tensor(x, dtype=torch.float64, device=device)[:, None, None]   # noqa: E731
    s, dz = filter_grid(xp, S, S, col(rows[:, 6]), col(rows[:, 0]), col(rows[:, 1]), col(np.radians(rows[:, 2])), **where)
    s2 = s * s
    c = -xp.sin(col(a) * dz * s2 - col(b) * s2 * s2 + col(shift))
    wd = c * c
    wn = xp.abs(c) if mode == "flip" else xp.ones_like(c)
    Hs, ldv = S // 2 + 1, torch_ops.class_spectrum_shapes(S)[5][1]
    if device is None:
        out = np.zeros((2, len(rows), S + 1, ldv), dtype=np.float32)
        out[0, :, :, :Hs], out[1, :, :, :Hs] = wn, wd
    else:
        out = torch.zeros((2, len(rows), S + 1, ldv), dtype=torch.float32, device=device)
        out[0, :, :, :Hs], out[1, :, :, :Hs] = wn.float(), wd.float()
    return out[0], out[1]


def check_fit_args(apix, kv, cs, ac, min_res, max_res, min_defocus, max_defocus):
    """ValueError for values the fit cannot work with (``apix`` and ``max_res`` may be None: taken from the file / apix)"""
    for name, v in (("apix", apix), ("kv", kv), ("min_res", min_res), ("max_res", max_res), ("min_defocus", min_defocus),
                    ("max_defocus", max_defocus)):
        if v is not None and not (np.isfinite(v) and v > 0):
            raise ValueError("%s must be positive, got %r" % (name, v))
    if not (np.isfinite(cs) and cs >= 0):
        raise ValueError("cs must be at least 0 (millimetres), got %r" % (cs,))
    if not 0 <= ac < 1:
        raise ValueError("ac (the amplitude contrast) must lie in [0, 1), got %r" % (ac,))
    if max_res is not None and not max_res < min_res:
        raise ValueError("max_res %r must be finer (smaller) than min_res %r" % (max_res, min_res))
    if apix is not None and max_res is not None and max_res < 2 * apix:
        raise ValueError("max_res %r lies beyond the Nyquist limit of %r Angstrom per pixel" % (max_res, apix))
    if not min_defocus < max_defocus:
        raise ValueError("min_defocus %r must be below max_defocus %r" % (min_defocus, max_defocus))


def _detrend(y, w):
    """y [..., n] minus its running mean over w bins on either side (the window clamped at the ends), then centred"""
    n = y.shape[-1]
    csum = np.concatenate([np.zeros(y.shape[:-1] + (1,)), np.cumsum(y, axis=-1)], axis=-1)
    lo, hi = np.maximum(np.arange(n) - w, 0), np.minimum(np.arange(n) + w + 1, n)
    d = y - (csum[..., hi] - csum[..., lo]) / (hi - lo)
    return d - d.mean(axis=-1, keepdims=True)


def fit_range(T, apix, min_res, max_res):
    """-> the rings k >= 1 whose spatial frequency k / (T apix) lies between 1 / min_res and 1 / max_res"""
    k = np.arange(1, T // 2 + 1)
    s = k / (T * float(apix))
    k = k[(s >= 1.0 / min_res) & (s <= 1.0 / max_res)]
    if len(k) < 16:
        raise ValueError("only %d rings of a %d tile at %g Angstrom per pixel lie between %g and %g Angstrom: too few to fit"
                         % (len(k), T, apix, min_res, max_res))
    return k


def fit_curves(profile, T, apix, kv, cs, ac, min_res, max_res, defocus):
    """-> (k, residual, model): the rings of the fit, the detrended log profile there and the detrended CTF^2 of
    ``defocus`` (an array of candidates gives a model row each)"""
    k = fit_range(T, apix, min_res, max_res)
    p = np.asarray(profile, dtype=np.float64)[k]
    if not (np.isfinite(p).all() and (p > 0).all()):
        raise ValueError("the radial profile must be positive and finite over the fitted rings")
    w = max(1, len(k) // 8)
    s = k / (T * float(apix))
    model = ctf(s, np.asarray(defocus, dtype=np.float64)[..., None], kv, cs, ac) ** 2
    return k, _detrend(np.log(p), w), _detrend(model, w)


def _scores(profile, T, apix, kv, cs, ac, min_res, max_res, candidates):
    _, y, m = fit_curves(profile, T, apix, kv, cs, ac, min_res, max_res, candidates)
    norm = np.sqrt((y * y).sum()) * np.sqrt((m * m).sum(axis=-1))
    return (m @ y) / np.where(norm > 0, norm, np.inf)


def fit_defocus(profile, T, apix, kv=300.0, cs=2.7, ac=0.07, min_res=30.0, max_res=None, min_defocus=3000.0,
                max_defocus=50000.0):
    """One defocus value for a radial profile (``radial_profile`` of a [T, T/2 + 1] spectrum at ``apix`` Angstrom per
    pixel): over the rings between ``min_res`` and ``max_res`` (default max(4, 2.2 apix)) the log of the profile minus its
    running mean (one eighth of the range on either side), centred, is compared by normalised cross-correlation with
    CTF^2 put through the same two steps; candidates on a grid of 100 Angstrom over [min_defocus, max_defocus], then in
    steps of 5 Angstrom over one coarse step on either side of the best.  The first of equal scores wins.
    -> (defocus in Angstrom, score in [-1, 1])."""
    if max_res is None:
        max_res = max(4.0, 2.2 * apix)
    check_fit_args(apix, kv, cs, ac, min_res, max_res, min_defocus, max_defocus)
    args = (profile, T, apix, kv, cs, ac, min_res, max_res)
    coarse = np.arange(float(min_defocus), float(max_defocus) + 0.5 * COARSE_STEP, COARSE_STEP)
    best = coarse[int(np.argmax(_scores(*args, coarse)))]
    fine = best + FINE_STEP * np.arange(-round(COARSE_STEP / FINE_STEP), round(COARSE_STEP / FINE_STEP) + 1)
    fine = fine[(fine >= min_defocus) & (fine <= max_defocus)]
    scores = _scores(*args, fine)
    i = int(np.argmax(scores))
    return float(fine[i]), float(scores[i])


# ---- the 2-D fit: astigmatism ---------------------------------------------------------------------------
# RELION's convention: dz(phi) = d0 + d1 cos(2 (phi - theta)), d0 = (U + V) / 2, d1 = (U - V) / 2 >= 0, phi = atan2(u', v)
# with u' the signed row frequency and v the column frequency of the stored half plane.  With e1 = d1 cos 2 theta and e2 =
# d1 sin 2 theta the phase of cos 2 chi, in turns, is linear in the candidate: t = b + p (d0 - D_ref) + q e1 + r e2.
def check_astigmatism(max_astigmatism, min_defocus):
    """ValueError unless 0 < max_astigmatism < inf and DefocusV stays positive over the whole search"""
    if not (np.isfinite(max_astigmatism) and max_astigmatism > 0):
        raise ValueError("max_astigmatism must be positive and finite, got %r" % (max_astigmatism,))
    if max_astigmatism + ASTIG_RANGE + ASTIG_STEP >= min_defocus:
        raise ValueError("max_astigmatism %r + %g reaches min_defocus %r: DefocusV could not stay positive"
                         % (max_astigmatism, ASTIG_RANGE + ASTIG_STEP, min_defocus))


def fit_bins(Pm, profile, T, apix, kv, cs, ac, min_res, max_res, d_ref):
    """The operand of ``torch.ops.sprk.ctf_score``: float32 [5, n], rows b, p, q, r, Y, computed in float64 and rounded
    once, one column per kept bin of the half plane Pm [T, T/2 + 1] in row-major order.  A bin is kept when its ring
    ``radial_bins(T)`` lies in ``fit_range`` and neither u' nor v is 0 (the two axes carry the cross the untapered tile
    edges leave).  p = lambda s^2, q = p cos 2 phi, r = p sin 2 phi, b = frac(-Cs lambda^3 s^4 / 2 + atan2(ac, sqrt(1 -
    ac^2)) / pi + p d_ref): with the 1-D fit's defocus folded in here, |t| stays within a few tens of turns.  Y = log Pm
    minus the running mean of the log radial profile at the bin's ring (the trend ``_detrend`` subtracts in the 1-D fit:
    the same window), centred over the kept bins."""
    Pm = np.asarray(Pm, dtype=np.float64)
    if Pm.shape != (T, T // 2 + 1):
        raise ValueError("a half-plane spectrum [%d, %d] is expected, got %s" % (T, T // 2 + 1, Pm.shape))
    kf = fit_range(T, apix, min_res, max_res)
    u = np.arange(T, dtype=np.int64)
    u = np.where(u > T // 2, u - T, u)[:, None]
    v = np.arange(T // 2 + 1, dtype=np.int64)[None, :]
    k = radial_bins(T)
    keep = (k >= kf[0]) & (k <= kf[-1]) & (u != 0) & (v != 0)
    uu, vv = np.broadcast_to(u, k.shape)[keep].astype(np.float64), np.broadcast_to(v, k.shape)[keep].astype(np.float64)
    power = Pm[keep]
    if not (np.isfinite(power).all() and (power > 0).all()):
        raise ValueError("the spectrum must be positive and finite over the fitted bins")
    logp = np.log(np.asarray(profile, dtype=np.float64)[kf])
    if not np.isfinite(logp).all():
        raise ValueError("the radial profile must be positive and finite over the fitted rings")
    w = max(1, len(kf) // 8)
    trend = _running_mean(logp, w)
    lam, csa = wavelength(kv), cs * 1e7
    s2 = (uu * uu + vv * vv) / (T * float(apix)) ** 2
    phi2 = 2.0 * np.arctan2(uu, vv)
    p = lam * s2
    b = -0.5 * csa * lam ** 3 * s2 * s2 + math.atan2(ac, math.sqrt(1 - ac * ac)) / math.pi + p * float(d_ref)
    Y = np.log(power) - trend[k[keep] - kf[0]]
    return np.stack([b - np.floor(b), p, p * np.cos(phi2), p * np.sin(phi2), Y - Y.mean()]).astype(np.float32)


def _running_mean(y, w):
    """the mean of y over w bins on either side, the window clamped at the ends: what ``_detrend`` subtracts"""
    n = len(y)
    csum = np.concatenate([[0.0], np.cumsum(y)])
    lo, hi = np.maximum(np.arange(n) - w, 0), np.minimum(np.arange(n) + w + 1, n)
    return (csum[hi] - csum[lo]) / (hi - lo)


def score(S, Y):
    """S float64 [ncand, 3] = (sum c, sum c^2, sum Y c) over the n bins, c = cos 2 pi t -> the Pearson correlation of Y with
    -c per candidate, float64 [ncand]; 0 where a variance is not positive"""
    S = np.asarray(S, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.size
    sy, syy = Y.sum(), (Y * Y).sum()
    var = (S[:, 1] - S[:, 0] ** 2 / n) * (syy - sy * sy / n)
    ok = var > 0
    return np.where(ok, -(S[:, 2] - S[:, 0] * sy / n) / np.sqrt(np.where(ok, var, 1.0)), 0.0)


def device_sums(bins, cand, device="cuda"):
    """``torch.ops.sprk.ctf_score`` on float32 NumPy arrays [5, n] and [ncand, 3] -> float64 [ncand, 3]"""
    b = torch.from_numpy(np.array(bins, dtype=np.float32, order="C"))      # a copy: the caller's may be read-only
    pad = -b.shape[1] % 4                                        # the operator wants a row stride that is a multiple of 4
    b = torch.nn.functional.pad(b, (0, pad)).to(device)[:, :b.shape[1]]
    c = torch.from_numpy(np.array(cand, dtype=np.float32, order="C")).to(device)
    return torch.ops.sprk.ctf_score(b, c).cpu().numpy()


def astigmatism_grids(max_astigmatism):
    """-> (coarse float64 [m, 3], fine offsets float64 [9261, 3]) in (d0 - D_ref, e1, e2): d0 outermost, e2 innermost,
    ascending.  Coarse: d0 over -500 .. 500, e1 and e2 over the multiples of 50 within max_astigmatism, kept inside the
    circle e1^2 + e2^2 <= max_astigmatism^2; fine: steps of 5 over -50 .. 50 in all three."""
    m = int(math.floor(max_astigmatism / ASTIG_STEP))
    e = ASTIG_STEP * np.arange(-m, m + 1)
    d = ASTIG_STEP * np.arange(-round(ASTIG_RANGE / ASTIG_STEP), round(ASTIG_RANGE / ASTIG_STEP) + 1)
    g = np.stack(np.meshgrid(d, e, e, indexing="ij"), axis=-1).reshape(-1, 3)
    coarse = g[g[:, 1] ** 2 + g[:, 2] ** 2 <= max_astigmatism ** 2]
    f = FINE_STEP * np.arange(-round(ASTIG_STEP / FINE_STEP), round(ASTIG_STEP / FINE_STEP) + 1)
    return coarse, np.stack(np.meshgrid(f, f, f, indexing="ij"), axis=-1).reshape(-1, 3)


def fit_astigmatism(Pm, T, apix, kv=300.0, cs=2.7, ac=0.07, min_res=30.0, max_res=None, min_defocus=3000.0,
                    max_defocus=50000.0, max_astigmatism=MAX_ASTIGMATISM, sums=None):
    """DefocusU, DefocusV and the angle for a mean power spectrum Pm [T, T/2 + 1]: the 1-D fit of its radial profile gives
    D_ref; every candidate (d0 - D_ref, e1, e2) of ``astigmatism_grids`` is scored by the correlation of the detrended log
    spectrum with -cos 2 chi over the bins of ``fit_bins``, first the coarse grid, then the fine one around its best.  The
    first of equal scores wins.  ``sums(bins, cand) -> float64 [ncand, 3]`` does the work: ``device_sums`` by default, a
    NumPy model for a caller without a GPU.
    -> (defocus_u, defocus_v, angle in degrees in [0, 180), score)."""
    if max_res is None:
        max_res = max(4.0, 2.2 * apix)
    check_fit_args(apix, kv, cs, ac, min_res, max_res, min_defocus, max_defocus)
    check_astigmatism(max_astigmatism, min_defocus)
    profile = radial_profile(Pm)
    d_ref, _ = fit_defocus(profile, T, apix, kv, cs, ac, min_res, max_res, min_defocus, max_defocus)
    bins = fit_bins(Pm, profile, T, apix, kv, cs, ac, min_res, max_res, d_ref)
    sums = device_sums if sums is None else sums
    coarse, fine = astigmatism_grids(float(max_astigmatism))
    best = coarse[int(np.argmax(score(sums(bins, coarse.astype(np.float32)), bins[4])))]
    fine = best + fine
    scores = score(sums(bins, fine.astype(np.float32)), bins[4])
    i = int(np.argmax(scores))
    d0, e1, e2 = d_ref + fine[i, 0], fine[i, 1], fine[i, 2]
    d1 = math.hypot(e1, e2)
    angle = math.degrees(0.5 * math.atan2(e2, e1)) % 180.0 if d1 > 0 else 0.0
    if angle >= 180.0:                                           # a tiny negative angle rounds up to the modulus
        angle = 0.0
    return float(d0 + d1), float(d0 - d1), float(angle), float(scores[i])


# ---- `joint ctf` ---------------------------------------------------------------------------------------------------------
def header_apix(header):
    """the pixel size an MRC header states, xlen / mx, or None when it states none: no sampling or no cell length, or the
    cell of one unit sample (mx = 1, xlen = 1) that writers who do not know the pixel size leave on a wider image"""
    if not (header.mx > 0 and np.isfinite(header.xlen) and header.xlen > 0):
        return None
    if header.mx == 1 and header.xlen == 1 and header.nx > 1:
        return None
    return float(header.xlen) / header.mx


def star_row(name, defocus, score, apix, kv, cs, ac, defocus_v=None, angle=0.0):
    """one row of micrographs_ctf.star; ``defocus`` is DefocusU, and DefocusV as well unless ``defocus_v`` is given"""
    return "%s\t%.2f\t%.2f\t%.2f\t%.2f\t%.4f\t%.4f\t%.2f\t%.5f\t%.6f\n" % (
        name, defocus, defocus if defocus_v is None else defocus_v, angle, kv, cs, ac, MAGNIFICATION, apix, score)


def write_profile(path, profile, T, apix, k_fit, residual, model):
    """{name}_profile.txt: ring, spatial frequency, mean power, and over the fitted rings the residual and the fitted CTF^2
    (both detrended; nan elsewhere)"""
    res, mod = np.full(len(profile), np.nan), np.full(len(profile), np.nan)
    res[k_fit], mod[k_fit] = residual, model
    with open(path, "w") as f:
        f.write("k\tinv_angstrom\tpower\tresidual\tfitted_ctf2\n")
        for k in range(len(profile)):
            f.write("%d\t%.8f\t%.9g\t%.6f\t%.6f\n" % (k, k / (T * apix), profile[k], res[k], mod[k]))


def ctf_dataset(dataset, out_dir, apix=None, kv=300.0, cs=2.7, ac=0.07, tile=512, min_res=30.0, max_res=None,
                min_defocus=3000.0, max_defocus=50000.0, device="cuda", astigmatism=False, max_astigmatism=MAX_ASTIGMATISM):
    """``joint ctf``: for every raw MRC micrograph of the table / directory ``dataset``: ``out_dir/{name}_psd.mrc`` (the
    mean power spectrum, float32 [T, T/2 + 1]), ``out_dir/{name}_profile.txt`` and one row of
    ``out_dir/micrographs_ctf.star``, written at the end.  ``apix``: Angstrom per pixel, from each file's header (xlen /
    mx) when None.  Runs in one process: the per-micrograph work is a millisecond of device time and the rest is the read
    of the file, so the table is not spread over ranks (WORLD_SIZE is ignored).
    ``astigmatism``: the row carries DefocusU, DefocusV, the angle and the score of ``fit_astigmatism`` (candidates within
    ``max_astigmatism`` Angstrom of half-difference) in place of the 1-D fit's; the other two files stay as they are.
    -> {name: {"defocus", "score", "apix", "tiles"}}, with ``astigmatism`` also "defocus_u", "defocus_v", "angle" and
    "score_2d"."""
    T = check_tile(tile)
    check_fit_args(apix, kv, cs, ac, min_res, max_res, min_defocus, max_defocus)
    if astigmatism:
        check_astigmatism(max_astigmatism, min_defocus)
    rows = micrograph_io.read_image_table(dataset)
    if not rows:
        raise ValueError("no micrographs found in %s" % dataset)
    os.makedirs(out_dir, exist_ok=True)
    results, star = {}, []
    for _, name, path in rows:
        raw, header = ingest.read_raw(path, device)
        a = float(apix) if apix is not None else header_apix(header)
        if a is None:
            raise ValueError("%s: the header states no pixel size (xlen %r, mx %r): give --apix" % (path, header.xlen, header.mx))
        res = max(4.0, 2.2 * a) if max_res is None else max_res
        check_fit_args(a, kv, cs, ac, min_res, res, min_defocus, max_defocus)
        P, ntiles = psd_sum((raw, header), T, device)
        Pm = mean_power(P.cpu().numpy(), ntiles, T)
        profile = radial_profile(Pm)
        defocus, score = fit_defocus(profile, T, a, kv, cs, ac, min_res, res, min_defocus, max_defocus)
        with open(os.path.join(out_dir, name + "_psd.mrc"), "wb") as f:
            micrograph_io.write_mrc(f, Pm.astype(np.float32))
        k_fit, residual, model = fit_curves(profile, T, a, kv, cs, ac, min_res, res, defocus)
        write_profile(os.path.join(out_dir, name + "_profile.txt"), profile, T, a, k_fit, residual, model)
        results[name] = {"defocus": defocus, "score": score, "apix": a, "tiles": ntiles}
        if astigmatism:
            du, dv, angle, score2 = fit_astigmatism(Pm, T, a, kv, cs, ac, min_res, res, min_defocus, max_defocus, max_astigmatism,
                                                    sums=lambda b, c: device_sums(b, c, device))
            star.append(star_row(os.path.basename(path), du, score2, a, kv, cs, ac, dv, angle))
            results[name].update(defocus_u=du, defocus_v=dv, angle=angle, score_2d=score2)
        else:
            star.append(star_row(os.path.basename(path), defocus, score, a, kv, cs, ac))
    with open(os.path.join(out_dir, "micrographs_ctf.star"), "w") as f:
        f.write(CTF_STAR_HEADER)
        f.writelines(star)
    logger.info("%s: %d micrographs fitted, %s", dataset, len(star), os.path.join(out_dir, "micrographs_ctf.star"))
    return results


def read_ctf_star(path):
    """``micrographs_ctf.star`` (or any flat loop_ table with the columns of CTF_STAR_COLUMNS) ->
    {micrograph name: {column: text}}"""
    labels, table = [], {}
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#") or line.startswith("data_") or line == "loop_":
                continue
            if line.startswith("_rln"):
                labels.append(line.split()[0][4:])
                continue
            fields = line.split()
            if len(fields) != len(labels):
                raise ValueError("%s: a row of %d fields under %d labels: %r" % (path, len(fields), len(labels), line))
            row = dict(zip(labels, fields))
            table[row.get("MicrographName")] = row
    missing = [c for c in CTF_STAR_COLUMNS if c not in labels]
    if missing:
        raise ValueError("%s: no column _rln%s" % (path, ", _rln".join(missing)))
    return table
