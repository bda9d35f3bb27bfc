"""``joint align --dose``: dose-weighted movie sums, accumulated in Fourier space on the device.

    Y = IDFT2[by, bx]( sum_f  G_f . crop( DFT2[ny, nx](D_f) ) ),    G_f[k, v] = Phi_f[k, v] e^{-2 pi i (k dy_f / ny + v dx_f / nx)}

over the kept frequencies: columns v = 0 .. bx // 2 (Hs of them; the inverse weighs v = 0 and, for even bx, v = bx / 2 once
and every other column twice), rows k = -h .. h with h = by // 2 (``kept_rows``: for even by the rows +-h are kept apart,
each with its own phase, at half weight; the convention of ``align.shift_matrix64`` and ``extract.filter_matrices64``).
With Phi = 1 this is ``sum_f shift_matrix64(ny, by, dy_f) D_f shift_matrix64(nx, bx, dx_f)^T``.

Phi is the exposure filter of Grant & Grigorieff (eLife 2015;4:e06980), as in unblur: the critical exposure
Ne(q) = s (0.245 q^-1.665 + 2.81) e/A^2 at spatial frequency q in 1/A, s = 1 at 300 kV and 0.8 at 200 kV (between the two
voltages s is interpolated linearly: that interpolation is ours, the paper states the two values), N_f the exposure at the
end of frame f, w_f = exp(-N_f / (2 Ne)) and Phi_f = w_f sqrt(Z / sum_g w_g^2), so that sum_f Phi_f^2 = Z at every
frequency: white noise keeps the power it has in the plain sum.  Phi_f = 1 at q = 0.

The device half: ``torch.ops.sprk.align_spectrum`` per frame (the forward transform along both axes and the complex
multiply-add into the running spectrum F) and ``torch.ops.sprk.align_synthesize`` once per movie (csrc/alignsum.hip).  The
four matrices carry no shift and are built once per geometry; per frame only ``g`` [2Ku, roundup(Hs, 4)] is built."""
import numpy as np
import torch

from . import fourier, torch_ops
from .fourier import column_weights, kept_rows, wrap_delta

KV_RANGE = (200.0, 300.0)
_BLOCK = 1 << 23                                 # entries of a matrix built at a time (float64 and int64 temporaries)


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def check_dose_args(dose, pre_dose=0.0, kv=300.0, apix=None):
    """-> (dose, pre_dose, kv, apix) as floats (apix may stay None: the movie's header is asked then)"""
    def number(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError("%s must be a finite number, got %r" % (name, v))
        return float(v)
    dose, pre_dose, kv = number("dose", dose), number("pre_dose", pre_dose), number("kv", kv)
    if not dose > 0:
        raise ValueError("dose must be positive (e/A^2 per frame), got %r" % dose)
    if pre_dose < 0:
        raise ValueError("pre_dose must not be negative (e/A^2), got %r" % pre_dose)
    if not KV_RANGE[0] <= kv <= KV_RANGE[1]:
        raise ValueError("kv must lie in %g..%g (the critical exposure is known at those two voltages), got %r"
                         % (KV_RANGE + (kv,)))
    if apix is not None:
        apix = number("apix", apix)
        if not apix > 0:
            raise ValueError("apix must be positive (A per pixel), got %r" % apix)
    return dose, pre_dose, kv, apix


def _check_sizes(ny, nx, by, bx):
    ny, nx, by, bx = int(ny), int(nx), int(by), int(bx)
    if not (2 <= by <= ny <= torch_ops.INGEST_MAX_SIDE and 2 <= bx <= nx <= torch_ops.INGEST_MAX_SIDE):
        raise ValueError("a %dx%d frame summed to %dx%d: 2 <= by <= ny <= %d and 2 <= bx <= nx <= %d"
                         % (ny, nx, by, bx, torch_ops.INGEST_MAX_SIDE, torch_ops.INGEST_MAX_SIDE))
    return ny, nx, by, bx


# ---- the kept frequencies and the four matrices -------------------------------------------------------------------------------
def spectrum_matrices64(ny, nx, by, bx):
    """The four real matrices of ``align_spectrum`` / ``align_synthesize`` in float64 (``fourier.four_stage64``): W1 [2Hs, nx]
    the half-plane DFT along the rows of a frame, W2 [2Ku, 2ny] the DFT along its columns at the kept rows, W3 [2by, 2Ku]
    the inverse along the columns with the row weights and 1 / ny, W4 [bx, 2Hs] the inverse along the rows with the column
    weights and 1 / nx."""
    ny, nx, by, bx = _check_sizes(ny, nx, by, bx)
    return fourier.four_stage64(ny, nx, by, bx, ny, nx)


_matrices = {}


def spectrum_matrices(ny, nx, by, bx, device):
    """``spectrum_matrices64`` rounded to float32 as the operands of the two operators: contiguous tensors on ``device``,
    columns rounded up to a multiple of 4 with exact zeros (``torch_ops.align_spectrum_shapes``).  Built there with torch in
    row blocks (W2 of a 16384-pixel frame is 4.3 GB in float32; its float64 form never exists), operation for operation as
    the NumPy ones, once per (ny, nx, by, bx, device): the two most recent geometries stay cached (a cache of its own: the
    one of ``fourier.operands`` has no bound)."""
    ny, nx, by, bx = _check_sizes(ny, nx, by, bx)
    device = torch.device(device)
    key = (ny, nx, by, bx, str(device))
    if key in _matrices:
        return _matrices[key]
    k, a = kept_rows(ny, by)
    Ku, Hs = len(k), bx // 2 + 1
    v = np.arange(Hs, dtype=np.int64)
    a = torch.as_tensor(a / ny, device=device)[None, :]
    w = torch.as_tensor(column_weights(bx) / nx, device=device)[None, :]
    W1, W2, W3, W4 = (torch.zeros(s, dtype=torch.float32, device=device)
                      for s in torch_ops.align_spectrum_shapes(ny, nx, by, bx, Ku)[:4])
    for s, c, sn in fourier.trig_blocks(v, np.arange(nx), nx, device, _BLOCK):
        W1[s, :nx], W1[Hs + s.start:Hs + s.stop, :nx] = c.float(), sn.float()
    for s, c, sn in fourier.trig_blocks(k, np.arange(ny), ny, device, _BLOCK):
        lo = slice(Ku + s.start, Ku + s.stop)
        W2[s, :ny], W2[s, ny:2 * ny] = c.float(), (-sn).float()
        W2[lo, :ny], W2[lo, ny:2 * ny] = (-sn).float(), (-c).float()
    for s, c, sn in fourier.trig_blocks(np.arange(by), k, by, device, _BLOCK):
        lo = slice(by + s.start, by + s.stop)
        c, sn = a * c, a * sn
        W3[s, :Ku], W3[s, Ku:2 * Ku] = c.float(), (-sn).float()
        W3[lo, :Ku], W3[lo, Ku:2 * Ku] = sn.float(), c.float()
    for s, c, sn in fourier.trig_blocks(np.arange(bx), v, bx, device, _BLOCK):
        W4[s, :Hs], W4[s, Hs:2 * Hs] = (w * c).float(), (-(w * sn)).float()
    while len(_matrices) >= 2:
        _matrices.pop(next(iter(_matrices)))
    _matrices[key] = (W1, W2, W3, W4)
    return _matrices[key]


# ---- the exposure filter --------------------------------------------------------------------------------------------------------
def critical_dose(q, kv=300.0):
    """Ne(q) in e/A^2 at spatial frequency q (1/A; array or scalar): s (0.245 q^-1.665 + 2.81), s = 1 at 300 kV, 0.8 at 200 kV
    and linear in between; infinite at q = 0."""
    kv = float(kv)
    if not KV_RANGE[0] <= kv <= KV_RANGE[1]:
        raise ValueError("kv must lie in %g..%g, got %r" % (KV_RANGE + (kv,)))
    s = 0.8 + 0.2 * (kv - 200.0) / 100.0
    q = np.asarray(q, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return s * (0.245 * np.power(q, -1.665) + 2.81)


def frequencies(ny, nx, by, bx, apix):
    """-> q float64 [Ku, Hs] in 1/A: sqrt((k / (ny apix))^2 + (v / (nx apix))^2) over the kept rows and columns"""
    k, _ = kept_rows(ny, by)
    v = np.arange(bx // 2 + 1, dtype=np.float64)
    return np.sqrt((k[:, None] / (ny * float(apix))) ** 2 + (v[None, :] / (nx * float(apix))) ** 2)


def _exponent(ny, nx, by, bx, apix, kv):
    """E = -1 / (2 Ne) [Ku, Hs], exactly 0 at q = 0"""
    q = frequencies(ny, nx, by, bx, apix)
    return np.where(q == 0, 0.0, -0.5 / critical_dose(np.where(q == 0, 1.0, q), kv))


def dose_filter64(ny, nx, by, bx, apix, dose, pre_dose, kv, Z):
    """-> Phi float64 [Z, Ku, Hs]: w_f sqrt(Z / sum_g w_g^2) with w_f = exp(-N_f / (2 Ne)), N_f = pre_dose + (f + 1) dose;
    exactly 1 at q = 0 (set, not computed)."""
    ny, nx, by, bx = _check_sizes(ny, nx, by, bx)
    dose, pre_dose, kv, apix = check_dose_args(dose, pre_dose, kv, apix)
    E = _exponent(ny, nx, by, bx, apix, kv)
    N = pre_dose + (np.arange(int(Z), dtype=np.float64) + 1.0) * dose
    w = np.exp(N[:, None, None] * E[None])
    phi = w * np.sqrt(int(Z) / (w * w).sum(axis=0))[None]
    phi[:, E == 0] = 1.0
    return phi


def frame_filter64(phi, ny, nx, by, bx, dy, dx):
    """G = phi e^{-2 pi i (k dy / ny + v dx / nx)}: complex128 [Ku, Hs] for one frame's float64 phi [Ku, Hs] (or 1.0) and its
    shift (dy, dx) in raw pixels, out(t) = in(t - d)"""
    k, _ = kept_rows(ny, by)
    v = np.arange(bx // 2 + 1, dtype=np.float64)
    py = np.exp(1j * ((-2.0 * np.pi / ny) * (k * wrap_delta(ny, dy))))
    px = np.exp(1j * ((-2.0 * np.pi / nx) * (v * wrap_delta(nx, dx))))
    return phi * (py[:, None] * px[None, :])


def pack_filter(G):
    """complex [Ku, Hs] -> the float32 operand g [2Ku, roundup(Hs, 4)] (NumPy): real rows over imaginary rows, rounded once"""
    Ku, Hs = G.shape
    g = np.zeros((2 * Ku, torch_ops._up4(Hs)), dtype=np.float32)
    g[:Ku, :Hs], g[Ku:, :Hs] = G.real.astype(np.float32), G.imag.astype(np.float32)
    return g


class FrameFilters:
    """The per-frame operand ``g`` of ``align_spectrum``, built on ``device`` with torch in float64 and rounded once:
    exp(N_f E) from the cached E = -1 / (2 Ne), times the cached normaliser sqrt(Z / sum_g w_g^2), times the outer product
    of the two phase vectors."""

    def __init__(self, ny, nx, by, bx, Z, device, apix, dose, pre_dose=0.0, kv=300.0):
        self.ny, self.nx, self.by, self.bx = _check_sizes(ny, nx, by, bx)
        self.Z, self.device = int(Z), torch.device(device)
        dose, pre_dose, kv, apix = check_dose_args(dose, pre_dose, kv, apix)
        if apix is None:
            raise ValueError("dose weighting needs the pixel size (apix)")
        k, _ = kept_rows(self.ny, self.by)
        self.Ku, self.Hs = len(k), self.bx // 2 + 1
        self._k = torch.as_tensor(k, device=self.device).double()
        self._v = torch.arange(self.Hs, device=self.device).double()
        self._N = pre_dose + (np.arange(self.Z, dtype=np.float64) + 1.0) * dose
        self._E = torch.as_tensor(_exponent(self.ny, self.nx, self.by, self.bx, apix, kv), device=self.device)
        total = torch.zeros_like(self._E)
        for n in self._N:
            total += torch.exp((2.0 * float(n)) * self._E)
        self._norm = torch.sqrt(self.Z / total)                      # exactly 1 where E is 0: Z / (Z ones)

    def phi64(self, f):
        """Phi_f float64 [Ku, Hs] on the device"""
        return torch.exp(float(self._N[f]) * self._E) * self._norm

    def filter64(self, f, dy, dx):
        """-> (Gr, Gi) float64 [Ku, Hs] on the device, before the rounding"""
        ay = (-2.0 * np.pi / self.ny) * (self._k * wrap_delta(self.ny, dy))
        ax = (-2.0 * np.pi / self.nx) * (self._v * wrap_delta(self.nx, dx))
        cy, sy, cx, sx = torch.cos(ay)[:, None], torch.sin(ay)[:, None], torch.cos(ax)[None, :], torch.sin(ax)[None, :]
        phi = self.phi64(f)
        return phi * (cy * cx - sy * sx), phi * (cy * sx + sy * cx)

    def g(self, f, dy, dx):
        """-> float32 [2Ku, roundup(Hs, 4)] on the device: a fresh tensor (the call that reads it is only enqueued)"""
        gr, gi = self.filter64(f, dy, dx)
        out = torch.zeros((2 * self.Ku, torch_ops._up4(self.Hs)), dtype=torch.float32, device=self.device)
        out[:self.Ku, :self.Hs], out[self.Ku:, :self.Hs] = gr.float(), gi.float()
        return out


def sum_frames_weighted(movie, by, bx, shifts_y, shifts_x, apix, dose, pre_dose=0.0, kv=300.0):
    """``align.sum_frames`` through Fourier space -> float32 CUDA [by, bx]: sum over the frames of (frame f shifted by
    (shifts_y[f], shifts_x[f]) raw pixels, weighted by Phi_f and Fourier-cropped), ``align_spectrum`` per frame,
    ``align_synthesize`` once, and the anchor term at the end (one fp32 add: Phi is 1 at the origin)."""
    h = movie.header
    dev = movie._reader.device
    W1, W2, W3, W4 = spectrum_matrices(h.ny, h.nx, by, bx, dev)
    filters = FrameFilters(h.ny, h.nx, by, bx, h.nz, dev, apix, dose, pre_dose, kv)
    F = torch.empty((2 * filters.Ku, torch_ops._up4(filters.Hs)), dtype=torch.float32, device=dev)
    for k in range(h.nz):
        raw = movie.frame(k)
        torch.ops.sprk.align_spectrum(raw, h.mode, h.ny, h.nx, W1, W2, filters.g(k, shifts_y[k], shifts_x[k]), movie.anchor,
                                      F, k == 0)
    y = torch.ops.sprk.align_synthesize(F, by, bx, W3, W4)
    if h.mode != 2:
        y += float(np.float32(h.nz * movie.anchor))
    return y
