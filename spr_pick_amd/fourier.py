"""The real operand matrices of the fp32 MFMA transform kernels: every numerical contract they share, stated once
(DESIGN §4.3m).  ``ingest``, ``ctf``, ``extract``, ``align`` and ``dose`` keep the names their callers know, each with its
own argument check in front where it has one, and build through this module.

* the phase: an integer product is reduced mod its period in int64 before it is scaled by 2 pi / period (``reduced``,
  ``phase``), so the angle is as exact as float64 can hold it whatever the size;
* the kept frequencies and their weights (``kept_rows``, ``column_weights``);
* the four matrices of a Fourier crop in four GEMM stages (``four_stage64``; ``half_plane64`` is its first);
* the Dirichlet kernel of a Fourier crop (``resample_matrix64``) and of a shift and crop (``shift_matrix64``, NumPy or
  torch from one body), which share the exact reduction of their integer phase (``dirichlet_phase``) and nothing after it:
  ``shift_matrix64(B, S, 0)`` is ``resample_matrix64(B, S)`` within 1e-12, not in bits, and the torch build differs from the
  NumPy one by what the two sines differ;
* "rounded to float32, padded with exact zeros to the operand's shape, on the device, built once" (``operands``)."""
import numpy as np
import torch

from . import torch_ops


def _ints(n):
    return np.arange(n, dtype=np.int64)


# ---- the phase -------------------------------------------------------------------------------------------------------------
def reduced(n, period):
    """2 pi (n mod period) / period in float64 for an int64 array or tensor n"""
    n = n % period
    return (2.0 * np.pi / period) * (n.double() if torch.is_tensor(n) else n)


def phase(rows, cols, period):
    """``reduced`` of the outer product of two int64 vectors: [len(rows), len(cols)]"""
    return reduced(rows[:, None] * cols[None, :], period)


def trig_blocks(rows, cols, period, device, block):
    """cos and sin of ``phase(rows, cols, period)`` on ``device``, rows of at most ``block`` entries at a time: yields
    (slice, cos, sin)"""
    cols = torch.as_tensor(cols, dtype=torch.int64, device=device)
    step = max(1, block // max(1, len(cols)))
    for r0 in range(0, len(rows), step):
        ang = phase(torch.as_tensor(rows[r0:r0 + step], dtype=torch.int64, device=device), cols, period)
        yield slice(r0, r0 + len(ang)), torch.cos(ang), torch.sin(ang)


# ---- the kept frequencies and the four stages ------------------------------------------------------------------------------
def kept_rows(B, S):
    """-> (k int64 [Ku], weights float64 [Ku]): the row frequencies of B samples that an output of S keeps, -h .. h with
    h = S // 2.  Even S: Ku = S + 1 and the rows +-h weigh 1/2 each (also for S == B, where they are one frequency of the
    frame).  Odd S: Ku = S, every weight 1."""
    B, S = int(B), int(S)
    if not 2 <= S <= B:
        raise ValueError("kept_rows: 2 <= S <= B, got B = %d, S = %d" % (B, S))
    h = S // 2
    k = np.arange(-h, h + 1, dtype=np.int64)
    return k, np.where((np.abs(k) == h) & (S % 2 == 0), 0.5, 1.0)


def column_weights(bx):
    """-> float64 [Hs]: what the last inverse stage weighs column v = 0 .. bx // 2 with: 1 at v = 0 and, even bx, at bx / 2"""
    v = np.arange(bx // 2 + 1)
    return np.where((v == 0) | ((bx % 2 == 0) & (v == bx // 2)), 1.0, 2.0)


def half_plane64(H, n):
    """-> float64 [2H, n], the half-plane DFT along rows of n samples: row v cos(2 pi v c / n), row H + v the sine"""
    a = phase(_ints(H), _ints(n), n)
    return np.concatenate([np.cos(a), np.sin(a)])


def four_stage64(ny, nx, by, bx, row_div, col_div):
    """The four real matrices that take [ny, nx] samples to [by, bx] through the kept frequencies, in float64, Hs = bx // 2
    + 1 and k, Ku of ``kept_rows(ny, by)``: W1 [2Hs, nx] = ``half_plane64``, W2 [2Ku, 2ny] = [[C, -S], [-S, -C]] the DFT
    along the columns at the kept rows, W3 [2by, 2Ku] = [[C, -S], [S, C]] the inverse along the columns with the row weights
    over ``row_div``, W4 [bx, 2Hs] = [C, -S] the inverse along the rows with the column weights over ``col_div``."""
    k, a = kept_rows(ny, by)
    v = _ints(bx // 2 + 1)
    a2, a3, a4 = phase(k, _ints(ny), ny), phase(_ints(by), k, by), phase(_ints(bx), v, bx)
    a = a[None, :] / row_div
    w = column_weights(bx)[None, :] / col_div
    C2, S2, C3, S3 = np.cos(a2), np.sin(a2), a * np.cos(a3), a * np.sin(a3)
    return (half_plane64(len(v), nx), np.block([[C2, -S2], [-S2, -C2]]), np.block([[C3, -S3], [S3, C3]]),
            np.concatenate([w * np.cos(a4), -w * np.sin(a4)], axis=1))


# ---- the Dirichlet crop and the shift ---------------------------------------------------------------------------------------
def _crop_sizes(who, B, S):
    B, S = int(B), int(S)
    if not 2 <= S <= B:
        raise ValueError("%s: 2 <= S <= B, got B = %d, S = %d" % (who, B, S))
    return B, S


def dirichlet_phase(B, S, xp=np, **where):
    """-> (t, tn) int64 [S, B]: t = s B - b S reduced to (-S B / 2, S B / 2] and t mod 2B reduced to (-B, B], exactly, as
    arrays of ``xp`` (NumPy, or torch with ``device=``)"""
    period = S * B
    t = (xp.arange(S, dtype=xp.int64, **where)[:, None] * B - xp.arange(B, dtype=xp.int64, **where)[None, :] * S) % period
    t = xp.where(2 * t > period, t - period, t)                  # numerator and denominator change sign together
    tn = t % (2 * B)
    return t, xp.where(tn > B, tn - 2 * B, tn)


def resample_matrix64(B, S):
    """The Fourier crop of B samples to S as a real [S, B] matrix in float64, IDFT_S . crop . DFT_B scaled by S / B: the
    operator of ``extract.crop_matrix64`` with its sum over k in closed form (a Dirichlet kernel).  With the phase
    t = (s B - b S) mod (S B) in integers and theta / 2 = pi t / (S B):
        M[s, b] = (1/B) sin(pi (t mod 2B) / B) / sin(theta / 2)              for odd S,
        the same times cos(theta / 2)                                        for even S (the Nyquist term is shared),
        S / B where t == 0;
    t is taken in (-S B / 2, S B / 2] and then t mod 2B in (-B, B] (``dirichlet_phase``): M keeps its value, and the sines
    of small arguments their relative accuracy.  Every row sums to 1.  S == B is the identity and is returned as such.
    Not the bits of ``crop_matrix64`` (they differ by a few 1e-13): that one stays the contract of ``joint extract --scale``."""
    B, S = _crop_sizes("resample_matrix", B, S)
    if S == B:
        return np.eye(B)
    t, tn = dirichlet_phase(B, S)
    zero = t == 0
    half = (np.pi / (S * B)) * t
    m = np.sin((np.pi / B) * tn) / np.sin(np.where(zero, 1.0, half)) / B
    if S % 2 == 0:
        m = m * np.cos(half)
    return np.where(zero, S / B, m)


def resample_matrix(B, S, device=None):
    """``resample_matrix64`` rounded to float32.  Without a device: the [S, B] array.  With one: an operand of
    ``torch.ops.sprk.ingest_resample``, a contiguous tensor [roundup(S, 16), roundup(B, 4)] on that device whose added
    rows and columns are exact zeros, built once per (B, S, device)."""
    B, S = int(B), int(S)
    return operands(resample_matrix64, (B, S), torch_ops.crop_matrix_shape(B, S), device)


def wrap_delta(B, delta):
    delta = float(delta)
    if not np.isfinite(delta):
        raise ValueError("shift must be finite, got %r" % (delta,))
    return delta - B * np.round(delta / B)                       # the operator has period B in delta


def _shift_matrix64(xp, B, S, delta, **where):
    B, S = _crop_sizes("shift_matrix", B, S)
    delta = wrap_delta(B, delta)
    t, tn = (xp.asarray(i, dtype=xp.float64) for i in dirichlet_phase(B, S, xp, **where))
    w = (tn - S * delta) / B                                     # the numerator is sin(pi w)
    w = w - 2.0 * xp.round(w / 2.0)
    w = xp.where(w > 0.5, 1.0 - w, xp.where(w < -0.5, -1.0 - w, w))
    half = (np.pi / (S * B)) * (t - S * delta)
    den = xp.sin(half)
    zero = den == 0
    m = xp.sin(np.pi * w) / xp.where(zero, xp.ones_like(den), den) / B
    if S % 2 == 0:
        m = m * xp.cos(half)
    return xp.where(zero, xp.full_like(m, S / B), m)


def shift_matrix64(B, S, delta):
    """Shift B periodic samples by ``delta`` samples (out(t) = in(t - delta)) and Fourier-crop them to S, as a real [S, B]
    matrix in float64: (S/B) IDFT_S . crop . diag(e^{-2 pi i k delta / B}) . DFT_B with its sum over k in closed form, a
    Dirichlet kernel at u = s B / S - b - delta.  With x = pi u / B:
        M[s, b] = (1/B) sin(S x) / sin(x)                for odd S,
        the same times cos(x)                            for even S (the +-S/2 term is shared at half weight each),
        S / B where sin(x) == 0.
    The integer part t = s B - b S of S u is reduced exactly (``dirichlet_phase``; the numerator's argument is then folded
    about +-pi/2) before ``delta`` enters, so that the sines keep their relative accuracy.  Every row sums to 1; ``delta`` =
    0 is ``resample_matrix64`` (within 1e-12), the identity for S == B."""
    return _shift_matrix64(np, B, S, delta)


def shift_matrix_device64(B, S, delta, device):
    """``shift_matrix64`` built on ``device`` with torch, the same body: float64 [S, B].  (On the host, 40 frames times two
    4096^2 matrices of sines are tens of seconds.)  It differs from the NumPy one by what the two sines differ."""
    return _shift_matrix64(torch, B, S, delta, device=device)


def shift_matrix(B, S, delta, device=None):
    """``shift_matrix64`` rounded to float32.  Without a device: the [S, B] array.  With one: an operand of
    ``torch.ops.sprk.align_accumulate``, built there (``shift_matrix_device64``) and padded as ``resample_matrix(B, S,
    device)`` is: [roundup(S, 16), roundup(B, 4)] with exact zeros added.  Not cached: one per frame and iteration."""
    if device is None:
        return shift_matrix64(B, S, delta).astype(np.float32)
    B, S = int(B), int(S)
    padded = torch.zeros(torch_ops.crop_matrix_shape(B, S), dtype=torch.float32, device=device)
    padded[:S, :B] = shift_matrix_device64(B, S, delta, device).float()
    return padded


# ---- float32 operands, built once --------------------------------------------------------------------------------------------
_cache = {}


def _padded(m, shape, device):
    out = np.zeros(shape, dtype=np.float32)
    out[:m.shape[0], :m.shape[1]] = m
    return torch.from_numpy(out).to(device)


def operands(build64, args, shapes, device=None):
    """``build64(*args)``, one matrix or a tuple of them, rounded to float32.  Without a device: NumPy arrays.  With one:
    contiguous tensors there of ``shapes`` (one shape or a tuple) whose added rows and columns are exact zeros.  Built once
    per (build64, args, device)."""
    key = (build64, tuple(args), None if device is None else str(torch.device(device)))
    if key not in _cache:
        if device is None:
            m = build64(*args)
            _cache[key] = tuple(x.astype(np.float32) for x in m) if isinstance(m, tuple) else m.astype(np.float32)
        else:
            m = operands(build64, args, shapes)
            _cache[key] = (tuple(_padded(x, s, device) for x, s in zip(m, shapes)) if isinstance(m, tuple)
                           else _padded(m, shapes, device))
    return _cache[key]
