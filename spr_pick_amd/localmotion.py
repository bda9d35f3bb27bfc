"""Local (patch-wise) motion for ``joint align --patch PY,PX``.

Beam-induced motion is no rigid shift: the ice domes, and the corners of a frame move by pixels against its centre.  After
the whole-frame estimate (``align.estimate_shifts``) one smooth field per movie is fitted, MotionCor2's form: frame f is
pulled by

    E_f(u, v) = sum over k = 1 .. 3 of t_f^k q_k(u, v),    t_f = f / (Z - 1),

per axis, q_k a quadratic in the normalised coordinates u = j / nx - 1/2, v = i / ny - 1/2 of a pixel (``basis``: 1, u, v,
uu, uv, vv), 18 coefficients per axis; E_0 = 0, so the sum lives in frame 0's local geometry.

* ``estimate_field``: on the globally shifted reduced frames G_f.  Per iteration every frame is warped by the current field
  (``torch.ops.sprk.align_warp``), the reference of frame f is the sum of the OTHER warped frames, and the PY x PX patches of
  G_f (as they are) are cross-correlated with the same patches of their reference in one ``torch.ops.sprk.align_corr``
  launch over Z PY PX "frames".  Every iteration so measures the absolute field, as the global loop does, and no
  interpolation error accumulates.  ``fit_field`` then solves, per axis and in float64, for the 18 coefficients plus one
  offset per patch, the position of that patch's reference, which nothing observes and nothing applies.
* ``LocalMovie``: what ``align.sum_frames`` and ``dose.sum_frames_weighted`` use of a movie, with frame k shifted by its
  whole-frame estimate (``align_accumulate`` at full size) and then warped by E_k in raw pixels; both sums run unchanged on
  it with zero shifts, so ``--ftbin``, ``--dose`` and the ``--gain`` group compose without code of their own.

The warp interpolates with Catmull-Rom taps, whose transfer function at a half-pixel shift is 0.88 at half Nyquist and zero
at Nyquist; local motion finer than this one smooth field (per-particle polishing) is not covered."""
import logging

import numpy as np
import torch

from . import torch_ops

logger = logging.getLogger("joint.align")
MIN_PATCHES, MAX_PATCHES = 3, 16                 # per axis: a quadratic needs three positions
DEFAULT_PATCH_SHIFT, DEFAULT_PATCH_ITERS = 6, 4
ORDER, TERMS = 3, torch_ops.WARP_TERMS           # powers of t; terms of a quadratic in (u, v)
TOLERANCE = 0.01                                 # reduced pixels: the loop stops when no patch-centre value moves by this much
MAX_DROPPED = 0.25                               # of the observations: more peaks on a window border refuse the movie
MAX_FIELD = torch_ops.WARP_MAX_SHIFT


# ---- arguments and geometry ----------------------------------------------------------------------------------------------
def parse_patch(text):
    """``"PY,PX"`` -> (PY, PX)"""
    parts = str(text).split(",")
    try:
        if len(parts) != 2:
            raise ValueError
        return int(parts[0]), int(parts[1])
    except ValueError:
        raise ValueError("--patch takes PY,PX, two integers in %d..%d, got %r" % (MIN_PATCHES, MAX_PATCHES, text)) from None


def check_patch_args(patch, patch_shift=DEFAULT_PATCH_SHIFT, patch_iters=DEFAULT_PATCH_ITERS):
    """-> ((PY, PX), R, I), checked as ``align.check_align_args`` checks"""
    def integer(v):
        return not isinstance(v, bool) and isinstance(v, (int, np.integer))
    if not isinstance(patch, (tuple, list)) or len(patch) != 2 or not all(integer(v) for v in patch) \
            or not all(MIN_PATCHES <= v <= MAX_PATCHES for v in patch):
        raise ValueError("patch must be (PY, PX), two integers in %d..%d, got %r" % (MIN_PATCHES, MAX_PATCHES, patch))
    for name, v, lo, hi in (("patch_shift", patch_shift, 1, torch_ops.ALIGN_MAX_SHIFT), ("patch_iters", patch_iters, 1, 100)):
        if not integer(v) or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d..%d, got %r" % (name, lo, hi, v))
    return (int(patch[0]), int(patch[1])), int(patch_shift), int(patch_iters)


def patch_geometry(Sy, Sx, PY, PX, R):
    """The PY x PX patches laid over reduced frames of [Sy, Sx] -> {"ph", "pw", "y0" [PY], "x0" [PX], "v" [PY], "u" [PX]}.
    The patch width is the multiple of 64 nearest Sx / PX (halves go up), at least 64 (``align_corr``'s rule), the height
    round(Sy / PY); the first and the last patch are flush with the edges, the others evenly spaced (they may overlap).
    u, v: the normalised coordinates of the patch centres.  Refused: a patch larger than the frame, and a window of
    2R + 1 pixels that exceeds either side of a patch."""
    Sy, Sx, PY, PX, R = int(Sy), int(Sx), int(PY), int(PX), int(R)
    pw = max(64, 64 * ((2 * Sx + 64 * PX) // (128 * PX)))
    ph = max(1, (2 * Sy + PY) // (2 * PY))
    if pw > Sx or ph > Sy:
        raise ValueError("%dx%d patches of %dx%d do not fit the %dx%d reduced frames" % (PY, PX, ph, pw, Sy, Sx))
    if 2 * R + 1 > min(ph, pw):
        raise ValueError("a window of +-%d pixels does not fit the %dx%d patches of a %dx%d grid over %dx%d reduced frames "
                         "(fewer patches, a smaller --patch_shift or a larger --align_size)" % (R, ph, pw, PY, PX, Sy, Sx))
    y0 = np.array([(2 * n * (Sy - ph) + (PY - 1)) // (2 * (PY - 1)) for n in range(PY)])
    x0 = np.array([(2 * n * (Sx - pw) + (PX - 1)) // (2 * (PX - 1)) for n in range(PX)])
    return {"ph": ph, "pw": pw, "y0": y0, "x0": x0, "v": (y0 + 0.5 * (ph - 1)) / Sy - 0.5, "u": (x0 + 0.5 * (pw - 1)) / Sx - 0.5}


# ---- the field -------------------------------------------------------------------------------------------------------------
def basis(u, v):
    """-> [..., 6]: 1, u, v, uu, uv, vv, the order of ``align_warp``'s coefficients"""
    u, v = np.broadcast_arrays(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64))
    return np.stack([np.ones_like(u), u, v, u * u, u * v, v * v], axis=-1)


def frame_times(Z):
    return np.arange(Z) / (Z - 1.0)


def frame_coefficients(q, Z):
    """q [3, 6] (q_1 .. q_3 of one axis) -> [Z, 6]: the quadratic of every frame, sum over k of t_f^k q_k"""
    t = frame_times(Z)
    return np.stack([t ** k for k in range(1, ORDER + 1)], axis=1) @ np.asarray(q, dtype=np.float64)


def design(Z, u, v):
    """The observations' matrix, [Z P, 18 + P] for P = len(v) len(u) patches, rows in (frame, patch row, patch column)
    order: the value of patch n in frame f is sum_k t_f^k q_k(u_n, v_n) + o_n.  Columns k * 6 + term, then the offsets."""
    b = basis(np.asarray(u)[None, :], np.asarray(v)[:, None]).reshape(-1, TERMS)        # [P, 6]
    P = len(b)
    t = frame_times(Z)
    field = np.concatenate([(t ** k)[:, None, None] * b[None] for k in range(1, ORDER + 1)], axis=2)      # [Z, P, 18]
    offsets = np.broadcast_to(np.eye(P)[None], (Z, P, P))
    return np.concatenate([field, offsets], axis=2).reshape(Z * P, ORDER * TERMS + P)


def fit_field(A, m, keep):
    """A: ``design``; m [Z P] the measured values of one axis; keep [Z P] bool -> (q [3, 6], fitted [Z P]): least squares
    over the kept observations in float64"""
    sol = np.linalg.lstsq(A[keep], np.asarray(m, dtype=np.float64)[keep], rcond=None)[0]
    return sol[:ORDER * TERMS].reshape(ORDER, TERMS), A @ sol


# ---- the estimate ----------------------------------------------------------------------------------------------------------
def _cut(frames, geo):
    """frames [Z, Sy, Sx] -> contiguous [Z P, ph, pw], the mean of every patch taken out"""
    ph, pw = geo["ph"], geo["pw"]
    p = torch.stack([frames[:, y:y + ph, x:x + pw] for y in geo["y0"].tolist() for x in geo["x0"].tolist()], dim=1)
    p = p - p.mean(dim=(2, 3), keepdim=True)
    return p.reshape(-1, ph, pw).contiguous()


def warp_frames(G, cy, cx, out):
    """G [Z, ny, nx] float32 CUDA; cy, cx [Z, 6] -> out[f] = ``align_warp`` of G[f] by its quadratic"""
    for f in range(len(G)):
        torch.ops.sprk.align_warp(G[f], [float(c) for c in cy[f]], [float(c) for c in cx[f]], out[f], True)
    return out


def estimate_field(G, patch, patch_shift=DEFAULT_PATCH_SHIFT, patch_iters=DEFAULT_PATCH_ITERS, name=""):
    """G: float32 CUDA [Z, Sy, Sx], the reduced frames shifted by their whole-frame estimate -> (qy, qx, info): the
    coefficients [3, 6] per axis in reduced pixels, and {"iterations", "moved", "dropped", "geometry", "measured" [Z, P, 2],
    "fitted" [Z, P, 2]} ((y, x) in reduced pixels, the patch offsets included in both)."""
    from .align import fit_peaks
    Z, Sy, Sx = G.shape
    if Z < ORDER + 1:
        raise ValueError("%s: a cubic in time needs at least %d frames, the movie has %d" % (name, ORDER + 1, Z))
    (PY, PX), R, iters = check_patch_args(patch, patch_shift, patch_iters)
    geo = patch_geometry(Sy, Sx, PY, PX, R)
    A = design(Z, geo["u"], geo["v"])
    centres = A[:, :ORDER * TERMS]
    a = _cut(G, geo)
    qy, qx = np.zeros((ORDER, TERMS)), np.zeros((ORDER, TERMS))
    W = torch.empty_like(G)
    info = None
    for it in range(iters):
        warp_frames(G, frame_coefficients(qy, Z), frame_coefficients(qx, Z), W)
        refs = W.sum(dim=0, keepdim=True) - W
        py, px, edge = fit_peaks(torch.ops.sprk.align_corr(a, _cut(refs, geo), R, 0).cpu().numpy())
        dropped = int(edge.sum())
        if dropped:
            logger.warning("%s: local iteration %d: %d of %d correlation peaks sit on the border of the +-%d pixel window "
                           "and are left out of the fit (patch, frame): %s", name, it + 1, dropped, len(edge), R,
                           ", ".join("(%d, %d)" % (i % (PY * PX), i // (PY * PX)) for i in np.nonzero(edge)[0][:20]))
        if dropped > MAX_DROPPED * len(edge):
            raise ValueError("%s: %d of %d patch correlations peak on the border of the +-%d pixel window: no local field is "
                             "fitted to that (a larger --patch_shift, fewer patches, or no --patch)"
                             % (name, dropped, len(edge), R))
        new_y, fit_y = fit_field(A, -py, ~edge)                  # a patch displaced by d peaks at -d: the pull is d
        new_x, fit_x = fit_field(A, -px, ~edge)
        moved = float(max(np.abs(centres @ (new_y - qy).ravel()).max(), np.abs(centres @ (new_x - qx).ravel()).max()))
        qy, qx = new_y, new_x
        info = {"iterations": it + 1, "moved": moved, "dropped": dropped, "geometry": geo,
                "measured": np.stack([-py, -px], axis=1).reshape(Z, PY * PX, 2),
                "fitted": np.stack([fit_y, fit_x], axis=1).reshape(Z, PY * PX, 2)}
        if moved < TOLERANCE:
            break
    return qy, qx, info


def field_extreme(q, Z):
    """the largest |E_f| of one axis over the frames, on a 33 x 33 grid of the frame (float64)"""
    g = np.linspace(-0.5, 0.5, 33)
    return float(np.abs(basis(g[None, :], g[:, None]).reshape(-1, TERMS) @ frame_coefficients(q, Z).T).max())


# ---- the corrected movie -----------------------------------------------------------------------------------------------------
class LocalMovie:
    """What ``align.sum_frames`` and ``dose.sum_frames_weighted`` use of an ``align.Movie`` (or a
    ``moviefix.CorrectedMovie``): ``frame(k)`` is frame k shifted by (shifts_y[k], shifts_x[k]) raw pixels
    (``align_accumulate`` at full size) and warped by E_k (``align_warp``; qy, qx [3, 6] in raw pixels), float32, as its
    bytes.  The anchor of an integer movie stays out of the interpolation: the frames here are samples minus the anchor,
    ``anchor`` is 0, and ``anchor_term`` is what the caller adds to a sum of them."""

    def __init__(self, movie, shifts_y, shifts_x, qy, qx):
        self.movie = movie
        self.header = movie.header._replace(mode=2)
        self.anchor = 0.0
        self._reader = movie._reader
        self.shifts_y, self.shifts_x = shifts_y, shifts_x
        Z = movie.header.nz
        self.cy, self.cx = frame_coefficients(qy, Z), frame_coefficients(qx, Z)
        for axis, q in (("y", qy), ("x", qx)):
            if field_extreme(q, Z) > MAX_FIELD:
                logger.warning("%s: the fitted local field reaches %.1f raw pixels along %s; it is applied clamped to +-%d",
                               getattr(movie, "path", "movie"), field_extreme(q, Z), axis, MAX_FIELD)

    @property
    def anchor_term(self):
        h = self.movie.header
        return 0.0 if h.mode == 2 else float(np.float32(h.nz * self.movie.anchor))

    def frame(self, k):
        from .align import shift_matrix
        h = self.movie.header
        raw = self.movie.frame(k)
        dev = raw.device
        shifted = torch.empty((h.ny, h.nx), dtype=torch.float32, device=dev)
        torch.ops.sprk.align_accumulate(raw, h.mode, h.ny, h.nx, h.ny, h.nx, shift_matrix(h.ny, h.ny, self.shifts_y[k], dev),
                                        shift_matrix(h.nx, h.nx, self.shifts_x[k], dev), self.movie.anchor, shifted, True)
        out = torch.empty_like(shifted)
        torch.ops.sprk.align_warp(shifted, [float(c) for c in self.cy[k]], [float(c) for c in self.cx[k]], out, True)
        return out.view(torch.uint8).reshape(-1)


# ---- the report --------------------------------------------------------------------------------------------------------------
def write_local(path, local):
    """``{name}_local.txt``: the 2 x 18 coefficients in raw pixels, the patch grid, the count of dropped observations and,
    per patch and frame, the measured and the fitted pull (dx, dy) in raw pixels, the patch's offset included in both."""
    geo, (PY, PX) = local["geometry"], local["patch"]
    lines = ["# local motion: frame f is pulled by E_f(u, v) = sum_k t^k q_k(u, v), t = f / (Z - 1), u = x / nx - 1/2, "
             "v = y / ny - 1/2; raw pixels",
             "patches\t%d\t%d" % (PY, PX),
             "patch_size\t%d\t%d\t# rows, columns, pixels of the %dx%d reduced frames" % (geo["ph"], geo["pw"], *local["reduced"]),
             "patch_rows\t" + "\t".join(str(int(v)) for v in geo["y0"]),
             "patch_columns\t" + "\t".join(str(int(v)) for v in geo["x0"]),
             "iterations\t%d" % local["iterations"], "dropped\t%d" % local["dropped"],
             "axis\tk\tc_1\tc_u\tc_v\tc_uu\tc_uv\tc_vv"]
    for axis in ("x", "y"):
        for k in range(ORDER):
            lines.append("%s\t%d\t" % (axis, k + 1) + "\t".join("%.6f" % c for c in local["q" + axis][k]))
    lines.append("patch\tframe\tmeasured_dx\tmeasured_dy\tfitted_dx\tfitted_dy")
    Z, P, _ = local["measured"].shape
    for n in range(P):
        for f in range(Z):
            (my, mx), (fy, fx) = local["measured"][f, n], local["fitted"][f, n]
            lines.append("%d\t%d\t%.4f\t%.4f\t%.4f\t%.4f" % (n, f, mx, my, fx, fy))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
