"""Raw detector movies in: gain and dark references, defect lists and hot pixels for ``joint align``.

A movie as a detector writes it carries a fixed pattern, the same in every frame: the gain of every pixel, a dark offset,
dead columns, listed defect rectangles and hot pixels.  A fixed pattern correlates with itself at shift zero, and the
estimate of ``align.estimate_shifts`` then stays there.  Here it is taken out before anything else sees a frame:

* ``torch.ops.sprk.movie_correct`` (csrc/moviefix.hip), one launch per frame: c = (sample - dark) * gain, and every pixel
  the fix map marks replaced by the mean of the good pixels around it;
* the fix map (``build_fix``): 0 where the pixel is good, else the radius of the smallest window that holds a good one.
  Bad are the pixels whose gain is not finite or not positive, the pixels of the defect rectangles (``static_bad``) and,
  with ``hot_sigma``, the pixels of the corrected movie's plain sum that stand out (``detect_hot``);
* ``CorrectedMovie`` hands the corrected frames, float32, to ``align.align_movie``, ``align.sum_frames`` and
  ``dose.sum_frames_weighted`` in place of the ``align.Movie`` it wraps.

The correction multiplies by the gain reference; a reference meant to be divided by is not covered.  Everything here but
the kernel runs once per movie or once per run."""
import io
import struct

import numpy as np
import torch

from . import micrograph_io, torch_ops

FIX_MAX_RADIUS = torch_ops.FIX_MAX_RADIUS
HOT_ROUNDS = 4
GAIN_ROTS, GAIN_FLIPS = (0, 1, 2, 3), ("ud", "lr")


# ---- arguments and files ---------------------------------------------------------------------------------------------------
def check_fix_args(gain=None, gain_rot=0, gain_flip=None, dark=None, defects=None, hot_sigma=None):
    """-> True when any of them asks for a correction"""
    if isinstance(gain_rot, bool) or gain_rot not in GAIN_ROTS:
        raise ValueError("gain_rot must be one of %s (quarter turns of np.rot90), got %r" % (GAIN_ROTS, gain_rot))
    if gain_flip is not None and gain_flip not in GAIN_FLIPS:
        raise ValueError("gain_flip must be one of %s, got %r" % (GAIN_FLIPS, gain_flip))
    if gain is None and (gain_rot != 0 or gain_flip is not None):
        raise ValueError("gain_rot and gain_flip turn the gain reference: give gain as well")
    if hot_sigma is not None:
        if isinstance(hot_sigma, bool) or not isinstance(hot_sigma, (int, float, np.integer, np.floating)) \
                or not np.isfinite(hot_sigma) or not hot_sigma > 0:
            raise ValueError("hot_sigma must be a finite number above 0, got %r" % (hot_sigma,))
    return gain is not None or dark is not None or defects is not None or hot_sigma is not None


def read_reference(path, ny, nx, rot=0, flip=None):
    """A gain or dark reference: a single-image MRC of mode 0 / 1 / 2 / 6 -> float32 [ny, nx], turned by ``np.rot90(g, rot)``
    first and then flipped (``"ud"``: ``np.flipud``, ``"lr"``: ``np.fliplr``).  Refused unless the result is [ny, nx]."""
    check_fix_args(path, rot, flip)
    with open(path, "rb") as f:
        array, header, _ = micrograph_io.parse_mrc(f.read())
    if header.nz != 1 or array.ndim != 2:
        raise ValueError("%s: expected a single image, got shape %s" % (path, (header.nz, header.ny, header.nx)))
    if array.size != header.ny * header.nx:
        raise ValueError("%s: %d samples, the header promises %d" % (path, array.size, header.ny * header.nx))
    g = np.rot90(array.astype(np.float32), rot)
    if flip is not None:
        g = np.flipud(g) if flip == "ud" else np.fliplr(g)
    if g.shape != (ny, nx):
        raise ValueError("%s: a reference of %dx%d%s, the frames are %dx%d"
                         % (path, g.shape[0], g.shape[1], " after the turn" if rot % 2 else "", ny, nx))
    return np.ascontiguousarray(g)


def read_defects(path, ny, nx):
    """A defect file in MotionCor2's layout: every line that is not empty and does not start with ``#`` holds four integers
    ``x y w h``, x the column and y the row of the rectangle's first sample as stored -> bool [ny, nx]."""
    bad = np.zeros((ny, nx), dtype=bool)
    with open(path) as f:
        for number, line in enumerate(f, 1):
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            try:
                x, y, w, h = (int(v) for v in line.split())
            except ValueError:
                raise ValueError("%s, line %d: expected four integers x y w h, got %r" % (path, number, line)) from None
            if w < 1 or h < 1 or x < 0 or y < 0 or x + w > nx or y + h > ny:
                raise ValueError("%s, line %d: the rectangle x %d y %d w %d h %d leaves the %dx%d frame (nx %d, ny %d)"
                                 % (path, number, x, y, w, h, ny, nx, nx, ny))
            bad[y:y + h, x:x + w] = True
    return bad


class References:
    """The references of one run: read and uploaded at the first movie, and checked against every later movie's frames."""

    def __init__(self, gain=None, gain_rot=0, gain_flip=None, dark=None, defects=None, hot_sigma=None):
        self.active = check_fix_args(gain, gain_rot, gain_flip, dark, defects, hot_sigma)
        self.paths = (gain, gain_rot, gain_flip, dark, defects)
        self.hot_sigma = None if hot_sigma is None else float(hot_sigma)
        self._shape, self._tensors = None, None

    def for_frames(self, ny, nx, device):
        """-> (gain, dark, defects): float32 / float32 / bool tensors [ny, nx] on ``device``, or None each"""
        if self._shape is None:
            gain, rot, flip, dark, defects = self.paths
            g = None if gain is None else torch.from_numpy(read_reference(gain, ny, nx, rot, flip)).to(device)
            d = None if dark is None else torch.from_numpy(read_reference(dark, ny, nx)).to(device)
            b = None if defects is None else torch.from_numpy(read_defects(defects, ny, nx)).to(device)
            self._shape, self._tensors = (ny, nx), (g, d, b)
        if self._shape != (ny, nx):
            raise ValueError("frames of %dx%d, the references of this run were read for %dx%d" % (ny, nx, *self._shape))
        return self._tensors


# ---- the fix map -----------------------------------------------------------------------------------------------------------
def static_bad(gain, defects):
    """gain float32 [ny, nx] or None, defects bool [ny, nx] or None (tensors on one device) -> bool [ny, nx]: the gain is
    not finite or is <= 0, or a rectangle covers the pixel.  None when both are None."""
    if gain is None:
        return None if defects is None else defects.clone()
    bad = ~torch.isfinite(gain) | ~(gain > 0)
    return bad if defects is None else bad | defects


def build_fix(bad):
    """bad: bool tensor [ny, nx] (CPU or CUDA) -> uint8 [ny, nx]: 0 where good, otherwise the smallest r in 1 ..
    ``FIX_MAX_RADIUS`` whose window, clamped to the frame, holds a good pixel.  A bad pixel without one raises."""
    if bad.dtype != torch.bool or bad.dim() != 2:
        raise ValueError("build_fix: a bool [ny, nx] tensor, got %s %s" % (bad.dtype, tuple(bad.shape)))
    good = (~bad).to(torch.float32)[None, None]
    fix = torch.zeros(bad.shape, dtype=torch.uint8, device=bad.device)
    for r in range(FIX_MAX_RADIUS, 0, -1):                       # descending: the smallest radius is written last
        reach = torch.nn.functional.max_pool2d(good, 2 * r + 1, 1, r)[0, 0] > 0
        fix[bad & reach] = r
    lost = bad & (fix == 0)
    count = int(lost.sum())
    if count:
        y, x = (int(v) for v in torch.nonzero(lost)[0])
        raise ValueError("%d bad pixel(s) without a good one within %d pixels, the first at row %d, column %d"
                         % (count, FIX_MAX_RADIUS, y, x))
    return fix


def detect_hot(T, bad, sigma):
    """T [ny, nx] (the plain sum of the corrected frames), bad bool [ny, nx] (tensors on one device) -> bad with the hot
    pixels added, a new tensor.  Per round, over the pixels not bad so far, in float64: mu the mean, sd the population
    standard deviation; new = ~bad & (T > mu + sigma * sd).  It stops when a round finds nothing new, after ``HOT_ROUNDS``
    at most: the first round's sd is inflated by the hot pixels themselves, the second round finds what that hid."""
    T = T.to(torch.float64)
    bad = bad.clone()
    for _ in range(HOT_ROUNDS):
        v = T[~bad]
        if v.numel() == 0:
            break
        mu, sd = v.mean(), v.std(unbiased=False)
        new = ~bad & (T > mu + float(sigma) * sd)
        if not bool(new.any()):
            break
        bad |= new
    return bad


# ---- the corrected movie -----------------------------------------------------------------------------------------------------
class CorrectedMovie:
    """What ``align.align_movie``, ``align.sum_frames`` and ``dose.sum_frames_weighted`` use of an ``align.Movie``, with
    corrected frames: ``frame(k)`` is a fresh float32 frame from ``movie_correct``, as its bytes.  The raw frames stay
    resident as the movie keeps them; corrected ones are not cached (a frame is used two or three times, and the correction
    is small beside the GEMMs that follow)."""

    def __init__(self, movie, gain, dark, fix):
        self.movie = movie
        self.raw_header = movie.header
        self.header = movie.header._replace(mode=2)
        self.anchor = 0.0
        self.gain, self.dark, self.fix = gain, dark, fix
        self._reader = movie._reader

    def corrected(self, k, out=None, total=None, first=True):
        h = self.raw_header
        raw = self.movie.frame(k)
        if out is None:
            out = torch.empty((h.ny, h.nx), dtype=torch.float32, device=raw.device)
        torch.ops.sprk.movie_correct(raw, h.mode, h.ny, h.nx, self.gain, self.dark, self.fix, out, total, first)
        return out

    def frame(self, k):
        return self.corrected(k).view(torch.uint8).reshape(-1)


def prepare(movie, gain, dark, defects, hot_sigma=None):
    """movie: an ``align.Movie``; gain, dark float32 and defects bool, [ny, nx] on the movie's device, or None ->
    (CorrectedMovie, {"static": bad pixels of the references, "hot": hot pixels found, "fix": the uint8 map}).  With
    ``hot_sigma`` one pass over all frames forms their plain sum under the static map, ``detect_hot`` reads it, and the map
    is built again with what it found."""
    h = movie.header
    dev = movie._reader.device
    bad = static_bad(gain, defects)
    if bad is None:
        bad = torch.zeros((h.ny, h.nx), dtype=torch.bool, device=dev)
    if tuple(bad.shape) != (h.ny, h.nx):
        raise ValueError("references of %dx%d for frames of %dx%d" % (*bad.shape, h.ny, h.nx))
    n_static = int(bad.sum())
    fix = build_fix(bad)
    n_hot = 0
    if hot_sigma is not None:
        first = CorrectedMovie(movie, gain, dark, fix if n_static else None)
        total = torch.empty((h.ny, h.nx), dtype=torch.float32, device=dev)
        out = torch.empty_like(total)
        for k in range(h.nz):
            first.corrected(k, out, total, k == 0)
        found = detect_hot(total, bad, hot_sigma)
        n_hot = int(found.sum()) - n_static
        if n_hot:
            fix = build_fix(found)
    return (CorrectedMovie(movie, gain, dark, fix if n_static + n_hot else None),
            {"static": n_static, "hot": n_hot, "fix": fix})


def write_fix_map(path, fix):
    """The fix map as a mode 0 (int8) MRC image"""
    fix = np.ascontiguousarray(fix, dtype=np.int8)
    buf = io.BytesIO()
    micrograph_io.write_mrc(buf, fix.astype(np.float32))
    head = bytearray(buf.getvalue()[:1024])
    struct.pack_into("<i", head, 12, 0)
    with open(path, "wb") as f:
        f.write(bytes(head))
        f.write(fix.tobytes())
