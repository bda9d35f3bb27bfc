"""``joint align``: whole-frame motion correction of movies on the device — the step before ``joint bin`` /
``joint eval --bin`` / ``joint ctf`` / ``joint extract``, in place of a MotionCor2 or ``relion_motioncorr`` run.

A movie is an MRC stack (or a TIFF, below) of Z >= 2 short-exposure frames (modes 0 / 1 / 2 / 6): gain-corrected, or as the detector wrote it
together with its references (``gain``, ``dark``, ``defects``, ``hot_sigma``; ``joint align --gain ...``): every frame then
passes ``torch.ops.sprk.movie_correct`` first (``moviefix.CorrectedMovie``), and what follows sees float32
frames whose fixed pattern is gone.  Per movie:

* every frame is uploaded through two pinned slots (``MovieReader``) and Fourier-cropped to about ``align_size`` pixels a
  side (``align_geometry``; ``torch.ops.sprk.ingest_resample``), its mean taken out;
* the shifts are estimated on the reduced frames (``estimate_shifts``): each frame, as it is, is cross-correlated
  (``torch.ops.sprk.align_corr``, a window of +-``max_shift`` reduced pixels) with the sum of the OTHER frames shifted by
  the current estimate (``torch.ops.sprk.align_accumulate`` with the matrices of ``shift_matrix``); the peak of every
  window, refined by a three-point parabola per axis, is the new estimate; the mean over the frames is taken out;
* the raw frames are shifted by the estimate, summed and (``ftbin``) Fourier-cropped in one pass, ``align_accumulate`` per
  frame: Y = sum_f My_f D_f Mx_f^T with one fp32 accumulator chain per pixel that runs on through the frames.

A sub-pixel shift with periodic edges is the same kind of operator as the Fourier crop: the real matrix
``shift_matrix64`` = (S/B) IDFT_S . crop . diag(e^{-2 pi i k delta / B}) . DFT_B per axis.  What leaves a frame at one edge
wraps round to the other, as in every Fourier shift; nothing is tapered.

With a dose per frame (``dose``; ``joint align --dose``) a second, dose-weighted sum is formed beside the plain one, in
Fourier space (``dose.sum_frames_weighted``); the plain sum and the shifts are what they are without it.

With ``patch`` (``joint align --patch PY,PX``) one smooth local field per movie is fitted after the whole-frame estimate and
every frame is warped by it before it is summed (``localmotion``): ``torch.ops.sprk.align_warp``.

A movie may also be a multi-page TIFF (``.tif`` / ``.tiff``: stored or LZW strips, as SerialEM and EPU write them; ``tiffio``,
DESIGN §4.3o): its strips are uploaded as they lie in the file and decoded on the device (``torch.ops.sprk.tiff_decode``)
into the sample block an MRC frame is, and everything after that is the same.

Out of scope: local motion finer than that one smooth field (per-particle polishing), EER input, TIFF with another
compression, a predictor or tiles, TIFF references, and gain references meant to be divided by.

Coordinates and signs: x runs along nx (columns), y along ny (rows).  ``{name}_shifts.txt`` lists, per frame, the
displacement (dx, dy) of the frame's content in raw pixels against the movie's mean position (mean zero over the frames);
the sum applies its negative."""
import io
import logging
import os

import numpy as np
import torch

from . import ingest, micrograph_io, torch_ops
from .fourier import shift_matrix, shift_matrix64, shift_matrix_device64      # the shift-and-crop operator

logger = logging.getLogger("joint.align")
MAX_SHIFT = torch_ops.ALIGN_MAX_SHIFT
DEFAULT_ALIGN_SIZE, DEFAULT_MAX_SHIFT, DEFAULT_ITERS = 1024, 16, 6
TOLERANCE = 0.01                                 # reduced pixels: the loop stops when no component moves by this much
RESIDENT_BYTES = 8 << 30                         # frames of a movie below this size stay on the device for the second pass


# ---- arguments and geometry ----------------------------------------------------------------------------------------------
def check_align_args(align_size, max_shift, iters):
    for name, v, lo, hi in (("align_size", align_size, 64, ingest.MAX_SIDE), ("max_shift", max_shift, 1, MAX_SHIFT),
                            ("iters", iters, 1, 100)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d..%d, got %r" % (name, lo, hi, v))
    return int(align_size), int(max_shift), int(iters)


def align_geometry(ny, nx, align_size=DEFAULT_ALIGN_SIZE):
    """-> (Sy, Sx): the size of the reduced frames the shifts are estimated on.  Sx is the multiple of 64 nearest
    nx * A / max(ny, nx) (halves go up), at least 64 and at most nx; Sy = round(ny * Sx / nx), at most ny.  A shift of one
    reduced pixel is ny / Sy raw pixels along y and nx / Sx along x."""
    ny, nx, A = int(ny), int(nx), int(align_size)
    if not (64 <= nx <= ingest.MAX_SIDE and 2 <= ny <= ingest.MAX_SIDE):
        raise ValueError("a %dx%d frame: 64 <= nx <= %d and 2 <= ny <= %d" % (ny, nx, ingest.MAX_SIDE, ingest.MAX_SIDE))
    if A < 64:
        raise ValueError("align_size must be at least 64, got %d" % A)
    m = max(ny, nx)
    Sx = 64 * ((2 * nx * A + 64 * m) // (128 * m))            # floor(nx A / (64 m) + 1/2) in integers
    Sx = min(max(Sx, 64), nx // 64 * 64)
    Sy = min(max((2 * ny * Sx + nx) // (2 * nx), 2), ny)
    return Sy, Sx


# ---- the estimate ----------------------------------------------------------------------------------------------------------
def fit_peaks(cc):
    """cc [Z, 2R+1, 2R+1] correlation windows -> (py, px, edge): the position of each window's maximum in pixels from its
    centre, float64 [Z], refined per axis by the parabola through the maximum and its two neighbours; ``edge`` [Z] bool:
    the maximum sits on the window's border (its index is clamped to the interior before the fit)."""
    cc = np.asarray(cc, dtype=np.float64)
    Z, n, n2 = cc.shape
    if n != n2 or n < 3 or n % 2 == 0:
        raise ValueError("fit_peaks: windows of %dx%d (odd and square, at least 3)" % (n, n2))
    R = (n - 1) // 2
    iy, ix = np.unravel_index(cc.reshape(Z, -1).argmax(axis=1), (n, n))
    edge = (iy == 0) | (iy == n - 1) | (ix == 0) | (ix == n - 1)
    iy, ix = np.clip(iy, 1, n - 2), np.clip(ix, 1, n - 2)
    f = np.arange(Z)

    def vertex(lo, c, hi):
        curv = lo - 2.0 * c + hi
        with np.errstate(divide="ignore", invalid="ignore"):
            off = np.where(curv < 0, 0.5 * (lo - hi) / curv, 0.0)
        return np.clip(off, -0.5, 0.5)

    c = cc[f, iy, ix]
    py = iy - R + vertex(cc[f, iy - 1, ix], c, cc[f, iy + 1, ix])
    px = ix - R + vertex(cc[f, iy, ix - 1], c, cc[f, iy, ix + 1])
    return py, px, edge


def _flat_bytes(t):
    return t.view(torch.uint8).reshape(-1)


def estimate_shifts(reduced, max_shift=DEFAULT_MAX_SHIFT, iters=DEFAULT_ITERS, name=""):
    """reduced: float32 CUDA [Z, Sy, Sx], every frame's mean taken out -> (sy, sx, info): the shift of every frame, in
    reduced pixels, that lays it on the others (mean zero over the frames; float64 [Z]), and {"iterations", "edge_frames",
    "moved"}.  Each iteration correlates the frames as they are with the sum of the other frames shifted by the current
    estimate; a frame is left out of its own reference (its noise correlates with itself at shift zero and pulls the
    estimate there)."""
    Z, Sy, Sx = reduced.shape
    R = int(max_shift)
    dev = reduced.device
    sy, sx = np.zeros(Z), np.zeros(Z)
    shifted = torch.empty_like(reduced)
    info = {"iterations": 0, "edge_frames": [], "moved": None}
    for it in range(int(iters)):
        for f in range(Z):
            torch.ops.sprk.align_accumulate(_flat_bytes(reduced[f]), 2, Sy, Sx, Sy, Sx, shift_matrix(Sy, Sy, sy[f], dev),
                                            shift_matrix(Sx, Sx, sx[f], dev), 0.0, shifted[f], True)
        refs = shifted.sum(dim=0, keepdim=True) - shifted
        cc = torch.ops.sprk.align_corr(reduced, refs, R, 0).cpu().numpy()
        py, px, edge = fit_peaks(cc)
        py, px = py - py.mean(), px - px.mean()
        moved = float(max(np.abs(py - sy).max(), np.abs(px - sx).max()))
        sy, sx = py, px
        info = {"iterations": it + 1, "edge_frames": [int(f) for f in np.nonzero(edge)[0]], "moved": moved}
        if edge.any():
            logger.warning("%s: iteration %d: the correlation peak of frame(s) %s sits on the edge of the +-%d pixel window; "
                           "the clamped position is used (a larger --max_shift or a smaller --align_size reaches further)",
                           name, it + 1, ", ".join(str(f) for f in info["edge_frames"]), R)
        if moved < TOLERANCE:
            break
    return sy, sx, info


# ---- movies ----------------------------------------------------------------------------------------------------------------
def read_movie_header(path, f):
    """The 1024-byte MRC header of an open movie -> (MRCHeader, byte offset of frame 0).  ``ingest.read_header``'s refusals,
    with the one about stacks turned round: a single image is refused."""
    head = f.read(ingest._HEADER_BYTES)
    if len(head) < ingest._HEADER_BYTES:
        raise ValueError("MRC file shorter than its 1024-byte header")
    header = micrograph_io.MRCHeader._make(micrograph_io._HEADER.unpack(head))
    if header.mode not in micrograph_io._MODES:
        raise ValueError("Unsupported MRC mode: %d" % header.mode)
    if header.nz < 2:
        raise ValueError("%s: expected a movie, a stack of at least 2 frames, got shape %s"
                         % (path, (header.nz, header.ny, header.nx)))
    if header.ny < 1 or header.nx < 1 or header.next < 0:
        raise ValueError("%s: bad MRC header (nx %d, ny %d, next %d)" % (path, header.nx, header.ny, header.next))
    if header.ny > ingest.MAX_SIDE or header.nx > ingest.MAX_SIDE:
        raise ValueError("%s: frames of %dx%d are larger than joint align takes (%d a side)"
                         % (path, header.ny, header.nx, ingest.MAX_SIDE))
    return header, ingest._HEADER_BYTES + header.next


class MovieReader(ingest.RawReader):
    """``ingest.RawReader`` for the frames of a stack: frame k of an open file through the two pinned slots, so that the
    read of frame k+1 overlaps the upload and the GEMMs of frame k."""

    def read_frame(self, f, path, start, nbytes, k):
        """-> (uint8 CUDA tensor with frame k's ny*nx samples, the first ``nbytes`` of the pinned slot as a NumPy view,
        valid until the slot is used again: two reads later)"""
        return self.read_range(f, path, start + k * nbytes, nbytes, k, "of samples, the header promises")

    def read_range(self, f, path, offset, nbytes, k, what="of strips, the directory of the frame promises"):
        """``nbytes`` bytes of the file from ``offset`` on, frame k's -> as ``read_frame``"""
        slot = self._slot(nbytes)
        f.seek(offset)
        host = self._bufs[slot].numpy()[:nbytes]
        got = f.readinto(memoryview(host))
        if got != nbytes:
            raise ValueError("%s: frame %d has %d bytes %s %d" % (path, k, got, what, nbytes))
        raw = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        raw.copy_(self._bufs[slot][:nbytes], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._events[slot] = ev
        return raw, host


TIFF_EXTS = (".tif", ".tiff")


def is_tiff(path):
    return os.path.splitext(path)[1].lower() in TIFF_EXTS


def require_movie(path):
    """a TIFF movie (``tiffio``), or what ``ingest.require_mrc`` lets pass"""
    if not is_tiff(path):
        ingest.require_mrc(path)


def tiff_header(t):
    """The MRC header a TIFF movie would have: its size, the mapped mode and, when the file states a pixel size, the cell
    of that sampling; without one, the header of an MRC movie that states none."""
    buf = io.BytesIO()
    micrograph_io.write_mrc(buf, np.zeros((1, 1, 1), dtype=np.float32))
    h = micrograph_io.MRCHeader._make(micrograph_io._HEADER.unpack(buf.getvalue()[:1024]))
    h = h._replace(nx=t.nx, ny=t.ny, nz=t.frames, mode=t.mode, mx=t.nx, my=t.ny, mz=t.frames, xlen=0.0, ylen=0.0, zlen=0.0)
    if t.apix is not None:
        h = h._replace(xlen=float(np.float32(t.apix * t.nx)), ylen=float(np.float32(t.apix * t.ny)),
                       zlen=float(np.float32(t.apix * t.frames)))
    return h


class Movie:
    """An open MRC movie: ``frame(k)`` -> the uint8 CUDA tensor of frame k's samples.  The frames stay on the device after
    their first read when the whole movie is at most ``resident_bytes``; they are read again from the file otherwise.
    ``anchor``: the first sample of frame 0 (0.0 for float32), known on the host without a device read.
    ``open_movie`` opens a path as this or, for a TIFF, as ``TiffMovie``, which differs in ``_open`` and ``_read`` only."""

    def __init__(self, path, device="cuda", resident_bytes=RESIDENT_BYTES):
        self._require(path)
        self.path = path
        self._reader = MovieReader(device)
        self._f = open(path, "rb")
        try:
            self._open()
        except Exception:
            self._f.close()
            raise
        h = self.header
        self.dtype = np.dtype(micrograph_io._MODES[h.mode])
        self.frame_bytes = h.ny * h.nx * self.dtype.itemsize
        self.resident = h.nz * self.frame_bytes <= resident_bytes
        self._frames = [None] * h.nz

    @staticmethod
    def _require(path):
        ingest.require_mrc(path)

    def _open(self):
        self.header, self._start = read_movie_header(self.path, self._f)
        self.anchor = None

    def _read(self, k):
        raw, host = self._reader.read_frame(self._f, self.path, self._start, self.frame_bytes, k)
        if k == 0 and self.anchor is None:
            self.anchor = 0.0 if self.header.mode == 2 else float(host[:self.dtype.itemsize].view(self.dtype)[0])
        return raw

    def verify(self):
        """Raises when frames read so far were damaged in a way only the device could see (``TiffMovie``); MRC: nothing."""

    def frame(self, k):
        if self._frames[k] is not None:
            return self._frames[k]
        raw = self._read(k)
        if self.resident:
            self._frames[k] = raw
        return raw

    def close(self):
        self._frames = []
        self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class TiffMovie(Movie):
    """An open TIFF movie (``.tif`` / ``.tiff``; ``tiffio``): ``tiff`` is its ``tiffio.TiffMovie``, ``header``
    the MRC header it would have, and ``frame(k)`` uploads the frame's strips as they lie in the file and decodes them on
    the device (``torch.ops.sprk.tiff_decode``) into the sample block an MRC frame is.  Residency counts decoded bytes.
    ``verify()`` raises when a strip of the frames decoded so far did not decode."""

    @staticmethod
    def _require(path):
        if not is_tiff(path):
            raise ValueError("%s: not a TIFF movie (.tif / .tiff)" % path)

    def _open(self):
        from . import tiffio
        t = self.tiff = tiffio.read_tiff_movie(self.path, self._f)
        self.header = tiff_header(t)
        self.anchor = 0.0 if t.mode == 2 else tiffio.first_sample(t, self._f)
        # per frame: the byte range from the lowest strip offset to the highest strip end, and the strips within it
        self._lo = [int(o.min()) for o in t.strip_offsets]
        self._span = [int((o + n).max()) - lo for o, n, lo in zip(t.strip_offsets, t.strip_lengths, self._lo)]
        tables = np.stack([np.stack([o - lo, n, tiffio.strip_bytes(t)]) for o, n, lo in
                           zip(t.strip_offsets, t.strip_lengths, self._lo)])
        self._tables = torch.from_numpy(tables).to(self._reader.device)                  # int64 [Z, 3, n_strips], once
        self._status = torch.zeros((t.frames, len(t.strip_rows)), dtype=torch.int32, device=self._reader.device)
        if len(t.strip_rows) == 1 and t.compression == tiffio.LZW:
            logger.warning("%s: every frame is one LZW strip (the writer's RowsPerStrip is %d for %d rows): a strip is decoded "
                           "by one wave, so each frame decodes serially; strips of 1 to 8 rows decode in parallel",
                           self.path, t.rows_per_strip, t.ny)

    def _read(self, k):
        t = self.tiff
        src, _ = self._reader.read_range(self._f, self.path, self._lo[k], max(self._span[k], 1), k)
        out = torch.empty(self.frame_bytes, dtype=torch.uint8, device=self._reader.device)
        off, length, size = self._tables[k]
        torch.ops.sprk.tiff_decode(src, off, length, size, t.compression, t.widen, out, self._status[k])
        return out

    def verify(self):
        """Raises ValueError naming the first strip of the frames decoded so far whose stream was damaged."""
        bad = torch.nonzero(self._status).cpu().numpy()
        if len(bad):
            k, s = (int(v) for v in bad[0])
            why = {1: "holds a code that is not in the table", 2: "ends before the strip's rows are complete",
                   3: "decodes to more bytes than the strip's rows hold"}[int(self._status[k, s])]
            raise ValueError("%s: frame %d, strip %d: the LZW stream %s (%d strip(s) of the movie are damaged): the file is "
                             "corrupt, copy or write it again" % (self.path, k, s, why, len(bad)))


def open_movie(path, device="cuda", resident_bytes=RESIDENT_BYTES):
    """By extension: ``.tif`` / ``.tiff`` (any case) a ``TiffMovie``, everything else what ``Movie`` makes of it"""
    return (TiffMovie if is_tiff(path) else Movie)(path, device, resident_bytes)


def sum_frames(movie, by, bx, shifts_y, shifts_x):
    """-> float32 CUDA [by, bx]: sum over the frames of (frame f shifted by (shifts_y[f], shifts_x[f]) raw pixels and
    Fourier-cropped to by x bx), ``align_accumulate`` per frame and the anchor term at the end (one fp32 add: the rows of
    every matrix sum to 1)."""
    h = movie.header
    dev = movie._reader.device
    y = torch.empty((by, bx), dtype=torch.float32, device=dev)
    for k in range(h.nz):
        raw = movie.frame(k)
        torch.ops.sprk.align_accumulate(raw, h.mode, h.ny, h.nx, by, bx, shift_matrix(h.ny, by, shifts_y[k], dev),
                                        shift_matrix(h.nx, bx, shifts_x[k], dev), movie.anchor, y, k == 0)
    if h.mode != 2:
        y += float(np.float32(h.nz * movie.anchor))
    return y


def _dose_args(dose, pre_dose, kv, apix):
    """None without a dose (the other three must then be at their defaults), else the checked (dose, pre_dose, kv, apix)"""
    if dose is None:
        if pre_dose != 0.0 or kv != 300.0 or apix is not None:
            raise ValueError("pre_dose, kv and apix belong to the dose weighting: give dose as well")
        return None
    from . import dose as dose_mod
    return dose_mod.check_dose_args(dose, pre_dose, kv, apix)


def _references(gain, gain_rot, gain_flip, dark, defects, hot_sigma):
    """None when every one of them is at its default (``moviefix`` is then not even imported), else the checked
    ``moviefix.References`` of a run"""
    if gain is None and gain_rot == 0 and gain_flip is None and dark is None and defects is None and hot_sigma is None:
        return None
    from . import moviefix
    return moviefix.References(gain, gain_rot, gain_flip, dark, defects, hot_sigma)


def _patch_args(patch, patch_shift, patch_iters, no_align):
    """None without ``patch`` (the other two must then be unset), else the checked ((PY, PX), R, I)"""
    if patch is None:
        if patch_shift is not None or patch_iters is not None:
            raise ValueError("patch_shift and patch_iters belong to the local motion: give patch as well")
        return None
    if no_align:
        raise ValueError("patch fits a local field on top of the whole-frame shifts: it does not go with no_align")
    from . import localmotion
    return localmotion.check_patch_args(patch, localmotion.DEFAULT_PATCH_SHIFT if patch_shift is None else patch_shift,
                                        localmotion.DEFAULT_PATCH_ITERS if patch_iters is None else patch_iters)


def align_movie(path, ftbin=1, align_size=DEFAULT_ALIGN_SIZE, max_shift=DEFAULT_MAX_SHIFT, iters=DEFAULT_ITERS,
                no_align=False, device="cuda", resident_bytes=RESIDENT_BYTES, dose=None, pre_dose=0.0, kv=300.0, apix=None,
                gain=None, gain_rot=0, gain_flip=None, dark=None, defects=None, hot_sigma=None, references=None, patch=None,
                patch_shift=None, patch_iters=None):
    """One movie -> (sum float32 CUDA [by, bx], drift float64 [Z, 2] (dx, dy) in raw pixels, header, info).  With ``dose``
    (e/A^2 per frame; ``pre_dose`` before frame 0, ``kv`` in 200..300, ``apix`` or else the header's pixel size):
    info["dose_weighted"] is the dose-weighted sum of the same frames at the same shifts, float32 CUDA [by, bx].
    With ``gain`` / ``dark`` (paths of single-image MRC references; ``gain_rot`` quarter turns, then ``gain_flip`` "ud" /
    "lr"), ``defects`` (a file of ``x y w h`` rectangles) or ``hot_sigma`` (``moviefix``; ``references``: a run's
    ``moviefix.References`` in their place): the frames are corrected first, and info["defects"] = {"static", "hot", "fix"}.
    With ``patch`` = (PY, PX) (``patch_shift``: the half width of the patches' correlation window in reduced pixels,
    ``patch_iters``: iterations at most; ``localmotion``): every frame is also warped by the fitted local field, and
    info["local"] = {"patch", "reduced", "qx", "qy" ([3, 6], raw pixels), "iterations", "moved", "dropped", "geometry",
    "measured", "fitted" ([Z, P, 2] (y, x), raw pixels)}."""
    align_size, max_shift, iters = check_align_args(align_size, max_shift, iters)
    patch = _patch_args(patch, patch_shift, patch_iters, no_align)
    weighting = _dose_args(dose, pre_dose, kv, apix)
    if references is None:
        references = _references(gain, gain_rot, gain_flip, dark, defects, hot_sigma)
    with open_movie(path, device, resident_bytes) as movie:
        source = movie
        h = movie.header
        fixed = None
        if references is not None and references.active:
            from . import moviefix
            movie, fixed = moviefix.prepare(movie, *references.for_frames(h.ny, h.nx, movie._reader.device),
                                            references.hot_sigma)
            h = movie.header                                     # the movie's with mode 2: the frames are float32 now
        if weighting is not None and weighting[3] is None:
            from .ctf import header_apix
            if header_apix(h) is None:
                raise ValueError("%s: dose weighting needs the pixel size, and the movie's header states none: give --apix"
                                 % path)
            weighting = weighting[:3] + (header_apix(h),)
        ny, nx, Z = h.ny, h.nx, h.nz
        by, bx = ingest.resample_geometry(ny, nx, ftbin)
        sy, sx = np.zeros(Z), np.zeros(Z)
        info = {"iterations": 0, "edge_frames": [], "moved": None}
        if not no_align:
            Sy, Sx = align_geometry(ny, nx, align_size)
            if 2 * max_shift + 1 > min(Sy, Sx):
                raise ValueError("%s: a window of +-%d pixels does not fit the %dx%d reduced frames" % (path, max_shift, Sy, Sx))
            dev = movie._reader.device
            my, mx = ingest.resample_matrix(ny, Sy, dev), ingest.resample_matrix(nx, Sx, dev)
            reduced = torch.empty((Z, Sy, Sx), dtype=torch.float32, device=dev)
            for k in range(Z):
                red, _ = torch.ops.sprk.ingest_resample(movie.frame(k), h.mode, ny, nx, Sy, Sx, my, mx)
                reduced[k] = red - red.mean()
            ry, rx, info = estimate_shifts(reduced, max_shift, iters, os.path.basename(path))
            sy, sx = ry * (ny / Sy), rx * (nx / Sx)
            info = dict(info, reduced=(Sy, Sx))
        summed, anchor_term = movie, None
        if patch is not None:
            from . import localmotion
            for f in range(Z):                                   # the reduced frames laid on each other, as estimate_shifts does
                shifted = reduced[f].clone()
                torch.ops.sprk.align_accumulate(_flat_bytes(shifted), 2, Sy, Sx, Sy, Sx, shift_matrix(Sy, Sy, ry[f], dev),
                                                shift_matrix(Sx, Sx, rx[f], dev), 0.0, reduced[f], True)
            qy, qx, local = localmotion.estimate_field(reduced, *patch, name=os.path.basename(path))
            scale = np.array([ny / Sy, nx / Sx])                 # they differ slightly
            local = dict(local, patch=patch[0], reduced=(Sy, Sx), qy=qy * scale[0], qx=qx * scale[1],
                         measured=local["measured"] * scale, fitted=local["fitted"] * scale)
            info = dict(info, local=local)
            summed = localmotion.LocalMovie(movie, sy, sx, local["qy"], local["qx"])
            anchor_term = summed.anchor_term
            sy, sx = np.zeros(Z), np.zeros(Z)                    # the frames of ``summed`` are shifted already
        total = sum_frames(summed, by, bx, sy, sx)
        if anchor_term:
            total += anchor_term
        if weighting is not None:
            from . import dose as dose_mod
            info = dict(info, dose_weighted=dose_mod.sum_frames_weighted(summed, by, bx, sy, sx, apix=weighting[3],
                                                                         dose=weighting[0], pre_dose=weighting[1],
                                                                         kv=weighting[2]))
            if anchor_term:
                info["dose_weighted"] += anchor_term
        if patch is not None:
            sy, sx = summed.shifts_y, summed.shifts_x
        if fixed is not None:
            info = dict(info, defects=fixed)
        source.verify()
    return total, np.stack([0.0 - sx, 0.0 - sy], axis=1), h, info             # 0.0 - x: no "-0.0000" in the table


def write_sum(path, image, header, by, bx):
    """The aligned sum as a float32 MRC: ``micrograph_io.write_mrc``'s file with the movie's pixel size times ny / by (the
    cell of the movie's frames on the new sampling), when the movie's header states one."""
    buf = io.BytesIO()
    micrograph_io.write_mrc(buf, image)
    out = bytearray(buf.getvalue())
    from .ctf import header_apix
    if header_apix(header) is not None:
        fields = list(micrograph_io.MRCHeader._make(micrograph_io._HEADER.unpack(bytes(out[:1024]))))
        names = micrograph_io.MRCHeader._fields
        my_in = header.my if header.my > 0 else header.ny
        cell = {"mx": bx, "my": by, "mz": 1, "xlen": header.xlen / header.mx * header.nx,
                "ylen": (header.ylen / my_in if header.ylen > 0 else header.xlen / header.mx) * header.ny, "zlen": 1.0}
        for key, v in cell.items():
            fields[names.index(key)] = v
        out[:1024] = micrograph_io._HEADER.pack(*fields)
    with open(path, "wb") as f:
        f.write(bytes(out))


def align_dataset(movies, out_dir, ftbin=1, align_size=DEFAULT_ALIGN_SIZE, max_shift=DEFAULT_MAX_SHIFT, iters=DEFAULT_ITERS,
                  no_align=False, device="cuda", resident_bytes=RESIDENT_BYTES, dose=None, pre_dose=0.0, kv=300.0, apix=None,
                  gain=None, gain_rot=0, gain_flip=None, dark=None, defects=None, hot_sigma=None, patch=None, patch_shift=None,
                  patch_iters=None):
    """``joint align``: for every movie of the table / directory ``movies``: ``out_dir/{name}.mrc`` (the aligned sum, float32
    [by, bx] with (by, bx) = ``ingest.resample_geometry(ny, nx, ftbin)``) and ``out_dir/{name}_shifts.txt`` (frame, dx, dy in
    raw pixels, mean zero), plus ``out_dir/images.txt`` (image_name, path) for the commands that follow.
    With ``dose`` (``align_movie``) also ``out_dir/{name}_DW.mrc``, the dose-weighted sum, and ``out_dir/images_DW.txt``; the
    other files are byte for byte what they are without it.
    With ``gain``, ``dark``, ``defects`` or ``hot_sigma`` (``align_movie``; the references are read and uploaded once, and
    every movie's frames must have their size) also ``out_dir/{name}_defects.mrc``, the fix map (mode 0).
    With ``patch`` (``align_movie``) also ``out_dir/{name}_local.txt`` (``localmotion.write_local``); without it no other
    file changes a byte.
    -> {name: {"frames", "shape", "shifts": [[dx, dy], ...], "iterations", "edge_frames"[, "dose_weighted": path]
               [, "defects": {"static": n, "hot": n}][, "local": {"path", "patch", "iterations", "dropped", "qx", "qy"}]}}."""
    ftbin = ingest.check_ftbin(ftbin)
    check_align_args(align_size, max_shift, iters)
    _dose_args(dose, pre_dose, kv, apix)
    _patch_args(patch, patch_shift, patch_iters, no_align)
    references = _references(gain, gain_rot, gain_flip, dark, defects, hot_sigma)
    rows = micrograph_io.read_image_table(movies)
    if not rows:
        raise ValueError("no movies found in %s" % movies)
    for _, _, path in rows:
        require_movie(path)
    os.makedirs(out_dir, exist_ok=True)
    results, lines, lines_dw = {}, ["image_name\tpath"], ["image_name\tpath"]
    for _, name, path in rows:
        total, drift, header, info = align_movie(path, ftbin, align_size, max_shift, iters, no_align, device, resident_bytes,
                                                 dose, pre_dose, kv, apix, references=references, patch=patch,
                                                 patch_shift=patch_shift, patch_iters=patch_iters)
        by, bx = total.shape
        out = os.path.join(out_dir, name + ".mrc")
        write_sum(out, total.cpu().numpy(), header, by, bx)
        with open(os.path.join(out_dir, name + "_shifts.txt"), "w") as f:
            f.write("frame\tdx\tdy\n" + "".join("%d\t%.4f\t%.4f\n" % (k, dx, dy) for k, (dx, dy) in enumerate(drift)))
        lines.append("%s\t%s" % (name, out))
        results[name] = {"frames": int(header.nz), "shape": [int(by), int(bx)], "shifts": [[float(dx), float(dy)] for dx, dy in drift],
                         "iterations": info["iterations"], "edge_frames": info["edge_frames"]}
        if dose is not None:
            out_dw = os.path.join(out_dir, name + "_DW.mrc")
            write_sum(out_dw, info["dose_weighted"].cpu().numpy(), header, by, bx)
            lines_dw.append("%s\t%s" % (name, out_dw))
            results[name]["dose_weighted"] = out_dw
        if "defects" in info:
            from . import moviefix
            moviefix.write_fix_map(os.path.join(out_dir, name + "_defects.mrc"), info["defects"]["fix"].cpu().numpy())
            results[name]["defects"] = {"static": info["defects"]["static"], "hot": info["defects"]["hot"]}
        if "local" in info:
            from . import localmotion
            local = info["local"]
            out_local = os.path.join(out_dir, name + "_local.txt")
            localmotion.write_local(out_local, local)
            results[name]["local"] = {"path": out_local, "patch": list(local["patch"]), "iterations": local["iterations"],
                                      "dropped": local["dropped"], "qx": local["qx"].tolist(), "qy": local["qy"].tolist()}
        logger.info("%s: %d frames of %dx%d -> %dx%d, %d iteration(s), largest displacement %.2f raw pixels", name, header.nz,
                    header.ny, header.nx, by, bx, info["iterations"], float(np.abs(drift).max()))
    with open(os.path.join(out_dir, "images.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    if dose is not None:
        with open(os.path.join(out_dir, "images_DW.txt"), "w") as f:
            f.write("\n".join(lines_dw) + "\n")
    return results
