"""Device-side micrograph ingest: raw aligned micrographs -> the network's input, without the
``newstack -bin N`` copy of the dataset the upstream README starts with and without the host passes of
``micrograph_io.load_image`` + ``MicrographFeed`` (min-max, quantise, /255, transpose, reflect-pad).

The file's sample block is read straight into a pinned buffer, uploaded once (non-blocking) and decoded, binned,
ranged, normalised and laid out by csrc/ingest.hip (``torch.ops.sprk.ingest_bin`` / ``ingest_finish``).  The result
is bit for bit what the host path produces from the binned image: ``binned_uint8(path, N)`` equals ``load_image`` of
the float32 MRC that ``joint bin --bin N`` writes, and ``ingest(path, 1)`` equals ``MicrographFeed``'s tensor.

``clip=(lo_pct, hi_pct)`` (``--clip LO[,HI]``) clamps the binned image to two of its own order statistics before the
min-max step (``torch.ops.sprk.ingest_clip``, an exact selection on the device), so that hot pixels and black spots do
not set the 8-bit range; ``joint bin --clip`` writes the clamped block means, and the closure above holds with the flag
on both sides.  ``None`` adds no launch and changes no byte.

``flatten=R`` (``--flatten R``) subtracts from every binned pixel the mean over its (2R+1) x (2R+1) window, clamped at the
edges (``torch.ops.sprk.ingest_flatten``, exact integer window sums on the device), so that a slow gradient across the
micrograph does not take the levels of the 8-bit range.  With ``clip`` as well the order is clip, flatten, clip again
by the same percentages: the background is estimated without the outliers, and the final range comes from the order
statistics of the flattened image.  The closure holds with the flags on both sides; ``None`` adds no launch.

``ftbin=F`` (``--ftbin F``, instead of ``bin``) resamples by a Fourier crop: any rational 1 <= F <= 64, the whole extent of
both axes (no margin dropped), no aliasing — ``newstack -ftreduce``, MotionCor2 ``-FtBin``.  The operator is separable,
Y = My D Mx^T with the real matrices of ``resample_matrix``, and runs as two fp32 MFMA GEMMs over the whole micrograph
(``torch.ops.sprk.ingest_resample``, csrc/resample.hip) in place of ``ingest_bin``; ``clip`` and ``flatten`` follow as
they are.  A Fourier crop takes the image as periodic: what leaves at one edge wraps round to the other, as in the
tools named; it is not tapered.  Output pixel s sits at input position s * B / S (``to_raw`` / ``to_scaled``).

Coordinates: x runs along nx (columns), y along ny (rows) — the frame of the label tables and of ``*_scores.txt``.
Bin factor N keeps the centred area: binned pixel (x, y) covers samples ox + N*x .. ox + N*x + N-1 (oy likewise)."""
import logging
import math
import os
from fractions import Fraction

import numpy as np
import torch

from . import micrograph_io, sampler as sampler_mod, torch_ops
from .datasets import DetectionDataset
from .fourier import resample_matrix, resample_matrix64          # the operands of --ftbin

MAX_BIN = torch_ops.INGEST_MAX_BIN
MAX_FLATTEN = torch_ops.INGEST_MAX_FLATTEN
logger = logging.getLogger("joint.ingest")
_HEADER_BYTES = 1024


def check_bin(N):
    if not isinstance(N, (int, np.integer)) or not 1 <= N <= MAX_BIN:
        raise ValueError("bin factor must be an integer in 1..%d, got %r" % (MAX_BIN, N))
    return int(N)


def binned_geometry(ny, nx, N):
    """-> (by, bx, oy, ox): size of the binned image and the first sample of its first block."""
    N = check_bin(N)
    by, bx = ny // N, nx // N
    if by < 1 or bx < 1:
        raise ValueError("a %dx%d image has no %dx%d block" % (ny, nx, N, N))
    return by, bx, (ny % N) // 2, (nx % N) // 2


def to_unbinned(x, y, N, ox, oy):
    """Binned pixel -> the sample at the centre of its block (the upper-left of the four central ones for even N)."""
    return ox + N * x + N // 2, oy + N * y + N // 2


def to_binned(x, y, N, ox, oy, bx, by):
    """Sample -> (x, y of the binned pixel whose block holds it, inside); ``inside`` is False for samples in the margin
    that binning drops (outside [0, bx) x [0, by)).  Inverse of ``to_unbinned``."""
    xb, yb = (np.asarray(x) - ox) // N, (np.asarray(y) - oy) // N
    return xb, yb, (xb >= 0) & (xb < bx) & (yb >= 0) & (yb < by)


MAX_FTBIN = 64
MAX_SIDE = torch_ops.INGEST_MAX_SIDE


def check_ftbin(F):
    """The factor of ``--ftbin F`` -> Fraction: an int, a Fraction, decimal or ``p/q`` text, or a float (through its
    ``str``: 9.64 is 241/25, not the binary neighbour), 1 <= F <= MAX_FTBIN."""
    try:
        if isinstance(F, bool):
            raise ValueError
        if isinstance(F, (float, np.floating)):
            F = str(float(F))
        elif isinstance(F, np.integer):
            F = int(F)
        F = Fraction(F)
    except (TypeError, ValueError, ZeroDivisionError):
        raise ValueError("ftbin factor must be a rational number in 1..%d, got %r" % (MAX_FTBIN, F)) from None
    if not 1 <= F <= MAX_FTBIN:
        raise ValueError("ftbin factor must be a rational number in 1..%d, got %s" % (MAX_FTBIN, F))
    return F


def resample_geometry(ny, nx, F):
    """-> (by, bx): the size of the Fourier-cropped image, floor(n / F + 1/2) per axis in exact rational arithmetic.  Both
    axes keep their whole extent; the factor per axis is ny / by and nx / bx.  F = 1: (ny, nx)."""
    F = check_ftbin(F)
    ny, nx = int(ny), int(nx)
    if ny > MAX_SIDE or nx > MAX_SIDE:
        raise ValueError("a %dx%d image is larger than --ftbin takes (%d a side)" % (ny, nx, MAX_SIDE))
    by, bx = (math.floor(Fraction(n) / F + Fraction(1, 2)) for n in (ny, nx))
    if by < 2 or bx < 2:
        raise ValueError("a %dx%d image resampled by %s leaves %dx%d pixels (at least 2 a side)" % (ny, nx, F, by, bx))
    return by, bx


def to_raw(x, y, ny, nx, by, bx):
    """Pixel of the [by, bx] Fourier-cropped image -> the sample nearest to its position x * nx / bx (halves go up)."""
    return (2 * x * nx + bx) // (2 * bx), (2 * y * ny + by) // (2 * by)


def to_scaled(x, y, ny, nx, by, bx):
    """Sample -> (x, y of the nearest pixel of the [by, bx] image, inside); ``inside`` is False for points outside the
    micrograph.  ``to_scaled(to_raw(x))`` is x for every pixel."""
    x, y = np.asarray(x), np.asarray(y)
    xs = np.minimum((2 * x * bx + nx) // (2 * nx), bx - 1)
    ys = np.minimum((2 * y * by + ny) // (2 * ny), by - 1)
    return xs, ys, (x >= 0) & (x < nx) & (y >= 0) & (y < ny)


def require_mrc(path):
    if os.path.splitext(path)[1] != ".mrc":
        raise ValueError("%s: raw micrograph ingest (--bin) reads MRC files only; convert TIFF / PNG inputs, or "
                         "evaluate them without --bin" % path)


def read_header(path, f):
    """The 1024-byte MRC header of an open file -> (MRCHeader, byte offset of the samples).  Refuses what
    ``load_image`` refuses: unknown modes and stacks."""
    head = f.read(_HEADER_BYTES)
    if len(head) < _HEADER_BYTES:
        raise ValueError("MRC file shorter than its 1024-byte header")
    header = micrograph_io.MRCHeader._make(micrograph_io._HEADER.unpack(head))
    if header.mode not in micrograph_io._MODES:
        raise ValueError("Unsupported MRC mode: %d" % header.mode)
    if header.nz != 1:
        raise ValueError("%s: expected a single 2-D micrograph, got shape %s" % (path, (header.nz, header.ny, header.nx)))
    if header.ny < 1 or header.nx < 1 or header.next < 0:
        raise ValueError("%s: bad MRC header (nx %d, ny %d, next %d)" % (path, header.nx, header.ny, header.next))
    return header, _HEADER_BYTES + header.next


class RawReader:
    """File -> device bytes through two pinned slots, each as large as the largest file seen so far and re-used only
    after the copy that last read it has completed (its event) — ``feed.PinnedRing`` for buffers of varying size.  The
    read of micrograph k+1 therefore overlaps the upload and the network pass of micrograph k without a second thread."""

    SLOTS = 2

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("micrograph ingest runs on the GPU only (device %s)" % self.device)
        self._bufs = [None] * self.SLOTS
        self._events = [None] * self.SLOTS
        self._next = 0

    def _slot(self, nbytes):
        k = self._next
        self._next = (k + 1) % self.SLOTS
        if self._events[k] is not None:
            self._events[k].synchronize()
            self._events[k] = None
        if self._bufs[k] is None or self._bufs[k].numel() < nbytes:
            self._bufs[k] = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        return k

    def read(self, path):
        """-> (uint8 CUDA tensor with the ny*nx samples as they sit in the file, MRCHeader).  The upload is in flight
        on the current stream when this returns."""
        require_mrc(path)
        with open(path, "rb") as f:
            header, start = read_header(path, f)
            nbytes = header.ny * header.nx * np.dtype(micrograph_io._MODES[header.mode]).itemsize
            k = self._slot(nbytes)
            f.seek(start)
            got = f.readinto(memoryview(self._bufs[k].numpy())[:nbytes])
        if got != nbytes:
            raise ValueError("%s: %d bytes of samples, the header promises %d" % (path, got, nbytes))
        raw = torch.empty(nbytes, dtype=torch.uint8, device=self.device)     # the allocator aligns far beyond 16 bytes
        raw.copy_(self._bufs[k][:nbytes], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._events[k] = ev
        return raw, header


_readers = {}


def _reader(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _readers:
        _readers[device] = RawReader(device)
    return _readers[device]


def read_raw(path, device="cuda"):
    """-> (raw uint8 CUDA tensor, MRCHeader) through the device's shared ``RawReader``."""
    return _reader(device).read(path)


def parse_clip(text):
    """``--clip LO[,HI]`` -> (lo_pct, hi_pct): the percentages of the pixels clipped at the dark and at the bright end,
    HI = LO when omitted.  ValueError for anything but two finite numbers >= 0 with LO + HI < 100."""
    parts = str(text).split(",")
    try:
        if not 1 <= len(parts) <= 2:
            raise ValueError
        lo = float(parts[0])
        hi = float(parts[1]) if len(parts) == 2 else lo
    except ValueError:
        raise ValueError("clip must be LO or LO,HI in percent, got %r" % (text,)) from None
    return check_clip((lo, hi))


def check_clip(clip):
    try:
        lo, hi = (float(v) for v in clip)
    except (TypeError, ValueError):
        raise ValueError("clip must be a pair (lo_pct, hi_pct), got %r" % (clip,)) from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo >= 0 and hi >= 0 and lo + hi < 100):
        raise ValueError("clip percentages must be >= 0 with LO + HI < 100, got %r, %r" % (lo, hi))
    return lo, hi


def clip_ranks(n, clip):
    """-> (k_lo, k_hi): the ranks (from 0, among the n pixels in ascending order) the image is clamped to:
    k_lo = floor(LO/100 * (n-1)), k_hi = (n-1) - floor(HI/100 * (n-1)).  (0, 0) -> (0, n-1), the identity."""
    lo, hi = check_clip(clip)
    if n < 1:
        raise ValueError("clip_ranks: an image of %d pixels" % n)
    return int(math.floor(lo / 100 * (n - 1))), (n - 1) - int(math.floor(hi / 100 * (n - 1)))


def check_flatten(R):
    """The radius of ``--flatten R`` in binned pixels: an integer in 1..MAX_FLATTEN (SPRK_INGEST_MAX_FLATTEN)."""
    if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or not 1 <= R <= MAX_FLATTEN:
        raise ValueError("flatten radius must be an integer in 1..%d, got %r" % (MAX_FLATTEN, R))
    return int(R)


def _exclusive(bin, ftbin):
    """``ftbin`` takes the place of ``bin``: with it, ``bin`` is None or 1."""
    if ftbin is not None and bin not in (None, 1):
        raise ValueError("bin %r and ftbin %r exclude one another" % (bin, ftbin))


def _bin(path, N, device, clip=None, flatten=None, ftbin=None):
    _exclusive(N, ftbin)
    if ftbin is None:
        N = check_bin(N)
    else:
        ftbin = check_ftbin(ftbin)
    if clip is not None:
        clip = check_clip(clip)
    if flatten is not None:
        flatten = check_flatten(flatten)
    raw, header = read_raw(path, device)
    if ftbin is None:
        geometry = binned_geometry(header.ny, header.nx, N)
        binned, rng = torch.ops.sprk.ingest_bin(raw, header.mode, header.ny, header.nx, N)
    else:                     # the Fourier crop of the whole micrograph: two fp32 MFMA GEMMs (csrc/resample.hip)
        ny, nx = header.ny, header.nx
        by, bx = resample_geometry(ny, nx, ftbin)
        geometry = (by, bx, ny, nx)
        binned, rng = torch.ops.sprk.ingest_resample(raw, header.mode, ny, nx, by, bx, resample_matrix(ny, by, raw.device),
                                                     resample_matrix(nx, bx, raw.device))
    if clip is not None:      # the image clamped to two of its order statistics, which become the range (csrc/ingest.hip)
        binned, rng = torch.ops.sprk.ingest_clip(binned, rng, *clip_ranks(binned.numel(), clip))
    if flatten is not None:   # minus the local mean; the background of the clamped image, then the clip of the flat one
        binned, rng = torch.ops.sprk.ingest_flatten(binned, rng, flatten)
        if clip is not None:
            binned, rng = torch.ops.sprk.ingest_clip(binned, rng, *clip_ranks(binned.numel(), clip))
    return binned, rng, geometry


def binned(path, bin, device="cuda", clip=None, flatten=None, ftbin=None):
    """-> (float32 CUDA tensor [by, bx]: the N x N block means, geometry) — what ``joint bin`` writes.  ``clip``
    (lo_pct, hi_pct): clamped to the order statistics of ``clip_ranks``; ``flatten`` R: minus the mean over the
    (2R+1)^2 window (with ``clip``: clip, flatten, clip); None: as they are.  ``ftbin`` F (``bin`` None or 1): the
    Fourier crop to ``resample_geometry`` instead of block means, geometry (by, bx, ny, nx)."""
    b, _, geometry = _bin(path, bin, device, clip, flatten, ftbin)
    return b, geometry


def binned_uint8(path, bin, device="cuda", clip=None, flatten=None, ftbin=None):
    """-> uint8 array [by, bx]: ``micrograph_io.load_image`` of the binned (and, with ``clip`` / ``flatten``, clamped /
    flattened) micrograph; with ``ftbin``: of the Fourier-cropped one."""
    b, rng, _ = _bin(path, bin, device, clip, flatten, ftbin)
    u8, _ = torch.ops.sprk.ingest_finish(b, rng, True, False)
    return u8.cpu().numpy()


def ingest(path, bin, device="cuda", clip=None, flatten=None, ftbin=None):
    """-> (network input float32 CUDA [1, 1, S, S], (by, bx), (by, bx, oy, ox)): the binned micrograph (with ``clip``:
    clamped to its two order statistics first; with ``flatten``: its local mean subtracted) min-max quantised, /255,
    transposed and reflect-padded, as ``MicrographFeed`` hands it to the network.  With ``ftbin`` (``bin`` None or 1): the
    Fourier-cropped micrograph, and (by, bx, ny, nx) as the geometry."""
    b, rng, geometry = _bin(path, bin, device, clip, flatten, ftbin)
    _, net = torch.ops.sprk.ingest_finish(b, rng, False, True)
    return net[None, None], geometry[:2], geometry


class RawMicrographFeed:
    """``feed.MicrographFeed`` for raw micrographs: same rows (``micrograph_io.read_image_table``), same order
    (``count`` wrapping, ``rank`` / ``world`` striding), same items — but a file is read when its turn comes (nothing
    is held in memory) and its tensor comes from ``ingest``.  IMAGE_SHAPE is [1, bx, by] (tensors are transposed), the
    target is all zeros (evaluation has no labels to draw), BIN_GEOMETRY carries (by, bx, oy, ox) — with ``ftbin``
    (``bin`` None or 1) (by, bx, ny, nx)."""

    def __init__(self, rows, bin, count=None, device="cuda", rank=0, world=1, gt=None, clip=None,
                 flatten=None, ftbin=None):
        _exclusive(bin, ftbin)
        self.ftbin = None if ftbin is None else check_ftbin(ftbin)
        self.bin = check_bin(bin) if ftbin is None else None
        self.clip = None if clip is None else check_clip(clip)
        self.flatten = None if flatten is None else check_flatten(flatten)
        self.device = torch.device(device)
        self.gt = gt or {}
        images = {}
        for source, name, path in rows:                      # grouping and order of feed.load_micrographs
            images.setdefault(source, {})[name] = path
        self.items = [(path, name) for name, path in next(iter(images.values())).items()] if images else []
        if not self.items:
            raise ValueError("empty evaluation set")
        for path, _ in self.items:                           # before the first micrograph is evaluated, not at its turn
            require_mrc(path)
        order = sampler_mod.sequential_indices(len(self.items), count)
        self.order = [(pos, k) for pos, k in enumerate(order) if pos % world == rank]
        self._reader = _reader(self.device)

    def __len__(self):
        return len(self.order)

    def __iter__(self):
        M = DetectionDataset.Metadata
        for pos, k in self.order:
            path, name = self.items[k]
            inp, (by, bx), geometry = ingest(path, self.bin, self.device, self.clip, self.flatten, self.ftbin)
            md = {M.INDEXES: torch.tensor([k]), M.NAME: [name], M.IMAGE_SHAPE: torch.tensor([[1, bx, by]]), M.GT: [],
                  M.BIN_GEOMETRY: [geometry]}
            if name in self.gt:
                g = micrograph_io.to_unit_float(self.gt[name]).T[None]
                md[M.GT] = [torch.from_numpy(np.ascontiguousarray(g))]
            hm = torch.zeros_like(inp)
            yield pos, DetectionDataset.make_batch(inp, hm[..., :bx, :by], hm=hm, metadata=md)


def unbinned_map(N, ox, oy):
    """The coordinate map ``picks.write_scores`` applies for ``{name}_scores_unbinned.txt``: plain ints through
    ``to_unbinned``."""
    def to_raw(x, y):
        return to_unbinned(int(x), int(y), N, ox, oy)
    return to_raw


def unscaled_map(ny, nx, by, bx):
    """The coordinate map ``picks.write_scores`` applies for ``{name}_scores_unbinned.txt`` under ``ftbin``: plain ints
    through ``to_raw``."""
    def map_(x, y):
        return to_raw(int(x), int(y), ny, nx, by, bx)
    return map_


def bin_dataset(dataset, bin, out_dir, labels=None, device="cuda", clip=None, flatten=None, ftbin=None):
    """``joint bin``: every micrograph of the table / directory ``dataset`` binned on the device and written as a
    float32 MRC ``out_dir/{name}.mrc``, plus ``out_dir/images.txt`` (image_name, path) and, with ``labels``,
    ``out_dir/labels.txt`` (coordinates through ``to_binned``, points outside the binned area dropped, other columns
    kept).  Label rows of images that are not in the dataset are dropped too, with a warning that names them.
    ``clip`` / ``flatten``: the image ``binned`` returns for them — what ``joint eval --bin N`` with the same flags sees.
    ``ftbin`` F (``bin`` None or 1): Fourier-cropped instead (``joint bin --ftbin F``), labels through ``to_scaled``
    (points outside the micrograph dropped), geometry (by, bx, ny, nx).
    -> {"images": path, "labels": path or None, "geometry": {name: (by, bx, oy, ox)},
        "label_rows": {"kept", "outside", "unknown_image"} or None}."""
    from . import coordinates
    _exclusive(bin, ftbin)
    if ftbin is None:
        bin = check_bin(bin)
    else:
        ftbin = check_ftbin(ftbin)
    if clip is not None:
        clip = check_clip(clip)
    if flatten is not None:
        flatten = check_flatten(flatten)
    rows = micrograph_io.read_image_table(dataset)
    if not rows:
        raise ValueError("no micrographs found in %s" % dataset)
    os.makedirs(out_dir, exist_ok=True)
    geometry, lines = {}, ["image_name\tpath"]
    for _, name, path in rows:
        b, geometry[name] = binned(path, bin, device, clip, flatten, ftbin)
        out = os.path.join(out_dir, name + ".mrc")
        with open(out, "wb") as f:
            micrograph_io.write_mrc(f, b.cpu().numpy())
        lines.append("%s\t%s" % (name, out))
    images = os.path.join(out_dir, "images.txt")
    with open(images, "w") as f:
        f.write("\n".join(lines) + "\n")
    labels_out, counts = None, None
    if labels:
        table = coordinates.read_coordinates(labels)
        keep = np.zeros(len(table), dtype=bool)
        unknown = {}
        xs, ys = table["x_coord"].to_numpy().copy(), table["y_coord"].to_numpy().copy()
        for i, name in enumerate(table["image_name"].astype(str)):
            if name not in geometry:                         # not a micrograph of this dataset (a misspelt name?)
                unknown[name] = unknown.get(name, 0) + 1
                continue
            if ftbin is not None:
                by, bx, ny, nx = geometry[name]
                xs[i], ys[i], keep[i] = to_scaled(xs[i], ys[i], ny, nx, by, bx)
                continue
            by, bx, oy, ox = geometry[name]
            xs[i], ys[i], keep[i] = to_binned(xs[i], ys[i], bin, ox, oy, bx, by)
        outside = len(table) - int(keep.sum()) - sum(unknown.values())
        logger.info("%s: %d of %d label rows kept, %d outside the binned area", labels, int(keep.sum()), len(table), outside)
        if unknown:
            logger.warning("%s: %d label rows dropped because their image_name is not in %s: %s", labels,
                           sum(unknown.values()), dataset, ", ".join(sorted(unknown)[:10]) + (" ..." if len(unknown) > 10 else ""))
        counts = {"kept": int(keep.sum()), "outside": outside, "unknown_image": sum(unknown.values())}
        table = table.assign(x_coord=xs, y_coord=ys).loc[keep]
        labels_out = os.path.join(out_dir, "labels.txt")
        table.to_csv(labels_out, sep="\t", index=False)
    return {"images": images, "labels": labels_out, "geometry": geometry, "label_rows": counts}
