"""Particle extraction on the device: pick tables plus RAW micrographs in, per-micrograph ``.mrcs`` particle
stacks plus one ``particles.star`` out — the step between ``joint eval`` and 2-D classification, without leaving for
``relion_preprocess`` and without decoding a micrograph on the host a second time.

A file's sample block is uploaded once by ``ingest.read_raw``; csrc/extract.hip (``torch.ops.sprk.extract_boxes``) cuts
every box of that micrograph in one launch: box x box raw samples around each centre, binned N x N, normalised to zero
mean and unit variance of the background outside ``bg_radius`` (in output pixels), optionally contrast-inverted.  Boxes
that are not entirely inside the image (status 1) and boxes with no or a flat background (status 2) come back as zeros
and are not written.

Coordinates: x runs along nx (columns), y along ny (rows), in raw samples — the frame of ``{name}_scores_unbinned.txt``.
Picks in a binned frame (``{name}_scores.txt`` of ``joint eval --bin K``) are mapped through ``ingest.to_unbinned``."""
import logging
import os

import numpy as np
import torch

from . import _lib, export, ingest, micrograph_io, picks as picks_mod, torch_ops

logger = logging.getLogger("joint.extract")
OK, OUTSIDE, FLAT = 0, 1, 2                     # status codes of sprk_extract_boxes



def default_bg_radius(box, bin=1):
    """3/8 of the output side: RELION's rule of thumb of a background circle of 75 % of the box."""
    return 3 * (box // bin) // 8


def check_box(box, bin=1, bg_radius=None):
    """-> (b, bg_radius) or ValueError: 2 <= box <= 1024, box a multiple of bin, b = box // bin >= 2, bg_radius >= 0."""
    ingest.check_bin(bin)
    if not isinstance(box, (int, np.integer)):
        raise ValueError("box must be an integer, got %r" % (box,))
    if bg_radius is None:
        bg_radius = default_bg_radius(box, bin)
    try:
        return torch_ops.extract_side(int(box), int(bin), int(bg_radius)), int(bg_radius)
    except _lib.SprkError as e:
        raise ValueError(str(e)) from None


def extract_particles(path_or_raw, xy, box, bin=1, bg_radius=None, normalize=True, invert=False, device="cuda"):
    """path_or_raw: an MRC file, or the ``(raw, header)`` pair ``ingest.read_raw`` returns for one.  xy: [P, 2] integer
    (x, y) centres in raw samples, array or int32 CUDA tensor.
    -> (particles float32 CUDA [P, b, b], status int32 CUDA [P]); nothing is synchronised."""
    b, bg_radius = check_box(box, bin, bg_radius)
    if isinstance(path_or_raw, (str, os.PathLike)):
        raw, header = ingest.read_raw(os.fspath(path_or_raw), device)
    else:
        raw, header = path_or_raw
    if not raw.is_cuda:
        raise _lib.SprkError("extract_particles runs on the GPU only (raw samples on %s)" % raw.device)
    if not torch.is_tensor(xy):
        xy = np.asarray(xy).reshape(-1, 2)
        if xy.dtype.kind not in "iu":
            raise ValueError("particle centres must be integers (raw samples), got %s" % xy.dtype)
        info = np.iinfo(np.int32)                                # far outside either way: status 1
        xy = torch.from_numpy(np.clip(xy, info.min, info.max).astype(np.int32))
    xy = xy.to(raw.device)
    return torch.ops.sprk.extract_boxes(raw, header.mode, header.ny, header.nx, xy, int(box), int(bin), bg_radius,
                                        bool(normalize), bool(invert))


_pinned = None


def _pinned_out(shape):
    """A float32 pinned host tensor of this shape: one persistent buffer, grown to the largest stack seen (allocating
    pinned memory costs more than the copy it serves)."""
    global _pinned
    n = int(np.prod(shape))
    if _pinned is None or _pinned.numel() < n:
        _pinned = torch.empty(n, dtype=torch.float32).pin_memory()
    return _pinned[:n].view(shape)


def _extract_file(path, xy, box, bin, bg_radius, normalize, invert, device):
    """The device half of ``extract_dataset`` for one micrograph: one read, one upload, one launch.
    -> (float32 array [K, b, b] of the status-0 particles in pick order, through pinned memory — a view of a buffer
    the next call overwrites; status array [P])."""
    out, status = extract_particles(path, xy, box, bin, bg_radius, normalize, invert, device)
    status = status.cpu().numpy()                                # waits for the launch
    keep = np.flatnonzero(status == OK)
    if len(keep) < len(status):
        out = out.index_select(0, torch.from_numpy(keep).to(out.device))
    host = _pinned_out(tuple(out.shape))
    host.copy_(out, non_blocking=True)
    torch.cuda.current_stream(out.device).synchronize()
    return host.numpy(), status


def read_pick_tables(picks, names, picks_bin=1):
    """picks: a directory that holds ``{name}_scores_unbinned.txt`` (raw frame; looked for when ``picks_bin`` is 1) or
    ``{name}_scores.txt`` per micrograph, or one scores file, or a list of them (rows are matched by image_name).
    -> {name: (xy int64 [n, 2], scores float64 [n])} for the names that have a table."""
    tables = {}

    def add(path, only=None):
        row_names, xy, scores = picks_mod.read_scores(path)
        row_names = np.asarray(row_names, dtype=object)
        for name in ([only] if only is not None else list(dict.fromkeys(row_names))):
            sel = row_names == name
            if name in tables:
                sel_xy, sel_s = tables[name]
                tables[name] = (np.concatenate([sel_xy, xy[sel]]), np.concatenate([sel_s, scores[sel]]))
            else:
                tables[name] = (xy[sel], scores[sel])

    if isinstance(picks, (str, os.PathLike)) and os.path.isdir(picks):
        suffixes = ("_scores_unbinned.txt", "_scores.txt") if picks_bin == 1 else ("_scores.txt",)
        for name in names:
            for suffix in suffixes:
                path = os.path.join(picks, name + suffix)
                if os.path.exists(path):
                    add(path, only=name)
                    break
    else:
        for path in ([picks] if isinstance(picks, (str, os.PathLike)) else list(picks)):
            add(os.fspath(path))
    return tables


def extract_dataset(dataset, picks, out_dir, box, bin=1, picks_bin=1, threshold=None, bg_radius=None, normalize=True,
                    invert=False, device="cuda"):
    """``joint extract``: for every micrograph of the table / directory ``dataset`` that has a pick table, the picks
    with score > ``threshold`` (all of them when None), mapped from the ``picks_bin`` frame to raw samples, extracted in
    one launch and written as the float32 stack ``out_dir/{name}.mrcs`` (status-0 particles only, pick order); at the
    end ``out_dir/particles.star`` with one row per written particle.  A micrograph without a surviving particle writes
    no stack; micrographs without a pick table are skipped with a warning.
    -> {name: {"written", "outside", "flat"}} for the micrographs that had a table."""
    b, bg_radius = check_box(box, bin, bg_radius)
    picks_bin = ingest.check_bin(picks_bin)
    rows = micrograph_io.read_image_table(dataset)
    if not rows:
        raise ValueError("no micrographs found in %s" % dataset)
    tables = read_pick_tables(picks, [name for _, name, _ in rows], picks_bin)
    os.makedirs(out_dir, exist_ok=True)
    counts, star, missing = {}, [], []
    for _, name, path in rows:
        if name not in tables:
            missing.append(name)
            continue
        ingest.require_mrc(path)
        with open(path, "rb") as f:
            header, _ = ingest.read_header(path, f)
        xy, scores = tables[name]
        if threshold is not None:
            sel = scores > threshold
            xy, scores = xy[sel], scores[sel]
        if picks_bin > 1:
            _, _, oy, ox = ingest.binned_geometry(header.ny, header.nx, picks_bin)
            x, y = ingest.to_unbinned(xy[:, 0], xy[:, 1], picks_bin, ox, oy)
            xy = np.stack([x, y], axis=1).reshape(-1, 2)
        counts[name] = {"written": 0, "outside": 0, "flat": 0}
        if not len(xy):
            continue
        particles, status = _extract_file(path, xy, box, bin, bg_radius, normalize, invert, device)
        ok = np.flatnonzero(status == OK)
        counts[name] = {"written": len(ok), "outside": int((status == OUTSIDE).sum()), "flat": int((status == FLAT).sum())}
        if not len(ok):
            continue
        stack = name + ".mrcs"
        with open(os.path.join(out_dir, stack), "wb") as f:
            micrograph_io.write_mrc(f, particles)
        for k, i in enumerate(ok):
            star.append("%d\t%d\t%06d@%s\t%s\t%s\n" % (xy[i, 0], xy[i, 1], k + 1, stack, os.path.basename(path),
                                                      str(scores[i])))
    if missing:
        logger.warning("%s: %d micrographs skipped because %s has no pick table for them: %s", dataset, len(missing), picks,
                       ", ".join(missing[:10]) + (" ..." if len(missing) > 10 else ""))
    with open(os.path.join(out_dir, "particles.star"), "w") as f:
        f.write(export.PARTICLES_STAR_HEADER)
        f.writelines(star)
    logger.info("%s: %d particles of %d micrographs written to %s", dataset, len(star), len(counts), out_dir)
    return counts
