"""Particle extraction on the device: pick tables plus RAW micrographs in, per-micrograph ``.mrcs`` particle
stacks plus one ``particles.star`` out — the step between ``joint eval`` and 2-D classification, without leaving for
``relion_preprocess`` and without decoding a micrograph on the host a second time.

A file's sample block is uploaded once by ``ingest.read_raw``; csrc/extract.hip (``torch.ops.sprk.extract_boxes``) cuts
every box of that micrograph in one launch: box x box raw samples around each centre, binned N x N — or, with ``scale``,
Fourier-cropped to any S x S (``torch.ops.sprk.extract_scale``: M D M^T with the matrix of ``crop_matrix``) — normalised to zero
mean and unit variance of the background outside ``bg_radius`` (in output pixels), optionally contrast-inverted.  With
``ctf_correct`` every box is multiplied in Fourier space by the CTF filter of its micrograph on the way
(``torch.ops.sprk.extract_filter``, csrc/extractfilter.hip: four GEMMs with the matrices of ``filter_matrices``).  Boxes
that are not entirely inside the image (status 1) and boxes with no or a flat background (status 2) come back as zeros
and are not written.

Coordinates: x runs along nx (columns), y along ny (rows), in raw samples — the frame of ``{name}_scores_unbinned.txt``.
Picks in a binned frame (``{name}_scores.txt`` of ``joint eval --bin K``) are mapped through ``ingest.to_unbinned``."""
import logging
import os

import numpy as np
import torch

from . import _lib, ctf as ctf_mod, export, fourier, ingest, micrograph_io, picks as picks_mod, torch_ops

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


def check_scale(box, scale, bg_radius=None):
    """-> (S, bg_radius) or ValueError: 2 <= scale <= box <= 1024, bg_radius >= 0 (default 3/8 of the output side)."""
    if not isinstance(box, (int, np.integer)) or not isinstance(scale, (int, np.integer)):
        raise ValueError("box and scale must be integers, got %r and %r" % (box, scale))
    if bg_radius is None:
        bg_radius = default_bg_radius(scale)
    try:
        return torch_ops.extract_scale_side(int(box), int(scale), int(bg_radius)), int(bg_radius)
    except _lib.SprkError as e:
        raise ValueError(str(e)) from None


def crop_matrix64(B, S):
    """The Fourier crop of B samples to S as a real [S, B] matrix in float64: IDFT_S . crop . DFT_B scaled by S / B,
    M[s, b] = (1/B) sum_{k=-h..h} w_k cos(2 pi k (s/S - b/B)), h = S // 2, w_k = 1 except that for even S the two ends
    k = +-S/2 weigh 1/2 each (the Nyquist row of the output is shared by both signs).  Every row sums to 1.  The phase
    k (sB - bS) is reduced mod SB in integers before the cosine, and the sum over k runs in one [S, B] array (the two
    signs of k together: the cosine is even).  S == B is the identity and is returned as such."""
    B, S = int(B), int(S)
    if not 2 <= S <= B:
        raise ValueError("crop_matrix: 2 <= S <= B, got B = %d, S = %d" % (B, S))
    if S == B:
        return np.eye(B)
    h = S // 2
    base = np.arange(S, dtype=np.int64)[:, None] * B - np.arange(B, dtype=np.int64)[None, :] * S
    acc = np.ones((S, B), dtype=np.float64)                      # k = 0
    for k in range(1, h + 1):
        w = 1.0 if (S % 2 or k < h) else 0.5                     # both signs: 2 w cos
        acc += (2.0 * w) * np.cos(fourier.reduced(k * base, S * B))
    return acc / B


def crop_matrix(B, S, device=None):
    """``crop_matrix64`` rounded to float32.  Without a device: the [S, B] array.  With one: the operand of
    ``torch.ops.sprk.extract_scale``, a contiguous tensor [roundup(S, 16), roundup(B, 4)] on that device whose added
    rows and columns are exact zeros, built once per (B, S, device)."""
    B, S = int(B), int(S)
    return fourier.operands(crop_matrix64, (B, S), torch_ops.crop_matrix_shape(B, S), device)


def check_filter(box, scale=None, bg_radius=None):
    """-> (S, bg_radius) or ValueError: box and S even, 16 <= S <= box <= 1024 (S = box without ``scale``), bg_radius >= 0
    (default 3/8 of the output side)."""
    scale = box if scale is None else scale
    if not isinstance(box, (int, np.integer)) or not isinstance(scale, (int, np.integer)):
        raise ValueError("box and scale must be integers, got %r and %r" % (box, scale))
    if bg_radius is None:
        bg_radius = default_bg_radius(scale)
    try:
        return torch_ops.extract_filter_side(int(box), int(scale), int(bg_radius)), int(bg_radius)
    except _lib.SprkError as e:
        raise ValueError(str(e)) from None


def filter_matrices64(B, S):
    """The four real matrices of ``torch.ops.sprk.extract_filter`` in float64 (include/sprk.h), h = S/2, Hs = h + 1, Ku =
    S + 1, k = -h .. h: W1 [2Hs, B] the half-plane DFT along the rows of the box, W2 [2Ku, 2B] the DFT along its columns at
    the kept k, W3 [2S, 2Ku] the inverse along the columns with the weights a_k (1/2 at k = +-h), W4 [S, 2Hs] the inverse
    along the rows with w_v (1 at v = 0 and h, else 2) and 1/B^2: ``fourier.four_stage64`` of a square box.  With a filter of
    ones the four stages are ``crop_matrix64(B, S)`` applied on both sides."""
    B, S = int(B), int(S)
    check_filter(B, S)
    return fourier.four_stage64(B, B, S, S, 1.0, float(B) * B)


def filter_matrices(B, S, device=None):
    """``filter_matrices64`` rounded to float32.  Without a device: the four arrays.  With one: the operands of
    ``torch.ops.sprk.extract_filter``, contiguous tensors on that device whose columns are rounded up to a multiple of 4
    with exact zeros (``torch_ops.extract_filter_shapes``), built once per (B, S, device)."""
    B, S = int(B), int(S)
    return fourier.operands(filter_matrices64, (B, S), torch_ops.extract_filter_shapes(B, S)[:4], device)


def extract_particles(path_or_raw, xy, box, bin=1, bg_radius=None, normalize=True, invert=False, device="cuda", scale=None,
                      ctf_filter=None, max_batch=0):
    """path_or_raw: an MRC file, or the ``(raw, header)`` pair ``ingest.read_raw`` returns for one.  xy: [P, 2] integer
    (x, y) centres in raw samples, array or int32 CUDA tensor.  scale = S: boxes Fourier-cropped to S x S instead of
    binned (``bin`` must be 1), b = S.  ctf_filter = the float32 [b + 1, b/2 + 1] array or tensor of
    ``ctf.correction_filter``: every box is multiplied by it in Fourier space (``torch.ops.sprk.extract_filter``; box and
    b even, b >= 16, ``bin`` must be 1; ``max_batch`` particles share the workspace at a time, 0 = the library's choice).
    -> (particles float32 CUDA [P, b, b], status int32 CUDA [P]); nothing is synchronised."""
    if ctf_filter is not None:
        if bin != 1:
            raise ValueError("a CTF filter and bin > 1 exclude one another (use scale)")
        b, bg_radius = check_filter(box, scale, bg_radius)
    elif scale is not None:
        if bin != 1:
            raise ValueError("scale and bin > 1 exclude one another")
        b, bg_radius = check_scale(box, scale, bg_radius)
    else:
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
    if ctf_filter is not None:
        if not torch.is_tensor(ctf_filter):
            ctf_filter = torch.from_numpy(np.ascontiguousarray(ctf_filter, dtype=np.float32))
        return torch.ops.sprk.extract_filter(raw, header.mode, header.ny, header.nx, xy, int(box), b,
                                             *filter_matrices(box, b, raw.device), ctf_filter.to(raw.device).contiguous(),
                                             bg_radius, bool(normalize), bool(invert), int(max_batch))
    if scale is not None:
        return torch.ops.sprk.extract_scale(raw, header.mode, header.ny, header.nx, xy, int(box), b,
                                            crop_matrix(box, b, raw.device), bg_radius, bool(normalize), bool(invert))
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
    return _to_host(*extract_particles(path, xy, box, bin, bg_radius, normalize, invert, device))


def _extract_file_scaled(path, xy, box, scale, bg_radius, normalize, invert, device):
    """``_extract_file`` with the boxes Fourier-cropped to scale x scale."""
    return _to_host(*extract_particles(path, xy, box, 1, bg_radius, normalize, invert, device, scale=scale))


def _extract_file_filtered(path, xy, box, scale, bg_radius, normalize, invert, device, ctf_filter):
    """``_extract_file_scaled`` with the boxes multiplied by ``ctf_filter`` in Fourier space."""
    return _to_host(*extract_particles(path, xy, box, 1, bg_radius, normalize, invert, device, scale=scale,
                                       ctf_filter=ctf_filter))


def _to_host(out, status):
    """-> (the status-0 particles as a float32 array through pinned memory, status array)"""
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


def _ctf_filter(row, box, side, mode):
    """``ctf.correction_filter`` from one row of ``micrographs_ctf.star`` (``ctf.read_ctf_star``); the raw pixel size is
    DetectorPixelSize . 10^4 / Magnification Angstrom."""
    apix = float(row["DetectorPixelSize"]) * 1e4 / float(row["Magnification"])
    return ctf_mod.correction_filter(box, side, apix, float(row["DefocusU"]), float(row["DefocusV"]), float(row["DefocusAngle"]),
                                     float(row["Voltage"]), float(row["SphericalAberration"]), float(row["AmplitudeContrast"]),
                                     mode)


def _ctf_columns(star, named_paths, pixel_factor):
    """The text appended to every ``particles.star`` row of a micrograph, {name: "\\t..."}: the columns of its row in the
    ``micrographs_ctf.star`` table ``star`` (matched by the file name, as ``_rlnMicrographName`` is written), verbatim
    except ``_rlnDetectorPixelSize``, which is multiplied by ``pixel_factor``.  ValueError naming the micrographs of
    ``named_paths`` that have no row."""
    table = ctf_mod.read_ctf_star(star)
    absent = [name for name, path in named_paths if os.path.basename(path) not in table]
    if absent:
        raise ValueError("%s has no row for %d micrographs that have picks: %s" % (star, len(absent), ", ".join(absent)))
    cols = {}
    for name, path in named_paths:
        row = dict(table[os.path.basename(path)])
        row["DetectorPixelSize"] = "%.5f" % (float(row["DetectorPixelSize"]) * pixel_factor)
        cols[name] = "".join("\t" + row[c] for c in ctf_mod.CTF_STAR_COLUMNS[1:])
    return cols


def extract_dataset(dataset, picks, out_dir, box, bin=1, picks_bin=1, threshold=None, bg_radius=None, normalize=True,
                    invert=False, device="cuda", scale=None, ctf=None, ctf_correct=None):
    """``joint extract``: for every micrograph of the table / directory ``dataset`` that has a pick table, the picks
    with score > ``threshold`` (all of them when None), mapped from the ``picks_bin`` frame to raw samples, extracted in
    one launch and written as the float32 stack ``out_dir/{name}.mrcs`` (status-0 particles only, pick order); at the
    end ``out_dir/particles.star`` with one row per written particle.  A micrograph without a surviving particle writes
    no stack; micrographs without a pick table are skipped with a warning.  scale = S: stacks of side S by Fourier
    cropping (``bin`` must be 1); the coordinates of ``particles.star`` stay in raw samples either way.  ctf = the
    ``micrographs_ctf.star`` of ``joint ctf``: every row gains its micrograph's CTF columns, ``_rlnDetectorPixelSize``
    multiplied by ``bin`` (or box / S) so that it states the pixel size of the stacks; a micrograph with picks and without a
    row there is a ValueError before anything is extracted.  ctf_correct = "flip" or "multiply" (needs ``ctf``; ``bin``
    must be 1, box and S even, S >= 16): every particle is multiplied in Fourier space by the filter
    ``ctf.correction_filter`` builds from its micrograph's row, before the crop to S and the normalisation; the STAR
    format has no column that says so, downstream tools must be told (``relion_refine --ctf_phase_flipped``).
    -> {name: {"written", "outside", "flat"}} for the micrographs that had a table."""
    if ctf_correct is not None:
        if ctf_correct not in ctf_mod.CORRECTION_MODES:
            raise ValueError("ctf_correct %r (one of %s)" % (ctf_correct, ", ".join(ctf_mod.CORRECTION_MODES)))
        if ctf is None:
            raise ValueError("ctf_correct needs the micrographs_ctf.star of `joint ctf` (ctf)")
        if bin != 1:
            raise ValueError("ctf_correct and bin > 1 exclude one another (use scale)")
        b, bg_radius = check_filter(box, scale, bg_radius)
    elif scale is not None:
        if bin != 1:
            raise ValueError("scale and bin > 1 exclude one another")
        b, bg_radius = check_scale(box, scale, bg_radius)
    else:
        b, bg_radius = check_box(box, bin, bg_radius)
    picks_bin = ingest.check_bin(picks_bin)
    rows = micrograph_io.read_image_table(dataset)
    if not rows:
        raise ValueError("no micrographs found in %s" % dataset)
    tables = read_pick_tables(picks, [name for _, name, _ in rows], picks_bin)
    ctf_cols, ctf_table = None, None
    if ctf is not None:
        ctf_cols = _ctf_columns(ctf, [(name, path) for _, name, path in rows if name in tables and len(tables[name][0])],
                                float(box) / b)
        if ctf_correct is not None:
            ctf_table = ctf_mod.read_ctf_star(ctf)
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
        if ctf_correct is not None:
            phi = _ctf_filter(ctf_table[os.path.basename(path)], box, b, ctf_correct)
            particles, status = _extract_file_filtered(path, xy, box, b, bg_radius, normalize, invert, device, phi)
        elif scale is not None:
            particles, status = _extract_file_scaled(path, xy, box, b, bg_radius, normalize, invert, device)
        else:
            particles, status = _extract_file(path, xy, box, bin, bg_radius, normalize, invert, device)
        ok = np.flatnonzero(status == OK)
        counts[name] = {"written": len(ok), "outside": int((status == OUTSIDE).sum()), "flat": int((status == FLAT).sum())}
        if not len(ok):
            continue
        stack = name + ".mrcs"
        with open(os.path.join(out_dir, stack), "wb") as f:
            micrograph_io.write_mrc(f, particles)
        for k, i in enumerate(ok):
            star.append("%d\t%d\t%06d@%s\t%s\t%s%s\n" % (xy[i, 0], xy[i, 1], k + 1, stack, os.path.basename(path),
                                                        str(scores[i]), ctf_cols[name] if ctf_cols else ""))
    if missing:
        logger.warning("%s: %d micrographs skipped because %s has no pick table for them: %s", dataset, len(missing), picks,
                       ", ".join(missing[:10]) + (" ..." if len(missing) > 10 else ""))
    with open(os.path.join(out_dir, "particles.star"), "w") as f:
        f.write(export.PARTICLES_STAR_HEADER)
        if ctf_cols is not None:
            f.write("".join("_rln%s #%d\n" % (c, 6 + k) for k, c in enumerate(ctf_mod.CTF_STAR_COLUMNS[1:])))
        f.writelines(star)
    logger.info("%s: %d particles of %d micrographs written to %s", dataset, len(star), len(counts), out_dir)
    return counts
