"""Reference-free 2-D classification on the device: the particle stacks of ``joint extract`` in, K class
averages and a class, an in-plane angle and a shift per particle out — the look at the picks that otherwise needs a
RELION / EMAN2 job.

A multi-reference alignment with a divisive start.  Every particle has a class, an angle index a (of ``A_n`` = 360 / step)
and an integer shift (dy, dx), |shift| <= R.  One iteration:

  (a) the bank: every class average at every angle, masked to the radius and normalised to zero mean and unit norm under the
      mask (``torch.ops.sprk.class_transform``), once packed to the D pixels of the mask (the GEMM's K) and once as images;
  (b) Q: every particle at its current shift, packed the same way;
  (c) ``torch.ops.sprk.class_score``: Q against the bank on fp32 MFMA; the best bank row of a particle is its class and angle;
  (d) the shift: ``torch.ops.sprk.align_corr`` of every particle (as it is) with its best bank image, a window of +-R; the first
      maximum of the window in row-major order is the particle's absolute shift (no parabola).  The bank image is zero beyond
      the mask radius <= S/2 - R - 2, so the periodic wrap of the correlation reaches no product that counts;
  (e) ``torch.ops.sprk.class_average``: every particle turned back by its angle (index (A_n - a) mod A_n) at its shift, summed
      per class in a fixed order.

It starts from one class, the plain mean of all particles.  A level runs at most ``iters`` iterations, at least 2, and stops
when no assignment changed; then, while there are fewer than K classes, the min(Kc, K - Kc) largest classes are each split at
the median of their members' scores (``split_classes``), both halves averaged from the aligned particles of the last
iteration.  The level with K classes ends the run.  A class that loses all its members keeps its average and is reported as
empty.

With ``ctf`` (``joint class2d --ctf_weight``) step (e) and the start are Wiener sums instead of plain means, for
stacks that went through ``joint extract --ctf STAR --ctf_correct``: per class IDFT2(sum wn_i DFT2(y_i) / (sum wd_i + tau)),
y_i the particle turned back as in (e), wn and wd the tables ``ctf.weight_tables`` builds from the particle's CTF row
(``torch.ops.sprk.class_transform`` into images, then ``class_spectrum``, ``class_wiener`` and ``class_synthesize``).
Turning a particle back by the angle index a turns its CTF with it: a row with DefocusU != DefocusV gets a table per (row, a)
that occurs, at DefocusAngle + 360 a / A_n.  Scoring, the shift search and the splitting are the same.

Not covered: scoring against CTF-modulated references, stacks that were not CTF-corrected, per-particle defocus, soft
(probabilistic) assignment, sub-pixel shifts, boxes that are not 64 or 128 pixels."""
import logging
import os

import numpy as np

from . import micrograph_io

logger = logging.getLogger(__name__)

DEFAULT_ANGLE_STEP = 5.0
DEFAULT_MAX_SHIFT = 3
DEFAULT_ITERS = 8
MAX_ANGLES = 720                                 # torch_ops.CLASS_MAX_ANGLES
MAX_SHIFT = 31                                   # torch_ops.ALIGN_MAX_SHIFT
SIDES = (64, 128)                                # align_corr needs Sx % 64 == 0, class_transform S <= 128
CORR_CHUNK = 65535                               # particles per align_corr call at most
STAR_COLUMNS = ("ClassNumber", "AnglePsi", "OriginX", "OriginY")
DEFAULT_WIENER = 1.0                             # tau of the Wiener sums: 1 / SNR per particle and bin
CTF_COLUMNS = ("DefocusU", "DefocusV", "DefocusAngle", "Voltage", "SphericalAberration", "AmplitudeContrast", "Magnification",
               "DetectorPixelSize")              # what --ctf_weight reads from particles.star


def angle_count(angle_step):
    """-> A_n = 360 / step, which must be an integer in 1..720"""
    if not angle_step > 0:
        raise ValueError("--angle_step %r: a positive number of degrees that divides 360 (5 is the default)" % (angle_step,))
    A_n = int(round(360.0 / angle_step))
    if not 1 <= A_n <= MAX_ANGLES or abs(A_n * angle_step - 360.0) > 1e-9 * 360.0:
        raise ValueError("--angle_step %r: 360 / step must be an integer in 1..%d (try 5, 6, 7.5 or 10)"
                         % (angle_step, MAX_ANGLES))
    return A_n


def default_radius(S, R):
    return S // 2 - R - 2


def check_class2d_args(classes, angle_step=DEFAULT_ANGLE_STEP, max_shift=DEFAULT_MAX_SHIFT, radius=None,
                       iters=DEFAULT_ITERS):
    """What can be refused before a file is read -> A_n."""
    if classes < 1:
        raise ValueError("--classes %d: at least 1 class" % classes)
    A_n = angle_count(angle_step)
    if not 1 <= max_shift <= MAX_SHIFT:
        raise ValueError("--max_shift %d: the shift search covers 1..%d pixels (3 is the default)" % (max_shift, MAX_SHIFT))
    if radius is not None and radius < 1:
        raise ValueError("--radius %d: a mask radius of at least 1 pixel (default: S/2 - max_shift - 2)" % radius)
    if iters < 2:
        raise ValueError("--iters %d: a level runs at least 2 iterations (8 is the default)" % iters)
    return A_n


def check_ctf_weight(mode, tau):
    """``--ctf_weight`` and ``--wiener`` -> tau (the default where None), or ValueError"""
    from .ctf import CORRECTION_MODES
    if mode is None:
        if tau is not None:
            raise ValueError("--wiener %r belongs to the Wiener-weighted averages: give --ctf_weight flip (or multiply: what "
                             "`joint extract --ctf_correct` was given) as well" % (tau,))
        return None
    if mode not in CORRECTION_MODES:
        raise ValueError("--ctf_weight %r: one of %s, what `joint extract --ctf_correct` was given" % (mode, ", ".join(CORRECTION_MODES)))
    tau = DEFAULT_WIENER if tau is None else float(tau)
    if not (np.isfinite(tau) and tau > 0):
        raise ValueError("--wiener %r: a finite number > 0, 1 / SNR per particle and frequency (1.0 is the default)" % (tau,))
    return tau


def ctf_rows(labels, rows, path="particles.star"):
    """The CTF columns of a ``particles.star`` -> (index int64 [N]: each particle's row of ``table``, table float64 [M, 7]:
    the distinct (DefocusU, DefocusV, DefocusAngle, kV, Cs, Q, apix of the stack) in order of appearance), apix =
    DetectorPixelSize . 10^4 / Magnification.  ValueError when a column is missing."""
    missing = [c for c in CTF_COLUMNS if c not in labels]
    if missing:
        raise ValueError("%s: --ctf_weight needs the column%s _rln%s; write the stacks with `joint extract --ctf STAR "
                         "--ctf_correct flip`" % (path, "s" if len(missing) > 1 else "", ", _rln".join(missing)))
    cols = [labels.index(c) for c in CTF_COLUMNS]
    seen, index, table = {}, [], []
    for row in rows:
        fields = row.split()
        key = tuple(fields[c] for c in cols)
        if key not in seen:
            u, v, angle, kv, cs, q, mag, dps = (float(x) for x in key)
            if not (mag > 0 and dps > 0):
                raise ValueError("%s: Magnification %r and DetectorPixelSize %r must be positive" % (path, key[6], key[7]))
            seen[key] = len(table)
            table.append((u, v, angle, kv, cs, q, dps * 1e4 / mag))
        index.append(seen[key])
    return np.array(index, dtype=np.int64), np.array(table, dtype=np.float64).reshape(-1, 7)


def ctf_groups(index, table, inv, A_n):
    """The weight tables an averaging step needs beyond one per row -> (group int64 [N], extra float64 [G - M, 7]): a particle
    of a row with DefocusU == DefocusV uses table ``index`` (the row as it is); the distinct (row, a) pairs of the others, a
    = ``inv`` the angle index the particle is turned back by, follow from M on, each the row at DefocusAngle + 360 a / A_n."""
    index, inv = np.asarray(index, dtype=np.int64), np.asarray(inv, dtype=np.int64)
    astig = (table[:, 0] != table[:, 1])[index]
    group = index.copy()
    if not astig.any():
        return group, np.zeros((0, 7))
    keys, where = np.unique(index[astig] * A_n + inv[astig], return_inverse=True)
    extra = table[keys // A_n].copy()
    extra[:, 2] += 360.0 * (keys % A_n) / A_n
    group[astig] = len(table) + where
    return group, extra


def check_geometry(S, N, classes, max_shift, radius=None):
    """What depends on the stacks -> the mask radius.  Before any launch."""
    if S not in SIDES:
        raise ValueError("particles of side %d: the classification takes boxes of 64 or 128 pixels (the correlation kernel "
                         "needs a multiple of 64, the transform at most 128); extract them with `joint extract --scale 64`"
                         % S)
    if classes < 1 or classes > N:
        raise ValueError("--classes %d with %d particles: at least 1 class and at most one per particle (lower --classes)"
                         % (classes, N))
    limit = default_radius(S, max_shift)
    if limit < 1:
        raise ValueError("--max_shift %d leaves no mask in a box of %d pixels (S/2 - max_shift - 2 = %d): lower --max_shift"
                         % (max_shift, S, limit))
    if radius is None:
        return limit
    if not 1 <= radius <= limit:
        raise ValueError("--radius %d: at most S/2 - max_shift - 2 = %d pixels (the shift search wraps at the box edges); "
                         "lower --radius or --max_shift" % (radius, limit))
    return radius


def angle_table(A_n):
    """-> float32 [A_n, 2]: (cos, sin) of 2 pi a / A_n, formed in float64 and rounded once"""
    a = 2.0 * np.pi * np.arange(A_n, dtype=np.float64) / A_n
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)


def packed_pixels(S, radius):
    """-> int32 [D]: the linear indices of the pixels with (i - S/2)^2 + (j - S/2)^2 <= radius^2, ascending"""
    c = S // 2
    i, j = np.mgrid[0:S, 0:S]
    return np.flatnonzero(((i - c) ** 2 + (j - c) ** 2 <= radius * radius).ravel()).astype(np.int32)


def split_classes(cls, scores, Kc, K):
    """The divisive step.  cls int [N] in 0 .. Kc-1, scores [N] -> (new cls, parents): the min(Kc, K - Kc) largest classes
    (ties in size by a stable sort: the lower class first) are each split at the median of their members' scores; members
    at or above it keep the class, the rest found class Kc + t, t the rank of their parent among the split ones."""
    cls = np.array(cls, dtype=np.int64)
    scores = np.asarray(scores, dtype=np.float64)
    sizes = np.bincount(cls, minlength=Kc)
    order = np.argsort(-sizes, kind="stable")[:min(Kc, K - Kc)]
    for t, k in enumerate(order):
        members = np.flatnonzero(cls == k)
        if len(members):
            cls[members[scores[members] < np.median(scores[members])]] = Kc + t
    return cls, [int(k) for k in order]


def classify(P, classes, angle_step=DEFAULT_ANGLE_STEP, max_shift=DEFAULT_MAX_SHIFT, radius=None, iters=DEFAULT_ITERS,
             ctf=None):
    """P: float32 CUDA tensor [N, S, S], all particles on the device -> dict: ``cls`` int [N], ``ang`` int [N] (angle index),
    ``shift`` int [N, 2] (dy, dx: the aligned particle is P[i + dy, j + dx]), ``scores`` float32 [N], ``averages`` float32
    [K, S, S], ``levels`` [(classes, iterations used)], ``A_n`` and ``radius``; all NumPy.
    ctf = (index int [N], table [M, 7], mode, tau): Wiener-weighted averages; each particle's row of ``table`` (``ctf_rows``),
    the mode ``joint extract --ctf_correct`` was given and tau of ``check_ctf_weight``."""
    import torch
    from . import torch_ops  # noqa: F401  (registers torch.ops.sprk)
    A_n = check_class2d_args(classes, angle_step, max_shift, radius, iters)
    if not (isinstance(P, torch.Tensor) and P.is_cuda and P.dtype == torch.float32 and P.dim() == 3
            and P.shape[1] == P.shape[2]):
        raise ValueError("classify: P must be a float32 CUDA tensor [N, S, S]")
    N, S, _ = P.shape
    K, R = classes, max_shift
    radius = check_geometry(S, N, K, R, radius)
    P = P.contiguous()
    dev = P.device
    ops = torch.ops.sprk

    def i32(a):
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=dev)

    cs = torch.as_tensor(angle_table(A_n), device=dev)
    pix = i32(packed_pixels(S, radius))
    D = int(pix.numel())
    ldo = (D + 3) & ~3
    flags = torch_ops.CLASS_MASK | torch_ops.CLASS_NORMALIZE
    avgs = torch.zeros((K, S, S), dtype=torch.float32, device=dev)
    bank = torch.empty((K * A_n, ldo), dtype=torch.float32, device=dev)
    bank_images = torch.empty((K * A_n, S, S), dtype=torch.float32, device=dev)
    Q = torch.empty((N, ldo), dtype=torch.float32, device=dev)
    best_score = torch.empty(N, dtype=torch.float32, device=dev)
    best_index = torch.empty(N, dtype=torch.int32, device=dev)
    everyone = torch.arange(N, dtype=torch.int32, device=dev)
    zeros = torch.zeros(N, dtype=torch.int32, device=dev)
    cls = torch.zeros(N, dtype=torch.int64, device=dev)
    ang = torch.zeros(N, dtype=torch.int32, device=dev)
    shift = torch.zeros((N, 2), dtype=torch.int32, device=dev)
    n = 2 * R + 1
    if ctf is not None:
        from . import ctf as ctf_mod, extract
        ctf_index, ctf_table, ctf_mode, tau = ctf
        ctf_index, ctf_table = np.asarray(ctf_index, dtype=np.int64), np.asarray(ctf_table, dtype=np.float64).reshape(-1, 7)
        tau = check_ctf_weight(ctf_mode, tau)
        if ctf_index.shape != (N,) or not len(ctf_table) or ctf_index.min() < 0 or ctf_index.max() >= len(ctf_table):
            raise ValueError("classify: ctf needs one row index per particle into a table [M, 7]")
        w1, w2, w3, w4 = extract.filter_matrices(S, S, dev)
        base_wn, base_wd = ctf_mod.weight_tables(S, ctf_table, ctf_mode, dev)            # (row, 0): once per run
        aligned = torch.empty((N, S, S), dtype=torch.float32, device=dev)
        spec = torch.empty((N,) + torch_ops.class_spectrum_shapes(S)[4], dtype=torch.float32, device=dev)
        fsum = torch.zeros((K,) + tuple(spec.shape[1:]), dtype=torch.float32, device=dev)   # an empty class keeps its spectrum

    def average(Kc):
        """avgs[:Kc] from the state: members grouped by class, ascending within a class"""
        members = torch.argsort(cls, stable=True).to(torch.int32)
        offsets = torch.zeros(Kc + 1, dtype=torch.int32, device=dev)
        offsets[1:] = torch.cumsum(torch.bincount(cls, minlength=Kc), 0).to(torch.int32)
        inv = ((A_n - ang) % A_n).to(torch.int32)
        if ctf is None:
            ops.class_average(P, inv, shift, cs, members, offsets, avgs[:Kc])
            return
        ops.class_transform(P, everyone, inv, shift, cs, 0, 0, None, aligned)
        ops.class_spectrum(aligned, w1, w2, 0, spec)
        group, extra = ctf_groups(ctf_index, ctf_table, inv.cpu().numpy(), A_n)
        wn, wd = base_wn, base_wd
        if len(extra):
            more = ctf_mod.weight_tables(S, extra, ctf_mode, dev)
            wn, wd = torch.cat([wn, more[0]]), torch.cat([wd, more[1]])
        ops.class_wiener(spec, S, wn, wd, i32(group), members, offsets, tau, fsum[:Kc])
        ops.class_synthesize(fsum[:Kc], S, w3, w4, avgs[:Kc])

    average(1)                                                   # the plain mean: angle 0, shift 0, one class
    Kc, levels = 1, []
    while True:
        used = 0
        rows = Kc * A_n
        bank_src = i32(np.repeat(np.arange(Kc), A_n))
        bank_ang = i32(np.tile(np.arange(A_n), Kc))
        bank_shift = torch.zeros((rows, 2), dtype=torch.int32, device=dev)
        for it in range(iters):
            used = it + 1
            ops.class_transform(avgs[:Kc], bank_src, bank_ang, bank_shift, cs, radius, flags, pix, bank[:rows])
            ops.class_transform(avgs[:Kc], bank_src, bank_ang, bank_shift, cs, radius, flags, None, bank_images[:rows])
            ops.class_transform(P, everyone, zeros, shift, cs, radius, 0, pix, Q)
            ops.class_score(Q, bank[:rows], ldo, None, best_score, best_index)
            best = best_index.to(torch.int64)
            new_cls, new_ang = best // A_n, (best % A_n).to(torch.int32)
            new_shift = torch.empty_like(shift)
            for c0 in range(0, N, CORR_CHUNK):
                c1 = min(N, c0 + CORR_CHUNK)
                cc = ops.align_corr(P[c0:c1], bank_images[best[c0:c1]], R, 0)
                peak = cc.reshape(c1 - c0, n * n).argmax(dim=1)  # the first maximum in row-major order
                new_shift[c0:c1, 0] = (R - peak // n).to(torch.int32)
                new_shift[c0:c1, 1] = (R - peak % n).to(torch.int32)
            same = bool((torch.equal(new_cls, cls) and torch.equal(new_ang, ang) and torch.equal(new_shift, shift)))
            cls, ang, shift = new_cls, new_ang, new_shift
            average(Kc)
            if same and used >= 2:
                break
        levels.append((Kc, used))
        if Kc >= K:
            break
        host_cls, parents = split_classes(cls.cpu().numpy(), best_score.cpu().numpy(), Kc, K)
        cls = torch.as_tensor(host_cls, device=dev)
        avgs[Kc:Kc + len(parents)] = avgs[torch.as_tensor(parents, device=dev)]   # an empty half starts as its parent
        if ctf is not None:
            fsum[Kc:Kc + len(parents)] = fsum[torch.as_tensor(parents, device=dev)]
        Kc += len(parents)
        average(Kc)
    return {"cls": cls.cpu().numpy(), "ang": ang.cpu().numpy().astype(np.int64), "shift": shift.cpu().numpy().astype(np.int64),
            "scores": best_score.cpu().numpy(), "averages": avgs.cpu().numpy(), "levels": levels, "A_n": A_n,
            "radius": radius}


# ---- files -------------------------------------------------------------------------------------------------------------------
def read_particles_star(path):
    """``particles.star`` -> (head, labels, rows): the lines up to and including the last label line verbatim, the label
    names without ``_rln``, and the data rows verbatim (without their line ends)"""
    with open(path) as f:
        lines = f.read().split("\n")
    last = max((k for k, line in enumerate(lines) if line.strip().startswith("_rln")), default=-1)
    if last < 0:
        raise ValueError("%s: no _rln column labels (is it the particles.star of `joint extract`?)" % path)
    labels = [line.split()[0][4:] for line in lines[:last + 1] if line.strip().startswith("_rln")]
    rows = [line for line in lines[last + 1:] if line.strip()]
    if "ImageName" not in labels:
        raise ValueError("%s: no column _rlnImageName" % path)
    for row in rows:
        if len(row.split()) != len(labels):
            raise ValueError("%s: a row of %d fields under %d labels: %r" % (path, len(row.split()), len(labels), row))
    return lines[:last + 1], labels, rows


def load_particles(star):
    """-> (P float32 [N, S, S] NumPy, head, labels, rows, header of the first stack): the images that ``_rlnImageName``
    (``000001@name.mrcs``, relative to the STAR file) names, in row order"""
    head, labels, rows = read_particles_star(star)
    if not rows:
        raise ValueError("%s lists no particles" % star)
    col = labels.index("ImageName")
    base = os.path.dirname(os.path.abspath(star))
    stacks, first, images = {}, None, []
    for row in rows:
        number, _, name = row.split()[col].partition("@")
        if name not in stacks:
            with open(os.path.join(base, name), "rb") as f:
                array, header, _ = micrograph_io.parse_mrc(f.read())
            if header.mode != 2:
                raise ValueError("%s: mode %d; the stacks of `joint extract` are float32 (mode 2)" % (name, header.mode))
            array = array.reshape(header.nz, header.ny, header.nx)
            if first is None:
                first = header
            if header.ny != header.nx or (header.ny, header.nx) != (first.ny, first.nx):
                raise ValueError("%s holds images of %dx%d, %s of %dx%d: all stacks must have one square box; extract "
                                 "them again with one `joint extract --scale 64`"
                                 % (name, header.ny, header.nx, rows[0].split()[col].partition("@")[2], first.ny, first.nx))
            stacks[name] = array
        k = int(number) - 1
        if not 0 <= k < len(stacks[name]):
            raise ValueError("%s: image %s of a stack of %d" % (name, number, len(stacks[name])))
        images.append(stacks[name][k])
    return np.stack(images).astype(np.float32), head, labels, rows, first


def star_columns(labels):
    """-> the label lines that ``particles_class2d.star`` adds: the numbering continues whatever columns the input has"""
    return ["_rln%s #%d" % (c, len(labels) + 1 + k) for k, c in enumerate(STAR_COLUMNS)]


def write_averages(path, averages, header):
    """K float32 averages as an MRC stack with the pixel size of the input stack's ``header`` (xlen / mx)"""
    averages = np.ascontiguousarray(averages, dtype=np.float32)
    K, S, _ = averages.shape
    apix = header.xlen / header.mx if header.mx > 0 else 1.0
    h = header._replace(nx=S, ny=S, nz=K, mode=2, mx=S, my=S, mz=K, xlen=apix * S, ylen=apix * S, zlen=apix * K,
                        amin=float(averages.min()), amax=float(averages.max()), amean=float(averages.mean()),
                        rms=float(averages.std()), next=0)
    with open(path, "wb") as f:
        f.write(micrograph_io._HEADER.pack(*h))
        f.write(averages.tobytes())


def class2d_dataset(particles, out_dir, classes, angle_step=DEFAULT_ANGLE_STEP, max_shift=DEFAULT_MAX_SHIFT, radius=None,
                    iters=DEFAULT_ITERS, device="cuda", ctf_weight=None, wiener=None):
    """``joint class2d``: the particles of ``particles`` (the STAR file of ``joint extract``) classified into ``classes``
    classes; writes ``classes.mrcs``, ``particles_class2d.star`` (the input rows and header verbatim plus _rlnClassNumber,
    1-based, _rlnAnglePsi in degrees: the in-plane rotation of the class average that fits the particle, and _rlnOriginX /
    _rlnOriginY in pixels of the stack: the displacement that aligns the particle) and ``class2d.txt`` into ``out_dir``.
    ctf_weight = "flip" or "multiply", what ``joint extract --ctf_correct`` was given (the STAR file has no column for it):
    the averages are Wiener sums with tau = ``wiener`` (default 1.0) over the CTF columns of ``particles``, which must be
    there (refused before any stack is read); the STAR output is the same.
    -> {"particles", "classes": [{"members", "mean_score"}], "levels"}"""
    import torch
    A_n = check_class2d_args(classes, angle_step, max_shift, radius, iters)
    tau = check_ctf_weight(ctf_weight, wiener)
    ctf = None
    if ctf_weight is not None:
        _, labels, rows = read_particles_star(particles)
        ctf = ctf_rows(labels, rows, particles) + (ctf_weight, tau)
    P, head, labels, rows, header = load_particles(particles)
    radius = check_geometry(P.shape[1], len(P), classes, max_shift, radius)
    res = classify(torch.as_tensor(P, device=device), classes, angle_step, max_shift, radius, iters, ctf=ctf)
    os.makedirs(out_dir, exist_ok=True)
    write_averages(os.path.join(out_dir, "classes.mrcs"), res["averages"], header)
    step = 360.0 / A_n
    with open(os.path.join(out_dir, "particles_class2d.star"), "w") as f:
        f.write("\n".join(head + star_columns(labels)) + "\n")
        for k, row in enumerate(rows):
            f.write("%s\t%d\t%s\t%d\t%d\n" % (row, res["cls"][k] + 1, repr(float(res["ang"][k] * step)),
                                             -res["shift"][k, 1], -res["shift"][k, 0]))
    summary = []
    for k in range(classes):
        mem = res["cls"] == k
        summary.append({"members": int(mem.sum()), "mean_score": float(res["scores"][mem].mean()) if mem.any() else 0.0})
    with open(os.path.join(out_dir, "class2d.txt"), "w") as f:
        f.write("# %d particles of %dx%d, %d classes, %d angles, max shift %d, mask radius %d%s\n"
                % (len(P), P.shape[1], P.shape[2], classes, A_n, max_shift, radius,
                   "" if ctf is None else ", ctf_weight %s, wiener %s" % (ctf_weight, repr(tau))))
        f.write("# class\tmembers\tmean_score\n")
        for k, s in enumerate(summary):
            f.write("%d\t%d\t%s\n" % (k + 1, s["members"], repr(s["mean_score"]) if s["members"] else "empty"))
        f.write("# level (classes)\titerations\n")
        for Kc, used in res["levels"]:
            f.write("%d\t%d\n" % (Kc, used))
    logger.info("%s: %d particles in %d classes written to %s", particles, len(P), classes, out_dir)
    return {"particles": len(P), "classes": summary, "levels": [list(l) for l in res["levels"]]}
