"""``joint`` command line (cli/cli.py, cli/cmds/train.py:24-300, cli/cmds/eval.py:15-71 of the
reference): ``joint train start|resume`` and ``joint eval`` with the same flags and the same
flag -> configuration mapping, plus ``joint bin`` (the README's ``newstack -bin`` preparation, on the GPU), ``joint extract``
(particle stacks from the pick tables and the raw micrographs, on the GPU) and ``joint ctf`` (tiled power spectra of the raw
micrographs on the GPU, one fitted defocus each, or with ``--astigmatism`` two and an angle, ``micrographs_ctf.star`` for
``joint extract --ctf``, which with ``--ctf_correct`` also phase-flips the stacks) and ``joint align`` (whole-frame motion
correction of movies on the GPU, the sums the other commands start from; with ``--dose`` a dose-weighted sum beside the plain
one, with ``--patch`` a smooth local field on top of the whole-frame shifts).
Run as ``python -m spr_pick_amd ...``; for several GPUs launch it
under ``python -m torch.distributed.run --nproc-per-node N -m spr_pick_amd -- ...`` (keep the ``--``)."""
import argparse

from . import __version__, cfg as cfg_mod
from .params import ConfigValue, NoiseAlgorithm, NoiseValue


def _shared_train_args(p, start):
    p.add_argument("--train_dataset", "-t", required=start, help="Tab-separated table (image_name, path) of training micrographs.")
    p.add_argument("--alpha", "-ap", type=float, required=start, help="alpha value")
    p.add_argument("--tau", "-tau", type=float, required=start,
                   help="tau value for positive unlabeled learning - percentage of positives")
    p.add_argument("--train_gt", "-gt", help="Path to ground truth dataset")
    p.add_argument("--train_label", "-l", required=start, help="Particle coordinates table (image_name, x_coord, y_coord).")
    p.add_argument("--validation_dataset", "-v", help="Table of validation micrographs.")
    p.add_argument("--validation_label", "-vl", help="Validation particle coordinates.")
    p.add_argument("--validation_gt", "-vgt", help="Path to validation ground truth dataset")
    p.add_argument("--iterations", "-iter", required=start, type=int, help="Number of joint training iterations")
    p.add_argument("--num", "-num", type=int, default=1, help="Number of eval samples during training")
    p.add_argument("--lr", "-lr", type=float, help="learning rate")
    p.add_argument("--nms", "-nms", type=int, help="non_maximum suppression radius")
    p.add_argument("--bb", "-bb", type=int, help="bounding box radius for particle of interests")
    p.add_argument("--eval_interval", type=int, help="Iterations between evaluations.")
    p.add_argument("--checkpoint_interval", type=int, help="Iterations between checkpoints.")
    p.add_argument("--print_interval", type=int, help="Iterations between progress lines.")
    p.add_argument("--train_batch_size", type=int, help="Batch size to use for training images.")
    p.add_argument("--validation_batch_size", type=int, help="Batch size to use for validation images.")
    p.add_argument("--patch_size", type=int, help="Patch size to use for training (square).")
    p.add_argument("--fraction", help="percent fraction of frames.")


def _bin_factor(text):
    """--bin N: an integer in 1..ingest.MAX_BIN (= SPRK_INGEST_MAX_BIN; imported here so that the parser alone stays light)."""
    from .ingest import MAX_BIN
    try:
        n = int(text)
    except ValueError:
        n = 0
    if not 1 <= n <= MAX_BIN:
        raise argparse.ArgumentTypeError("bin factor must be an integer in 1..%d, got %r" % (MAX_BIN, text))
    return n


def _ftbin(text):
    """--ftbin F: ingest.check_ftbin of the decimal (or p/q) text, its ValueError as the parser's usage error."""
    from .ingest import check_ftbin
    try:
        return check_ftbin(str(text))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def _clip(text):
    """--clip LO[,HI]: ingest.parse_clip, its ValueError as the parser's usage error."""
    from .ingest import parse_clip
    try:
        return parse_clip(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def _flatten(text):
    """--flatten R: ingest.check_flatten of an integer, its ValueError as the parser's usage error."""
    from .ingest import check_flatten
    try:
        return check_flatten(int(text))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


class _Parser(argparse.ArgumentParser):
    """A (sub-)parser may carry ``check``: arguments validated against each other at parse time (ValueError -> the
    parser's usage error), so that `--box 100 --bin 3` is refused like any other bad value and not by a traceback."""
    check = None

    def parse_known_args(self, args=None, namespace=None):
        ns, rest = super().parse_known_args(args, namespace)
        if self.check is not None:
            try:
                self.check(ns)
            except ValueError as e:
                self.error(str(e))
        return ns, rest


def _check_eval(ns):
    if ns.bin is not None and ns.ftbin is not None:
        raise ValueError("--bin and --ftbin exclude one another")
    raw = ns.bin is not None or ns.ftbin is not None
    if ns.clip is not None and not raw:
        raise ValueError("--clip belongs to the raw-micrograph ingest: give --bin N as well (N = 1 for unbinned files)")
    if ns.flatten is not None and not raw:
        raise ValueError("--flatten belongs to the raw-micrograph ingest: give --bin N as well (N = 1 for unbinned files)")


def _check_bin(ns):
    if ns.bin is not None and ns.ftbin is not None:
        raise ValueError("--bin and --ftbin exclude one another")
    if ns.bin is None and ns.ftbin is None:
        raise ValueError("one of the arguments --bin --ftbin is required")


def _check_extract(ns):
    from .extract import check_box, check_filter, check_scale
    if ns.ctf_correct is not None:
        if ns.ctf is None:
            raise ValueError("--ctf_correct needs --ctf STAR (the micrographs_ctf.star of `joint ctf`)")
        if ns.bin > 1:
            raise ValueError("--ctf_correct and --bin %d exclude one another: use --scale S for smaller stacks" % ns.bin)
        check_filter(ns.box, ns.scale, ns.bg_radius)
        return
    if ns.scale is None:
        check_box(ns.box, ns.bin, ns.bg_radius)
        return
    if ns.bin > 1:
        raise ValueError("--scale and --bin %d exclude one another (binning before the Fourier crop is not implemented)" % ns.bin)
    check_scale(ns.box, ns.scale, ns.bg_radius)


def _check_ctf(ns):
    from .ctf import check_fit_args, check_tile
    check_tile(ns.tile)
    check_fit_args(ns.apix, ns.kv, ns.cs, ns.ac, ns.min_res, ns.max_res, ns.min_defocus, ns.max_defocus)
    if ns.max_astigmatism is not None and not ns.astigmatism:
        raise ValueError("--max_astigmatism belongs to the 2-D fit: give --astigmatism as well")
    if ns.astigmatism:
        from .ctf import MAX_ASTIGMATISM, check_astigmatism
        check_astigmatism(MAX_ASTIGMATISM if ns.max_astigmatism is None else ns.max_astigmatism, ns.min_defocus)


def _check_class2d(ns):
    from .class2d import check_class2d_args
    check_class2d_args(ns.classes, ns.angle_step, ns.max_shift, ns.radius, ns.iters)
    from .class2d import check_ctf_weight
    check_ctf_weight(ns.ctf_weight, ns.wiener)


def _check_align(ns):
    from .align import check_align_args
    check_align_args(ns.align_size, ns.max_shift, ns.iters)
    from .moviefix import check_fix_args
    if ns.gain is None and (ns.gain_rot is not None or ns.gain_flip is not None):
        raise ValueError("--gain_rot and --gain_flip turn the gain reference: give --gain G as well")
    check_fix_args(ns.gain, ns.gain_rot or 0, ns.gain_flip, ns.dark, ns.defects, ns.hot_sigma)
    if ns.patch is None:
        for flag in ("patch_shift", "patch_iters"):
            if getattr(ns, flag) is not None:
                raise ValueError("--%s belongs to the local motion: give --patch PY,PX as well" % flag)
    else:
        from . import localmotion
        if ns.no_align:
            raise ValueError("--patch fits a local field on top of the whole-frame shifts: it does not go with --no_align")
        localmotion.check_patch_args(localmotion.parse_patch(ns.patch),
                                     localmotion.DEFAULT_PATCH_SHIFT if ns.patch_shift is None else ns.patch_shift,
                                     localmotion.DEFAULT_PATCH_ITERS if ns.patch_iters is None else ns.patch_iters)
    if ns.dose is None:
        for flag in ("pre_dose", "kv", "apix"):
            if getattr(ns, flag) is not None:
                raise ValueError("--%s belongs to the dose weighting: give --dose E as well" % flag)
        return
    from .dose import check_dose_args
    check_dose_args(ns.dose, 0.0 if ns.pre_dose is None else ns.pre_dose, 300.0 if ns.kv is None else ns.kv, ns.apix)


def build_parser():
    parser = _Parser(prog="joint", description="Joint denoising + particle picking on MI355X "
                                     "(train / evaluate), drop-in for spr_pick's `joint` command.")
    parser.add_argument("--version", action="version", version="%(prog)s v" + __version__)
    cmds = parser.add_subparsers(dest="command", required=True)

    train = cmds.add_parser("train", help="Train or resume training of a Denoiser model.")
    actions = train.add_subparsers(dest="train_cmd", required=True)
    start = actions.add_parser("start", help="start a new run")
    _shared_train_args(start, True)
    start.add_argument("--algorithm", "-a", required=True, choices=[a.value for a in NoiseAlgorithm],
                       help="The algorithm to train.")
    start.add_argument("--noise_style", "-n", required=True, help="Noise style, e.g. 'gaussian'.")
    start.add_argument("--noise_value", choices=[v.value for v in NoiseValue],
                       help="[joint] Whether the noise value should be estimated.")
    start.add_argument("--dn_only", action="store_true", help="denoising only")
    start.add_argument("--runs_dir", default=cfg_mod.DEFAULT_RUN_DIR,
                       help="Directory in which the output directory is generated.")
    resume = actions.add_parser("resume", help="Resume a run from its latest *.training file.")
    resume.add_argument("run_dir", help="Path to run directory to resume.")
    _shared_train_args(resume, False)

    ev = cmds.add_parser("eval", help="Evaluate a pre-trained model.")
    ev.add_argument("--model", "-m", required=True, help="Path to model weights or training file.")
    ev.add_argument("--dataset", "-d", required=True, help="Table of micrographs to evaluate.")
    ev.add_argument("--runs_dir", default=cfg_mod.DEFAULT_RUN_DIR,
                    help="Directory in which the output directory is generated.")
    ev.add_argument("--batch_size", type=int, help="Batch size to use, defaults to that used while training.")
    ev.add_argument("--gt_dataset", "-g", help="ground truth image")
    ev.add_argument("--nms", "-nms", type=int, help="non maximum suppression radius")
    ev.add_argument("--num", "-num", type=int, default=10, help="Number of micrographs to evaluate")
    ev.add_argument("--contamination", action="store_true",
                    help="exclude picks on ice contamination, carbon edges and holes (the reference's find_contamination, "
                         "computed on the GPU); writes {name}_contam.png")
    ev.add_argument("--bin", type=_bin_factor, metavar="N",
                    help="the dataset holds RAW micrographs (MRC mode 0/1/2/6): bin each N x N, normalise and pad it on "
                         "the GPU instead of preparing binned copies; for N > 1 also writes {name}_scores_unbinned.txt")
    ev.add_argument("--ftbin", type=_ftbin, metavar="F",
                    help="instead of --bin: Fourier-crop each RAW micrograph by the factor F (any decimal or p/q in 1..64, "
                         "e.g. 9.64) to round(ny / F) x round(nx / F) pixels on the GPU: no aliasing, no margin dropped, "
                         "periodic at the edges like newstack -ftreduce; writes {name}_scores_unbinned.txt when the size changes")
    ev.add_argument("--clip", type=_clip, metavar="LO[,HI]",
                    help="with --bin or --ftbin: clamp each binned micrograph to its LO %% / (100 - HI) %% order statistics before the "
                         "min-max normalisation, so that hot pixels and black spots do not set the range (HI = LO when "
                         "omitted; 0 changes nothing)")
    ev.add_argument("--flatten", type=_flatten, metavar="R",
                    help="with --bin or --ftbin: subtract from each binned micrograph its mean over a (2R+1) x (2R+1) window (R in "
                         "binned pixels, 1..1023) before the min-max normalisation, so that a slow gradient does not take "
                         "the grey levels; with --clip: clip, flatten, clip again")
    ev.check = _check_eval

    bn = cmds.add_parser("bin", help="Bin raw micrographs N x N on the GPU (replaces the `newstack -bin N` preparation).")
    bn.add_argument("--dataset", "-d", required=True, help="Table (image_name, path) or directory of raw MRC micrographs.")
    bn.add_argument("--bin", type=_bin_factor, metavar="N", help="bin factor (at most 16, SPRK_INGEST_MAX_BIN)")
    bn.add_argument("--ftbin", type=_ftbin, metavar="F",
                    help="instead of --bin: Fourier-crop by the factor F (any decimal or p/q in 1..64) to round(ny / F) x "
                         "round(nx / F) pixels, as `joint eval --ftbin F` sees the micrographs; one of the two is required")
    bn.add_argument("--out", "-o", required=True, help="Directory for {name}.mrc (float32), images.txt and labels.txt.")
    bn.add_argument("--labels", "-l", help="Particle coordinates of the raw micrographs; written binned to labels.txt.")
    bn.add_argument("--clip", type=_clip, metavar="LO[,HI]",
                    help="write the block means clamped to their LO %% / (100 - HI) %% order statistics (as `joint eval "
                         "--bin N --clip` sees them); HI = LO when omitted")
    bn.add_argument("--flatten", type=_flatten, metavar="R",
                    help="write the block means minus their mean over a (2R+1) x (2R+1) window (as `joint eval --bin N "
                         "--flatten R` sees them); with --clip: clip, flatten, clip again")
    bn.check = _check_bin

    ex = cmds.add_parser("extract", help="Cut normalised particle stacks out of raw micrographs on the GPU "
                                         "(replaces the relion_preprocess step after picking).")
    ex.add_argument("--dataset", "-d", required=True, help="Table (image_name, path) or directory of raw MRC micrographs.")
    ex.add_argument("--picks", "-p", required=True,
                    help="Directory of {name}_scores_unbinned.txt / {name}_scores.txt pick tables (joint eval's eval_imgs), "
                         "or one scores file.")
    ex.add_argument("--box", "-b", type=int, required=True, metavar="B", help="box side in raw samples (2..1024, a multiple of --bin)")
    ex.add_argument("--out", "-o", required=True, help="Directory for {name}.mrcs (float32 stacks) and particles.star.")
    ex.add_argument("--bin", type=_bin_factor, default=1, metavar="N", help="bin every box N x N: stacks of side B / N")
    ex.add_argument("--scale", type=int, metavar="S",
                    help="Fourier-crop every box to S x S pixels (any 2 <= S <= B; relion_preprocess --scale): no aliasing, "
                         "no divisibility rule; excludes --bin N > 1")
    ex.add_argument("--picks_bin", type=_bin_factor, default=1, metavar="K",
                    help="the pick tables are in the frame of `joint eval --bin K` ({name}_scores.txt); default 1: raw samples")
    ex.add_argument("--bg_radius", type=int, metavar="R",
                    help="background = output pixels farther than R from the box centre (default 3/8 of B / N, or of S)")
    ex.add_argument("--threshold", type=float, metavar="S", help="keep picks with score > S (default: all)")
    ex.add_argument("--invert", action="store_true", help="invert the contrast")
    ex.add_argument("--no_norm", action="store_true", help="block means only, no background normalisation")
    ex.add_argument("--ctf", metavar="STAR",
                    help="micrographs_ctf.star of `joint ctf`: append each micrograph's CTF columns to its rows of "
                         "particles.star, _rlnDetectorPixelSize multiplied by N (--bin) or B / S (--scale); a micrograph "
                         "with picks and no row there is an error")
    ex.add_argument("--ctf_correct", choices=("flip", "multiply"), metavar="{flip,multiply}",
                    help="multiply every particle in Fourier space by its micrograph's CTF sign (flip) or by the CTF itself "
                         "(multiply), from the row of --ctf STAR, before the crop to --scale S and the normalisation; needs "
                         "--ctf, an even --box and --scale (at least 16), excludes --bin N > 1.  The flat particles.star has "
                         "no column that says so: tell downstream tools that the data are flipped (relion_refine "
                         "--ctf_phase_flipped)")
    ex.check = _check_extract

    cf = cmds.add_parser("ctf", help="Power spectra of raw micrographs on the GPU and one defocus value each "
                                     "(replaces a CTFFIND / Gctf run before 2-D classification); with --astigmatism a 2-D fit "
                                     "of DefocusU, DefocusV and the angle, scored on the GPU (without it DefocusU = "
                                     "DefocusV, angle 0).")
    cf.add_argument("--dataset", "-d", required=True, help="Table (image_name, path) or directory of raw MRC micrographs.")
    cf.add_argument("--out", "-o", required=True,
                    help="Directory for {name}_psd.mrc, {name}_profile.txt and micrographs_ctf.star.")
    cf.add_argument("--apix", type=float, metavar="A", help="Angstrom per pixel (default: the MRC header's xlen / mx)")
    cf.add_argument("--kv", type=float, default=300, metavar="V", help="acceleration voltage in kV (default 300)")
    cf.add_argument("--cs", type=float, default=2.7, metavar="C", help="spherical aberration in mm (default 2.7)")
    cf.add_argument("--ac", type=float, default=0.07, metavar="Q", help="amplitude contrast in [0, 1) (default 0.07)")
    cf.add_argument("--tile", type=int, default=512, metavar="T",
                    help="tile side: a multiple of 16 in 16..1024 (default 512); tiles overlap by half, and a trailing "
                         "margin of fewer than T / 2 samples is not covered")
    cf.add_argument("--min_res", type=float, default=30, metavar="R", help="coarsest resolution fitted, Angstrom (default 30)")
    cf.add_argument("--max_res", type=float, metavar="R", help="finest resolution fitted, Angstrom (default max(4, 2.2 A))")
    cf.add_argument("--min_defocus", type=float, default=3000, metavar="D", help="lowest defocus searched, Angstrom (default 3000)")
    cf.add_argument("--max_defocus", type=float, default=50000, metavar="D", help="highest defocus searched, Angstrom (default 50000)")
    cf.add_argument("--astigmatism", action="store_true",
                    help="fit DefocusU, DefocusV and DefocusAngle to the 2-D spectrum (candidates around the 1-D fit scored on "
                         "the GPU); _rlnCtfFigureOfMerit is then the 2-D score")
    cf.add_argument("--max_astigmatism", type=float, metavar="A",
                    help="largest (DefocusU - DefocusV) / 2 searched, Angstrom (default 1000; needs --astigmatism, and "
                         "A + 550 < --min_defocus)")
    cf.check = _check_ctf

    al_help = ("Whole-frame motion correction of movies (MRC stacks) on the GPU: shifts estimated by iterated "
               "cross-correlation, frames shifted, summed and (--ftbin) Fourier-cropped (replaces a MotionCor2 / "
               "relion_motioncorr run before everything else).  Movies as the detector wrote them are corrected first "
               "(--gain, --dark, --defects, --hot_sigma); a fixed pattern left in the frames holds every estimated shift at "
               "zero.  With --patch PY,PX one smooth local field per movie (MotionCor2's form: a quadratic in the position, a "
               "cubic in time) is fitted to PY x PX patches after the whole-frame estimate, and every frame is warped by it "
               "before it is summed; {name}_local.txt reports it.  With --dose also a dose-weighted sum per movie, "
               "{name}_DW.mrc: give the plain sums (images.txt) to `joint ctf`, the weighted ones (images_DW.txt) to `joint "
               "eval` / `joint extract`, and pass those tables, not the directory, which then holds both.  Not covered: "
               "local motion finer than the one smooth field of --patch (per-particle polishing), EER input, TIFF that is "
               "tiled, uses a predictor or another compression than LZW, and references meant to be divided by.")
    al = cmds.add_parser("align", help=al_help, description=al_help)
    al.add_argument("--movies", "-d", required=True, metavar="T",
                    help="Table (image_name, path) or directory of MRC movie stacks (modes 0 / 1 / 2 / 6, at least 2 frames, "
                         "at most 16384 pixels a side; gain-corrected, or raw together with --gain / --dark / --defects / "
                         "--hot_sigma).  A movie may also be a multi-page TIFF (.tif / .tiff; a directory is searched for "
                         ".tiff, a table names either), as SerialEM and EPU write them: little-endian classic or BigTIFF, one "
                         "frame per directory, in strips, stored or LZW without a predictor, uint8 / int8 / uint16 / int16 / "
                         "float32; the strips are decoded on the GPU, and both kinds may stand in one table.  Row r of the "
                         "TIFF is row r of the frame; IMOD shows TIFF flipped in Y against MRC, so a gain reference that "
                         "IMOD converted to MRC needs --gain_flip ud.  --gain, --dark and --defects stay MRC and text.")
    al.add_argument("--out", "-o", required=True,
                    help="Directory for {name}.mrc (the aligned sum, float32), {name}_shifts.txt (frame, dx, dy in raw pixels, "
                         "mean zero) and images.txt.")
    al.add_argument("--ftbin", type=_ftbin, default=1, metavar="F",
                    help="Fourier-crop the sum by the factor F (any decimal or p/q in 1..64) in the same pass; default 1")
    al.add_argument("--align_size", type=int, default=1024, metavar="A",
                    help="the shifts are estimated on frames Fourier-cropped to about A pixels on their longer side "
                         "(64..16384, default 1024)")
    al.add_argument("--max_shift", type=int, default=16, metavar="R",
                    help="half width of the correlation window in pixels of the reduced frames (1..31, default 16)")
    al.add_argument("--iters", type=int, default=6, metavar="I",
                    help="iterations of the estimate at most (default 6; it stops when no shift moves by 0.01 reduced pixel)")
    al.add_argument("--no_align", action="store_true", help="sum (and crop) the frames as they are: all shifts zero")
    al.add_argument("--patch", metavar="PY,PX",
                    help="local motion correction: fit one smooth field to PY x PX patches (3..16 each; 5,5 is MotionCor2's "
                         "usual choice for a 4096^2 frame) and warp every frame by it, Catmull-Rom taps (0.88 of the signal at "
                         "half Nyquist for a half-pixel shift, none at Nyquist: sums that are cropped with --ftbin 2 lose "
                         "little).  Writes {name}_local.txt.  Needs at least 4 frames; not with --no_align")
    al.add_argument("--patch_shift", type=int, metavar="R",
                    help="half width of the patches' correlation window in pixels of the reduced frames (1..31, default 6; "
                         "2R+1 must fit a patch; needs --patch)")
    al.add_argument("--patch_iters", type=int, metavar="I",
                    help="iterations of the local estimate at most (default 4; it stops when no patch-centre value of the "
                         "field moves by 0.01 reduced pixel; needs --patch)")
    al.add_argument("--dose", type=float, metavar="E",
                    help="dose weighting (Grant & Grigorieff 2015, as in unblur): the exposure per frame in e/A^2 (> 0); writes "
                         "{name}_DW.mrc and images_DW.txt beside the plain sums, which stay what they are without it")
    al.add_argument("--pre_dose", type=float, metavar="P", help="exposure before the first frame, e/A^2 (>= 0, default 0; "
                                                                "needs --dose)")
    al.add_argument("--kv", type=float, metavar="V",
                    help="acceleration voltage in 200..300 kV (default 300; needs --dose).  The critical exposure is scaled by 1 at "
                         "300 kV and 0.8 at 200 kV; in between the scale is interpolated linearly, which is this program's choice")
    al.add_argument("--apix", type=float, metavar="A",
                    help="pixel size of the frames in Angstrom (default: the movie header's; a movie whose header states none is "
                         "refused; needs --dose)")
    al.add_argument("--gain", metavar="G",
                    help="gain reference, a single-image MRC (mode 0 / 1 / 2 / 6) of the frames' size: every sample is "
                         "MULTIPLIED by it (a reference meant to be divided by is not covered: invert it first).  Pixels "
                         "whose gain is not finite or not above 0 are replaced by the mean of the good pixels around them.  "
                         "Also writes {name}_defects.mrc, the map of the replaced pixels, as every flag of this group does")
    al.add_argument("--gain_rot", type=int, choices=(0, 1, 2, 3), metavar="{0,1,2,3}",
                    help="quarter turns of the gain reference, counter-clockwise as numpy.rot90 (default 0; needs --gain)")
    al.add_argument("--gain_flip", choices=("ud", "lr"),
                    help="flip the gain reference upside down or left to right, after the turn (needs --gain)")
    al.add_argument("--dark", metavar="D",
                    help="dark reference, a single-image MRC of the frames' size, subtracted from every sample before the gain")
    al.add_argument("--defects", metavar="FILE",
                    help="defect file in MotionCor2's layout: one rectangle `x y w h` per line (x the column, y the row of its "
                         "first sample; # starts a comment); its pixels are replaced like those of a bad gain")
    al.add_argument("--hot_sigma", type=float, metavar="S",
                    help="also replace hot pixels: those of the movie's plain sum more than S standard deviations above its "
                         "mean, found in up to 4 rounds (finite, > 0; 6 is recommended; off by default).  Works without "
                         "--gain, for gain-corrected movies that still have hot pixels")
    al.check = _check_align

    c2_help = ("Reference-free 2-D class averages of extracted particles on the GPU: a multi-reference alignment over "
               "in-plane angles and integer shifts that starts from one class and splits the largest classes until there "
               "are K (replaces a first relion_refine / EMAN2 2-D classification run when the aim is to judge the picks).  "
               "Reads the particles.star and the float32 stacks of `joint extract --scale 64` (or 128).  With --ctf_weight "
               "the averages are Wiener sums over the particles' CTFs.  Not covered: CTF weighting of the scores (the "
               "references are not CTF-modulated), per-particle defocus, soft (probabilistic) assignment, sub-pixel shifts, "
               "boxes that are not 64 or 128 pixels.")
    c2 = cmds.add_parser("class2d", help=c2_help, description=c2_help)
    c2.add_argument("--particles", "-p", required=True, metavar="STAR",
                    help="particles.star of `joint extract`; the {name}.mrcs stacks of _rlnImageName lie beside it")
    c2.add_argument("--classes", "-k", type=int, required=True, metavar="K", help="number of classes (1..the particle count)")
    c2.add_argument("--out", "-o", required=True,
                    help="Directory for classes.mrcs (K float32 averages), particles_class2d.star (the input rows plus "
                         "_rlnClassNumber, _rlnAnglePsi, _rlnOriginX, _rlnOriginY) and class2d.txt.")
    c2.add_argument("--angle_step", type=float, default=5.0, metavar="A",
                    help="in-plane angle step in degrees; 360 / A must be an integer in 1..720 (default 5)")
    c2.add_argument("--max_shift", type=int, default=3, metavar="R", help="shifts searched, +-R pixels (1..31, default 3)")
    c2.add_argument("--radius", type=int, metavar="P",
                    help="mask radius in pixels (default and at most S/2 - R - 2 for a box of S pixels)")
    c2.add_argument("--iters", type=int, default=8, metavar="I",
                    help="iterations per level at most (default 8, at least 2; a level stops when no assignment changes)")
    c2.add_argument("--ctf_weight", choices=("flip", "multiply"), metavar="MODE",
                    help="Wiener-weighted class averages for stacks of `joint extract --ctf STAR --ctf_correct MODE` (flip or "
                         "multiply: say which, the STAR file has no column for it); needs the CTF columns in particles.star")
    c2.add_argument("--wiener", type=float, metavar="T",
                    help="tau of the Wiener sums, 1 / SNR per particle and frequency: finite and > 0 (default 1.0; needs "
                         "--ctf_weight)")
    c2.check = _check_class2d
    return parser


def run_train(args, parser):
    from .train import DenoiserTrainer, resume_run
    if args["train_cmd"] == "start":
        if args["algorithm"] == "ssdn" and args.get("noise_value") is None:
            parser.error("SSDN requires --noise_value")
        cfg = cfg_mod.base()
        cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm(args["algorithm"])
        cfg[ConfigValue.NOISE_STYLE] = args["noise_style"]
        if args.get("noise_value") is not None:
            cfg[ConfigValue.NOISE_VALUE] = NoiseValue(args["noise_value"])
        for flag, key in (("lr", ConfigValue.LEARNING_RATE), ("bb", ConfigValue.BB), ("nms", ConfigValue.NMS)):
            if args.get(flag) is not None:
                cfg[key] = args[flag]
        if args["dn_only"]:
            trainer = DenoiserTrainer(cfg, mode="denoise", runs_dir=args["runs_dir"])
        else:
            trainer = DenoiserTrainer(cfg, mode="joint", alpha=args["alpha"], tau=args["tau"],
                                      runs_dir=args["runs_dir"])
    else:
        trainer = resume_run(args["run_dir"])
        cfg = trainer.cfg
        if args.get("alpha") is not None:
            trainer.alpha = args["alpha"]
        if args.get("tau") is not None:
            trainer.tau = args["tau"]

    for flag, setter in (("train_dataset", trainer.set_train_data), ("train_gt", trainer.set_train_gt_data),
                         ("train_label", trainer.set_train_label), ("validation_dataset", trainer.set_test_data),
                         ("validation_gt", trainer.set_test_gt_data), ("validation_label", trainer.set_test_label)):
        if args.get(flag) is not None:
            setter(args[flag])
    for flag, key in (("iterations", ConfigValue.ITERATIONS), ("num", ConfigValue.NUM_EVAL),
                      ("eval_interval", ConfigValue.EVAL_INTERVAL), ("checkpoint_interval", ConfigValue.SNAPSHOT_INTERVAL),
                      ("print_interval", ConfigValue.PRINT_INTERVAL), ("train_batch_size", ConfigValue.TRAIN_MINIBATCH_SIZE),
                      ("validation_batch_size", ConfigValue.TEST_MINIBATCH_SIZE), ("patch_size", ConfigValue.TRAIN_PATCH_SIZE),
                      ("alpha", ConfigValue.ALPHA), ("tau", ConfigValue.TAU)):
        if args.get(flag) is not None:
            cfg[key] = args[flag]
    trainer.train()
    return trainer


def run_eval(args):
    from .eval import DenoiserEvaluator
    evaluator = DenoiserEvaluator(args["model"], runs_dir=args["runs_dir"], contamination=args.get("contamination", False),
                                  bin=args.get("bin"), clip=args.get("clip"), flatten=args.get("flatten"),
                                  ftbin=args.get("ftbin"))
    for flag, key in (("batch_size", ConfigValue.TEST_MINIBATCH_SIZE), ("nms", ConfigValue.NMS),
                      ("num", ConfigValue.NUM_EVAL)):
        if args.get(flag) is not None:
            evaluator.cfg[key] = args[flag]
    evaluator.set_test_data(args["dataset"])
    evaluator.set_test_gt_data(args["gt_dataset"])
    evaluator.evaluate()
    return evaluator


def run_bin(args):
    from . import ingest
    return ingest.bin_dataset(args["dataset"], args.get("bin"), args["out"], labels=args.get("labels"), clip=args.get("clip"),
                              flatten=args.get("flatten"), ftbin=args.get("ftbin"))


def run_extract(args):
    import json
    from . import extract
    counts = extract.extract_dataset(args["dataset"], args["picks"], args["out"], args["box"], bin=args["bin"],
                                     picks_bin=args["picks_bin"], threshold=args.get("threshold"),
                                     bg_radius=args.get("bg_radius"), normalize=not args["no_norm"], invert=args["invert"],
                                     scale=args.get("scale"), ctf=args.get("ctf"), ctf_correct=args.get("ctf_correct"))
    summary = {"particles": sum(c["written"] for c in counts.values()), "micrographs": counts}
    if args.get("ctf_correct") is not None:
        summary["ctf_correct"] = args["ctf_correct"]
    print(json.dumps(summary))
    return counts


def run_ctf(args):
    import json
    from . import ctf
    res = ctf.ctf_dataset(args["dataset"], args["out"], apix=args.get("apix"), kv=args["kv"], cs=args["cs"], ac=args["ac"],
                          tile=args["tile"], min_res=args["min_res"], max_res=args.get("max_res"),
                          min_defocus=args["min_defocus"], max_defocus=args["max_defocus"],
                          **({"astigmatism": True, "max_astigmatism": args["max_astigmatism"] or ctf.MAX_ASTIGMATISM}
                             if args.get("astigmatism") else {}))
    print(json.dumps({"micrographs": res}))
    return res


def run_align(args):
    import json
    from . import align
    if args.get("patch") is not None:
        from .localmotion import parse_patch
        args = dict(args, patch=parse_patch(args["patch"]))
    res = align.align_dataset(args["movies"], args["out"], ftbin=args["ftbin"], align_size=args["align_size"],
                              max_shift=args["max_shift"], iters=args["iters"], no_align=args["no_align"],
                              **({} if args.get("dose") is None else
                                 {"dose": args["dose"], "pre_dose": args["pre_dose"] or 0.0, "kv": args["kv"] or 300.0,
                                  "apix": args.get("apix")}),
                              **{k: args[k] for k in ("gain", "dark", "defects", "hot_sigma") if args.get(k) is not None},
                              **({} if args.get("patch") is None else
                                 {"patch": tuple(args["patch"]), "patch_shift": args["patch_shift"],
                                  "patch_iters": args["patch_iters"]}),
                              **({} if args.get("gain") is None else
                                 {"gain_rot": args["gain_rot"] or 0, "gain_flip": args["gain_flip"]}))
    print(json.dumps({"movies": res}))
    return res


def run_class2d(args, parser):
    import json
    from . import class2d
    try:
        res = class2d.class2d_dataset(args["particles"], args["out"], args["classes"], angle_step=args["angle_step"],
                                      max_shift=args["max_shift"], radius=args.get("radius"), iters=args["iters"],
                                      ctf_weight=args.get("ctf_weight"), wiener=args.get("wiener"))
    except ValueError as e:                      # what only the stacks can tell: their side, their number
        parser.error(str(e))
    print(json.dumps(res))
    return res


def start(argv=None):
    import sys
    argv = list(sys.argv[1:] if argv is None else argv)
    if argv[:1] == ["--"]:      # `torch.distributed.run ... -m spr_pick_amd -- eval --num 8`: the separator keeps
        argv = argv[1:]         # the launcher's own parser from prefix-matching our flags (--num ~ --numa-binding)
    parser = build_parser()
    args = vars(parser.parse_args(argv))
    if args["command"] == "train":
        return run_train(args, parser)
    if args["command"] == "bin":
        return run_bin(args)
    if args["command"] == "extract":
        return run_extract(args)
    if args["command"] == "ctf":
        return run_ctf(args)
    if args["command"] == "align":
        return run_align(args)
    if args["command"] == "class2d":
        return run_class2d(args, parser)
    return run_eval(args)
