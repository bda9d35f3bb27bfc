"""Drop-ins for ``spr_pick.utils.algorithms.non_maximum_suppression`` (utils/algorithms.py:59-103) and
``find_contamination`` (utils/algorithms.py:24-57) running on the GPU (libsprk.so: sprk_nms2d, sprk_contam_mask)."""
import numpy as np
import torch

from . import _lib
from . import torch_ops  # noqa: F401  (registers torch.ops.sprk.nms2d / contam_mask)

ROUNDS_PER_CALL = 12


def _max_picks(H, W, r):
    if r <= 0:
        return H * W
    # picks are pairwise more than r apart: disks of radius r/2 around them are disjoint
    bound = int((H + r) * (W + r) / (0.7853 * r * r)) + 16
    return max(1, min(H * W, bound))


def nms_device(score, r, threshold, max_out=None):
    """score: [H,W] float32 CUDA tensor.  Returns (scores[n], coords[n,2]) CUDA tensors, picks in
    descending-score order, coords[:,0] = x (column), coords[:,1] = y (row)."""
    L = _lib.lib()
    if not score.is_cuda or score.dtype != torch.float32 or score.dim() != 2:
        raise _lib.SprkError("nms_device expects a 2-D float32 CUDA tensor")
    score = score.contiguous()
    H, W = score.shape
    thr = float(max(threshold, -3.0e38))
    cap = int(max_out) if max_out else _max_picks(H, W, int(r))
    while True:
        out_s = torch.empty(cap, dtype=torch.float32, device=score.device)
        out_xy = torch.empty((cap, 2), dtype=torch.int32, device=score.device)
        cnt = torch.zeros(2, dtype=torch.int32, device=score.device)
        nb = L.sprk_nms2d_ws_bytes(H, W, cap)
        ws = torch.empty(nb, dtype=torch.uint8, device=score.device)
        resume = 0
        while True:
            torch.ops.sprk.nms2d(score, int(r), thr, out_s, out_xy, cnt, ROUNDS_PER_CALL, resume, ws)
            n, undecided = cnt.tolist()
            if undecided == 0:
                break
            resume = 1
        if n <= cap:
            return out_s[:n], out_xy[:n]
        cap = n  # list overflowed (only possible with a caller-supplied max_out): redo with room


UPDATE_EMPTY_CONTAM = False   # see non_maximum_suppression


def _disk_offsets(r):
    ii, jj = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1))
    keep = (ii ** 2 + jj ** 2) <= r * r
    return ii[keep], jj[keep]


def non_maximum_suppression(x, r, contam=None, threshold=-np.inf):
    """Same signature and return convention as the reference: ``x`` is an [H,W] score map (NumPy
    array or tensor), returns (scores float32[n], coords int32[n,2]) NumPy arrays.

    ``contam`` is the reference's suppressed-index set (utils/algorithms.py:77): flat indices already in it are never
    emitted and suppress nothing, and the reference ADDS every index its picks suppress (clip-to-H/W quirk included).
    Both are reproduced: the pre-suppressed pixels are taken out of the device score map (a score of -inf is never
    reached before the threshold stops the walk, which is exactly "skipped"), and the picks' disks are added to the
    set afterwards.  The reference's only caller passes a fresh ``set()`` and drops it (train.py:564); adding
    ~1000 indices per pick to a Python set costs seconds per micrograph, so an EMPTY set is left untouched unless
    ``algorithms.UPDATE_EMPTY_CONTAM`` is set."""
    if isinstance(x, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    else:
        t = x.detach().to(device="cuda", dtype=torch.float32)
    H, W = t.shape
    seeded = contam is not None and len(contam) > 0
    if seeded:
        idx = np.fromiter((i for i in contam if 0 <= i < H * W), dtype=np.int64)
        t = t.clone()
        t.view(-1)[torch.from_numpy(idx).to(t.device)] = float("-inf")
    s, c = nms_device(t, r, threshold)
    s, c = s.cpu().numpy(), c.cpu().numpy()
    if contam is not None and (seeded or UPDATE_EMPTY_CONTAM) and len(s):
        di, dj = _disk_offsets(int(r))
        yc = np.clip(c[:, 1:2].astype(np.int64) + di[None, :], 0, H)      # clip bounds H / W as in the reference
        xc = np.clip(c[:, 0:1].astype(np.int64) + dj[None, :], 0, W)
        contam.update(np.unique(yc * W + xc).tolist())
    return s, c


# find_contamination's constants (utils/algorithms.py:28-37): crop of the blurred region, blur size, the two seed
# thresholds in standard deviations, disk radius
CONTAM_PARAMS = dict(crop=3, ksize=5, k_low=1.5, k_high=2.0, radius=15)
CONTAM_STATS = ("min", "max", "mean", "std", "thr_low", "thr_high", "seeds", "masked")


def _contam(img, set_bitmap, params):
    p = dict(CONTAM_PARAMS)
    unknown = set(params) - set(p)
    if unknown:
        raise TypeError("unknown contamination parameter(s): %s" % ", ".join(sorted(unknown)))
    p.update(params)
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).cuda()
    if not img.is_cuda or img.dtype != torch.float32:
        raise _lib.SprkError("contamination_mask expects a float32 CUDA tensor (or a NumPy array)")
    while img.dim() > 2 and img.shape[0] == 1:
        img = img[0]
    if img.dim() != 2:
        raise _lib.SprkError("contamination_mask expects a 2-D map, got shape %s" % (tuple(img.shape),))
    img = img.contiguous()
    H, W = img.shape
    if set_bitmap is not None:
        Hb, Wb = H - 2 * p["crop"], W - 2 * p["crop"]
        set_bitmap = torch.empty((Hb + 1) * Wb + 1, dtype=torch.uint8, device=img.device)
    stats = torch.empty(len(CONTAM_STATS), dtype=torch.float64, device=img.device)
    mask = torch.ops.sprk.contam_mask(img, p["crop"], p["ksize"], p["k_low"], p["k_high"], p["radius"], set_bitmap, stats)
    return mask, set_bitmap, stats


def contamination_mask(img, stats=False, **params):
    """Contamination mask of a denoised micrograph ``img`` ([H,W] float32, CUDA tensor or NumPy array) in the frame of
    the score map that shares img's frame: bool CUDA tensor [H,W], True where the reference's find_contamination
    (run on img) would suppress picks, the index set placed as DESIGN §4 states.  ``params`` override CONTAM_PARAMS.
    No host synchronisation.  stats=True also returns a float64 CUDA tensor of CONTAM_STATS."""
    mask, _, st = _contam(img, None, params)
    mask = mask.view(torch.bool)
    return (mask, st) if stats else mask


def find_contamination(out_img, **params):
    """Drop-in for the reference's find_contamination(out_img): the set of flat indices it returns, in its own frame
    (row-major over the blurred crop, Wb = W - 6 wide, clip bounds Hb / Wb; largest index (Hb+1)*Wb).  Handing this
    set to non_maximum_suppression reproduces the reference's own (frame-skewed) use; the evaluation path uses
    contamination_mask instead."""
    _, bitmap, _ = _contam(out_img, True, params)
    return set(torch.nonzero(bitmap).view(-1).cpu().tolist())
