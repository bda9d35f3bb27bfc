"""GPU: the contamination mask (csrc/contam.hip) bit for bit against the reference's own index sets and
the NumPy model (tests/contam_model.py), the find_contamination / non_maximum_suppression drop-ins against the oracle,
and contamination-aware picking in the evaluation output path (flag off: today's files; flag on: masked picks)."""
import os

import numpy as np
import pytest
import torch

import contam_model as M
from conftest import golden

pytestmark = pytest.mark.gpu


def _device_mask(img, **kw):
    from spr_pick_amd.algorithms import contamination_mask
    m, st = contamination_mask(torch.from_numpy(img).cuda(), stats=True, **kw)
    return m.cpu().numpy(), st.cpu().numpy()


def _blobs(H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.ogrid[0:H, 0:W]
    img = rng.normal(size=(H, W)).astype(np.float32)
    for cy, cx, r, a in ((H // 3, W // 4, 60, -6), (H - 10, W - 5, 40, 7), (5, W // 2, 30, -7), (H // 2, 0, 25, 6),
                         (H - 1, 0, 20, -6), (2 * H // 3, W - 1, 35, -7)):
        img += np.float32(a) * (((yy - cy) ** 2 + (xx - cx) ** 2) <= r * r)
    return img


def _grid_two_level(H, W):
    """8x8 dark squares every 15 px on a bright background: the dark level is 28 % of the map, under the ~31 % at
    which mean - 1.5 std would reach it, so the squares' cores (7 % of the pixels) are seeds and every pixel is masked.
    Seeds cannot be a majority: by Cantelli's inequality at most ~31 % + 20 % of a map lie beyond the two thresholds."""
    yy, xx = np.ogrid[0:H, 0:W]
    return np.where(((yy % 15) < 8) & ((xx % 15) < 8), 0.0, 1.0).astype(np.float32)


def test_device_mask_equals_reference_fixtures():
    from spr_pick_amd.algorithms import _contam
    z = golden("contamination.npz")
    for k in range(3):
        img, want = z["img%d" % k], z["set%d" % k]
        H, W = img.shape
        mask, bitmap, st = _contam(torch.from_numpy(img).cuda(), True, {})
        bits = np.flatnonzero(bitmap.cpu().numpy())
        assert np.array_equal(bits, want), k
        assert np.array_equal(mask.cpu().numpy().astype(bool), M.score_mask(np.isin(np.arange(bitmap.numel()), want), H, W))
        st = st.cpu().numpy()
        u = M.normalise(img)
        lo, hi = M.thresholds(u)
        assert st[0] == img.min() and st[1] == img.max()
        assert st[2] == np.mean(u) and abs(st[3] - np.std(u)) <= 1e-12 * max(1.0, np.std(u))
        assert abs(st[4] - lo) <= 1e-9 and abs(st[5] - hi) <= 1e-9
        assert st[6] == M.seeds(img).sum() and st[7] == len(want)


def test_device_mask_equals_model():
    cases = [("noise+blobs 1000x1100", _blobs(1000, 1100, 1)), ("noise+blobs 4096x4096", _blobs(4096, 4096, 2)),
             ("constant", np.full((300, 257), 0.25, np.float32)), ("two-level 1024x1024", _grid_two_level(1024, 1024))]
    nonfinite = _blobs(200, 230, 3)
    nonfinite[7, 9], nonfinite[100, 3], nonfinite[150, 200] = np.nan, np.inf, -np.inf
    cases.append(("non-finite", nonfinite))
    for name, img in cases:
        got, st = _device_mask(img)
        want = M.contam_mask(img)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        if name == "constant":
            assert not got.any() and st[6] == 0
        if name.startswith("two-level"):
            assert got[3:-3, 3:-3].all() and st[6] > 0.05 * img.size
        print("%s: %.4f %% masked, %d seeds" % (name, 100.0 * got.mean(), int(st[6])))
    allnan = np.full((40, 50), np.nan, np.float32)
    got, st = _device_mask(allnan)
    assert not got.any() and np.isnan(st[0]) and np.isnan(st[1])


def _time_ms(img, reps=20):
    from spr_pick_amd.algorithms import contamination_mask
    t = torch.from_numpy(img).cuda()
    for _ in range(3):
        contamination_mask(t)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        contamination_mask(t)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def test_mask_time_is_reported():
    """Printed, not asserted (DESIGN §4 records the measured values)."""
    for name, img in (("noise+blobs 1024^2", _blobs(1024, 1024, 4)), ("noise+blobs 4096^2", _blobs(4096, 4096, 5)),
                      ("two-level (dense seeds) 4096^2", _grid_two_level(4096, 4096))):
        print("contamination mask %s: %.3f ms" % (name, _time_ms(img)))


def _peaks(H, W, seed, centres=None):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    s = np.zeros((H, W), np.float32)
    pts = centres if centres is not None else list(zip(rng.integers(0, H, 60), rng.integers(0, W, 60)))
    for cy, cx in pts:
        s = np.maximum(s, np.float32(rng.uniform(0.1, 1.0)) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 40.0))
    return np.round(s * 4096) / np.float32(4096)


def test_find_contamination_and_nms_dropins():
    from oracle import nms as oracle_nms
    from spr_pick_amd.algorithms import find_contamination, non_maximum_suppression
    z = golden("contamination.npz")
    img = z["img0"]
    got = find_contamination(img)
    assert got == set(M.contam_set_literal(img).tolist()) == set(z["set0"].tolist())
    score = _peaks(*img.shape, seed=11)
    s, c = non_maximum_suppression(score, 18, set(got), 0.02)
    s2, c2 = oracle_nms.nms_literal(score, 18, 0.02, contam=set(got))
    assert len(s) > 5 and np.array_equal(s, s2) and np.array_equal(c, c2)


def _eval_case(tmp_path, contamination):
    from spr_pick_amd import cfg as cfg_mod
    from spr_pick_amd.datasets import DetectionDataset as D
    from spr_pick_amd.params import ConfigValue, NoiseAlgorithm, NoiseValue, PipelineOutput as P
    from spr_pick_amd.train import DenoiserTrainer
    c = cfg_mod.base()
    c[ConfigValue.ALGORITHM] = NoiseAlgorithm.SELFSUPERVISED_DENOISING
    c[ConfigValue.NOISE_STYLE] = "gaussian"
    c[ConfigValue.NOISE_VALUE] = NoiseValue.UNKNOWN_VARIABLE
    c[ConfigValue.NMS] = 18
    t = DenoiserTrainer(c, "joint", runs_dir=str(tmp_path), device="cuda:0", contamination=contamination)
    t.init_state()
    H, W, Hp, Wp = 300, 280, 320, 288                 # un-padded frame inside a padded batch tensor
    rng = np.random.default_rng(9)
    den = np.zeros((Hp, Wp), np.float32)
    den[:H, :W] = rng.normal(size=(H, W)).astype(np.float32)
    yy, xx = np.ogrid[0:H, 0:W]
    dark = ((yy - 150) ** 2 + (xx - 140) ** 2) <= 45 ** 2   # planted dark disk in the middle
    den[:H, :W][dark] -= 8.0
    inside = [(150, 140), (130, 160), (170, 120)]
    outside = [(60, 60), (60, 220), (240, 60), (240, 220), (150, 240), (45, 140)]
    sc = np.zeros((Hp, Wp), np.float32)
    sc[:H, :W] = _peaks(H, W, seed=3, centres=inside + outside)
    sc[:H, :W][150, 140] = 2.0                         # the strongest peak sits in the contamination
    meta = {D.Metadata.NAME: ["micA"], D.Metadata.IMAGE_SHAPE: torch.tensor([[1, H, W]]),
            D.Metadata.INDEXES: torch.tensor([0])}
    outputs = {P.INPUTS: [torch.from_numpy(den)[None, None].cuda(), None, None, None, meta],
               P.IMG_DENOISED: torch.from_numpy(den)[None, None].cuda(),
               P.DETECT: torch.from_numpy(sc)[None, None].cuda()}
    out = str(tmp_path / ("on" if contamination else "off"))
    t._save_image_outputs(outputs, out, "{name}_{desc}.png", 0, "{name}_{desc}.txt")
    t.writer.drain()
    return out, den[:H, :W], sc[:H, :W], dark


def test_eval_path_with_and_without_contamination(tmp_path):
    from oracle import nms as oracle_nms
    from spr_pick_amd import picks
    from spr_pick_amd.algorithms import nms_device
    out, den, score, dark = _eval_case(tmp_path, False)
    files = sorted(os.listdir(out))
    assert "micA_scores.txt" in files and not any("contam" in f for f in files)
    s, c = nms_device(torch.from_numpy(np.ascontiguousarray(score)).cuda(), 18, 0.02)
    ref = str(tmp_path / "ref_scores.txt")
    picks.write_scores(ref, "micA", s.cpu().numpy(), c.cpu().numpy(), score.shape)
    assert open(os.path.join(out, "micA_scores.txt"), "rb").read() == open(ref, "rb").read()
    _, xy_off, _ = picks.read_scores(ref)
    assert any(dark[y, x] for y, x in xy_off)                # the contaminated peak is picked without the flag

    out, den, score, dark = _eval_case(tmp_path, True)
    assert "micA_contam.png" in os.listdir(out)
    mask = M.contam_mask(den)
    assert mask[dark].all()
    _, xy, _ = picks.read_scores(os.path.join(out, "micA_scores.txt"))
    assert len(xy) >= 4 and not any(mask[y, x] for y, x in xy)   # x_coord = array row (picks.py)
    s2, c2 = oracle_nms.nms_literal(np.where(mask, -np.inf, score).astype(np.float32), 18, 0.02)
    picks.write_scores(ref, "micA", s2, c2, score.shape)             # the 30-px filter and the file format
    assert open(os.path.join(out, "micA_scores.txt"), "rb").read() == open(ref, "rb").read()
    from PIL import Image
    png = np.array(Image.open(os.path.join(out, "micA_contam.png")))
    assert np.array_equal(png, mask.T.astype(np.uint8) * 255)      # file orientation, like every output PNG
