"""CPU: the contamination mask's contract — the NumPy model against the reference's own index sets
(tests/golden/contamination.npz, written by tests/make_contamination_golden.py), the threshold margins those
fixtures rely on, the operator's fake shape and the --contamination flag."""
import numpy as np
import pytest
import torch

import contam_model as M
from conftest import golden


def _fixtures():
    z = golden("contamination.npz")
    return [(z["img%d" % k], z["set%d" % k]) for k in range(3)]


def test_model_equals_reference_sets():
    for img, want in _fixtures():
        assert np.array_equal(M.contam_set_literal(img), want)
        assert np.array_equal(np.flatnonzero(M.contam_set_bitmap(img)), want)
        H, W = img.shape
        Hb, Wb = H - 6, W - 6
        # the clip and wrap paths are pinned: row 0, the virtual row Hb, the wrapped column and the last index
        assert (want < Wb).any() and ((want >= Hb * Wb) & (want < (Hb + 1) * Wb)).any()
        assert (want == (Hb + 1) * Wb).any() and ((want % Wb == 0) & (want >= Wb)).any()


def test_fixture_thresholds_keep_a_margin_from_integers():
    """The device std sums the histogram instead of NumPy's pairwise sum (a few ulp apart): harmless unless a
    threshold lies next to an integer, the value a blurred uint8 pixel can take."""
    for img, _ in _fixtures():
        for t in M.thresholds(M.normalise(img)):
            assert abs(t - round(t)) >= 1e-6, t


def test_score_frame_mapping():
    img, want = _fixtures()[0]
    H, W = img.shape
    m = M.score_mask(M.contam_set_bitmap(img), H, W)
    Wb = W - 6
    assert m.sum() == len(want)
    assert m[want // Wb + 3, want % Wb + 3].all()
    # nothing outside rows 3..H-2 and columns 3..W-4; row H-2 only at column 3 (the last index)
    assert not m[:3].any() and not m[H - 1].any() and not m[:, :3].any() and not m[:, W - 3:].any()
    assert not m[H - 2, 4:].any()


def test_model_forms_agree_on_random_maps():
    rng = np.random.default_rng(5)
    for _ in range(12):
        H, W = (int(v) for v in rng.integers(7, 48, 2))
        img = rng.normal(size=(H, W)).astype(np.float32)
        img[rng.integers(0, H, 3), rng.integers(0, W, 3)] += 40
        for kw in ({}, dict(r=4), dict(crop=2, ksize=3, r=7)):
            assert np.array_equal(M.contam_set_literal(img, **kw), np.flatnonzero(M.contam_set_bitmap(img, **kw)))


def test_contam_mask_fake_shape():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from spr_pick_amd import torch_ops
    assert "contam_mask" in torch_ops.registered()
    with FakeTensorMode():
        img = torch.empty(130, 97, device="cuda")
        stats = torch.empty(8, dtype=torch.float64, device="cuda")
        m = torch.ops.sprk.contam_mask(img, 3, 5, 1.5, 2.0, 15, None, stats)
        assert tuple(m.shape) == (130, 97) and m.dtype == torch.uint8


def test_contamination_flag_parses_default_off():
    from spr_pick_amd import cli
    p = cli.build_parser()
    assert vars(p.parse_args(["eval", "-m", "x.wt", "-d", "t.txt"]))["contamination"] is False
    assert vars(p.parse_args(["eval", "-m", "x.wt", "-d", "t.txt", "--contamination"]))["contamination"] is True


def test_contamination_is_not_in_cfg():
    from spr_pick_amd.params import ConfigValue
    assert not [v for v in ConfigValue if "contam" in v.name.lower() or "contam" in str(v.value).lower()]


def test_abi_declares_contamination_entry_points():
    from spr_pick_amd import _lib
    assert _lib.ABI_VERSION == 430
    assert {"sprk_contam_ws_bytes", "sprk_contam_mask"} <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert L.sprk_contam_ws_bytes(0, 10) == 0 and L.sprk_contam_ws_bytes(64, 64) >= 64 * 64
    assert L.sprk_contam_mask(None, 8, 8, 3, 5, 1.5, 2.0, 15, None, None, None, None, 0, None) == -1
    assert b"null" in L.sprk_last_error()
