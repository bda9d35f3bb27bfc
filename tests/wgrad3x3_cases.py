"""The backward-weight calls tests/test_gpu_wgrad3x3.py and tests/test_wgrad3x3_route_cpu.py share: 3x3 layers the
streaming kernel (wgrad3x3_kernel, csrc/wgrad3x3.hip; SPRK_STAGE_WGRAD3X3) takes, and neighbours it refuses.

pad = (top, bottom, left, right).  SYM is what Conv2d passes, SHIFT what ShiftConv2d passes (the blind-spot layers pad two
rows on top and none below).  The shapes are the smallest at which plan_wgrad (256 CUs) still gives the plan the kernel is
written for -- one chunk of 48 input channels per workgroup, 27 k-tiles -- so the batch sizes are what the planner asks
for, not what the kernel needs: with few tiles it cuts the channels into shorter chunks on more workgroups."""
import ctypes

import conv_variant_cases as cv

WGRAD3X3, MFMA = 8, 5
SYM, SHIFT = (1, 1, 1, 1), (2, 0, 1, 1)

# name: N, C1, C2, Cout, H, W, pad, 64-pixel tiles per group on a 256-CU device
TAKEN = {
    # 48 -> 48 (NT = 3), 1 x 64 tiles: halo rows on both sides of every tile
    "48-48-64x64-N4-one-tile": (4, 48, 0, 48, 64, 64, SHIFT, 1),
    "48-48-64x64-N7-two-tiles": (7, 48, 0, 48, 64, 64, SHIFT, 2),
    "48-48-64x64-N11-short-last-group": (11, 48, 0, 48, 64, 64, SHIFT, 3),     # 704 tiles: 234 groups of 3 (they cross
    "48-48-64x64-N8-sym": (8, 48, 0, 48, 64, 64, SYM, 2),                      # images) and one of 2
    "48-48-128x64": (4, 48, 0, 48, 128, 64, SHIFT, 2),
    "48-48-32x32-N16": (16, 48, 0, 48, 32, 32, SHIFT, 1),                      # 2 x 32 tiles
    "48-48-32x32-N32-sym": (32, 48, 0, 48, 32, 32, SYM, 2),
    "48-48-16x16-N64": (64, 48, 0, 48, 16, 16, SHIFT, 1),                      # 4 x 16 tiles
    "48-48-16x16-N128-sym": (128, 48, 0, 48, 16, 16, SYM, 2),
    "48-40-ragged-block": (16, 48, 0, 40, 32, 32, SHIFT, 1),                   # zero-filled rows of gy
    "pads-0-2-0-2": (16, 48, 0, 48, 32, 32, (0, 2, 0, 2), 1),                  # the other same-size layouts
    "pads-1-1-2-0": (16, 48, 0, 48, 32, 32, (1, 1, 2, 0), 1),
    # blocks of 96 output channels (NT = 6)
    "96-96-32x32": (16, 96, 0, 96, 32, 32, SYM, 2),
    "96-96-16x16": (256, 96, 0, 96, 16, 16, SHIFT, 8),
    "48-96": (16, 48, 0, 96, 32, 32, SHIFT, 1),
    "96-48": (32, 96, 0, 48, 32, 32, SHIFT, 4),
    "144-96-two-sources": (64, 96, 48, 96, 32, 32, SHIFT, 13),
    "96-two-sources-of-48": (64, 48, 48, 96, 32, 32, SYM, 8),
    "96-90-ragged-block": (16, 96, 0, 90, 32, 32, SYM, 2),
}

# Smaller batches of the same layers, whose plan on a 256-CU device is NOT the kernel's (up to 256 tiles, or a tile count
# at which shorter chunks cost less): they keep conv_wgrad_mfma_kernel whatever the switch says, and are compared all the same
PLANNED_ELSEWHERE = {
    "48-48-64x64-N2": (2, 48, 0, 48, 64, 64, SHIFT),
    "48-48-64x64-N5": (5, 48, 0, 48, 64, 64, SHIFT),
    "48-48-64x64-N9": (9, 48, 0, 48, 64, 64, SHIFT),
    "48-48-32x32-N8": (8, 48, 0, 48, 32, 32, SHIFT),
    "48-48-16x16-N32": (32, 48, 0, 48, 16, 16, SHIFT),
}

# name: N, C1, C2, Cout, H, W, what
REFUSED = {
    "stride2": (32, 48, 0, 48, 32, 32, {"stride": 2}),
    "dilation2": (32, 48, 0, 48, 32, 32, {"dil": 2, "pad": (2, 2, 2, 2)}),
    "5x5": (32, 48, 0, 48, 32, 32, {"K": 5, "pad": (2, 2, 2, 2)}),
    "1x1": (32, 48, 0, 48, 32, 32, {"K": 1, "pad": (0, 0, 0, 0)}),
    "up1": (32, 48, 0, 48, 32, 32, {"up1": 1}),
    "60x44": (8, 48, 0, 48, 60, 44, {}),
    "unaligned-x": (32, 48, 0, 48, 32, 32, {"xoff": 1}),
    "Cin40": (32, 40, 0, 48, 32, 32, {}),
    "bf16": (32, 48, 0, 48, 32, 32, {"dtype": "bf16"}),
    "storage16": (32, 48, 0, 48, 32, 32, {"dtype": "bf16", "storage16": 1}),
}


def geom_of(N, C1, C2, Cout, H, W, pad=SYM, K=3, stride=1, dil=1, up1=0, dtype=0):
    from spr_pick_amd import _lib
    Ho = cv.out_size(H, K, stride, dil, pad[0], pad[1])
    Wo = cv.out_size(W, K, stride, dil, pad[2], pad[3])
    return _lib.ConvGeom(N, C1, C2, H, W, up1, Cout, Ho, Wo, K, K, stride, dil, pad[0], pad[2], int(dtype))


def refused_geom(case):
    from spr_pick_amd import _lib
    N, C1, C2, Cout, H, W, what = REFUSED[case]
    dt = (_lib.DT_BF16 if what.get("dtype") else 0) | ((_lib.DT_X16 | _lib.DT_Y16) if what.get("storage16") else 0)
    return geom_of(N, C1, C2, Cout, H, W, pad=what.get("pad", SHIFT), K=what.get("K", 3), stride=what.get("stride", 1),
                   dil=what.get("dil", 1), up1=what.get("up1", 0), dtype=dt)


def query(g, xoff=0, has_x2=False):
    """sprk_conv2d_variant(2, ...) for tensors at 16-byte aligned addresses (x: xoff floats off) -> the record as a dict"""
    return cv.as_dict(2, cv._query(2, g, cv.A0 + 4 * xoff, cv.A0 if has_x2 else None, cv.A0))


def switch(on):
    from spr_pick_amd import _lib
    _lib.lib().sprk_wgrad3x3_enable(int(on))


def launches():
    from spr_pick_amd import _lib
    return _lib.lib().sprk_wgrad3x3_launch_count()


def last_record():
    from spr_pick_amd import _lib
    out = (ctypes.c_int32 * 24)()
    assert _lib.lib().sprk_conv2d_last_variant(2, out) == 0
    return cv.as_dict(2, list(out))
