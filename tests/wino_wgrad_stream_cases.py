"""The backward-weight calls tests/test_gpu_wino_wgrad_stream.py makes: 3x3 same-size layers that take the Winograd
backward-weight stage (wino_wgrad_eligible, csrc/wino.hip), each run on wino_wgrad_stream_kernel and on wino_wgrad_kernel.

A region is 4 x 16 output pixels, and the stage wants 2048 of them (8192 when a source has a tail of <= 16 channels), so
the planes can be tiny and the batch makes the count.  A launch has `parts` workgroups (256 / the source's groups of 48
channels on a 256-CU device); workgroup j walks regions slot(j), slot(j) + parts, ...: floor or ceil of regions / parts of
them.  Per case below: the workgroup lengths, and their residues mod 2 (the kernel's two LDS stages: the last region of a
workgroup falls in either) and mod 3 (for a version with three stages).

  name                      regions  launches (MT x groups, parts)      lengths     mod 2   mod 3   planes: region types
  48-96-4x16-N2048          2048     3x1 256                            8           0       2       one region: first-and-last both ways
  48-96-4x16-N2049          2049     3x1 256                            8, 9        0, 1    2, 0    (one workgroup of 9)
  96-96-8x32-N512           2048     3x2 128                            16          0       1       first / last only
  144-81-4x48-N683          2049     3x3 85                             24, 25      0, 1    0, 1    one region row; cx, cy carry; XCD order off
  96+48-96-12x48-N228       2052     3x2 128 | 3x1 256                  16, 17 | 8, 9  both  1, 2 | 2, 0   inner regions both ways; cx, cy carry
  96-96-16x16-N525          2100     3x2 128                            16, 17      0, 1    1, 2    one region column
  48-96-4x48-N700           2100     3x1 256                            8, 9        0, 1    2, 0    cx, cy carry; lengths differ in one launch
  49-96-4x16-N8192          8192     3x1 256 | 1x1 256                  32          0       2       tail of one channel
  96+16-90-8x32-N2048       8192     3x2 128 | 1x16 256                 64 | 32     0       1 | 2   second source only a tail; cut output half
  48+5-96-4x48-N2731        8193     3x1 256 | 1x5 256                  32, 33      0, 1    2, 0    second source only a tail; cx, cy carry

(padT, padL) takes each of (2, 1), (0, 1), (1, 0), (2, 2), (4, 4), (0, 3): both parities of padL, so both positions of the
raw tile in its LDS stage."""

WINO = 3          # SPRK_STAGE_WINOGRAD (include/sprk.h)

# name: N, C1, C2, Cout, H, W, (padT, padL), does a workgroup's region cursor carry in x / in y (sprk_conv2d_variant's cx, cy)
CASES = {
    "48-96-4x16-N2048": (2048, 48, 0, 96, 4, 16, (2, 1), False),
    "48-96-4x16-N2049": (2049, 48, 0, 96, 4, 16, (1, 0), False),
    "96-96-8x32-N512": (512, 96, 0, 96, 8, 32, (2, 2), False),
    "144-81-4x48-N683": (683, 144, 0, 81, 4, 48, (2, 1), True),
    "96+48-96-12x48-N228": (228, 96, 48, 96, 12, 48, (4, 4), True),
    "96-96-16x16-N525": (525, 96, 0, 96, 16, 16, (0, 3), False),
    "48-96-4x48-N700": (700, 48, 0, 96, 4, 48, (0, 1), True),
    "49-96-4x16-N8192": (8192, 49, 0, 96, 4, 16, (2, 1), False),
    "96+16-90-8x32-N2048": (2048, 96, 16, 90, 8, 32, (0, 1), False),
    "48+5-96-4x48-N2731": (2731, 48, 5, 96, 4, 48, (1, 0), True),
}


def geom_of(N, C1, C2, Cout, H, W, pad):
    """ConvGeom of the 3x3 stride-1 same-size layer with padT rows above and padL columns left of the image"""
    from spr_pick_amd import _lib
    return _lib.ConvGeom(N, C1, C2, H, W, 0, Cout, H, W, 3, 3, 1, 1, pad[0], pad[1], 0)


def switch(on):
    from spr_pick_amd import _lib
    _lib.lib().sprk_wino_wgrad_stream_enable(int(on))


def launches():
    """-> (calls that ran on the streaming kernel, calls of the Winograd stage)"""
    from spr_pick_amd import _lib
    L = _lib.lib()
    return L.sprk_wino_wgrad_stream_launch_count(), L.sprk_wino_launch_count()
