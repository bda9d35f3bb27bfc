"""The backward-weight of the heads' wide 1x1 layers on the streaming kernel (wgrad1x1_kernel, csrc/wgrad1x1.hip;
SPRK_STAGE_WGRAD1X1).

fp32 1x1 calls in the row form whose plan has 3 k-tiles per wave and blocks of 6 output tiles, over planes whose
64-pixel tiles are 64 consecutive floats, leave conv_wgrad_mfma_kernel<3, 6, 2, 1> for a kernel that issues the same
chain of v_mfma_f32_16x16x4_f32 per element of the partial slabs, on the same split into groups, channel chunks and
output blocks, followed by the same reduction.  So every comparison is bit for bit (int32 views: -0 and +0 are told
apart) between the call with the stage on (sprk_wgrad1x1_enable(1): sprk_wgrad1x1_launch_count advances by exactly 1,
the last variant says stage 7) and the same call with it off (counter still, stage 5), finished in the call and
deferred to reduce_pending; the first case of each family is also held against the fp64 product at
tests/test_gpu_ops.py's gradient budget (5e-5 of the largest element).

Shapes: the smallest the planner still gives that plan on a 256-CU device (sprk_conv2d_variant, which needs no GPU:
the record's tile count is asserted, not restated).  The kernel walks a group's tiles through two LDS stages with the
DMA two tiles ahead and one barrier per tile: 1 tile per group, exactly 2 (each stage is filled once), 3 (the first
re-use of a stage), 4 and 6, a last group that is shorter than the others, groups that cross an image (4 tiles per
16 x 16 plane against 3 per group) and that do not (64 per 64 x 64 plane); one, two and eight workgroups per group
(192 -> 384: one channel chunk; 384 -> 96; 384 -> 384); output blocks whose last tiles are zero-filled (90 and 200
channels); chunks shorter than 192 rows (320 input channels: two chunks of 160, the x rows behind them zero-filled);
tiles of sixteen rows of 4, eight rows of 8, two rows of 32, and two tiles side by side in a row of 128."""
import ctypes

import pytest
import torch

import conv_variant_cases as cv
from test_gpu_ops import close, dev

pytestmark = pytest.mark.gpu

GRAD_REL = 5e-5
WGRAD1X1, MFMA = 7, 5


def _lib_():
    from spr_pick_amd import _lib
    return _lib.lib()


def _record():
    out = (ctypes.c_int32 * 24)()
    assert _lib_().sprk_conv2d_last_variant(2, out) == 0
    return cv.as_dict(2, list(out))


def _bits_equal(a, b, what):
    assert not bool(torch.isnan(a).any()), "%s: elements left unwritten (NaN guard)" % what
    assert a.shape == b.shape
    same = torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    assert same, "%s: %d elements differ between the two kernels (max |d| %.3e)" % (
        what, int((a != b).sum()), float((a - b).abs().max()))


def _inputs(N, Cin, Cout, H, W, seed, Ho=None, Wo=None):
    """x and gy with zeros of both signs and two rows whose products are all +-0: input channel 0 is -0 everywhere (every
    product of its row is a signed zero, and the sum of a row of them must keep its sign rules), output channel 1 of gy +0."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    gy = torch.randn(N, Cout, Ho or H, Wo or W, generator=g)
    for t in (x, gy):
        t[torch.rand(t.shape, generator=g) < 0.02] = 0.0
        t[torch.rand(t.shape, generator=g) < 0.02] = -0.0
    x[:, 0] = -0.0
    gy[:, 1] = 0.0
    return x, gy


def _on_off(x, gy, Cin_w, xoff=0, goff=0, dtype=0, pad=(0, 0, 0, 0), stride=1, x2=None):
    """The raw backward-weight call, finished and deferred, with the stage on and off
    -> {on: (gw finished, gw deferred, launches of the stage, record of the last call)} or the SprkError both raise"""
    from spr_pick_amd import _lib, ops
    L, S, d = _lib_(), torch.ops.sprk, dev()
    xd, gyd = cv.float_offset(x, xoff, d), cv.float_offset(gy, goff, d)
    x2d = None if x2 is None else x2.to(d)
    w = torch.empty(gy.shape[1], Cin_w, 1, 1, device=d)
    geom = ops.make_geom(xd, x2d, w, False, stride, 1, pad, dtype=dtype)
    assert (geom.Hout, geom.Wout) == tuple(gy.shape[2:])
    res = {}
    try:
        for on in (1, 0):
            L.sprk_wgrad1x1_enable(on)
            n0 = L.sprk_wgrad1x1_launch_count()
            got = []
            for defer in (False, True):
                gw = torch.full_like(w, float("nan"))
                try:
                    S.conv2d_bwd_weight(xd, x2d, gyd, ops.geom_list(geom), gw, defer)
                except _lib.SprkError as e:
                    got.append(str(e))
                    continue
                if defer:
                    S.reduce_pending(gw)
                torch.cuda.synchronize()
                got.append(gw)
            res[on] = (got[0], got[1], L.sprk_wgrad1x1_launch_count() - n0, _record())
    finally:
        L.sprk_wgrad1x1_enable(1)
    return res


# name: N, Cin, Cout, H, W, 64-pixel tiles per group on a 256-CU device, the last group is shorter
TAKEN = {
    "384-384-one-tile": (8, 384, 384, 16, 16, 1, False),
    "384-384-two-tiles": (16, 384, 384, 16, 16, 2, False),
    "384-384-three-tiles": (24, 384, 384, 16, 16, 3, False),
    "384-384-four-tiles": (32, 384, 384, 16, 16, 4, False),
    "384-384-six-tiles": (48, 384, 384, 16, 16, 6, False),
    "384-384-short-last-group": (23, 384, 384, 16, 16, 3, True),     # 92 tiles: 30 groups of 3 and one of 2
    "384-384-32x32": (8, 384, 384, 32, 32, 4, False),
    "384-384-64x64": (2, 384, 384, 64, 64, 4, False),
    "384-384-2x32": (128, 384, 384, 2, 32, 4, False),                # a tile is two rows
    "384-96": (64, 384, 96, 16, 16, 2, False),
    "192-384-one-chunk": (32, 192, 384, 16, 16, 2, False),
    "384-90-ragged-block": (64, 384, 90, 16, 16, 2, False),
    "384-200-three-blocks": (21, 384, 200, 16, 16, 2, False),
    "384-384-16x4": (64, 384, 384, 16, 4, 2, False),                 # a tile is sixteen rows of 4: a whole plane
    "384-384-16x8": (32, 384, 384, 16, 8, 2, False),                 # eight rows of 8
    "384-384-4x128": (8, 384, 384, 4, 128, 2, False),                # two tiles side by side in a row (tilesX = 2)
    "320-384-chunks-of-160": (32, 320, 384, 16, 16, 4, False),       # 10 k-tiles per chunk: zero-filled x rows 160 .. 191
}


@pytest.mark.parametrize("case", list(TAKEN))
def test_on_equals_off(case):
    N, Cin, Cout, H, W, tiles, short = TAKEN[case]
    x, gy = _inputs(N, Cin, Cout, H, W, seed=len(case) + N)
    res = _on_off(x, gy, Cin)
    (fin1, def1, n1, rec1), (fin0, def0, n0, rec0) = res[1], res[0]
    # two calls per switch position
    assert (n1, n0) == (2, 0) and (rec1["stage"], rec0["stage"]) == (WGRAD1X1, MFMA), (n1, n0, rec1, rec0)
    assert {k: v for k, v in rec1.items() if k != "stage"} == {k: v for k, v in rec0.items() if k != "stage"}
    assert (rec1["IT"], rec1["NT"], rec1["MODE"], rec1["xrow"]) == (3, 6, 1, 1), rec1
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert rec1["tiles"] == tiles, rec1
        assert (N * H * W // 64 % rec1["tiles"] != 0) == short
    _bits_equal(fin1, fin0, case + " finished")
    _bits_equal(def1, def0, case + " deferred")
    _bits_equal(fin1, def1, case + " finished against deferred")
    # the row of -0 inputs and the column of +0 gradients: sums of signed zeros from a +0 accumulator are +0
    assert bool((fin1[:, 0].contiguous().view(torch.int32) == 0).all())
    assert bool((fin1[1].contiguous().view(torch.int32) == 0).all())
    if case in ("384-384-one-tile", "384-96", "192-384-one-chunk", "384-90-ragged-block", "384-200-three-blocks",
                "384-384-64x64", "384-384-16x4", "384-384-4x128", "320-384-chunks-of-160"):
        want = torch.einsum("nchw,nkhw->ck", gy.double(), x.double()).view(Cout, Cin, 1, 1)
        close(fin1, want, rel=GRAD_REL, name=case)


REFUSED = {
    # name: N, Cin, Cout, H, W, what
    "60x44": (8, 384, 384, 60, 44, {}),                        # tiles of 64 x 1 pixels that overhang the rows
    "padding": (32, 384, 384, 16, 16, {"pad": (1, 1, 1, 1)}),
    "stride2": (32, 384, 384, 32, 32, {"stride": 2}),
    "C2": (32, 368, 384, 16, 16, {"C2": 16}),
    "Cin128-IT2": (32, 128, 384, 16, 16, {}),
    "Cout48-NT3": (32, 384, 48, 16, 16, {}),
    "bf16": (32, 384, 384, 16, 16, {"dtype": "bf16"}),
    "unaligned-x": (32, 384, 384, 16, 16, {"xoff": 1}),
    "unaligned-gy": (32, 384, 384, 16, 16, {"goff": 1}),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refusals_keep_their_kernel(case):
    from spr_pick_amd import _lib
    N, Cin, Cout, H, W, what = REFUSED[case]
    pad, stride = what.get("pad", (0, 0, 0, 0)), what.get("stride", 1)
    Ho = (H + pad[0] + pad[1] - 1) // stride + 1
    Wo = (W + pad[2] + pad[3] - 1) // stride + 1
    x, gy = _inputs(N, Cin, Cout, H, W, seed=len(case), Ho=Ho, Wo=Wo)
    x2 = torch.randn(N, what["C2"], H, W) if what.get("C2") else None
    res = _on_off(x, gy, Cin + what.get("C2", 0), xoff=what.get("xoff", 0), goff=what.get("goff", 0),
                  dtype=_lib.DT_BF16 if what.get("dtype") else 0, pad=pad, stride=stride, x2=x2)
    (fin1, def1, n1, rec1), (fin0, def0, n0, rec0) = res[1], res[0]
    assert (n1, n0) == (0, 0) and rec1 == rec0 and rec1["stage"] != WGRAD1X1, (n1, n0, rec1, rec0)
    if case in ("unaligned-x", "unaligned-gy"):
        # the row form has no staging for these tensors: the call is refused as it was, whatever the switch says
        assert rec1["stage"] == -1 and isinstance(fin1, str) and (fin1, def1) == (fin0, def0), (fin1, fin0)
        assert "16-byte aligned" in fin1
        return
    assert rec1["stage"] == MFMA, rec1
    _bits_equal(fin1, fin0, case + " finished")
    _bits_equal(def1, def0, case + " deferred")


def test_training_pass_and_graph_replay_on_equal_off(oracle_state):
    """The joint step of 2 patches of 64 x 64 (blind-spot DualNetwork, fp32: 8 rotated images, 512 tiles) through
    GraphedTrainStep: the eager pass with the stage on and the HIP-graph replay captured with it on give the outputs and
    the flat gradient of the eager pass with it off.  A pass makes 2 launches of the stage: output_block[0] and [2] of the
    main U-Net (the sigma-net's heads reduce over at most 96 channels and stay)."""
    from spr_pick_amd import Denoiser, graph_step
    from spr_pick_amd.params import PipelineOutput as P
    from test_gpu_pipeline import make_cfg
    L = _lib_()
    den = Denoiser(make_cfg(), device="cuda:0", mode="joint")
    den.load_state_dict({"models." + k: v for k, v in oracle_state.items()}, strict=False)
    den.train(); den.unfill()
    bn0 = {k: v.clone() for k, v in den.state_dict().items() if "running_" in k or "num_batches" in k}
    g = torch.Generator().manual_seed(29)
    inp = ((torch.rand(2, 1, 64, 64, generator=g) * 255).round() / 255).cuda()
    tgt = torch.tensor([[1.0], [-1.0]])
    st = graph_step.GraphedTrainStep(den, 2, 64, 0.75, 0.01, eager_warmup=1)
    keys = (P.LOSS, P.DENOISE_LOSS, P.DETECT, P.IMG_MU, P.IMG_DENOISED, P.NOISE_STD_DEV, P.MODEL_STD_DEV)

    def run(eager):
        den.load_state_dict(bn0, strict=False)
        torch.cuda.manual_seed(4321)
        st.grads.flat.fill_(float("nan"))
        n0 = L.sprk_wgrad1x1_launch_count()
        o = st(inp, tgt, flip_p=0.25, eager=eager)
        torch.cuda.synchronize()
        return ([o[k].detach().clone() for k in keys] + [st.grads.flat[:st.grads.live_numel].clone()],
                L.sprk_wgrad1x1_launch_count() - n0)

    try:
        L.sprk_wgrad1x1_enable(0)
        run(True)                      # the first pass finds the live parameters and compacts the gradient buffer
        off, n_off = run(True)
        L.sprk_wgrad1x1_enable(1)
        on, n_on = run(True)
        st.prepare(inp, tgt)
        assert st.fallback_reason is None
        replay, _ = run(False)
    finally:
        L.sprk_wgrad1x1_enable(1)
    assert (n_off, n_on) == (0, 2), (n_off, n_on)
    assert not bool(torch.isnan(off[-1]).any())
    for i, (a, b, c) in enumerate(zip(off, on, replay)):
        assert torch.equal(a, b), "eager on against eager off: tensor %d differs (max |d| %.3e)" % (i, float((a - b).abs().max()))
        assert torch.equal(a, c), "replay on against eager off: tensor %d differs (max |d| %.3e)" % (i, float((a - c).abs().max()))
