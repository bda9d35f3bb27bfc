"""The activation mask inside the backward-data kernel of the 1x1 head layers, and the strided stem on a tiled kernel.

Part 1 (mask1x1_kernel, csrc/mask1x1.hip): sprk_conv2d_bwd_data_masked on a 1x1 layer of at most 96 reduced channels
multiplies by act'(mask) before its only store.  The kernel walks the prepared weight slab of conv_mfma_kernel with that
kernel's chain of v_mfma_f32_16x16x4_f32 per output element, so every comparison with today's composition (unmasked
conv2d_bwd_data, then act_bwd with the mask) is torch.equal.  sprk_conv2d_bwd_data_mask_fused tells beforehand which calls
apply the mask in their kernel, and sprk_mask1x1_launch_count what a call did.

Part 2 (conv_bwd_data_stem_kernel, csrc/conv.hip): backward-data of the strided, few-input-channel layers (the
detector's 7x7 stride-2 stem).  A workgroup stages the layer's weights and its tile's window of gy in LDS, and every
thread then runs the loops of conv_bwd_data_direct_kernel (ky, kx, co ascending, invalid taps skipped, one chain
s += gy * w from 0): the same operations in the same order, torch.equal against the same call with SPRK_DT_NAIVE in the
geometry's dtype, which keeps the one-thread-per-element kernel."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

UNITS0 = 32     # networks.ResNet8: units[0]


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _both(N, Cin, H, W, Cout, K, stride, pad, dil=1, seed=0):
    """(tiled, naive) input gradients of one layer; the output block is poisoned first, so an element the tiled kernel
    leaves unwritten shows as NaN."""
    from spr_pick_amd import _lib, ops
    S = torch.ops.sprk
    g = torch.Generator().manual_seed(seed)
    x = torch.empty(N, Cin, H, W, device=dev())
    w = (torch.randn(Cout, Cin, K, K, generator=g) / K).to(dev())
    geom = ops.make_geom(x, None, w, False, stride, dil, pad)
    gy = torch.randn(N, Cout, geom.Hout, geom.Wout, generator=g)
    gy[torch.rand(gy.shape, generator=g) < 0.05] = 0.0
    gy = gy.to(dev())
    naive = ops.make_geom(x, None, w, False, stride, dil, pad, dtype=_lib.DT_NAIVE)
    want = S.conv2d_bwd_data(gy, w, ops.geom_list(naive), None, ops.ACT_NONE, None)
    poison = torch.full_like(want, float("nan"))
    del poison
    got = S.conv2d_bwd_data(gy, w, ops.geom_list(geom), None, ops.ACT_NONE, None)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (N, Cin, H, W)
    assert float(want.abs().max()) > 0
    return got, want


def _same(got, want):
    assert not bool(torch.isnan(got).any()), "the tiled kernel left elements of gin unwritten"
    assert torch.equal(got, want), "max |d| %.3e at %d elements" % (float((got - want).abs().max()), int((got != want).sum()))


@pytest.mark.parametrize("H,W,pad", [(64, 64, (0, 0, 0, 0)), (64, 64, (3, 3, 3, 3)), (61, 61, (3, 3, 3, 3))],
                         ids=["64x64-nopad", "64x64-pad3", "61x61-pad3"])
def test_stem_tiled_equals_naive(H, W, pad):
    """[4,1,H,W], 7x7, stride 2, Cout = units[0].  64 columns are two tiles of 32, 64 rows eight tiles of 8; without
    padding the last input row and column (63) are reached by no tap at all and must be written as 0; 61 leaves ragged
    last tiles in both directions."""
    got, want = _both(4, 1, H, W, UNITS0, 7, 2, pad, seed=H + pad[0])
    _same(got, want)
    if pad[0] == 0 and H == 64:
        # (64 - 7) // 2 + 1 = 29 output rows reach input rows 0..62
        assert bool((got[:, :, 63, :] == 0).all()) and bool((got[:, :, :, 63] == 0).all())


@pytest.mark.parametrize("case", ["cin3-stride3", "dil2", "asym-pad"])
def test_stem_tiled_other_geometries(case):
    """The per-thread channel loop (Cin = 3), a stride that does not divide the tile, dilation, and unequal paddings:
    the window arithmetic of the tile (first reachable output row / column, window size) in its other branches."""
    if case == "cin3-stride3":
        got, want = _both(3, 3, 50, 70, 16, 5, 3, (2, 2, 1, 1), seed=11)
    elif case == "dil2":
        got, want = _both(2, 2, 40, 36, 8, 3, 2, (2, 2, 2, 2), dil=2, seed=12)
    else:
        got, want = _both(2, 1, 33, 65, UNITS0, 7, 2, (1, 4, 5, 0), seed=13)
    _same(got, want)


def test_weights_beyond_the_lds_rule_keep_the_old_kernel():
    """64 x 8 x 7 x 7 weights are 98 KB, more than the 64 KB the tiled kernel may use: the call keeps
    conv_bwd_data_direct_kernel and still equals the SPRK_DT_NAIVE call."""
    got, want = _both(2, 8, 32, 32, 64, 7, 2, (3, 3, 3, 3), seed=21)
    _same(got, want)


# ---- Part 1: the mask in the store of the 1x1 backward-data kernel ---------------------------------------------------
def _mask_and_grad(N, C, H, W, K, seed):
    """mask: a LeakyReLU output of seeded noise with a few entries forced to +0.0, -0.0 and a negative value; gy."""
    g = torch.Generator().manual_seed(seed)
    mask = torch.nn.functional.leaky_relu(torch.randn(N, C, H, W, generator=g), 0.1)
    flat = mask.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:96]
    flat[idx[:32]] = 0.0
    flat[idx[32:64]] = -0.0
    flat[idx[64:]] = -1.5
    gy = torch.randn(N, K, H, W, generator=g)
    gy[torch.rand(gy.shape, generator=g) < 0.02] = 0.0
    return mask.to(dev()), gy.to(dev())


def _fused_and_composed(N, C, H, W, K, act, ksize=1, dtype=0, seed=0):
    """-> (masked call, unmasked call + act_bwd, launches of the 1x1 kernel the masked call made, the query's answer)"""
    from spr_pick_amd import _lib, ops
    S, L = torch.ops.sprk, _lib.lib()
    mask, gy = _mask_and_grad(N, C, H, W, K, seed)
    g = torch.Generator().manual_seed(seed + 1)
    w = (torch.randn(K, C, ksize, ksize, generator=g) / (C ** 0.5 * ksize)).to(dev())
    pad = (ksize // 2,) * 4
    geom = ops.make_geom(mask, None, w, False, 1, 1, pad, dtype=dtype)
    plain = S.conv2d_bwd_data(gy, w, ops.geom_list(geom), None, ops.ACT_NONE, None)
    want = S.act_bwd(plain, mask, act, [N, C, H, W], 0, True, None, False, 0)
    del plain
    poison = torch.full_like(want, float("nan"))
    del poison
    asked = int(L.sprk_conv2d_bwd_data_mask_fused(ctypes.byref(geom)))
    n0 = L.sprk_mask1x1_launch_count()
    got = S.conv2d_bwd_data(gy, w, ops.geom_list(geom), mask, act, None)
    n1 = L.sprk_mask1x1_launch_count()
    torch.cuda.synchronize()
    return got, want, n1 - n0, asked


# (N images, C = the layer's input channels = output channels of the GEMM, H, W, K = the layer's Cout = reduced channels)
FUSED_CASES = {
    # the first three: the smallest launches plan_fwd still gives MT = 4 (512 workgroups of 256 pixels x one slab)
    "K96-N384-leaky": (8, 384, 64, 64, 96, "leaky"),      # 8 x 16 tiles x 4 slabs of 96 channels
    "K96-N96-relu": (32, 96, 64, 64, 96, "relu"),         # 32 x 16 tiles x 1 slab
    "K2-N96": (32, 96, 64, 64, 2, "leaky"),               # ragged K: rows 2, 3 of the one k-step are zero rows
    "K1-N96": (32, 96, 64, 64, 1, "leaky"),
    "K96-N384-40x40": (16, 384, 40, 40, 96, "leaky"),     # 1600 pixels: rows shorter than a tile, 12.5 tiles of 128 per plane
    "K96-N100": (16, 100, 64, 64, 96, "leaky"),           # 7 channel tiles in 2 slabs of 4: the last slab is ragged
    "K96-N384-MT2": (4, 384, 64, 64, 96, "leaky"),        # 256 workgroups at MT = 4: the plan falls to MT = 2
    "K40-N96": (32, 96, 64, 64, 40, "relu"),              # chunks of 16, 16 and 8 reduced channels
}


@pytest.mark.parametrize("case", list(FUSED_CASES))
def test_fused_equals_composed(case):
    from spr_pick_amd import ops
    N, C, H, W, K, act = FUSED_CASES[case]
    got, want, launches, asked = _fused_and_composed(N, C, H, W, K, ops.ACT_LEAKY if act == "leaky" else ops.ACT_RELU,
                                                     seed=len(case) + K)
    assert launches == 1 and asked == 1, (launches, asked)
    _same(got, want)
    assert float(want.abs().max()) > 0


REFUSED_CASES = {
    "small-plan": (2, 96, 16, 16, 96, 1, 0),              # 2 images of 16 x 16: an MT = 1 plan (chunk_mma_small)
    "HW-not-4n": (128, 96, 31, 31, 96, 1, 0),             # 961 pixels per plane; 128 images keep the plan at MT = 4
    "K128": (32, 96, 64, 64, 128, 1, 0),
    "3x3-not-winograd": (32, 16, 64, 64, 96, 3, 0),       # 16 GEMM output channels: the Winograd kernel wants 33
    "bf16": (32, 96, 64, 64, 96, 1, "bf16"),
}


@pytest.mark.parametrize("case", list(REFUSED_CASES))
def test_refusals_take_the_old_path(case):
    """The counter does not move, the query says 0, and the result is the composition's."""
    from spr_pick_amd import _lib, ops
    N, C, H, W, K, ks, dt = REFUSED_CASES[case]
    got, want, launches, asked = _fused_and_composed(N, C, H, W, K, ops.ACT_LEAKY, ksize=ks,
                                                     dtype=_lib.DT_BF16 if dt == "bf16" else 0, seed=len(case))
    assert launches == 0 and asked == 0, (launches, asked)
    _same(got, want)


def test_30x30_planes_are_900_pixels():
    """30 x 30 planes have a pixel count that IS a multiple of 4 (rows of 120 bytes, planes of 3600): with 128 images
    the plan is MT = 4 and the 1x1 kernel takes the call; query and counter agree, and the result is the composition's."""
    from spr_pick_amd import ops
    got, want, launches, asked = _fused_and_composed(128, 96, 30, 30, 96, ops.ACT_LEAKY, seed=30)
    assert launches == asked == 1, (launches, asked)
    _same(got, want)


def test_wide_3x3_is_fused_by_winograd_not_by_the_1x1_kernel():
    from spr_pick_amd import ops
    got, want, launches, asked = _fused_and_composed(8, 96, 64, 64, 96, ops.ACT_LEAKY, ksize=3, seed=33)
    assert launches == 0 and asked == 1, (launches, asked)


def _switches(on):
    from spr_pick_amd import networks
    networks.FUSE_HEAD_MASK_IN = networks.FUSE_HEAD_MASK_12 = networks.FUSE_HEAD_MASK_23 = on


def _net(kind, seed=5):
    from spr_pick_amd import networks
    torch.manual_seed(seed)
    cls = networks.DualNetworkShallow if kind == "shallow" else networks.DualNetwork
    net = cls(in_channels=1, out_channels=1 if kind == "shallow" else 2, blindspot=False, zero_output_weights=False).to(dev())
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.05)
    return net


@pytest.mark.parametrize("kind", ["shallow", "dual"])
def test_training_pass_switches_on_equals_off(kind):
    """32 patches of 64 x 64 through a U-Net without a blind spot, forward + backward: output, every parameter gradient
    (the bias gradients with their final sums finished at once, and left pending inside a FlatGrads context) and the
    input gradient are torch.equal with the three links fused and unfused; fused, the pass makes 3 launches of the 1x1
    kernel (decode_block_1[2] -> output_block[0] -> output_block[2] -> output_conv)."""
    from spr_pick_amd import _lib, graph_step
    L = _lib.lib()
    net = _net(kind)
    params = list(net.parameters())
    x0 = torch.rand(32, 1, 64, 64, generator=torch.Generator().manual_seed(9)).to(dev())
    res = []
    try:
        for deferred in (False, True):
            for on in (False, True):
                _switches(on)
                x = x0.clone().requires_grad_(True)
                fg = graph_step.FlatGrads(params)
                fg.begin_step()
                n0 = L.sprk_mask1x1_launch_count()
                if deferred:
                    with fg:
                        o = net(x)
                        o.square().mean().backward()
                else:
                    o = net(x)
                    o.square().mean().backward()
                torch.cuda.synchronize()
                assert L.sprk_mask1x1_launch_count() - n0 == (3 if on else 0)
                grads = [None if q.grad is None else q.grad.clone() for q in params]
                res.append(("%s, %s" % ("fused" if on else "unfused", "deferred" if deferred else "immediate"),
                            [o.detach().clone(), x.grad.clone()] + grads))
                for q in params:
                    q.grad = None
                del o, fg
    finally:
        _switches(True)
    name0, ref = res[0]
    assert sum(t is not None for t in ref) > 20 and float(ref[1].abs().max()) > 0
    for name, ts in res[1:]:
        for i, (a, c) in enumerate(zip(ref, ts)):
            assert (a is None) == (c is None), (name, i)
            if a is not None:
                assert torch.equal(a, c), "%s against %s: tensor %d differs (max |d| %.3e)" % (
                    name, name0, i, float((a - c).abs().max()))


def test_graphed_train_step_replay_fused_equals_eager_unfused(oracle_state):
    """The joint step of 32 patches through GraphedTrainStep: the eager pass with the links unfused, the eager pass
    with them fused and the HIP-graph replay of the fused pass give the same outputs and the same flat gradient."""
    from spr_pick_amd import Denoiser, _lib, graph_step
    from spr_pick_amd.params import PipelineOutput as P
    from test_gpu_pipeline import make_cfg
    L = _lib.lib()
    den = Denoiser(make_cfg(), device="cuda:0", mode="joint")
    den.load_state_dict({"models." + k: v for k, v in oracle_state.items()}, strict=False)
    den.train(); den.unfill()
    bn0 = {k: v.clone() for k, v in den.state_dict().items() if "running_" in k or "num_batches" in k}
    g = torch.Generator().manual_seed(17)
    inp = ((torch.rand(32, 1, 64, 64, generator=g) * 255).round() / 255).cuda()
    tgt = torch.where(torch.rand(32, 1, generator=g) < 0.5, 1.0, -1.0)
    st = graph_step.GraphedTrainStep(den, 32, 64, 0.75, 0.01, eager_warmup=1)
    keys = (P.LOSS, P.DENOISE_LOSS, P.DETECT, P.IMG_MU, P.IMG_DENOISED, P.NOISE_STD_DEV, P.MODEL_STD_DEV)

    def run(eager):
        den.load_state_dict(bn0, strict=False)
        torch.cuda.manual_seed(4321)
        st.grads.flat.fill_(float("nan"))
        n0 = L.sprk_mask1x1_launch_count()
        o = st(inp, tgt, flip_p=0.25, eager=eager)
        torch.cuda.synchronize()
        return [o[k].detach().clone() for k in keys] + [st.grads.flat[:st.grads.live_numel].clone()], L.sprk_mask1x1_launch_count() - n0

    try:
        _switches(False)
        run(True)                      # the first pass finds the live parameters and compacts the gradient buffer
        off, n_off = run(True)
        _switches(True)
        on, n_on = run(True)
        st.prepare(inp, tgt)
        assert st.fallback_reason is None
        replay, _ = run(False)
    finally:
        _switches(True)
    # the sigma-net's three links, and output_block[0] -> [2] -> output_conv of the blind-spot net
    assert n_off == 0 and n_on >= 5, (n_off, n_on)
    assert not bool(torch.isnan(off[-1]).any())
    for i, (a, b, c) in enumerate(zip(off, on, replay)):
        assert torch.equal(a, b), "eager fused against eager unfused: tensor %d differs (max |d| %.3e)" % (i, float((a - b).abs().max()))
        assert torch.equal(a, c), "replay fused against eager unfused: tensor %d differs (max |d| %.3e)" % (i, float((a - c).abs().max()))
