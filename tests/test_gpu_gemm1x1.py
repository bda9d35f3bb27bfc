"""The wide 1x1 layers of the heads on the streaming GEMM kernel (gemm1x1_kernel, csrc/gemm1x1.hip; SPRK_STAGE_GEMM1X1).

Unmasked forward and backward-data calls of 1x1 layers with at least 192 reduced channels whose plan is the one of the
launches that fill the machine (MT = 4, NT = 6) leave conv_mfma_kernel for a kernel that issues the same chain of
v_mfma_f32_16x16x4_f32 per output element from the same weight slabs and the same epilogue arithmetic.  So every
comparison here is bit for bit (int32 views: -0 and +0 are told apart) between the call with the stage switched on
(sprk_gemm1x1_enable(1): sprk_gemm1x1_launch_count advances by exactly 1, the last variant says GEMM1X1) and the same
call with it switched off (counter still, last variant MFMA), next to the fp64 CPU product at tests/test_gpu_ops.py's
budgets (2e-5 outputs, 5e-5 gradients; on the first and the last image, which hold the first and the last tile).

Shapes: the smallest launches the plan still gives MT = 4 (512 workgroups of 256 pixels x 96 channels: 8 images of
64 x 64 at 384 output channels, 32 at 96).  The kernel walks K in chunks of 32 rows through two LDS stages that carry
on across a workgroup's items: K = 192 (the minimum: 6 chunks, so no call has exactly 2), 196 / 197 / 200 / 388 (an
odd number of chunks, so consecutive items start in alternating stages; a last chunk of 1, 1 and 2 k-steps; 197: three
zero weight rows paired with the last 16-channel chunk's first channel).  An item is 256 pixels x two slabs of 96
channels (one slab for <= 96 channels); a persistent workgroup walks item b, b + grid, ...: 8, 16 and 20 images at 384
channels give every workgroup of a 256-CU device 1 item, exactly 2, and 2 or 3 (ragged last round)."""
import ctypes

import pytest
import torch

import conv_variant_cases as cv
from test_gpu_ops import REL, close, dev

pytestmark = pytest.mark.gpu

GRAD_REL = 5e-5
GEMM1X1, MFMA = 6, 5
NONE, LEAKY, RELU = 0, 1, 2


def _lib_():
    from spr_pick_amd import _lib
    return _lib.lib()


def _stage(which):
    out = (ctypes.c_int32 * 24)()
    assert _lib_().sprk_conv2d_last_variant(which, out) == 0
    return out[0]


def _bits_equal(a, b, what):
    assert not bool(torch.isnan(a).any()), "%s: elements left unwritten (NaN guard)" % what
    assert a.shape == b.shape
    same = torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    assert same, "%s: %d elements differ between the two kernels (max |d| %.3e)" % (
        what, int((a != b).sum()), float((a - b).abs().max()))


def _inputs(N, K, Cout, H, W, seed, zeros=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, K, H, W, generator=g)
    w = torch.randn(Cout, K, 1, 1, generator=g) / K ** 0.5
    if zeros:
        # products and whole sums of -0 and +0: channel 0 has only -0 weights, channel 1 only +0, and x has zeros of both signs
        x[torch.rand(x.shape, generator=g) < 0.02] = 0.0
        x[torch.rand(x.shape, generator=g) < 0.02] = -0.0
        w[0] = -0.0
        w[1] = 0.0
    return x, w, g


def _epilogue(kind, Cout, g):
    """-> bias, scale, shift, act"""
    b = torch.randn(Cout, generator=g)
    if kind == "none":
        return None, None, None, NONE
    if kind == "bias":
        return b, None, None, NONE
    if kind == "bias-leaky":
        return b, None, None, LEAKY
    if kind == "bias-relu":
        return b, None, None, RELU
    assert kind == "scale-shift"
    return None, torch.rand(Cout, generator=g) + 0.5, b, NONE


def _ref(x, w, b, sc, sh, act, imgs):
    y = torch.einsum("nkhw,ck->nchw", x[imgs].double(), w[:, :, 0, 0].double())
    if sc is not None:
        y = y * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    elif b is not None:
        y = y + b.double().view(1, -1, 1, 1)
    if act == LEAKY:
        y = torch.nn.functional.leaky_relu(y, 0.1)
    elif act == RELU:
        y = torch.relu(y)
    return y


def _forward_on_off(x, w, ep, xoff=0, dtype=0, pad=(0, 0, 0, 0), up1=False, x2=None):
    """The raw forward call with the stage on and off -> (y on, y off, launches of the stage on / off, stage on / off)"""
    from spr_pick_amd import ops
    L, d = _lib_(), dev()
    b, sc, sh, act = ep
    xd = cv.float_offset(x, xoff, d)
    x2d = None if x2 is None else x2.to(d)
    wd = w.to(d)
    bd, scd, shd = (None if t is None else t.to(d) for t in (b, sc, sh))
    geom = ops.make_geom(xd, x2d, wd, up1, 1, 1, pad, dtype=dtype)
    res = {}
    try:
        for on in (1, 0):
            L.sprk_gemm1x1_enable(on)
            poison = torch.full((x.shape[0], w.shape[0], geom.Hout, geom.Wout), float("nan"), device=d)
            del poison
            n0 = L.sprk_gemm1x1_launch_count()
            y = ops.conv2d_forward(xd, x2d, wd, geom, bias=bd, act=act, scale=scd, shift=shd)
            res[on] = (y, L.sprk_gemm1x1_launch_count() - n0, _stage(0))
            torch.cuda.synchronize()
    finally:
        L.sprk_gemm1x1_enable(1)
    return res[1][0], res[0][0], (res[1][1], res[0][1]), (res[1][2], res[0][2])


def _rounds(N, H, W, Cout):
    """items of the busiest and of the idlest workgroup (gemm1x1_grid: one workgroup per CU, whole groups of 8 x the
    channel parts of a tile)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nblk = -(-Cout // 96)
    nh = -(-nblk // (2 if nblk >= 2 else 1))
    items = N * -(-(H * W) // 256) * nh
    grid = min(items, cus)
    if grid >= 8 * nh:
        grid -= grid % (8 * nh)
    return -(-items // grid), items // grid


# name: N, K, Cout, H, W, epilogue, items of (busiest, idlest) workgroup on a 256-CU device or None
TAKEN = {
    "384-384-N8-one-item": (8, 384, 384, 64, 64, "bias-leaky", (1, 1)),
    "384-384-N16-two-items": (16, 384, 384, 64, 64, "bias", (2, 2)),
    "384-384-N20-ragged-round": (20, 384, 384, 64, 64, "bias-leaky", (3, 2)),
    "384-96-N32": (32, 384, 96, 64, 64, "bias-leaky", (2, 2)),
    "192-96-N32-minK": (32, 192, 96, 64, 64, "bias-relu", None),
    "192-384-N8-none": (8, 192, 384, 64, 64, "none", None),
    "192-384-N8-bias": (8, 192, 384, 64, 64, "bias", None),
    "192-384-N8-relu": (8, 192, 384, 64, 64, "bias-relu", None),
    "192-384-N8-scale-shift": (8, 192, 384, 64, 64, "scale-shift", None),
    "K196": (32, 196, 96, 64, 64, "bias-leaky", None),
    "K197": (32, 197, 96, 64, 64, "none", None),
    "K200": (32, 200, 96, 64, 64, "scale-shift", None),
    "K388-N8": (8, 388, 384, 64, 64, "bias-leaky", None),
    "Cout90": (32, 192, 90, 64, 64, "bias-leaky", None),       # a partial last 16-channel tile
    "Cout200": (11, 192, 200, 64, 64, "bias-leaky", None),     # three slabs: the second item of a tile has one
    "40x40": (16, 192, 384, 40, 40, "bias-leaky", None),       # 1600 pixels: a quarter-filled last tile per plane
    "30x30": (128, 192, 96, 30, 30, "bias-leaky", None),       # 900 pixels, a multiple of 4
}


@pytest.mark.parametrize("case", list(TAKEN))
def test_forward_on_equals_off(case):
    N, K, Cout, H, W, kind, rounds = TAKEN[case]
    x, w, g = _inputs(N, K, Cout, H, W, seed=len(case) + K, zeros=kind == "none")
    ep = _epilogue(kind, Cout, g)
    on, off, launches, stages = _forward_on_off(x, w, ep)
    assert launches == (1, 0) and stages == (GEMM1X1, MFMA), (launches, stages)
    if rounds is not None and torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert _rounds(N, H, W, Cout) == rounds
    _bits_equal(on, off, case)
    imgs = [0, N - 1]
    close(on[imgs], _ref(x, w, *ep, imgs), rel=REL, name=case)
    if kind == "none":
        # c * 1 + 0 turns the -0 sums of channel 0 into +0
        assert bool((on[:, :2].contiguous().view(torch.int32) == 0).all())


def test_cout_100_plans_four_tile_slabs_and_is_refused():
    """7 channel tiles are planned as 2 slabs of 4 (NT = 4), not as slabs of 6: the stage takes NT = 6 plans only."""
    x, w, g = _inputs(32, 196, 100, 64, 64, seed=100)
    on, off, launches, stages = _forward_on_off(x, w, _epilogue("bias-leaky", 100, g))
    assert launches == (0, 0) and stages == (MFMA, MFMA), (launches, stages)
    _bits_equal(on, off, "Cout100")


REFUSED = {
    # name: N, K, Cout, H, W, what
    "31x31": (128, 192, 96, 31, 31, {}),                      # 961 pixels per plane
    "padding": (32, 192, 96, 64, 64, {"pad": (1, 1, 1, 1)}),
    "up1": (32, 192, 96, 64, 64, {"up1": True}),
    "C2": (32, 192, 96, 64, 64, {"C2": 16}),
    "K128": (32, 128, 96, 64, 64, {}),
    "bf16": (32, 192, 96, 64, 64, {"dtype": "bf16"}),
    "unaligned-x": (32, 192, 96, 64, 64, {"xoff": 1}),
    "MT2-N4": (4, 384, 384, 64, 64, {}),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refusals_keep_their_kernel(case):
    from spr_pick_amd import _lib
    N, K, Cout, H, W, what = REFUSED[case]
    up1 = what.get("up1", False)
    x, w, g = _inputs(N, K, Cout, H // 2 if up1 else H, W // 2 if up1 else W, seed=len(case))
    x2 = None
    if what.get("C2"):
        x2 = torch.randn(N, what["C2"], H, W, generator=g)
        w = torch.randn(Cout, K + what["C2"], 1, 1, generator=g) / K ** 0.5
    on, off, launches, stages = _forward_on_off(x, w, _epilogue("bias-leaky", Cout, g), xoff=what.get("xoff", 0),
                                                dtype=_lib.DT_BF16 if what.get("dtype") else 0,
                                                pad=what.get("pad", (0, 0, 0, 0)), up1=up1, x2=x2)
    assert launches == (0, 0) and stages[0] == stages[1] != GEMM1X1, (launches, stages)
    if not what.get("dtype"):
        assert stages[0] == MFMA
    _bits_equal(on, off, case)


def test_masked_backward_data_is_refused():
    """A masked call of 384 reduced channels: too wide for mask1x1_kernel, and this stage takes unmasked calls only."""
    from spr_pick_amd import ops
    L, S, d = _lib_(), torch.ops.sprk, dev()
    g = torch.Generator().manual_seed(7)
    mask = torch.nn.functional.leaky_relu(torch.randn(8, 384, 64, 64, generator=g), 0.1).to(d)
    gy = torch.randn(8, 384, 64, 64, generator=g).to(d)
    w = (torch.randn(384, 384, 1, 1, generator=g) / 384 ** 0.5).to(d)
    geom = ops.make_geom(mask, None, w, False, 1, 1, (0, 0, 0, 0))
    res = []
    try:
        for on in (1, 0):
            L.sprk_gemm1x1_enable(on)
            n0 = L.sprk_gemm1x1_launch_count()
            res.append(S.conv2d_bwd_data(gy, w, ops.geom_list(geom), mask, ops.ACT_LEAKY, None))
            assert L.sprk_gemm1x1_launch_count() == n0 and _stage(1) == MFMA
            torch.cuda.synchronize()
    finally:
        L.sprk_gemm1x1_enable(1)
    _bits_equal(res[0], res[1], "masked backward-data")


@pytest.mark.parametrize("case", ["384-384", "96-384"])
def test_backward_data_on_equals_off(case):
    """ops.conv2d + autograd of a linear 1x1 layer: the input gradient reduces over the layer's output channels (384).
    Its -0 sums leave as +0 (the old epilogue's c * 1 + 0): weights of input channel 0 are all -0."""
    from spr_pick_amd import ops
    L, d = _lib_(), dev()
    N, Cin = (8, 384) if case == "384-384" else (32, 96)
    g = torch.Generator().manual_seed(N)
    x = torch.randn(N, Cin, 64, 64, generator=g)
    w = torch.randn(384, Cin, 1, 1, generator=g) / Cin ** 0.5
    w[:, 0] = -0.0
    gy = torch.randn(N, 384, 64, 64, generator=g)
    gy[torch.rand(gy.shape, generator=g) < 0.02] = 0.0
    gyd = gy.to(d)
    res = {}
    try:
        for on in (1, 0):
            L.sprk_gemm1x1_enable(on)
            xd, wd = x.to(d).requires_grad_(True), w.to(d).requires_grad_(True)
            ran = {}
            n0 = L.sprk_gemm1x1_launch_count()
            y = ops.conv2d(xd, wd, None)
            nf = L.sprk_gemm1x1_launch_count() - n0
            # the backward calls run on the autograd engine's thread, where the record of the last call lives
            xd.register_hook(lambda _g: ran.update(bwd=_stage(1)))
            poison = torch.full_like(xd, float("nan"))
            del poison
            y.backward(gyd)
            torch.cuda.synchronize()
            res[on] = (xd.grad, wd.grad, L.sprk_gemm1x1_launch_count() - n0 - nf, ran["bwd"], nf)
    finally:
        L.sprk_gemm1x1_enable(1)
    # the forward of the 384 -> 384 layer is a wide GEMM too; the 96 -> 384 layer reduces over 96 channels there
    assert res[1][2:] == (1, GEMM1X1, 1 if case == "384-384" else 0) and res[0][2:] == (0, MFMA, 0), (res[1][2:], res[0][2:])
    _bits_equal(res[1][0], res[0][0], case + " gx")
    _bits_equal(res[1][1], res[0][1], case + " gw")
    assert bool((res[1][0][:, 0].contiguous().view(torch.int32) == 0).all())
    imgs = [0, N - 1]
    want = torch.einsum("nchw,ck->nkhw", gy[imgs].double(), w[:, :, 0, 0].double())
    close(res[1][0][imgs], want, rel=GRAD_REL, name=case + " gx")


def test_training_pass_and_graph_replay_on_equal_off(oracle_state):
    """The joint step of 32 patches of 64 x 64 (blind-spot DualNetwork, fp32) through GraphedTrainStep: the eager pass
    with the stage on and the HIP-graph replay captured with it on give the outputs and the flat gradient of the eager
    pass with it off.  A pass makes 3 launches of the stage: output_block[0] and [2] forward, output_block[0]
    backward-data (the backward-data of [2] and of output_conv are masked calls)."""
    from spr_pick_amd import Denoiser, graph_step
    from spr_pick_amd.params import PipelineOutput as P
    from test_gpu_pipeline import make_cfg
    L = _lib_()
    den = Denoiser(make_cfg(), device="cuda:0", mode="joint")
    den.load_state_dict({"models." + k: v for k, v in oracle_state.items()}, strict=False)
    den.train(); den.unfill()
    bn0 = {k: v.clone() for k, v in den.state_dict().items() if "running_" in k or "num_batches" in k}
    g = torch.Generator().manual_seed(23)
    inp = ((torch.rand(32, 1, 64, 64, generator=g) * 255).round() / 255).cuda()
    tgt = torch.where(torch.rand(32, 1, generator=g) < 0.5, 1.0, -1.0)
    st = graph_step.GraphedTrainStep(den, 32, 64, 0.75, 0.01, eager_warmup=1)
    keys = (P.LOSS, P.DENOISE_LOSS, P.DETECT, P.IMG_MU, P.IMG_DENOISED, P.NOISE_STD_DEV, P.MODEL_STD_DEV)

    def run(eager):
        den.load_state_dict(bn0, strict=False)
        torch.cuda.manual_seed(4321)
        st.grads.flat.fill_(float("nan"))
        n0 = L.sprk_gemm1x1_launch_count()
        o = st(inp, tgt, flip_p=0.25, eager=eager)
        torch.cuda.synchronize()
        return ([o[k].detach().clone() for k in keys] + [st.grads.flat[:st.grads.live_numel].clone()],
                L.sprk_gemm1x1_launch_count() - n0)

    try:
        L.sprk_gemm1x1_enable(0)
        run(True)                      # the first pass finds the live parameters and compacts the gradient buffer
        off, n_off = run(True)
        L.sprk_gemm1x1_enable(1)
        on, n_on = run(True)
        st.prepare(inp, tgt)
        assert st.fallback_reason is None
        replay, _ = run(False)
    finally:
        L.sprk_gemm1x1_enable(1)
    assert (n_off, n_on) == (0, 3), (n_off, n_on)
    assert not bool(torch.isnan(off[-1]).any())
    for i, (a, b, c) in enumerate(zip(off, on, replay)):
        assert torch.equal(a, b), "eager on against eager off: tensor %d differs (max |d| %.3e)" % (i, float((a - b).abs().max()))
        assert torch.equal(a, c), "replay on against eager off: tensor %d differs (max |d| %.3e)" % (i, float((a - c).abs().max()))
