"""The backward-weight of the 3x3 layers on chunks of 48 input channels on the streaming kernel (wgrad3x3_kernel,
csrc/wgrad3x3.hip; SPRK_STAGE_WGRAD3X3).

fp32 3x3 stride-1 same-size calls whose plan is MODE 2 with one chunk of 48 input channels per workgroup (27 k-tiles) and
blocks of 3 or 6 output tiles, over planes of 16, 32 or 64 columns, leave conv_wgrad_mfma_kernel<7, 3 | 6, ., 2> for a
kernel that issues the same chain of v_mfma_f32_16x16x4_f32 per element of the partial slabs, on the same split into
groups, channel chunks and output blocks, followed by the same reduction.  So every comparison is bit for bit (int32
views: -0 and +0 are told apart) between the call with the stage on (sprk_wgrad3x3_enable(1): sprk_wgrad3x3_launch_count
advances by exactly 1 per call, the last variant says stage 8) and the same call with it off (counter still, stage 5),
finished in the call and deferred to reduce_pending; the first case of each family is also held against the fp64 product
at tests/test_gpu_ops.py's gradient budget (5e-5 of the largest element).

Shapes (tests/wgrad3x3_cases.py): the smallest the planner still gives that plan on a 256-CU device.  1 x 64 tiles (halo
rows on both sides of every tile), 2 x 32 and 4 x 16; 1, 2 and 3 tiles per group (each LDS stage filled once; the first
re-use of a stage), a shorter last group, groups that cross images; 48 -> 48, 96 -> 96 (two chunks, eight waves of 7 k-tiles),
48 -> 96, 96 -> 48, 144 -> 96 and 48 + 48 -> 96 with the second source, 40 and 90 output channels (zero-filled gy rows); the
symmetric pads of Conv2d, the shifted ones of ShiftConv2d and the two other same-size layouts."""
import pytest
import torch

import conv_variant_cases as cv
import wgrad3x3_cases as w3
from test_gpu_ops import close, dev

pytestmark = pytest.mark.gpu

GRAD_REL = 5e-5


def _bits_equal(a, b, what):
    assert not bool(torch.isnan(a).any()), "%s: elements left unwritten (NaN guard)" % what
    assert a.shape == b.shape
    same = torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    assert same, "%s: %d elements differ between the two kernels (max |d| %.3e)" % (
        what, int((a != b).sum()), float((a - b).abs().max()))


def _inputs(N, C1, C2, Cout, Hx, Wx, Ho, Wo, seed, H2=None, W2=None):
    """x (x2) and gy with zeros of both signs and two rows whose products are all +-0: input channel 0 is -0 everywhere
    (every product of its rows is a signed zero, and their sum must keep its sign rules), output channel 1 of gy +0."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C1, Hx, Wx, generator=g)
    x2 = torch.randn(N, C2, H2 or Hx, W2 or Wx, generator=g) if C2 else None
    gy = torch.randn(N, Cout, Ho, Wo, generator=g)
    for t in (x, x2, gy):
        if t is not None:
            t[torch.rand(t.shape, generator=g) < 0.02] = 0.0
            t[torch.rand(t.shape, generator=g) < 0.02] = -0.0
    x[:, 0] = -0.0
    gy[:, 1] = 0.0
    return x, x2, gy


def _on_off(x, x2, gy, K, pad, stride=1, dil=1, up1=False, xoff=0, dtype=0):
    """The raw backward-weight call, finished and deferred, with the stage on and off
    -> {on: (gw finished, gw deferred, launches of the stage, record of the last call)}; a refused call leaves its message"""
    from spr_pick_amd import _lib, ops
    S, d = torch.ops.sprk, dev()
    xd, gyd = cv.float_offset(x, xoff, d), gy.to(d)
    x2d = None if x2 is None else x2.to(d)
    w = torch.empty(gy.shape[1], x.shape[1] + (0 if x2 is None else x2.shape[1]), K, K, device=d)
    geom = ops.make_geom(xd, x2d, w, up1, stride, dil, pad, dtype=dtype)
    assert (geom.Hout, geom.Wout) == tuple(gy.shape[2:])
    res = {}
    try:
        for on in (1, 0):
            w3.switch(on)
            n0 = w3.launches()
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
            res[on] = (got[0], got[1], w3.launches() - n0, w3.last_record())
    finally:
        w3.switch(1)
    return res


def _reference(x, x2, gy, pad):
    xx = x if x2 is None else torch.cat([x, x2], 1)
    xp = torch.nn.functional.pad(xx.double(), (pad[2], pad[3], pad[0], pad[1]))
    H, W = gy.shape[2:]
    taps = [torch.einsum("nchw,nkhw->ck", gy.double(), xp[:, :, ky:ky + H, kx:kx + W]) for ky in range(3) for kx in range(3)]
    return torch.stack(taps, -1).view(gy.shape[1], xx.shape[1], 3, 3)


FP64_TOO = ("48-48-64x64-N4-one-tile", "48-48-32x32-N16", "48-48-16x16-N64", "48-40-ragged-block", "96-96-32x32",
            "144-96-two-sources", "96-90-ragged-block", "pads-0-2-0-2", "pads-1-1-2-0")


@pytest.mark.parametrize("case", list(w3.TAKEN))
def test_on_equals_off(case):
    N, C1, C2, Cout, H, W, pad, tiles = w3.TAKEN[case]
    x, x2, gy = _inputs(N, C1, C2, Cout, H, W, H, W, seed=len(case) + N)
    res = _on_off(x, x2, gy, 3, pad)
    (fin1, def1, n1, rec1), (fin0, def0, n0, rec0) = res[1], res[0]
    # two calls per switch position
    assert (n1, n0) == (2, 0) and (rec1["stage"], rec0["stage"]) == (w3.WGRAD3X3, w3.MFMA), (n1, n0, rec1, rec0)
    assert {k: v for k, v in rec1.items() if k != "stage"} == {k: v for k, v in rec0.items() if k != "stage"}
    assert (rec1["IT"], rec1["MODE"]) == (7, 2), rec1
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert rec1["tiles"] == tiles, rec1
    _bits_equal(fin1, fin0, case + " finished")
    _bits_equal(def1, def0, case + " deferred")
    _bits_equal(fin1, def1, case + " finished against deferred")
    # the rows of -0 inputs and the column of +0 gradients: sums of signed zeros from a +0 accumulator are +0
    assert bool((fin1[:, 0].contiguous().view(torch.int32) == 0).all())
    assert bool((fin1[1].contiguous().view(torch.int32) == 0).all())
    if case in FP64_TOO:
        close(fin1, _reference(x, x2, gy, pad), rel=GRAD_REL, name=case)


@pytest.mark.parametrize("case", list(w3.PLANNED_ELSEWHERE))
def test_other_plans_keep_their_kernel(case):
    N, C1, C2, Cout, H, W, pad = w3.PLANNED_ELSEWHERE[case]
    x, x2, gy = _inputs(N, C1, C2, Cout, H, W, H, W, seed=len(case) + N)
    res = _on_off(x, x2, gy, 3, pad)
    (fin1, def1, n1, rec1), (fin0, def0, n0, rec0) = res[1], res[0]
    assert (n1, n0) == (0, 0) and rec1 == rec0 and rec1["stage"] == w3.MFMA, (n1, n0, rec1, rec0)
    _bits_equal(fin1, fin0, case + " finished")
    _bits_equal(def1, def0, case + " deferred")


@pytest.mark.parametrize("case", list(w3.REFUSED))
def test_refusals_keep_their_kernel(case):
    N, C1, C2, Cout, H, W, what = w3.REFUSED[case]
    g = w3.refused_geom(case)
    up1 = bool(what.get("up1"))
    x, x2, gy = _inputs(N, C1, C2, Cout, H // 2 if up1 else H, W // 2 if up1 else W, g.Hout, g.Wout, seed=len(case))
    pad = what.get("pad", w3.SHIFT)
    res = _on_off(x, x2, gy, what.get("K", 3), pad, stride=what.get("stride", 1), dil=what.get("dil", 1), up1=up1,
                  xoff=what.get("xoff", 0), dtype=g.dtype)
    (fin1, def1, n1, rec1), (fin0, def0, n0, rec0) = res[1], res[0]
    assert (n1, n0) == (0, 0) and rec1 == rec0 and rec1["stage"] != w3.WGRAD3X3, (n1, n0, rec1, rec0)
    if case == "storage16":
        # no kernel takes fp32 tensors declared as 16-bit storage: the call is refused as it was, whatever the switch says
        assert rec1["stage"] == -1 and isinstance(fin1, str) and (fin1, def1) == (fin0, def0), (fin1, fin0)
        return
    assert rec1["stage"] == w3.MFMA, rec1
    _bits_equal(fin1, fin0, case + " finished")
    _bits_equal(def1, def0, case + " deferred")


def test_training_pass_and_graph_replay_on_equal_off(oracle_state):
    """The joint step of 2 patches of 64 x 64 (blind-spot DualNetwork, fp32: 8 rotated images, 512 tiles at full resolution)
    through GraphedTrainStep: the eager pass with the stage on and the HIP-graph replay captured with it on give the outputs
    and the flat gradient of the eager pass with it off.  The launches of the stage per pass are what the predicate says:
    counted from the records of the eager pass with the stage on (every backward-weight call whose record says stage 8)."""
    import ctypes

    from spr_pick_amd import Denoiser, _lib, graph_step
    from spr_pick_amd.params import PipelineOutput as P
    from test_gpu_pipeline import make_cfg
    L = _lib.lib()
    den = Denoiser(make_cfg(), device="cuda:0", mode="joint")
    den.load_state_dict({"models." + k: v for k, v in oracle_state.items()}, strict=False)
    den.train(); den.unfill()
    bn0 = {k: v.clone() for k, v in den.state_dict().items() if "running_" in k or "num_batches" in k}
    g = torch.Generator().manual_seed(31)
    inp = ((torch.rand(2, 1, 64, 64, generator=g) * 255).round() / 255).cuda()
    tgt = torch.tensor([[1.0], [-1.0]])
    st = graph_step.GraphedTrainStep(den, 2, 64, 0.75, 0.01, eager_warmup=1)
    keys = (P.LOSS, P.DENOISE_LOSS, P.DETECT, P.IMG_MU, P.IMG_DENOISED, P.NOISE_STD_DEV, P.MODEL_STD_DEV)

    # what the predicate says: the routes of the pass's backward-weight calls, asked again through sprk_conv2d_variant
    geoms = []
    real = L.sprk_conv2d_bwd_weight_partial, L.sprk_conv2d_bwd_weight

    def spy(fn):
        def f(*a):
            gm = a[4]._obj
            geoms.append((_lib.ConvGeom(*[getattr(gm, k) for k, _ in _lib.ConvGeom._fields_]), a[0], a[1], a[2]))
            return fn(*a)
        return f

    def run(eager):
        den.load_state_dict(bn0, strict=False)
        torch.cuda.manual_seed(4321)
        st.grads.flat.fill_(float("nan"))
        n0 = w3.launches()
        o = st(inp, tgt, flip_p=0.25, eager=eager)
        torch.cuda.synchronize()
        return ([o[k].detach().clone() for k in keys] + [st.grads.flat[:st.grads.live_numel].clone()], w3.launches() - n0)

    try:
        w3.switch(0)
        run(True)                      # the first pass finds the live parameters and compacts the gradient buffer
        off, n_off = run(True)
        w3.switch(1)
        L.sprk_conv2d_bwd_weight_partial, L.sprk_conv2d_bwd_weight = spy(real[0]), spy(real[1])
        try:
            on, n_on = run(True)
        finally:
            L.sprk_conv2d_bwd_weight_partial, L.sprk_conv2d_bwd_weight = real
        st.prepare(inp, tgt)
        assert st.fallback_reason is None
        replay, _ = run(False)
        want = 0
        for gm, x, x2, gy in geoms:
            out = (ctypes.c_int32 * 24)()
            assert L.sprk_conv2d_variant(2, ctypes.byref(gm), None, x, x2, gy, out) == 0
            want += out[0] == w3.WGRAD3X3
    finally:
        w3.switch(1)
    assert len(geoms) > 20 and (n_off, n_on) == (0, want), (n_off, n_on, want, len(geoms))
    assert not bool(torch.isnan(off[-1]).any())
    def bits(t):
        return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t

    for i, (a, b, c) in enumerate(zip(off, on, replay)):
        assert torch.equal(bits(a), bits(b)), "eager on against eager off: tensor %d differs (max |d| %.3e)" % (
            i, float((a - b).abs().max()))
        assert torch.equal(bits(a), bits(c)), "replay on against eager off: tensor %d differs (max |d| %.3e)" % (
            i, float((a - c).abs().max()))
