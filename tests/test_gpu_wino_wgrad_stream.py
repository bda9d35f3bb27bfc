"""The Winograd backward-weight on wino_wgrad_stream_kernel (csrc/wino.hip).

The calls wino_wgrad takes run the same launches (MT, groups, parts, source, XCD order) on a kernel with the operand reads
rebuilt: the same regions in the same order, the same operands, one v_mfma_f32_16x16x4_f32 per k-step into every
accumulator, the same final transform and reduction.  So every comparison is bit for bit (int32 views: -0 and +0 are told
apart) between the call with the kernel on (sprk_wino_wgrad_stream_enable(1): sprk_wino_wgrad_stream_launch_count advances by
1 per call) and off (wino_wgrad_kernel, which tests/test_gpu_wino_variants.py holds to fp64; counter still);
sprk_wino_launch_count advances either way and the variant record is the same.  x, x2 and gy are the inner slice along N of
buffers whose first and last image are NaN; they hold zeros of both signs, input channel 0 is -0 and gradient channel 1 +0
everywhere.  Shapes: tests/wino_wgrad_stream_cases.py."""
import ctypes

import pytest
import torch

import wino_variant_cases as wv
import wino_wgrad_stream_cases as ws
from test_gpu_ops import dev

pytestmark = pytest.mark.gpu


def _bits_equal(a, b, what):
    assert not bool(torch.isnan(a).any()), "%s: elements left unwritten or read from a neighbouring image (NaN)" % what
    assert a.shape == b.shape
    same = torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    assert same, "%s: %d elements differ between the two kernels (max |d| %.3e)" % (
        what, int((a != b).sum()), float((a - b).abs().max()))


def _guarded(shape, g, d, zero_channel):
    """random values with zeros of both signs and one channel of signed zeros, as the inner slice of a NaN-framed buffer"""
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), float("nan"), device=d)
    v = buf[1:-1]
    v.normal_(generator=g)
    r = torch.rand(shape, generator=g, device=d)
    v[r < 0.02] = 0.0
    v[r > 0.98] = -0.0
    v[:, zero_channel[0]] = zero_channel[1]
    assert v.is_contiguous() and v.data_ptr() % 16 == 0
    return v


def _last_variant():
    from spr_pick_amd import _lib
    out = (ctypes.c_int32 * 24)()
    assert _lib.lib().sprk_conv2d_last_variant(2, out) == 0
    return wv.as_dict(2, list(out))


@pytest.mark.parametrize("case", list(ws.CASES))
def test_on_equals_off(case):
    from spr_pick_amd import torch_ops
    N, C1, C2, Cout, H, W, pad, carries = ws.CASES[case]
    d = dev()
    g = torch.Generator(device=d).manual_seed(wv.seed_of(case))
    x = _guarded((N, C1, H, W), g, d, (0, -0.0))
    x2 = _guarded((N, C2, H, W), g, d, (C2 - 1, -0.0)) if C2 else None
    gy = _guarded((N, Cout, H, W), g, d, (1, 0.0))
    geom = ws.geom_of(N, C1, C2, Cout, H, W, pad)
    plan = wv.as_dict(2, wv.query(2, geom))
    assert plan["stage"] == ws.WINO and (plan["padT"], plan["padL"]) == pad, plan
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert (plan["cx"] != 0, plan["cy"] != 0) == (carries, carries), plan
    res = {}
    try:
        for on in (1, 0):
            ws.switch(on)
            s0, w0 = ws.launches()
            gw = torch.full((Cout, C1 + C2, 3, 3), float("nan"), device=d)
            torch.ops.sprk.conv2d_bwd_weight(x, x2, gy, torch_ops.geom_list(geom), gw, False)
            torch.cuda.synchronize()
            s1, w1 = ws.launches()
            res[on] = (gw, s1 - s0, w1 - w0, _last_variant())
    finally:
        ws.switch(1)
    (gw1, ns1, nw1, rec1), (gw0, ns0, nw0, rec0) = res[1], res[0]
    assert (ns1, nw1, ns0, nw0) == (1, 1, 0, 1), (ns1, nw1, ns0, nw0)
    assert rec1 == rec0 == plan, (rec1, rec0, plan)
    _bits_equal(gw1, gw0, case)


def test_training_pass_and_graph_replay_on_equal_off(oracle_state):
    """The joint step of 16 patches of 64 x 64 (blind-spot DualNetwork, fp32) through GraphedTrainStep, the smallest batch at
    which the 64 x 64 decoder layers reach the Winograd backward-weight: the eager pass with the kernel on and the HIP-graph
    replay captured with it on give the outputs and the flat gradient of the eager pass with it off.  The kernel's calls per
    pass are the backward-weight calls whose route sprk_conv2d_variant reports as the Winograd stage."""
    from spr_pick_amd import Denoiser, _lib, graph_step
    from spr_pick_amd.params import PipelineOutput as P
    from test_gpu_pipeline import make_cfg
    L = _lib.lib()
    B = 16
    den = Denoiser(make_cfg(), device="cuda:0", mode="joint")
    den.load_state_dict({"models." + k: v for k, v in oracle_state.items()}, strict=False)
    den.train(); den.unfill()
    bn0 = {k: v.clone() for k, v in den.state_dict().items() if "running_" in k or "num_batches" in k}
    g = torch.Generator().manual_seed(37)
    inp = ((torch.rand(B, 1, 64, 64, generator=g) * 255).round() / 255).cuda()
    tgt = torch.tensor([[1.0], [-1.0]] * (B // 2))
    st = graph_step.GraphedTrainStep(den, B, 64, 0.75, 0.01, eager_warmup=1)
    keys = (P.LOSS, P.DENOISE_LOSS, P.DETECT, P.IMG_MU, P.IMG_DENOISED, P.NOISE_STD_DEV, P.MODEL_STD_DEV)

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
        n0 = ws.launches()[0]
        o = st(inp, tgt, flip_p=0.25, eager=eager)
        torch.cuda.synchronize()
        return ([o[k].detach().clone() for k in keys] + [st.grads.flat[:st.grads.live_numel].clone()], ws.launches()[0] - n0)

    try:
        ws.switch(0)
        run(True)                      # the first pass finds the live parameters and compacts the gradient buffer
        off, n_off = run(True)
        ws.switch(1)
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
            want += out[0] == ws.WINO
    finally:
        ws.switch(1)
    assert len(geoms) > 20 and want >= 1 and (n_off, n_on) == (0, want), (n_off, n_on, want, len(geoms))
    assert not bool(torch.isnan(off[-1]).any())

    def bits(t):
        return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t

    for i, (a, b, c) in enumerate(zip(off, on, replay)):
        assert torch.equal(bits(a), bits(b)), "eager on against eager off: tensor %d differs (max |d| %.3e)" % (
            i, float((a - b).abs().max()))
        assert torch.equal(bits(a), bits(c)), "replay on against eager off: tensor %d differs (max |d| %.3e)" % (
            i, float((a - c).abs().max()))
