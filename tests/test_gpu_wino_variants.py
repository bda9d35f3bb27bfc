"""GPU: one convolution per reachable loop shape of the Winograd kernels (wino_conv_kernel<NT, SQ, UNROT> forward and
backward-data, wino_wgrad_kernel<MT> backward-weight; csrc/wino.hip), each against the fp64 CPU convolution at
tests/test_gpu_ops.py's budgets and against the plain per-output-element kernels, with proof of the variant that ran.

The cases are tests/golden/wino_variants.json, found by tests/wino_variant_cases.py --search on the CPU through
sprk_conv2d_variant; tests/test_wino_variants_cpu.py keeps that list complete.  Here sprk_conv2d_last_variant says
what each call actually launched: it must be the recorded variant, field by field.  x, x2 and gy are the inner slice
along N of a buffer whose first and last image are NaN, so a read that strays into a neighbouring image shows."""
import ctypes
import warnings

import pytest
import torch
import torch.nn.functional as F

import wino_variant_cases as wv
from test_gpu_ops import REL, close, dev, ref_conv

pytestmark = pytest.mark.gpu

GRAD_REL = 5e-5          # tests/test_gpu_ops.py: gradients, relative to the gradient's own scale
FX = wv.load()
CASES, EPILOGUES, UNROTS = FX["cases"], FX["epilogue_cases"], FX["unrot_cases"]


def last_variant(which):
    from spr_pick_amd import _lib
    out = (ctypes.c_int32 * 24)()
    assert _lib.lib().sprk_conv2d_last_variant(which, out) == 0
    return wv.as_dict(which, list(out))


def same_variant(name, what, ran, want):
    assert ran == want, "%s: %s launched\n  %s\nthe fixture records\n  %s" % (name, what, ran, want)


def run_conv(c, dtype, x, x2, w, b, gy):
    """ops.conv2d forward + backward of case c on guarded tensors -> y, (gx, gx2, gw, gb), the variants of the three calls"""
    from spr_pick_amd import ops
    d = dev()
    xd = wv.guarded(x, d).requires_grad_(True)
    x2d = wv.guarded(x2, d).requires_grad_(True) if x2 is not None else None
    wd = w.to(d).requires_grad_(True)
    bd = b.to(d).requires_grad_(True) if b is not None else None
    y = ops.conv2d(xd, wd, bd, x2=x2d, pad=tuple(c["pad"]), act=c["act"], dtype=dtype)
    ran = {"fwd": last_variant(0)}
    # the backward calls run on the autograd engine's thread and the record is per thread: read it there, from a hook on
    # the gradient of x, which fires once the node's backward (backward-weight, then backward-data) has returned
    xd.register_hook(lambda _g: ran.update(bwd=last_variant(1), wg=last_variant(2)))
    y.backward(wv.guarded(gy, d))
    torch.cuda.synchronize()
    grads = (xd.grad, None if x2d is None else x2d.grad, wd.grad, None if bd is None else bd.grad)
    return y.detach(), grads, ran


def conv_case(c):
    from spr_pick_amd import _lib
    name = c["name"]
    x, x2, w, b, gy = wv.tensors(c)
    y, grads, ran = run_conv(c, c["dtype"], x, x2, w, b, gy)
    for d in ("fwd", "bwd", "wg"):
        same_variant(name, d, ran[d], c["plan"][d])

    # fp64 CPU reference; the backward of (Leaky)ReLU uses the sign pattern of the GPU output (tests/test_gpu_ops.py)
    leaves = [t.double().requires_grad_(True) if t is not None else None for t in (x, x2, w, b)]
    args = (0, 1, 1, tuple(c["pad"]))
    pre = ref_conv(leaves[0], leaves[1], leaves[2], leaves[3], *args, 0)
    with torch.no_grad():
        want = ref_conv(leaves[0], leaves[1], leaves[2], leaves[3], *args, c["act"])
    close(y, want, rel=REL, name=name + " y")
    yr = torch.where(y.cpu() > 0, pre, pre * (0.1 if c["act"] == 1 else 0.0)) if c["act"] else pre
    yr.backward(gy.double())
    for got, leaf, what in zip(grads, leaves, ("gx", "gx2", "gw", "gb")):
        if leaf is not None:
            close(got, leaf.grad, rel=GRAD_REL, name="%s %s" % (name, what))

    # the same call on the plain per-output-element kernels: a disagreement above says which side is wrong
    y2, grads2, ran2 = run_conv(c, c["dtype"] | _lib.DT_NAIVE, x, x2, w, b, gy)
    assert [ran2[d]["stage"] for d in ("fwd", "bwd", "wg")] == [0, 0, 0], ran2
    close(y, y2, rel=REL, name=name + " y, Winograd against direct")
    # the two gradients are comparable where both runs applied the same activation mask; an output within rounding of
    # zero may land on either side (its backward then differs by design), which is said aloud, not passed over
    # (tests/test_gpu_conv_variants.py: the rule and its bound)
    flipped = int(((y > 0) != (y2 > 0)).sum()) if c["act"] else 0
    if flipped:
        assert flipped <= 1e-4 * y.numel() + 1, "%s: %d of %d activation signs differ between the two kernels" % (
            name, flipped, y.numel())
        warnings.warn("%s: %d of %d outputs change sign between the Winograd and the direct kernel; gradients compared "
                      "with fp64 only" % (name, flipped, y.numel()))
    else:
        for got, other, what in zip(grads, grads2, ("gx", "gx2", "gw", "gb")):
            if got is not None:
                close(got, other, rel=GRAD_REL, name="%s %s, Winograd against direct" % (name, what))


def wgrad_case(c):
    """the backward-weight entry called directly (no forward, no backward-data)"""
    from spr_pick_amd import _lib, torch_ops
    name = c["name"]
    x, x2, _, _, gy = wv.tensors(c)
    d = dev()
    xd, x2d, gyd = wv.guarded(x, d), None if x2 is None else wv.guarded(x2, d), wv.guarded(gy, d)
    shape = (c["Cout"], c["C1"] + c["C2"], 3, 3)
    gw = torch.full(shape, float("nan"), device=d)
    torch.ops.sprk.conv2d_bwd_weight(xd, x2d, gyd, torch_ops.geom_list(wv.case_geom(c)), gw, False)
    same_variant(name, "wg", last_variant(2), c["plan"]["wg"])
    want = wv.ref_wgrad(x.double(), None if x2 is None else x2.double(), gy.double(), c["pad"])
    close(gw, want, rel=GRAD_REL, name=name + " gw")
    gw2 = torch.full(shape, float("nan"), device=d)
    torch.ops.sprk.conv2d_bwd_weight(xd, x2d, gyd, torch_ops.geom_list(wv.case_geom(c, c["dtype"] | _lib.DT_NAIVE)), gw2, False)
    assert last_variant(2)["stage"] == 0
    close(gw, gw2, rel=GRAD_REL, name=name + " gw, Winograd against direct")


def fwd_case(c):
    """the forward entry called directly (pads whose backward calls leave the Winograd stage)"""
    from spr_pick_amd import _lib, ops
    name = c["name"]
    x, x2, w, b, _ = wv.tensors(c)
    d = dev()
    xd, x2d, wd = wv.guarded(x, d), None if x2 is None else wv.guarded(x2, d), w.to(d)
    bd = None if b is None else b.to(d)
    pad = tuple(c["pad"])

    def run(dtype):
        geom = ops.make_geom(xd, x2d, wd, False, 1, 1, pad, dtype=dtype)
        return ops.conv2d_forward(xd, x2d, wd, geom, bias=bd, act=c["act"])

    y = run(c["dtype"])
    same_variant(name, "fwd", last_variant(0), c["plan"]["fwd"])
    want = ref_conv(x.double(), None if x2 is None else x2.double(), w.double(), None if b is None else b.double(), 0, 1, 1, pad,
                    c["act"])
    close(y, want, rel=REL, name=name + " y")
    y2 = run(c["dtype"] | _lib.DT_NAIVE)
    assert last_variant(0)["stage"] == 0
    close(y, y2, rel=REL, name=name + " y, Winograd against direct")


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_wino_variant(case):
    {"wgrad": wgrad_case, "fwd": fwd_case, "conv": conv_case}[case["kind"]](case)


# ---- the epilogue forms ----------------------------------------------------------------------------------------------
def _affine(c, g):
    scale, shift = torch.rand(c["Cout"], generator=g) + 0.5, torch.randn(c["Cout"], generator=g)
    return scale, shift


def _act64(y, act):
    return F.leaky_relu(y, 0.1) if act == 1 else F.relu(y) if act == 2 else y


@pytest.mark.parametrize("case", EPILOGUES, ids=[c["name"] for c in EPILOGUES])
def test_wino_epilogue(case):
    """plain / up2: the forward call with act x (bias | scale + shift | neither); mask: the backward-data call with the
    activation backward of the layer's producer in its store (ops.conv2d(x_act=...), as the conv -> conv chains of
    tests/test_gpu_ops.py reach it)"""
    from spr_pick_amd import _lib, ops
    c = case
    name = c["name"]
    d = dev()
    g = torch.Generator().manual_seed(wv.seed_of(name))
    pad = tuple(c["pad"])
    if c["mode"] == "mask":
        # the layer Cout -> few channels: its backward-data is the Winograd call with the partly filled last group
        C, K = c["Cout"], c["C1"] + c["C2"] + 3
        x = torch.randn(c["N"], C, c["H"], c["W"], generator=g)          # "the saved output of the producer": both signs
        w = torch.randn(K, C, 3, 3, generator=g) / (3 * C ** 0.5)
        gy = torch.randn(c["N"], K, c["H"], c["W"], generator=g)
        ran = {}

        def run(dtype):
            xd, wd = wv.guarded(x, d).requires_grad_(True), w.to(d).requires_grad_(True)
            y = ops.conv2d(xd, wd, None, pad=pad, act=0, dtype=dtype, x_act=c["mact"])
            xd.register_hook(lambda _g: ran.update(bwd=last_variant(1)))
            y.backward(wv.guarded(gy, d))
            torch.cuda.synchronize()
            return xd.grad

        gx = run(c["dtype"])
        same_variant(name, "bwd", ran["bwd"], c["plan"])
        xr = x.double().requires_grad_(True)
        ref_conv(xr, None, w.double(), None, 0, 1, 1, pad, 0).backward(gy.double())
        slope = 0.1 if c["mact"] == 1 else 0.0
        want = xr.grad * torch.where(x > 0, 1.0, slope).double()
        close(gx, want, rel=GRAD_REL, name=name + " masked gx")
        gx2 = run(c["dtype"] | _lib.DT_NAIVE)
        assert ran["bwd"]["stage"] == 0
        close(gx, gx2, rel=GRAD_REL, name=name + " masked gx, Winograd against direct")
        return

    x, x2, w, _, _ = wv.tensors(c)
    b = torch.randn(c["Cout"], generator=g) * 0.1 if c["ep"] == "bias" else None
    scale, shift = _affine(c, g) if c["ep"] == "affine" else (None, None)
    up = c["mode"] == "up2"
    xd, x2d, wd = wv.guarded(x, d), None if x2 is None else wv.guarded(x2, d), w.to(d)
    on = lambda t: None if t is None else t.to(d)

    def run(dtype):
        geom = ops.make_geom(xd, x2d, wd, False, 1, 1, pad, dtype=dtype)
        return ops.conv2d_forward(xd, x2d, wd, geom, bias=on(b), act=c["act"], scale=on(scale), shift=on(shift), up_out=up)

    y = run(c["dtype"])
    same_variant(name, "fwd", last_variant(0), c["plan"])
    pre = ref_conv(x.double(), None if x2 is None else x2.double(), w.double(), None if b is None else b.double(), 0, 1, 1, pad, 0)
    if scale is not None:
        pre = pre * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    want = _act64(pre, c["act"])
    if up:
        want = F.interpolate(want, scale_factor=2, mode="nearest")
    close(y, want, rel=REL, name=name + " y")
    y2 = run(c["dtype"] | _lib.DT_NAIVE)
    assert last_variant(0)["stage"] == 0
    close(y, y2, rel=REL, name=name + " y, Winograd against direct")


# ---- the un-rotated store --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", UNROTS, ids=[u["name"] for u in UNROTS])
def test_wino_unrot_store(case):
    """bit-identical to the convolution followed by the un-rotation operator, every element of f written by the one
    launch, and the un-rotated result against the fp64 statement of the layer (tests/test_gpu_unrot_train.py)"""
    from spr_pick_amd import ops
    PAD = wv.UNROT_PAD
    u = case
    B, C1, C2, Cout = u["B"], u["C1"], u["C2"], u["Cout"]
    c = dict(name=u["name"], N=4 * B, C1=C1, C2=C2, H=64, W=64, Cout=Cout, bias=True)
    x, x2, w, b, _ = wv.tensors(c)
    d = dev()
    xd, x2d, wd, bd = wv.guarded(x, d), None if x2 is None else wv.guarded(x2, d), w.to(d), b.to(d)
    with torch.enable_grad():
        assert ops.unrot_store_eligible(xd, wd, bd, PAD, ops.ACT_LEAKY, x2=x2d)
    with torch.no_grad():
        geom = ops.make_geom(xd, x2d, wd, False, 1, 1, PAD)
        want = ops.unrot4_shift_concat(ops.conv2d_forward(xd, x2d, wd, geom, bias=bd, act=ops.ACT_LEAKY))
        # the allocator hands the next tensor of this size the block freed here: NaNs wherever the kernel does not write
        poison = torch.full_like(want, float("nan"))
        del poison
        got = ops.conv2d_forward(xd, x2d, wd, geom, bias=bd, act=ops.ACT_LEAKY, unrot=True)
        torch.cuda.synchronize()
    same_variant(u["name"], "fwd", last_variant(0), u["plan"])
    assert not bool(torch.isnan(got).any()), "the fused store left elements of f unwritten"
    assert torch.equal(got, want), "max |d| %.3e at %d elements" % (float((got - want).abs().max()), int((got != want).sum()))
    assert wv.zero_lines(got) and float(got.abs().max()) > 0
    xin = x.double() if x2 is None else torch.cat((x.double(), x2.double()), 1)
    pre, unrot = wv.ref_unrot_layer(xin, w.double(), b.double())
    close(got, unrot(F.leaky_relu(pre, 0.1)), rel=REL, name=u["name"] + " f")
