"""GPU: one convolution per reachable variant of the fp32 MFMA kernels (conv_mfma_kernel<MT, NT, RB, XTAB> forward and
backward-data, conv_wgrad_mfma_kernel<IT, NT, WJ, MODE> backward-weight, and both values of their run-time flags), each
against the fp64 CPU convolution at tests/test_gpu_ops.py's budgets, with proof of the variant that ran.

The cases are tests/golden/conv_variants.json, found by tests/conv_variant_cases.py --search on the CPU through
sprk_conv2d_variant; tests/test_conv_variants_cpu.py keeps that list complete.  Here sprk_conv2d_last_variant says
what each of the three calls of ops.conv2d actually launched: it must be the recorded variant, field by field."""
import ctypes
import warnings

import pytest
import torch

import conv_variant_cases as cv
from test_gpu_ops import REL, close, dev, ref_conv

pytestmark = pytest.mark.gpu

GRAD_REL = 5e-5          # tests/test_gpu_ops.py: gradients, relative to the gradient's own scale
CASES = cv.load()["cases"]


def last_variant(which):
    from spr_pick_amd import _lib
    out = (ctypes.c_int32 * 24)()
    assert _lib.lib().sprk_conv2d_last_variant(which, out) == 0
    return cv.as_dict(which, list(out))


def run(c, dtype, x, x2, w, b, gy):
    """ops.conv2d forward + backward of case c on tensors with the case's alignment offsets -> y, (gx, gx2, gw, gb), and
    the variants the three calls launched"""
    from spr_pick_amd import ops
    d = dev()
    off = c["off"]
    xd = cv.float_offset(x, off["x"], d).requires_grad_(True)
    x2d = cv.float_offset(x2, off["x2"], d).requires_grad_(True) if x2 is not None else None
    wd = w.to(d).requires_grad_(True)
    bd = b.to(d).requires_grad_(True) if b is not None else None
    y = ops.conv2d(xd, wd, bd, x2=x2d, up1=bool(c["up1"]), stride=c["stride"], dil=c["dil"], pad=tuple(c["pad"]),
                   act=c["act"], dtype=dtype)
    ran = {"fwd": last_variant(0)}
    # the backward calls run on the autograd engine's thread and the record is per thread: read it there, from a hook on
    # the gradient of x, which fires once the node's backward (backward-weight, then backward-data) has returned
    xd.register_hook(lambda _g: ran.update(bwd=last_variant(1), wg=last_variant(2)))
    y.backward(cv.float_offset(gy, cv.gy_offset(c), d))
    torch.cuda.synchronize()
    grads = (xd.grad, None if x2d is None else x2d.grad, wd.grad, None if bd is None else bd.grad)
    return y.detach(), grads, ran


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_conv_variant(case):
    from spr_pick_amd import _lib
    c = case
    x, x2, w, b, gy = cv.tensors(c)
    y, grads, ran = run(c, 0, x, x2, w, b, gy)

    # the kernel under test ran: exactly the recorded variant in each direction (another CU count re-plans: both shown)
    for d in ("fwd", "bwd", "wg"):
        assert ran[d] == c["plan"][d], "%s: %s launched\n  %s\nthe fixture records\n  %s\n(sprk_conv2d_variant on this device: %s)" % (
            c["name"], d, ran[d], c["plan"][d], cv.planned(c)[d])

    # fp64 CPU reference; the backward of (Leaky)ReLU uses the sign pattern of the GPU output (tests/test_gpu_ops.py)
    leaves = [t.double().requires_grad_(True) if t is not None else None for t in (x, x2, w, b)]
    args = (c["up1"], c["stride"], c["dil"], tuple(c["pad"]))
    pre = ref_conv(leaves[0], leaves[1], leaves[2], leaves[3], *args, 0)
    with torch.no_grad():
        want = ref_conv(leaves[0], leaves[1], leaves[2], leaves[3], *args, c["act"])
    name = c["name"]
    close(y, want, rel=REL, name=name + " y")
    yr = torch.where(y.cpu() > 0, pre, pre * (0.1 if c["act"] == 1 else 0.0)) if c["act"] else pre
    yr.backward(gy.double())
    for got, leaf, what in zip(grads, leaves, ("gx", "gx2", "gw", "gb")):
        if leaf is not None:
            close(got, leaf.grad, rel=GRAD_REL, name="%s %s" % (name, what))

    # the same call on the plain per-output-element kernels: a disagreement above says which side is wrong
    y2, grads2, ran2 = run(c, _lib.DT_NAIVE, x, x2, w, b, gy)
    assert [ran2[d]["stage"] for d in ("fwd", "bwd", "wg")] == [0, 0, 0], ran2
    close(y, y2, rel=REL, name=name + " y, MFMA against direct")
    # the two gradients are comparable where both runs applied the same activation mask; an output within rounding of
    # zero may land on either side (its backward then differs by design), which is said aloud, not passed over
    # (a flip needs |pre-activation| below the kernels' disagreement, at most REL of the scale, itself 4-5 sigma of a
    # near-normal output: a share of about 2 * REL * 5 * 0.4 = 8e-5 of the elements at the very most)
    flipped = int(((y > 0) != (y2 > 0)).sum()) if c["act"] else 0
    if flipped:
        assert flipped <= 1e-4 * y.numel() + 1, "%s: %d of %d activation signs differ between the two kernels" % (
            name, flipped, y.numel())
        warnings.warn("%s: %d of %d outputs change sign between the MFMA and the direct kernel; gradients compared with "
                      "fp64 only" % (name, flipped, y.numel()))
    else:
        for got, other, what in zip(grads, grads2, ("gx", "gx2", "gw", "gb")):
            if got is not None:
                close(got, other, rel=GRAD_REL, name="%s %s, MFMA against direct" % (name, what))
