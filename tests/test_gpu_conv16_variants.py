"""GPU: one convolution per reachable loop shape of the 16-bit kernels (conv16_mfma_kernel, conv16_tile_kernel,
conv16_head_kernel forward and backward-data, csrc/conv16.hip; wgrad16_kernel, wgrad16_1x1_kernel backward-weight,
csrc/wgrad16.hip), each against the exact model of tests/test_gpu_ops.py (test_conv2d_16bit_operands /
test_conv2d_16bit_storage: an fp64 CPU convolution of operands rounded on the CPU by torch casts) at those tests' own
budgets, with proof of the variant that ran.

The cases are tests/golden/conv16_variants.json, found by tests/conv16_variant_cases.py --search on the CPU through
sprk_conv2d_variant; tests/test_conv16_variants_cpu.py keeps that list complete.  Here sprk_conv2d_last_variant says
what each call actually launched: it must be the recorded variant, field by field, and the launch counters must have
moved by the 16-bit calls of the case.  Tensors have the storage types of the case.  x, x2 and gy are the inner slice
along N of a buffer whose outer images are NaN, so a read that strays into a neighbouring image shows.  No element is
left out of a comparison: the activation mask of the reference is the device's own y."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv16_variant_cases as cv
from test_gpu_ops import dev

pytestmark = pytest.mark.gpu

FX = cv.load()
CASES, EPILOGUES = FX["cases"], FX["epilogue_cases"]
S16 = cv.S16


def last_variant(which):
    from spr_pick_amd import _lib
    out = (ctypes.c_int32 * 24)()
    assert _lib.lib().sprk_conv2d_last_variant(which, out) == 0
    return cv.as_dict(which, list(out))


def same_variant(name, what, ran, want):
    assert ran == want, "%s: %s launched\n  %s\nthe fixture records\n  %s" % (name, what, ran, want)


def within(name, what, got, ref, bud):
    """every element of ``got`` within its budget of ``ref`` (cv.budget); the figure is printed before it is asserted"""
    assert got.shape == ref.shape, (name, what, got.shape, ref.shape)
    got = got.detach().cpu()
    assert bool(torch.isfinite(got.float()).all()), "%s: %s is not finite" % (name, what)
    r = cv.ratio(got, ref, bud)
    print("%s: %s worst error / budget %.3f" % (name, what, r))
    assert r <= 1.0, "%s: %s beyond the budget: worst ratio %.3f" % (name, what, r)


def one_of_four(name, yv):
    """an up-sampled output is four identical copies of y, bit for bit (NaN included: no element escapes) -> y"""
    q = [yv[:, :, i::2, j::2].contiguous().view(torch.int16 if yv.element_size() == 2 else torch.int32) for i in (0, 1) for j in (0, 1)]
    assert all(torch.equal(q[0], o) for o in q[1:]), name + ": the four copies of an up-sampled output differ"
    return yv[:, :, 0::2, 0::2]


def counters():
    from spr_pick_amd import _lib
    L = _lib.lib()
    return L.sprk_conv16_launch_count(), L.sprk_wgrad16_launch_count()


def conv_case(c):
    """ops.conv2d forward (kind "fwd": that alone) and backward"""
    from spr_pick_amd import _lib, ops
    name, plan = c["name"], c["plan"]
    t16 = cv.torch_type(c["dt"])
    x, x2, w, b, gy = cv.tensors(c)
    d = dev()
    store = (lambda t: t.to(t16)) if c["x16"] else (lambda t: t)
    grad = c["kind"] == "conv"
    xd = cv.guarded(store(x), d).requires_grad_(grad)
    x2d = cv.guarded(store(x2), d).requires_grad_(grad) if x2 is not None else None
    wd = w.to(d).requires_grad_(grad)
    bd = b.to(d).requires_grad_(grad) if b is not None else None
    n0, w0 = counters()
    with torch.set_grad_enabled(grad):
        y = ops.conv2d(xd, wd, bd, x2=x2d, pad=tuple(c["pad"]), act=c["act"], up_out=c["up_out"], dtype=cv.base_dtype(c),
                       store16=bool(c["y16"]))
    ran = {"fwd": last_variant(0)}
    same_variant(name, "fwd", ran["fwd"], plan["fwd"])
    assert y.dtype == (t16 if c["y16"] else torch.float32)
    assert counters() == (n0 + 1, w0), "%s: the forward call did not launch one 16-bit kernel" % name
    yv = y.detach().cpu()
    if c["up_out"]:
        yv = one_of_four(name, yv)
    within(name, "y", yv, cv.model_forward(c, x, x2, w, b, torch.float64), cv.budget(c, "y", plan))
    if not grad:
        return

    # the backward calls run on the autograd engine's thread and the record is per thread: read it there, from a hook on
    # the gradient of x, which fires once the node's backward (backward-weight, then backward-data) has returned
    xd.register_hook(lambda _g: ran.update(bwd=last_variant(1), wg=last_variant(2)))
    gyd = cv.guarded(gy.to(y.dtype), d)
    y.backward(gyd)
    torch.cuda.synchronize()
    same_variant(name, "bwd", ran["bwd"], plan["bwd"])
    same_variant(name, "wg", ran["wg"], plan["wg"])
    wg16 = int(plan["wg"]["stage"] == S16)
    assert counters() == (n0 + 2 + wg16, w0 + wg16), "%s: the launch counters after backward" % name
    assert xd.grad.dtype == xd.dtype and (x2d is None or x2d.grad.dtype == x2d.dtype)
    gpre, g16 = cv.model_gpre(c, yv, gy)
    gin = cv.model_gin(c, w, g16, torch.float64)
    gx = xd.grad.detach().cpu()
    got = gx if x2d is None else torch.cat((gx, x2d.grad.detach().cpu()), 1)
    within(name, "gin", got, gin, cv.budget(c, "gin", plan))
    if wg16:
        within(name, "gw", wd.grad, cv.model_gw(c, x, x2, g16, torch.float64), cv.budget(c, "gw", plan))
    else:
        # the small layers' backward-weight stays on the fp32 kernels: the unrounded fp64 statement at 8 u, as
        # test_conv2d_16bit_operands holds it
        xs = store(x).double() if c["x16"] else x.double()
        x2s = None if x2 is None else (store(x2).double() if c["x16"] else x2.double())
        gsrc = g16 if (c["x16"] or c["y16"]) else gpre
        xin = xs if x2s is None else torch.cat((xs, x2s), 1)
        pt, pb, pl, pr = c["pad"]
        ref = torch.nn.grad.conv2d_weight(F.pad(xin, (pl, pr, pt, pb)), tuple(w.shape), gsrc)
        within(name, "gw (fp32 kernels)", wd.grad, ref, cv.budget(c, "gw", plan))
    if b is not None:
        within(name, "gb", bd.grad, gpre.sum((0, 2, 3)), cv.budget(c, "gb", plan))


def wgrad_case(c):
    """the backward-weight entry called directly (no forward, no backward-data)"""
    from spr_pick_amd import torch_ops
    name = c["name"]
    t16 = cv.torch_type(c["dt"])
    x, x2, _, _, gy = cv.tensors(c)
    d = dev()
    store = (lambda t: t.to(t16)) if c["x16"] else (lambda t: t)
    xd, x2d, gyd = cv.guarded(store(x), d), None if x2 is None else cv.guarded(store(x2), d), cv.guarded(store(gy), d)
    gw = torch.full((c["Cout"], c["C1"] + c["C2"], c["K"], c["K"]), float("nan"), device=d)
    n0, w0 = counters()
    torch.ops.sprk.conv2d_bwd_weight(xd, x2d, gyd, torch_ops.geom_list(cv.case_geom(c, cv.call_dtypes(c)["wg"])), gw, False)
    same_variant(name, "wg", last_variant(2), c["plan"]["wg"])
    assert counters() == (n0 + 1, w0 + 1), "%s: the call did not launch one 16-bit backward-weight kernel" % name
    within(name, "gw", gw, cv.model_gw(c, x, x2, gy.to(t16).double(), torch.float64), (0.0, 1e-4))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_conv16_variant(case):
    (wgrad_case if case["kind"] == "wgrad" else conv_case)(case)


_EP_REF = {}


def _epilogue_reference(c):
    """x, x2, w of an epilogue case and the fp64 convolution of their rounded values: computed once per geometry and
    shared, unchanged, among its forms (the forms differ in the per-channel constants and the activation alone)"""
    if c["seed"] not in _EP_REF:
        x, x2, w, _, _ = cv.tensors(c)
        r = lambda v: None if v is None else v.to(cv.torch_type(c["dt"])).double()
        _EP_REF[c["seed"]] = (x, x2, w, cv.ref_conv(r(x), r(x2), r(w), None, c["pad"], c["K"]))
    return _EP_REF[c["seed"]]


@pytest.mark.parametrize("case", EPILOGUES, ids=[e["name"] for e in EPILOGUES])
def test_conv16_epilogue(case):
    """the forward call with act x (bias | scale + shift | neither) x up2, fp32 and 16-bit tensors"""
    from spr_pick_amd import ops
    c = case
    name = c["name"]
    t16 = cv.torch_type(c["dt"])
    d = dev()
    g = torch.Generator().manual_seed(cv.seed_of(name))
    x, x2, w, pre0 = _epilogue_reference(c)
    b = torch.randn(c["Cout"], generator=g) * 0.1 if c["ep"] == "bias" else None
    scale = torch.rand(c["Cout"], generator=g) + 0.5 if c["ep"] == "affine" else None
    shift = torch.randn(c["Cout"], generator=g) if c["ep"] == "affine" else None
    store = (lambda t: t.to(t16)) if c["x16"] else (lambda t: t)
    xd, x2d, wd = cv.guarded(store(x), d), None if x2 is None else cv.guarded(store(x2), d), w.to(d)
    on = lambda t: None if t is None else t.to(d)
    geom = ops.make_geom(xd, x2d, wd, False, 1, 1, tuple(c["pad"]), dtype=cv.call_dtypes(c)["fwd"])
    n0, w0 = counters()
    y = ops.conv2d_forward(xd, x2d, wd, geom, bias=on(b), act=c["act"], scale=on(scale), shift=on(shift), up_out=c["up_out"])
    same_variant(name, "fwd", last_variant(0), c["plan"])
    assert counters() == (n0 + 1, w0) and y.dtype == (t16 if c["y16"] else torch.float32)
    pre = pre0 if b is None else pre0 + b.double().view(1, -1, 1, 1)
    if scale is not None:
        pre = pre * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    yv = y.detach().cpu()
    if c["up_out"]:
        yv = one_of_four(name, yv)
    within(name, "y", yv, cv.act_fn(c["act"])(pre), cv.budget(c, "y", None))
