"""``torch.ops.sprk.*``: the libsprk.so entry points registered as PyTorch custom operators (torch.library).

One operator per C-ABI function of include/sprk.h, schema-typed, with a CUDA implementation (the ctypes call on
torch's current stream of the tensors' device) and a fake / meta implementation (output shapes only), so the
dispatcher, ``torch.library.opcheck``-style tooling, FakeTensor tracing and CUDA-graph capture all see them as ordinary
operators.  Autograd is NOT registered here: ops.py's ``autograd.Function`` classes call these operators in their
forward and backward (the backward kernels are operators too), which keeps a single place for the saved-tensor policy.
There is no CPU implementation — dispatching a CPU tensor raises — and a missing libsprk.so raises at first use.

Geometry travels as the 16 integers of ``sprk_conv_geom`` (``ConvGeom`` field order: N, C1, C2, Hin, Win, up1, Cout,
Hout, Wout, KH, KW, stride, dil, pad_top, pad_left, dtype).
"""
import ctypes

import torch

from . import _lib
from ._lib import ConvEpilogue, ConvGeom, check

_LIB = torch.library.Library("sprk", "DEF")
_NAMES = []


def _stream(t):
    """torch's current stream on the device that holds ``t`` (a kernel must be enqueued on a stream of the
    device its pointers live on).  One process drives one GPU here; a tensor on another device than the
    process's current one is a set-up error and raises instead of launching on the wrong card."""
    dev = t.device
    if dev.index is not None and dev.index != torch.cuda.current_device():
        raise _lib.SprkError("tensor on %s but the current device is cuda:%d — call torch.cuda.set_device(%d) "
                             "(Denoiser / DenoiserTrainer / DenoiserEvaluator do it for their own device)"
                             % (dev, torch.cuda.current_device(), dev.index))
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ws(nbytes, like):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=like.device)


def _f32(like, shape):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


# storage types of activation tensors: SPRK_DT_* codes <-> torch dtypes (include/sprk.h: SPRK_IO2 / SPRK_IO3)
TORCH_OF = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
CODE_OF = {v: k for k, v in TORCH_OF.items()}


def code(t):
    c = CODE_OF.get(t.dtype)
    if c is None:
        raise _lib.SprkError("activation tensors are float32, bfloat16 or float16 (got %s)" % t.dtype)
    return c


def _alloc(like, shape, c):
    return torch.empty(shape, dtype=TORCH_OF[c], device=like.device)


def _out_code(geom_dtype):
    """storage type of a convolution call's output tensor: the operand type with SPRK_DT_Y16, else fp32"""
    return (geom_dtype & 0xff) if (geom_dtype & _lib.DT_Y16) else 0


def _register(name, schema, impl, fake):
    _LIB.define(name + schema)
    _LIB.impl(name, impl, "CUDA")
    torch.library.register_fake("sprk::" + name, fake, lib=_LIB)
    _NAMES.append(name)


def geom_list(g):
    return [getattr(g, f) for f, _ in ConvGeom._fields_]


# ---- convolution -----------------------------------------------------------------------------------------------------
def _epilogue(bias, scale, shift, res, res_off, act, up_out):
    return ConvEpilogue(_p(bias), _p(scale), _p(shift), _p(res), 0 if res is None else res.shape[2],
                        0 if res is None else res.shape[3], res_off, act, 1 if up_out else 0)


def _conv2d_fwd(x, x2, w, bias, scale, shift, res, geom, res_off, act, up_out, ws):
    """ws: a caller-owned workspace (prepared weights, ops.WeightPrep) or None = a fresh one."""
    L = _lib.lib()
    g = ConvGeom(*geom)
    m = 2 if up_out else 1
    y = _alloc(x, (g.N, g.Cout, g.Hout * m, g.Wout * m), _out_code(g.dtype))
    ep = _epilogue(bias, scale, shift, res, res_off, act, up_out)
    if ws is None:
        ws = _ws(L.sprk_conv2d_fwd_ws_bytes(ctypes.byref(g)), x)
    check(L.sprk_conv2d_fwd(_p(x), _p(x2), _p(w), _p(y), ctypes.byref(g), ctypes.byref(ep), _p(ws), ws.numel(), _stream(x)),
          "sprk_conv2d_fwd")
    return y


def _conv2d_fwd_unrot(x, x2, w, bias, geom, act, ws):
    """The convolution of a 4-rotation stack whose kernel stores the un-rotated tensor: -> f [N/4, 4*Cout, P, P]
    (sprk_conv2d_fwd_unrot; the caller asked sprk_conv2d_fwd_unrot_eligible)."""
    L = _lib.lib()
    g = ConvGeom(*geom)
    f = _f32(x, (g.N // 4, 4 * g.Cout, g.Hout, g.Wout))
    ep = _epilogue(bias, None, None, None, 0, act, False)
    if ws is None:
        ws = _ws(L.sprk_conv2d_fwd_ws_bytes(ctypes.byref(g)), x)
    check(L.sprk_conv2d_fwd_unrot(_p(x), _p(x2), _p(w), _p(f), ctypes.byref(g), ctypes.byref(ep), _p(ws), ws.numel(), _stream(x)),
          "sprk_conv2d_fwd_unrot")
    return f


_register("conv2d_fwd_unrot", "(Tensor x, Tensor? x2, Tensor w, Tensor? bias, int[] geom, int act, Tensor? ws) -> Tensor",
          _conv2d_fwd_unrot,
          lambda x, x2, w, bias, geom, act, ws: x.new_empty((geom[0] // 4, 4 * geom[6], geom[7], geom[8])))


def _conv2d_fwd_fake(x, x2, w, bias, scale, shift, res, geom, res_off, act, up_out, ws):
    m = 2 if up_out else 1
    return x.new_empty((geom[0], geom[6], geom[7] * m, geom[8] * m), dtype=TORCH_OF[_out_code(geom[15])])


_register("conv2d_fwd", "(Tensor x, Tensor? x2, Tensor w, Tensor? bias, Tensor? scale, Tensor? shift, Tensor? res, "
                        "int[] geom, int res_off, int act, int up_out, Tensor? ws) -> Tensor", _conv2d_fwd, _conv2d_fwd_fake)


def _conv2d_bwd_data(gy, w, geom, mask_y, mask_act, ws):
    """mask_y / mask_act: fuse the activation backward of the layer that produced this convolution's input (the saved
    input itself is the mask): the result is that layer's pre-activation gradient (sprk_conv2d_bwd_data_masked).
    ws: a caller-owned workspace (prepared weights) or None."""
    L = _lib.lib()
    g = ConvGeom(*geom)
    gin = _alloc(gy, (g.N, g.C1 + g.C2, g.Hin, g.Win), _out_code(g.dtype))
    if ws is None:
        ws = _ws(L.sprk_conv2d_bwd_data_ws_bytes(ctypes.byref(g)), gy)
    if mask_y is not None and mask_y.dtype != gin.dtype:
        raise _lib.SprkError("conv2d_bwd_data: the mask (%s) must have the storage type of the input gradient (%s)" % (
            mask_y.dtype, gin.dtype))
    if mask_y is not None and tuple(mask_y.shape) != tuple(gin.shape):
        raise _lib.SprkError("conv2d_bwd_data: mask %s does not match the input gradient %s" % (tuple(mask_y.shape), tuple(gin.shape)))
    check(L.sprk_conv2d_bwd_data_masked(_p(gy), _p(w), _p(gin), ctypes.byref(g), _p(mask_y), int(mask_act) if mask_y is not None else 0,
                                        _p(ws), ws.numel(), _stream(gy)), "sprk_conv2d_bwd_data_masked")
    return gin


_register("conv2d_bwd_data", "(Tensor gy, Tensor w, int[] geom, Tensor? mask_y, int mask_act, Tensor? ws) -> Tensor",
          _conv2d_bwd_data,
          lambda gy, w, geom, mask_y, mask_act, ws: gy.new_empty((geom[0], geom[1] + geom[2], geom[3], geom[4]),
                                                                  dtype=TORCH_OF[_out_code(geom[15])]))


def _head1x1_fwd(f, w1, b1, w2, b2, w3, b3):
    """Fused per-pixel head (inference): [B,K0,H,W] -> [B,N3,H,W] (sprk_head1x1_fwd)."""
    L = _lib.lib()
    B, K0, H, W = f.shape
    N1, N3 = w1.shape[0], w3.shape[0]
    out = _f32(f, (B, N3, H, W))
    nb = L.sprk_head1x1_fwd_ws_bytes(K0, N1)
    if nb == 0:
        raise _lib.SprkError("head1x1_fwd: no fused kernel for %d -> %d" % (K0, N1))
    ws = _ws(nb, f)
    check(L.sprk_head1x1_fwd(_p(f), _p(w1), _p(b1), _p(w2), _p(b2), _p(w3), _p(b3), _p(out), B, K0, N1, N3, H * W, _p(ws), nb,
                             _stream(f)), "sprk_head1x1_fwd")
    return out


_register("head1x1_fwd", "(Tensor f, Tensor w1, Tensor b1, Tensor w2, Tensor b2, Tensor w3, Tensor b3) -> Tensor", _head1x1_fwd,
          lambda f, w1, b1, w2, b2, w3, b3: f.new_empty((f.shape[0], w3.shape[0], f.shape[2], f.shape[3])))


def _head1x1_unrot_fwd(d, w1, b1, w2, b2, w3, b3):
    """Blind-spot head on the rotated stack: d [4B,96,P,P] -> [B,N3,P,P] (sprk_head1x1_unrot_fwd)."""
    L = _lib.lib()
    B4, C, P, P2 = d.shape
    if B4 % 4 or P != P2:
        raise _lib.SprkError("head1x1_unrot_fwd: bad shape %s" % (tuple(d.shape),))
    N3 = w3.shape[0]
    out = _f32(d, (B4 // 4, N3, P, P))
    nb = L.sprk_head1x1_fwd_ws_bytes(384, 384)
    ws = _ws(nb, d)
    check(L.sprk_head1x1_unrot_fwd(_p(d), _p(w1), _p(b1), _p(w2), _p(b2), _p(w3), _p(b3), _p(out), B4 // 4, C, P, N3, _p(ws), nb,
                                   _stream(d)), "sprk_head1x1_unrot_fwd")
    return out


_register("head1x1_unrot_fwd", "(Tensor d, Tensor w1, Tensor b1, Tensor w2, Tensor b2, Tensor w3, Tensor b3) -> Tensor",
          _head1x1_unrot_fwd,
          lambda d, w1, b1, w2, b2, w3, b3: d.new_empty((d.shape[0] // 4, w3.shape[0], d.shape[2], d.shape[3])))


# Pending second-stage sums (sprk_reduce_items): with defer=True the backward-weight / bias-gradient operators run only
# their main kernel, and the ~80 small sums of a training step are finished together by ``reduce_pending``.  An entry
# keeps its partial buffer alive until then; the destination must be kept alive by the caller (ops defers only
# gradients that live in graph_step.FlatGrads' buffer).
_PENDING = {}


def _pend(dev, item, *keep):
    if item.kind != 0:
        _PENDING.setdefault(dev.index, []).append((item, keep))


def pending_count(dev):
    return len(_PENDING.get(dev.index, ()))


def _conv2d_bwd_weight(x, x2, gy, geom, gw, defer):
    """Out variant: writes into ``gw`` (a fresh tensor or the parameter's slice of the flat gradient buffer).
    defer: leave the sum over the workgroups' partial results to ``reduce_pending`` (gw is undefined until then)."""
    L = _lib.lib()
    g = ConvGeom(*geom)
    nb = L.sprk_conv2d_bwd_weight_ws_bytes(ctypes.byref(g))
    ws = _ws(nb, gy)
    if defer:
        item = _lib.ReduceItem()
        check(L.sprk_conv2d_bwd_weight_partial(_p(x), _p(x2), _p(gy), _p(gw), ctypes.byref(g), _p(ws), nb, ctypes.byref(item),
                                               _stream(x)), "sprk_conv2d_bwd_weight_partial")
        _pend(gy.device, item, ws)     # not gw: autograd adopts a gradient tensor only while nobody else holds it
        return
    check(L.sprk_conv2d_bwd_weight(_p(x), _p(x2), _p(gy), _p(gw), ctypes.byref(g), _p(ws), nb, _stream(x)),
          "sprk_conv2d_bwd_weight")


_register("conv2d_bwd_weight", "(Tensor x, Tensor? x2, Tensor gy, int[] geom, Tensor(a!) gw, bool defer) -> ()",
          _conv2d_bwd_weight, lambda x, x2, gy, geom, gw, defer: None)


def _reduce_pending(like):
    """Finish every pending sum of ``like``'s device in one launch per 48 items."""
    items = _PENDING.pop(like.device.index, [])
    if not items:
        return
    arr = (_lib.ReduceItem * len(items))(*[it for it, _ in items])
    check(_lib.lib().sprk_reduce_items(arr, len(items), _stream(like)), "sprk_reduce_items")


_register("reduce_pending", "(Tensor like) -> ()", _reduce_pending, lambda like: None)


def drop_pending(dev):
    """Forget pending sums without running them (error paths)."""
    _PENDING.pop(dev.index, None)


def _act_bwd(gy, y, act, geom4, up2, want_gpre, gbias, defer, out_code):
    """gpre = gy * act'(y) (2x2-summed first when up2); bias gradient into ``gbias`` when given (defer: its final
    sum is left to ``reduce_pending``).  Returns gpre (or gy itself when no new tensor is needed).  out_code: storage
    type of gpre (SPRK_DT_*; gy, y and gpre may each be fp32 or the 16-bit type)."""
    L = _lib.lib()
    N, C, H, W = geom4
    gpre = _alloc(gy, (N, C, H, W), out_code) if want_gpre else None
    io = code(gy) | ((code(y) if y is not None else 0) << 4) | ((out_code if want_gpre else code(gy)) << 8)
    # gy may be a channel slice of a wider tensor (dense planes, a larger stride between images): read in place
    gstride = 0
    if not gy.is_contiguous():
        if want_gpre and gy.dim() == 4 and gy[0].is_contiguous() and gy.stride(0) >= gy[0].numel():
            gstride = gy.stride(0)
        else:
            gy = gy.contiguous()
    nb = L.sprk_act_bwd_ws_bytes(N, C, H * W)
    ws = _ws(nb, gy)
    if defer and gbias is not None:
        item = _lib.ReduceItem()
        check(L.sprk_act_bwd_partial(_p(gy), _p(y), _p(gpre), _p(gbias), act, N, C, H, W, up2, gstride, io, _p(ws), nb,
                                     ctypes.byref(item), _stream(gy)), "sprk_act_bwd_partial")
        _pend(gy.device, item, ws)
    else:
        check(L.sprk_act_bwd(_p(gy), _p(y), _p(gpre), _p(gbias), act, N, C, H, W, up2, gstride, io, _p(ws), nb, _stream(gy)),
              "sprk_act_bwd")
    return gpre if want_gpre else gy.new_empty(0)


_register("act_bwd", "(Tensor gy, Tensor? y, int act, int[] nchw, int up2, bool want_gpre, Tensor(a!)? gbias, bool defer, "
                     "int out_code) -> Tensor", _act_bwd,
          lambda gy, y, act, nchw, up2, want_gpre, gbias, defer, out_code: gy.new_empty(
              tuple(nchw) if want_gpre else (0,), dtype=TORCH_OF[out_code] if want_gpre else gy.dtype))


def _unrot_act_bwd(gf, f, act, gbias, defer):
    """Un-rotation backward + activation backward in one pass (sprk_unrot_act_bwd): gf, f [B,4C,P,P] -> gpre [4B,C,P,P];
    bias gradient into ``gbias`` when given (defer: its final sum is left to ``reduce_pending``)."""
    L = _lib.lib()
    B, C4, P, P2 = gf.shape
    if C4 % 4 or P != P2 or tuple(f.shape) != tuple(gf.shape) or gf.dtype != torch.float32 or f.dtype != torch.float32:
        raise _lib.SprkError("unrot_act_bwd: bad tensors %s %s / %s %s" % (tuple(gf.shape), gf.dtype, tuple(f.shape), f.dtype))
    C = C4 // 4
    gpre = _f32(gf, (4 * B, C, P, P))
    nb = L.sprk_act_bwd_ws_bytes(4 * B, C, P * P)
    ws = _ws(nb, gf)
    item = _lib.ReduceItem() if (defer and gbias is not None) else None
    check(L.sprk_unrot_act_bwd(_p(gf), _p(f), _p(gpre), _p(gbias), act, B, C, P, _p(ws), nb,
                               ctypes.byref(item) if item is not None else None, _stream(gf)), "sprk_unrot_act_bwd")
    if item is not None:
        _pend(gf.device, item, ws)
    return gpre


_register("unrot_act_bwd", "(Tensor gf, Tensor f, int act, Tensor(a!)? gbias, bool defer) -> Tensor", _unrot_act_bwd,
          lambda gf, f, act, gbias, defer: gf.new_empty((4 * gf.shape[0], gf.shape[1] // 4, gf.shape[2], gf.shape[3])))


def _concat_up_bwd(gin, C1, C2, up1, x_shape, x2_shape):
    L = _lib.lib()
    N, _, H, W = gin.shape
    gx = _f32(gin, tuple(x_shape))
    gx2 = _f32(gin, tuple(x2_shape)) if C2 else gin.new_empty(0)
    check(L.sprk_concat_up_bwd(_p(gin), _p(gx), _p(gx2) if C2 else None, N, C1, C2, H, W, up1, _stream(gin)),
          "sprk_concat_up_bwd")
    return gx, gx2


_register("concat_up_bwd", "(Tensor gin, int C1, int C2, int up1, int[] x_shape, int[] x2_shape) -> (Tensor, Tensor)",
          _concat_up_bwd, lambda gin, C1, C2, up1, xs, x2s: (gin.new_empty(tuple(xs)), gin.new_empty(tuple(x2s) if C2 else (0,))))


# ---- U-Net plumbing ----------------------------------------------------------------------------------------------------
def _typed(name, schema, cfn, out_shape, out_dtype, args):
    """Register an operator whose C function takes (inputs..., output, ints..., stream): out_shape(*a), out_dtype(*a) ->
    shape and torch dtype of the output (the operators whose tensors may be fp32 or 16-bit), args(a, y) -> C arguments
    incl. the io word."""
    def impl(*a):
        L = _lib.lib()
        tensors = [t for t in a if torch.is_tensor(t)]
        y = torch.empty(out_shape(*a), dtype=out_dtype(*a), device=tensors[0].device)
        check(getattr(L, cfn)(*args(a, y), _stream(tensors[0])), cfn)
        return y
    _register(name, schema, impl, lambda *a: [t for t in a if torch.is_tensor(t)][0].new_empty(out_shape(*a), dtype=out_dtype(*a)))


def _simple(name, schema, cfn, out_shape, args):
    """_typed with an fp32 output."""
    _typed(name, schema, cfn, out_shape, lambda *a: torch.float32, args)


_typed("shift_maxpool2_fwd", "(Tensor x, int shift) -> Tensor", "sprk_shift_maxpool2_fwd",
       lambda x, shift: (x.shape[0], x.shape[1], x.shape[2] // 2, x.shape[3] // 2), lambda x, shift: x.dtype,
       lambda a, y: (_p(a[0]), _p(y), a[0].shape[0] * a[0].shape[1], a[0].shape[2], a[0].shape[3], a[1],
                     code(a[0]) | (code(y) << 4)))
_typed("shift_maxpool2_bwd", "(Tensor gy, Tensor x, int shift, int act) -> Tensor", "sprk_shift_maxpool2_bwd",
       lambda gy, x, shift, act: tuple(x.shape), lambda gy, x, shift, act: x.dtype,
       lambda a, y: (_p(a[0]), _p(a[1]), _p(y), a[1].shape[0] * a[1].shape[1], a[1].shape[2], a[1].shape[3], a[2], a[3],
                     code(a[0]) | (code(a[1]) << 4) | (code(y) << 8)))
_simple("rot4_stack_fwd", "(Tensor x) -> Tensor", "sprk_rot4_stack_fwd",
        lambda x: (4 * x.shape[0], x.shape[1], x.shape[2], x.shape[3]),
        lambda a, y: (_p(a[0]), _p(y), a[0].shape[0], a[0].shape[1], a[0].shape[2]))
_simple("rot4_stack_bwd", "(Tensor gy) -> Tensor", "sprk_rot4_stack_bwd",
        lambda gy: (gy.shape[0] // 4, gy.shape[1], gy.shape[2], gy.shape[3]),
        lambda a, y: (_p(a[0]), _p(y), a[0].shape[0] // 4, a[0].shape[1], a[0].shape[2]))
_typed("unrot4_shift_concat_fwd", "(Tensor d) -> Tensor", "sprk_unrot4_shift_concat_fwd",
       lambda d: (d.shape[0] // 4, 4 * d.shape[1], d.shape[2], d.shape[3]), lambda d: d.dtype,
       lambda a, y: (_p(a[0]), _p(y), a[0].shape[0] // 4, a[0].shape[1], a[0].shape[2], code(a[0]) | (code(y) << 4)))
_typed("unrot4_shift_concat_bwd", "(Tensor gf) -> Tensor", "sprk_unrot4_shift_concat_bwd",
       lambda gf: (4 * gf.shape[0], gf.shape[1] // 4, gf.shape[2], gf.shape[3]), lambda gf: gf.dtype,
       lambda a, y: (_p(a[0]), _p(y), a[0].shape[0], a[0].shape[1] // 4, a[0].shape[2], code(a[0]) | (code(y) << 4)))

# ---- per-pixel pipeline maths ----------------------------------------------------------------------------------------------
_simple("reparam_fwd", "(Tensor out_stats, Tensor eps) -> Tensor", "sprk_reparam_fwd",
        lambda o, e: (o.shape[0], 1, o.shape[2], o.shape[3]),
        lambda a, y: (_p(a[0]), _p(a[1]), _p(y), a[0].shape[0], a[0].shape[2] * a[0].shape[3]))
_simple("reparam_bwd", "(Tensor gz, Tensor out_stats, Tensor eps) -> Tensor", "sprk_reparam_bwd",
        lambda gz, o, e: tuple(o.shape),
        lambda a, y: (_p(a[0]), _p(a[1]), _p(a[2]), _p(y), a[1].shape[0], a[1].shape[2] * a[1].shape[3]))
_simple("sigmoid_clamp_fwd", "(Tensor x) -> Tensor", "sprk_sigmoid_clamp_fwd", lambda x: tuple(x.shape),
        lambda a, y: (_p(a[0]), _p(y), a[0].numel()))
_simple("sigmoid_clamp_bwd", "(Tensor gp, Tensor x) -> Tensor", "sprk_sigmoid_clamp_bwd", lambda gp, x: tuple(x.shape),
        lambda a, y: (_p(a[0]), _p(a[1]), _p(y), a[1].numel()))


# ---- fused pieces of the training step's tail (include/sprk.h, ABI 410) ---------------------------------------------------
def _crop_shape(x, off, stride, out_h, out_w):
    return (x.shape[0], x.shape[1], out_h, out_w)


def _crop_add(y, x, off, stride, out_h, out_w):
    out = _f32(x, _crop_shape(x, off, stride, out_h, out_w))
    check(_lib.lib().sprk_crop_add_fwd(_p(y), _p(x), _p(out), x.shape[0] * x.shape[1], out_h, out_w, x.shape[2], x.shape[3],
                                       off, stride, _stream(x)), "sprk_crop_add_fwd")
    return out


_register("crop_add_fwd", "(Tensor? y, Tensor x, int off, int stride, int out_h, int out_w) -> Tensor", _crop_add,
          lambda y, x, off, stride, out_h, out_w: x.new_empty(_crop_shape(x, off, stride, out_h, out_w)))
_simple("crop_embed_bwd", "(Tensor g, int off, int stride, int hx, int wx) -> Tensor", "sprk_crop_embed_bwd",
        lambda g, off, stride, hx, wx: (g.shape[0], g.shape[1], hx, wx),
        lambda a, y: (_p(a[0]), _p(y), a[0].shape[0] * a[0].shape[1], a[0].shape[2], a[0].shape[3], a[3], a[4], a[1], a[2]))


def _noise_std_fwd(est):
    B, HW = est.shape[0], est[0].numel()
    out, z = _f32(est, (B, 1, 1, 1)), _f32(est, (B,))
    check(_lib.lib().sprk_noise_std_fwd(_p(est), _p(out), _p(z), B, HW, _stream(est)), "sprk_noise_std_fwd")
    return out, z


_register("noise_std_fwd", "(Tensor est) -> (Tensor, Tensor)", _noise_std_fwd,
          lambda est: (est.new_empty((est.shape[0], 1, 1, 1)), est.new_empty((est.shape[0],))))
_simple("noise_std_bwd", "(Tensor g, Tensor z, int c, int h, int w) -> Tensor", "sprk_noise_std_bwd",
        lambda g, z, c, h, w: (z.shape[0], c, h, w),
        lambda a, y: (_p(a[0]), _p(a[1]), _p(y), a[1].shape[0], a[2] * a[3] * a[4]))


def _joint_loss_fwd(loss_out, pred, p, pf, axis, alpha, wc):
    B, H, W = p.shape[0], p.shape[2], p.shape[3]
    final, consis = _f32(p, (B, 1)), _f32(p, (1,))
    check(_lib.lib().sprk_joint_loss_fwd(_p(loss_out), _p(pred), _p(p), _p(pf), _p(final), _p(consis), B, H, W, axis,
                                         ctypes.c_float(alpha), ctypes.c_float(wc), _stream(p)), "sprk_joint_loss_fwd")
    return final, consis


def _joint_loss_bwd(g, p, pf, axis, alpha, wc):
    B, H, W = p.shape[0], p.shape[2], p.shape[3]
    gl, gpred, gp, gpf = _f32(p, (B, 1)), _f32(p, (1,)), _f32(p, tuple(p.shape)), _f32(p, tuple(p.shape))
    check(_lib.lib().sprk_joint_loss_bwd(_p(g), _p(p), _p(pf), _p(gl), _p(gpred), _p(gp), _p(gpf), B, H, W, axis,
                                         ctypes.c_float(alpha), ctypes.c_float(wc), _stream(p)), "sprk_joint_loss_bwd")
    return gl, gpred, gp, gpf


_register("joint_loss_fwd", "(Tensor loss_out, Tensor pred, Tensor p, Tensor pf, int axis, float alpha, float wc) -> (Tensor, Tensor)",
          _joint_loss_fwd, lambda lo, pred, p, pf, axis, alpha, wc: (p.new_empty((p.shape[0], 1)), p.new_empty((1,))))
_register("joint_loss_bwd", "(Tensor g, Tensor p, Tensor pf, int axis, float alpha, float wc) -> (Tensor, Tensor, Tensor, Tensor)",
          _joint_loss_bwd, lambda g, p, pf, axis, alpha, wc: (p.new_empty((p.shape[0], 1)), p.new_empty((1,)),
                                                             p.new_empty(p.shape), p.new_empty(p.shape)))


def _pu_loss(p, y, log_binom, slack):
    """-> (loss [1], d loss / d p [B]) in one launch."""
    B = p.numel()
    if log_binom.shape != (B + 1, B + 1) or y.numel() != B:
        raise ValueError("pu_loss: table %s / labels %d do not match %d scores" % (tuple(log_binom.shape), y.numel(), B))
    loss, gp = _f32(p, (1,)), _f32(p, (B,))
    check(_lib.lib().sprk_pu_loss(_p(p), _p(y), _p(log_binom), B, ctypes.c_float(slack), _p(loss), _p(gp), _stream(p)),
          "sprk_pu_loss")
    return loss, gp


_register("pu_loss", "(Tensor p, Tensor y, Tensor log_binom, float slack) -> (Tensor, Tensor)", _pu_loss,
          lambda p, y, t, slack: (p.new_empty((1,)), p.new_empty((p.numel(),))))


def _ssdn_fwd(x, out_stats, noise_std, style):
    """-> (loss [B,1], pme [B,1,H,W], model_std [1,B,H,W], noise_std_map [B,H,W] (poisson) or empty (gaussian))"""
    L = _lib.lib()
    B, _, H, W = out_stats.shape
    loss, pme, mstd = _f32(x, (B, 1)), _f32(x, (B, 1, H, W)), _f32(x, (1, B, H, W))
    nsmap = _f32(x, (B, H, W)) if style == 1 else _f32(x, (0,))
    nb = L.sprk_ssdn_ws_bytes(B, H * W)
    ws = _ws(nb, x)
    check(L.sprk_ssdn_fwd(_p(x), _p(out_stats), _p(noise_std), _p(loss), _p(pme), _p(mstd), _p(nsmap) if style == 1 else None,
                          int(style), B, H * W, _p(ws), nb, _stream(x)), "sprk_ssdn_fwd")
    return loss, pme, mstd, nsmap


def _ssdn_fwd_fake(x, out_stats, noise_std, style):
    B, _, H, W = out_stats.shape
    return (x.new_empty((B, 1)), x.new_empty((B, 1, H, W)), x.new_empty((1, B, H, W)),
            x.new_empty((B, H, W) if style == 1 else (0,)))


_register("ssdn_fwd", "(Tensor x, Tensor out_stats, Tensor noise_std, int style) -> (Tensor, Tensor, Tensor, Tensor)", _ssdn_fwd,
          _ssdn_fwd_fake)


def _ssdn_bwd(gloss, x, out_stats, noise_std, style):
    L = _lib.lib()
    B, _, H, W = out_stats.shape
    go, gns = torch.empty_like(out_stats), _f32(x, (B,))
    nb = L.sprk_ssdn_ws_bytes(B, H * W)
    ws = _ws(nb, x)
    check(L.sprk_ssdn_bwd(_p(gloss), _p(x), _p(out_stats), _p(noise_std), _p(go), _p(gns), int(style), B, H * W, _p(ws), nb,
                          _stream(x)), "sprk_ssdn_bwd")
    return go, gns


_register("ssdn_bwd", "(Tensor gloss, Tensor x, Tensor out_stats, Tensor noise_std, int style) -> (Tensor, Tensor)", _ssdn_bwd,
          lambda gl, x, o, ns, style: (torch.empty_like(o), x.new_empty((o.shape[0],))))


# ---- BatchNorm -----------------------------------------------------------------------------------------------------------
def _bn_eval_fwd(x, gamma, beta, running_mean, running_var, eps, relu):
    N, C, H, W = x.shape
    y = torch.empty_like(x)
    check(_lib.lib().sprk_bn_eval_fwd(_p(x), _p(y), _p(gamma), _p(beta), _p(running_mean), _p(running_var), N, C, H * W,
                                      float(eps), int(relu), _stream(x)), "sprk_bn_eval_fwd")
    return y


_register("bn_eval_fwd", "(Tensor x, Tensor gamma, Tensor beta, Tensor running_mean, Tensor running_var, float eps, "
                         "bool relu) -> Tensor", _bn_eval_fwd, lambda x, *a: torch.empty_like(x))


def _bn_train_fwd(x, gamma, beta, running_mean, running_var, momentum, eps, relu, groups):
    """`groups` passes stacked along N, each with its own batch statistics: returns (y, save_mean [groups, C],
    save_invstd [groups, C]); updates the running statistics in place, group after group."""
    L = _lib.lib()
    N, C, H, W = x.shape
    y, mean, invstd = torch.empty_like(x), _f32(x, (groups, C)), _f32(x, (groups, C))
    nb = L.sprk_bn_ws_bytes(N, C, H * W, groups)
    ws = _ws(nb, x)
    check(L.sprk_bn_train_fwd(_p(x), _p(y), _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(mean), _p(invstd),
                              N, C, H * W, groups, momentum, eps, int(relu), _p(ws), nb, _stream(x)), "sprk_bn_train_fwd")
    return y, mean, invstd


_register("bn_train_fwd", "(Tensor x, Tensor gamma, Tensor beta, Tensor(a!) running_mean, Tensor(b!) running_var, "
                          "float momentum, float eps, bool relu, int groups) -> (Tensor, Tensor, Tensor)", _bn_train_fwd,
          lambda x, g, b, rm, rv, mo, eps, relu, groups: (torch.empty_like(x), g.new_empty((groups,) + tuple(g.shape)),
                                                         g.new_empty((groups,) + tuple(g.shape))))


def _bn_train_bwd(gy, x, y, gamma, mean, invstd, relu, groups, ggamma, gbeta):
    L = _lib.lib()
    N, C, H, W = x.shape
    gx = torch.empty_like(x)
    nb = L.sprk_bn_ws_bytes(N, C, H * W, groups)
    ws = _ws(nb, x)
    check(L.sprk_bn_train_bwd(_p(gy), _p(x), _p(y), _p(gamma), _p(mean), _p(invstd), _p(gx), _p(ggamma), _p(gbeta),
                              N, C, H * W, groups, int(relu), _p(ws), nb, _stream(x)), "sprk_bn_train_bwd")
    return gx


_register("bn_train_bwd", "(Tensor gy, Tensor x, Tensor y, Tensor gamma, Tensor mean, Tensor invstd, bool relu, "
                          "int groups, Tensor(a!) ggamma, Tensor(b!) gbeta) -> Tensor", _bn_train_bwd,
          lambda gy, x, *a: torch.empty_like(x))


# ---- NMS (one relaxation call; algorithms.nms_device drives the fixed point) -------------------------------------------------
def _nms2d(score, r, threshold, out_s, out_xy, cnt, rounds, resume, ws):
    H, W = score.shape
    check(_lib.lib().sprk_nms2d(_p(score), H, W, int(r), ctypes.c_float(threshold), _p(out_s), _p(out_xy), _p(cnt),
                                out_s.shape[0], rounds, resume, _p(ws), ws.numel(), _stream(score)), "sprk_nms2d")


_register("nms2d", "(Tensor score, int r, float threshold, Tensor(a!) out_s, Tensor(b!) out_xy, Tensor(c!) cnt, "
                   "int rounds, int resume, Tensor(d!) ws) -> ()", _nms2d, lambda *a: None)


# ---- contamination mask (algorithms.contamination_mask / find_contamination) -----------------------------------------------
def _contam_mask(img, crop, ksize, k_low, k_high, radius, set_bitmap, stats):
    L = _lib.lib()
    H, W = img.shape
    mask = torch.empty((H, W), dtype=torch.uint8, device=img.device)
    ws = _ws(L.sprk_contam_ws_bytes(H, W), img)
    check(L.sprk_contam_mask(_p(img), H, W, int(crop), int(ksize), float(k_low), float(k_high), int(radius), _p(mask),
                             _p(set_bitmap), _p(stats), _p(ws), ws.numel(), _stream(img)), "sprk_contam_mask")
    return mask


_register("contam_mask", "(Tensor img, int crop, int ksize, float k_low, float k_high, int radius, Tensor(a!)? set_bitmap, "
                         "Tensor(b!) stats) -> Tensor", _contam_mask,
          lambda img, *a: img.new_empty(tuple(img.shape), dtype=torch.uint8))


# ---- micrograph ingest (ingest.py: raw MRC samples -> binned image -> uint8 image / network input) ---------------------------
MRC_ITEMSIZE = {0: 1, 1: 2, 2: 4, 6: 2}          # bytes per sample of the MRC modes sprk_ingest_bin decodes
INGEST_MAX_BIN = 16                              # SPRK_INGEST_MAX_BIN


def _up4(n):
    return -(-int(n) // 4) * 4


def _up16(n):
    return -(-int(n) // 16) * 16


def crop_matrix_shape(B, S):
    """-> the shape of the operand that holds an [S, B] crop or shift matrix: [roundup(S, 16), roundup(B, 4)]"""
    return _up16(S), _up4(B)


# the operand checks that the operators below share: ``who`` is the operator's name, ``like`` the tensor whose device counts
def _mode_check(who, mode):
    if mode not in MRC_ITEMSIZE:
        raise _lib.SprkError("%s: unsupported MRC mode %d" % (who, mode))


def _raw_check(who, raw, mode, ny, nx, contiguous=False):
    """after ``_mode_check``, which every operator makes first"""
    if (raw.dtype != torch.uint8 or raw.dim() != 1 or (contiguous and not raw.is_contiguous())
            or raw.numel() < ny * nx * MRC_ITEMSIZE[mode]):
        raise _lib.SprkError("%s: raw must be a flat uint8 tensor of at least ny*nx samples (%d bytes), got %s %s"
                             % (who, ny * nx * MRC_ITEMSIZE[mode], raw.dtype, tuple(raw.shape)))


def _range_check(who, rng, like):
    if rng.dtype != torch.float32 or rng.numel() != 2 or not rng.is_contiguous() or rng.device != like.device:
        raise _lib.SprkError("%s: range must be a contiguous float32 tensor of 2 elements on %s, got %s %s on %s"
                             % (who, like.device, rng.dtype, tuple(rng.shape), rng.device))


def _xy_check(who, xy, like):
    if xy.dtype != torch.int32 or xy.dim() != 2 or xy.shape[1] != 2 or xy.device != like.device:
        raise _lib.SprkError("%s: xy must be an int32 tensor [P, 2] on %s, got %s %s on %s"
                             % (who, like.device, xy.dtype, tuple(xy.shape), xy.device))


def _matrix_check(who, name, m, shape, like, of=None):
    """m: float32 of ``shape`` on the device of ``like``; ``of``: what builds it ("matrix of ingest.resample_matrix(...)")"""
    if m.dtype != torch.float32 or tuple(m.shape) != tuple(shape) or m.device != like.device:
        what = "float32 [%d, %d]" % tuple(shape) if of is None else "the float32 %s, [%d, %d]" % (of, *shape)
        raise _lib.SprkError("%s: %s must be %s on %s, got %s %s on %s"
                             % (who, name, what, like.device, m.dtype, tuple(m.shape), m.device))


def _binned_shape(mode, ny, nx, bin):
    _mode_check("ingest_bin", mode)
    if not 1 <= bin <= INGEST_MAX_BIN or ny // bin < 1 or nx // bin < 1:
        raise _lib.SprkError("ingest_bin: bin factor %d on a %dx%d image (1..%d, at least one block)"
                             % (bin, ny, nx, INGEST_MAX_BIN))
    return ny // bin, nx // bin


def net_size(by, bx):
    """side of the network input of a [by, bx] image: both axes rounded up to a multiple of 32, then squared"""
    return max((by + 31) // 32 * 32, (bx + 31) // 32 * 32)


def _ingest_bin(raw, mode, ny, nx, bin):
    """raw: uint8 CUDA tensor holding the file's ny*nx samples -> (binned float32 [by, bx], range float32 [2])."""
    by, bx = _binned_shape(mode, ny, nx, bin)
    _raw_check("ingest_bin", raw, mode, ny, nx, contiguous=True)
    L = _lib.lib()
    binned, rng = _f32(raw, (by, bx)), _f32(raw, (2,))
    ws = _ws(L.sprk_ingest_ws_bytes(ny, nx, bin), raw)
    check(L.sprk_ingest_bin(_p(raw), int(mode), int(ny), int(nx), int(bin), _p(binned), _p(rng), _p(ws), ws.numel(),
                            _stream(raw)), "sprk_ingest_bin")
    return binned, rng


_register("ingest_bin", "(Tensor raw, int mode, int ny, int nx, int bin) -> (Tensor, Tensor)", _ingest_bin,
          lambda raw, mode, ny, nx, bin: (raw.new_empty(_binned_shape(mode, ny, nx, bin), dtype=torch.float32),
                                          raw.new_empty((2,), dtype=torch.float32)))


def _finish_shapes(binned, want_u8, want_net):
    if binned.dim() != 2 or binned.dtype != torch.float32:
        raise _lib.SprkError("ingest_finish: binned must be a 2-D float32 tensor, got %s %s" % (binned.dtype, tuple(binned.shape)))
    by, bx = binned.shape
    S = net_size(by, bx)
    return ((by, bx) if want_u8 else (0, 0)), ((S, S) if want_net else (0, 0))


def _ingest_finish(binned, rng, want_u8, want_net):
    """-> (u8 [by, bx], net float32 [S, S]); the one that is not asked for is an empty tensor."""
    if not (want_u8 or want_net):
        raise _lib.SprkError("ingest_finish: neither output asked for")
    su, sn = _finish_shapes(binned, want_u8, want_net)
    _range_check("ingest_finish", rng, binned)
    binned = binned.contiguous()
    u8 = torch.empty(su, dtype=torch.uint8, device=binned.device)
    net = _f32(binned, sn)
    by, bx = binned.shape
    check(_lib.lib().sprk_ingest_finish(_p(binned), by, bx, _p(rng), _p(u8) if want_u8 else None,
                                        _p(net) if want_net else None, sn[0], _stream(binned)), "sprk_ingest_finish")
    return u8, net


def _ingest_finish_fake(binned, rng, want_u8, want_net):
    su, sn = _finish_shapes(binned, want_u8, want_net)
    return binned.new_empty(su, dtype=torch.uint8), binned.new_empty(sn, dtype=torch.float32)


_register("ingest_finish", "(Tensor binned, Tensor range, bool want_u8, bool want_net) -> (Tensor, Tensor)", _ingest_finish,
          _ingest_finish_fake)


def _clip_check(binned, rng, k_lo, k_hi):
    if binned.dim() != 2 or binned.dtype != torch.float32 or binned.numel() < 1:
        raise _lib.SprkError("ingest_clip: binned must be a non-empty 2-D float32 tensor, got %s %s"
                             % (binned.dtype, tuple(binned.shape)))
    _range_check("ingest_clip", rng, binned)
    if not 0 <= k_lo <= k_hi <= binned.numel() - 1:
        raise _lib.SprkError("ingest_clip: ranks %d, %d of %d elements (0 <= k_lo <= k_hi <= n-1)"
                             % (k_lo, k_hi, binned.numel()))


def _ingest_clip(binned, rng, k_lo, k_hi):
    """-> (binned clamped to its k_lo-th and k_hi-th smallest elements, float32 [by, bx]; range float32 [2] = the two
    elements).  Functional: neither argument is written."""
    _clip_check(binned, rng, k_lo, k_hi)
    binned = binned.contiguous()
    by, bx = binned.shape
    L = _lib.lib()
    out, rng_out = _f32(binned, (by, bx)), _f32(binned, (2,))
    ws = _ws(L.sprk_ingest_clip_ws_bytes(by, bx), binned)
    check(L.sprk_ingest_clip(_p(binned), _p(out), by, bx, int(k_lo), int(k_hi), _p(rng), _p(rng_out), _p(ws), ws.numel(),
                             _stream(binned)), "sprk_ingest_clip")
    return out, rng_out


def _ingest_clip_fake(binned, rng, k_lo, k_hi):
    _clip_check(binned, rng, k_lo, k_hi)
    return binned.new_empty(tuple(binned.shape), dtype=torch.float32), binned.new_empty((2,), dtype=torch.float32)


_register("ingest_clip", "(Tensor binned, Tensor range, int k_lo, int k_hi) -> (Tensor, Tensor)", _ingest_clip,
          _ingest_clip_fake)

INGEST_MAX_FLATTEN = 1023                        # SPRK_INGEST_MAX_FLATTEN: a window's integer sum stays below 2^53


def _flatten_check(binned, rng, R):
    if binned.dim() != 2 or binned.dtype != torch.float32 or binned.numel() < 1:
        raise _lib.SprkError("ingest_flatten: binned must be a non-empty 2-D float32 tensor, got %s %s"
                             % (binned.dtype, tuple(binned.shape)))
    _range_check("ingest_flatten", rng, binned)
    if not 1 <= R <= INGEST_MAX_FLATTEN:
        raise _lib.SprkError("ingest_flatten: radius %d (1..%d)" % (R, INGEST_MAX_FLATTEN))


def _ingest_flatten(binned, rng, R):
    """-> (binned minus its mean over the clamped (2R+1)^2 window, float32 [by, bx]; range float32 [2] = the result's min
    and max).  ``rng`` must bound ``binned`` (ingest_bin's or ingest_clip's).  Functional: neither argument is written."""
    _flatten_check(binned, rng, R)
    binned = binned.contiguous()
    by, bx = binned.shape
    L = _lib.lib()
    out, rng_out = _f32(binned, (by, bx)), _f32(binned, (2,))
    ws = _ws(L.sprk_ingest_flatten_ws_bytes(by, bx, int(R)), binned)
    check(L.sprk_ingest_flatten(_p(binned), _p(out), by, bx, int(R), _p(rng), _p(rng_out), _p(ws), ws.numel(),
                                _stream(binned)), "sprk_ingest_flatten")
    return out, rng_out


def _ingest_flatten_fake(binned, rng, R):
    _flatten_check(binned, rng, R)
    return binned.new_empty(tuple(binned.shape), dtype=torch.float32), binned.new_empty((2,), dtype=torch.float32)


_register("ingest_flatten", "(Tensor binned, Tensor range, int R) -> (Tensor, Tensor)", _ingest_flatten,
          _ingest_flatten_fake)

INGEST_MAX_SIDE = 16384                          # sprk_ingest_resample: the longest image side it takes


def _resample_check(raw, mode, ny, nx, by, bx, my, mx):
    _mode_check("ingest_resample", mode)
    if not (2 <= by <= ny <= INGEST_MAX_SIDE and 2 <= bx <= nx <= INGEST_MAX_SIDE):
        raise _lib.SprkError("ingest_resample: a %dx%d image resampled to %dx%d (2 <= by <= ny <= %d and 2 <= bx <= nx <= %d)"
                             % (ny, nx, by, bx, INGEST_MAX_SIDE, INGEST_MAX_SIDE))
    _raw_check("ingest_resample", raw, mode, ny, nx)
    for name, m, S, B in (("my", my, by, ny), ("mx", mx, bx, nx)):
        _matrix_check("ingest_resample", name, m, crop_matrix_shape(B, S), raw,
                      "matrix of ingest.resample_matrix(%d, %d)" % (B, S))


def _ingest_resample(raw, mode, ny, nx, by, bx, my, mx):
    """raw: uint8 CUDA tensor holding the file's ny*nx samples; my, mx: ingest.resample_matrix(ny, by) / (nx, bx) ->
    (the Fourier-cropped image float32 [by, bx], range float32 [2])."""
    _resample_check(raw, mode, ny, nx, by, bx, my, mx)
    if not raw.is_contiguous() or not my.is_contiguous() or not mx.is_contiguous():
        raise _lib.SprkError("ingest_resample: raw, my and mx must be contiguous")
    L = _lib.lib()
    out, rng = _f32(raw, (by, bx)), _f32(raw, (2,))
    ws = _ws(L.sprk_ingest_resample_ws_bytes(int(ny), int(nx), int(by), int(bx)), raw)
    check(L.sprk_ingest_resample(_p(raw), int(mode), int(ny), int(nx), int(by), int(bx), _p(my), int(my.shape[1]), _p(mx),
                                 int(mx.shape[1]), _p(out), _p(rng), _p(ws), ws.numel(), _stream(raw)),
          "sprk_ingest_resample")
    return out, rng


def _ingest_resample_fake(raw, mode, ny, nx, by, bx, my, mx):
    _resample_check(raw, mode, ny, nx, by, bx, my, mx)
    return raw.new_empty((by, bx), dtype=torch.float32), raw.new_empty((2,), dtype=torch.float32)


_register("ingest_resample", "(Tensor raw, int mode, int ny, int nx, int by, int bx, Tensor my, Tensor mx) -> (Tensor, Tensor)",
          _ingest_resample, _ingest_resample_fake)


# ---- whole-frame motion correction of movies (align.py: csrc/align.hip) --------------------------------------------------------
ALIGN_MAX_SHIFT = 31                             # sprk_align_corr: the largest window radius R
ALIGN_TILES = (0, 16, 32, 64)                    # ... and its tilings (0: the library's choice); the bytes are the same


def _align_corr_check(a, r, R, tile):
    if a.dtype != torch.float32 or a.dim() != 3 or r.dtype != torch.float32 or r.device != a.device:
        raise _lib.SprkError("align_corr: a must be float32 [Z, Sy, Sx] and r float32 on the same device, got %s %s and %s %s"
                             % (a.dtype, tuple(a.shape), r.dtype, tuple(r.shape)))
    Z, Sy, Sx = a.shape
    if tuple(r.shape) not in ((Z, Sy, Sx), (Sy, Sx)):
        raise _lib.SprkError("align_corr: r must be [%d, %d, %d] (one reference per frame) or [%d, %d] (one shared), got %s"
                             % (Z, Sy, Sx, Sy, Sx, tuple(r.shape)))
    if not (1 <= R <= ALIGN_MAX_SHIFT and Z >= 1 and Sx >= 64 and Sx % 64 == 0 and 1 <= Sy and max(Sy, Sx) <= INGEST_MAX_SIDE):
        raise _lib.SprkError("align_corr: %d frames of %dx%d with R %d (1 <= R <= %d, Sx a multiple of 64, both sides at most %d)"
                             % (Z, Sy, Sx, R, ALIGN_MAX_SHIFT, INGEST_MAX_SIDE))
    if tile not in ALIGN_TILES:
        raise _lib.SprkError("align_corr: tile %r (one of %s)" % (tile, ALIGN_TILES))
    return Z, Sy, Sx


def _align_corr(a, r, R, tile=0):
    """a: reduced frames float32 [Z, Sy, Sx]; r: their references [Z, Sy, Sx], or one shared [Sy, Sx] -> the correlation
    windows float32 [Z, 2R+1, 2R+1] (sprk_align_corr)."""
    Z, Sy, Sx = _align_corr_check(a, r, R, tile)
    if not a.is_contiguous() or not r.is_contiguous():
        raise _lib.SprkError("align_corr: a and r must be contiguous")
    cc = _f32(a, (Z, 2 * R + 1, 2 * R + 1))
    check(_lib.lib().sprk_align_corr(_p(a), _p(r), Sy * Sx if r.dim() == 3 else 0, Z, Sy, Sx, int(R), int(tile), _p(cc),
                                     _stream(a)), "sprk_align_corr")
    return cc


def _align_corr_fake(a, r, R, tile=0):
    Z, _, _ = _align_corr_check(a, r, R, tile)
    return a.new_empty((Z, 2 * R + 1, 2 * R + 1))


_register("align_corr", "(Tensor a, Tensor r, int R, int tile=0) -> Tensor", _align_corr, _align_corr_fake)


def _align_accumulate_check(raw, mode, ny, nx, by, bx, my, mx, y):
    _resample_check(raw, mode, ny, nx, by, bx, my, mx)
    if y.dtype != torch.float32 or tuple(y.shape) != (by, bx) or y.device != raw.device:
        raise _lib.SprkError("align_accumulate: y must be float32 [%d, %d] on %s, got %s %s on %s"
                             % (by, bx, raw.device, y.dtype, tuple(y.shape), y.device))


def _align_accumulate(raw, mode, ny, nx, by, bx, my, mx, anchor, y, first):
    """raw, mode, sizes and matrices as ``ingest_resample``'s; anchor: what the integer modes subtract from every sample (a
    sample value; 0 for float32); y float32 [by, bx]: the running sum, updated in place (overwritten when ``first``)
    (sprk_align_accumulate)."""
    _align_accumulate_check(raw, mode, ny, nx, by, bx, my, mx, y)
    if not raw.is_contiguous() or not my.is_contiguous() or not mx.is_contiguous() or not y.is_contiguous():
        raise _lib.SprkError("align_accumulate: raw, my, mx and y must be contiguous")
    L = _lib.lib()
    ws = _ws(L.sprk_align_accumulate_ws_bytes(int(ny), int(nx), int(by), int(bx)), raw)
    check(L.sprk_align_accumulate(_p(raw), int(mode), int(ny), int(nx), int(by), int(bx), _p(my), int(my.shape[1]), _p(mx),
                                  int(mx.shape[1]), float(anchor), _p(y), 1 if first else 0, _p(ws), ws.numel(),
                                  _stream(raw)), "sprk_align_accumulate")


def _align_accumulate_fake(raw, mode, ny, nx, by, bx, my, mx, anchor, y, first):
    _align_accumulate_check(raw, mode, ny, nx, by, bx, my, mx, y)


_register("align_accumulate", "(Tensor raw, int mode, int ny, int nx, int by, int bx, Tensor my, Tensor mx, float anchor, "
          "Tensor(a!) y, bool first) -> ()", _align_accumulate, _align_accumulate_fake)


# dose-weighted sums (dose.py: csrc/alignsum.hip): the movie accumulated in Fourier space
def align_spectrum_shapes(ny, nx, by, bx, Ku):
    """-> the shapes of w1, w2, w3, w4 and of F / g for a [ny, nx] frame, a [by, bx] sum and Ku kept rows (Hs = bx // 2 + 1)"""
    Hs = bx // 2 + 1
    return ((2 * Hs, _up4(nx)), (2 * Ku, _up4(2 * ny)), (2 * by, _up4(2 * Ku)), (bx, _up4(2 * Hs)), (2 * Ku, _up4(Hs)))


def _align_spectrum_check(raw, mode, ny, nx, w1, w2, g, F):
    _mode_check("align_spectrum", mode)
    if not (2 <= ny <= INGEST_MAX_SIDE and 2 <= nx <= INGEST_MAX_SIDE):
        raise _lib.SprkError("align_spectrum: a %dx%d frame (2 <= ny, nx <= %d)" % (ny, nx, INGEST_MAX_SIDE))
    _raw_check("align_spectrum", raw, mode, ny, nx)
    if w1.dim() != 2 or w2.dim() != 2 or w1.shape[0] % 2 or w2.shape[0] % 2:
        raise _lib.SprkError("align_spectrum: w1 must be [2Hs, roundup(nx, 4)] and w2 [2Ku, roundup(2ny, 4)], got %s and %s"
                             % (tuple(w1.shape), tuple(w2.shape)))
    Hs, Ku = w1.shape[0] // 2, w2.shape[0] // 2
    if not (1 <= Hs <= nx // 2 + 1 and 1 <= Ku <= ny + 1):
        raise _lib.SprkError("align_spectrum: %d kept rows and %d kept columns of a %dx%d frame (1 <= Ku <= ny + 1, "
                             "1 <= Hs <= nx / 2 + 1)" % (Ku, Hs, ny, nx))
    for name, m, shape in (("w1", w1, (2 * Hs, _up4(nx))), ("w2", w2, (2 * Ku, _up4(2 * ny))), ("g", g, (2 * Ku, _up4(Hs))),
                           ("F", F, (2 * Ku, _up4(Hs)))):
        _matrix_check("align_spectrum", name, m, shape, raw)
    return Ku, Hs


def _align_spectrum(raw, mode, ny, nx, w1, w2, g, anchor, F, first):
    """raw, mode and anchor as ``align_accumulate``'s; w1 [2Hs, roundup(nx, 4)], w2 [2Ku, roundup(2ny, 4)]; g, F float32
    [2Ku, roundup(Hs, 4)], real rows over imaginary rows: F (+)= g . crop(DFT2(D)), in place (overwritten when ``first``)
    (sprk_align_spectrum)."""
    Ku, Hs = _align_spectrum_check(raw, mode, ny, nx, w1, w2, g, F)
    if not all(t.is_contiguous() for t in (raw, w1, w2, g, F)):
        raise _lib.SprkError("align_spectrum: raw, w1, w2, g and F must be contiguous")
    L = _lib.lib()
    ws = _ws(L.sprk_align_spectrum_ws_bytes(int(ny), int(nx), Hs), raw)
    check(L.sprk_align_spectrum(_p(raw), int(mode), int(ny), int(nx), Ku, Hs, _p(w1), _p(w2), _p(g), float(anchor), _p(F),
                                1 if first else 0, _p(ws), ws.numel(), _stream(raw)), "sprk_align_spectrum")


def _align_spectrum_fake(raw, mode, ny, nx, w1, w2, g, anchor, F, first):
    _align_spectrum_check(raw, mode, ny, nx, w1, w2, g, F)


_register("align_spectrum", "(Tensor raw, int mode, int ny, int nx, Tensor w1, Tensor w2, Tensor g, float anchor, "
          "Tensor(a!) F, bool first) -> ()", _align_spectrum, _align_spectrum_fake)


def _align_synthesize_check(F, by, bx, w3, w4):
    if not (2 <= by <= INGEST_MAX_SIDE and 2 <= bx <= INGEST_MAX_SIDE):
        raise _lib.SprkError("align_synthesize: a %dx%d sum (2 <= by, bx <= %d)" % (by, bx, INGEST_MAX_SIDE))
    if F.dtype != torch.float32 or F.dim() != 2 or F.shape[0] % 2 or not 1 <= F.shape[0] // 2 <= by + 1:
        raise _lib.SprkError("align_synthesize: F must be float32 [2Ku, roundup(Hs, 4)] with 1 <= Ku <= by + 1 = %d, got %s %s"
                             % (by + 1, F.dtype, tuple(F.shape)))
    Ku, Hs = F.shape[0] // 2, bx // 2 + 1
    for name, m, shape in (("F", F, (2 * Ku, _up4(Hs))), ("w3", w3, (2 * by, _up4(2 * Ku))), ("w4", w4, (bx, _up4(2 * Hs)))):
        _matrix_check("align_synthesize", name, m, shape, F)
    return Ku, Hs


def _align_synthesize(F, by, bx, w3, w4):
    """F float32 [2Ku, roundup(Hs, 4)] with Hs = bx // 2 + 1; w3 [2by, roundup(2Ku, 4)], w4 [bx, roundup(2Hs, 4)] -> the sum
    float32 [by, bx] (sprk_align_synthesize)."""
    Ku, Hs = _align_synthesize_check(F, by, bx, w3, w4)
    if not all(t.is_contiguous() for t in (F, w3, w4)):
        raise _lib.SprkError("align_synthesize: F, w3 and w4 must be contiguous")
    L = _lib.lib()
    y = _f32(F, (by, bx))
    ws = _ws(L.sprk_align_synthesize_ws_bytes(int(by), Hs), F)
    check(L.sprk_align_synthesize(_p(F), Ku, Hs, int(by), int(bx), _p(w3), _p(w4), _p(y), _p(ws), ws.numel(), _stream(F)),
          "sprk_align_synthesize")
    return y


def _align_synthesize_fake(F, by, bx, w3, w4):
    _align_synthesize_check(F, by, bx, w3, w4)
    return F.new_empty((by, bx))


_register("align_synthesize", "(Tensor F, int by, int bx, Tensor w3, Tensor w4) -> Tensor", _align_synthesize,
          _align_synthesize_fake)


# raw detector movies in (moviefix.py: csrc/moviefix.hip): dark, gain and the repair of marked pixels, one frame per call
FIX_MAX_RADIUS = 8                               # SPRK_FIX_MAX_RADIUS: larger values of the fix map are clamped to it


def _movie_correct_check(raw, mode, ny, nx, gain, dark, fix, out, sum):
    _mode_check("movie_correct", mode)
    if not (1 <= ny <= INGEST_MAX_SIDE and 1 <= nx <= INGEST_MAX_SIDE):
        raise _lib.SprkError("movie_correct: a %dx%d frame (both sides in 1..%d)" % (ny, nx, INGEST_MAX_SIDE))
    _raw_check("movie_correct", raw, mode, ny, nx)
    for name, t, dtype in (("gain", gain, torch.float32), ("dark", dark, torch.float32), ("fix", fix, torch.uint8),
                           ("out", out, torch.float32), ("sum", sum, torch.float32)):
        if t is not None and (t.dtype != dtype or tuple(t.shape) != (ny, nx) or t.device != raw.device):
            raise _lib.SprkError("movie_correct: %s must be %s [%d, %d] on %s, got %s %s on %s"
                                 % (name, dtype, ny, nx, raw.device, t.dtype, tuple(t.shape), t.device))


def _movie_correct(raw, mode, ny, nx, gain, dark, fix, out, sum, first):
    """raw: uint8 CUDA tensor holding one frame's ny*nx samples; gain, dark float32 [ny, nx] or None; fix uint8 [ny, nx] or
    None (0: keep, r > 0: the mean of the good pixels within r, at most ``FIX_MAX_RADIUS``); out float32 [ny, nx],
    overwritten; sum float32 [ny, nx] or None: out is written to it when ``first``, else added (sprk_movie_correct)."""
    _movie_correct_check(raw, mode, ny, nx, gain, dark, fix, out, sum)
    if not all(t is None or t.is_contiguous() for t in (raw, gain, dark, fix, out, sum)):
        raise _lib.SprkError("movie_correct: raw, gain, dark, fix, out and sum must be contiguous")
    check(_lib.lib().sprk_movie_correct(_p(raw), int(mode), int(ny), int(nx), _p(gain), _p(dark), _p(fix), _p(out), _p(sum),
                                        1 if first else 0, _stream(raw)), "sprk_movie_correct")


def _movie_correct_fake(raw, mode, ny, nx, gain, dark, fix, out, sum, first):
    _movie_correct_check(raw, mode, ny, nx, gain, dark, fix, out, sum)


_register("movie_correct", "(Tensor raw, int mode, int ny, int nx, Tensor? gain, Tensor? dark, Tensor? fix, Tensor(a!) out, "
          "Tensor(b!)? sum, bool first) -> ()", _movie_correct, _movie_correct_fake)


# local motion (localmotion.py: csrc/warp.hip): one frame through a quadratic displacement field, Catmull-Rom taps
WARP_MAX_SHIFT = 16                              # SPRK_WARP_MAX_SHIFT: the field is clamped to +- this many pixels
WARP_TERMS = 6                                   # coefficients per axis: 1, u, v, u u, u v, v v


def _align_warp_check(src, cy, cx, y):
    if src.dtype != torch.float32 or src.dim() != 2:
        raise _lib.SprkError("align_warp: src must be float32 [ny, nx], got %s %s" % (src.dtype, tuple(src.shape)))
    ny, nx = src.shape
    if not (1 <= ny <= INGEST_MAX_SIDE and 1 <= nx <= INGEST_MAX_SIDE):
        raise _lib.SprkError("align_warp: a %dx%d frame (both sides in 1..%d)" % (ny, nx, INGEST_MAX_SIDE))
    if y.dtype != torch.float32 or tuple(y.shape) != (ny, nx) or y.device != src.device:
        raise _lib.SprkError("align_warp: y must be float32 [%d, %d] on %s, got %s %s on %s"
                             % (ny, nx, src.device, y.dtype, tuple(y.shape), y.device))
    if len(cy) != WARP_TERMS or len(cx) != WARP_TERMS:
        raise _lib.SprkError("align_warp: %d + %d coefficients (%d per axis: 1, u, v, uu, uv, vv)"
                             % (len(cy), len(cx), WARP_TERMS))
    c32 = (ctypes.c_float * WARP_TERMS)(*cy), (ctypes.c_float * WARP_TERMS)(*cx)    # rounded to float32 here
    for c in c32:
        for v in c:
            if v != v or v in (float("inf"), float("-inf")):
                raise _lib.SprkError("align_warp: every coefficient must be finite in float32, got %s and %s"
                                     % (list(cy), list(cx)))
    return c32


def _align_warp(src, cy, cx, y, first):
    """src float32 CUDA [ny, nx]; cy, cx: the 6 coefficients each of the row and column displacement (1, u, v, uu, uv, vv;
    u = j / nx - 1/2, v = i / ny - 1/2), passed by value; y float32 [ny, nx]: out(i, j) = src(i + sy, j + sx), periodic,
    Catmull-Rom, |s| clamped to ``WARP_MAX_SHIFT``, written to y when ``first``, else added (sprk_align_warp)."""
    c32y, c32x = _align_warp_check(src, cy, cx, y)
    if not (src.is_contiguous() and y.is_contiguous()):
        raise _lib.SprkError("align_warp: src and y must be contiguous")
    if src.data_ptr() == y.data_ptr():
        raise _lib.SprkError("align_warp: y must not be src")
    check(_lib.lib().sprk_align_warp(_p(src), int(src.shape[0]), int(src.shape[1]), c32y, c32x, _p(y), 1 if first else 0,
                                     _stream(src)), "sprk_align_warp")


def _align_warp_fake(src, cy, cx, y, first):
    _align_warp_check(src, cy, cx, y)


_register("align_warp", "(Tensor src, float[] cy, float[] cx, Tensor(a!) y, bool first) -> ()", _align_warp, _align_warp_fake)


# TIFF movies in (tiffio.py, align.TiffMovie: csrc/tiff.hip): the strips of one frame decoded, one wave per strip
TIFF_MAX_STRIPS = 1 << 20
TIFF_COMPRESSIONS = (1, 5)                       # stored, LZW


def _tiff_decode_check(src, strip_off, strip_len, strip_out, compression, widen, out, status):
    if src.dtype != torch.uint8 or src.dim() != 1 or src.numel() < 1:
        raise _lib.SprkError("tiff_decode: src must be uint8 [nbytes >= 1], got %s %s" % (src.dtype, tuple(src.shape)))
    n = strip_off.numel()
    if not 1 <= n <= TIFF_MAX_STRIPS:
        raise _lib.SprkError("tiff_decode: %d strips (1..%d)" % (n, TIFF_MAX_STRIPS))
    for name, t in (("strip_off", strip_off), ("strip_len", strip_len), ("strip_out", strip_out)):
        if t.dtype != torch.int64 or tuple(t.shape) != (n,) or t.device != src.device:
            raise _lib.SprkError("tiff_decode: %s must be int64 [%d] on %s, got %s %s on %s"
                                 % (name, n, src.device, t.dtype, tuple(t.shape), t.device))
    if compression not in TIFF_COMPRESSIONS:
        raise _lib.SprkError("tiff_decode: compression %d (1: stored, 5: LZW)" % compression)
    if out.dtype != torch.uint8 or out.dim() != 1 or out.numel() < (2 if widen else 1) or out.device != src.device \
            or (widen and out.numel() % 2):
        raise _lib.SprkError("tiff_decode: out must be uint8 [decoded bytes%s] on %s, got %s %s on %s"
                             % (" x 2" if widen else "", src.device, out.dtype, tuple(out.shape), out.device))
    if status.dtype != torch.int32 or tuple(status.shape) != (n,) or status.device != src.device:
        raise _lib.SprkError("tiff_decode: status must be int32 [%d] on %s, got %s %s on %s"
                             % (n, src.device, status.dtype, tuple(status.shape), status.device))
    return n, out.numel() // (2 if widen else 1)


def _tiff_decode(src, strip_off, strip_len, strip_out, compression, widen, out, status):
    """src: uint8 CUDA [nbytes], a frame's strips as they lie in the file; strip_off, strip_len, strip_out: int64 [n_strips]
    (offset into src, bytes, decoded bytes to yield); compression 1 (stored) or 5 (LZW); widen: every decoded byte becomes
    one little-endian uint16; out: uint8 [sum of strip_out (x 2 with widen)], the sample block; status int32 [n_strips]:
    0 ok, 1 bad code, 2 input ran out, 3 a string past the strip's end (sprk_tiff_decode)."""
    n, out_elems = _tiff_decode_check(src, strip_off, strip_len, strip_out, compression, widen, out, status)
    if not all(t.is_contiguous() for t in (src, strip_off, strip_len, strip_out, out, status)):
        raise _lib.SprkError("tiff_decode: src, the strip tables, out and status must be contiguous")
    check(_lib.lib().sprk_tiff_decode(_p(src), src.numel(), _p(strip_off), _p(strip_len), _p(strip_out), n, int(compression),
                                      1 if widen else 0, _p(out), out_elems, _p(status), _stream(src)), "sprk_tiff_decode")


def _tiff_decode_fake(src, strip_off, strip_len, strip_out, compression, widen, out, status):
    _tiff_decode_check(src, strip_off, strip_len, strip_out, compression, widen, out, status)


_register("tiff_decode", "(Tensor src, Tensor strip_off, Tensor strip_len, Tensor strip_out, int compression, bool widen, "
          "Tensor(a!) out, Tensor(b!) status) -> ()", _tiff_decode, _tiff_decode_fake)


# ---- reference-free 2-D classification (class2d.py: csrc/class2d.hip) ----------------------------------------------------------
CLASS_MAX_SIDE = 128                             # sprk_class_transform / _average: S even, at most this
CLASS_MAX_ANGLES = 720                           # rows of the cos / sin table at most
CLASS_MASK, CLASS_NORMALIZE = 1, 2               # SPRK_CLASS_*
CLASS_MAX_BANK = 65536                           # sprk_class_score: bank rows at most
CLASS_MAX_D = 16384                              # ... and columns (a multiple of 4, at least 4)


def _is_i32(t, shape, dev):
    return t.dtype == torch.int32 and tuple(t.shape) == tuple(shape) and t.device == dev


def _class_images(who, src, cs):
    if src.dtype != torch.float32 or src.dim() != 3 or src.shape[1] != src.shape[2] or src.shape[0] < 1:
        raise _lib.SprkError("%s: src must be float32 [n, S, S], got %s %s" % (who, src.dtype, tuple(src.shape)))
    S = src.shape[1]
    if not (2 <= S <= CLASS_MAX_SIDE and S % 2 == 0):
        raise _lib.SprkError("%s: images of side %d (even, 2..%d)" % (who, S, CLASS_MAX_SIDE))
    if cs.dtype != torch.float32 or cs.dim() != 2 or cs.shape[1] != 2 or not 1 <= cs.shape[0] <= CLASS_MAX_ANGLES \
            or cs.device != src.device:
        raise _lib.SprkError("%s: cs must be float32 [A_n, 2] (cos, sin; 1 <= A_n <= %d) on %s, got %s %s on %s"
                             % (who, CLASS_MAX_ANGLES, src.device, cs.dtype, tuple(cs.shape), cs.device))
    return int(src.shape[0]), int(S), int(cs.shape[0])


def _class_transform_check(src, idx, ang, shift, cs, radius, flags, pix, out):
    n_src, S, A_n = _class_images("class_transform", src, cs)
    M = idx.shape[0] if idx.dim() == 1 else 0
    if M < 1 or not (_is_i32(idx, (M,), src.device) and _is_i32(ang, (M,), src.device) and _is_i32(shift, (M, 2), src.device)):
        raise _lib.SprkError("class_transform: idx and ang must be int32 [M] and shift int32 [M, 2] on %s (M >= 1), got %s, %s, "
                             "%s" % (src.device, tuple(idx.shape), tuple(ang.shape), tuple(shift.shape)))
    if flags & ~(CLASS_MASK | CLASS_NORMALIZE):
        raise _lib.SprkError("class_transform: unknown flags 0x%x" % flags)
    if flags and not 0 <= radius <= S:
        raise _lib.SprkError("class_transform: mask radius %d (0..%d)" % (radius, S))
    if out.dtype != torch.float32 or out.device != src.device:
        raise _lib.SprkError("class_transform: out must be float32 on %s, got %s on %s" % (src.device, out.dtype, out.device))
    if pix is None:
        if tuple(out.shape) != (M, S, S):
            raise _lib.SprkError("class_transform: out must be [%d, %d, %d], got %s" % (M, S, S, tuple(out.shape)))
        return n_src, S, A_n, M, 0, 0
    D = pix.shape[0] if pix.dim() == 1 else 0
    if not (1 <= D <= S * S and _is_i32(pix, (D,), src.device)):
        raise _lib.SprkError("class_transform: pix must be int32 [D] on %s with 1 <= D <= S*S = %d, got %s %s"
                             % (src.device, S * S, pix.dtype, tuple(pix.shape)))
    if out.dim() != 2 or out.shape[0] != M or out.shape[1] < D or out.shape[1] % 4:
        raise _lib.SprkError("class_transform: the packed out must be [%d, ldo] with ldo a multiple of 4, at least D = %d, got "
                             "%s" % (M, D, tuple(out.shape)))
    return n_src, S, A_n, M, D, int(out.shape[1])


def _class_transform(src, idx, ang, shift, cs, radius, flags, pix, out):
    """src float32 [n, S, S]; idx, ang int32 [M]; shift int32 [M, 2] (dy, dx); cs float32 [A_n, 2]: out[m] = the rigid
    transform of src[idx[m]] by the angle cs[ang[m]] and its shift, bilinear, zero beyond the edges; flags CLASS_MASK /
    CLASS_NORMALIZE with the mask ``radius``; out float32 [M, S, S], or with pix (int32 [D] linear pixel indices) the packed
    [M, ldo], columns D .. ldo-1 zeros (sprk_class_transform)."""
    n_src, S, A_n, M, D, ldo = _class_transform_check(src, idx, ang, shift, cs, radius, flags, pix, out)
    for t in (src, idx, ang, shift, cs, out) + (() if pix is None else (pix,)):
        if not t.is_contiguous():
            raise _lib.SprkError("class_transform: every tensor must be contiguous")
    check(_lib.lib().sprk_class_transform(_p(src), n_src, S, _p(idx), _p(ang), _p(shift), M, _p(cs), A_n, int(radius),
                                          int(flags), _p(pix), D, ldo, _p(out), _stream(src)), "sprk_class_transform")


def _class_transform_fake(src, idx, ang, shift, cs, radius, flags, pix, out):
    _class_transform_check(src, idx, ang, shift, cs, radius, flags, pix, out)


_register("class_transform", "(Tensor src, Tensor idx, Tensor ang, Tensor shift, Tensor cs, int radius, int flags, Tensor? pix, "
          "Tensor(a!) out) -> ()", _class_transform, _class_transform_fake)


def _class_score_check(Q, B, D, scores, best_score, best_index):
    if Q.dtype != torch.float32 or Q.dim() != 2 or B.dtype != torch.float32 or B.dim() != 2 or B.device != Q.device:
        raise _lib.SprkError("class_score: Q [N, ldq] and B [Mb, ldb] must be float32 on one device, got %s %s and %s %s"
                             % (Q.dtype, tuple(Q.shape), B.dtype, tuple(B.shape)))
    N, ldq = Q.shape
    Mb, ldb = B.shape
    if not (N >= 1 and 1 <= Mb <= CLASS_MAX_BANK and 4 <= D <= CLASS_MAX_D and D % 4 == 0):
        raise _lib.SprkError("class_score: %d rows against a bank of %d with D = %d (N >= 1, 1 <= Mb <= %d, D a multiple of 4 in "
                             "4..%d)" % (N, Mb, D, CLASS_MAX_BANK, CLASS_MAX_D))
    if ldq < D or ldq % 4 or ldb < D or ldb % 4:
        raise _lib.SprkError("class_score: row strides %d and %d (multiples of 4, at least D = %d)" % (ldq, ldb, D))
    if best_score.dtype != torch.float32 or tuple(best_score.shape) != (N,) or best_score.device != Q.device \
            or not _is_i32(best_index, (N,), Q.device):
        raise _lib.SprkError("class_score: best_score must be float32 [%d] and best_index int32 [%d] on %s"
                             % (N, N, Q.device))
    if scores is not None and (scores.dtype != torch.float32 or scores.dim() != 2 or scores.shape[0] != N
                               or scores.shape[1] < Mb or scores.device != Q.device):
        raise _lib.SprkError("class_score: scores must be float32 [%d, at least %d] on %s, got %s %s"
                             % (N, Mb, Q.device, scores.dtype, tuple(scores.shape)))
    return int(N), int(ldq), int(Mb), int(ldb)


def _class_score(Q, B, D, scores, best_score, best_index):
    """Q float32 [N, ldq], B float32 [Mb, ldb] (columns D .. ld-1 zeros): s[n, m] = the fmaf chain over d < D of Q[n, d] *
    B[m, d] on MFMA; best_score[n] its maximum over m, best_index[n] the lowest m that attains it; scores (or None) receives
    s in its columns 0 .. Mb-1 (sprk_class_score)."""
    N, ldq, Mb, ldb = _class_score_check(Q, B, D, scores, best_score, best_index)
    for t in (Q, B, best_score, best_index) + (() if scores is None else (scores,)):
        if not t.is_contiguous():
            raise _lib.SprkError("class_score: every tensor must be contiguous")
    check(_lib.lib().sprk_class_score(_p(Q), ldq, N, _p(B), ldb, Mb, int(D), _p(scores),
                                      0 if scores is None else int(scores.shape[1]), _p(best_score), _p(best_index),
                                      _stream(Q)), "sprk_class_score")


def _class_score_fake(Q, B, D, scores, best_score, best_index):
    _class_score_check(Q, B, D, scores, best_score, best_index)


_register("class_score", "(Tensor Q, Tensor B, int D, Tensor(a!)? scores, Tensor(b!) best_score, Tensor(c!) best_index) -> ()",
          _class_score, _class_score_fake)


def _class_average_check(src, ang, shift, cs, members, offsets, out):
    n_src, S, A_n = _class_images("class_average", src, cs)
    if not (_is_i32(ang, (n_src,), src.device) and _is_i32(shift, (n_src, 2), src.device)):
        raise _lib.SprkError("class_average: ang must be int32 [%d] and shift int32 [%d, 2] on %s (one per particle), got %s "
                             "and %s" % (n_src, n_src, src.device, tuple(ang.shape), tuple(shift.shape)))
    N = members.shape[0] if members.dim() == 1 else 0
    K = offsets.shape[0] - 1 if offsets.dim() == 1 else 0
    if not (N >= 1 and 1 <= K <= 65535 and _is_i32(members, (N,), src.device) and _is_i32(offsets, (K + 1,), src.device)):
        raise _lib.SprkError("class_average: members must be int32 [N >= 1] and offsets int32 [K + 1] (1 <= K <= 65535) on %s, "
                             "got %s %s and %s %s" % (src.device, members.dtype, tuple(members.shape), offsets.dtype,
                                                      tuple(offsets.shape)))
    if out.dtype != torch.float32 or tuple(out.shape) != (K, S, S) or out.device != src.device:
        raise _lib.SprkError("class_average: out must be float32 [%d, %d, %d] on %s, got %s %s"
                             % (K, S, S, src.device, out.dtype, tuple(out.shape)))
    return n_src, S, A_n, int(N), int(K)


def _class_average(src, ang, shift, cs, members, offsets, out):
    """src float32 [n, S, S]; ang int32 [n], shift int32 [n, 2]: each particle's angle index and shift; members int32 [N]
    grouped by class, offsets int32 [K + 1]: out[k] = the fp32 sum, in list order, of the class's transformed members times
    1 / count; an empty class keeps what out[k] holds (sprk_class_average)."""
    n_src, S, A_n, N, K = _class_average_check(src, ang, shift, cs, members, offsets, out)
    for t in (src, ang, shift, cs, members, offsets, out):
        if not t.is_contiguous():
            raise _lib.SprkError("class_average: every tensor must be contiguous")
    if src.data_ptr() == out.data_ptr():
        raise _lib.SprkError("class_average: out must not be src")
    check(_lib.lib().sprk_class_average(_p(src), n_src, S, _p(ang), _p(shift), _p(cs), A_n, _p(members), N, _p(offsets), K,
                                        _p(out), _stream(src)), "sprk_class_average")


def _class_average_fake(src, ang, shift, cs, members, offsets, out):
    _class_average_check(src, ang, shift, cs, members, offsets, out)


_register("class_average", "(Tensor src, Tensor ang, Tensor shift, Tensor cs, Tensor members, Tensor offsets, Tensor(a!) out) "
          "-> ()", _class_average, _class_average_fake)


# Wiener-weighted class averages (class2d.py with ctf=: csrc/classctf.hip)
CLASS_CTF_MIN_SIDE = 16                          # sprk_class_spectrum / _wiener / _synthesize: side even, 16..CLASS_MAX_SIDE


def class_ctf_side(who, side):
    """Argument check shared by the three operators and ctf.weight_tables -> side."""
    if not (CLASS_CTF_MIN_SIDE <= side <= CLASS_MAX_SIDE) or side % 2:
        raise _lib.SprkError("%s: a side of %d (even, %d..%d; `joint extract --scale 64` writes such stacks)"
                             % (who, side, CLASS_CTF_MIN_SIDE, CLASS_MAX_SIDE))
    return int(side)


def class_spectrum_shapes(side):
    """-> the shapes of w1, w2, w3, w4 (``extract_filter_shapes(side, side)``), of one spectrum [2Ku, roundup(Hs, 4)] and
    of one weight table [Ku, roundup(Hs, 4)]"""
    hs, ku = side // 2 + 1, side + 1
    return extract_filter_shapes(side, side)[:4] + ((2 * ku, _up4(hs)), (ku, _up4(hs)))


def _class_spectra_check(who, name, t, side, like):
    """t: float32 [n, 2Ku, ldv] on the device of ``like`` -> n"""
    shape = class_spectrum_shapes(side)[4]
    if t.dtype != torch.float32 or t.dim() != 3 or tuple(t.shape[1:]) != shape or t.device != like.device:
        raise _lib.SprkError("%s: %s must be float32 [n, %d, %d] on %s, got %s %s on %s"
                             % (who, name, *shape, like.device, t.dtype, tuple(t.shape), t.device))
    return int(t.shape[0])


def _class_spectrum_check(img, w1, w2, max_batch, spec):
    if img.dtype != torch.float32 or img.dim() != 3 or img.shape[1] != img.shape[2]:
        raise _lib.SprkError("class_spectrum: img must be float32 [n, S, S], got %s %s" % (img.dtype, tuple(img.shape)))
    n, S = int(img.shape[0]), class_ctf_side("class_spectrum", int(img.shape[1]))
    if max_batch < 0:
        raise _lib.SprkError("class_spectrum: max_batch %d (0 = the library's choice, or a positive number of images)" % max_batch)
    shapes = class_spectrum_shapes(S)
    for name, m, shape in (("w1", w1, shapes[0]), ("w2", w2, shapes[1])):
        _matrix_check("class_spectrum", name, m, shape, img, "matrix of extract.filter_matrices(%d, %d)" % (S, S))
    if _class_spectra_check("class_spectrum", "spec", spec, S, img) != n:
        raise _lib.SprkError("class_spectrum: %d images but room for %d spectra" % (n, spec.shape[0]))
    return n, S


def _class_spectrum(img, w1, w2, max_batch, spec):
    """img float32 [n, S, S]; w1, w2 of ``extract.filter_matrices(S, S)``; spec float32 [n, 2Ku, roundup(Hs, 4)] receives the
    half-plane spectrum of every image, Re rows over Im rows (sprk_class_spectrum)."""
    n, S = _class_spectrum_check(img, w1, w2, max_batch, spec)
    if not all(t.is_contiguous() for t in (img, w1, w2, spec)):
        raise _lib.SprkError("class_spectrum: img, w1, w2 and spec must be contiguous")
    if n == 0:
        return
    L = _lib.lib()
    ws = _ws(L.sprk_class_spectrum_ws_bytes(n, S, int(max_batch)), img)
    check(L.sprk_class_spectrum(_p(img), n, S, _p(w1), _p(w2), int(max_batch), _p(spec), _p(ws), ws.numel(), _stream(img)),
          "sprk_class_spectrum")


def _class_spectrum_fake(img, w1, w2, max_batch, spec):
    _class_spectrum_check(img, w1, w2, max_batch, spec)


_register("class_spectrum", "(Tensor img, Tensor w1, Tensor w2, int max_batch, Tensor(a!) spec) -> ()", _class_spectrum,
          _class_spectrum_fake)


def _class_wiener_check(spec, side, wn, wd, group, members, offsets, tau, out):
    S = class_ctf_side("class_wiener", side)
    n = _class_spectra_check("class_wiener", "spec", spec, S, spec)
    table = class_spectrum_shapes(S)[5]
    G = int(wn.shape[0]) if wn.dim() == 3 else 0
    for name, t in (("wn", wn), ("wd", wd)):
        if t.dtype != torch.float32 or G < 1 or tuple(t.shape) != (G,) + table or t.device != spec.device:
            raise _lib.SprkError("class_wiener: %s must be the float32 [G >= 1, %d, %d] of ctf.weight_tables on %s, got %s %s "
                                 "on %s" % (name, *table, spec.device, t.dtype, tuple(t.shape), t.device))
    N = members.shape[0] if members.dim() == 1 else -1
    K = offsets.shape[0] - 1 if offsets.dim() == 1 else 0
    if not (_is_i32(group, (n,), spec.device) and N >= 0 and 1 <= K <= 65535 and _is_i32(members, (N,), spec.device)
            and _is_i32(offsets, (K + 1,), spec.device)):
        raise _lib.SprkError("class_wiener: group must be int32 [%d] (one table per image), members int32 [N] and offsets "
                             "int32 [K + 1] (1 <= K <= 65535) on %s, got %s, %s and %s"
                             % (n, spec.device, tuple(group.shape), tuple(members.shape), tuple(offsets.shape)))
    if not (tau > 0 and tau != float("inf")):
        raise _lib.SprkError("class_wiener: tau %r (finite and > 0; 1.0 is the default of --wiener)" % (tau,))
    if _class_spectra_check("class_wiener", "out", out, S, spec) != K:
        raise _lib.SprkError("class_wiener: %d classes but room for %d spectra" % (K, out.shape[0]))
    return n, S, G, int(N), int(K)


def _class_wiener(spec, side, wn, wd, group, members, offsets, tau, out):
    """spec float32 [n, 2Ku, ldv]; wn, wd float32 [G, Ku, ldv]; group int32 [n]: each image's table; members int32 [N] grouped
    by class, offsets int32 [K + 1]: out[k] = sum of wn . spec over the class's members in list order over (sum of wd + tau);
    an empty class keeps what out[k] holds (sprk_class_wiener)."""
    n, S, G, N, K = _class_wiener_check(spec, side, wn, wd, group, members, offsets, tau, out)
    for t in (spec, wn, wd, group, members, offsets, out):
        if not t.is_contiguous():
            raise _lib.SprkError("class_wiener: every tensor must be contiguous")
    if spec.data_ptr() == out.data_ptr():
        raise _lib.SprkError("class_wiener: out must not be spec")
    check(_lib.lib().sprk_class_wiener(_p(spec), n, S, _p(wn), _p(wd), G, _p(group), _p(members), N, _p(offsets), K, float(tau),
                                       _p(out), _stream(spec)), "sprk_class_wiener")


def _class_wiener_fake(spec, side, wn, wd, group, members, offsets, tau, out):
    _class_wiener_check(spec, side, wn, wd, group, members, offsets, tau, out)


_register("class_wiener", "(Tensor spec, int side, Tensor wn, Tensor wd, Tensor group, Tensor members, Tensor offsets, float tau, "
          "Tensor(a!) out) -> ()", _class_wiener, _class_wiener_fake)


def _class_synthesize_check(f, side, w3, w4, out):
    S = class_ctf_side("class_synthesize", side)
    K = _class_spectra_check("class_synthesize", "f", f, S, f)
    if not 1 <= K <= 65535:
        raise _lib.SprkError("class_synthesize: %d spectra (1..65535; split a larger stack into several calls)" % K)
    shapes = class_spectrum_shapes(S)
    for name, m, shape in (("w3", w3, shapes[2]), ("w4", w4, shapes[3])):
        _matrix_check("class_synthesize", name, m, shape, f, "matrix of extract.filter_matrices(%d, %d)" % (S, S))
    if out.dtype != torch.float32 or tuple(out.shape) != (K, S, S) or out.device != f.device:
        raise _lib.SprkError("class_synthesize: out must be float32 [%d, %d, %d] on %s, got %s %s"
                             % (K, S, S, f.device, out.dtype, tuple(out.shape)))
    return K, S


def _class_synthesize(f, side, w3, w4, out):
    """f float32 [K, 2Ku, ldv]; w3, w4 of ``extract.filter_matrices(S, S)``; out float32 [K, S, S] receives the image of
    every spectrum (sprk_class_synthesize)."""
    K, S = _class_synthesize_check(f, side, w3, w4, out)
    if not all(t.is_contiguous() for t in (f, w3, w4, out)):
        raise _lib.SprkError("class_synthesize: f, w3, w4 and out must be contiguous")
    L = _lib.lib()
    ws = _ws(L.sprk_class_synthesize_ws_bytes(K, S), f)
    check(L.sprk_class_synthesize(_p(f), K, S, _p(w3), _p(w4), _p(out), _p(ws), ws.numel(), _stream(f)), "sprk_class_synthesize")


def _class_synthesize_fake(f, side, w3, w4, out):
    _class_synthesize_check(f, side, w3, w4, out)


_register("class_synthesize", "(Tensor f, int side, Tensor w3, Tensor w4, Tensor(a!) out) -> ()", _class_synthesize,
          _class_synthesize_fake)


# ---- particle extraction (extract.py: raw MRC samples + pick coordinates -> normalised particle stack) ------------------------
EXTRACT_MAX_BOX = 1024                           # sprk_extract_boxes: the int64 sum of squares stays below 2^63 up to here
EXTRACT_NORMALIZE, EXTRACT_INVERT = 1, 2         # SPRK_EXTRACT_*


def extract_side(box, bin, bg_radius=0):
    """Argument check shared by the operator, extract.py and the command line -> b = box // bin, the output side."""
    if not 1 <= bin <= INGEST_MAX_BIN:
        raise _lib.SprkError("extract_boxes: bin factor %d (1..%d)" % (bin, INGEST_MAX_BIN))
    if not 2 <= box <= EXTRACT_MAX_BOX or box % bin or box // bin < 2:
        raise _lib.SprkError("extract_boxes: box %d with bin %d (2..%d, a multiple of the bin factor, at least 2 output "
                             "pixels a side)" % (box, bin, EXTRACT_MAX_BOX))
    if bg_radius < 0:
        raise _lib.SprkError("extract_boxes: background radius %d (>= 0)" % bg_radius)
    return box // bin


def _extract_shapes(raw, mode, ny, nx, xy, box, bin, bg_radius):
    _mode_check("extract_boxes", mode)
    b = extract_side(box, bin, bg_radius)
    if ny < 1 or nx < 1 or ny * nx >= 1 << 31:
        raise _lib.SprkError("extract_boxes: bad image size %dx%d" % (ny, nx))
    _raw_check("extract_boxes", raw, mode, ny, nx)
    _xy_check("extract_boxes", xy, raw)
    return xy.shape[0], b


def _extract_boxes(raw, mode, ny, nx, xy, box, bin, bg_radius, normalize, invert):
    """-> (out float32 [P, b, b], status int32 [P]: 0 ok, 1 outside the image, 2 no or flat background)."""
    P, b = _extract_shapes(raw, mode, ny, nx, xy, box, bin, bg_radius)
    if not raw.is_contiguous():
        raise _lib.SprkError("extract_boxes: raw must be contiguous")
    xy = xy.contiguous()
    out = _f32(raw, (P, b, b))
    status = torch.empty((P,), dtype=torch.int32, device=raw.device)
    flags = (EXTRACT_NORMALIZE if normalize else 0) | (EXTRACT_INVERT if invert else 0)
    check(_lib.lib().sprk_extract_boxes(_p(raw), int(mode), int(ny), int(nx), _p(xy), P, int(box), int(bin),
                                        int(bg_radius), flags, _p(out), _p(status), _stream(raw)), "sprk_extract_boxes")
    return out, status


def _extract_boxes_fake(raw, mode, ny, nx, xy, box, bin, bg_radius, normalize, invert):
    P, b = _extract_shapes(raw, mode, ny, nx, xy, box, bin, bg_radius)
    return raw.new_empty((P, b, b), dtype=torch.float32), raw.new_empty((P,), dtype=torch.int32)


_register("extract_boxes", "(Tensor raw, int mode, int ny, int nx, Tensor xy, int box, int bin, int bg_radius, "
                           "bool normalize, bool invert) -> (Tensor, Tensor)", _extract_boxes, _extract_boxes_fake)


def extract_scale_side(box, side, bg_radius=0):
    """Argument check shared by the operator, extract.py and the command line -> side, the output side."""
    if not (2 <= side <= box <= EXTRACT_MAX_BOX):
        raise _lib.SprkError("extract_scale: box %d with output side %d (2 <= side <= box <= %d)"
                             % (box, side, EXTRACT_MAX_BOX))
    if bg_radius < 0:
        raise _lib.SprkError("extract_scale: background radius %d (>= 0)" % bg_radius)
    return side


def _extract_scale_shapes(raw, mode, ny, nx, xy, box, side, m, bg_radius):
    _mode_check("extract_scale", mode)
    extract_scale_side(box, side, bg_radius)
    if ny < 1 or nx < 1 or ny * nx >= 1 << 31:
        raise _lib.SprkError("extract_scale: bad image size %dx%d" % (ny, nx))
    _raw_check("extract_scale", raw, mode, ny, nx)
    _xy_check("extract_scale", xy, raw)
    _matrix_check("extract_scale", "m", m, crop_matrix_shape(box, side), raw,
                  "matrix of extract.crop_matrix(%d, %d)" % (box, side))
    return xy.shape[0]


def _extract_scale(raw, mode, ny, nx, xy, box, side, m, bg_radius, normalize, invert):
    """-> (out float32 [P, side, side], status int32 [P]: 0 ok, 1 outside the image, 2 no or flat background)."""
    P = _extract_scale_shapes(raw, mode, ny, nx, xy, box, side, m, bg_radius)
    if not raw.is_contiguous() or not m.is_contiguous():
        raise _lib.SprkError("extract_scale: raw and m must be contiguous")
    xy = xy.contiguous()
    out = _f32(raw, (P, side, side))
    status = torch.empty((P,), dtype=torch.int32, device=raw.device)
    flags = (EXTRACT_NORMALIZE if normalize else 0) | (EXTRACT_INVERT if invert else 0)
    check(_lib.lib().sprk_extract_scale(_p(raw), int(mode), int(ny), int(nx), _p(xy), P, int(box), int(side), _p(m),
                                        int(m.shape[1]), int(bg_radius), flags, _p(out), _p(status), _stream(raw)),
          "sprk_extract_scale")
    return out, status


def _extract_scale_fake(raw, mode, ny, nx, xy, box, side, m, bg_radius, normalize, invert):
    P = _extract_scale_shapes(raw, mode, ny, nx, xy, box, side, m, bg_radius)
    return raw.new_empty((P, side, side), dtype=torch.float32), raw.new_empty((P,), dtype=torch.int32)


_register("extract_scale", "(Tensor raw, int mode, int ny, int nx, Tensor xy, int box, int side, Tensor m, int bg_radius, "
                           "bool normalize, bool invert) -> (Tensor, Tensor)", _extract_scale, _extract_scale_fake)


EXTRACT_FILTER_MIN_SIDE = 16                     # sprk_extract_filter: box and side even, 16 <= side <= box <= 1024


def extract_filter_side(box, side, bg_radius=0):
    """Argument check shared by the operator, extract.py and the command line -> side, the output side."""
    if not (EXTRACT_FILTER_MIN_SIDE <= side <= box <= EXTRACT_MAX_BOX) or box % 2 or side % 2:
        raise _lib.SprkError("extract_filter: box %d with output side %d (both even, %d <= side <= box <= %d)"
                             % (box, side, EXTRACT_FILTER_MIN_SIDE, EXTRACT_MAX_BOX))
    if bg_radius < 0:
        raise _lib.SprkError("extract_filter: background radius %d (>= 0)" % bg_radius)
    return side


def extract_filter_shapes(box, side):
    """-> the shapes of the operands w1, w2, w3, w4 and phi: the columns of the matrices rounded up to a multiple of 4"""
    hs, ku = side // 2 + 1, side + 1
    return (2 * hs, _up4(box)), (2 * ku, 2 * box), (2 * side, _up4(2 * ku)), (side, _up4(2 * hs)), (ku, hs)


def _extract_filter_shapes(raw, mode, ny, nx, xy, box, side, w1, w2, w3, w4, phi, bg_radius, max_batch):
    _mode_check("extract_filter", mode)
    extract_filter_side(box, side, bg_radius)
    if max_batch < 0:
        raise _lib.SprkError("extract_filter: max_batch %d (0 = the library's choice, or a positive number of particles)"
                             % max_batch)
    if ny < 1 or nx < 1 or ny * nx >= 1 << 31:
        raise _lib.SprkError("extract_filter: bad image size %dx%d" % (ny, nx))
    _raw_check("extract_filter", raw, mode, ny, nx)
    _xy_check("extract_filter", xy, raw)
    for name, m, shape in zip(("w1", "w2", "w3", "w4", "phi"), (w1, w2, w3, w4, phi), extract_filter_shapes(box, side)):
        _matrix_check("extract_filter", name, m, shape, raw, "filter of ctf.correction_filter" if name == "phi" else
                      "matrix of extract.filter_matrices(%d, %d)" % (box, side))
    return xy.shape[0]


def _extract_filter(raw, mode, ny, nx, xy, box, side, w1, w2, w3, w4, phi, bg_radius, normalize, invert, max_batch):
    """-> (out float32 [P, side, side], status int32 [P]: 0 ok, 1 outside the image, 2 no or flat background)."""
    P = _extract_filter_shapes(raw, mode, ny, nx, xy, box, side, w1, w2, w3, w4, phi, bg_radius, max_batch)
    if not all(t.is_contiguous() for t in (raw, w1, w2, w3, w4, phi)):
        raise _lib.SprkError("extract_filter: raw, the matrices and phi must be contiguous")
    xy = xy.contiguous()
    L = _lib.lib()
    out = _f32(raw, (P, side, side))
    status = torch.empty((P,), dtype=torch.int32, device=raw.device)
    flags = (EXTRACT_NORMALIZE if normalize else 0) | (EXTRACT_INVERT if invert else 0)
    ws = _ws(L.sprk_extract_filter_ws_bytes(P, int(box), int(side), int(max_batch)), raw)
    check(L.sprk_extract_filter(_p(raw), int(mode), int(ny), int(nx), _p(xy), P, int(box), int(side), _p(w1), _p(w2), _p(w3),
                                _p(w4), _p(phi), int(bg_radius), flags, int(max_batch), _p(out), _p(status), _p(ws),
                                ws.numel(), _stream(raw)), "sprk_extract_filter")
    return out, status


def _extract_filter_fake(raw, mode, ny, nx, xy, box, side, w1, w2, w3, w4, phi, bg_radius, normalize, invert, max_batch):
    P = _extract_filter_shapes(raw, mode, ny, nx, xy, box, side, w1, w2, w3, w4, phi, bg_radius, max_batch)
    return raw.new_empty((P, side, side), dtype=torch.float32), raw.new_empty((P,), dtype=torch.int32)


_register("extract_filter", "(Tensor raw, int mode, int ny, int nx, Tensor xy, int box, int side, Tensor w1, Tensor w2, "
                            "Tensor w3, Tensor w4, Tensor phi, int bg_radius, bool normalize, bool invert, int max_batch) "
                            "-> (Tensor, Tensor)", _extract_filter, _extract_filter_fake)


# ---- tiled power spectra (ctf.py: raw MRC samples -> the summed power spectrum of overlapping tiles) --------------------------
PSD_MIN_TILE, PSD_MAX_TILE = 16, 1024            # sprk_psd_tiles: T a multiple of 16 in this range


def psd_tile(T):
    """Argument check shared by the operator, ctf.py and the command line -> T."""
    if not PSD_MIN_TILE <= T <= PSD_MAX_TILE or T % 16:
        raise _lib.SprkError("psd_tiles: tile side %d (a multiple of 16 in %d..%d)" % (T, PSD_MIN_TILE, PSD_MAX_TILE))
    return T


def psd_matrix_shapes(T):
    """-> the shapes of the operands w1 and w2: [roundup(2H, 16), T] and [2T, 2T]"""
    return (_up16(T + 2), T), (2 * T, 2 * T)


def _psd_check(raw, mode, ny, nx, T, w1, w2, max_batch):
    _mode_check("psd_tiles", mode)
    psd_tile(T)
    if not (T <= ny <= INGEST_MAX_SIDE and T <= nx <= INGEST_MAX_SIDE):
        raise _lib.SprkError("psd_tiles: a %dx%d image with tiles of %d (tile <= ny <= %d and tile <= nx <= %d)"
                             % (ny, nx, T, INGEST_MAX_SIDE, INGEST_MAX_SIDE))
    if max_batch < 0:
        raise _lib.SprkError("psd_tiles: max_batch %d (0 = the library's choice, or a positive number of tiles)" % max_batch)
    _raw_check("psd_tiles", raw, mode, ny, nx)
    for name, m, shape in zip(("w1", "w2"), (w1, w2), psd_matrix_shapes(T)):
        _matrix_check("psd_tiles", name, m, shape, raw, "matrix of ctf.dft_matrices(%d)" % T)


def _psd_tiles(raw, mode, ny, nx, T, w1, w2, max_batch):
    """raw: uint8 CUDA tensor holding the file's ny*nx samples; w1, w2: ctf.dft_matrices(T, device) -> P float32
    [T, T/2 + 1], the un-normalised sum of the tiles' power spectra."""
    _psd_check(raw, mode, ny, nx, T, w1, w2, max_batch)
    if not raw.is_contiguous() or not w1.is_contiguous() or not w2.is_contiguous():
        raise _lib.SprkError("psd_tiles: raw, w1 and w2 must be contiguous")
    L = _lib.lib()
    out = _f32(raw, (T, T // 2 + 1))
    ws = _ws(L.sprk_psd_tiles_ws_bytes(int(ny), int(nx), int(T), int(max_batch)), raw)
    check(L.sprk_psd_tiles(_p(raw), int(mode), int(ny), int(nx), int(T), _p(w1), int(w1.shape[1]), _p(w2), int(w2.shape[1]),
                           int(max_batch), _p(out), _p(ws), ws.numel(), _stream(raw)), "sprk_psd_tiles")
    return out


def _psd_tiles_fake(raw, mode, ny, nx, T, w1, w2, max_batch):
    _psd_check(raw, mode, ny, nx, T, w1, w2, max_batch)
    return raw.new_empty((T, T // 2 + 1), dtype=torch.float32)


_register("psd_tiles", "(Tensor raw, int mode, int ny, int nx, int T, Tensor w1, Tensor w2, int max_batch) -> Tensor",
          _psd_tiles, _psd_tiles_fake)


# ---- scores of the 2-D Thon-ring fit (ctf.py: bins of the spectrum x candidates -> three fp64 sums each) --------------------
CTF_MAX_BINS, CTF_MAX_CAND = 1 << 20, 1 << 24    # sprk_ctf_score


def _ctf_check(bins, cand):
    if bins.dtype != torch.float32 or bins.dim() != 2 or bins.shape[0] != 5:
        raise _lib.SprkError("ctf_score: bins must be float32 [5, n] (ctf.fit_bins), got %s %s" % (bins.dtype, tuple(bins.shape)))
    if cand.dtype != torch.float32 or cand.dim() != 2 or cand.shape[1] != 3 or cand.device != bins.device:
        raise _lib.SprkError("ctf_score: cand must be float32 [ncand, 3] on %s, got %s %s on %s"
                             % (bins.device, cand.dtype, tuple(cand.shape), cand.device))
    n, ncand = bins.shape[1], cand.shape[0]
    if not (1 <= n <= CTF_MAX_BINS and 1 <= ncand <= CTF_MAX_CAND):
        raise _lib.SprkError("ctf_score: %d bins and %d candidates (1 <= bins <= %d, 1 <= candidates <= %d)"
                             % (n, ncand, CTF_MAX_BINS, CTF_MAX_CAND))
    ldb = bins.stride(0)
    if bins.stride(1) != 1 or ldb < n or ldb % 4:
        raise _lib.SprkError("ctf_score: the rows of bins must be dense, their stride %d a multiple of 4 and at least the "
                             "%d bins (strides %s)" % (ldb, n, tuple(bins.stride())))
    if not cand.is_contiguous():
        raise _lib.SprkError("ctf_score: cand must be contiguous")


def _ctf_score(bins, cand):
    """bins: float32 CUDA [5, n] (rows b, p, q, r, Y; a view of a wider buffer may have a row stride above n); cand: float32
    [ncand, 3] -> float64 [ncand, 3]: S1, S2, S3 of include/sprk.h."""
    _ctf_check(bins, cand)
    if bins.data_ptr() % 16 or cand.data_ptr() % 16:
        raise _lib.SprkError("ctf_score: bins and cand must start 16-byte aligned")
    L = _lib.lib()
    n, ncand = int(bins.shape[1]), int(cand.shape[0])
    out = torch.empty((ncand, 3), dtype=torch.float64, device=bins.device)
    need = L.sprk_ctf_score_ws_bytes(n, ncand)
    ws = _ws(need, bins)
    check(L.sprk_ctf_score(_p(bins), int(bins.stride(0)), n, _p(cand), ncand, _p(out), _p(ws), ws.numel(), _stream(bins)),
          "sprk_ctf_score")
    return out


def _ctf_score_fake(bins, cand):
    _ctf_check(bins, cand)
    return bins.new_empty((cand.shape[0], 3), dtype=torch.float64)


_register("ctf_score", "(Tensor bins, Tensor cand) -> Tensor", _ctf_score, _ctf_score_fake)


def registered():
    """Names of the operators under torch.ops.sprk (tests)."""
    return tuple(_NAMES)
