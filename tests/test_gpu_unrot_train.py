"""Training at P = 64: the un-rotation of the blind-spot U-Net (Shift2d + chunk + rotate + concat) runs inside its
neighbours: the Winograd kernel of the convolution in front of it stores the un-rotated tensor itself
(sprk_conv2d_fwd_unrot), and its backward runs inside that convolution's activation backward (sprk_unrot_act_bwd);
ops.conv2d(..., unrot_out=UNROT_STORE | UNROT_BWD).  Both fused forms re-order memory accesses only, so every comparison
with the separate kernels is torch.equal; the fp64 comparison uses the budgets of
tests/test_gpu_ops.py::test_conv2d_winograd."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

P = 64
PAD = (2, 0, 1, 1)


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def close(got, want, rel, name):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = want.abs().max().item() + 1e-30
    worst = (got - want).abs().max().item()
    assert worst <= rel * scale, "%s: max err %.3e of scale %.3e (rel %.2e)" % (name, worst, scale, worst / scale)


def _stack_and_grad(B, C, seed):
    """d [4B,C,P,P] with exact zeros and negatives in its interior, f = unrot(d), and a gradient for f."""
    from spr_pick_amd import ops
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(4 * B, C, P, P, generator=g)
    d[torch.rand(d.shape, generator=g) < 0.1] = 0.0
    assert bool((d[:, :, 1:-1, 1:-1] == 0).any()) and bool((d[:, :, 1:-1, 1:-1] < 0).any())
    gf = torch.randn(B, 4 * C, P, P, generator=g)
    d, gf = d.to(dev()), gf.to(dev())
    with torch.no_grad():
        f = ops.unrot4_shift_concat(d)
    return d, f, gf


@pytest.mark.parametrize("B,C", [(2, 96), (5, 96), (5, 3)])
def test_fused_backward_equals_unrot_bwd_then_act_bwd(B, C):
    """gpre and the bias gradient, bit for bit, with the final bias sum finished at once and left pending inside a
    FlatGrads context.  (5, 96): N = 20 images over act_nsplit = 16 workgroups per channel, so some walk two images."""
    from spr_pick_amd import graph_step, ops, torch_ops
    S = torch.ops.sprk
    d, f, gf = _stack_and_grad(B, C, 100 + B + C)
    results = []
    for deferred in (False, True):
        for fused in (False, True):
            bias = torch.nn.Parameter(torch.zeros(C, device=dev()))
            fg = graph_step.FlatGrads([bias])
            fg.begin_step()
            if deferred:
                with fg:
                    gb, defer = ops._grad_dest(bias)
                    assert defer
                    gpre = _run(S, fused, gf, f, d, gb, defer, B, C)
                    assert torch_ops.pending_count(dev()) == 1
                assert torch_ops.pending_count(dev()) == 0
            else:
                gb, defer = ops._grad_dest(bias)
                assert not defer
                gpre = _run(S, fused, gf, f, d, gb, defer, B, C)
            results.append((deferred, fused, gpre, gb.clone()))
    _, _, gpre0, gb0 = results[0]
    assert float(gb0.abs().max()) > 0
    for deferred, fused, gpre, gb in results[1:]:
        what = "%s, %s" % ("fused" if fused else "two kernels", "deferred" if deferred else "immediate")
        assert torch.equal(gpre, gpre0), what + ": gpre differs"
        assert torch.equal(gb, gb0), what + ": bias gradient differs (max |d| %.3e)" % float((gb - gb0).abs().max())
    # Shift2d dropped the last stack row: its gradient is +0
    last = gpre0[:, :, P - 1, :]
    assert bool((last == 0).all()) and not bool(torch.signbit(last).any())


def _run(S, fused, gf, f, d, gb, defer, B, C):
    from spr_pick_amd import ops
    if fused:
        return S.unrot_act_bwd(gf, f, ops.ACT_LEAKY, gb, defer)
    gd = S.unrot4_shift_concat_bwd(gf)
    return S.act_bwd(gd, d, ops.ACT_LEAKY, [4 * B, C, P, P], 0, True, gb, defer, 0)


def _zero_lines(f):
    """Row 0 of the shifted plane is zero: row i = 0 for k = 0, and its images under the other rotations."""
    C = f.shape[1] // 4
    return (bool((f[:, 0:C, 0, :] == 0).all()) and bool((f[:, C:2 * C, :, P - 1] == 0).all())
            and bool((f[:, 2 * C:3 * C, P - 1, :] == 0).all()) and bool((f[:, 3 * C:, :, 0] == 0).all()))


@pytest.mark.parametrize("B,C1", [(2, 96), (5, 96), (2, 10)])
def test_fused_store_equals_conv_then_unrot(B, C1):
    """96 output channels, pad (2,0,1,1), LeakyReLU, bias.  B = 2: 128 tiles, the smallest call the Winograd kernel
    takes; B = 5: 320 tiles on 256 persistent workgroups, so a workgroup's second tile lies in another image and for
    some in another rotation; C1 = 10: a ragged last chunk.  The output tensor is poisoned first: every element of f,
    the zero lines included, must be written by the one launch."""
    from spr_pick_amd import _lib, ops
    g = torch.Generator().manual_seed(31 + B + C1)
    x = torch.randn(4 * B, C1, P, P, generator=g).to(dev())
    w = (torch.randn(96, C1, 3, 3, generator=g) / np.sqrt(C1 * 9)).to(dev())
    b = (torch.randn(96, generator=g) * 0.1).to(dev())
    L = _lib.lib()
    with torch.enable_grad():
        assert ops.unrot_store_eligible(x, w, b, PAD, ops.ACT_LEAKY)
    with torch.no_grad():
        want = ops.unrot4_shift_concat(ops.conv2d(x, w, b, pad=PAD, act=ops.ACT_LEAKY))
        # the allocator hands the next tensor of this size the block freed here: NaNs wherever the kernel does not write
        poison = torch.full_like(want, float("nan"))
        del poison
        geom = ops.make_geom(x, None, w, False, 1, 1, PAD)
        n0, l0 = L.sprk_wino_launch_count(), L.sprk_launch_count()
        ops.conv2d_forward(x, None, w, geom, bias=b, act=ops.ACT_LEAKY)
        n1, l1 = L.sprk_wino_launch_count(), L.sprk_launch_count()
        got = ops.conv2d_forward(x, None, w, geom, bias=b, act=ops.ACT_LEAKY, unrot=True)
        n2, l2 = L.sprk_wino_launch_count(), L.sprk_launch_count()
        torch.cuda.synchronize()
    # one Winograd launch, and as many launches in all as the plain convolution (no fill in front)
    assert n1 == n0 + 1 and n2 == n1 + 1 and l2 - l1 == l1 - l0, (n0, n1, n2, l0, l1, l2)
    assert not bool(torch.isnan(got).any()), "the fused store left elements of f unwritten"
    assert torch.equal(got, want), "max |d| %.3e at %d elements" % (float((got - want).abs().max()), int((got != want).sum()))
    assert _zero_lines(got) and float(got.abs().max()) > 0


def _ref_layer(x, w, b):
    """fp64: ShiftConv2d + LeakyReLU, then Shift2d + chunk + rotate + concat (oracle/networks.py)."""
    from oracle.networks import rot90cw, shift_down
    pt, pb, pl, pr = PAD
    pre = F.conv2d(F.pad(x, (pl, pr, pt, pb)), w, b)
    return pre, lambda y: torch.cat([rot90cw(q, a) for q, a in zip(torch.chunk(shift_down(y), 4, dim=0), (0, 270, 180, 90))], dim=1)


@pytest.mark.parametrize("mode", [3, 2, 1], ids=["store+bwd", "bwd", "store"])
@pytest.mark.parametrize("B,C1", [(2, 96), (5, 96), (2, 10)])
def test_layer_through_autograd(B, C1, mode):
    """conv2d(unrot_out=mode) against unrot4_shift_concat(conv2d(...)): output and all gradients torch.equal.  Launches
    per forward + backward: two fewer with both halves (no un-rotation kernel in either direction, the zero lines are
    written by the convolution's own launch); one fewer with the fused backward alone; as many with the fused store
    alone (its two-kernel backward un-rotates f once more to get the mask back).  With both halves also against the
    fp64 statement of the layer."""
    from spr_pick_amd import _lib, ops
    g = torch.Generator().manual_seed(7 + B + C1)
    x = torch.randn(4 * B, C1, P, P, generator=g)
    w = torch.randn(96, C1, 3, 3, generator=g) / np.sqrt(C1 * 9)
    b = torch.randn(96, generator=g) * 0.1
    gf = torch.randn(B, 384, P, P, generator=g)
    L = _lib.lib()
    out = []
    for fused in (False, True):
        xl, wl, bl = (t.to(dev()).requires_grad_(True) for t in (x, w, b))
        assert ops.unrot_train_eligible(xl, ops.ACT_LEAKY) and ops.unrot_store_eligible(xl, wl, bl, PAD, ops.ACT_LEAKY)
        torch.cuda.synchronize()
        n0 = L.sprk_launch_count()
        if fused:
            f = ops.conv2d(xl, wl, bl, pad=PAD, act=ops.ACT_LEAKY, unrot_out=mode)
        else:
            f = ops.unrot4_shift_concat(ops.conv2d(xl, wl, bl, pad=PAD, act=ops.ACT_LEAKY))
        f.backward(gf.to(dev()))
        torch.cuda.synchronize()
        out.append((f.detach(), xl.grad, wl.grad, bl.grad, L.sprk_launch_count() - n0))
    for a, c, name in zip(out[0][:4], out[1][:4], ("f", "gx", "gw", "gb")):
        assert torch.equal(a, c), "%s differs (max |d| %.3e)" % (name, float((a - c).abs().max()))
    assert out[1][4] == out[0][4] - {3: 2, 2: 1, 1: 0}[mode], (out[0][4], out[1][4])
    f = out[1][0]
    assert _zero_lines(f)
    if B != 2 or mode != 3:
        return      # (the fp64 convolution of the larger stack takes the CPU longer than the rest of this file)
    # fp64 reference, backward with the sign pattern of the GPU output (tests/test_gpu_ops.py)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    pre, unrot = _ref_layer(xr, wr, br)
    close(f, unrot(F.leaky_relu(pre, 0.1)), 2e-5, "f")
    with torch.no_grad():
        y_gpu = ops.conv2d(x.to(dev()), w.to(dev()), b.to(dev()), pad=PAD, act=ops.ACT_LEAKY).cpu()
    unrot(torch.where(y_gpu > 0, pre, pre * 0.1)).backward(gf.double())
    close(out[1][1], xr.grad, 5e-5, "gx")
    close(out[1][2], wr.grad, 5e-5, "gw")
    close(out[1][3], br.grad, 5e-5, "gb")


def _blindspot_net(seed=3):
    from spr_pick_amd import networks
    torch.manual_seed(seed)
    net = networks.DualNetwork(in_channels=1, out_channels=2, blindspot=True, zero_output_weights=False).to(dev())
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.05)
    return net


@pytest.mark.parametrize("what", ["P32", "P128", "bf16", "no_grad"])
def test_fallbacks_take_the_old_path(what):
    """Other patch sizes, 16-bit operands and no_grad: the eligibility query is false, the network runs the two-kernel
    path and its results do not depend on the switch."""
    from spr_pick_amd import _lib, networks, ops
    p = {"P32": 32, "P128": 128}.get(what, 64)
    dtype = _lib.DT_BF16 if what == "bf16" else 0
    x = torch.randn(4, 96, p, p, device=dev())
    if what == "no_grad":
        with torch.no_grad():
            assert not ops.unrot_train_eligible(x, ops.ACT_LEAKY, dtype)
    else:
        assert not ops.unrot_train_eligible(x, ops.ACT_LEAKY, dtype)
    assert not ops.unrot_train_eligible(x, ops.ACT_NONE, 0)
    w, b = torch.randn(96, 96, 3, 3, device=dev()), torch.zeros(96, device=dev())
    if what == "no_grad":
        with torch.no_grad():
            assert not ops.unrot_store_eligible(x, w, b, PAD, ops.ACT_LEAKY, dtype)
    else:
        # (P = 32 at 4 images is too small for the Winograd kernel as well; at 128 images it takes it, still no store)
        x_big = x if p != 32 else torch.randn(128, 96, p, p, device=dev())
        assert not ops.unrot_store_eligible(x_big, w, b, PAD, ops.ACT_LEAKY, dtype)
    assert not ops.unrot_store_eligible(torch.randn(8, 96, P, P, device=dev()), w, b, PAD, ops.ACT_NONE, 0)
    assert not ops.unrot_store_eligible(torch.randn(8, 96, P, P, device=dev()), w[:32], b[:32], PAD, ops.ACT_LEAKY, 0)
    assert bool(_lib.lib().sprk_unrot_act_bwd_eligible(1, 96, p, ops.ACT_LEAKY)) == (p == 64)
    net = _blindspot_net()
    if what == "bf16":
        networks.set_conv_dtype(net, "bf16")
    inp = torch.rand(1, 1, p, p, device=dev())
    res = []
    for switch in (True, False):
        networks.FUSE_UNROT_BWD = networks.FUSE_UNROT_STORE = switch
        try:
            for q in net.parameters():
                q.grad = None
            if what == "no_grad":
                with torch.no_grad():
                    res.append([net(inp)])
            else:
                o = net(inp)
                o.square().mean().backward()
                res.append([o.detach()] + [q.grad.clone() for q in net.parameters()])
        finally:
            networks.FUSE_UNROT_BWD = networks.FUSE_UNROT_STORE = True
    for a, c in zip(*res):
        assert torch.equal(a, c)


def test_dualnetwork_training_pass_switch_on_equals_off_and_replay_equals_eager():
    """One blind-spot DualNetwork forward + backward at batch 2, patch 64: outputs and every parameter gradient are
    torch.equal whichever of the two switches are on (off/off is the separate un-rotation operator: two launches more
    than on/on); with both on, a HIP-graph replay of the pass equals the eager pass."""
    from spr_pick_amd import _lib, networks
    net = _blindspot_net()
    params = list(net.parameters())
    inp = torch.rand(2, 1, P, P, device=dev())
    L = _lib.lib()

    def run():
        for q in params:
            q.grad = None
        o = net(inp)
        o.square().mean().backward()
        return o

    # Every pass of this network, eager and captured, runs on ONE side stream: autograd binds a parameter's
    # AccumulateGrad node to the stream of its first use, and a node born on another stream drags that stream into the
    # capture, which hipStreamEndCapture does not survive (graph_step.GraphedTrainStep._eager).
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    res, launches = [], []
    with torch.cuda.stream(s):
        for store, bwd in ((False, False), (True, False), (False, True), (True, True)):
            networks.FUSE_UNROT_STORE, networks.FUSE_UNROT_BWD = store, bwd
            try:
                torch.cuda.synchronize()
                n0 = L.sprk_launch_count()
                o = run()
                torch.cuda.synchronize()
                launches.append(L.sprk_launch_count() - n0)
                res.append([o.detach().clone()] + [q.grad.clone() for q in params])
            finally:
                networks.FUSE_UNROT_STORE = networks.FUSE_UNROT_BWD = True
            del o           # no older autograd graph stays alive into the capture
    torch.cuda.current_stream().wait_stream(s)
    assert [launches[0] - n for n in launches] == [0, 0, 1, 2], launches
    for k in (1, 2, 3):
        for i, (a, c) in enumerate(zip(res[0], res[k])):
            assert torch.equal(a, c), "switches %d: tensor %d differs (max |d| %.3e)" % (k, i, float((a - c).abs().max()))
    # replay: capture the same pass on that stream (the eager passes above were its warm-up), poison, replay, compare
    for q in params:
        q.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        o = net(inp)
        o.square().mean().backward()
    grads = [q.grad for q in params]
    for t in [o] + grads:
        t.detach().fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for i, (a, c) in enumerate(zip([o.detach()] + grads, res[3])):
        assert torch.equal(a, c), "replay: tensor %d differs from the eager pass" % i
