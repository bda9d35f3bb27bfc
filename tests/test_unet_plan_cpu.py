"""CPU: the forward plan of the U-Nets — which functional operator is called with which arguments — is pinned.

The networks are run under FakeTensorMode on fake ``cuda`` tensors with ``ops.conv2d``, ``ops.shift_maxpool2``,
``ops.rot4_stack``, ``ops.unrot4_shift_concat``, ``ops.head1x1`` and ``ops.head1x1_unrot`` wrapped by a recorder that
calls through.  Every call is recorded with the shapes and dtypes of its tensor arguments and every other argument, and
the list is compared with tests/golden/unet_plan.json (recorded with ``python tests/test_unet_plan_cpu.py --record``).
The host-side queries the plan depends on (sprk_conv2d_storage16, sprk_conv2d_bwd_data_mask_fused,
sprk_conv2d_fwd_unrot_eligible) plan for 256 compute units when there is no device, the MI355X's own count, so the
fixture is the same with and without a GPU.

Independently of the fixture, every plan is checked for the promise pairs of the fused activation backward
(``ops.conv2d``: premasked / x_act): a producer called with ``premasked`` has exactly one consumer of its output (by
tensor identity), which takes it as its first input and was called with ``x_act`` equal to the producer's ``act``; and
every ``x_act`` other than ACT_NONE is backed by such a producer.

A backward pass under fake ``cuda`` tensors needs a device context, so the backward is pinned on the GPU
(tests/test_gpu_unet_trace.py)."""
import contextlib
import inspect
import json
import os
import sys
import warnings

import pytest
import torch

from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "unet_plan.json")
RECORDED = ("conv2d", "shift_maxpool2", "rot4_stack", "unrot4_shift_concat", "head1x1", "head1x1_unrot")

# name: (network, conv dtype of set_conv_dtype or None, input shape, grad enabled, module switches set to False)
CONFIGS = {
    "bs-f32-2x64": ("bs", None, (2, 1, 64, 64), True, ()),
    "bs-f32-1x32": ("bs", None, (1, 1, 32, 32), True, ()),
    "bs-f32-32x64": ("bs", None, (32, 1, 64, 64), True, ()),
    "deep-f32-32x64": ("deep", None, (32, 1, 64, 64), True, ()),
    "shallow-f32-32x64": ("shallow", None, (32, 1, 64, 64), True, ()),
    "deep-f32-2x32": ("deep", None, (2, 1, 32, 32), True, ()),
    "shallow-f32-2x32": ("shallow", None, (2, 1, 32, 32), True, ()),
    "bs-bf16-2x64": ("bs", "bf16", (2, 1, 64, 64), True, ()),
    "bs-f16-2x64": ("bs", "f16", (2, 1, 64, 64), True, ()),
    "bs-bf16operands-2x64": ("bs", "bf16/operands", (2, 1, 64, 64), True, ()),
    "shallow-bf16-32x64": ("shallow", "bf16", (32, 1, 64, 64), True, ()),
    "nograd-bs-f32-1x64": ("bs", None, (1, 1, 64, 64), False, ()),
    "nograd-shallow-mixed16-1x64": ("shallow", "mixed16", (1, 1, 64, 64), False, ()),
    "nograd-deep-f32-1x64": ("deep", None, (1, 1, 64, 64), False, ()),
    "nograd-bs-f32-1x64-no-FUSED_HEAD": ("bs", None, (1, 1, 64, 64), False, ("FUSED_HEAD",)),
    "nograd-bs-f32-1x64-no-FUSED_UNROT": ("bs", None, (1, 1, 64, 64), False, ("FUSED_UNROT",)),
    "nograd-shallow-f32-1x64-no-FUSED_HEAD": ("shallow", None, (1, 1, 64, 64), False, ("FUSED_HEAD",)),
    "bs-f32-2x64-no-FUSE_ACT_BWD": ("bs", None, (2, 1, 64, 64), True, ("FUSE_ACT_BWD",)),
    "shallow-f32-32x64-no-FUSE_ACT_BWD": ("shallow", None, (32, 1, 64, 64), True, ("FUSE_ACT_BWD",)),
    "bs-f32-2x64-no-FUSE_UNROT_STORE": ("bs", None, (2, 1, 64, 64), True, ("FUSE_UNROT_STORE",)),
    "bs-f32-2x64-no-FUSE_UNROT_BWD": ("bs", None, (2, 1, 64, 64), True, ("FUSE_UNROT_BWD",)),
    "bs-f32-2x64-no-FUSE_UNROT_STORE-no-FUSE_UNROT_BWD": ("bs", None, (2, 1, 64, 64), True,
                                                          ("FUSE_UNROT_STORE", "FUSE_UNROT_BWD")),
    "shallow-f32-32x64-no-FUSE_HEAD_MASK_IN": ("shallow", None, (32, 1, 64, 64), True, ("FUSE_HEAD_MASK_IN",)),
    "shallow-f32-32x64-no-FUSE_HEAD_MASK_12": ("shallow", None, (32, 1, 64, 64), True, ("FUSE_HEAD_MASK_12",)),
    "shallow-f32-32x64-no-FUSE_HEAD_MASK_23": ("shallow", None, (32, 1, 64, 64), True, ("FUSE_HEAD_MASK_23",)),
    "deep-f32-32x64-no-FUSE_HEAD_MASK_IN": ("deep", None, (32, 1, 64, 64), True, ("FUSE_HEAD_MASK_IN",)),
    "bs-f32-32x64-no-FUSE_HEAD_MASK_12": ("bs", None, (32, 1, 64, 64), True, ("FUSE_HEAD_MASK_12",)),
    "bs-f32-32x64-no-FUSE_HEAD_MASK_23": ("bs", None, (32, 1, 64, 64), True, ("FUSE_HEAD_MASK_23",)),
}


def _describe(v):
    if torch.is_tensor(v):
        return "%s%s" % (str(v.dtype).replace("torch.", ""), list(v.shape))
    if isinstance(v, torch.nn.Module):
        return "module%s" % (list(v.weight.shape),)
    if isinstance(v, (tuple, list)):
        return [_describe(e) for e in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    raise TypeError("unrecorded argument type %r" % (type(v),))


class Recorder:
    """Wraps the functional operators of ``ops`` the networks call; keeps every call's arguments and output alive, so
    that tensor identity tells producers and consumers apart."""

    def __init__(self, ops):
        self.ops, self.calls, self._saved = ops, [], {}

    def __enter__(self):
        for name in RECORDED:
            fn = getattr(self.ops, name)
            self._saved[name] = fn
            setattr(self.ops, name, self._wrap(name, fn))
        return self

    def __exit__(self, *exc):
        for name, fn in self._saved.items():
            setattr(self.ops, name, fn)
        return False

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        def wrapped(*a, **kw):
            b = sig.bind(*a, **kw)
            b.apply_defaults()
            out = fn(*a, **kw)
            self.calls.append((name, dict(b.arguments), out))
            return out
        return wrapped

    def plan(self):
        return [[name, {k: _describe(v) for k, v in args.items()}, _describe(out)] for name, args, out in self.calls]


def check_pairs(calls, ACT_NONE=0):
    """The promise pairs of one recorded plan (see the module docstring)."""
    def inputs(args):
        return [v for v in args.values() if torch.is_tensor(v)]

    def first_input(args):
        return next(iter(args.values()))

    n = 0
    for i, (name, args, out) in enumerate(calls):
        if args.get("premasked"):
            users = [j for j, (_, a, _) in enumerate(calls) if any(t is out for t in inputs(a))]
            assert len(users) == 1, "call %d (%s) is premasked but its output has %d consumers" % (i, name, len(users))
            cname, cargs, _ = calls[users[0]]
            assert first_input(cargs) is out, "call %d: its consumer %s does not take it as its first input" % (i, cname)
            assert cargs.get("x_act", ACT_NONE) == args["act"] != ACT_NONE, (
                "call %d (%s, act %d) is premasked, but its consumer %s was called with x_act = %r"
                % (i, name, args["act"], cname, cargs.get("x_act")))
            n += 1
        if args.get("x_act", ACT_NONE) != ACT_NONE:
            x = first_input(args)
            prod = [(a.get("premasked"), a.get("act")) for _, a, o in calls[:i] if o is x]
            assert prod == [(True, args["x_act"])], (
                "call %d (%s) has x_act = %d, but the producer of its input says %r" % (i, name, args["x_act"], prod))
    return n


@contextlib.contextmanager
def _switched_off(networks, names):
    saved = {n: getattr(networks, n) for n in names}
    try:
        for n in names:
            setattr(networks, n, False)
        yield
    finally:
        for n, v in saved.items():
            setattr(networks, n, v)


def make_net(kind, device=None):
    from spr_pick_amd import networks
    if kind == "shallow":
        net = networks.DualNetworkShallow(in_channels=1, out_channels=1, blindspot=False)
    else:
        net = networks.DualNetwork(in_channels=1, out_channels=2, blindspot=kind == "bs", zero_output_weights=False)
    return net if device is None else net.to(device)


def run_config(name):
    """-> the Recorder of one forward pass of configuration ``name`` on fake cuda tensors."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    from spr_pick_amd import networks, ops
    kind, conv_dtype, shape, grad, off = CONFIGS[name]
    with FakeTensorMode():
        with torch.device("cuda"):      # (a module of fake tensors cannot be moved: its parameters are created there)
            net = make_net(kind)
        if conv_dtype is not None:
            networks.set_conv_dtype(net, conv_dtype)
        x = torch.empty(shape, device="cuda", requires_grad=grad)
        with _switched_off(networks, off), torch.set_grad_enabled(grad), Recorder(ops) as rec:
            net(x)
    return rec


@pytest.fixture(scope="module")
def fixture_plans():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_the_configurations(fixture_plans):
    assert sorted(fixture_plans) == sorted(CONFIGS)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_forward_plan(name, fixture_plans):
    with warnings.catch_warnings():
        # eligibility queries must not read data pointers (of fake tensors: deprecated, soon an error)
        warnings.filterwarnings("error", module=r"spr_pick_amd(\..*)?$")
        rec = run_config(name)
    check_pairs(rec.calls)
    got = json.loads(json.dumps(rec.plan()))
    want = fixture_plans[name]
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "call %d differs:\n got  %s\n want %s" % (i, g, w)


def test_known_premasked_counts():
    """What the untouched plans were measured to hold: 11 premasked producers in the blind-spot net at [2,1,64,64], 7 in
    the shallow net at [2,1,32,32] (its head links unfused), and the three head links on top at [32,1,64,64]."""
    assert check_pairs(run_config("bs-f32-2x64").calls) == 11
    assert check_pairs(run_config("shallow-f32-2x32").calls) == 7
    assert check_pairs(run_config("shallow-f32-32x64").calls) == 10
    assert check_pairs(run_config("bs-f32-2x64-no-FUSE_ACT_BWD").calls) == 0


def test_pair_check_catches_a_broken_promise():
    """The check itself: a consumer that was not told, and a consumer told without a producer's promise."""
    a, b, c = torch.empty(1), torch.empty(1), torch.empty(1)
    good = [("conv2d", {"x": a, "act": 1, "x_act": 0, "premasked": True}, b),
            ("conv2d", {"x": b, "act": 1, "x_act": 1, "premasked": False}, c)]
    assert check_pairs(good) == 1
    untold = [good[0], ("conv2d", {"x": b, "act": 1, "x_act": 0, "premasked": False}, c)]
    unpromised = [("conv2d", {"x": a, "act": 1, "x_act": 0, "premasked": False}, b), good[1]]
    two_users = good + [("shift_maxpool2", {"x": b, "shift": 0, "x_act": 1}, torch.empty(1))]
    for bad in (untold, unpromised, two_users):
        with pytest.raises(AssertionError):
            check_pairs(bad)


def _record():
    plans = {}
    for name in CONFIGS:
        rec = run_config(name)
        check_pairs(rec.calls)
        plans[name] = rec.plan()
    with open(FIXTURE, "w") as f:
        f.write("{\n")
        for k, (name, plan) in enumerate(plans.items()):
            f.write(" %s: [\n" % json.dumps(name))
            f.write(",\n".join("  " + json.dumps(c) for c in plan))
            f.write("\n ]%s\n" % ("," if k + 1 < len(plans) else ""))
        f.write("}\n")
    print("recorded %d plans, %d calls -> %s" % (len(plans), sum(len(p) for p in plans.values()), FIXTURE))


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_unet_plan_cpu.py --record")
    _record()
