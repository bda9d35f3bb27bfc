"""GPU: the operator trace and the results of a U-Net forward + backward are pinned, bit for bit.

A TorchDispatchMode records every ``torch.ops.sprk.*`` call of one forward and one backward pass: the operator's name,
its integer / bool / float arguments in full (the 16 geometry integers with their dtype bits among them), and shape,
dtype and strides of every tensor argument (stored as a digest per call, to keep the fixture small).  The output, the
input gradient and every parameter gradient (``named_parameters()`` order, None recorded as such) are stored as sha256
of their bytes.  Weights, inputs and the output gradient are drawn from a seeded CPU generator and copied to the device.
Compared with tests/golden/unet_trace.json, which ``python tests/test_gpu_unet_trace.py --record [FILE]`` writes (every
configuration is run twice there, and both the trace and the checksums must reproduce).

Together with tests/test_unet_plan_cpu.py (the forward plan, on the CPU) this pins what the Python plumbing around the
kernels does: a change there that alters which operator runs, with which arguments, in which order, or any bit of a
result, fails here."""
import contextlib
import hashlib
import json
import os
import sys

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from conftest import GOLDEN
from test_unet_plan_cpu import _switched_off, make_net

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "unet_trace.json")

# name: (network, conv dtype of set_conv_dtype or None, input shape, grad enabled, inside a FlatGrads context, switches off)
CONFIGS = {
    "bs-f32-2x64": ("bs", None, (2, 1, 64, 64), True, False, ()),
    "bs-f32-1x32": ("bs", None, (1, 1, 32, 32), True, False, ()),
    "deep-f32-32x64": ("deep", None, (32, 1, 64, 64), True, False, ()),
    "shallow-f32-32x64": ("shallow", None, (32, 1, 64, 64), True, False, ()),
    "bs-bf16-2x64": ("bs", "bf16", (2, 1, 64, 64), True, False, ()),
    "bs-f16-2x64": ("bs", "f16", (2, 1, 64, 64), True, False, ()),
    "shallow-bf16operands-2x32": ("shallow", "bf16/operands", (2, 1, 32, 32), True, False, ()),
    "bs-f32-2x64-flatgrads": ("bs", None, (2, 1, 64, 64), True, True, ()),
    "shallow-f32-32x64-flatgrads": ("shallow", None, (32, 1, 64, 64), True, True, ()),
    "nograd-bs-f32-1x64": ("bs", None, (1, 1, 64, 64), False, False, ()),
    "nograd-shallow-mixed16-1x64": ("shallow", "mixed16", (1, 1, 64, 64), False, False, ()),
    "nograd-bs-f32-1x64-no-FUSED_HEAD": ("bs", None, (1, 1, 64, 64), False, False, ("FUSED_HEAD",)),
    "nograd-bs-f32-1x64-no-FUSED_UNROT": ("bs", None, (1, 1, 64, 64), False, False, ("FUSED_UNROT",)),
}


def _tensor_desc(t):
    return "%s%s/%s" % (str(t.dtype).replace("torch.", ""), list(t.shape), list(t.stride()))


class SprkTrace(TorchDispatchMode):
    """calls: [name, non-tensor arguments (a tensor's place holds "T"), digest of the tensor descriptions];
    tensors: the descriptions themselves, per call (for the failure message)."""

    def __init__(self):
        super().__init__()
        self.calls, self.tensors = [], []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = func._schema.name
        if name.startswith("sprk::"):
            descs, plain = [], []
            for a in list(args) + [kwargs[k] for k in sorted(kwargs)]:
                if torch.is_tensor(a):
                    descs.append(_tensor_desc(a))
                    plain.append("T")
                elif a is None or isinstance(a, (bool, int, float)):
                    plain.append(a)
                elif isinstance(a, (list, tuple)) and all(isinstance(e, (bool, int)) for e in a):
                    plain.append([int(e) for e in a])
                else:
                    raise TypeError("%s: unrecorded argument type %r" % (name, type(a)))
            self.calls.append([name[len("sprk::"):], plain, hashlib.sha256(" ".join(descs).encode()).hexdigest()[:12]])
            self.tensors.append(descs)
        return func(*args, **kwargs)


def _sha(t):
    if t is None:
        return None
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _seeded_net(kind, seed):
    g = torch.Generator().manual_seed(seed)
    net = make_net(kind)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=g) / (p.shape[1] * p.shape[2] * p.shape[3]) ** 0.5)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return net.to("cuda:0"), g


def run_config(name):
    """-> (SprkTrace, {"out": sha, "gx": sha, "grads": {parameter name: sha or None}})"""
    from spr_pick_amd import graph_step, networks
    assert torch.cuda.is_available(), "these tests need the MI355X"
    kind, conv_dtype, shape, grad, flat, off = CONFIGS[name]
    net, g = _seeded_net(kind, 1234)
    if conv_dtype is not None:
        networks.set_conv_dtype(net, conv_dtype)
    x = torch.rand(shape, generator=g).to("cuda:0").requires_grad_(grad)
    sums = {}
    with _switched_off(networks, off), torch.set_grad_enabled(grad), SprkTrace() as trace:
        if not grad:
            out = net(x)
        else:
            fg = graph_step.FlatGrads(list(net.parameters())) if flat else None
            if fg is not None:
                fg.begin_step()
            with (fg if fg is not None else contextlib.nullcontext()):
                out = net(x)
                out.backward(torch.randn(out.shape, generator=g).to("cuda:0"))
            sums["gx"] = _sha(x.grad)
            sums["grads"] = {n: _sha(p.grad) for n, p in net.named_parameters()}
        torch.cuda.synchronize()
        sums["out"] = _sha(out)
    return trace, sums


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_the_configurations(recorded):
    assert sorted(recorded) == sorted(CONFIGS)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_trace_and_checksums(name, recorded):
    trace, sums = run_config(name)
    want = recorded[name]
    got = json.loads(json.dumps(trace.calls))
    assert [c[0] for c in got] == [c[0] for c in want["calls"]], "the operator sequence differs"
    for i, (a, b) in enumerate(zip(got, want["calls"])):
        assert a == b, "call %d differs:\n got  %s %s\n want %s" % (i, a, trace.tensors[i], b)
    if CONFIGS[name][4]:
        assert [c[0] for c in got].count("reduce_pending") == 1
    assert sums["out"] == want["sums"]["out"], "the output differs"
    if CONFIGS[name][3]:
        assert sums["gx"] == want["sums"]["gx"], "the input gradient differs"
        assert list(sums["grads"]) == list(want["sums"]["grads"])
        bad = [n for n in sums["grads"] if sums["grads"][n] != want["sums"]["grads"][n]]
        assert not bad, "parameter gradients differ: %s" % bad
        assert sum(v is not None for v in sums["grads"].values()) > 20


def _record(path):
    res = {}
    for name in CONFIGS:
        trace, sums = run_config(name)
        trace2, sums2 = run_config(name)
        assert trace.calls == trace2.calls, "%s: the trace does not reproduce" % name
        assert sums == sums2, "%s: the checksums do not reproduce" % name
        res[name] = {"calls": trace.calls, "sums": sums}
        print("%s: %d calls, reproduced" % (name, len(trace.calls)), flush=True)
    with open(path, "w") as f:
        f.write("{\n")
        for k, (name, r) in enumerate(res.items()):
            f.write(" %s: {\n  \"sums\": %s,\n  \"calls\": [\n" % (json.dumps(name), json.dumps(r["sums"])))
            f.write(",\n".join("   " + json.dumps(c) for c in r["calls"]))
            f.write("\n  ]\n }%s\n" % ("," if k + 1 < len(res) else ""))
        f.write("}\n")
    print("recorded %d configurations -> %s" % (len(res), path))


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"] or len(sys.argv) > 3:
        sys.exit("usage: python tests/test_gpu_unet_trace.py --record [FILE]")
    _record(sys.argv[2] if len(sys.argv) == 3 else FIXTURE)
