"""The whole-tensor gradient checker (tests/oracle_parity.py) can fail: fed the fp64 oracle's own gradients at the initial
weights (B = 2, the smallest batch the detector's BatchNorm trains on: its last planes are 1x1; one joint train step
on the CPU) and their fp32-rounded copy it accepts both, with the fp32 oracle as
yardstick; a wrong gradient of the kinds a broken kernel produces is rejected — one output channel scaled by 1.01, two
input channels swapped, mirrored 3x3 taps, one BatchNorm gamma gradient zeroed — and so is a gradient-free parameter that
gained a gradient or lost its own."""
import pytest
import torch

import oracle_parity


@pytest.fixture(scope="module")
def grads(oracle_state):
    from oracle import pipeline
    g = torch.Generator().manual_seed(3)
    inp = (torch.rand(2, 1, 64, 64, generator=g) * 255).round() / 255
    tgt = torch.tensor([[1.0], [-1.0]])
    eps, eps_f = torch.randn(2, 1, 64, 64, generator=g), torch.randn(2, 1, 64, 64, generator=g)

    def run(dt):
        sd = {k: (v.clone().to(dt) if v.is_floating_point() else v.clone()) for k, v in oracle_state.items()}
        for k, v in sd.items():
            if v.is_floating_point() and "running" not in k:
                v.requires_grad_(True)
        r = pipeline.joint_pipeline(sd, inp.to(dt), tgt.to(dt), 0.75, 0.01, True, eps.to(dt), eps_f.to(dt), 0.3)
        r["LOSS"].mean().backward()
        return {k: (None if v.grad is None else v.grad.detach().clone()) for k, v in sd.items()
                if v.is_floating_point() and "running" not in k}

    return run(torch.float64), run(torch.float32)


def _weight3(ref):
    """The 3x3 weight gradient with the largest max|g| (the checker's absolute floor must not hide the change)."""
    names = [n for n, g in ref.items() if g is not None and g.dim() == 4 and g.shape[-1] == 3 and g.shape[1] >= 2]
    return max(names, key=lambda n: float(ref[n].abs().max()))


def _rejects(ref, ref32, name, bad):
    got = {k: (None if v is None else v.to(torch.float32)) for k, v in ref.items()}
    got[name] = bad
    # a failure, not a pass through the yardstick: the fp32 oracle's own deviation is rounding-level here
    return bool(oracle_parity.grad_report(got, ref, ref32)["failures"])


def test_checker_accepts_the_oracle_and_its_fp32_rounding(grads):
    ref, ref32 = grads
    assert sum(g is None for g in ref.values()) >= 1           # never-grad parameters exist on this path
    assert {k for k, v in ref.items() if v is None} == {k for k, v in ref32.items() if v is None}
    rep = oracle_parity.check_grads(ref, ref, ref32)
    assert rep["loose"] == 0 and all(r["err"] == 0 for r in rep["rows"].values())
    rounded = {k: (None if v is None else v.to(torch.float32)) for k, v in ref.items()}
    rep = oracle_parity.check_grads(rounded, ref, ref32)
    assert rep["numel"] > 2_000_000 and not rep["yardstick"]
    # the fp32 oracle itself passes the base rule at the initial weights (the golden tests' premise)
    oracle_parity.check_grads(ref32, ref, None)


def test_checker_rejects_a_scaled_output_channel(grads):
    ref, ref32 = grads
    n = _weight3(ref)
    g = ref[n].clone()
    co = int(g.abs().flatten(1).max(1).values.argmax())
    g[co] *= 1.01
    assert _rejects(ref, ref32, n, g.float()), n


def test_checker_rejects_swapped_input_channels(grads):
    ref, ref32 = grads
    n = _weight3(ref)
    g = ref[n].clone()
    g[:, [0, 1]] = g[:, [1, 0]]
    assert _rejects(ref, ref32, n, g.float()), n


def test_checker_rejects_mirrored_taps(grads):
    ref, ref32 = grads
    n = _weight3(ref)
    assert _rejects(ref, ref32, n, ref[n].flip(-1).float()), n


def test_checker_rejects_a_zeroed_batchnorm_gamma_gradient(grads):
    ref, ref32 = grads
    gammas = [n for n, g in ref.items() if g is not None and "bn" in n and n.endswith(".weight")]
    assert gammas
    n = max(gammas, key=lambda k: float(ref[k].abs().max()))
    g = ref[n].clone()
    g[int(g.abs().argmax())] = 0
    assert _rejects(ref, ref32, n, g.float()), n


def test_checker_rejects_a_changed_set_of_parameters_with_gradients(grads):
    ref, ref32 = grads
    got = {k: (None if v is None else v.to(torch.float32)) for k, v in ref.items()}
    nograd = next(k for k, v in ref.items() if v is None)
    extra = dict(got)
    extra[nograd] = torch.zeros(1)
    assert oracle_parity.grad_report(extra, ref, ref32)["failures"]
    lost = dict(got)
    lost[_weight3(ref)] = None
    assert oracle_parity.grad_report(lost, ref, ref32)["failures"]


def test_yardstick_admits_k_times_the_fp32_oracles_deviation_under_a_cap():
    """Only where the fp32 oracle itself misses the base rule, within K of its deviation and under CAP."""
    ref = {"t": torch.linspace(-1, 1, 1000, dtype=torch.float64)}
    ref32 = {"t": ref["t"] + 5e-3}                  # an ill-conditioned tensor: the fp32 oracle itself misses the base rule
    rep = oracle_parity.grad_report({"t": ref["t"] + 1.5e-2}, ref, ref32)          # 3x the fp32 oracle's deviation
    assert not rep["failures"] and rep["yardstick"] == ["t"]
    with pytest.raises(AssertionError):
        oracle_parity.check_grads({"t": ref["t"] + 1.5e-2}, ref, ref32)           # the caller allows no such tensor
    assert oracle_parity.grad_report({"t": ref["t"] + 2.5e-2}, ref, ref32)["failures"]        # 5x: beyond K
    wide = {"t": ref["t"] + 1e-2}
    assert oracle_parity.grad_report({"t": ref["t"] + 3.5e-2}, ref, wide)["failures"]         # 3.5x but beyond CAP
    assert oracle_parity.grad_report({"t": ref["t"] + 1.5e-2}, ref, None)["failures"]         # no yardstick given
    # a tensor the fp32 oracle itself gets right has no yardstick, however close to it the error is
    fine = {"t": ref["t"] + 1e-3}
    assert oracle_parity.grad_report({"t": ref["t"] + 3.5e-3}, ref, fine)["failures"]
    # the fp32 oracle is evaluated only when a tensor misses the base rule
    calls = []
    lazy = lambda: calls.append(1) or ref32
    assert not oracle_parity.grad_report({"t": ref["t"] + 1e-3}, ref, lazy)["failures"] and not calls
    assert oracle_parity.grad_report({"t": ref["t"] + 1.5e-2}, ref, lazy)["yardstick"] == ["t"] and calls == [1]
    o = oracle_parity.output_report(ref["t"] + 2e-4, ref["t"], ref32["t"])
    assert o["ok"] and o["yardstick"]
    o = oracle_parity.output_report(ref["t"] + 5e-5, ref["t"], ref32["t"])
    assert o["ok"] and not o["yardstick"]
    assert not oracle_parity.output_report(ref["t"] + 2.5e-2, ref["t"], ref32["t"])["ok"]
    assert not oracle_parity.output_report(ref["t"] + 2e-4, ref["t"], ref["t"] + 5e-5)["ok"]     # fp32 oracle within rel
    assert not oracle_parity.output_report(ref["t"] + 5e-5, ref["t"], lambda: 1 / 0)["yardstick"]   # never evaluated
