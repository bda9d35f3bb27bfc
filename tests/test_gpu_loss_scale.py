"""GPU: dynamic loss scaling (graph_step.LossScaler, csrc/scale.hip, sprk_adam_multi_skip).

  * the unscale + non-finite check against torch, bit for bit, at awkward lengths and alignments;
  * skip-aware Adam: a set flag leaves everything untouched, a clear flag equals sprk_adam_multi bit for bit;
  * the device schedule against GradScaler's rule (tests/test_loss_scale_cpu.py);
  * a power-of-two scale is exact: replayed f32 / bf16 steps with and without 2^16 give identical gradients and
    identical parameters after Adam;
  * f16 gradients with the loss scale are at least as accurate as bf16's on the sigma-net and the U-Net of a
    model trained for 1000 steps, where unscaled f16 is not;
  * an overflowing step is skipped, and the dynamic scale backs off until a step is taken;
  * the trainer: checkpoint, resume and metrics of a loss-scaled f16 run."""
import os

import numpy as np
import pytest
import torch

from test_gpu_graph_step import _denoiser
from test_loss_scale_cpu import gradscaler_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, offset", [(1, 0), (3, 0), (1023, 0), (2_106_950, 0), (1023, 1), (4099, 3), (6, 2)])
def test_unscale_check_matches_torch(n, offset):
    from spr_pick_amd import graph_step
    g = torch.Generator(device=DEV).manual_seed(n + offset)
    base = torch.randn(n + offset + 1, device=DEV, generator=g) * 3e4
    sc = graph_step.LossScaler(DEV, init_scale=2.0 ** 16)
    rng = np.random.default_rng(n)
    cases = [None] + [(v, where) for v in (float("inf"), float("-inf"), float("nan")) for where in ("first", "last", "random")]
    for inv in (2.0 ** -16, 1.0 / 3.0):
        sc.inv_scale.fill_(inv)
        for case in cases:
            buf = base.clone()
            x = buf[offset:offset + n]
            if case is not None:
                v, where = case
                x[{"first": 0, "last": n - 1, "random": int(rng.integers(0, n))}[where]] = v
            want = x * sc.inv_scale          # torch's fp32 multiply by the same device scalar
            sc._found.zero_()
            sc.unscale_(x)
            assert torch.equal(_bits(x), _bits(want)), (n, offset, inv, case)
            assert int(sc.found_nonfinite) == int((~torch.isfinite(want)).any()), (n, offset, inv, case)
            assert int(sc._found[1 - sc._cur]) == 0
            assert torch.equal(_bits(buf[:offset]), _bits(base[:offset])) and torch.equal(_bits(buf[offset + n:]),
                                                                                           _bits(base[offset + n:]))


def _adam_pair():
    from spr_pick_amd import graph_step
    g = torch.Generator(device=DEV).manual_seed(3)
    shapes = [(96, 96, 3, 3), (7,), (1, 1), (1025,), (48, 1, 3, 3)]
    out = []
    for _ in range(2):
        ps = [torch.nn.Parameter(torch.randn(s, device=DEV, generator=torch.Generator(device=DEV).manual_seed(k)))
              for k, s in enumerate(shapes)]
        out.append((ps, graph_step.make_adam(ps, lr=1e-3)))
    return out, g


def test_skip_aware_adam():
    from spr_pick_amd import graph_step
    (pa, oa), (pb, ob) = _adam_pair()[0]
    sc = graph_step.LossScaler(DEV)
    for step in range(3):
        grads = [torch.randn(p.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(100 * step + k))
                 for k, p in enumerate(pa)]
        for p, q, gr in zip(pa, pb, grads):
            p.grad, q.grad = gr.clone(), gr.clone()
        # flag clear: exactly sprk_adam_multi
        oa.step()
        ob.step(scaler=sc)
        for p, q in zip(pa, pb):
            assert torch.equal(_bits(p.data), _bits(q.data))
        assert torch.equal(oa.exp_avg, ob.exp_avg) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq)
        assert float(oa._steps[oa._cur]) == float(ob._steps[ob._cur]) == step + 1
        sc.update()
        # flag set: nothing moves, the step count is carried into the other buffer
        before = ([p.data.clone() for p in pb], ob.exp_avg.clone(), ob.exp_avg_sq.clone())
        sc.found_nonfinite.fill_(1)
        ob.step(scaler=sc)
        assert all(torch.equal(_bits(p.data), _bits(b)) for p, b in zip(pb, before[0]))
        assert torch.equal(_bits(ob.exp_avg), _bits(before[1])) and torch.equal(_bits(ob.exp_avg_sq), _bits(before[2]))
        assert float(ob._steps[ob._cur]) == step + 1
        sc.update()
    assert sc.skipped_steps() == 3


def test_schedule_matches_gradscaler_rule():
    from spr_pick_amd import graph_step
    seq = [False, False, False, True, False, False, True, True, False, False, False, False, False, False, True, False]
    sc = graph_step.LossScaler(DEV, init_scale=2.0 ** 10, growth_interval=3)
    clean, bad = torch.ones(5, device=DEV), torch.tensor([1.0, float("nan"), 2.0, 3.0, 4.0], device=DEV)
    want = gradscaler_model(seq, 2.0 ** 10, interval=3)
    for k, overflow in enumerate(seq):
        sc.unscale_((bad if overflow else clean).clone())
        assert int(sc.found_nonfinite) == int(overflow)
        sc.update()
        got = (float(sc.scale), int(sc.growth_tracker), sc.skipped_steps())
        assert got == want[k], (k, got, want[k])
        assert float(sc.inv_scale) == 1.0 / want[k][0]
        assert int(sc.found_nonfinite) == 0        # the next step starts with a clear flag
    sd = sc.state_dict()
    assert sd["scale"] == want[-1][0] and sd["_growth_tracker"] == want[-1][1] and sd["growth_interval"] == 3
    fresh = graph_step.LossScaler(DEV)
    fresh.load_state_dict(sd)
    assert fresh.state_dict() == sd
    static = graph_step.LossScaler(DEV, init_scale=2.0 ** 8, dynamic=False, growth_interval=1)
    for overflow in (False, True, False):
        static.unscale_((bad if overflow else clean).clone())
        static.update()
        assert float(static.scale) == 2.0 ** 8
    assert static.skipped_steps() == 1


# ---- one training step ---------------------------------------------------------------------------------------------
def _batch(B=32):
    from spr_pick_amd import synthetic
    mics = [synthetic.micrograph(k, size=384, blobs=30, seed=11) for k in range(2)]
    inp, tgt = synthetic.patch_batches(1, B, mics, seed=5, device=DEV)[0]
    g = torch.Generator(device=DEV).manual_seed(17)
    eps = torch.randn(B, 1, 64, 64, device=DEV, generator=g)
    return inp, tgt, eps, torch.randn(B, 1, 64, 64, device=DEV, generator=g)


def _grads(oracle_state, dtype, scale=None, graph=False, batch=None, adam=False):
    """One step of a fresh model (identical parameters and BatchNorm state) on a fixed batch and noise:
    -> ({parameter name: unscaled gradient}, flag, {parameter name: value after Adam} or None)."""
    from spr_pick_amd import graph_step
    den = _denoiser(oracle_state, dtype)
    sc = None if scale is None else graph_step.LossScaler(DEV, init_scale=scale, dynamic=False)
    inp, tgt, eps, epf = batch or _batch()
    st = graph_step.GraphedTrainStep(den, inp.shape[0], 64, 0.75, 0.01, draw_eps=False, eager_warmup=1 if graph else 0,
                                     graph=graph, scaler=sc)
    if graph:
        st.prepare(inp, tgt, eps, epf)
    st(inp, tgt, flip_p=0.25, eps=eps, eps_flip=epf)
    if graph:
        assert st._graphs, "the step was not replayed from a graph"
    st.grads.all_reduce(1)
    flag = 0
    if sc is not None:
        sc.unscale_(st.grads)
        flag = int(sc.found_nonfinite)
    grads = {n: p.grad.detach().clone() for n, p in den.named_parameters() if p.grad is not None}
    after = None
    if adam:
        opt = graph_step.make_adam(den.parameters(), lr=1e-4)
        opt.step(scaler=sc)
        after = {n: p.detach().clone() for n, p in den.named_parameters()}
    torch.cuda.synchronize()
    return grads, flag, after


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_power_of_two_scale_is_exact(oracle_state, dtype):
    batch = _batch(16)
    g0, f0, p0 = _grads(oracle_state, dtype, None, graph=True, batch=batch, adam=True)
    g1, f1, p1 = _grads(oracle_state, dtype, 2.0 ** 16, graph=True, batch=batch, adam=True)
    assert f1 == 0 and sorted(g0) == sorted(g1)
    bad = ["%s: %d of %d elements differ" % (n, int((_bits(g0[n]) != _bits(g1[n])).sum()), g0[n].numel())
           for n in g0 if not torch.equal(_bits(g0[n]), _bits(g1[n]))]
    assert not bad, bad
    assert all(torch.equal(_bits(p0[n]), _bits(p1[n])) for n in p0)


def _scaled_f16(state, batch, start=2.0 ** 16):
    """f16 gradients at the largest power of two <= start whose step does not overflow (what the dynamic scaler
    settles on) -> (gradients, scale)."""
    s = start
    while True:
        g, flag, _ = _grads(state, "f16", s, batch=batch)
        if not flag:
            return g, s
        s /= 2
        assert s >= 1.0, "f16 gradients overflow even unscaled"


def gradient_table(state, batch=None):
    """Per parameter tensor: the relative L2 error of the bf16, f16 and loss-scaled f16 gradients against fp32 and
    the fraction of exact zeros, from one eager step at batch 32 (same parameters, BatchNorm state, batch and noise
    for every format).  DESIGN.md 4.10 holds the table."""
    batch = batch or _batch(32)
    runs = {k: _grads(state, k, batch=batch)[0] for k in ("f32", "bf16", "f16")}
    runs["f16s"], scale = _scaled_f16(state, batch)
    ref = runs["f32"]
    table = {}
    for n in ref:
        row = {"numel": ref[n].numel(), "f32_norm": float(ref[n].double().norm()),
               "zero_f32": float((ref[n] == 0).double().mean())}
        for k in ("bf16", "f16", "f16s"):
            row["err_" + k] = float((runs[k][n].double() - ref[n].double()).norm() / max(row["f32_norm"], 1e-300))
            row["zero_" + k] = float((runs[k][n] == 0).double().mean())
        table[n] = row
    return table, scale


def _trained_state(oracle_state, steps):
    """The fixture's model trained in fp32 for `steps` graph-replayed steps (batch 32, lr 1e-4) -> its state."""
    from spr_pick_amd import graph_step, synthetic
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    np.random.seed(0)
    den = _denoiser(oracle_state, "f32")
    mics = [synthetic.micrograph(k, size=512, blobs=40, seed=3) for k in range(8)]
    batches = synthetic.patch_batches(64, 32, mics, seed=9, device=DEV)
    st = graph_step.GraphedTrainStep(den, 32, 64, 0.75, 0.01, eager_warmup=1)
    st.prepare(*batches[0])
    opt = graph_step.make_adam(den.parameters(), lr=1e-4)
    for k in range(steps):
        st(*batches[k % len(batches)])
        st.grads.all_reduce(1)
        opt.step()
    torch.cuda.synchronize()
    return {k[len("models."):]: v.detach().clone() for k, v in den.state_dict().items() if k.startswith("models.")}


UNET, SIGMA = "models.denoiser_model.denoise_branch.", "models.sigma_estimation_model."


def test_f16_with_loss_scale_is_as_accurate_as_bf16(oracle_state):
    """The premise of loss scaling, measured where it holds.  At the initial weights no f16 gradient underflows (unscaled
    f16 is 2-5x more accurate than bf16 there).  After 1000 fp32 training steps the sigma-net's
    gradients have shrunk: unscaled f16 is WORSE than bf16 on 24 of its 28 tensors (up to 6 % extra exact zeros),
    while f16 at the scale the dynamic scaler settles on (2^15) is 12x better than bf16 on every one of them.

    Bound: scaled f16 <= bf16 on every sigma-net and U-Net tensor (measured scaled / bf16: sigma-net <= 0.082,
    U-Net <= 0.72, i.e. margins 12x and 1.4x); the U-Net's output_conv, an fp32 layer in every mode, is left out
    (its 2-element bias measured 1.08).  Contrast: unscaled f16 worse than bf16 on at least half the sigma-net's
    tensors (measured 24 of 28).  Every tensor counts (all have fp32 norms >= 1e-3 of their network's largest)."""
    table, scale = gradient_table(_trained_state(oracle_state, 1000))
    assert 1.0 <= scale <= 2.0 ** 16
    sigma = {n: r for n, r in table.items() if n.startswith(SIGMA)}
    unet = {n: r for n, r in table.items() if n.startswith(UNET) and ".output_conv." not in n}
    assert len(sigma) >= 20 and len(unet) >= 30
    for n, r in list(sigma.items()) + list(unet.items()):
        assert np.isfinite(r["err_f16s"]) and r["err_f16s"] <= r["err_bf16"], (n, scale, r)
    worse = [n for n, r in sigma.items() if r["err_f16"] > r["err_bf16"]]
    assert len(worse) >= len(sigma) // 2, (len(worse), len(sigma))


def test_overflow_skips_the_step_and_backs_off(oracle_state):
    from spr_pick_amd import graph_step
    batch = _batch(16)
    den = _denoiser(oracle_state, "f16")
    sc = graph_step.LossScaler(DEV, init_scale=2.0 ** 40, dynamic=False)
    inp, tgt, eps, epf = batch
    st = graph_step.GraphedTrainStep(den, 16, 64, 0.75, 0.01, draw_eps=False, eager_warmup=1, scaler=sc)
    st.prepare(inp, tgt, eps, epf)
    opt = graph_step.make_adam(den.parameters(), lr=1e-4)
    p0 = {n: p.detach().clone() for n, p in den.named_parameters()}
    st(inp, tgt, flip_p=0.25, eps=eps, eps_flip=epf)
    sc.unscale_(st.grads)
    opt.step(scaler=sc)
    assert int(sc.found_nonfinite) == 1
    assert all(torch.equal(_bits(p.detach()), _bits(p0[n])) for n, p in den.named_parameters())
    assert float(opt._steps[opt._cur]) == 0.0
    sc.update()
    assert float(sc.scale) == 2.0 ** 40 and sc.skipped_steps() == 1

    # dynamic, started at 2^40: halves on every skipped step until one is taken
    sc.dynamic = True
    sc.load_state_dict({"scale": 2.0 ** 40, "_growth_tracker": 0})
    scale, taken = 2.0 ** 40, False
    for k in range(40):
        st(inp, tgt, flip_p=0.25, eps=eps, eps_flip=epf)
        sc.unscale_(st.grads)
        opt.step(scaler=sc)
        skipped = int(sc.found_nonfinite)
        sc.update()
        if skipped:
            scale *= 0.5
            assert float(sc.scale) == scale and sc.skipped_steps() == k + 1
            assert float(opt._steps[opt._cur]) == 0.0
        else:
            taken = True
            assert float(sc.scale) == scale and float(opt._steps[opt._cur]) == 1.0
            assert any(not torch.equal(p.detach(), p0[n]) for n, p in den.named_parameters())
            break
    assert taken and 2.0 ** 8 <= scale < 2.0 ** 40 and sc.skipped_steps() >= 1


# ---- the trainer --------------------------------------------------------------------------------------------------
def test_cli_f16_dynamic_train_resume(tmp_path, monkeypatch):
    from spr_pick_amd import checkpoint, cli, train
    from test_gpu_trainer import _write_set
    imgs, lab = _write_set(str(tmp_path))

    def run(runs, iters):
        argv = ("train start -a ssdn -n gaussian --noise_value var -t %s -l %s -ap 0.75 -tau 0.01 -iter %d "
                "--train_batch_size 16 --eval_interval 1000000 --print_interval 16 --checkpoint_interval 16 --nms 18 "
                "--bb 24 --runs_dir %s" % (imgs, lab, iters, runs)).split()
        t = cli.start(argv)
        return t, t.run_dir_path

    monkeypatch.setenv("SPRK_CONV_DTYPE", "f16")
    monkeypatch.setenv("SPRK_LOSS_SCALE", "dynamic")
    t, rd = run(str(tmp_path / "runs16"), 48)
    assert t.scaler is not None and t.scaler.dynamic
    ck = checkpoint.load(os.path.join(rd, "training_jt", "model_00000048.training"))
    assert sorted(ck) == ["denoiser", "optimizer", "rng", "scaler", "state"]
    assert ck["scaler"]["scale"] == t.scaler.get_scale() and ck["scaler"]["_growth_tracker"] == int(t.scaler.growth_tracker)
    assert ck["scaler"]["growth_interval"] == 2000 and ck["scaler"]["growth_factor"] == 2.0
    metrics = open(os.path.join(rd, "metrics.tsv")).read()
    assert "train/loss_scale\t16\t" in metrics and "train/skipped_steps\t48\t" in metrics
    log = open(os.path.join(rd, "log.txt")).read()
    assert "loss_scale=" in log and "skipped_steps=" in log and "without loss scaling" not in log

    monkeypatch.delenv("SPRK_LOSS_SCALE")
    r = train.resume_run(rd)                      # the checkpoint turns scaling on, with the scale it had reached
    assert r.scaler is not None and r.scaler.get_scale() == ck["scaler"]["scale"]
    assert int(r.scaler.growth_tracker) == ck["scaler"]["_growth_tracker"]
    assert r.scaler.skipped_steps() == ck["scaler"]["skipped_steps"]
    del r
    resumed = cli.start(["train", "resume", rd, "--iterations", "64"])
    assert resumed.scaler is not None and resumed.state[train.StateValue.ITERATION] == 64
    ck2 = checkpoint.load(os.path.join(rd, "training_jt", "model_00000064.training"))
    s0, s1 = ck["scaler"], ck2["scaler"]                  # one more step: counted as clean or as skipped
    assert (s1["_growth_tracker"], s1["skipped_steps"]) in ((s0["_growth_tracker"] + 1, s0["skipped_steps"]),
                                                            (0, s0["skipped_steps"] + 1))

    monkeypatch.setenv("SPRK_CONV_DTYPE", "f32")
    t32, rd32 = run(str(tmp_path / "runs32"), 16)
    assert t32.scaler is None
    ck32 = checkpoint.load(os.path.join(rd32, "training_jt", "model_00000016.training"))
    assert "scaler" not in ck32
    metrics32 = open(os.path.join(rd32, "metrics.tsv")).read()
    assert "loss_scale" not in metrics32 and "skipped_steps" not in metrics32
    assert "loss_scale" not in open(os.path.join(rd32, "log.txt")).read()
