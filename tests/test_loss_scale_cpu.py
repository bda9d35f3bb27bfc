"""CPU: the loss-scaling knob (SPRK_LOSS_SCALE / DenoiserTrainer(loss_scale=)) and a Python model of
torch.amp.GradScaler's schedule, which tests/test_gpu_loss_scale.py holds the device kernels to."""
import pytest


def gradscaler_model(steps, init_scale, growth=2.0, backoff=0.5, interval=2000):
    """GradScaler's rule (torch/_amp_update_scale_) over a sequence of steps (True = the step found inf / NaN):
    -> [(scale, growth_tracker, skipped_steps) after each update]."""
    scale, tracker, skipped, out = float(init_scale), 0, 0, []
    for overflow in steps:
        if overflow:
            scale *= backoff
            tracker = 0
            skipped += 1
        else:
            tracker += 1
            if tracker == interval:
                scale *= growth
                tracker = 0
        out.append((scale, tracker, skipped))
    return out


def test_schedule_model():
    seq = [False, False, False, True, False, False, True, True, False, False, False, False]
    got = gradscaler_model(seq, 1024.0, interval=3)
    assert got == [(1024, 1, 0), (1024, 2, 0), (2048, 0, 0), (1024, 0, 1), (1024, 1, 1), (1024, 2, 1),
                   (512, 0, 2), (256, 0, 3), (256, 1, 3), (256, 2, 3), (512, 0, 3), (512, 1, 3)]


@pytest.mark.parametrize("spec, want", [
    (None, None), ("off", None), ("", None), ("OFF", None), ("dynamic", "dynamic"), (" Dynamic ", "dynamic"),
    ("65536", 65536.0), ("2**16", 65536.0), ("1", 1.0), ("0.5", 0.5), ("1e3", ValueError), ("3", ValueError),
    ("-4", ValueError), ("inf", ValueError), ("nan", ValueError), ("2**2000", ValueError), ("static", ValueError),
    ("1.5", ValueError), (65536.0, 65536.0)])
def test_parse_loss_scale(spec, want):
    from spr_pick_amd import graph_step
    if want is ValueError:
        with pytest.raises(ValueError):
            graph_step.parse_loss_scale(spec)
    else:
        assert graph_step.parse_loss_scale(spec) == want


def test_trainer_reads_the_knob(monkeypatch):
    from spr_pick_amd.train import DenoiserTrainer
    monkeypatch.delenv("SPRK_LOSS_SCALE", raising=False)
    assert DenoiserTrainer(None, "joint", device="cpu").loss_scale is None
    monkeypatch.setenv("SPRK_LOSS_SCALE", "dynamic")
    assert DenoiserTrainer(None, "joint", device="cpu").loss_scale == "dynamic"
    assert DenoiserTrainer(None, "joint", device="cpu", loss_scale="1024").loss_scale == 1024.0   # the argument wins
    monkeypatch.setenv("SPRK_LOSS_SCALE", "1000")
    with pytest.raises(ValueError):
        DenoiserTrainer(None, "joint", device="cpu")


def test_scaler_needs_the_gpu():
    from spr_pick_amd import graph_step
    with pytest.raises(RuntimeError):
        graph_step.LossScaler("cpu")
