"""bench.py without --full: the timed steps and nothing else, and --dump-outputs writes what the last timed step computed.
Two runs with the same arguments see the same seeded inputs, so their outputs agree bit for bit (no kernel of the
training step accumulates with atomics)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
                                                         "SPRK_BENCH_STUB", "SPRK_DIST_FORCE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + extra, env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_dumps_reproducible_outputs(tmp_path):
    runs = []
    for d in ("a", "b"):
        j = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / d)])
        assert j["steps"] == 3 and j["warmup"] == 1 and j["full"] is False and j["graph_fallback"] is None
        assert abs(j["value"] - 32 * 3 / (j["ms_per_step"] * 3e-3)) < 1e-6 * j["value"]
        for key in ("roofline", "sustained", "bit_identical", "train_bf16", "batch16", "inference", "full_pipeline",
                    "cpu_baseline"):
            assert key not in j, key
        runs.append(j)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"out_loss.npy", "out_detect.npy", "out_img_denoised.npy", "grad.npy", "state.npy"} <= set(names), names
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and np.all(np.isfinite(x)), n
        assert x.shape == tuple(runs[0]["dump_outputs"]["arrays"][n[:-4]]["shape"]), n
        np.testing.assert_array_equal(x, y, err_msg=n)
    assert np.load(tmp_path / "a" / "out_loss.npy").size == 32            # one loss per patch of the batch
    assert np.abs(np.load(tmp_path / "a" / "grad.npy")).max() > 0
    assert runs[0]["final_loss"] == runs[1]["final_loss"]
