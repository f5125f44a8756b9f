"""A plain `bench.py --gpus 1 --steps K --warmup W` run: the headline line with exactly K timed steps and nothing measured besides
it, and --dump-outputs holding what the last timed step computed (its loss is the line's final_loss)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_only_and_dumps_the_last_step(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    out = tmp_path / "outputs"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "molecules/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] / 1e3 - 512) < 512 * 2e-3
    for extra in ("ms_per_step_repeats", "epoch_sample", "same_code_round3_shapes", "roofline", "cpu_baseline"):
        assert extra not in line, extra
    assert sorted(os.listdir(out)) == ["gradients.npy", "loss.npy", "parameters.npy"]
    loss, params, grads = (np.load(out / f"{n}.npy") for n in ("loss", "parameters", "gradients"))
    assert loss.dtype == params.dtype == grads.dtype == np.float32
    assert loss.shape == (1,) and abs(float(loss[0]) - line["final_loss"]) <= 2e-6 * max(1.0, abs(line["final_loss"]))
    assert params.shape == grads.shape and params.ndim == 1 and params.size > 1_000_000
    assert np.isfinite(params).all() and np.isfinite(grads).all() and np.abs(grads).sum() > 0
    assert loss.nbytes + params.nbytes + grads.nbytes <= 64 << 20
