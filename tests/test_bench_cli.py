"""bench.py's command line and its --dump-outputs writer (no GPU): a plain run is the headline only, --full adds the rest,
the dump is float32 .npy files within the size bound, each parameter's slice of the optimiser's flat buffers without padding."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

from tests.conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_cli_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_is_the_default_and_full_and_dump_are_options():
    b = _bench()
    a = b.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    a = b.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"
    with pytest.raises(SystemExit):
        b.parse_args(["--steps", "0"])


def test_dump_writes_float32_npy_and_keeps_float64(tmp_path):
    b = _bench()
    d = tmp_path / "dump"
    n = b.dump_outputs(str(d), {"loss": torch.tensor([0.5], dtype=torch.float16), "ids": np.arange(4),
                                "wide": np.ones(3, dtype=np.float64)})
    assert sorted(os.listdir(d)) == ["ids.npy", "loss.npy", "wide.npy"]
    assert np.load(d / "loss.npy").dtype == np.float32 and np.load(d / "loss.npy")[0] == 0.5
    assert np.load(d / "ids.npy").dtype == np.float32 and np.load(d / "ids.npy").tolist() == [0, 1, 2, 3]
    assert np.load(d / "wide.npy").dtype == np.float64
    assert n == 4 + 16 + 24


def test_dump_over_the_bound_writes_nothing(tmp_path):
    b = _bench()
    d = tmp_path / "dump"
    with pytest.raises(ValueError):
        b.dump_outputs(str(d), {"a": np.zeros(300, np.float32), "b": np.zeros(300, np.float32)}, limit_bytes=2000)
    assert not d.exists()


def test_step_outputs_drop_the_flat_buffers_padding():
    from fragnet_amd import parallel
    b = _bench()
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(3, 1), torch.nn.Linear(1, 5))      # 3 + 1 | 1 + 5 elements: padding after the biases
    opt = parallel.FlatAdam(list(m.parameters()), lr=1e-3)
    opt.grad.copy_(torch.arange(opt.grad.numel(), dtype=torch.float32))
    run = types.SimpleNamespace(opt=opt, last_loss=torch.tensor(0.25))
    out = b.step_outputs(run)
    want_p = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    want_g = torch.cat([torch.arange(off, off + p.numel(), dtype=torch.float32) for p, off in zip(opt.params, opt.offsets)])
    assert torch.equal(out["parameters"], want_p) and torch.equal(out["gradients"], want_g)
    assert out["loss"].shape == (1,) and float(out["loss"][0]) == 0.25
