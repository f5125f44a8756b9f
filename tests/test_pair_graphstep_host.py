"""CPU-side checks of the captured pair step's surface: the numpy reference of the FN_STAGE_ROWS_I64 staging kind against
``graphstep.pad_pair_batch`` (the torch counterpart of the staging launch for a CDRP / DTA batch), the padding rules of such a batch,
and the trainers' keyword sets."""
import inspect
import os

import numpy as np
import pytest
import torch

from fragnet_amd import graphstep, train
from tests import batch_io_rows_i64_ref as R64
from tests import pair_step_helpers as H


def test_rows_i64_reference_zero_rows_behind_the_real_ones():
    from fragnet_amd import _lib
    assert R64.STAGE_ROWS_I64 == _lib.STAGE_ROWS_I64                 # the reference is of the kind the binding names
    src = np.arange(15, dtype=np.int64).reshape(5, 3) - 7
    out = R64.stage_rows_i64(src, 5, 8, 3)
    assert out.dtype == np.int64 and out.shape == (8, 3)
    assert np.array_equal(out[:5], src) and not out[5:].any()
    assert not R64.stage_rows_i64(None, 0, 4, 2).any()
    assert np.array_equal(R64.stage_rows_i64(src, 5, 5, 3), src)
    assert np.array_equal(R64.stage_rows_i64(src, 2, 4, 3)[:2], src[:2])          # only the first n_real rows are read


def test_new_kind_is_the_next_free_number_and_the_table_size_stays():
    from fragnet_amd import _lib
    older = (_lib.STAGE_ROWS, _lib.STAGE_IDS, _lib.STAGE_COLS, _lib.STAGE_MASK, _lib.STAGE_COUNT, _lib.STAGE_BUMP, _lib.STAGE_ZERO,
             _lib.STAGE_OFFSETS)
    assert sorted(older) == list(range(8)) and _lib.STAGE_ROWS_I64 == R64.STAGE_ROWS_I64 == 8
    assert _lib.FN_MAX_STAGE_FIELDS == 40 and _lib.ABI_VERSION == 12
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "fragnet_hip.h")).read()
    assert "#define FN_STAGE_ROWS_I64 8" in header


@pytest.mark.parametrize("kind", H.KINDS)
def test_pad_pair_batch_pads_the_second_input_with_zero_rows(kind):
    batches = [H.batch(kind, n, 700 + n) for n in (6, 5, 4)]
    shapes = graphstep.StaticShapes.from_batches(batches, margin=0.05)
    key = H.SECOND[kind]
    assert key in graphstep.PAIR_FIELDS and key not in graphstep.FIELDS
    for b in batches:
        n = b["y"].shape[0]
        padded = graphstep.pad_pair_batch(b, shapes)
        second = padded[key]
        assert second.dtype == torch.int64 and second.shape == (shapes.cap["mol"], b[key].shape[1])
        assert second.shape[0] == padded["y"].shape[0]                              # the mol capacity is that of y
        assert torch.equal(second[:n], b[key]) and not bool(second[n:].any())       # real rows untouched, zero rows behind them
        assert np.array_equal(second.numpy(), R64.stage_rows_i64(b[key].numpy(), n, shapes.cap["mol"], b[key].shape[1]))
        base = graphstep.pad_batch(b, shapes)                                       # everything else is pad_batch's
        assert set(padded) == set(base) | {key}
        for k, v in base.items():
            assert torch.equal(padded[k], v), k
        assert torch.equal(padded["y"][:n], b["y"]) and not bool(padded["y"][n:].any())
        assert float(padded[graphstep.MASK_KEY].sum()) == n


def test_pair_trainers_keep_their_keywords_and_take_graph_step_last():
    kws = ("model", "loader", "optimizer", "scheduler", "device", "val_loader", "label_mean", "label_sdev")
    for cls in (train.TrainerFineTuneCDRP, train.TrainerFineTuneDTA):
        trainer = cls(target_pos=None, target_type="regr", n_multi_task_heads=0)
        params = inspect.signature(trainer.train).parameters
        assert all(k in params for k in kws), cls
        assert list(params)[-1] == "graph_step" and params["graph_step"].default is None, cls
        for fn in (trainer.validate, trainer.test):
            assert all(k in inspect.signature(fn).parameters for k in ("model", "loader", "device", "label_mean", "label_sdev"))
            assert "graph_step" not in inspect.signature(fn).parameters          # validation and test passes stay eager


def test_drivers_refuse_graph_step_with_factored_pairs():
    assert train.check_pair_graph_step({}) is False and train.check_pair_graph_step({"graph_step": False, "factored_pairs": True}) is False
    assert train.check_pair_graph_step({"graph_step": True}) is True
    with pytest.raises(SystemExit, match="finetune.graph_step.*finetune.factored_pairs"):
        train.check_pair_graph_step({"graph_step": True, "factored_pairs": True})


def test_pair_step_class_reuses_the_property_step_machinery():
    cls = graphstep.PairGraphedTrainStep
    assert issubclass(cls, graphstep.GraphedTrainStep)
    for name in ("_capture", "replay", "__call__", "_eager", "_fwd_bwd_static", "_sync_adam_state"):       # extended through, not copied
        assert name not in vars(cls), name
