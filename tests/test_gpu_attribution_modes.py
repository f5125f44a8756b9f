"""The attribution drivers run their model in evaluation mode and hand it back in the mode it came in (``attribution.evaluation``):
``leave_one_out``, ``input_gradients``, ``integrated_gradients`` and ``attention_weights`` on a model left in ``train()`` with
``drop_ratio=0.2`` -- a pass that stayed in training mode would draw dropout masks and change every number.  The other two drivers,
``fragment_contributions`` and ``fragment_shapley``, have the restored flag pinned in their own files (the tests that count one encoder
pass and one read-out per chunk).

Expected values: the same call on the same model in ``eval()`` mode, bit for bit -- the mode is the only difference."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTOR = dict(n_classes=2, num_layer=2, num_heads=4, drop_ratio=0.2, h1=16, h2=16, h3=16, h4=16, act="relu", fthead="FTHead3")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


@pytest.fixture(scope="module")
def store():
    from fragnet_amd import synth
    from fragnet_amd.dataset import FlatMolStore
    return FlatMolStore.from_records(synth.synth_molecules(4, seed=29, profile="esol")).to(DEV)


def _model(viz):
    from fragnet_amd import model as M
    from fragnet_amd import viz_model as V
    torch.manual_seed(3)
    return (V.FragNetFineTuneViz(**CTOR, edge_features=17) if viz else M.FragNetFineTune(**CTOR)).to(DEV)


def _drivers():
    from fragnet_amd import attention, attribution
    from fragnet_amd import gradient_attribution as ga
    return {"leave_one_out": (False, lambda m, s: attribution.leave_one_out(m, s)),
            "input_gradients": (False, lambda m, s: ga.input_gradients(m, s, target=1, return_gradients=True)),
            "integrated_gradients": (False, lambda m, s: ga.integrated_gradients(m, s, steps=2, target=1)),
            "attention_weights": (True, lambda m, s: attention.attention_weights(m, s, batch_size=3))}


@pytest.mark.parametrize("driver", ["leave_one_out", "input_gradients", "integrated_gradients", "attention_weights"])
def test_a_driver_evaluates_a_training_model_and_hands_it_back_training(driver, store):
    viz, run = _drivers()[driver]
    model = _model(viz)
    want = run(model.eval(), store).arrays()
    assert not model.training
    got = run(model.train(), store).arrays()
    assert model.training, f"{driver} left the model in evaluation mode"
    assert list(got) == list(want)
    for key in want:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), f"{driver}: {key} differs between a training and an evaluation model"
    assert any(np.abs(v).max() > 0 for k, v in want.items() if v.dtype == np.float32 and v.size), "every number is zero: nothing was compared"


def test_a_refusal_in_mid_pass_hands_the_model_back_training(store):
    from fragnet_amd import gradient_attribution as ga
    model = _model(False).train()
    with pytest.raises(IndexError, match="target 2"):
        ga.integrated_gradients(model, store, steps=2, target=CTOR["n_classes"])
    assert model.training
