"""``TrainerFineTune.evaluate`` / ``test_on_device`` (fragnet_amd/train.py) against ``test`` on small synthetic stores: a tox21-profile
classification store and an esol-profile regression store of about 100 molecules in batches of 32 (the last batch is short), and DTA
pairs with a non-trivial label mean and deviation.

- ``true`` and ``pred`` equal ``test``'s arrays bit for bit (for DTA: the de-normalised ``pred``).
- The classification score equals ``test``'s sklearn score within 1e-12: both are means of ratios of exact integers in float64.
- The regression MSE equals the float64 MSE of the returned arrays within relative 1e-12 (an fp64 sum of ~100 terms carries at most
  100 x 2^-53).  It is NOT compared with ``test``'s own score, an fp32 numpy mean that differs from it at the 1e-7 level.
- ``evaluate`` leaves the model's mode and its dropout stream alone: a training step after it equals one without it."""
import copy

import numpy as np
import pytest
import torch

from fragnet_amd import metrics as M
from tests import pair_step_helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = dict(num_layer=2, num_heads=4, h1=32, h2=64, h3=64, h4=32, act="relu", fthead="FTHead3")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _store_loader(profile, n, seed):
    from fragnet_amd import synth, train
    from fragnet_amd.dataset import FlatMolStore
    store = FlatMolStore.from_records(synth.synth_molecules(n, seed=seed, profile=profile)).to(DEV)
    return train.StoreLoader(store, 32)


def _model(n_classes, drop=0.0, seed=0):
    from fragnet_amd.model import FragNetFineTune
    torch.manual_seed(seed)
    return FragNetFineTune(n_classes=n_classes, drop_ratio=drop, **SMALL).to(DEV)


def test_classification_matches_test():
    from fragnet_amd import train
    loader, model, trainer = _store_loader("tox21", 101, 70), _model(12), train.TrainerFineTune(target_type="clsf")
    score, true, pred = trainer.test(model, loader)
    model.train()
    res = trainer.evaluate(model, loader)
    assert model.training                                                   # put back as it came
    score_d, true_d, pred_d = trainer.test_on_device(model, loader)
    assert true_d.shape == (101, 12) and true_d.dtype == np.float32
    assert true_d.tobytes() == true.tobytes() and pred_d.tobytes() == pred.tobytes()
    print(f"clsf: test {score!r} evaluate {res['neg_auc']!r}")
    assert abs(res["neg_auc"] - score) <= 1e-12 and score_d == res["neg_auc"] == res["score"]
    assert res["auc"].shape == (12,) and abs(-np.nanmean(res["auc"]) - score) <= 1e-12
    assert np.array_equal(M.reference_counts(pred, true, M.CLSF_LABEL_FLOOR)[:, 2] > 0, ~np.isnan(res["auc"]))
    assert trainer.last_metrics["neg_auc"] == score_d


def test_regression_matches_float64_mse_of_the_arrays():
    from fragnet_amd import train
    loader, model, trainer = _store_loader("esol", 100, 71), _model(1), train.TrainerFineTune(target_type="regr")
    _, true, pred = trainer.test(model, loader)
    model.eval()
    res = trainer.evaluate(model, loader)
    assert not model.training
    score_d, true_d, pred_d = trainer.test_on_device(model, loader)
    assert true_d.shape == pred_d.shape == (100,)
    assert true_d.tobytes() == true.tobytes() and pred_d.tobytes() == pred.tobytes()
    t, p = true.astype(np.float64), pred.astype(np.float64)
    want = ((t - p) ** 2).mean()
    print(f"regr: evaluate mse {res['mse']!r} float64 mse of the arrays {want!r}")
    assert abs(res["mse"] - want) <= 1e-12 * want and score_d == res["mse"] == res["score"]
    assert abs(res["rmse"] - np.sqrt(want)) <= 1e-12 * np.sqrt(want)
    assert abs(res["mae"] - np.abs(t - p).mean()) <= 1e-12 * np.abs(t - p).mean()
    assert res["ci"] == M.concordance_index(M.reference_counts(pred, true))
    ref = M.regression_metrics(M.reference_sums(pred, true))
    assert abs(res["pearson"] - ref["pearson"][0]) <= 1e-9 and abs(res["r2"] - ref["r2"][0]) <= 1e-9 * max(1.0, abs(ref["r2"][0]))


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
def test_pair_trainers_match_test(kind):
    from fragnet_amd import data, train
    recs = H.records(kind, 70, 7200)
    collate = data.collate_fn_cdrp if kind == "cdrp" else data.collate_fn_dta
    loader = H.Loader([data.batch_to(collate(recs[lo:lo + 32]), DEV) for lo in range(0, 70, 32)])
    loader.dataset = recs
    model = H.model(kind, DEV, seed=3)
    ys = np.array([float(r.y) for r in recs])
    if kind == "cdrp":
        trainer, kw = train.TrainerFineTuneCDRP(target_type="regr"), dict(label_mean=None, label_sdev=None)
    else:
        trainer, kw = train.TrainerFineTuneDTA(target_type="regr"), dict(label_mean=float(ys.mean()) + 0.37, label_sdev=float(ys.std()) + 1.3)
    _, true, pred = trainer.test(model, loader, device=DEV, **kw)
    model.train()                                                          # (``test`` leaves the model in eval mode)
    score_d, true_d, pred_d = trainer.test_on_device(model, loader, device=DEV, **kw)
    assert model.training
    assert true_d.shape == pred_d.shape == (70,)
    assert true_d.tobytes() == true.tobytes() and pred_d.tobytes() == pred.tobytes()
    t, p = true.astype(np.float64), pred.astype(np.float64)
    want = ((t - p) ** 2).mean()
    print(f"{kind}: test_on_device mse {score_d!r} float64 mse of the arrays {want!r}")
    assert abs(score_d - want) <= 1e-12 * want
    res = trainer.evaluate(model, loader, device=DEV, **kw)
    assert res == trainer.last_metrics
    assert res["ci"] == M.concordance_index(M.reference_counts(pred, true))


def test_evaluate_leaves_the_training_path_alone():
    from fragnet_amd import train
    loader, trainer = _store_loader("tox21", 64, 72), train.TrainerFineTune(target_type="clsf")
    a = _model(12, drop=0.2, seed=5).train()
    b = copy.deepcopy(a)
    batch = next(iter(loader))

    def step(model):
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        opt.zero_grad()
        loss = trainer._loss(model, batch)
        loss.backward()
        opt.step()
        return loss.detach().cpu(), [q.detach().cpu() for q in model.parameters()]

    offset = a.pretrain.rng.offset
    torch.manual_seed(11)
    trainer.evaluate(a, loader)
    assert a.training and a.pretrain.rng.offset == offset
    loss_a, params_a = step(a)
    torch.manual_seed(11)
    loss_b, params_b = step(b)
    assert torch.equal(loss_a, loss_b)
    assert all(torch.equal(x, y) for x, y in zip(params_a, params_b))


def test_an_empty_loader_is_refused():
    from fragnet_amd import train
    empty = H.Loader([])
    with pytest.raises(ValueError, match="empty"):
        train.TrainerFineTune(target_type="regr").evaluate(_model(1), empty)
