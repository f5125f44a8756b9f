"""The captured training step of the pair models (graphstep.PairGraphedTrainStep) against the launch-by-launch step: small CDRP and
DTA models (2 layers, 4 heads; 903 gene values, 1000 protein tokens), batches of 6, 5 and 4 synthetic pairs, capacities from
``StaticShapes.from_batches(batches, margin=0.05)``.

Tolerances are tests/test_graphstep.py's for the same comparison -- loss atol 1e-5 / rtol 1e-4 per step, ``opt.flat`` atol 2e-5 /
rtol 1e-3 after the steps -- and so is Adam's eps = 1e-4 in the multi-step weight comparisons (why: the comment above ADAM_EPS
there; the default eps turns rounding-level gradient differences into lr-sized steps)."""
import copy

import pytest
import torch

from tests import pair_step_helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ADAM_EPS = 1e-4
LR = 1e-3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


_BATCHES = {}


def _batches(kind):
    """(the three batches of 6, 5 and 4 pairs, one of 12 beyond the capacities, the shapes): built once per kind, never written to"""
    if kind not in _BATCHES:
        from fragnet_amd import graphstep
        small = [H.batch(kind, n, 800 + n, DEV) for n in (6, 5, 4)]
        shapes = graphstep.StaticShapes.from_batches(small, margin=0.05)
        big = H.batch(kind, 12, 900, DEV)
        assert all(shapes.fits(graphstep.batch_counts(b), b.max_per_mol) for b in small) and not shapes.fits(graphstep.batch_counts(big), big.max_per_mol)
        _BATCHES[kind] = (small, big, shapes)
    return _BATCHES[kind]


def _fresh(b):
    """the same tensors in a dict of its own: a plan cached on it stays with this use"""
    return b.like(dict(b))


def _spec(b, y=None):
    from fragnet_amd import _lib
    return (_lib.LOSS_MSE, b["y"] if y is None else y, None)


def _opt(model, probe_batch, lr=LR):
    from fragnet_amd import parallel

    def probe():
        model(_fresh(probe_batch), loss=_spec(probe_batch))[1].backward()
    return parallel.FlatAdam.for_live_parameters(model, probe, lr=lr, eps=ADAM_EPS)


def _eager_step(model, opt, b, y=None):
    opt.zero_grad()
    _, loss = model(_fresh(b), loss=_spec(b, y))
    loss.backward()
    opt.step()
    return loss.detach()


def _pair(kind, drop=0.0, lr=LR, seed=99):
    """(model_a, opt_a) eager and (model_b, opt_b) for the captured step: equal weights, equal dropout seeds"""
    small, _, _ = _batches(kind)
    model_a = H.model(kind, DEV, seed=3, drop=drop)
    model_b = copy.deepcopy(model_a)
    model_a.drug_model.pretrain.rng.seed = model_b.drug_model.pretrain.rng.seed = seed
    return model_a, _opt(model_a, small[0], lr), model_b, _opt(model_b, small[0], lr)


@pytest.mark.parametrize("kind", H.KINDS)
def test_captured_pair_step_matches_the_eager_step(kind):
    from fragnet_amd import data, graphstep
    small, big, shapes = _batches(kind)
    model_a, opt_a, model_b, opt_b = _pair(kind)
    step = graphstep.PairGraphedTrainStep(model_b, opt_b, shapes, _fresh(small[0]))
    torch.testing.assert_close(opt_b.flat, opt_a.flat, atol=0, rtol=0)                # capture does not move the weights
    assert step.adam_in_graph and step.rng is model_b.drug_model.pretrain.rng
    assert H.SECOND[kind] in step.static.t and step.static.t[H.SECOND[kind]].shape[0] == shapes.cap["mol"]
    for i in range(6):
        b = small[i % 3]
        loss_a = _eager_step(model_a, opt_a, b)
        loss_b = step(_fresh(b)).clone()
        torch.testing.assert_close(loss_b, loss_a, atol=1e-5, rtol=1e-4)
    assert step.replays == 6 and step.fallbacks == 0
    torch.testing.assert_close(opt_b.flat, opt_a.flat, atol=2e-5, rtol=1e-3)
    # beyond the capacities: the eager step, on the same optimiser state; the next fitting batch replays
    before = opt_b.flat.detach().clone()
    step(_fresh(big))
    assert step.fallbacks == 1 and step.replays == 6 and not torch.equal(before, opt_b.flat)
    step(_fresh(small[1]))
    assert step.replays == 7 and step.fallbacks == 1
    # a factored batch falls back too, however small
    before = opt_b.flat.detach().clone()
    step(data.as_factored(_fresh(small[2])))
    assert step.fallbacks == 2 and step.replays == 7 and not torch.equal(before, opt_b.flat)
    assert opt_b.steps == 9


@pytest.mark.parametrize("kind", H.KINDS)
def test_captured_pair_step_with_dropout_is_reproducible_across_a_fallback(kind):
    from fragnet_amd import graphstep
    small, big, shapes = _batches(kind)
    runs = []
    for _ in range(2):
        _, _, model, opt = _pair(kind, drop=0.15, seed=1234)
        step = graphstep.PairGraphedTrainStep(model, opt, shapes, _fresh(small[0]))
        losses = [step(_fresh(b)).clone() for b in (small[0], small[1], big, small[2], small[0])]      # an eager step between replays
        assert step.replays == 4 and step.fallbacks == 1
        runs.append((torch.stack(losses), opt.flat.detach().clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_replays_of_one_batch_draw_fresh_dropout_masks():
    from fragnet_amd import graphstep
    small, _, shapes = _batches("cdrp")
    _, _, model, opt = _pair("cdrp", drop=0.15, lr=0.0)
    step = graphstep.PairGraphedTrainStep(model, opt, shapes, _fresh(small[0]))
    losses = [float(step(_fresh(small[0]))) for _ in range(3)]          # lr = 0: only the masks differ between replays
    assert len(set(losses)) == 3, losses
    assert int(model.drug_model.pretrain.rng.dev) > 0


@pytest.mark.parametrize("kind", H.KINDS)
def test_trainers_with_a_captured_step_match_the_eager_trainers(kind):
    from fragnet_amd import graphstep, train
    small, _, shapes = _batches(kind)
    loader = H.Loader(small)
    loader.dataset = list(range(15))
    model_a, opt_a, model_b, opt_b = _pair(kind)
    step = graphstep.PairGraphedTrainStep(model_b, opt_b, shapes, _fresh(small[0]))
    trainer_a, trainer_b = ((train.TrainerFineTuneCDRP if kind == "cdrp" else train.TrainerFineTuneDTA)(target_type="regr") for _ in range(2))
    stats = dict(label_mean=2.0, label_sdev=3.0) if kind == "dta" else dict(label_mean=None, label_sdev=None)
    for epoch, mean in enumerate((stats["label_mean"], 0.5)):              # the second epoch moves the mean: no re-capture
        kw = dict(stats, label_mean=mean) if kind == "dta" else stats
        loss_a = trainer_a.train(model=model_a, loader=loader, optimizer=opt_a, scheduler=None, device=DEV, val_loader=None, **kw)
        loss_b = trainer_b.train(model=model_b, loader=loader, optimizer=opt_b, scheduler=None, device=DEV, val_loader=None, **kw, graph_step=step)
        assert loss_b == pytest.approx(loss_a, rel=1e-4)
        assert step.replays == 3 * (epoch + 1) and step.fallbacks == 0
        torch.testing.assert_close(opt_b.flat, opt_a.flat, atol=2e-5, rtol=1e-3)
    if kind == "dta":                                                      # the staged target was the normalised one
        want = (small[2]["y"] - 0.5) / (3.0 + 1e-5)
        assert torch.equal(step.static.t["y"][: want.shape[0]], want) and not bool(step.static.t["y"][want.shape[0]:].any())


def test_pair_step_refusals():
    from fragnet_amd import graphstep
    small, _, shapes = _batches("cdrp")
    _, _, model, opt = _pair("cdrp")
    with pytest.raises(ValueError, match="overlap"):
        graphstep.PairGraphedTrainStep(model, opt, shapes, _fresh(small[0]), overlap=True)
    model.eval()
    with pytest.raises(RuntimeError, match="TRAINING step"):
        graphstep.PairGraphedTrainStep(model, opt, shapes, _fresh(small[0]))
    model.train()
    with pytest.raises(TypeError, match="pair model"):
        graphstep.PairGraphedTrainStep(model.drug_model, opt, shapes, _fresh(small[0]))
