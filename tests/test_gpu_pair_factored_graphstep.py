"""The captured training step of the pair models on FACTORED batches (graphstep.FactoredPairGraphedTrainStep) against the
launch-by-launch factored step: the small CDRP and DTA models of tests/pair_step_helpers.py, four factored batches whose pair, drug and
second-input counts all differ -- one with a single distinct drug, one with all pairs distinct -- and one beyond the pair capacity
(tests/pair_factored_step_helpers.py), capacities from ``FactoredPairShapes.from_batches(batches, margin=0.05)``.

Tolerances are tests/test_gpu_pair_graphstep.py's, for the same comparison: loss atol 1e-5 / rtol 1e-4 per step, ``opt.flat`` atol
2e-5 / rtol 1e-3 after the steps, Adam's eps = 1e-4 in the multi-step weight comparisons (why: the comment above ADAM_EPS in
tests/test_graphstep.py)."""
import copy

import pytest
import torch

from tests import pair_factored_step_helpers as F
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
    """(the four small factored batches, the one beyond the pair capacity, the shapes): built once per kind, never written to"""
    if kind not in _BATCHES:
        from fragnet_amd import graphstep
        small, big, shapes = F.batches(kind, DEV)
        fits = lambda b: shapes.fits(graphstep.factored_batch_counts(b), b.max_per_mol)
        assert all(fits(b) for b in small) and not fits(big)
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


def _step(model, opt, kind, **kw):
    from fragnet_amd import graphstep
    small, _, shapes = _batches(kind)
    return graphstep.FactoredPairGraphedTrainStep(model, opt, shapes, _fresh(small[0]), **kw)


@pytest.mark.parametrize("kind", H.KINDS)
def test_captured_factored_step_matches_the_eager_factored_step(kind):
    from fragnet_amd import _lib, data, graphstep, plan
    small, big, shapes = _batches(kind)
    model_a, opt_a, model_b, opt_b = _pair(kind)
    step = _step(model_b, opt_b, kind)
    torch.testing.assert_close(opt_b.flat, opt_a.flat, atol=0, rtol=0)                # capture does not move the weights
    assert step.adam_in_graph and step.rng is model_b.drug_model.pretrain.rng
    assert step.static.n_fields <= _lib.FN_MAX_STAGE_FIELDS                           # one staging launch holds everything
    t = step.static.t
    assert t[H.SECOND[kind]].shape[0] == shapes.second_cap and t["y"].shape == (shapes.pair_cap,)
    assert t[plan.N_MOLS_KEY] == shapes.cap["mol"] and t["x_atoms"].shape[0] == shapes.cap["atom"]
    for i in range(6):
        b = small[i % 4]
        loss_a = _eager_step(model_a, opt_a, b)
        loss_b = step(_fresh(b)).clone()
        torch.testing.assert_close(loss_b, loss_a, atol=1e-5, rtol=1e-4)
        # what the step staged is what the torch counterpart pads, bit for bit; the counts are the batch's
        want = graphstep.pad_factored_pair_batch(b, shapes)
        for k, v in want.items():
            if torch.is_tensor(v):
                assert torch.equal(t[k], v), k
        assert torch.equal(t.offsets, want.offsets)
        c = graphstep.factored_batch_counts(b)
        assert int(t[graphstep.REAL_PAIRS_KEY]) == c["pair"] and int(t[plan.REAL_MOLS_KEY]) == c["mol"]
        # and the orderings the captured launch built are the collate's
        for k in data.PAIR_ORDER_KEYS:
            n = c["pair"] if k.endswith("perm") else b[k].numel()
            assert torch.equal(t[k][:n], b[k][:n]), k
            assert bool((t[k][n:] == (-1 if k.endswith("perm") else c["pair"])).all()), k
    assert step.replays == 6 and step.fallbacks == 0
    torch.testing.assert_close(opt_b.flat, opt_a.flat, atol=2e-5, rtol=1e-3)
    # beyond a capacity: exactly one fallback, on the same optimiser state; the next fitting batch replays
    before = opt_b.flat.detach().clone()
    loss_a, loss_b = _eager_step(model_a, opt_a, big), step(_fresh(big)).clone()
    torch.testing.assert_close(loss_b, loss_a, atol=1e-5, rtol=1e-4)
    assert step.fallbacks == 1 and step.replays == 6 and not torch.equal(before, opt_b.flat)
    step(_fresh(small[1]))
    assert step.replays == 7 and step.fallbacks == 1 and opt_b.steps == 8


@pytest.mark.parametrize("kind", H.KINDS)
def test_one_record_per_pair_batch_is_staged_through_as_factored(kind):
    from fragnet_amd import data
    small, _, shapes = _batches(kind)
    model_a, opt_a, model_b, opt_b = _pair(kind)
    step = _step(model_b, opt_b, kind)
    plain = H.batch(kind, 5, 805, DEV)                                                 # 5 pairs = 5 molecules = 5 second rows: it fits
    loss_a = _eager_step(model_a, opt_a, data.as_factored(_fresh(plain)))
    loss_b = step(_fresh(plain)).clone()
    assert step.replays == 1 and step.fallbacks == 0
    torch.testing.assert_close(loss_b, loss_a, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(opt_b.flat, opt_a.flat, atol=2e-5, rtol=1e-3)


@pytest.mark.parametrize("kind", H.KINDS)
def test_captured_factored_step_with_dropout_is_reproducible_across_a_fallback(kind):
    small, big, _ = _batches(kind)
    runs = []
    for _ in range(2):
        _, _, model, opt = _pair(kind, drop=0.15, seed=1234)
        step = _step(model, opt, kind)
        losses = [step(_fresh(b)).clone() for b in (small[0], small[1], big, small[2], small[3])]      # an eager step between replays
        assert step.replays == 4 and step.fallbacks == 1
        runs.append((torch.stack(losses), opt.flat.detach().clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_replays_of_one_batch_draw_fresh_dropout_masks():
    small, _, _ = _batches("cdrp")
    _, _, model, opt = _pair("cdrp", drop=0.15, lr=0.0)
    step = _step(model, opt, "cdrp")
    losses = [float(step(_fresh(small[0]))) for _ in range(3)]          # lr = 0: only the masks differ between replays
    assert len(set(losses)) == 3, losses
    assert int(model.drug_model.pretrain.rng.dev) > 0


@pytest.mark.parametrize("kind", H.KINDS)
def test_trainers_with_the_captured_factored_step_match_the_eager_trainers(kind):
    from fragnet_amd import train
    small, _, _ = _batches(kind)
    loader = H.Loader(small[:3])
    loader.dataset = list(range(28))
    model_a, opt_a, model_b, opt_b = _pair(kind)
    step = _step(model_b, opt_b, kind)
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


def test_factored_step_refusals(monkeypatch):
    import torch.distributed as dist
    from fragnet_amd import data, graphstep
    from fragnet_amd.model import FragNetFineTune
    small, _, shapes = _batches("cdrp")
    _, _, model, opt = _pair("cdrp")
    cls = graphstep.FactoredPairGraphedTrainStep
    with pytest.raises(ValueError, match="overlap"):
        cls(model, opt, shapes, _fresh(small[0]), overlap=True)
    with pytest.raises(TypeError, match="pair model"):                     # a property model, or a bare encoder
        cls(model.drug_model, opt, shapes, _fresh(small[0]))
    with pytest.raises(TypeError, match="pair model"):
        cls(FragNetFineTune(**H.SMALL).to(DEV).train(), opt, shapes, _fresh(small[0]))
    with pytest.raises(TypeError, match="FactoredPairShapes"):
        cls(model, opt, graphstep.StaticShapes(shapes.cap, shapes.slack), _fresh(small[0]))
    grid = data.batch_to(data.pair_grid_batch(H.records("cdrp", 3, 1), torch.zeros(2, H.GENE_DIM), "cdrp"), DEV)
    with pytest.raises(ValueError, match="grid batch"):
        cls(model, opt, shapes, grid)
    # more than one rank: refused before anything is staged (the process group is only ASKED for its size)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(ValueError, match="single-GPU"):
        cls(model, opt, shapes, _fresh(small[0]))
    monkeypatch.undo()
    model.eval()
    with pytest.raises(RuntimeError, match="TRAINING step"):
        cls(model, opt, shapes, _fresh(small[0]))
    model.train()
    # a grid batch handed to a built step: no target, no training step
    step = cls(model, opt, shapes, _fresh(small[0]))
    with pytest.raises(ValueError, match="grid batch"):
        step(grid)
    assert step.fallbacks == 1 and step.replays == 0
