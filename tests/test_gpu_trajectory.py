"""Six Adam steps of the HIP training path against an INDEPENDENT trajectory: the CPU oracle (oracle/fragnet_ref.py) after
``.double()``, float64 batches and torch.optim.Adam in float64.  Every other multi-step test compares two HIP paths with each other
(captured vs eager, rider vs single launch); a step counter off by one, a workspace stale on the second step or an update rule wrong
the same way on both sides passes all of those and fails here.

Three models at num_layer = 2, dropout 0, three ESOL/Tox21-profile batches of 8, 10 and 12 molecules cycled over 6 steps, lr = 1e-3,
eps = 1e-4 (test_graphstep.ADAM_EPS says why: at eps = 1e-8 a gradient of rounding size moves its weight by lr, and two correct
float32 paths part by lr per step in those directions; the update at the default eps is pinned one step at a time in
test_gpu_adam.py).  Same initial weights on both sides (state dict of the oracle model).  The HIP side runs twice: eager steps with
FlatAdam, and GraphedTrainStep with Adam and its rider inside the graph.  Compared: the loss of every step, all weights after
steps 1, 3 and 6.

The bound is 8 x SPREAD, the distance between the FLOAT32 oracle and the float64 oracle on the same batches and seeds -- what a
second correct float32 implementation of the same trajectory is off by.  Measured on the CPU by
test_float32_oracle_stays_within_the_recorded_spread_of_the_float64_oracle (max over steps 1, 3, 6 and all weights, absolute; max
over the six losses, relative to max(1, |loss|)):

    regr     (FTHead3, MSE)                 weights 1.10e-7     losses 0.96e-7
    clsf     (FTHead4, 12 classes, BCE)     weights 1.12e-7     losses 1.01e-7
    pretrain (FragNetPreTrain, 3 x MSE)     weights 1.18e-7     losses 1.15e-7

(two float32 ulps of a weight below 1, one ulp of a loss between 1 and 2: the float32 oracle is as close as float32 can hold the
numbers).  SPREAD holds them rounded up: 1.2e-7 for the weights, 1.5e-7 for the losses.  The factor 8 covers the HIP path's
other summation orders (segment sums, split weight-gradient products, tree reductions in the losses); 8 x 1.2e-7 is still about
1000 x below one wrong Adam step (lr = 1e-3 per weight).  The bound does not come from what the HIP path shows; what it shows is
printed by the tests and recorded in DESIGN.md."""
import copy
import functools

import pytest
import torch

from fragnet_amd import data, synth
from tests.test_graphstep import ADAM_EPS, CFG

gpu = pytest.mark.gpu

LR, STEPS, CHECK_AT, FACTOR = 1e-3, 6, (1, 3, 6), 8.0
SPREAD = {kind: dict(w=1.2e-7, loss=1.5e-7) for kind in ("regr", "clsf", "pretrain")}
CLSF_CFG = dict(n_classes=12, atom_features=167, frag_features=167, edge_features=17, num_layer=2, num_heads=4, drop_ratio=0.0,
                h1=64, act="relu", emb_dim=128, fthead="FTHead4")
PT_CFG = dict(num_layer=2, drop_ratio=0.0, edge_features=17)
SIZES = (8, 10, 12)


@functools.lru_cache(maxsize=None)
def _batches(kind):
    if kind == "pretrain":
        return tuple(data.collate_fn_pt(synth.synth_molecules(n, seed=300 + i, profile="esol", pretrain_targets=True))
                     for i, n in enumerate(SIZES))
    profile = "tox21" if kind == "clsf" else "esol"
    return tuple(data.collate_fn(synth.synth_molecules(n, seed=200 + i, profile=profile)) for i, n in enumerate(SIZES))


def _cast(batch, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}


def _oracle(kind):
    from oracle import fragnet_ref as ref
    torch.manual_seed(41)
    if kind == "pretrain":
        return ref.FragNetPreTrain(**PT_CFG).train(), lambda out, b: ref.pretrain_loss(out, b)
    if kind == "clsf":
        return ref.FragNetFineTune(**CLSF_CFG).train(), lambda out, b: ref.finetune_bce_loss(out, b["y"])
    return ref.FragNetFineTune(**CFG).train(), lambda out, b: ref.finetune_regr_loss(out, b["y"])


@functools.lru_cache(maxsize=None)
def oracle_trajectory(kind, dtype):
    """(initial state dict (float32), losses [6] as floats, {step: {name: float64 tensor}}) of the oracle run in ``dtype``.  Computed
    once per (model, dtype) and shared; callers do not modify it."""
    model, loss_fn = _oracle(kind)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    model.to(dtype)
    opt = torch.optim.Adam(model.parameters(), lr=LR, eps=ADAM_EPS)
    batches = [_cast(b, dtype) for b in _batches(kind)]
    losses, weights = [], {}
    for k in range(1, STEPS + 1):
        b = batches[(k - 1) % len(batches)]
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(model(dict(b)), b)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if k in CHECK_AT:
            weights[k] = {n: p.detach().double().clone() for n, p in model.named_parameters()}
    moved = max(float((weights[STEPS][n] - sd0[n].double()).abs().max()) for n in weights[STEPS])
    assert moved > 2 * LR, "the trajectory hardly moved: nothing to compare"
    return sd0, tuple(losses), weights


def distance(losses, weights, kind):
    """(largest absolute weight difference with its (step, name), largest loss difference relative to max(1, |loss|)) against the
    float64 oracle; ``weights`` = {step: {name: tensor}}"""
    _, ref_losses, ref_w = oracle_trajectory(kind, torch.float64)
    worst_w, where = 0.0, None
    for k in CHECK_AT:
        for n, want in ref_w[k].items():
            if n not in weights[k]:
                continue
            d = float((weights[k][n].detach().double().cpu() - want).abs().max())
            if d > worst_w:
                worst_w, where = d, (k, n)
    worst_l = max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(losses, ref_losses))
    return worst_w, where, worst_l


@pytest.mark.parametrize("kind", ["regr", "clsf", "pretrain"])
def test_float32_oracle_stays_within_the_recorded_spread_of_the_float64_oracle(kind):
    _, losses, weights = oracle_trajectory(kind, torch.float32)
    w, where, l = distance(losses, weights, kind)
    print(f"{kind}: float32 oracle vs float64 oracle: weights {w:.2e} at {where}, losses {l:.2e}")
    assert 0 < w <= SPREAD[kind]["w"] and 0 < l <= SPREAD[kind]["loss"]
    # what the bound is small against: one Adam step more or fewer
    _, _, w64 = oracle_trajectory(kind, torch.float64)
    one_step = max(float((w64[3][n] - w64[1][n]).abs().max()) for n in w64[1]) / 2
    assert one_step > 100 * FACTOR * SPREAD[kind]["w"]


# ----------------------------------------------------------------------------------------------------------------- GPU
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _hip_model(kind, dev):
    from fragnet_amd import train
    from fragnet_amd.model import FragNetFineTune, FragNetPreTrain
    sd0, _, _ = oracle_trajectory(kind, torch.float64)
    if kind == "pretrain":
        model, loss_fn = FragNetPreTrain(**PT_CFG), lambda out, b: train.pretrain_loss(out, b)
    elif kind == "clsf":
        model, loss_fn = FragNetFineTune(**CLSF_CFG), lambda out, b: train.compute_bce_loss(out, b["y"])
    else:
        model, loss_fn = FragNetFineTune(**CFG), lambda out, b: torch.nn.functional.mse_loss(out.view(-1), b["y"])
    model.load_state_dict(sd0)                       # the oracle's initial weights, reference key layout
    return model.to(dev).train(), loss_fn


def _snapshot(model):
    return {n: p.detach().clone() for n, p in model.named_parameters()}


def _report_and_check(kind, path, losses, weights):
    w, where, l = distance(losses, weights, kind)
    print(f"{kind} / {path}: HIP vs float64 oracle: weights {w:.2e} at {where} (bound {FACTOR * SPREAD[kind]['w']:.1e}), "
          f"losses {l:.2e} (bound {FACTOR * SPREAD[kind]['loss']:.1e})")
    assert l <= FACTOR * SPREAD[kind]["loss"], f"{kind} / {path}: loss off by {l:.2e}"
    assert w <= FACTOR * SPREAD[kind]["w"], f"{kind} / {path}: weights off by {w:.2e}, first worst at (step, parameter) {where}"


@gpu
@pytest.mark.parametrize("kind", ["regr", "clsf", "pretrain"])
def test_eager_steps_follow_the_float64_oracle(kind):
    from fragnet_amd import parallel
    dev = _dev()
    batches = [data.batch_to(b, dev) for b in _batches(kind)]
    model, loss_fn = _hip_model(kind, dev)
    opt = parallel.FlatAdam.for_live_parameters(model, lambda: loss_fn(model(dict(batches[0])), batches[0]).backward(), lr=LR, eps=ADAM_EPS)
    losses, weights = [], {}
    for k in range(1, STEPS + 1):
        b = batches[(k - 1) % len(batches)]
        opt.zero_grad()
        loss = loss_fn(model(dict(b)), b)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if k in CHECK_AT:
            weights[k] = _snapshot(model)
    assert opt.steps == STEPS
    _report_and_check(kind, "eager", losses, weights)


@gpu
@pytest.mark.parametrize("kind", ["regr", "clsf", "pretrain"])
def test_captured_steps_follow_the_float64_oracle(kind):
    from fragnet_amd import graphstep, parallel
    dev = _dev()
    batches = [data.batch_to(b, dev) for b in _batches(kind)]
    shapes = graphstep.StaticShapes.from_batches(batches, margin=0.05)
    model, loss_fn = _hip_model(kind, dev)
    opt = parallel.FlatAdam.for_live_parameters(model, lambda: loss_fn(model(dict(batches[0])), batches[0]).backward(), lr=LR, eps=ADAM_EPS)
    before = copy.deepcopy(_snapshot(model))
    step = graphstep.GraphedTrainStep(model, opt, shapes, dict(batches[0]), loss=kind)
    assert step.adam_in_graph
    if kind != "pretrain":                                # the head's slice of the update rides in the encoder's backward
        assert step._rider_lo is not None and 0 < step._rider_lo < opt.flat.numel()
    for n, p in model.named_parameters():                 # the capture and its warm-up steps must not move the weights
        assert torch.equal(p, before[n]), n
    losses, weights = [], {}
    for k in range(1, STEPS + 1):
        losses.append(float(step(dict(batches[(k - 1) % len(batches)]))))
        if k in CHECK_AT:
            weights[k] = _snapshot(model)
    assert step.replays == STEPS and step.fallbacks == 0 and opt.steps == STEPS
    _report_and_check(kind, "captured", losses, weights)
