"""Bit fingerprints of the captured training step (fragnet_amd/graphstep.py), in the manner of tools/engine_bits.py: run it on
two versions of the HOST code and diff the outputs.  A change that is meant to leave what the step launches alone -- the staging
table, the kernels, their order and arguments, the counters the replays read -- must leave every line alone.

    python tools/graphstep_bits.py > bits.txt
    python tools/graphstep_bits.py --calls > calls.txt

Cases (24 synthetic molecules per batch, profile esol, two layers): the regression step with Adam in the graph (head slice riding,
and with the rider off), with Adam outside the graph, as two graphs (overlap=True), the classification step, the pretrain step of
FragNetPreTrain and of FragNetPreTrainMasked2 (a second Philox stream), and GraphedForward.  Every training case runs replay,
replay, one batch of 48 molecules (beyond the capacities: the eager fallback), replay, replay.  Cases 3 and 5 hand the step plain
dicts; the others CollatedBatches, whose offsets table is one more staged field.

Per case: the staging table after construction as (kind, cap, width, pad_hi, pad_mod) per field; after every step the SHA-256 of
the loss, of the flat parameters and of the flat gradients, the device counters (dropout blocks, Adam steps, mask blocks), the
optimiser's host step count and replays/fallbacks.  With --calls: the fn_* entry points of the library in call order instead,
for the construction (warm-up + capture) and for every step."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import engine_bits
from engine_bits import digest, record_calls
from fragnet_amd import data, graphstep, parallel, synth, train
from fragnet_amd import model as M

DEV = "cuda:0"
B, BIG = 24, 48


def line(name, text):
    """one line of the record: the fingerprints, or (--calls) the library calls since the last line"""
    if engine_bits.CALLS is not None:
        engine_bits.report(name, [])
    else:
        torch.cuda.synchronize()
        print(f"{name:34s} {text}", flush=True)


def table(static):
    rows = [(f.kind, f.cap, f.width, f.pad_hi, f.pad_mod) for f in (static._fields[i] for i in range(static.n_fields))]
    return f"n_fields={static.n_fields} {rows}"


def make_batches(pretrain, clsf=False):
    coll = data.collate_fn_pt if pretrain else data.collate_fn
    out = []
    for n, seed in ((B, 61), (B, 62), (B, 63), (BIG, 64)):
        b = coll(synth.synth_molecules(n, seed=seed, profile="esol", pretrain_targets=pretrain))
        if clsf:        # 0 / 1 labels, every fifth one missing (train/utils.py:297: targets <= -0.5)
            y = (b["y"] > b["y"].median()).float()
            y[::5] = -1.0
            b["y"] = y
        out.append(data.batch_to(b, DEV))
    return out[:3], out[3]


def fresh(b, plain):
    """a copy the step may add its plan to: a CollatedBatch (layout promise + offsets table: FN_STAGE_OFFSETS is staged, the plan is
    built by the one-launch builder) or, ``plain``, a dict without either"""
    return dict(b) if plain else b.like(dict(b))


def train_case(name, loss="regr", cls=None, rider=True, plain=False, **kw):
    pretrain = loss == "pretrain"
    bs, big = make_batches(pretrain, loss == "clsf")
    torch.manual_seed(11)
    if pretrain:
        net = cls(num_layer=2, drop_ratio=0.1, edge_features=17) if cls is M.FragNetPreTrainMasked2 else \
            M.FragNetPreTrain(num_layer=2, drop_ratio=0.1, num_heads=4, emb_dim=128, atom_features=167, frag_features=167, edge_features=17)
        loss_of = lambda b: train.pretrain_loss(net(b), b)
    else:
        net = M.FragNetFineTune(n_classes=1, num_layer=2, num_heads=4, drop_ratio=0.1, h1=32, h2=32, h3=32, h4=32, act="relu", fthead="FTHead3")
        loss_of = (lambda b: torch.nn.functional.mse_loss(net(b).view(-1), b["y"])) if loss == "regr" else \
            (lambda b: graphstep.masked_bce_loss(net(b), b["y"], torch.ones(b["y"].shape[0], device=DEV)))
    net = net.to(DEV).train()
    net.pretrain.rng.seed = 5
    if getattr(net, "mask_rng", None) is not None:
        net.mask_rng.seed = 7
    opt = parallel.FlatAdam.for_live_parameters(net, lambda: loss_of(dict(bs[0])).backward(), lr=1e-3, eps=1e-4)
    net.pretrain.rng.offset = 0
    if getattr(net, "mask_rng", None) is not None:
        net.mask_rng.offset = 0
    shapes = graphstep.StaticShapes.from_batches(bs, margin=0.05)
    if engine_bits.CALLS is not None:
        engine_bits.CALLS.clear()
    was = graphstep.ADAM_RIDER
    graphstep.ADAM_RIDER = rider
    try:
        step = graphstep.GraphedTrainStep(net, opt, shapes, fresh(bs[0], plain), loss=loss, **kw)
        line(f"{name} built", f"split={step.split} adam_in_graph={step.adam_in_graph} head_off={step.head_off} {table(step.static)}")
        for i, b in enumerate((bs[1], bs[2], big, bs[0], bs[1])):
            l = step(fresh(b, plain)).clone()
            counters = [int(step.rng.dev), int(step._counters[1])] + ([int(step.mask_rng.dev)] if step.mask_rng is not None else [])
            line(f"{name} step{i}", f"loss={digest([('loss', l)])} flat={digest([('flat', opt.flat)])} grad={digest([('grad', opt.grad)])} "
                                    f"counters={counters} steps={opt.steps} replays={step.replays} fallbacks={step.fallbacks}")
        assert step.replays == 4 and step.fallbacks == 1
    finally:
        graphstep.ADAM_RIDER = was


def forward_case(name):
    bs, big = make_batches(False)
    torch.manual_seed(11)
    net = M.FragNetFineTune(n_classes=1, num_layer=2, num_heads=4, drop_ratio=0.1, h1=32, h2=32, h3=32, h4=32, act="relu", fthead="FTHead3").to(DEV).eval()
    shapes = graphstep.StaticShapes.from_batches(bs, margin=0.05)
    if engine_bits.CALLS is not None:
        engine_bits.CALLS.clear()
    fwd = graphstep.GraphedForward(net, shapes, fresh(bs[0], False))
    line(f"{name} built", table(fwd.static))
    for i, b in enumerate((bs[1], bs[2], big, bs[0], bs[1])):
        out = fwd(fresh(b, False)).clone()
        line(f"{name} call{i}", f"out={digest([('out', out)])} replays={fwd.replays} fallbacks={fwd.fallbacks}")
    assert fwd.replays == 4 and fwd.fallbacks == 1


def main():
    train_case("1 regr adam+rider")
    train_case("2 regr rider off", rider=False)
    train_case("3 regr capture_adam=False", capture_adam=False, plain=True)
    train_case("4 regr overlap", overlap=True)
    train_case("5 clsf", loss="clsf", plain=True)
    train_case("6 pretrain", loss="pretrain")
    train_case("7 pretrain masked2", loss="pretrain", cls=M.FragNetPreTrainMasked2)
    forward_case("8 forward")


if __name__ == "__main__":
    if "--calls" in sys.argv[1:]:
        record_calls()
    main()
