#!/usr/bin/env python3
"""Side benchmark of the captured pair step on one GPU: the quick start's CDRP and DTA models (num_layer 4) on batches of 256 pairs,
drop_ratio 0 and 0.15, the launch-by-launch training step against graphstep.PairGraphedTrainStep, in ONE process, interleaved rounds.
    eager      what TrainerFineTuneCDRP / TrainerFineTuneDTA run per batch without ``graph_step``: zero_grad, the model's fused-loss call,
               backward, FlatAdam.step;
    captured   ``step(batch)``: the staging launch and one hipGraph replay (Adam inside);
    fwd+bwd    the eager step without its optimiser calls -- what DESIGN section 7k timed -- for orientation only.
Each arm trains a copy of its own of the same initial model on the same cycle of batches; a batch arrives as a fresh dict every time,
as from a loader, so the eager arms build its graph plan in every step (the captured step builds it inside the graph).  A window is --steps steps closed by a
synchronise: wall = host clock over the window, device = the span between two events around it, both per step.  Reported: the median,
min and max of --rounds windows.
dev tool: python tools/pair_graphstep_bench.py [--rounds 10] [--steps 5] [--markdown profiles/pair_graphstep.md]     prints one JSON line last"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import fragnet_amd
from fragnet_amd import _lib, data, graphstep, ops, parallel, synth
from fragnet_amd.cdrp import CDRPModel, FragNetFineTuneBase
from fragnet_amd.dta import DTAModel2

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=256)
ap.add_argument("--pool", type=int, default=4, help="distinct batches the arms cycle through (the capacities are sized from them)")
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--steps", type=int, default=5, help="steps per timed window")
ap.add_argument("--markdown", default=None, help="also write the table to this file")
args = ap.parse_args()
assert torch.cuda.is_available(), "pair_graphstep_bench needs a GPU: a timing taken anywhere else says nothing"
dev = torch.device("cuda:0")
fragnet_amd.prefer_rocblas_for_dense_heads()
M, GD = args.pairs, 903
CTOR = dict(n_classes=1, num_layer=4, h1=128, h2=1024, h3=1024, h4=512, act="relu")
unit = ops.unit_grad(dev)


def model_of(kind, drop):
    torch.manual_seed(0)
    base = FragNetFineTuneBase(drop_ratio=drop, **CTOR)
    return (CDRPModel(base, GD, dev) if kind == "cdrp" else DTAModel2(base)).to(dev).train()


def pool_of(kind):
    out = []
    for i in range(args.pool):
        mols = synth.synth_molecules(M, seed=1200 + i, profile="esol")
        recs = synth.attach_gene_expr(mols, GD, 1300 + i) if kind == "cdrp" else synth.attach_protein(mols, 1300 + i)
        out.append(data.batch_to((data.collate_fn_cdrp if kind == "cdrp" else data.collate_fn_dta)(recs), dev))
    return out


def fused(model, b):
    return model(b, loss=(_lib.LOSS_MSE, b["y"], None))[1]


def optimiser(model, b):
    return parallel.FlatAdam.for_live_parameters(model, lambda: fused(model, b).backward(), lr=1e-4)


class Cycle:
    """``fn(batch)`` over the pool, round and round"""

    def __init__(self, fn, pool):
        self.fn, self.pool, self.i = fn, pool, 0

    def __call__(self):
        b = self.pool[self.i % len(self.pool)]
        self.fn(b.like(dict(b)))           # a dict of its own, as a loader's batch is: nothing cached on it (the graph plan) is reused
        self.i += 1


def window(fn, n):
    """(wall ms per step, device ms per step) of n steps closed by a synchronise"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n, e0.elapsed_time(e1) / n


def interleaved(arms, rounds, steps):
    for _ in range(3):
        for fn in arms.values():
            window(fn, 2)
    out = {k: [] for k in arms}
    for _ in range(rounds):                # A, B, C, A, B, C, ...
        for k, fn in arms.items():
            out[k].append(window(fn, steps))
    return out


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


rows, res = [], {"what": "captured against launch-by-launch pair training step, one MI355X", "pairs": M, "num_layer": 4, "rounds": args.rounds,
                 "steps_per_window": args.steps, "pool": args.pool, "rows": []}
for kind in ("cdrp", "dta"):
    pool = pool_of(kind)
    shapes = graphstep.StaticShapes.from_batches(pool, margin=0.05)
    for drop in (0.0, 0.15):
        m_eager = model_of(kind, drop)
        m_graph, m_plain = copy.deepcopy(m_eager), copy.deepcopy(m_eager)
        o_eager, o_graph = optimiser(m_eager, pool[0]), optimiser(m_graph, pool[0])
        step = graphstep.PairGraphedTrainStep(m_graph, o_graph, shapes, pool[0])

        def eager(b):
            o_eager.zero_grad()
            fused(m_eager, b).backward()
            o_eager.step()

        def plain(b):
            for p in m_plain.parameters():
                p.grad = None
            fused(m_plain, b).backward(gradient=unit)

        t = interleaved({"eager": Cycle(eager, pool), "captured": Cycle(step, pool), "fwd_bwd": Cycle(plain, pool)}, args.rounds, args.steps)
        r = dict(model=kind, drop_ratio=drop, replays=step.replays, fallbacks=step.fallbacks, adam_in_graph=bool(step.adam_in_graph),
                 mol_capacity=shapes.cap["mol"])
        for k, v in t.items():
            r[k + "_wall_ms"], r[k + "_device_ms"] = stats([w for w, _ in v]), stats([d for _, d in v])
        r["captured_over_eager_wall"] = r["captured_wall_ms"]["median"] / r["eager_wall_ms"]["median"]
        res["rows"].append(r)
        cell = lambda s: f"{s['median']:.3f} ({s['min']:.3f} .. {s['max']:.3f})"
        rows.append(f"| {kind} | {drop} | {cell(r['eager_wall_ms'])} | {cell(r['eager_device_ms'])} | {cell(r['captured_wall_ms'])} | "
                    f"{cell(r['captured_device_ms'])} | {r['captured_over_eager_wall']:.2f} | {cell(r['fwd_bwd_wall_ms'])} | {step.replays} / {step.fallbacks} |")
        del step

table = "\n".join(["| model | drop_ratio | eager wall ms | eager device ms | captured wall ms | captured device ms | captured / eager (wall medians) | "
                   "eager fwd+bwd only, wall ms | replays / fallbacks |", "|---|---|---|---|---|---|---|---|---|"] + rows)
print(table)
if args.markdown:
    with open(args.markdown, "w") as f:
        f.write("# The captured pair step against the launch-by-launch step\n\n"
                f"`tools/pair_graphstep_bench.py --rounds {args.rounds} --steps {args.steps}` on one MI355X: {M} pairs per training step, the quick "
                "start's models (num_layer 4), a full optimiser step both ways (eager: zero_grad, fused-loss forward, backward, FlatAdam.step; "
                "captured: one staging launch and one hipGraph replay with Adam inside), each arm on a copy of its own of the same initial model, "
                f"cycling through the same {args.pool} batches, interleaved in one process.  A window is {args.steps} steps closed by a synchronise; "
                "wall is the host clock over it, device the span between two events around it, both per step: median (min .. max) of "
                f"{args.rounds} windows.  The last timing column is the eager step without its optimiser calls, the quantity DESIGN section 7k "
                "reported.\n\n" + table + "\n\nRaw numbers:\n\n```json\n" + json.dumps(res, indent=1) + "\n```\n")
print(json.dumps(res))
