#!/usr/bin/env python3
"""Side benchmark of the captured FACTORED pair step on one GPU: the quick start's CDRP and DTA models (num_layer 4), drop_ratio 0 and
0.15, on pair tables of profiles/pair_factored.md's shapes -- M pairs over U distinct drugs and C distinct second inputs -- three
arms on the SAME records, in ONE process, interleaved rounds.
    eager factored        what the trainers run per batch with ``finetune.factored_pairs``: zero_grad, the model's fused-loss call on the
                          factored batch (orderings from the collate), backward, FlatAdam.step;
    captured per pair     graphstep.PairGraphedTrainStep on the one-record-per-pair collate of the same records (``finetune.graph_step``);
    captured factored     graphstep.FactoredPairGraphedTrainStep on the factored collate (``finetune.factored_graph_step``): the staging
                          launch and one hipGraph replay with the orderings launch and Adam inside.
Each arm trains a copy of its own of the same initial model on the same cycle of --pool tables; a batch arrives as a fresh dict every
time, as from a loader.  A window is --steps full optimiser steps closed by a synchronise: wall = host clock over the window, device =
the span between two events around it, both per step.  Reported: the median, min and max of --rounds windows.
dev tool: python tools/pair_factored_graphstep_bench.py [--rounds 10] [--steps 5] [--markdown profiles/pair_factored_graphstep.md]
prints one JSON line last"""
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
from fragnet_amd import _lib, data, graphstep, parallel, synth
from fragnet_amd.cdrp import CDRPModel, FragNetFineTuneBase
from fragnet_amd.dta import DTAModel2

SHAPES = ((256, 256, 256), (256, 32, 64), (256, 8, 16), (2048, 32, 64))          # (pairs, distinct drugs, distinct second inputs)
ap = argparse.ArgumentParser()
ap.add_argument("--pool", type=int, default=4, help="distinct tables the arms cycle through (the capacities are sized from them)")
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--steps", type=int, default=5, help="steps per timed window")
ap.add_argument("--kinds", default="cdrp,dta")
ap.add_argument("--markdown", default=None, help="also write the table to this file")
args = ap.parse_args()
assert torch.cuda.is_available(), "pair_factored_graphstep_bench needs a GPU: a timing taken anywhere else says nothing"
dev = torch.device("cuda:0")
fragnet_amd.prefer_rocblas_for_dense_heads()
GD = 903
CTOR = dict(n_classes=1, num_layer=4, h1=128, h2=1024, h3=1024, h4=512, act="relu")


def model_of(kind, drop):
    torch.manual_seed(0)
    base = FragNetFineTuneBase(drop_ratio=drop, **CTOR)
    return (CDRPModel(base, GD, dev) if kind == "cdrp" else DTAModel2(base)).to(dev).train()


def pools_of(kind, M, U, C):
    """(factored batches, one-record-per-pair batches) of the same --pool tables"""
    fac, per = [], []
    for i in range(args.pool):
        recs = synth.pair_records(M, U, C, kind, 1200 + 17 * i, gene_dim=GD)
        fac.append(data.batch_to((data.collate_fn_cdrp_factored if kind == "cdrp" else data.collate_fn_dta_factored)(recs), dev))
        per.append(data.batch_to((data.collate_fn_cdrp if kind == "cdrp" else data.collate_fn_dta)(recs), dev))
    return fac, per


def fused(model, b):
    return model(b, loss=(_lib.LOSS_MSE, b["y"], None))[1]


def optimiser(model, b):
    return parallel.FlatAdam.for_live_parameters(model, lambda: fused(model, b.like(dict(b))).backward(), lr=1e-4)


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


ARMS = ("eager_factored", "captured_per_pair", "captured_factored")
rows, res = [], {"what": "captured factored pair step against the eager factored and the captured one-record-per-pair step, one MI355X",
                 "num_layer": 4, "rounds": args.rounds, "steps_per_window": args.steps, "pool": args.pool, "rows": []}
for kind in args.kinds.split(","):
    for M, U, C in SHAPES:
        fac, per = pools_of(kind, M, U, C)
        shapes_f = graphstep.FactoredPairShapes.from_batches(fac, margin=0.05)
        shapes_p = graphstep.StaticShapes.from_batches(per, margin=0.05)
        for drop in (0.0, 0.15):
            m_eager = model_of(kind, drop)
            m_per, m_fac = copy.deepcopy(m_eager), copy.deepcopy(m_eager)
            o_eager, o_per, o_fac = optimiser(m_eager, fac[0]), optimiser(m_per, per[0]), optimiser(m_fac, fac[0])
            s_per = graphstep.PairGraphedTrainStep(m_per, o_per, shapes_p, per[0].like(dict(per[0])))
            s_fac = graphstep.FactoredPairGraphedTrainStep(m_fac, o_fac, shapes_f, fac[0].like(dict(fac[0])))

            def eager(b):
                o_eager.zero_grad()
                fused(m_eager, b).backward()
                o_eager.step()

            t = interleaved({"eager_factored": Cycle(eager, fac), "captured_per_pair": Cycle(s_per, per), "captured_factored": Cycle(s_fac, fac)},
                            args.rounds, args.steps)
            r = dict(model=kind, pairs=M, drugs=U, seconds=C, drop_ratio=drop, per_pair_replays=s_per.replays, per_pair_fallbacks=s_per.fallbacks,
                     factored_replays=s_fac.replays, factored_fallbacks=s_fac.fallbacks, adam_in_graph=bool(s_fac.adam_in_graph),
                     stage_fields=int(s_fac.static.n_fields), factored_capacities=dict(mol=shapes_f.cap["mol"], pair=shapes_f.pair_cap,
                                                                                       second=shapes_f.second_cap))
            for k, v in t.items():
                r[k + "_wall_ms"], r[k + "_device_ms"] = stats([w for w, _ in v]), stats([d for _, d in v])
            res["rows"].append(r)
            cell = lambda s: f"{s['median']:.3f} ({s['min']:.3f} .. {s['max']:.3f})"
            rows.append(f"| {kind} | {M} over {U} x {C} | {drop} | " + " | ".join(cell(r[a + "_wall_ms"]) + " | " + cell(r[a + "_device_ms"]) for a in ARMS)
                        + f" | {s_per.replays} / {s_per.fallbacks} | {s_fac.replays} / {s_fac.fallbacks} |")
            print(rows[-1], flush=True)
            del s_per, s_fac

table = "\n".join(["| model | pairs over drugs x second inputs | drop_ratio | " + " | ".join(f"{a.replace('_', ' ')} wall ms | {a.replace('_', ' ')} device ms" for a in ARMS)
                   + " | per pair: replays / fallbacks | factored: replays / fallbacks |", "|" + "---|" * 11] + rows)
print(table)
if args.markdown:
    with open(args.markdown, "w") as f:
        f.write("# The captured factored pair step\n\n"
                f"`tools/pair_factored_graphstep_bench.py --rounds {args.rounds} --steps {args.steps}` on one MI355X: the quick start's models "
                "(num_layer 4), a full optimiser step in three ways on the same records -- eager on the factored batch (zero_grad, fused-loss "
                "forward, backward, FlatAdam.step), `PairGraphedTrainStep` on the one-record-per-pair batch, `FactoredPairGraphedTrainStep` on the "
                "factored batch (captured: one staging launch and one hipGraph replay with Adam inside) -- each arm on a copy of its own of the same "
                f"initial model, cycling through the same {args.pool} tables, interleaved in one process.  A window is {args.steps} steps closed by a "
                "synchronise; wall is the host clock over it, device the span between two events around it, both per step: median (min .. max) "
                f"of {args.rounds} windows.\n\n" + table + "\n\nRaw numbers:\n\n```json\n" + json.dumps(res, indent=1) + "\n```\n")
print(json.dumps(res))
