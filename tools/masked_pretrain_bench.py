#!/usr/bin/env python3
"""Side benchmark of masked-atom pretraining (model_version gat2_masked2) on one GPU: the captured pretrain step at the ESOL-shape
batch of 512 (tools/pretrain_bench.py's configuration), for FragNetPreTrainMasked2 and for FragNetPreTrain in ONE process,
interleaved A/B windows, timed with device events, medians.  The yardstick of the masked step is the unmasked step of the same run:
the masked step is that step plus the sampler launch (csrc/row_sample.hip) and the gate inside the prologue's pass over x_atoms.
Also timed: the sampler launch alone at the step's atom capacity.
dev tool: python tools/masked_pretrain_bench.py [--rounds 20] [--steps 30] [--out profiles/masked_pretrain_step.txt]   prints one JSON line last"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import fragnet_amd
from fragnet_amd import data, graphstep, ops, parallel, synth, train
from fragnet_amd.model import FragNetPreTrain, FragNetPreTrainMasked2

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--steps", type=int, default=30, help="steps per timed window")
ap.add_argument("--out", default=None, help="also write the figures as text to this file")
args = ap.parse_args()
assert torch.cuda.is_available(), "masked_pretrain_bench needs a GPU: a timing taken anywhere else says nothing"
dev = torch.device("cuda:0")
fragnet_amd.prefer_rocblas_for_dense_heads()
fragnet_amd.tune_library_gemms()
B = 512
batches = [data.batch_to(data.collate_fn_pt(synth.synth_molecules(B, seed=60 + i, profile="esol", pretrain_targets=True)), dev)
           for i in range(4)]
shapes = graphstep.StaticShapes.from_batches(batches, margin=0.02, spread_sigmas=0.0)


def fresh(b):
    return b.like(b)


def make(cls):
    torch.manual_seed(5)
    model = cls(num_layer=4, drop_ratio=0.2, edge_features=17).to(dev).train()
    opt = parallel.FlatAdam.for_live_parameters(model, lambda: train.pretrain_loss(model(fresh(batches[0])), batches[0]).backward(), lr=1e-4)
    return graphstep.GraphedTrainStep(model, opt, shapes, fresh(batches[0]), loss="pretrain")


steps = {"unmasked": make(FragNetPreTrain), "masked": make(FragNetPreTrainMasked2)}
count = {k: 0 for k in steps}


def window(name, n):
    step = steps[name]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step(fresh(batches[count[name] % 4]))
        count[name] += 1
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


for _ in range(3):                         # warm: every batch shape of the timed windows, both models
    for name in steps:
        window(name, 8)
times = {k: [] for k in steps}
for _ in range(args.rounds):               # interleaved: unmasked, masked, unmasked, masked, ...
    for name in steps:
        times[name].append(window(name, args.steps))

cap = shapes.cap["atom"]
rng = ops.mask_stream()
n_dev = torch.tensor([batches[0]["x_atoms"].shape[0]], dtype=torch.int32, device=dev)
out = torch.empty(cap, dtype=torch.uint8, device=dev)
sampler = []
for r in range(args.rounds + 3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(100):
        ops.sample_rows(cap, 0.85, rng, dev, n_dev=n_dev, out=out)
    e1.record()
    e1.synchronize()
    if r >= 3:
        sampler.append(e0.elapsed_time(e1) / 100)

med = {k: statistics.median(v) for k, v in times.items()}
res = {
    "batch": B, "atom_capacity": cap, "real_atoms": int(n_dev), "rounds": args.rounds, "steps_per_window": args.steps,
    "unmasked_ms": {"median": med["unmasked"], "min": min(times["unmasked"])},
    "masked_ms": {"median": med["masked"], "min": min(times["masked"])},
    "difference_ms": med["masked"] - med["unmasked"],
    "difference_pct_of_step": 100.0 * (med["masked"] - med["unmasked"]) / med["unmasked"],
    "paired_difference_ms_median": statistics.median(m - u for m, u in zip(times["masked"], times["unmasked"])),
    "sampler_launch_back_to_back_ms": {"median": statistics.median(sampler), "min": min(sampler)},
    "molecules_per_s": {k: B / v * 1e3 for k, v in med.items()},
    "replays": {k: s.replays for k, s in steps.items()}, "fallbacks": {k: s.fallbacks for k, s in steps.items()},
    "kept_last_step": int(steps["masked"].keep_mask[: int(n_dev)].sum()),
}
text = (f"captured pretrain step, ESOL-shape batch of {B} (atom capacity {cap}), {args.rounds} interleaved rounds of {args.steps} steps, device events\n"
        f"unmasked (FragNetPreTrain)        median {med['unmasked']:.4f} ms   min {min(times['unmasked']):.4f} ms   {res['molecules_per_s']['unmasked']:.0f} molecules/s\n"
        f"masked   (FragNetPreTrainMasked2) median {med['masked']:.4f} ms   min {min(times['masked']):.4f} ms   {res['molecules_per_s']['masked']:.0f} molecules/s\n"
        f"difference of the medians {res['difference_ms'] * 1e3:.1f} us = {res['difference_pct_of_step']:.2f} % of the step; median of the paired differences "
        f"{res['paired_difference_ms_median'] * 1e3:.1f} us\n"
        f"sampler launch alone, back to back at that capacity: median {statistics.median(sampler) * 1e3:.2f} us, min {min(sampler) * 1e3:.2f} us\n"
        f"replays {res['replays']}, fallbacks {res['fallbacks']}\n")
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
print(json.dumps(res))
