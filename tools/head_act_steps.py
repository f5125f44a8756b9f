#!/usr/bin/env python3
"""Captured finetune training step per head activation: median step time of one configuration, one JSON line.
dev tool:  python tools/head_act_steps.py CONFIG [--root TREE] [--steps N] [--warmup W]

CONFIG = esol-<act> (ESOL shape, FTHead3 128/1024/1024/512, B = 512, regression) or tox21-<act> (Tox21 shape, FTHead4 h1 = 128,
12 tasks, B = 1024, masked BCE); drop 0.1, the whole-step hipGraph (graphstep.GraphedTrainStep).  --root imports fragnet_amd from
another checkout (an A/B against a worktree of another commit: the same script, the other tree's kernels and heads)."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("config")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=8)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402

from fragnet_amd import data, graphstep, parallel, synth, train  # noqa: E402
from fragnet_amd.model import FragNetFineTune  # noqa: E402

shape, act = args.config.split("-", 1)
dev = torch.device("cuda:0")
if shape == "esol":
    B, profile, loss = 512, "esol", "regr"
    cfg = dict(n_classes=1, num_layer=4, drop_ratio=0.1, h1=128, h2=1024, h3=1024, h4=512, act=act, fthead="FTHead3")
else:
    B, profile, loss = 1024, "tox21", "clsf"
    cfg = dict(n_classes=12, num_layer=4, drop_ratio=0.1, h1=128, act=act, fthead="FTHead4")
batches = [data.batch_to(data.collate_fn(synth.synth_molecules(B, seed=80 + i, profile=profile)), dev) for i in range(3)]
shapes = graphstep.StaticShapes.from_batches(batches, margin=0.02, spread_sigmas=0.0)
torch.manual_seed(5)
model = FragNetFineTune(**cfg).to(dev).train()


def fresh(b):
    return b.like(b)


def probe():
    out = model(fresh(batches[0]))
    y = batches[0]["y"]
    (torch.nn.functional.mse_loss(out.view(-1), y) if loss == "regr" else train.compute_bce_loss(out, y)).backward()


opt = parallel.FlatAdam.for_live_parameters(model, probe, lr=1e-4)
step = graphstep.GraphedTrainStep(model, opt, shapes, fresh(batches[0]), loss=loss)
for i in range(args.warmup):
    step(fresh(batches[i % 3]))
torch.cuda.synchronize()
times = []
for i in range(args.steps):
    b = fresh(batches[i % 3])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    step(b)
    e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1))
times.sort()
print(json.dumps({"config": args.config, "root": os.path.basename(os.path.abspath(args.root)), "B": B,
                  "median_ms": round(times[len(times) // 2], 4), "min_ms": round(times[0], 4), "replays": step.replays,
                  "fallbacks": step.fallbacks, "loss": round(float(step.loss), 6)}))
