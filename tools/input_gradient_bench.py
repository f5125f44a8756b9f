#!/usr/bin/env python3
"""Input-feature gradients on one GPU: what the extra launch costs, what the attributions deliver, and the only other route.

    python tools/input_gradient_bench.py [--repeats 5] [--batches 20] > profiles/input_grad_bench.txt

Model: the quick start's (4 layers, 4 heads, FTHead3 128/1024/1024/512, relu), eval(); 1024 ESOL-profile molecules, batches of 512.
Every timing is device events around the timed region, arms alternating in this one process, min / median / max of the repeats.
1. COST OF THE FEATURE: the backward pass of one batch (out[:, 0].sum().backward(), forward outside the timed region) with no input
   requiring a gradient -- the pass as it always was -- against the same pass with all three inputs requiring one (zero-filled
   scratch + fn_encoder_backward_inputs).  Then the new launch alone (fn_linear_dx_f32 on the batch's three shapes, dx written)
   against its compulsory bytes 4 (128 M + 128 K + M K) per task.
2. WHAT IT DELIVERS: attributed molecules per second of input_gradients and of integrated_gradients at 32 steps.
3. THE OTHER ROUTE: the same model with use_engine=False (one autograd node per operator) and torch autograd on the inputs,
   forward + backward per batch, against the engine's forward + backward -- after checking that both give the same gradients."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import fragnet_amd
from fragnet_amd import gradient_attribution as ga, ops, synth
from fragnet_amd.dataset import FlatMolStore

KEYS = ga.TABLE_KEYS


def spread(xs):
    return f"min {min(xs):.3f}  median {statistics.median(xs):.3f}  max {max(xs):.3f}"


def overlap(a, b):
    return "overlap" if min(a) <= max(b) and min(b) <= max(a) else "do not overlap"


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn, n):
    t0, t1 = events()
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / n


def leaf_batch(store, idx, need):
    batch = store.collate(idx)
    for k in KEYS:
        batch[k] = batch[k].detach().clone().requires_grad_(need)
    return batch


def backward_ms(model, batch, n):
    """ms per backward pass of out[:, 0].sum(); the forward runs outside the timed region."""
    total = 0.0
    for _ in range(n):
        model.zero_grad(set_to_none=True)
        for k in KEYS:
            batch[k].grad = None
        loss = model(batch)[:, 0].sum()
        t0, t1 = events()
        t0.record()
        loss.backward()
        t1.record()
        t1.synchronize()
        total += t0.elapsed_time(t1)
    return total / n


def step_ms(model, batch, n):
    def one():
        model.zero_grad(set_to_none=True)
        for k in KEYS:
            batch[k].grad = None
        model(batch)[:, 0].sum().backward()
    return timed(one, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", type=int, default=20)
    args = ap.parse_args()
    if args.repeats < 5 or args.batches < 5:
        ap.error("at least 5 repeats of 5 batches")
    fragnet_amd.prefer_rocblas_for_dense_heads()
    torch.manual_seed(5)
    from fragnet_amd.model import FragNetFineTune
    model = FragNetFineTune(n_classes=1, num_layer=4, drop_ratio=0.1, h1=128, h2=1024, h3=1024, h4=512, act="relu").to("cuda:0").eval()
    mols = synth.synth_molecules(1024, seed=4200, profile="esol")
    store = FlatMolStore.from_records(mols).to("cuda:0")
    idx = np.arange(512)
    plain, leaves = leaf_batch(store, idx, False), leaf_batch(store, idx, True)
    N, E, EF = (leaves[k].shape[0] for k in KEYS)
    Ka, Kb, Kf = (leaves[k].shape[1] for k in KEYS)

    # ---- 1. cost of the feature
    arms = {"parameters only": plain, "parameters + inputs": leaves}
    for b in arms.values():
        backward_ms(model, b, 3)
    ms = {k: [] for k in arms}
    for _ in range(args.repeats):
        for k, b in arms.items():
            ms[k].append(backward_ms(model, b, args.batches))
    print(f"1. cost of the feature: backward pass of one evaluation batch, 512 molecules ({N} atoms, {E} directed bonds, {EF} directed fragment bonds), "
          f"ms per pass, {args.repeats} repeats x {args.batches} passes, arms alternating")
    for k in arms:
        print(f"   {k:20s} {spread(ms[k])}")
    a, b = ms["parameters only"], ms["parameters + inputs"]
    print(f"   difference of the medians: {(statistics.median(b) - statistics.median(a)) * 1e3:+.1f} us; the two arms' spreads {overlap(a, b)}")
    g = [torch.randn(m, 128, device="cuda:0") for m in (N, E, EF)]
    W = [p.detach() for p in (model.pretrain.layers[0].projection_a.weight, model.pretrain.layers[0].projection_b.weight, model.pretrain.layers[0].projection_fb.weight)]
    dx = [torch.empty(m * k, device="cuda:0") for m, k in ((N, Ka), (E, Kb), (EF, Kf))]
    tasks = [(gi, Wi, di, None, None) for gi, Wi, di in zip(g, W, dx)]
    timed(lambda: ops.linear_dx(tasks), 20)
    own = [timed(lambda: ops.linear_dx(tasks), 200) for _ in range(args.repeats)]
    nbytes = sum(4 * (128 * m + 128 * k + m * k) for m, k in ((N, Ka), (E, Kb), (EF, Kf)))
    med = statistics.median(own)
    print(f"   the new launch alone (three tasks, dx written, 200 launches back to back per repeat): ms {spread(own)}; compulsory bytes {nbytes / 1e6:.2f} MB "
          f"= {nbytes / (med * 1e-3) / 1e9:.0f} GB/s at the median")

    # ---- 2. what it delivers
    ga.input_gradients(model, store)
    ga.integrated_gradients(model, store, steps=32)
    rate = {"input_gradients": [], "integrated_gradients, 32 steps": []}
    for _ in range(args.repeats):
        rate["input_gradients"].append(len(store) / (timed(lambda: ga.input_gradients(model, store), 1) * 1e-3))
        rate["integrated_gradients, 32 steps"].append(len(store) / (timed(lambda: ga.integrated_gradients(model, store, steps=32), 1) * 1e-3))
    print(f"2. what it delivers: {len(store)} molecules, attributed molecules/s (collate, host work and the copy back included)")
    for k, v in rate.items():
        print(f"   {k:32s} {spread(v)}")

    # ---- 3. the other route
    def grads_of(use_engine):
        model.pretrain.use_engine = use_engine
        try:
            batch = leaf_batch(store, idx, True)
            model.zero_grad(set_to_none=True)
            model(batch)[:, 0].sum().backward()
            return [batch[k].grad.double().cpu().numpy() for k in KEYS]
        finally:
            model.pretrain.use_engine = True
    eng, lvl = grads_of(True), grads_of(False)
    for k, x, y in zip(KEYS, eng, lvl):
        err, bound = np.abs(x - y), 1e-4 * np.abs(y).max() + 1e-4 * np.abs(y)
        assert (err <= bound).all(), f"{k}: the two routes disagree (max|diff| {err.max():.3e})"
        print(f"3. {k}: engine vs per-level route max|diff| {err.max():.3e} (max|grad| {np.abs(y).max():.3e}): inside 1e-4 max|ref| + 1e-4 |ref|")
    ms = {"engine": [], "use_engine=False": []}
    step_ms(model, leaves, 3)
    model.pretrain.use_engine = False
    try:
        step_ms(model, leaves, 3)
        for _ in range(args.repeats):
            model.pretrain.use_engine = True
            ms["engine"].append(step_ms(model, leaves, args.batches))
            model.pretrain.use_engine = False
            ms["use_engine=False"].append(step_ms(model, leaves, args.batches))
    finally:
        model.pretrain.use_engine = True
    print(f"   forward + backward of one batch with the three inputs requiring a gradient, ms, {args.repeats} repeats x {args.batches} batches, arms alternating")
    for k, v in ms.items():
        print(f"   {k:20s} {spread(v)}")
    print(f"   the two arms' spreads {overlap(ms['engine'], ms['use_engine=False'])}")


if __name__ == "__main__":
    main()
