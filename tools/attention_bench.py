#!/usr/bin/env python3
"""Attention read-outs on one GPU: what the read-out costs on top of the plain evaluation pass, and what the engine route buys over
the per-level route.

    python tools/attention_bench.py [--repeats 5] [--batches 20] > profiles/attn_readout_bench.txt

1024 ESOL-profile molecules (two batches of 512; the timed batch is the first); arms alternate in this one process; min / median /
max over the repeats, each repeat timing `--batches` batches with device events (forward only, under no_grad).
1. COST OF THE READ-OUT: the read-out pass (FragNetFineTuneViz, eval: fn_encoder_forward_attn) against the plain evaluation pass of
   the same batch and weights (FragNetFineTune: fn_encoder_forward) -- the last layer's probability stores plus the one launch.
2. ENGINE AGAINST PER-LEVEL: the read-out pass against the only route there was before it: the same model with use_engine=False,
   i.e. `return_attentions` on the last layer, every layer one launch per operator, one fn_attn_by_src_f32 launch per level.
3. END TO END: attention.attention_weights on the 1024-molecule store (collate, passes, copies to the host, split), molecules/s.
Model: the quick start's (4 layers, 4 heads, FTHead3 128/1024/1024/512, relu)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import fragnet_amd
from fragnet_amd import attention, synth
from fragnet_amd.dataset import FlatMolStore
from fragnet_amd.model import FragNetFineTune
from fragnet_amd.viz_model import FragNetFineTuneViz


def spread(xs):
    return f"min {min(xs):.3f}  median {statistics.median(xs):.3f}  max {max(xs):.3f}"


def timed(fn, n):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / n


def verdict(fast, slow):
    """Is the `fast` arm faster than the `slow` arm by more than the two arms' run-to-run spread?"""
    if max(fast) < min(slow):
        return f"every repeat of the first arm is faster than every repeat of the second: outside both spreads ({min(slow) / max(fast):.2f} x at the least, {statistics.median(slow) / statistics.median(fast):.2f} x by medians)"
    return "the two arms' spreads overlap: no difference beyond run-to-run spread"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", type=int, default=20)
    args = ap.parse_args()
    if args.repeats < 5 or args.batches < 20:
        ap.error("at least 5 repeats of 20 batches")
    fragnet_amd.prefer_rocblas_for_dense_heads()
    torch.manual_seed(5)
    cfg = dict(n_classes=1, num_layer=4, drop_ratio=0.1, h1=128, h2=1024, h3=1024, h4=512, act="relu", edge_features=17)
    plain = FragNetFineTune(**cfg).to("cuda:0").eval()
    viz = FragNetFineTuneViz(**cfg).to("cuda:0").eval()
    viz.load_state_dict(plain.state_dict(), strict=True)
    slow = FragNetFineTuneViz(**cfg).to("cuda:0").eval()
    slow.load_state_dict(plain.state_dict(), strict=True)
    slow.use_engine = False
    store = FlatMolStore.from_records(synth.synth_molecules(1024, seed=4200, profile="esol")).to("cuda:0")
    batch = store.collate(np.arange(512))
    N, E, F_, EF = (batch[k].shape[0] for k in ("x_atoms", "node_features_bonds", "x_frags", "node_features_fbonds"))
    arms = {"plain evaluation pass": lambda: plain(batch), "read-out pass (engine)": lambda: viz(batch), "read-out, per-level route": lambda: slow(batch)}
    with torch.no_grad():
        for fn in arms.values():          # plans, library GEMM selection, allocator: outside the timed region
            timed(fn, 5)
        ms = {k: [] for k in arms}
        for _ in range(args.repeats):
            for k, fn in arms.items():
                ms[k].append(timed(fn, args.batches))
        a, b = viz(batch), slow(batch)
        worst = max(float((x - y).abs().max()) for x, y in zip(a, b))
    print(f"batch: 512 molecules, {N} atoms, {E} directed bonds, {F_} fragments, {EF} directed fragment connections; ms per batch (forward only, "
          f"model(batch) under no_grad), {args.repeats} repeats x {args.batches} batches, arms alternating; largest |engine - per-level| over the five outputs {worst:.2e}")
    for k in arms:
        print(f"   {k:27s} {spread(ms[k])}")
    p, r, s = ms["plain evaluation pass"], ms["read-out pass (engine)"], ms["read-out, per-level route"]
    over = statistics.median(r) / statistics.median(p) - 1.0
    inside = "inside" if max(r) <= max(p) and min(r) >= min(p) else "outside"
    print(f"1. cost of the read-out: read-out / plain medians {over * 100:+.2f} % ({(statistics.median(r) - statistics.median(p)) * 1e3:+.1f} us per batch); the read-out arm is {inside} the plain arm's own spread")
    print(f"2. engine against per-level: {verdict(r, s)}")
    attention.attention_weights(viz, store)              # warm-up
    torch.cuda.synchronize()
    secs = []
    for _ in range(5):
        t0 = time.perf_counter()
        res = attention.attention_weights(viz, store)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    rows = sum(int(res.offsets[k][-1]) for k in attention.LEVELS)
    print(f"3. attention_weights end to end: {len(res)} molecules, {rows} read-out rows; seconds {spread(secs)} (5 runs, host and device, collate, "
          f"copies and split included) = {len(res) / statistics.median(secs):.0f} molecules/s")


if __name__ == "__main__":
    main()
