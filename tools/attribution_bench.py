#!/usr/bin/env python3
"""Leave-one-out attribution on one GPU: what the row masks cost, and what the batched form buys.

    python tools/attribution_bench.py [--repeats 5] [--batches 20] [--sample 200] > profiles/attr_loo_bench.txt

1. COST OF THE MASK: forward-only time per batch of the masked pass against the UNMASKED evaluation pass of the same replica
   batch (~2048 replica molecules), both arms in this one process, alternating; min / median / max over the repeats, each repeat
   timing `--batches` batches with device events.  The yardstick is the unmasked arm.
2. WHAT THE FEATURE BUYS: attributed molecules per second of attribution.leave_one_out for a six-molecule set and a 1024-molecule
   ESOL-profile store, against the only other way to the same numbers: the per-layer scalar mask attributes, which leave the
   engine for the per-level path, one molecule and one masked element per forward.  That arm is timed on a SAMPLE of the replicas
   (`--sample`, spread evenly over the replica list) and EXTRAPOLATED to all of them.
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
from fragnet_amd import attribution as attr, data, synth
from fragnet_amd.dataset import FlatMolStore
from fragnet_amd.model import MASK_KEYS, FragNetFineTune

ATTRS = {attr.KIND_ATOM: "atom_mask_individual", attr.KIND_BOND: "bond_mask", attr.KIND_FBOND: "frag_bond_mask"}


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


def mask_cost(model, store, args):
    lens = store._host_lengths()
    table = attr.replica_table(lens["atom"], lens["edge"], lens["fedge"])
    mols = np.repeat(np.arange(len(store)), [t.shape[0] for t in table])[:2048]
    reps = np.concatenate(table, 0)[:2048]
    batch = store.collate(mols)
    status = torch.zeros(1, dtype=torch.int32, device=store.device)
    masks = attr.build_row_masks(batch, torch.from_numpy(attr.local_index(reps)).to(store.device), status)
    masked = batch.like({**batch, **dict(zip(MASK_KEYS, masks))})
    N, E, EF = (batch[k].shape[0] for k in ("x_atoms", "node_features_bonds", "node_features_fbonds"))
    arms = {"unmasked": lambda: model(batch), "masked": lambda: model(masked)}
    with torch.no_grad():
        for fn in arms.values():          # the plan of either batch is built here, outside the timed region
            timed(fn, 5)
        ms = {k: [] for k in arms}
        for _ in range(args.repeats):
            for k, fn in arms.items():
                ms[k].append(timed(fn, args.batches))
    assert int(status.item()) == 0
    print(f"1. cost of the mask: {len(mols)} replica molecules, {N} atoms, {E} directed bonds, {EF} directed fragment bonds; "
          f"mask bytes {N + E + EF}; ms per batch (forward only, model(batch) under no_grad), {args.repeats} repeats x {args.batches} batches, arms alternating")
    for k in arms:
        print(f"   {k:9s} {spread(ms[k])}")
    over = statistics.median(ms["masked"]) / statistics.median(ms["unmasked"]) - 1.0
    verdict = "inside" if max(ms["masked"]) <= max(ms["unmasked"]) else f"{(min(ms['masked']) / max(ms['unmasked']) - 1) * 100:+.1f} % (masked min against unmasked max) outside"
    print(f"   masked / unmasked medians: {over * 100:+.2f} %; the masked arm is {verdict} the unmasked arm's own spread")


def scalar_path(model, mols, sample):
    """Seconds per replica of the per-level path: scalar layer attributes, one molecule and one masked element per forward."""
    reps = [(i, int(k), int(x)) for i, m in enumerate(mols) for k, x in attr.replica_table([m.x_atoms.shape[0]], [m.node_features_bonds.shape[0]],
                                                                                           [m.node_feautures_fbondg.shape[0]])[0]]
    pick = [reps[j] for j in np.linspace(0, len(reps) - 1, min(sample, len(reps))).astype(int)]
    batches = {i: data.batch_to(data.collate_fn([mols[i]]), "cuda:0") for i in {p[0] for p in pick}}

    def run(i, kind, index):
        for layer in model.pretrain.layers:
            setattr(layer, ATTRS[kind], index)
        try:
            b = batches[i]
            return model(b.like(b))
        finally:
            for layer in model.pretrain.layers:
                setattr(layer, ATTRS[kind], None)
    with torch.no_grad():
        for p in pick[:10]:
            run(*p)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for p in pick:
            run(*p)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(pick), len(pick), len(reps)


def what_it_buys(model, mols, name, args):
    store = FlatMolStore.from_records(mols).to("cuda:0")
    attr.leave_one_out(model, store)              # warm-up: library GEMM selection, allocator
    torch.cuda.synchronize()
    secs = []
    for _ in range(3):
        t0 = time.perf_counter()
        res = attr.leave_one_out(model, store)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    n_rep = sum(int(res.tables[k]["offsets"][-1]) for k in res.kinds)
    per, n_s, n_all = scalar_path(model, mols, args.sample)
    assert n_all == n_rep
    batched = statistics.median(secs)
    scalar = per * (n_rep + len(mols))            # one unmasked forward per molecule as well
    print(f"2. {name}: {len(mols)} molecules, {n_rep} masked replicas")
    print(f"   leave_one_out (engine, batched): {batched * 1e3:.1f} ms (median of 3, host and device, collate included) = {len(mols) / batched:.0f} attributed molecules/s")
    print(f"   scalar layer attributes, per-level path, one molecule and one mask per forward: {per * 1e3:.3f} ms per forward on a sample of {n_s} "
          f"replicas; EXTRAPOLATED from that sample to {n_rep + len(mols)} forwards: {scalar:.2f} s = {len(mols) / scalar:.2f} attributed molecules/s")
    print(f"   ratio: {scalar / batched:.0f} x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--sample", type=int, default=200)
    args = ap.parse_args()
    if args.repeats < 5 or args.batches < 20 or args.sample < 200:
        ap.error("at least 5 repeats of 20 batches and a sample of 200 replicas")
    fragnet_amd.prefer_rocblas_for_dense_heads()
    torch.manual_seed(5)
    model = FragNetFineTune(n_classes=1, num_layer=4, drop_ratio=0.1, h1=128, h2=1024, h3=1024, h4=512, act="relu").to("cuda:0").eval()
    big = synth.synth_molecules(1024, seed=4200, profile="esol")
    mask_cost(model, FlatMolStore.from_records(big[:64]).to("cuda:0"), args)
    what_it_buys(model, synth.synth_molecules(6, seed=4100, profile="esol"), "six-molecule set", args)
    what_it_buys(model, big, "1024-molecule ESOL-profile store", args)


if __name__ == "__main__":
    main()
