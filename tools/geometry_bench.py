#!/usr/bin/env python3
"""Side benchmark of the geometry stage (csrc/geometry.hip) on one GPU, at the workload's batch of 512 ESOL-shape molecules, in ONE
process, interleaved windows, timed with device events, medians:
    collate full        FlatMolStore.collate(idx, pretrain=True) of a store that keeps all its tensors (the one-launch collate);
    collate geometry    the same batches from store.without_geometry(): positions ride along, then fn_bond_cos_f32 and
                        fn_pretrain_geometry_f32 fill edge_attr_bonds and the three targets;
    bond_cos, pretrain_geometry     the two launches alone on one batch.
Also: the largest difference between the two collates' derived tensors (the full store holds synth.geometry_from_positions' values),
and the store's bytes per molecule with and without the derived tensors.
dev tool: python tools/geometry_bench.py [--rounds 20] [--steps 10] [--batch 512] [--mols 4096]      prints one JSON line last"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fragnet_amd import ops, synth
from fragnet_amd.dataset import BatchSampler, FlatMolStore

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--mols", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--steps", type=int, default=10, help="calls per timed window")
args = ap.parse_args()
assert torch.cuda.is_available(), "geometry_bench needs a GPU: a timing taken anywhere else says nothing"
dev = torch.device("cuda:0")


def store_bytes(store):
    tensors = list(store.t.values()) + list(store.off.values()) + [store.y]
    return sum(t.numel() * t.element_size() for t in tensors) / len(store)


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def interleaved(fns):
    for _ in range(5):                         # every shape of the timed windows, every variant
        for fn in fns.values():
            window(fn, 2)
    ts = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            ts[k].append(window(fn, args.steps))
    return {k: {"median_us": statistics.median(v) * 1e3, "min_us": min(v) * 1e3} for k, v in ts.items()}


cpu = FlatMolStore.from_records(synth.attach_positions(
    synth.synth_molecules(args.mols, seed=900, profile="esol", pretrain_targets=True), seed=901))
full = cpu.to(dev)
lean = full.without_geometry()
both = lean.without_bond_graph_index()
batches = [b.clone() for b in BatchSampler(len(cpu), args.batch, shuffle=True, drop_last=True, seed=1)][: args.steps]

# same numbers first
want, got = full.collate(batches[0], pretrain=True), lean.collate(batches[0], pretrain=True)
assert getattr(got, "_keep", None) is not None, "the geometry store left the one-launch collate"
err = {k: float(((got[k] - want[k]).abs() / (1 + want[k].abs())).max()) for k in ("bnd_lngth", "bnd_angl", "dh_angl")}
err["edge_attr_bonds_abs"] = float((got["edge_attr_bonds"] - want["edge_attr_bonds"]).abs().max())
m = full.max_per_mol()
pos, ei, eib, bv = got["positions"], got["edge_index"], got["edge_index_bonds_graph"], got["batch"]
times = interleaved({
    "collate_full": lambda i: full.collate(batches[i % len(batches)], pretrain=True),
    "collate_geometry": lambda i: lean.collate(batches[i % len(batches)], pretrain=True),
    "bond_cos": lambda i: ops.bond_cos(pos, ei, eib),
    "pretrain_geometry": lambda i: ops.pretrain_geometry(pos, ei, bv, args.batch, max_per_mol=(m["atom"], m["edge"])),
})
print(json.dumps({"what": "geometry stage next to the collate, one MI355X, device events, median of windows", "B": args.batch,
                  "atoms": int(pos.shape[0]), "bonds": int(ei.shape[1]), "bond_graph_edges": int(eib.shape[1]), "rounds": args.rounds,
                  "calls_per_window": args.steps, "times": times, "max_difference_to_host_values": err,
                  "store_bytes_per_molecule": {"full": store_bytes(full), "without_geometry": store_bytes(lean),
                                               "without_geometry_and_bond_graph_index": store_bytes(both)}}))
