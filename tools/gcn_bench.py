#!/usr/bin/env python3
"""Side benchmark of the graph-convolution baseline (model_version gcn2) on one GPU, at B = 64 and B = 512 on the ESOL-shape synthetic
batch, in ONE process, interleaved A/B windows, timed with device events, medians.
    hip        fragnet_amd.gcn.FragNetFineTune: plan (fn_plan_build on the reduced task list), ops.linear128, ops.gcn_aggregate
               (csrc/gcn.hip), ops.segment_sum, ops.frag_mlp, ops.pool_cat, the dense-kernel head;
    stock      the same module tree (a deep copy: same parameter values) run as stock torch ops, which is what the reference's composition
               amounts to: F.linear, index_select, index_add_, F.dropout, torch.relu, library GEMMs in the head -- the baseline.  Like the
               HIP path it computes only what is read (no dead fragment half, no edge_embed).
A measurement is one training step without the optimiser (it is the same for both): forward, MSE, backward.  Also timed: the aggregate
launches alone (atom level forward / backward, fragment level forward) against their compulsory bytes -- one read of each gathered row,
one write of each output row, 4 B per value.
dev tool: python tools/gcn_bench.py [--rounds 20] [--steps 10] [--batches 64 512] [--md profiles/gcn_step.md]      prints one JSON line last"""
import argparse
import copy
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import fragnet_amd
from fragnet_amd import _lib, data, ops, synth
from fragnet_amd.gcn import FragNetFineTune
from fragnet_amd.plan import GCN_PLAN_KEY, _stream_ptr, gcn_plan_for

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, nargs="+", default=[64, 512])
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--steps", type=int, default=10, help="steps per timed window")
ap.add_argument("--md", default=None, help="also write the table as markdown to this file")
args = ap.parse_args()
assert torch.cuda.is_available(), "gcn_bench needs a GPU: a timing taken anywhere else says nothing"
dev = torch.device("cuda:0")
fragnet_amd.prefer_rocblas_for_dense_heads()
st = _stream_ptr(dev)


def zero(m):
    for p in m.parameters():
        p.grad = None


def window(fn, m, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        if m is not None:
            zero(m)
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def ab(fa, ma, fb, mb):
    for _ in range(5):                     # every shape of the timed windows, both ways
        window(fa, ma, 2), window(fb, mb, 2)
    ta, tb = [], []
    for _ in range(args.rounds):           # interleaved: A, B, A, B, ...
        ta.append(window(fa, ma, args.steps))
        tb.append(window(fb, mb, args.steps))
    return ta, tb


def one(fn):
    for _ in range(5):
        window(fn, None, 2)
    return [window(fn, None, args.steps) for _ in range(args.rounds)]


def med_min(ts):
    return {"median": statistics.median(ts), "min": min(ts)}


def stock_forward(model, batch):
    """gcn2.py's live part with stock torch ops (self loops, degree and norm are rebuilt per step, as the reference rebuilds them per layer)"""
    enc = model.pretrain
    p, train = enc.dropout.p, enc.training
    N, Fn, B = batch["x_atoms"].shape[0], batch["x_frags"].shape[0], batch["y"].shape[0]
    loop = torch.arange(N, device=dev)
    src, dst = torch.cat((batch["edge_index"][0], loop)), torch.cat((batch["edge_index"][1], loop))
    deg = torch.zeros(N, device=dev).index_add_(0, src, torch.ones(src.numel(), device=dev))
    dis = deg.pow(-0.5)
    dis[dis == float("inf")] = 0
    norm = (dis.index_select(0, src) * dis.index_select(0, dst)).view(-1, 1)
    x = F.dropout(batch["x_atoms"], p, train)
    for layer in enc.layers:
        h = F.linear(x, layer.atom_embed.weight, layer.atom_embed.bias)
        raw = torch.zeros(N, h.shape[1], device=dev).index_add_(0, dst, h.index_select(0, src) * norm)
        x = torch.relu(F.dropout(raw, p, train))
    last = enc.layers[-1]
    frags = torch.zeros(Fn, raw.shape[1], device=dev).index_add_(0, batch["atom_to_frag_ids"], raw)
    fsum = torch.zeros_like(frags).index_add_(0, batch["frag_index"][1], frags.index_select(0, batch["frag_index"][0]))
    xf = torch.relu(F.dropout(last.frag_mlp(fsum), p, train))
    pooled = torch.cat((torch.zeros(B, x.shape[1], device=dev).index_add_(0, batch["batch"], x),
                        torch.zeros(B, xf.shape[1], device=dev).index_add_(0, batch["frag_batch"], xf)), 1)
    return model.fthead(pooled)            # rng is None on the copy: the head's torch path (nn.Dropout, F.linear)


def bench(B):
    batch = data.batch_to(data.collate_fn(synth.synth_molecules(B, seed=900, profile="esol")), dev)
    torch.manual_seed(0)
    hip = FragNetFineTune(n_classes=1, atom_features=167, frag_features=167, edge_features=17, num_layer=4, drop_ratio=0.1, h1=128, h2=1024,
                          h3=1024, h4=512, act="relu", fthead="FTHead3").to(dev).train()
    stock = copy.deepcopy(hip)
    stock.fthead.rng = None

    def step_hip():
        batch.pop(GCN_PLAN_KEY, None)          # every step pays for its own graph plan
        F.mse_loss(hip(batch).view(-1), batch["y"]).backward()

    def step_stock():
        F.mse_loss(stock_forward(stock, batch).view(-1), batch["y"]).backward()

    # same numbers first (dropout off: the two paths draw different masks): faster and different is not faster
    hip.eval(), stock.eval()
    zero(hip), zero(stock)
    step_hip(), step_stock()
    torch.cuda.synchronize()
    gdiff = max(float((p.grad - q.grad).abs().max() / q.grad.abs().max().clamp_min(1e-30))
                for p, q in zip(hip.parameters(), stock.parameters()) if q.grad is not None)
    assert all((p.grad is None) == (q.grad is None) for p, q in zip(hip.parameters(), stock.parameters()))
    hip.train(), stock.train()
    t_hip, t_stock = ab(step_hip, hip, step_stock, stock)

    # the aggregate launches alone, against their compulsory bytes
    plan = gcn_plan_for(batch)
    parts = {}
    for name, lv, by_source, normalised in (("atom_fwd", plan.levels["atom"], 0, True), ("atom_bwd", plan.levels["atom"], 1, True),
                                            ("frag_fwd", plan.levels["frag"], 0, False), ("frag_bwd", plan.levels["frag"], 1, False)):
        x, out = torch.randn(lv.n, 128, device=dev), torch.empty(lv.n, 128, device=dev)
        coef = ops.gcn_coef(lv) if normalised else None
        ts = one(lambda: _lib.call("fn_gcn_aggregate_f32", x.data_ptr(), C.byref(lv.c), by_source, None if coef is None else coef.data_ptr(),
                                   out.data_ptr(), None, st))
        nbytes = (lv.m + lv.n) * 128 * 4
        parts[name] = dict(med_min(ts), rows=lv.n, items=lv.m, compulsory_MB=nbytes / 1e6, GBps_at_median=nbytes / statistics.median(ts) / 1e6)
    return {"B": B, "atoms": plan.levels["atom"].n, "fragments": plan.levels["frag"].n,
            "train_step_ms": {"hip": med_min(t_hip), "stock": med_min(t_stock), "ratio_hip_over_stock": statistics.median(t_hip) / statistics.median(t_stock)},
            "aggregate_ms": parts, "max_grad_rel_diff_hip_vs_stock": gdiff}


res = {"what": "gcn2 training step (plan + forward + MSE + backward, no optimiser) and the aggregate launches alone, one MI355X",
       "num_layer": 4, "drop_ratio": 0.1, "head": "FTHead3 128/1024/1024/512", "rounds": args.rounds, "steps_per_window": args.steps,
       "cases": [bench(B) for B in args.batches]}
if args.md:
    lines = ["# gcn2 training step and aggregate launches (tools/gcn_bench.py)", "",
             f"One MI355X, one process, interleaved windows of {args.steps} steps, {args.rounds} rounds, device events; medians (minimum in brackets).",
             "A step is plan + forward + MSE + backward without the optimiser; `stock` is the same module tree as F.linear / index_select / index_add_.", "",
             "| B | atoms | fragments | hip step ms | stock step ms | hip / stock | max rel. gradient difference (eval) |", "|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        t = c["train_step_ms"]
        lines.append(f"| {c['B']} | {c['atoms']} | {c['fragments']} | {t['hip']['median']:.3f} ({t['hip']['min']:.3f}) | "
                     f"{t['stock']['median']:.3f} ({t['stock']['min']:.3f}) | {t['ratio_hip_over_stock']:.2f} | {c['max_grad_rel_diff_hip_vs_stock']:.1e} |")
    lines += ["", "Aggregate launches alone (fn_gcn_aggregate_f32, raw output, no epilogue); compulsory bytes = (items + rows) x 512 B:", "",
              "| B | launch | rows | items | us median (min) | compulsory MB | GB/s at the median |", "|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        for name, q in c["aggregate_ms"].items():
            lines.append(f"| {c['B']} | {name} | {q['rows']} | {q['items']} | {q['median'] * 1e3:.1f} ({q['min'] * 1e3:.1f}) | {q['compulsory_MB']:.2f} | "
                         f"{q['GBps_at_median']:.0f} |")
    with open(args.md, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps(res))
