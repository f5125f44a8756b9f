#!/usr/bin/env python3
"""Side benchmark of the factored pair path on one GPU: the SAME model on the SAME 256 (drug, second input, y) records, collated the
duplicated way (collate_fn_cdrp / collate_fn_dta: one molecule and one second row per pair) and the factored way
(collate_fn_*_factored: every distinct input once), in ONE process, interleaved A/B rounds, timed with device events.
    step    one training step (forward + fused MSE + backward, no optimiser: it is the same for both), num_layer = 4, drop_ratio = 0 so
            that both ways compute the same numbers, at 256 pairs over (U, C) = (256, 256), (32, 64) and (8, 16) distinct inputs, and at
            --tall pairs over (32, 64);
    grid    256 drugs x 1024 second inputs in eval mode: one grid batch (data.pair_grid_batch) against a loop of 1024 duplicated batches,
            each the 256 drugs against one second input (the cheapest duplicated form: the molecule tensors are collated once and shared).
Also reported: device launches of one step (torch.profiler; kernels, and memsets apart).
dev tool: python tools/pair_factored_bench.py [--rounds 10] [--steps 5] [--markdown profiles/pair_factored.md]     prints one JSON line last"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import fragnet_amd
from fragnet_amd import _lib, data, ops, synth
from fragnet_amd.cdrp import CDRPModel, FragNetFineTuneBase
from fragnet_amd.dta import DTAModel2
from fragnet_amd.plan import plan_for

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=256)
ap.add_argument("--tall", type=int, default=2048, help="pairs of the last step row: a batch tall enough for the device to be the bound")
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--steps", type=int, default=5, help="steps per timed window")
ap.add_argument("--grid", type=int, nargs=2, default=[256, 1024], metavar=("U", "C"))
ap.add_argument("--markdown", default=None, help="also write the table to this file")
args = ap.parse_args()
assert torch.cuda.is_available(), "pair_factored_bench needs a GPU: a timing taken anywhere else says nothing"
dev = torch.device("cuda:0")
fragnet_amd.prefer_rocblas_for_dense_heads()
M, GD = args.pairs, 903
SHAPES = [(M, M, M), (M, 32, 64), (M, 8, 16), (args.tall, 32, 64)]      # (pairs, distinct drugs, distinct second inputs)
CTOR = dict(n_classes=1, num_layer=4, drop_ratio=0.0, h1=128, h2=1024, h3=1024, h4=512, act="relu")
COLLATE = {"cdrp": (data.collate_fn_cdrp, data.collate_fn_cdrp_factored, "gene_expr"),
           "dta": (data.collate_fn_dta, data.collate_fn_dta_factored, "protein")}
unit = ops.unit_grad(dev)


def model_of(kind):
    torch.manual_seed(0)
    base = FragNetFineTuneBase(**CTOR)
    return (CDRPModel(base, GD, dev) if kind == "cdrp" else DTAModel2(base)).to(dev).train()


def zero(m):
    for p in m.parameters():
        p.grad = None


def step(m, b):
    zero(m)
    _, loss = m(b, loss=(_lib.LOSS_MSE, b["y"], None))
    loss.backward(gradient=unit)
    return loss


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def ab(fa, fb, rounds, steps):
    for _ in range(3):
        window(fa, 2), window(fb, 2)
    ta, tb = [], []
    for _ in range(rounds):                # interleaved: A, B, A, B, ...
        ta.append(window(fa, steps))
        tb.append(window(fb, steps))
    return ta, tb


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        evs = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
        names = [e.name.lower() for e in evs]
        sets = sum("memset" in n for n in names)
        busy = sum(e.time_range.elapsed_us() for e in evs) / 1000.0          # ms the device spent inside kernels and memsets
        return len([n for n in names if "memcpy" not in n and "memset" not in n]), sets, busy
    except Exception as exc:               # the count is not measured then; the timings stand
        print(f"launch count not measured: {exc}", file=sys.stderr)
        return None, None, float("nan")


rows, res = [], {"what": "factored against duplicated pair batches, one MI355X", "pairs": M, "num_layer": 4, "rounds": args.rounds,
                 "steps_per_window": args.steps, "step": [], "grid": []}
for kind in ("cdrp", "dta"):
    dup_fn, fac_fn, key = COLLATE[kind]
    model = model_of(kind)
    for P, U, C in SHAPES:
        recs = synth.pair_records(P, U, C, kind, 700 + U)
        dup, fac = data.batch_to(dup_fn(recs), dev), data.batch_to(fac_fn(recs), dev)
        ld, lf = step(model, dup), step(model, fac)
        torch.cuda.synchronize()
        td, tf = ab(lambda: step(model, dup), lambda: step(model, fac), args.rounds, args.steps)
        (kd, sd, bd), (kf, sf, bf) = launches(lambda: step(model, dup)), launches(lambda: step(model, fac))
        r = dict(model=kind, pairs=P, U=U, C=C, dup_busy_ms=bd, fac_busy_ms=bf, dup_ms=statistics.median(td), dup_min_ms=min(td), fac_ms=statistics.median(tf), fac_min_ms=min(tf),
                 dup_launches=kd, fac_launches=kf, dup_memsets=sd, fac_memsets=sf, loss_abs_diff=abs(float(ld.detach()) - float(lf.detach())))
        r["fac_over_dup"] = r["fac_ms"] / r["dup_ms"]
        res["step"].append(r)
        rows.append(f"| {kind} step, {P} pairs | {U} x {C} | {r['dup_ms']:.3f} | {r['fac_ms']:.3f} | {r['fac_over_dup']:.2f} | {bd:.3f} | {bf:.3f} | {kd} (+{sd}) | {kf} (+{sf}) |")
    # the grid: every drug against every second input
    GU, GC = args.grid
    recs = synth.pair_records(max(GU, GC), GU, GC, kind, 800)
    fb = fac_fn(recs)
    first = [fb["pair_drug"].tolist().index(u) for u in range(GU)]
    drugs = [recs[i] for i in first]
    grid = data.batch_to(data.pair_grid_batch(drugs, fb[key], kind), dev)
    second = fb[key].to(dev)
    mols = data.batch_to(dup_fn(drugs), dev)          # the GU molecules once; their own second rows are replaced below
    plan_for(mols)                                    # ... and their graph plan: the loop's batches share both
    model.eval()

    def run_grid():
        with torch.no_grad():
            return model(grid)

    def run_loop():
        cols = []
        with torch.no_grad():
            for c in range(GC):
                b = mols.like(dict(mols))
                b[key] = second[c:c + 1].expand(GU, -1).contiguous()
                cols.append(model(b))
        return torch.cat(cols, 1)

    g1, g2 = run_grid(), run_loop()
    torch.cuda.synchronize()
    gdiff = float((g1 - g2).abs().max())
    tg, tl = ab(run_grid, run_loop, max(2, args.rounds // 4), 1)
    r = dict(model=kind, U=GU, C=GC, loop_ms=statistics.median(tl), grid_ms=statistics.median(tg), max_abs_diff=gdiff)
    r["grid_over_loop"] = r["grid_ms"] / r["loop_ms"]
    res["grid"].append(r)
    rows.append(f"| {kind} grid | {GU} x {GC} | {r['loop_ms']:.3f} | {r['grid_ms']:.3f} | {r['grid_over_loop']:.4f} | - | - | loop of {GC} batches | 1 batch |")

table = "\n".join(["| what | distinct drugs x second inputs | duplicated ms | factored ms | factored / duplicated | device busy ms, duplicated | device busy ms, factored | launches duplicated (+memsets) | launches factored (+memsets) |",
                   "|---|---|---|---|---|---|---|---|---|"] + rows)
print(table)
if args.markdown:
    with open(args.markdown, "w") as f:
        f.write("# Factored pair batches against duplicated ones\n\n"
                f"`tools/pair_factored_bench.py --rounds {args.rounds} --steps {args.steps}` on one MI355X: {M} pairs per training step "
                "(forward + fused MSE + backward, num_layer 4, drop_ratio 0), the same model and records both ways, interleaved in one "
                "process, medians of device-event windows.  Device busy: the sum of the kernels' durations in one profiled step (a run of its own, "
                "after the timed windows); where it is far below the step time the step is bound by the host enqueueing its launches.  The grid rows are an eval-mode screen, every drug against every second input.\n\n"
                + table + "\n\nRaw numbers:\n\n```json\n" + json.dumps(res, indent=1) + "\n```\n")
print(json.dumps(res))
