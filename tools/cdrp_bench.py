#!/usr/bin/env python3
"""Side benchmark of the cancer-drug-response (CDRP) training step on one GPU: B = 256, gene_dim = 903, num_layer = 4, two ways in ONE
process, interleaved A/B rounds, timed with device events.
    baseline   the cell-line tower and the pair head as stock nn.Linear / torch.cat modules (library GEMMs) on top of the encoder engine
               -- what the code before csrc/cdrp.hip could run;
    new        ops.cell_tower + ops.pair_head (csrc/cdrp.hip, fn_dense_*), the fused-loss call.
Both models share their initial parameters; the step is forward + loss + backward (no optimiser: it is the same for both).  Also timed:
the tower + pair-head part alone (forward + backward on a fixed drug encoding), and its device launch count (torch.profiler).
dev tool: python tools/cdrp_bench.py [--rounds 20] [--steps 10]      prints one JSON line last"""
import argparse
import copy
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import fragnet_amd
from fragnet_amd import _lib, data, ops, synth
from fragnet_amd.cdrp import CDRPModel, FragNetFineTuneBase

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--gene-dim", type=int, default=903)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--steps", type=int, default=10, help="steps per timed window")
args = ap.parse_args()
assert torch.cuda.is_available(), "cdrp_bench needs a GPU: a timing taken anywhere else says nothing"
dev = torch.device("cuda:0")
fragnet_amd.prefer_rocblas_for_dense_heads()
B, GD = args.batch, args.gene_dim
recs = synth.attach_gene_expr(synth.synth_molecules(B, seed=900, profile="esol"), GD, 901)
batch = data.batch_to(data.collate_fn_cdrp(recs), dev)
torch.manual_seed(0)
new = CDRPModel(FragNetFineTuneBase(n_classes=1, num_layer=4, drop_ratio=0.1, h1=128, h2=1024, h3=1024, h4=512, act="relu"), GD, dev).to(dev).train()
base = copy.deepcopy(new)
unit = ops.unit_grad(dev)


def step_new():
    _, loss = new(batch, loss=(_lib.LOSS_MSE, batch["y"], None))
    loss.backward(gradient=unit)
    return loss


def stock_tail(m, drug_enc, gene):
    v = gene.float()
    for lin in m.cell_model.predictor:
        v = F.relu(lin(v))
    return m.fc2(m.fc1(torch.cat((drug_enc, v), 1)))


def step_base():
    loss = F.mse_loss(stock_tail(base, base.drug_model(batch), batch["gene_expr"]).view(-1), batch["y"])
    loss.backward()
    return loss


drug_fixed = torch.randn(B, 256, device=dev)


def tail_new():
    d = drug_fixed.detach().requires_grad_(True)
    _, loss = ops.pair_head(d, new.cell_model(batch["gene_expr"]), new.fc1, new.fc2, loss=(_lib.LOSS_MSE, batch["y"], None))
    loss.backward(gradient=unit)


def tail_base():
    d = drug_fixed.detach().requires_grad_(True)
    F.mse_loss(stock_tail(base, d, batch["gene_expr"]).view(-1), batch["y"]).backward()


def zero(m):
    for p in m.parameters():
        p.grad = None


def window(fn, m, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
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


def launches(fn, m):
    try:
        from torch.profiler import ProfilerActivity, profile
        zero(m)
        fn()
        torch.cuda.synchronize()
        zero(m)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        return len(names)
    except Exception as exc:               # the count is not measured then; the timings stand
        print(f"launch count not measured: {exc}", file=sys.stderr)
        return None


# same numbers first: faster and different is not faster
lb, ln = step_base(), step_new()
torch.cuda.synchronize()
diff = abs(float(lb) - float(ln))
gdiff = max(float((p.grad - q.grad).abs().max()) for p, q in zip(base.parameters(), new.parameters()) if p.grad is not None)
step_b, step_n = ab(step_base, base, step_new, new)
tail_b, tail_n = ab(tail_base, base, tail_new, new)
res = {
    "what": "CDRP training step (forward + MSE + backward), one MI355X", "B": B, "gene_dim": GD, "num_layer": 4,
    "rounds": args.rounds, "steps_per_window": args.steps,
    "step_ms": {"baseline_median": statistics.median(step_b), "baseline_min": min(step_b), "new_median": statistics.median(step_n), "new_min": min(step_n)},
    "tower_pair_ms": {"baseline_median": statistics.median(tail_b), "baseline_min": min(tail_b), "new_median": statistics.median(tail_n), "new_min": min(tail_n)},
    "tower_pair_launches": {"baseline": launches(tail_base, base), "new": launches(tail_new, new)},
    "loss_abs_diff": diff, "grad_max_abs_diff": gdiff,
}
res["step_ratio_new_over_baseline"] = res["step_ms"]["new_median"] / res["step_ms"]["baseline_median"]
res["tower_pair_ratio_new_over_baseline"] = res["tower_pair_ms"]["new_median"] / res["tower_pair_ms"]["baseline_median"]
print(json.dumps(res))
