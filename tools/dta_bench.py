#!/usr/bin/env python3
"""Side benchmark of the drug-target-affinity (DTA) protein tower and training step on one GPU, at B = 64 and B = 512 (L = 1000 tokens,
Embedding(26, 300), Conv1d(1000, 32, 8), Linear(9376, 300)), in ONE process, interleaved A/B windows, timed with device events.
    eager      the tower as torch writes it: F.embedding -> F.conv1d -> F.linear and autograd (library kernels) -- the baseline;
    hip        ops.protein_tower (csrc/dta.hip: the convolution in its histogram form; fn_dense_*_f32 for the Linear).
Both towers share their parameters' values; a measurement is forward + backward (no optimiser: it is the same for both).  Also timed:
the four parts of the HIP tower one by one (convolution forward / backward through the C calls, the dense layer forward / backward), and
the full DTAModel2 training step (encoder engine + tower + pair head, fused loss, num_layer = 4).
dev tool: python tools/dta_bench.py [--rounds 20] [--steps 10] [--batches 64 512]      prints one JSON line last"""
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
from fragnet_amd.dta import DTAModel2, FragNetFineTuneBase
from fragnet_amd.plan import _stream_ptr

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, nargs="+", default=[64, 512])
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--steps", type=int, default=10, help="steps per timed window")
args = ap.parse_args()
assert torch.cuda.is_available(), "dta_bench needs a GPU: a timing taken anywhere else says nothing"
dev = torch.device("cuda:0")
fragnet_amd.prefer_rocblas_for_dense_heads()
unit = ops.unit_grad(dev)
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


def one(fn, m=None):
    for _ in range(5):
        window(fn, m, 2)
    return [window(fn, m, args.steps) for _ in range(args.rounds)]


def med_min(ts):
    return {"median": statistics.median(ts), "min": min(ts)}


def bench(B):
    recs = synth.attach_protein(synth.synth_molecules(B, seed=900, profile="esol"), 901)
    batch = data.batch_to(data.collate_fn_dta(recs), dev)
    torch.manual_seed(0)
    model = DTAModel2(FragNetFineTuneBase(n_classes=1, num_layer=4, drop_ratio=0.1, h1=128, h2=1024, h3=1024, h4=512, act="relu")).to(dev).train()
    tok = batch["protein"]
    hip = torch.nn.ModuleList([model.embedding_xt, model.conv_xt_1, model.fc1_xt])
    eager = copy.deepcopy(hip)
    g_xt = torch.randn(B, 300, device=dev)

    def tower_hip():
        ops.protein_tower(tok, *hip).backward(g_xt)

    def tower_eager():
        F.linear(F.conv1d(F.embedding(tok, eager[0].weight), eager[1].weight, eager[1].bias).flatten(1), eager[2].weight, eager[2].bias).backward(g_xt)

    # same numbers first: faster and different is not faster
    zero(hip), zero(eager)
    tower_hip(), tower_eager()
    torch.cuda.synchronize()
    gdiff = {n: float((p.grad - q.grad).abs().max() / q.grad.abs().max()) for (n, p), q in zip(hip.named_parameters(), eager.parameters())}
    t_hip, t_eager = ab(tower_hip, hip, tower_eager, eager)

    # the parts of the HIP tower, one by one
    E, Wc, bc, Wf, bf = (q.detach() for q in (hip[0].weight, hip[1].weight, hip[1].bias, hip[2].weight, hip[2].bias))
    L, (V, D) = tok.shape[1], E.shape
    K, N = Wf.shape[1], Wf.shape[0]
    A = torch.empty((B, V, 256), device=dev)
    conv, g_conv = torch.empty((B, K), device=dev), torch.randn((B, K), device=dev)
    xt = torch.empty((B, N), device=dev)
    dE, dWc, dbc, dWf, dbf = (torch.empty_like(q) for q in (E, Wc, bc, Wf, bf))
    ws = torch.empty(_lib.load().fn_dta_conv_bwd_ws(B, L, D, V), device=dev)
    gx = torch.empty_like(conv)
    parts = {
        "conv_fwd": lambda: _lib.call("fn_dta_conv_fwd_f32", tok.data_ptr(), E.data_ptr(), Wc.data_ptr(), bc.data_ptr(), A.data_ptr(), conv.data_ptr(),
                                      B, L, D, V, 32, 8, st),
        "dense_fwd": lambda: _lib.call("fn_dense_fwd_f32", conv.data_ptr(), Wf.data_ptr(), bf.data_ptr(), xt.data_ptr(), B, K, N, None, st),
        "dense_bwd": lambda: _lib.call("fn_dense_bwd_f32", g_xt.data_ptr(), conv.data_ptr(), Wf.data_ptr(), gx.data_ptr(), 0.0, dWf.data_ptr(),
                                       dbf.data_ptr(), B, K, N, B, st),
        "conv_bwd": lambda: _lib.call("fn_dta_conv_bwd_f32", g_conv.data_ptr(), tok.data_ptr(), E.data_ptr(), A.data_ptr(), dWc.data_ptr(),
                                      dbc.data_ptr(), dE.data_ptr(), ws.data_ptr(), B, L, D, V, 32, 8, st),
    }
    split = {k: med_min(one(f)) for k, f in parts.items()}

    def step():
        _, loss = model(batch, loss=(_lib.LOSS_MSE, batch["y"], None))
        loss.backward(gradient=unit)

    return {"B": B, "tower_ms": {"hip": med_min(t_hip), "eager": med_min(t_eager),
                                 "ratio_hip_over_eager": statistics.median(t_hip) / statistics.median(t_eager)},
            "hip_tower_parts_ms": split, "train_step_ms": med_min(one(step, model)), "tower_grad_rel_diff_hip_vs_eager": gdiff}


res = {"what": "DTA protein tower (forward + backward) and DTAModel2 training step (forward + MSE + backward), one MI355X",
       "L": 1000, "V": 26, "D": 300, "num_layer": 4, "rounds": args.rounds, "steps_per_window": args.steps,
       "cases": [bench(B) for B in args.batches]}
print(json.dumps(res))
