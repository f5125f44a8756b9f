#!/usr/bin/env python3
"""Cell-line attributions on one GPU: integrated gradients of the CDRP cell-line tower on the HIP kernels against stock torch.

    python tools/pair_attribution_bench.py [--repeats 7] [--cells 1000] [--steps 32] > profiles/pair_attr_bench.txt

Model: CDRPModel with the reference's tower (903 -> 1024 -> 256 -> 64 -> 256), default initialisation under a fixed seed; ``--cells``
cell lines of 903 genes drawn as collate_fn_cdrp leaves them (int64 of N(0, 2.5)), ``--steps`` midpoint nodes from the zero baseline.
  hip    pair_attribution.cell_line_attributions: per chunk of cells * steps <= 4096 rows the path forward, the four backward launches
         and fn_cdrp_gene_dx_f32; no [rows, 903] table in memory.
  stock  the same numbers from torch on the GPU: gene.float() replicas scaled by the nodes into one [cells * steps, 903] leaf, F.linear /
         relu, torch.autograd.grad, mean over a cell line's nodes, times the input -- all rows in ONE batch (library GEMMs like them tall).
Both arms return the [cells, 903] attributions and the scores as numpy arrays (the copy back is inside the timed region).  They are
checked first, against the stock arm run in float64: the scores (a continuous function) within 1e-4 + 1e-4 |ref|; the attributions
per cell line within 1e-4 max|ref| + 1e-4 |ref|.  Of cells * steps * 1600 pre-activations a few lie within float32 round-off of zero, and
a ReLU that falls on the other side at one node moves that cell line's whole row by 1 / steps of a gradient difference -- in either
float32 arm, whose first products add in different orders.  So the check counts the cell lines outside the bound for both arms, prints
both counts, and fails if the HIP arm's exceeds 10 % of the cell lines.  Then both arms run in this one process, alternating, each repeat
timed with device events; min / median / max of the repeats."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import fragnet_amd
from fragnet_amd import gradient_attribution as ga
from fragnet_amd import pair_attribution as pa

DEV = "cuda:0"
SMALL = dict(n_classes=1, num_layer=2, num_heads=4, drop_ratio=0.0, h1=32, h2=64, h3=64, h4=32, act="relu", fthead="FTHead3")


def spread(xs):
    return f"min {min(xs):.3f}  median {statistics.median(xs):.3f}  max {max(xs):.3f}"


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def stock(model, gene, steps, dtype=torch.float32):
    F = torch.nn.functional
    if dtype != torch.float32:
        import copy
        model = copy.deepcopy(model).to(dtype)
    v_s = pa.pair_vectors(model)[1].to(dtype)
    alpha = torch.from_numpy(ga.midpoint_alphas(steps)).to(gene.device).to(dtype)
    x = gene.to(dtype)
    leaf = (alpha.view(1, steps, 1) * x.unsqueeze(1)).reshape(-1, x.shape[1]).requires_grad_(True)
    h = leaf
    for lin in model.cell_model.predictor:
        h = F.relu(F.linear(h, lin.weight, lin.bias))
    (g,) = torch.autograd.grad((h @ v_s).sum(), leaf)
    attr = x * g.view(x.shape[0], steps, -1).mean(1)
    with torch.no_grad():
        h = x
        for lin in model.cell_model.predictor:
            h = F.relu(F.linear(h, lin.weight, lin.bias))
        score = h @ v_s
    return attr.cpu().numpy(), score.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cells", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=32)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    fragnet_amd.prefer_rocblas_for_dense_heads()
    from fragnet_amd.cdrp import CDRPModel, FragNetFineTuneBase
    torch.manual_seed(5)
    model = CDRPModel(FragNetFineTuneBase(**SMALL), 903, DEV).to(DEV).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    g = torch.Generator().manual_seed(6)
    gene = (torch.randn(args.cells, 903, generator=g) * 2.5).type(torch.long).to(DEV)

    hip = lambda: pa.cell_line_attributions(model, gene, method="ig", steps=args.steps)
    ref = lambda: stock(model, gene, args.steps)
    r, (a, s), (a64, s64) = hip(), ref(), stock(model, gene, args.steps, torch.float64)
    bound = 1e-4 * np.abs(a64).max() + 1e-4 * np.abs(a64)
    outside = {k: int((np.abs(v - a64) > bound).any(1).sum()) for k, v in (("hip", r.attr), ("stock", a))}
    print(f"cell-line integrated gradients, {args.cells} cell lines x 903 genes x {args.steps} nodes, zero baseline")
    for k, v, sc in (("hip", r.attr, r.score), ("stock", a, s)):
        print(f"agreement with float64, {k:5s}: scores max|diff| {np.abs(sc - s64).max():.3e}; attributions max|diff| {np.abs(v - a64).max():.3e} "
              f"(max|attr| {np.abs(a64).max():.3e}), {outside[k]} of {args.cells} cell lines outside 1e-4 max|ref| + 1e-4 |ref| (ReLU sides at path nodes)")
        assert (np.abs(sc - s64) <= 1e-4 + 1e-4 * np.abs(s64)).all(), f"{k}: the scores disagree with float64"
    assert outside["hip"] <= args.cells // 10, "the HIP arm disagrees with float64 on more than 10 % of the cell lines"
    for _ in range(2):
        hip(), ref()
    ms = {"hip": [], "stock": []}
    for _ in range(args.repeats):
        ms["hip"].append(timed(hip))
        ms["stock"].append(timed(ref))
    print(f"ms per call, {args.repeats} repeats, arms alternating, device events, copy back included")
    for k, v in ms.items():
        print(f"   {k:6s} {spread(v)}")
    a_, b_ = ms["hip"], ms["stock"]
    apart = not (min(a_) <= max(b_) and min(b_) <= max(a_))
    ratio = statistics.median(b_) / statistics.median(a_)
    if apart and ratio > 1:
        print(f"   the two arms' spreads do not overlap: hip is {ratio:.2f}x faster at the medians")
    elif apart:
        print(f"   the two arms' spreads do not overlap: hip is {1 / ratio:.2f}x SLOWER than stock torch at the medians")
    else:
        print(f"   the two arms' spreads overlap (ratio of the medians stock / hip = {ratio:.2f}): the HIP path does not beat stock torch by more than the spread")


if __name__ == "__main__":
    main()
