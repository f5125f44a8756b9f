"""Bit fingerprints of the prediction head's host code (ops.mlp_head and the loss nodes beside it): one line per case, the case name
and a SHA-256 over the outputs, the input gradient, every parameter gradient, the loss where there is one and the final Philox
offset.  Public API only, so the same file runs on two commits; diff the outputs: a change of the head's HOST code (which launches
it enqueues, with which arguments, in which order) that is meant to leave the arithmetic alone must leave every line alone.

    python tools/head_bits.py > bits.txt

Cases: FTHead1-5 x every activation kind the head takes x rows 1 / 37 / 64 and 80 with 64 live x p 0 / 0.1 x 1 / 12 classes, each
without a loss, with the fused MSE and with the fused BCE (seeded with ops.unit_grad and with a fresh 2.0); the tall route (library
GEMMs) on the shapes of tests/test_head_ops.py; PretrainTask's towers through ops.mlp_head; the three masked losses."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from fragnet_amd import _lib, data, ops, synth
from fragnet_amd import model as M
from fragnet_amd.train import pretrain_loss

DEV = "cuda:0"
KINDS = ["relu", "silu", "gelu", "celu", "selu", "relu6", "leakyrelu", "prelu"]
ROWS = [(1, None), (37, None), (64, None), (80, 64)]


def digest(items):
    h = hashlib.sha256()
    for name, t in items:
        h.update(name.encode())
        if t is None:
            h.update(b"<none>")
            continue
        a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        h.update(str(a.shape).encode() + str(a.dtype).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def report(name, items):
    torch.cuda.synchronize()
    print(f"{name:58s} {digest(items)}", flush=True)


def grads_of(params):
    items = [(f"p{i}", q.grad) for i, q in enumerate(params)]
    for q in params:
        q.grad = None
    return items


def make_head(name, kind, n_classes):
    torch.manual_seed(7)
    if name == "FTHead1":
        return M.FTHead1(n_classes=n_classes)
    if name == "FTHead2":
        return M.FTHead2(n_classes=n_classes)
    if name == "FTHead4":
        return M.FTHead4(n_classes=n_classes, act=kind)
    return getattr(M, name)(n_classes=n_classes, act=kind)


def head_case(name, head, rows, live, p, loss, seed_kind):
    """one forward + backward of a head module: ``loss`` None (gradient of sum(out * t)), "mse" or "bce" (the head armed with the
    targets, the loss seeded with the persistent unit gradient or a fresh 2.0)"""
    head.dropout.p = p
    head.rng = ops.PhiloxStream(seed=11)
    head.live_rows = live
    g = torch.Generator().manual_seed(rows * 7 + 1)
    n_classes = [q for q in head.parameters() if q.dim() == 2][-1].shape[0]
    x = torch.randn(rows, 256, generator=g).to(DEV).requires_grad_(True)
    t = torch.randn(rows, n_classes, generator=g).to(DEV)
    params = list(head.parameters())
    items = []
    if loss is None:
        out = head(x)
        (out * t).sum().backward()
    else:
        y = t if loss == "mse" else torch.where(t.abs() < 0.25, -torch.ones_like(t), (t > 0).float())       # -1: a missing label
        w = torch.zeros(rows, device=DEV)
        w[:rows if live is None else live] = 1.0
        head.loss_spec = (_lib.LOSS_MSE if loss == "mse" else _lib.LOSS_BCE, y, w)
        try:
            out = head(x)
        finally:
            head.loss_spec = None
        fused = getattr(out, "_fragnet_loss", None)
        val = fused[0] if fused is not None else (ops.masked_mse if loss == "mse" else ops.masked_bce)(out, y, w)
        val.backward(gradient=ops.unit_grad(DEV) if seed_kind == "unit" else torch.tensor(2.0, device=DEV))
        items.append(("loss", val))
    items += [("out", out), ("gx", x.grad)] + grads_of(params) + [("offset", np.int64(head.rng.offset))]
    report(name, items)


def linears(dims, seed=3):
    torch.manual_seed(seed)
    return [torch.nn.Linear(dims[i], dims[i + 1]).to(DEV) for i in range(len(dims) - 1)]


def mlp_case(name, shape, dims, p, live=None):
    lins = linears(dims)
    g = torch.Generator().manual_seed(shape[0])
    x = torch.randn(shape, generator=g).to(DEV).requires_grad_(True)
    t = torch.randn(shape[0], dims[-1], generator=g).to(DEV)
    rng = ops.PhiloxStream(seed=11)
    out = ops.mlp_head(x, lins, p, True, rng, live)
    (out * t).sum().backward()
    report(name, [("out", out), ("gx", x.grad)] + grads_of([q for lin in lins for q in lin.parameters()]) + [("offset", np.int64(rng.offset))])


def tall_cases():
    for p in (0.25, 0.0):
        mlp_case(f"tall_odd_input_small_last_p{p}", (5, 6), (6, 8, 4, 3), p)
        mlp_case(f"tall_wide_last_p{p}", (5, 6), (6, 8, 20), p)
        mlp_case(f"tall_padding_rows_p{p}", (9, 6), (6, 8, 4, 3), p, live=5)
    for p in (0.1, 0.0):
        mlp_case(f"tall_many_rows_p{p}", (4100, 8), (8, 8, 1), p)
    before = ops.DENSE_HEAD
    try:
        for flag in (True, False):
            ops.DENSE_HEAD = flag
            mlp_case(f"single_linear_dense_head_{int(flag)}", (5, 8), (8, 3), 0.25, live=3)
        mlp_case("single_linear_library", (5, 6), (6, 3), 0.25, live=3)
        ops.DENSE_HEAD = False
        head = make_head("FTHead3", "relu", 1).to(DEV).train()
        head_case("tall_FTHead3_dense_head_0", head, 64, None, 0.1, None, None)
    finally:
        ops.DENSE_HEAD = before


def pretrain_case():
    b = data.batch_to(data.collate_fn_pt(synth.synth_molecules(24, seed=8, profile="esol", pretrain_targets=True)), DEV)
    torch.manual_seed(2)
    net = M.FragNetPreTrain(num_layer=2, drop_ratio=0.0, edge_features=17).to(DEV).train()
    net.head.fused_towers = False
    outs = net(dict(b))
    pretrain_loss(outs, b).backward()
    report("pretrain_task_generic_towers", [(f"out{i}", o) for i, o in enumerate(outs)] + [(n, q.grad) for n, q in net.named_parameters()])


def loss_cases():
    g = torch.Generator().manual_seed(70)
    y = torch.randn(70, 3, generator=g).to(DEV)
    yb = torch.where(y.abs() < 0.25, -torch.ones_like(y), (y > 0).float())
    w = (torch.rand(70, generator=g) > 0.1).float().to(DEV)
    for seed_kind in ("unit", "fresh"):
        seed = lambda: ops.unit_grad(DEV) if seed_kind == "unit" else torch.tensor(2.0, device=DEV)     # noqa: E731
        for name, fn, tgt in (("masked_mse", ops.masked_mse, y), ("masked_bce", ops.masked_bce, yb)):
            out = torch.randn(70, 3, generator=g).to(DEV).requires_grad_(True)
            loss = fn(out, tgt, w)
            loss.backward(gradient=seed())
            report(f"{name}_{seed_kind}", [("loss", loss), ("g", out.grad)])
        outs = [torch.randn(70, 3, generator=g).to(DEV).requires_grad_(True) for _ in range(2)]
        scale = torch.tensor([0.9, 1.3], device=DEV)
        loss = ops.masked_mse_multi([(2.0, 0), (1.0, -1)], scale, outs[0], y, w, outs[1], y, w)
        loss.backward(gradient=seed())
        report(f"masked_mse_multi_{seed_kind}", [("loss", loss)] + [(f"g{i}", o.grad) for i, o in enumerate(outs)])


def main():
    for name in ("FTHead1", "FTHead2", "FTHead3", "FTHead4", "FTHead5"):
        for kind in (KINDS if name in ("FTHead3", "FTHead4", "FTHead5") else ["relu"]):
            for n_classes in (1, 12):
                head = make_head(name, kind, n_classes).to(DEV).train()
                for rows, live in ROWS:
                    for p in (0.0, 0.1):
                        tag = f"{name}_{kind}_c{n_classes}_r{rows}" + ("" if live is None else f"live{live}") + f"_p{p}"
                        head_case(tag, head, rows, live, p, None, None)
                        for loss in ("mse", "bce"):
                            for seed_kind in ("unit", "fresh"):
                                head_case(f"{tag}_{loss}_{seed_kind}", head, rows, live, p, loss, seed_kind)
    tall_cases()
    pretrain_case()
    loss_cases()


if __name__ == "__main__":
    main()
