#!/usr/bin/env python3
"""Generates tests/golden/input_grad_b6.npz, input_grad_lite_b6.npz and ig_b6.npz with the REFERENCE's own Python on the CPU: the
gradients of its gat2.py / gat2_lite.py FragNetFineTune (eval(), FTHead3) with respect to the three node-feature tables of a batch,
and integrated gradients of the gat2 model from a zero baseline.  Same loading of the reference as make_golden.py (whose stand-ins it
imports).  Run here only:
    python tests/golden/make_golden_inputgrad.py

The batch is tests/inputgrad_common.molecules() through the reference's collate_fn; the model is inputgrad_common.CTOR under
inputgrad_common.SEED, unscaled.  The files hold numbers only:
    cfg                      json: ctor, seeds
    pkeys, psums             state-dict keys and (sum, abs-sum) checksums
    n_atoms, n_bonds, n_fbonds   rows per molecule in the three tables
    input_grad*:  logits [6, 1]; grad/<table> fp32 and grad64/<table> (the same from a .double() copy of the model) of out[:, 0].sum()
                  (gat2_lite: no node_features_fbonds entry -- it never reads the table)
    ig_b6:        steps (the smallest of 16, 32, 64 whose |gap| <= 2 % of |pred - pred_baseline| on every molecule), gap_by_steps,
                  pred, pred_baseline, attr_other, gap [6]; m<i>/atom, m<i>/bond, m<i>/fbond per-entry attributions
"""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import install_stubs, param_checksums, quiet, zero_dead_bias  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import inputgrad_common as ic  # noqa: E402


def forward(model, batch, tables):
    b = dict(batch)
    for k, t in zip(ic.TABLE_KEYS, tables):
        b[k] = t
    with quiet():
        return model(b)


def gradients(model, batch, dtype=torch.float32):
    """(logits, [d out[:, 0].sum() / d table or None]) with the floating tensors of the batch in ``dtype``."""
    b = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in batch.items()}
    leaves = [b[k].clone().requires_grad_(True) for k in ic.TABLE_KEYS]
    out = forward(model, b, leaves)
    grads = torch.autograd.grad(out[:, 0].sum(), leaves, allow_unused=True)
    return out.detach(), grads


def grad_case(name, module, batch, counts):
    with quiet():
        model = ic.build(module, dict(ic.FEATURES, **ic.CTOR))
    zero_dead_bias(model)
    out, g32 = gradients(model, batch)
    _, g64 = gradients(copy.deepcopy(model).double(), batch, torch.float64)
    store = {"cfg": np.asarray(json.dumps({"ctor": dict(ic.FEATURES, **ic.CTOR), "seed": ic.SEED, "mol_seed": ic.MOL_SEED})),
             "logits": out.numpy().astype(np.float32)}
    store["pkeys"], store["psums"] = (lambda ks: (np.asarray(json.dumps(ks[0])), ks[1]))(param_checksums(model))
    for k, v in counts.items():
        store[k] = v
    for key, a, d in zip(ic.TABLE_KEYS, g32, g64):
        if a is None:
            print(f"  {name}: {key} does not reach the output (no gradient)")
            continue
        store[f"grad/{key}"], store[f"grad64/{key}"] = a.numpy().astype(np.float32), d.numpy()
        dev = float((a.double() - d).abs().max() / d.abs().max())
        print(f"  {name}: {key} max|grad| = {float(d.abs().max()):.3e}, fp32 vs float64 = {dev:.2e} of the maximum")
        assert dev < 2.5e-5
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **store)
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB")
    return model


def ig_case(model, batch, counts):
    xs = [batch[k].float() for k in ic.TABLE_KEYS]
    zeros = [torch.zeros_like(x) for x in xs]
    with torch.no_grad():
        pred = forward(model, batch, xs)[:, 0].numpy().astype(np.float32)
        pred0 = forward(model, batch, zeros)[:, 0].numpy().astype(np.float32)
    chosen, by_steps = None, {}
    for steps in ic.STEP_CHOICES:
        rows = [np.zeros(x.shape[0], dtype=np.float32) for x in xs]
        for j in range(steps):                                     # ascending j, float32 throughout
            alpha = np.float32((j + 0.5) / steps)
            leaves = [(alpha * x).requires_grad_(True) for x in xs]
            grads = torch.autograd.grad(forward(model, batch, leaves)[:, 0].sum(), leaves)
            for r, g, x in zip(rows, grads, xs):
                r += (g * x).sum(1).numpy()
        rows = [r / np.float32(steps) for r in rows]
        per_mol = ic.entry_sums(*rows, counts["n_atoms"], counts["n_bonds"], counts["n_fbonds"])
        total = np.asarray([float(a.astype(np.float64).sum() + b.astype(np.float64).sum() + f.astype(np.float64).sum() + o) for a, b, f, o in per_mol])
        gap = (pred.astype(np.float64) - pred0.astype(np.float64) - total).astype(np.float32)
        frac = np.abs(gap) / np.abs(pred.astype(np.float64) - pred0)
        by_steps[steps] = float(frac.max())
        print(f"  ig: {steps} steps, worst |gap| / |pred - pred_baseline| = {frac.max():.3e}")
        if chosen is None and (frac <= ic.GAP_FRACTION).all():
            chosen = (steps, per_mol, gap)
    assert chosen is not None, "no step count of 16, 32, 64 closes the gap to 2 % on every molecule: choose another seed"
    steps, per_mol, gap = chosen
    assert (np.abs(gap) <= ic.GAP_FRACTION * np.abs(pred.astype(np.float64) - pred0)).all()
    store = {"steps": np.asarray(steps), "gap_by_steps": np.asarray(json.dumps(by_steps)), "pred": pred, "pred_baseline": pred0,
             "attr_other": np.asarray([o for *_, o in per_mol], dtype=np.float32), "gap": gap}
    for k, v in counts.items():
        store[k] = v
    for i, (a, b, f, _) in enumerate(per_mol):
        store[f"m{i}/atom"], store[f"m{i}/bond"], store[f"m{i}/fbond"] = a, b, f
    path = os.path.join(HERE, "ig_b6.npz")
    np.savez_compressed(path, **store)
    print(f"ig_b6: {steps} steps, {os.path.getsize(path) / 1024:.1f} KiB")


def main():
    install_stubs()
    with quiet():
        from fragnet.model.gat import gat2 as ref_gat2
        from fragnet.model.gat import gat2_lite as ref_lite
        from fragnet.dataset import data as ref_data
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    mols = ic.molecules()
    batch = ref_data.collate_fn(mols)
    counts = {"n_atoms": np.asarray([m.x_atoms.shape[0] for m in mols], dtype=np.int64),
              "n_bonds": np.asarray([m.node_features_bonds.shape[0] for m in mols], dtype=np.int64),
              "n_fbonds": np.asarray([m.node_feautures_fbondg.shape[0] for m in mols], dtype=np.int64)}
    assert (counts["n_fbonds"] == 1).any(), "a molecule with one fragment (placeholder row) is wanted"
    deg = torch.bincount(batch["edge_index"][0], minlength=batch["x_atoms"].shape[0])
    assert bool((deg == 0).any()), "an atom without bonds is wanted"
    model = grad_case("input_grad_b6", ref_gat2, batch, counts)
    grad_case("input_grad_lite_b6", ref_lite, batch, counts)
    ig_case(model, batch, counts)


if __name__ == "__main__":
    main()
