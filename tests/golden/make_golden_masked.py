#!/usr/bin/env python3
"""Generates tests/golden/pt_masked2_b4.npz and pt_masked2_edge6.npz: the reference's FragNetPreTrainMasked2
(fragnet/model/gat/pretrain_heads.py:187-236) under the stand-ins of make_golden.py, in train() mode with drop_ratio = 0.

Run where the reference checkout exists (make_golden.py says where):
    python tests/golden/make_golden_masked.py

Per fixture, in save_case's layout:
    batch/<key>          the collate_fn_pt batch BEFORE the reference overwrites batch["x_atoms"]
    keep_atoms           uint8 [N], 1 = kept: recovered from which rows the reference zeroed (its random.sample under ``mask_seed``)
    out/*, gfull/.., ..  outputs, loss and gradients of the masked model
    out_unmasked/<name>  the four outputs of the reference's FragNetPreTrain with the same weights on the original batch

The generator asserts that masked and unmasked outputs differ by at least ten times the 1e-4 parity tolerance of
tests/test_gpu_parity.py -- what lets the parity test detect a port that ignores the mask -- and moves on to the next
``random.seed`` otherwise.  Only numbers go into the fixtures."""
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

PARITY_TOL = 1e-4
NAMES = ("bond_length", "bond_angle", "dihedral", "graph_rep")


def pretrain_targets(mols):
    """make_golden.py's pretrain targets of the collate fixture's molecules (main(), the loop over ``mols``)."""
    for m in mols:
        e, n = m.edge_index.shape[1], m.x_atoms.shape[0]
        g = torch.Generator().manual_seed(e * 1000 + n)
        m.bnd_lngth, m.bnd_angl, m.dh_angl = torch.rand(e, 1, generator=g), torch.rand(n, 1, generator=g), torch.rand(e, 1, generator=g)
    return mols


def reference_loss(outs, batch):
    """the reference's pretrain step, pretrain_utils.py:21-26 (the bond-length loss is overwritten)"""
    bl, ba, da, gr = outs
    mse = torch.nn.MSELoss()
    return mse(da, batch["dh_angl"]) + mse(ba, batch["bnd_angl"]) + mse(da, batch["dh_angl"]) + mse(gr.view(-1), batch["y"])


def masked_case(name, mols, ref_pt, ref_data, first_seed):
    cfg = dict(num_layer=4, drop_ratio=0.0, num_heads=4, emb_dim=128, atom_features=167, frag_features=167,
               edge_features=17, fedge_in=6, fbond_edge_in=6)
    original = ref_data.collate_fn_pt(mols)
    assert bool((original["x_atoms"] != 0).any(dim=1).all()), "an all-zero atom row: the zeroed rows could not be told from it"
    torch.manual_seed(1)
    with mg.quiet():
        plain = ref_pt.FragNetPreTrain(**cfg)
    mg.zero_dead_bias(plain)
    plain.train()
    with mg.quiet(), torch.no_grad():
        unmasked = plain({k: v.clone() for k, v in original.items()})
    for mask_seed in range(first_seed, first_seed + 64):
        torch.manual_seed(1)
        with mg.quiet():
            model = ref_pt.FragNetPreTrainMasked2(**cfg)
        mg.zero_dead_bias(model)
        assert list(model.state_dict()) == list(plain.state_dict())
        assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), plain.state_dict().values()))
        model.train()
        batch = {k: v.clone() for k, v in original.items()}
        trace, hooks = mg.run_layer_trace(model, batch)
        random.seed(mask_seed)
        with mg.quiet():
            outs = model(batch)
        for h in hooks:
            h.remove()
        diff = max(float((a.detach() - b).abs().max()) for a, b in zip(outs, unmasked))
        if diff >= 10 * PARITY_TOL:
            break
    else:
        raise SystemExit(f"{name}: no random.seed in [{first_seed}, {first_seed + 64}) separates masked from unmasked outputs")
    # the reference overwrote batch["x_atoms"]: a kept row is untouched, a masked row is zero
    after, before = batch["x_atoms"], original["x_atoms"]
    zeroed = (after == 0).all(dim=1)
    assert bool(((after == before).all(dim=1) | zeroed).all())
    keep = (~zeroed).to(torch.uint8)
    n = before.shape[0]
    assert int(keep.sum()) == int(n * 0.85), (int(keep.sum()), n)
    loss = reference_loss(outs, batch)
    loss.backward()
    mg.save_case(name, {"kind": "pretrain_masked2", "ctor": cfg, "seed": 1, "loss": "pretrain", "mask_seed": mask_seed,
                        "masked_vs_unmasked": diff}, original, model, dict(zip(NAMES, outs)), loss, trace)
    path = os.path.join(HERE, name + ".npz")
    store = dict(np.load(path))
    store["keep_atoms"] = keep.numpy()
    for nm, t in zip(NAMES, unmasked):
        store[f"out_unmasked/{nm}"] = t.numpy()
    np.savez_compressed(path, **store)
    print(f"{name}: N = {n}, kept {int(keep.sum())}, random.seed({mask_seed}), max |masked - unmasked| = {diff:.3e}, "
          f"{os.path.getsize(path) / 1024:.0f} KiB")


def main():
    mg.install_stubs()
    with mg.quiet():
        from fragnet.model.gat import pretrain_heads as ref_pt
        from fragnet.dataset import data as ref_data
    from fragnet_amd import synth
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    masked_case("pt_masked2_b4", synth.synth_molecules(4, seed=3000, profile="esol", pretrain_targets=True), ref_pt, ref_data, 7)
    masked_case("pt_masked2_edge6", pretrain_targets(mg.edge_case_molecules()), ref_pt, ref_data, 7)


if __name__ == "__main__":
    main()
