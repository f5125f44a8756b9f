#!/usr/bin/env python3
"""Generates the prediction-head activation fixtures tests/golden/ft_head*_b4.npz with the REFERENCE's own Python, the same way
and in the same layout as make_golden.py (whose stand-ins and writers it imports; see its docstring for how the reference is
loaded).  Run here only:
    python tests/golden/make_golden_heads.py

Cases (B = 4, drop 0, regression loss):
    ft_head3_celu_b4   FTHead3, act celu (FragNetFineTune's default)
    ft_head3_selu_b4   FTHead3, act selu (the reference's Lipophilicity config)
    ft_head4_prelu_b4  FTHead4, act prelu (one slope shared by the head)
    ft_head4_gelu_b4   FTHead4, act gelu
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import install_stubs, quiet, run_layer_trace, save_case, zero_dead_bias  # noqa: E402

CASES = {
    "ft_head3_celu_b4": (dict(fthead="FTHead3", act="celu", h1=64, h2=128, h3=128, h4=64), 4100, 11),
    "ft_head3_selu_b4": (dict(fthead="FTHead3", act="selu", h1=64, h2=128, h3=128, h4=64), 4200, 12),
    "ft_head4_prelu_b4": (dict(fthead="FTHead4", act="prelu", h1=64), 4300, 13),
    "ft_head4_gelu_b4": (dict(fthead="FTHead4", act="gelu", h1=64), 4400, 14),
}


def main():
    install_stubs()
    with quiet():
        from fragnet.model.gat import gat2 as ref_gat2
        from fragnet.dataset import data as ref_data
    from fragnet_amd import synth

    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    for name, (head, mol_seed, seed) in CASES.items():
        cfg = dict(n_classes=1, atom_features=167, frag_features=167, edge_features=17, num_layer=2, num_heads=4,
                   drop_ratio=0.0, emb_dim=128, **head)
        batch = ref_data.collate_fn(synth.synth_molecules(4, seed=mol_seed, profile="esol"))
        torch.manual_seed(seed)
        with quiet():
            model = ref_gat2.FragNetFineTune(**cfg)
        zero_dead_bias(model)
        model.train()
        trace, hooks = run_layer_trace(model, batch)
        with quiet():
            out = model(batch)
        for h in hooks:
            h.remove()
        loss = torch.nn.functional.mse_loss(out.view(-1), batch["y"])
        loss.backward()
        save_case(name, {"kind": "finetune", "ctor": cfg, "seed": seed, "loss": "mse"}, batch, model, {"logits": out}, loss, trace)


if __name__ == "__main__":
    main()
