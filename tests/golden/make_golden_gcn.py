#!/usr/bin/env python3
"""Generates the model_version gcn2 fixtures by running the REFERENCE's own fragnet/model/gcn/gcn2.py in the build container
(same rules as make_golden.py: run where the reference is, only numbers it computed go into the fixtures):

    python tests/golden/make_golden_gcn.py

    ft_gcn2_b6.npz        6 ESOL-shape molecules, num_layer = 3, FTHead3 / relu, MSE
    ft_gcn2_edge_b6.npz   edge_case_molecules() (two atoms without a bond among them), num_layer = 2, FTHead4 / silu, MSE

Besides make_golden.py's stand-ins the module needs ``torch_geometric.utils.degree`` (its documented semantics: a count per index),
and fragnet/model/gat on sys.path, because gcn2.py:9 imports ``gat2`` by its bare name.  Both fixtures carry the per-layer raw outputs
(x_atoms, x_frags of every layer, through forward hooks): the logits of this model differ between molecules only in the third decimal,
so the layer traces and the gradients carry the parity test.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, edge_case_molecules, install_stubs, quiet, save_case  # noqa: E402


def _stub_degree(index, num_nodes=None, dtype=None):
    n = int(num_nodes) if num_nodes is not None else int(index.max()) + 1
    return torch.zeros(n, dtype=dtype or torch.float32).scatter_add_(0, index, torch.ones(index.numel(), dtype=dtype or torch.float32))


def main():
    install_stubs()
    sys.modules["torch_geometric.utils"].degree = _stub_degree
    sys.path.insert(0, os.path.join(REF, "fragnet", "model", "gat"))
    with quiet():
        from fragnet.model.gcn import gcn2 as ref_gcn
        from fragnet.dataset import data as ref_data
    from fragnet_amd import synth
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)

    def case(name, mols, cfg, seed):
        batch = ref_data.collate_fn(mols)
        torch.manual_seed(seed)
        with quiet():
            model = ref_gcn.FragNetFineTune(**cfg)
        model.train()
        trace = []
        hooks = [l.register_forward_hook(lambda m, i, o: trace.append([t.detach().numpy().copy() for t in o[:2]]))
                 for l in model.pretrain.layers]
        with quiet():
            out = model(batch)
        for h in hooks:
            h.remove()
        loss = torch.nn.functional.mse_loss(out.view(-1), batch["y"])
        loss.backward()
        save_case(name, {"kind": "finetune_gcn2", "ctor": cfg, "seed": seed, "loss": "mse"}, batch, model, {"logits": out}, loss, trace)

    cfg = dict(n_classes=1, atom_features=167, frag_features=167, edge_features=17, num_layer=3, drop_ratio=0.0,
               h1=64, h2=128, h3=128, h4=64, act="relu", emb_dim=128, fthead="FTHead3")
    case("ft_gcn2_b6", synth.synth_molecules(6, seed=4300, profile="esol"), cfg, 7)
    cfg_edge = dict(n_classes=1, atom_features=167, frag_features=167, edge_features=17, num_layer=2, drop_ratio=0.0,
                    h1=64, act="silu", emb_dim=128, fthead="FTHead4")
    case("ft_gcn2_edge_b6", edge_case_molecules(), cfg_edge, 5)


if __name__ == "__main__":
    main()
