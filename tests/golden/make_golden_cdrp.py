#!/usr/bin/env python3
"""Generates tests/golden/cdrp_b5.npz by running the REFERENCE's cancer-drug-response model (needs the reference checkout that
make_golden.py names; run where that exists):
    python tests/golden/make_golden_cdrp.py

Uses make_golden.py's stand-ins for the third-party packages, then takes
    fragnet.model.cdrp.model   CDRPModel (with its MLP)
    fragnet.dataset.data       collate_fn_cdrp
from the reference, and FragNetFineTuneBase from its train/finetune/finetune_cdrp.py.  That file is a script with script-local imports
and cannot be imported: it is parsed with ``ast`` at run time and ONLY the class node is compiled and executed, in a namespace that
holds the reference's gat2 names.  Nothing but numbers the reference computed and a JSON of constructor arguments goes into the fixture.

The case: 5 synthetic ESOL-profile molecules, num_layer 2, num_heads 4, drop_ratio 0, gene_dim 903 (903 % 4 = 3); gene_expr ~ N(0, 2.5)
per molecule with -0.7, 2.9 and -1.5 placed by hand in the first record, so that the int64 batch shows truncation toward zero
(-0, 2, -1); model.train(), MSE against y.  Layout as make_golden.py's cases; out/drug_enc and out/cell_enc come from forward hooks.
"""
import ast
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

NAME = "cdrp_b5"
GENE_DIM = 903
MOL_SEED, GENE_SEED, SEED = 5000, 5001, 7
PINNED = (-0.7, 2.9, -1.5)
CTOR = dict(n_classes=1, atom_features=167, frag_features=167, edge_features=17, num_layer=2, num_heads=4, drop_ratio=0.0,
            h1=32, h2=64, h3=64, h4=32, act="relu", emb_dim=128, fthead="FTHead3")


def reference_base_class(ref_gat2):
    """FragNetFineTuneBase of the reference's finetune_cdrp.py: the class node alone, compiled in a namespace of gat2's names"""
    path = os.path.join(mg.REF, "fragnet", "train", "finetune", "finetune_cdrp.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "FragNetFineTuneBase")
    from torch_scatter import scatter_add
    ns = {"nn": torch.nn, "torch": torch, "scatter_add": scatter_add, "FragNet": ref_gat2.FragNet}
    for k in ("FTHead1", "FTHead2", "FTHead3", "FTHead4"):
        ns[k] = getattr(ref_gat2, k)
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns["FragNetFineTuneBase"]


def main():
    mg.install_stubs()
    with mg.quiet():
        from fragnet.model.gat import gat2 as ref_gat2
        from fragnet.model.cdrp.model import CDRPModel
        from fragnet.dataset import data as ref_data
    from fragnet_amd import synth
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    Base = reference_base_class(ref_gat2)

    mols = synth.attach_gene_expr(synth.synth_molecules(5, seed=MOL_SEED, profile="esol"), GENE_DIM, GENE_SEED, PINNED)
    batch = ref_data.collate_fn_cdrp(mols)
    assert batch["gene_expr"].dtype == torch.int64 and batch["gene_expr"][0, :3].tolist() == [0, 2, -1]
    torch.manual_seed(SEED)
    with mg.quiet():
        model = CDRPModel(Base(**CTOR), GENE_DIM, "cpu")
    mg.zero_dead_bias(model.drug_model)
    model.train()
    kept = {}
    hooks = [model.drug_model.register_forward_hook(lambda m, i, o: kept.__setitem__("drug_enc", o.detach().clone())),
             model.cell_model.register_forward_hook(lambda m, i, o: kept.__setitem__("cell_enc", o.detach().clone()))]
    with mg.quiet():
        out = model(batch)
    for h in hooks:
        h.remove()
    loss = torch.nn.functional.mse_loss(out.view(-1), batch["y"])
    loss.backward()
    cfg = {"kind": "cdrp", "ctor": CTOR, "gene_dim": GENE_DIM, "seed": SEED, "loss": "mse", "mol_seed": MOL_SEED, "gene_seed": GENE_SEED,
           "pinned": list(PINNED)}
    mg.save_case(NAME, cfg, batch, model, {"logits": out, **kept}, loss, [])
    size = os.path.getsize(os.path.join(HERE, NAME + ".npz"))
    print(f"{NAME}.npz: {size} bytes")
    assert size < (1 << 20)


if __name__ == "__main__":
    main()
