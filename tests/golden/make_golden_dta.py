#!/usr/bin/env python3
"""Generates tests/golden/dta_b5.npz by running the REFERENCE's drug-target-affinity model (needs the reference checkout that
make_golden.py names; run where that exists):
    python tests/golden/make_golden_dta.py

Uses make_golden.py's stand-ins for the third-party packages, then takes
    fragnet.model.dta.model    DTAModel2 (the model the reference's driver builds)
    fragnet.dataset.data       collate_fn_dta
from the reference, and FragNetFineTuneBase from its train/finetune/finetune_dta.py.  That file is a script with script-local imports
and cannot be imported: it is parsed with ``ast`` at run time and ONLY the class node is compiled and executed, in a namespace that
holds the reference's gat2 names.  Nothing but numbers the reference computed and a JSON of constructor arguments goes into the fixture.

The reference's model module calls torch.manual_seed(1) when it is imported, so the seed of the case is set AFTER that import.

The case: 5 synthetic ESOL-profile molecules, num_layer 2, num_heads 4, drop_ratio 0; proteins of 1000 tokens (synth.attach_protein):
record 0 full length, record 1 of length 1 (pinned), three of random lengths, zeros behind each; all 25 residue tokens occur.
model.train(), MSE against y.  Layout as make_golden.py's cases; out/drug_enc and out/prot_enc (fc1_xt's output) come from forward
hooks.  Gradients go through save_case, which samples the large ones (fc1_xt.weight has 2.8 M entries).
"""
import ast
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

NAME = "dta_b5"
MOL_SEED, PROT_SEED, SEED = 6000, 6001, 7
PINNED = {1: [7]}
CTOR = dict(n_classes=1, atom_features=167, frag_features=167, edge_features=17, num_layer=2, num_heads=4, drop_ratio=0.0,
            h1=32, h2=64, h3=64, h4=32, act="relu", emb_dim=128, fthead="FTHead3")


def reference_base_class(ref_gat2):
    """FragNetFineTuneBase of the reference's finetune_dta.py: the class node alone, compiled in a namespace of gat2's names"""
    path = os.path.join(mg.REF, "fragnet", "train", "finetune", "finetune_dta.py")
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
        from fragnet.model.dta.model import DTAModel2           # reseeds torch and numpy at import
        from fragnet.dataset import data as ref_data
    from fragnet_amd import synth
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    Base = reference_base_class(ref_gat2)

    mols = synth.attach_protein(synth.synth_molecules(5, seed=MOL_SEED, profile="esol"), PROT_SEED, length=1000, pinned=PINNED)
    batch = ref_data.collate_fn_dta(mols)
    prot = batch["protein"]
    assert prot.dtype == torch.int64 and prot.shape == (5, 1000)
    lengths = (prot != 0).sum(1).tolist()
    assert lengths[0] == 1000 and lengths[1] == 1 and all(1 < n < 1000 for n in lengths[2:]), lengths
    assert sorted(set(prot.reshape(-1).tolist())) == list(range(26))
    torch.manual_seed(SEED)
    with mg.quiet():
        model = DTAModel2(Base(**CTOR))
    mg.zero_dead_bias(model.drug_model)
    model.train()
    kept = {}
    hooks = [model.drug_model.register_forward_hook(lambda m, i, o: kept.__setitem__("drug_enc", o.detach().clone())),
             model.fc1_xt.register_forward_hook(lambda m, i, o: kept.__setitem__("prot_enc", o.detach().clone()))]
    with mg.quiet():
        out = model(batch)
    for h in hooks:
        h.remove()
    loss = torch.nn.functional.mse_loss(out.view(-1), batch["y"])
    loss.backward()
    cfg = {"kind": "dta", "ctor": CTOR, "seed": SEED, "loss": "mse", "mol_seed": MOL_SEED, "prot_seed": PROT_SEED,
           "pinned": {str(k): v for k, v in PINNED.items()}, "lengths": lengths}
    mg.save_case(NAME, cfg, batch, model, {"logits": out, **kept}, loss, [])
    size = os.path.getsize(os.path.join(HERE, NAME + ".npz"))
    print(f"{NAME}.npz: {size} bytes")
    assert size < (1 << 20)


if __name__ == "__main__":
    main()
